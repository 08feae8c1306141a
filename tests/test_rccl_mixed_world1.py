"""RCCL code paths of the batch-sharded mixed Sinkhorn divergence on the one-GPU box (-m gpu): world size 1 over the
``nccl`` backend, in a CHILD process (tools/nccl_mixed_selftest.py): the eager dist.sharded_mixed_sinkhorn_loss step, whose
all_gather_into_tensor calls write the halves of the stacked videos, and GraphedShardedMixedStep in both regimes, against
the single-GPU compute_mixed_sinkhorn_loss.  The multi-rank logic is covered over gloo (tests/test_dist_mixed.py)."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_rccl_sharded_mixed_steps_at_world_size_1():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("KCCOT_DIST_ROW_BLOCKS", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nccl_mixed_selftest.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "nccl mixed selftest ok: backend=nccl" in p.stdout, p.stdout[-2000:]
