"""GPU: KCCOTTrainer(bi_causal=True) -- the bi-causal loss in the training step on a small configuration (native
convolutions, as tests/test_gpu_train_step.py runs its in-process tests)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2


@pytest.fixture(autouse=True)
def _native_convolutions(monkeypatch):
    from kccotgan_amd import gan
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})


def _trainer(**kw):
    from kccotgan_amd.kernel_train import KCCOTTrainer
    return KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="1d", warmup=10,
                        device="cuda:0", bi_causal=True, **kw)


def test_bicausal_trainer_runs_iterations_with_a_finite_loss():
    from kccotgan_amd import gan_utils
    tr = _trainer()
    batches = [torch.rand(B, H, T, W, C) for _ in range(3)]
    gan_utils.last_info.clear()
    out = tr.fit(iter(batches), log=None)
    assert out["iterations"] == 3 and not out["exploded"]
    assert all(map(lambda v: v == v and abs(v) != float("inf"), out["history"]["Sinkhorn Loss"]))
    assert "compute_bicausal_sinkhorn_loss_costs" in gan_utils.last_info
    assert "compute_sinkhorn_loss_costs" not in gan_utils.last_info


def test_bicausal_trainer_loss_is_the_bicausal_loss_of_its_tensors(monkeypatch):
    """The discriminator step's loss equals compute_bicausal_sinkhorn_loss on the very tensors the step built."""
    from kccotgan_amd import gan_utils
    seen = []
    orig = gan_utils.compute_bicausal_sinkhorn_loss

    def spy(*a, **k):
        loss = orig(*a, **k)
        seen.append(([x.detach().clone() if torch.is_tensor(x) else x for x in a], dict(k), loss.detach().clone()))
        return loss
    monkeypatch.setattr(gan_utils, "compute_bicausal_sinkhorn_loss", spy)
    tr = _trainer()
    x = torch.rand(B, H, T, W, C, device="cuda:0")
    tr.disc_training_step(x[:, :, :iT], x[:, :, iT:], 5.0)
    assert len(seen) == 1
    args, kw, loss = seen[0]
    again = orig(*args, **kw)
    assert torch.isfinite(loss) and float(again) == float(loss)
    one = gan_utils.compute_sinkhorn_loss(*args, **kw)
    assert float(one) != float(loss)                     # the trainer did not run the one-batch loss
