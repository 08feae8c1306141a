"""GPU: KCCOTTrainer(mixed_sinkhorn=True) -- the two-minibatch training step on a small configuration (native
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
                        device="cuda:0", mixed_sinkhorn=True, **kw)


def test_mixed_steps_update_their_own_networks():
    from kccotgan_amd import gan_utils
    tr = _trainer()
    x, xp = torch.rand(B, H, T, W, C, device="cuda:0"), torch.rand(B, H, T, W, C, device="cuda:0")
    snap = lambda ps: [p.detach().clone() for p in ps]
    changed = lambda a, b: any(not torch.equal(p, q) for p, q in zip(a, b))
    g0, d0 = snap(tr.g_params), snap(tr.d_params)
    pm = tr.disc_training_step(x[:, :, :iT], x[:, :, iT:], 5.0, xp[:, :, :iT], xp[:, :, iT:])
    assert torch.isfinite(pm) and changed(d0, snap(tr.d_params)) and not changed(g0, snap(tr.g_params))
    assert "compute_mixed_sinkhorn_loss" in gan_utils.last_info
    d1 = snap(tr.d_params)
    loss = tr.gen_training_step(x[:, :, :iT], x[:, :, iT:], 5.0, xp[:, :, :iT], xp[:, :, iT:])
    assert torch.isfinite(loss) and changed(g0, snap(tr.g_params)) and not changed(d1, snap(tr.d_params))
    pm, loss = tr.train_iteration(x, 5.0, xp)
    assert torch.isfinite(pm) and torch.isfinite(loss)
    with pytest.raises(ValueError):
        tr.train_iteration(x, 5.0)


def test_mixed_fit_consumes_two_batches_per_iteration():
    tr = _trainer()
    batches = [torch.rand(B, H, T, W, C) for _ in range(5)]
    out = tr.fit(iter(batches), log=None)
    assert out["iterations"] == 2 and not out["exploded"]          # 5 batches -> 2 pairs, the odd one dropped
    assert all(map(lambda v: v == v, out["history"]["Sinkhorn Loss"]))


def test_mixed_with_a_process_group_is_refused():
    with pytest.raises(NotImplementedError):
        _trainer(group=object())
