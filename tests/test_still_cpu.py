"""Still clips without a GPU: the argument checks of the two ``vds_`` entry points (their declarations and binding:
tests/test_cabi.py), one ``distill.StillGMTrainer`` step on the oracle ops against plain autograd through ``img.unsqueeze(1).expand``,
and ``GMTrainer``'s two hooks, whose default bodies are the expressions they replaced."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.cpu_backend import OracleBackend, OracleGMOps
from video_distillation_amd import distill, hip, plan

C, SPC, T, HW = 2, 1, 8, 64
LR = 0.1


# ---- ABI --------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_back_as_codes_before_any_device_call():
    """-1 for a non-positive T / H / W or a negative n, 0 for n == 0, -1 for a null pointer with work to do -- with no GPU in
    the machine.  The addresses are never dereferenced on these paths."""
    lib = hip.lib()
    A = [0x10000 + 0x1000 * k for k in range(4)]
    names_e = ("images", "index", "n", "T", "H", "W", "out")
    base_e = dict(images=A[0], index=A[1], n=3, T=8, H=5, W=7, out=A[2])
    expand = lambda **k: lib.vds_still_expand(*[k.get(n, base_e[n]) for n in names_e], None)          # noqa: E731
    names_r = ("g_clips", "n", "T", "H", "W", "g_images")
    base_r = dict(g_clips=A[0], n=3, T=8, H=5, W=7, g_images=A[2])
    reduce_ = lambda **k: lib.vds_still_reduce(*[k.get(n, base_r[n]) for n in names_r], None)          # noqa: E731
    for call in (expand, reduce_):
        for dim in ("T", "H", "W"):
            assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1, dim
            assert call(n=0, **{dim: 0}) == -1, dim          # (the shape is checked before the empty batch is let through)
        assert call(n=-1) == -1
        assert call(n=0) == 0
    assert expand(n=0, images=None, out=None, index=None) == 0 and reduce_(n=0, g_clips=None, g_images=None) == 0
    assert expand(images=None) == -1 and expand(out=None) == -1
    assert reduce_(g_clips=None) == -1 and reduce_(g_images=None) == -1
    with pytest.raises(RuntimeError, match=r"^vds_still_reduce failed with code -1$"):
        hip.run("vds_still_reduce", A[0], 3, 0, 5, 7, A[2], None)


def test_python_wrappers_refuse_before_the_kernel():
    x = torch.zeros(2, 3, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.still_expand(x, None, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.still_reduce(torch.zeros(2, 4, 3, 5, 7))
    with pytest.raises(ValueError):
        hip.still_expand(torch.zeros(2, 1, 5, 7), None, 4)
    with pytest.raises(ValueError):
        hip.still_reduce(torch.zeros(2, 3, 5, 7))


# ---- the torch expressions the CPU oracle ops take -------------------------------------------------------------------------

def test_torch_expressions_of_expand_and_reduce():
    ops = OracleGMOps("ours")
    assert not hasattr(ops, "still_expand") and not hasattr(ops, "still_reduce")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 5, 7, generator=g)
    idx = torch.tensor([2, 0, 2])
    out = distill.still_expand(ops, x, idx, 6)
    assert out.shape == (3, 6, 3, 5, 7) and out.is_contiguous()
    assert torch.equal(out, x[idx].unsqueeze(1).expand(-1, 6, -1, -1, -1))
    assert torch.equal(distill.still_expand(ops, x, None, 2), torch.stack([x, x], 1))
    gc = torch.randn(3, 6, 3, 5, 7, generator=g)
    want = gc.numpy()[:, 0].copy()
    for t in range(1, 6):
        want = (want + gc.numpy()[:, t]).astype(np.float32)
    assert np.array_equal(distill.still_reduce(ops, gc).numpy(), want)


# ---- one StillGMTrainer step against plain autograd ------------------------------------------------------------------------

def still_case():
    """The inputs of the trainer tests here and in tests/test_gpu_still.py: 3 stills per class, the first of each as memory."""
    g = torch.Generator().manual_seed(4242)
    stills = torch.randn(C * 3, 3, HW, HW, generator=g)
    static0 = torch.stack([stills[0], stills[3]]).clone()
    init = lambda it: R.init_params(500 + it, 3, C)          # noqa: E731
    return stills, static0, init


def still_trainer(ops, dev, stills, static0, init, **kw):
    pool = distill.RealPool(stills.to(dev), [3] * C, [0, 3])
    kw.setdefault("outer_loop", 1)
    return distill.StillGMTrainer(ops, pool, plan.NetGeometry(T, HW, HW), C, SPC, batch_real=2, lr_img=LR, lr_net=0.01,
                                  static=static0.clone().to(dev), inner_loop=1, dropout_p=0.0, net_init=init, **kw)


def autograd_step(stills, static0, init, dtype=torch.float32, frame_noise=None):
    """The same iteration in plain autograd on the oracle net -> (loss, d loss / d img (C,3,H,W), per-frame gradient
    (C,T,3,H,W)): the clip is ``img.unsqueeze(1).expand``, the gradient is taken with respect to ``img``."""
    params = [p.to(dtype).requires_grad_(True) for p in init(0)]
    idx = distill.sample_real_indices(0, [3] * C, [0, 3], 2, list(range(C))).reshape(C, -1)
    total, g_img, g_frames = torch.zeros((), dtype=dtype), [], []          # (summed as the trainer sums: in the tensors' format)
    for c in range(C):
        real = stills[torch.as_tensor(idx[c])].to(dtype).unsqueeze(1).expand(-1, T, -1, -1, -1)
        if frame_noise is not None:
            real = real + frame_noise[torch.as_tensor(idx[c])].to(dtype)
        lab_r = torch.full((real.shape[0],), c, dtype=torch.int64)
        gw_real = [t.detach() for t in torch.autograd.grad(torch.nn.functional.cross_entropy(R.convnet3d_logits(real, params), lab_r), params)]
        img = static0[c * SPC:(c + 1) * SPC].to(dtype).clone().requires_grad_(True)
        clip = img.unsqueeze(1).expand(-1, T, -1, -1, -1)
        if frame_noise is not None:
            clip = clip + frame_noise[[3 * c]].to(dtype)          # (the memory of class c starts as still 3c)
        clip.retain_grad()
        lab_s = torch.full((SPC,), c, dtype=torch.int64)
        gw_syn = torch.autograd.grad(torch.nn.functional.cross_entropy(R.convnet3d_logits(clip, params), lab_s), params, create_graph=True)
        loss = R.match_loss(gw_syn, gw_real, "ours")
        loss.backward()
        total = total + loss.detach()
        g_img.append(img.grad.detach())
        g_frames.append(clip.grad.detach())
    return float(total), torch.cat(g_img), torch.cat(g_frames)


@pytest.fixture(scope="module")
def cpu_step():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    stills, static0, init = still_case()
    tr = still_trainer(OracleGMOps("ours"), "cpu", stills, static0, init)
    loss = float(tr.step(0))
    return dict(stills=stills, static0=static0, init=init, tr=tr, loss=loss, ref=autograd_step(stills, static0, init))


def test_still_step_equals_autograd_through_expand(cpu_step):
    """The loss is the same number.  The image gradient is a T-term fp32 sum taken in ascending t by the trainer and in
    autograd's own order by ``expand``'s backward: two orders of one sum differ by at most (T-1) * 2^-24 * sum_t |g_t|, so
    the two updated images -- static0 - lr * g, the final rounding of which is the trainer's own and checked bitwise
    below -- differ by at most lr times that, elementwise."""
    tr, (loss_ref, g_ref, g_frames) = cpu_step["tr"], cpu_step["ref"]
    static0 = cpu_step["static0"]
    assert cpu_step["loss"] == loss_ref
    assert tr.steps_done == 1 and tr.static.shape == (C * SPC, 3, HW, HW) and tr.buf.shape == tr.static.shape
    g_tr = tr.buf          # first step: the momentum buffer is the gradient
    assert float(g_ref.abs().max()) > 0
    bound = LR * (T - 1) * 2.0 ** -24 * g_frames.double().abs().sum(1)
    d = (static0.double() - LR * g_tr.double()) - (static0.double() - LR * g_ref.double())
    print("still step: loss %.9g; max |d| %.3e, max bound %.3e, elements with d != 0: %d of %d"
          % (loss_ref, float(d.abs().max()), float(bound.max()), int((d != 0).sum()), d.numel()))
    assert bool((d.abs() <= bound).all())
    assert torch.equal(tr.static, static0 - LR * g_tr)          # the optimiser's own arithmetic on that gradient
    assert torch.equal(tr.image_syn, tr.static.unsqueeze(1).expand(-1, T, -1, -1, -1))          # the next iteration's clips
    assert torch.equal(tr.gather_syn(), tr.image_syn) and tr.gather_static() is tr.static


def test_fp32_oracle_is_well_inside_the_gpu_bars_against_fp64(cpu_step):
    """tests/test_gpu_still.py compares HIP with this fp32 oracle under the bars of test_gm_trainer_hip_matches_oracle_trainer
    (loss 1e-3 relative, image update 5e-2 rel-l2 per class).  The seed is not a chaotic one if the fp32 oracle itself stays
    at least ten times inside both bars against the same computation in float64."""
    loss64, g64, _ = autograd_step(cpu_step["stills"], cpu_step["static0"], cpu_step["init"], dtype=torch.float64)
    g32 = cpu_step["tr"].buf.double()
    rel_loss = abs(cpu_step["loss"] - loss64) / abs(loss64)
    per = [float((g32[k] - g64[k]).norm() / g64[k].norm()) for k in range(C)]
    print("fp32 oracle vs float64: loss rel %.3e, image update rel-l2 per class %s" % (rel_loss, ["%.3e" % e for e in per]))
    assert rel_loss < 1e-4 and max(per) < 5e-3


def test_frame_noise_moves_the_gradient_far_less_than_the_bar(cpu_step):
    """The tie test of tests/test_gpu_still.py runs the step on clips whose frames carry per-frame noise (no exact ties).  The
    perturbation's own effect on the image gradient, measured here on the oracle, has to stay below a tenth of the 5e-2 bar
    for that comparison to say anything about ties.  Measured, rel-l2 per class: amplitude 1e-3 1.8e-2 / 2.9e-2 (too much:
    the 'ours' metric is touchy in the pixels), 3e-4 5.1e-3 / 5.9e-3, 1e-4 3.8e-3 / 1.5e-3, 3e-5 8.9e-4 / 1.7e-4 -- so the
    amplitude is 1e-4, NOISE below, and the bar stays where it is."""
    noise = still_noise()
    _, g_noisy, _ = autograd_step(cpu_step["stills"], cpu_step["static0"], cpu_step["init"], frame_noise=noise)
    _, g_ref, _ = cpu_step["ref"]
    per = [float((g_noisy[k].double() - g_ref[k].double()).norm() / g_ref[k].double().norm()) for k in range(C)]
    print("%g frame noise on real and synthetic clips, oracle: image gradient rel-l2 per class %s" % (NOISE, ["%.3e" % e for e in per]))
    assert max(per) < 5e-3


NOISE = 1e-4


def still_noise(amplitude: float = NOISE):
    """Per-frame noise for every still of ``still_case`` (the memory of class c, which starts as still 3c, takes row 3c)."""
    g = torch.Generator().manual_seed(777)
    return amplitude * (2 * torch.rand(C * 3, T, 3, HW, HW, generator=g) - 1)


# ---- GMTrainer's hooks -----------------------------------------------------------------------------------------------------

def test_gm_trainer_hooks_default_to_the_expressions_they_replaced():
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(4, 2, 3, 8, 8, generator=g)
    pool = distill.RealPool(clips, [2, 2], [0, 2])
    tr = distill.GMTrainer(OracleGMOps("ours"), pool, plan.NetGeometry(2, 8, 8), 2, 1, batch_real=2, lr_img=0.5)
    idx = torch.tensor([3, 0])
    assert torch.equal(tr._real_batch(idx), clips[idx])
    g_img = torch.randn(tr.image_syn.shape, generator=g)
    x, buf = tr.image_syn.clone(), tr.buf.clone()
    for first in (True, False):
        tr.steps_done = 0 if first else 3
        tr._apply_pixel_grad(g_img)
        OracleBackend.sgd(None, x, buf, g_img, 0.5, 0.5, first)
        assert torch.equal(tr.image_syn, x) and torch.equal(tr.buf, buf)
    assert distill.StillGMTrainer._real_batch is not distill.GMTrainer._real_batch
    assert distill.StillGMTrainer._apply_pixel_grad is not distill.GMTrainer._apply_pixel_grad


def test_still_trainer_refuses_a_clip_pool_and_a_class_outside_the_pool():
    geo = plan.NetGeometry(T, HW, HW)
    with pytest.raises(ValueError, match="pool of stills"):
        distill.StillGMTrainer(OracleGMOps("ours"), distill.RealPool(torch.zeros(2, T, 3, HW, HW), [1, 1], [0, 1]), geo, 2, 1, 1, 0.1)
    with pytest.raises(ValueError, match="rows 1..3 of a pool of 2"):
        distill.StillGMTrainer(OracleGMOps("ours"), distill.RealPool(torch.zeros(2, 3, HW, HW), [1, 2], [0, 1]), geo, 2, 1, 1, 0.1)
    tr = distill.StillGMTrainer(OracleGMOps("ours"), distill.RealPool(torch.arange(4.).view(4, 1, 1, 1).expand(4, 3, HW, HW).contiguous(),
                                                                     [2, 2], [0, 2]), geo, 2, 2, 1, 0.1)
    assert tr.static[:, 0, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0] and tr.ipc == tr.spc == 2          # --init real: the first spc stills


def test_gather_static_through_the_collective_path(tmp_path, monkeypatch):
    """One rank with the collectives forced on (a 1-rank all_gather is the identity): ``gather_static`` pads, gathers and cuts
    the images as ``gather_syn`` does the clips, rows in class order."""
    import torch.distributed as dist
    stills = torch.arange(6.).view(6, 1, 1, 1).expand(6, 3, HW, HW).contiguous()
    tr = distill.StillGMTrainer(OracleGMOps("ours"), distill.RealPool(stills, [3, 3], [0, 3]), plan.NetGeometry(T, HW, HW), 2, 2, 1, 0.1)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        monkeypatch.setenv("VD_FORCE_COLLECTIVES", "1")
        got, clips = tr.gather_static(), tr.gather_syn()
        assert got is not tr.static and torch.equal(got, tr.static) and got[:, 0, 0, 0].tolist() == [0.0, 1.0, 3.0, 4.0]
        assert clips.shape == (4, T, 3, HW, HW) and torch.equal(clips, tr.image_syn)
    finally:
        dist.destroy_process_group()


# ---- class sharding: two ranks reproduce one -------------------------------------------------------------------------------

def _still_run(rank, world):
    stills, static0, init = still_case()
    lo, hi = distill.class_range(C, rank, world)
    pool = distill.RealPool(stills, [3] * C, [0, 3])          # (every rank holds the whole toy pool; it reads its own classes)
    tr = distill.StillGMTrainer(OracleGMOps("ours"), pool, plan.NetGeometry(T, HW, HW), C, SPC, batch_real=2, lr_img=LR, lr_net=0.01,
                                rank=rank, world=world, static=static0[lo * SPC:hi * SPC].clone(), outer_loop=2, inner_loop=1,
                                dropout_p=0.0, net_init=init)
    loss = float(tr.global_loss(tr.step(0)))
    return loss, tr.gather_static(), tr.gather_syn()


def _worker_still(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        loss, static, clips = _still_run(rank, world)
        if rank == 0:
            q.put((loss, static.numpy(), clips.numpy()))
    finally:
        dist.destroy_process_group()


def test_still_trainer_class_sharding_identity_two_ranks_gloo():
    """Two ranks owning one class each, outer loop 2 (one all-gather of the expanded clips and a network update in between),
    reproduce the single-rank run: summed loss, gathered images in class order, gathered clips = the images repeated.  The bounds
    are those of test_gm_trainer_class_sharding_identity_two_ranks_gloo (the oracle's summation order depends on the thread
    count, which differs between the one-rank and the two-rank run), with its absolute term times T for the images: an image
    update is the sum of T frame updates, each of which that test bounds by 5e-5."""
    from tests.test_distributed_cpu import _spawn
    torch.set_num_threads(4)
    want_l, want_s, _ = _still_run(0, 1)
    got_l, got_s, got_c = _spawn(_worker_still, 2)
    np.testing.assert_allclose(got_l, want_l, rtol=1e-5)
    np.testing.assert_allclose(got_s, want_s.numpy(), rtol=1e-4, atol=T * 5e-5)
    assert got_s.shape == (C * SPC, 3, HW, HW) and got_c.shape == (C * SPC, T, 3, HW, HW)
    assert all(np.array_equal(got_c[:, t], got_s) for t in range(T))
    assert not np.allclose(want_s.numpy(), still_case()[1].numpy())
