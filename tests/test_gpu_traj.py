"""The ``vdt_`` kernels of csrc/traj.hip through the C ABI against tests/traj_oracle.py, the fused flat-parameter chain inside
``MTTTrainer`` against the torch expressions and against the reference's fixtures G10 / G13, and ``experts.ExpertStore`` on the
device.

Sizes: the scalar tail alone (1), one float4 (4), float4 + tail (5), around one workgroup (255, 256), two workgroups with a tail
(1028), odd (4099), P at 3 classes (3 641 603, odd, more than one pass of the grid), and 5 past what the capped grid covers in
ONE pass: BLOCK * MAX_BLOCKS * 4 = 256 * 2048 * 4 = 2 097 152 floats (csrc/traj.hip).

Tolerances: elementwise outputs are compared bit for bit (the header's promise).  The fp64 sums are compared with ``math.fsum``:
n additions of non-negative terms err by at most n * 2^-53 of the sum (4e-10 at n = 3.6 M; the block-ordered sum is far
better), so 1e-9 relative; the signed sum of d/d syn_lr by 1e-9 of the sum of its absolute terms.  Trainer against trainer: the
bounds tests/test_distributed_cpu.py uses for two computations of one iteration."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import traj_oracle as O

pytestmark = pytest.mark.gpu

BLOCK, MAX_BLOCKS = 256, 2048          # csrc/traj.hip
GRID_COVER = BLOCK * MAX_BLOCKS * 4
P3 = 3641603
SIZES = [1, 4, 5, 255, 256, 1028, 4099, P3, GRID_COVER + 5]
LR, SHARE = np.float32(0.0123), 0.75


def _inputs(n):
    g = np.random.default_rng(n)
    return [g.normal(0.0, 0.05, n).astype(np.float32) for _ in range(5)]          # theta, theta0, target, grad, hv


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _run(name, *args):
    from video_distillation_amd import hip
    rc = getattr(hip.lib(), name)(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", SIZES)
def test_chain_kernels_against_the_oracle(n):
    from video_distillation_amd import hip
    theta, theta0, target, grad, hv = _inputs(n)
    d_theta, d_theta0, d_target, d_grad, d_hv = (_dev(a) for a in (theta, theta0, target, grad, hv))
    lr = torch.tensor(float(LR), dtype=torch.float32, device="cuda")
    need = hip.lib().vdt_traj_scratch_doubles(n)
    assert need == 2 * min(MAX_BLOCKS, max(1, (n // 4 + BLOCK - 1) // BLOCK))
    scratch = torch.full((need + 2,), -7.0, dtype=torch.float64, device="cuda")          # two guard slots behind it
    # ---- step
    out = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
    assert _run("vdt_traj_step", d_theta.data_ptr(), d_grad.data_ptr(), lr.data_ptr(), n, out.data_ptr()) == 0
    assert np.array_equal(_bits(out[:n]), O.traj_step(theta, grad, LR).view(np.uint32))
    assert (out[n:] == -7.0).all()          # nothing behind the n-th element
    # ---- loss
    rec = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    tbar = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
    args = (d_theta.data_ptr(), d_theta0.data_ptr(), d_target.data_ptr(), n, scratch.data_ptr(), rec.data_ptr(), tbar.data_ptr())
    assert _run("vdt_traj_loss", *args) == 0
    dist, dist0 = O.traj_dists(theta, theta0, target)
    got = rec.cpu().numpy()
    print("n %d: dist rel err %.2e, dist0 rel err %.2e" % (n, abs(got[0] - dist) / dist, abs(got[1] - dist0) / dist0))
    assert abs(got[0] - dist) <= 1e-9 * dist and abs(got[1] - dist0) <= 1e-9 * dist0
    assert got[2] == got[0] / got[1] and got[3] == 0.0
    assert np.array_equal(_bits(tbar[:n]), O.traj_tbar(theta, target, got[1]).view(np.uint32))          # the kernel's own dist0
    assert (tbar[n:] == -7.0).all() and (scratch[need:] == -7.0).all()
    rec2 = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    tbar2 = torch.empty_like(tbar)
    assert _run("vdt_traj_loss", *args[:5], rec2.data_ptr(), tbar2.data_ptr()) == 0
    assert np.array_equal(_bits(rec), _bits(rec2)) and np.array_equal(_bits(tbar[:n]), _bits(tbar2[:n]))          # run to run
    # ---- adjoint, hv == NULL: tbar as it is
    tbar_np = tbar[:n].cpu().numpy()
    _, dot0, abs0, v0 = O.traj_adjoint(tbar_np, None, grad, LR, SHARE)
    g_lr = torch.zeros((2,), dtype=torch.float64, device="cuda")
    v = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
    before = tbar.clone()
    adj = lambda hvp, acc, vv: _run("vdt_traj_adjoint", tbar.data_ptr(), hvp, d_grad.data_ptr(), lr.data_ptr(),   # noqa: E731
                                    ctypes.c_float(SHARE), n, scratch.data_ptr(), acc.data_ptr(), vv.data_ptr())
    assert adj(None, g_lr, v) == 0
    assert np.array_equal(_bits(tbar), _bits(before))
    assert np.array_equal(_bits(v[:n]), v0.view(np.uint32)) and (v[n:] == -7.0).all()
    print("n %d: <tbar, g> err %.2e of sum|terms|" % (n, abs(-float(g_lr[0]) - dot0) / max(abs0, 1e-300)))
    assert abs(-float(g_lr[0]) - dot0) <= 1e-9 * abs0 and float(g_lr[1]) == 0.0
    # ---- adjoint with hv: tbar += hv in place, the sum over the UPDATED tbar, accumulated into the same g_lr
    t1, dot1, abs1, v1 = O.traj_adjoint(tbar_np, hv, grad, LR, SHARE)
    g_lr_b = torch.zeros((2,), dtype=torch.float64, device="cuda")
    v_b = torch.empty_like(v)
    assert adj(d_hv.data_ptr(), g_lr_b, v_b) == 0
    assert np.array_equal(_bits(tbar[:n]), t1.view(np.uint32)) and (tbar[n:] == -7.0).all()
    assert np.array_equal(_bits(v_b[:n]), v1.view(np.uint32))
    assert abs(-float(g_lr_b[0]) - dot1) <= 1e-9 * abs1
    # the same call on the same inputs (tbar restored): the same bits; and g_lr is decremented, not overwritten
    tbar.copy_(before)
    g_lr_c = torch.zeros((2,), dtype=torch.float64, device="cuda")
    assert adj(d_hv.data_ptr(), g_lr_c, v) == 0
    assert np.array_equal(_bits(g_lr_b), _bits(g_lr_c)) and np.array_equal(_bits(v[:n]), _bits(v_b[:n]))
    tbar.copy_(before)
    assert adj(d_hv.data_ptr(), g_lr_c, v) == 0
    assert float(g_lr_c[0]) == float(g_lr_b[0]) + float(g_lr_b[0])          # x - t - t with x = 0 is exact doubling
    assert (scratch[need:] == -7.0).all()


def test_a_misaligned_pointer_is_refused_and_nothing_is_written():
    n = 1028
    theta, theta0, target, grad, hv = (_dev(a) for a in _inputs(n))
    lr = torch.tensor(0.01, dtype=torch.float32, device="cuda")
    out = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
    rec = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    g_lr = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    scratch = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    assert _run("vdt_traj_step", theta.data_ptr() + 4, grad.data_ptr(), lr.data_ptr(), n - 4, out.data_ptr()) == -1
    assert _run("vdt_traj_step", theta.data_ptr(), grad.data_ptr(), lr.data_ptr(), n - 4, out.data_ptr() + 4) == -1
    assert _run("vdt_traj_loss", theta.data_ptr(), theta0.data_ptr() + 4, target.data_ptr(), n - 4, scratch.data_ptr(), rec.data_ptr(),
                out.data_ptr()) == -1
    assert _run("vdt_traj_adjoint", out.data_ptr(), hv.data_ptr() + 4, grad.data_ptr(), lr.data_ptr(), ctypes.c_float(1.0), n - 4,
                scratch.data_ptr(), g_lr.data_ptr(), theta.data_ptr()) == -1
    assert _run("vdt_traj_adjoint", out.data_ptr(), None, grad.data_ptr(), lr.data_ptr(), ctypes.c_float(1.0), 0,
                scratch.data_ptr(), g_lr.data_ptr(), theta.data_ptr()) == -2
    for t in (out, rec, g_lr, scratch):
        assert (t == -7.0).all()


# ---- the chain inside the trainer --------------------------------------------------------------------------------------------

def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def test_fused_chain_equals_the_torch_expressions_in_the_trainer():
    from oracle import ref_cpu as R
    from video_distillation_amd import distill, plan
    C, n_syn = 3, 6
    g = torch.Generator().manual_seed(31)
    start = R.init_params(9, 3, C)
    target = [p + 0.02 * p.abs().mean() * torch.randn(p.shape, generator=g) for p in start]
    image_syn = torch.randn(n_syn, 8, 3, 64, 64, generator=g)
    labels = torch.arange(C).repeat_interleave(2)
    chunks = [torch.tensor([0, 3, 4]), torch.tensor([5, 1, 2]), torch.tensor([2, 0, 5])]
    ops = distill.HipMTTOps(plan.NetGeometry(8, 64, 64), C, "cuda:0", dropout_p=0.0, fused_flat=True)
    chain = ops.flat
    got = {}
    for name, flat in (("off", None), ("on", chain)):
        ops.flat = flat
        tr = distill.MTTTrainer(ops, C, image_syn.clone().cuda(), labels.cuda(), 0.01, lr_img=100.0, lr_lr=1e-5, syn_steps=3,
                                batch_syn=3, expert_epochs=1, max_start_epoch=1)
        grand = tr.step(0, [start, target], start_epoch=0, index_chunks=chunks, update=False)
        torch.cuda.synchronize()
        g_img, g_lr = tr.last_grads
        assert grand.dim() == 0 and grand.dtype == torch.float32 and g_lr.dim() == 0 and g_lr.dtype == torch.float32
        got[name] = (float(grand), g_img.clone(), float(g_lr))
    assert chain.n == P3          # the fused leg ran on the vdt_ kernels
    (l0, x0, r0), (l1, x1, r1) = got["off"], got["on"]
    print("grand %.8f / %.8f, g_lr %.6e / %.6e, g_img rel-l2 %.2e" % (l0, l1, r0, r1, _rel(x1, x0)))
    assert abs(l1 - l0) / l0 < 1e-5
    assert abs(r1 - r0) / abs(r0) < 1e-3
    assert _rel(x1, x0) < 1e-3


def _fused_ops(monkeypatch):
    from video_distillation_amd import distill
    made = []

    class Fused(distill.HipMTTOps):
        def __init__(self, *a, **k):
            k["fused_flat"] = True
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(distill, "HipMTTOps", Fused)
    return made


def test_g10_with_the_fused_chain(monkeypatch, golden_dir):
    """tests/test_gpu_train.py's G10 test, its own assertions, with every HipMTTOps it makes created ``fused_flat=True``."""
    from tests import test_gpu_train as G
    made = _fused_ops(monkeypatch)
    G.test_g10_mtt_step_on_hip_vs_reference_golden(golden_dir)
    assert len(made) == 1 and made[0].flat is not None and made[0].flat.n > 0


def test_g13_with_the_fused_chain(monkeypatch):
    """``check_s2d_mtt_against_g13(tol=5e-3)`` as tests/test_gpu_train.py runs it, on the fused chain."""
    from tests import test_gpu_train as G
    made = _fused_ops(monkeypatch)
    G.test_g13_s2d_mtt_trainer_on_hip_vs_reference_golden()
    assert len(made) == 1 and made[0].flat is not None and made[0].flat.n == P3


# ---- the store on the device -------------------------------------------------------------------------------------------------

def test_store_rows_on_the_device_and_a_step_from_each_mode(tmp_path):
    from tests.test_traj_cpu import _random_walk
    from video_distillation_amd import checkpoint, distill, experts, plan
    C = 3
    gen = torch.Generator().manual_seed(6)
    walk = _random_walk(gen, 2, 3)
    checkpoint.save_expert_buffer(str(tmp_path), walk)
    image_syn = torch.randn(C, 8, 3, 64, 64, generator=gen)
    chunks = [torch.tensor([1, 2, 0]), torch.tensor([0, 2, 1])]
    ops = distill.HipMTTOps(plan.NetGeometry(8, 64, 64), C, "cuda:0", dropout_p=0.0, fused_flat=True)
    losses = {}
    for mode in ("host", "resident"):
        store = experts.ExpertStore(str(tmp_path), C, "cuda:0", mode=mode, walk="all", seed=3)
        traj = store.next()
        f, e = store.last
        assert f == 0 and traj.epochs == 3
        for epoch in (0, 2):
            row = traj.row(epoch)
            assert row.is_cuda and tuple(row.shape) == (P3,) and row.data_ptr() % 16 == 0
            assert torch.equal(row.cpu(), distill.flatten_params(walk[e][epoch]))
        tr = distill.MTTTrainer(ops, C, image_syn.clone().cuda(), torch.arange(C).cuda(), 0.01, lr_img=100.0, lr_lr=1e-5, syn_steps=2,
                                batch_syn=3, expert_epochs=1, max_start_epoch=2)
        losses[mode] = (e, float(tr.step(0, traj, start_epoch=1, index_chunks=chunks, update=False)))
        torch.cuda.synchronize()
        assert torch.equal(traj.row(1).cpu(), distill.flatten_params(walk[e][1]))          # the rows are as they were: out of place
    assert losses["host"][0] == losses["resident"][0]          # the same seed walks the same expert
    a, b = losses["host"][1], losses["resident"][1]
    print("grand loss host %.8f resident %.8f" % (a, b))
    assert np.isfinite(a) and abs(a - b) / abs(b) < 1e-5
