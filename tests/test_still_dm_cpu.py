"""Distribution matching on still clips without a GPU: the argument checks of ``vdsr_still_rows`` (its declaration and binding:
tests/test_cabi.py), three ``distill.StillDMTrainer`` steps on ``tests.cpu_backend.OracleBackend`` against a
hand-written loop that differentiates the oracle's DM loss through ``img.unsqueeze(1).expand`` by autograd, ``DMTrainer``'s two
hooks, class and batch sharding over two gloo ranks, and ``run_dm --memories static`` on the oracle backend."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.cpu_backend import OracleBackend
from video_distillation_amd import checkpoint, distill, hip, plan, run_dm

C, SPC, T, HW, PER, BATCH = 2, 2, 8, 64, 12, 8
LR, MU, STEPS = 0.1, 0.5, 3
SEED = 4343


# ---- ABI --------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_back_as_codes_before_any_device_call():
    """-1 for a non-positive T / H / W, a negative n or a prec outside 0..3; then 0 for n == 0; then -1 for a null ``images`` /
    ``out_hi`` -- with no GPU in the machine.  The addresses are never dereferenced on these paths."""
    lib = hip.lib()
    A = [0x10000 + 0x1000 * k for k in range(4)]
    names = ("images", "index", "n", "T", "H", "W", "out_hi", "out_lo", "prec")
    base = dict(images=A[0], index=A[1], n=3, T=8, H=5, W=7, out_hi=A[2], out_lo=A[3], prec=1)
    call = lambda **k: lib.vdsr_still_rows(*[k.get(n, base[n]) for n in names], None)          # noqa: E731
    for dim in ("T", "H", "W"):
        assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1, dim
        assert call(n=0, **{dim: 0}) == -1, dim          # (the shape is checked before the empty batch is let through)
    assert call(n=-1) == -1
    for prec in (-1, 4, 5, 100):
        assert call(prec=prec) == -1 and call(prec=prec, n=0) == -1, prec
    for prec in (0, 1, 2, 3):
        assert call(prec=prec, n=0) == 0, prec
    assert call(n=0, images=None, out_hi=None, out_lo=None, index=None) == 0
    assert call(images=None) == -1 and call(out_hi=None) == -1
    with pytest.raises(RuntimeError, match=r"^vdsr_still_rows failed with code -1$"):
        hip.run("vdsr_still_rows", A[0], None, 3, 0, 5, 7, A[2], None, 1, None)


def test_python_wrapper_refuses_before_the_kernel():
    x = torch.zeros(3, 3, 5, 7)
    for bad in ([0, 3], [-1], np.array([1, 5]), torch.tensor([3])):
        with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
            hip.still_rows(x, bad, 4, hip.PREC["f16"], 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.still_rows(x, [0, 2], 4, hip.PREC["f16"], 1)
    with pytest.raises(ValueError):
        hip.still_rows(torch.zeros(3, 1, 5, 7), None, 4, hip.PREC["f16"], 1)
    with pytest.raises(ValueError):
        hip.still_rows(x, None, 4, hip.PREC["f16c8"], 1)
    with pytest.raises(ValueError):
        hip.still_rows(x, None, 0, hip.PREC["f16"], 1)


# ---- three StillDMTrainer steps against plain autograd ---------------------------------------------------------------------

class RecordingBackend(OracleBackend):
    """The oracle backend, keeping every gradient its ``sgd`` was handed."""

    def __init__(self):
        super().__init__()
        self.grads = []

    def sgd(self, x, buf, g, lr, mu, first):
        self.grads.append(g.clone())
        OracleBackend.sgd(self, x, buf, g, lr, mu, first)


def still_dm_case():
    """The inputs of the trainer tests here and in tests/test_gpu_still_dm.py: 12 stills per class, the first two of each as
    memories; the network of iteration ``it`` is the oracle's of seed ``it`` (``OracleBackend.new_network``)."""
    g = torch.Generator().manual_seed(SEED)
    stills = torch.randn(C * PER, 3, HW, HW, generator=g)
    static0 = torch.cat([stills[c * PER:c * PER + SPC] for c in range(C)]).clone()
    return stills, static0


def still_dm_trainer(be, dev, stills, static0=None, **kw):
    pool = distill.RealPool(stills.to(dev), [PER] * C, [c * PER for c in range(C)])
    return distill.StillDMTrainer(be, pool, plan.NetGeometry(T, HW, HW), C, SPC, BATCH, LR, momentum=MU,
                                  static=None if static0 is None else static0.clone().to(dev), **kw)


def autograd_dm_step(it, stills, static, dtype=torch.float32):
    """Iteration ``it`` of the DM loss in plain autograd on the oracle net, the clips ``img.unsqueeze(1).expand`` of the images
    ``static`` -> (loss, d loss / d img (C*SPC,3,H,W), per-frame gradient (C*SPC,T,3,H,W)).  The real batch is embedded in one
    call and the loss written as ``OracleBackend.dm_loss`` writes it, so that the forward is the trainer's, number for number."""
    params = [p.to(dtype) for p in R.init_params(it)[:6]] + [None, None]
    idx = distill.sample_real_indices(it, [PER] * C, [c * PER for c in range(C)], BATCH, list(range(C)))
    with torch.no_grad():
        f_real = R.convnet3d_embed(stills[torch.as_tensor(idx)].to(dtype).unsqueeze(1).expand(-1, T, -1, -1, -1).contiguous(), params)
    img = static.to(dtype).clone().requires_grad_(True)
    clip = img.unsqueeze(1).expand(-1, T, -1, -1, -1)
    clip.retain_grad()
    f_syn = R.convnet3d_embed(clip, params)
    d = f_real.shape[1]
    loss = (((f_real.view(C, -1, d).mean(1) - f_syn.view(C, -1, d).mean(1)) ** 2).sum(1)).sum()
    loss.backward()
    return float(loss.detach()), img.grad.detach(), clip.grad.detach()


@pytest.fixture(scope="module")
def cpu_steps():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    stills, static0 = still_dm_case()
    be = RecordingBackend()
    tr = still_dm_trainer(be, "cpu", stills, static0)
    rec = []
    for it in range(STEPS):
        before = (tr.static.clone(), tr.buf.clone())
        loss = float(tr.step(it))
        rec.append(dict(before=before, loss=loss, g=be.grads[it], static=tr.static.clone(), buf=tr.buf.clone(), clips=tr.image_syn.clone()))
    return dict(stills=stills, static0=static0, tr=tr, rec=rec)


def test_three_still_dm_steps_equal_autograd_through_expand(cpu_steps):
    """Every step is compared with the hand-written loop started from the trainer's own state before that step.  The loss is the
    same number.  The image gradient is a T-term fp32 sum taken in ascending t by the trainer and in autograd's own order by
    ``expand``'s backward: two orders of one sum differ by at most (T-1) * 2^-24 * sum_t |g_t|, so the two updates differ by at
    most lr times that, elementwise (the bar of test_still_cpu.py::test_still_step_equals_autograd_through_expand).  What the
    optimiser makes of the trainer's gradient -- first step ``buf = g``, then ``buf = mu * buf + g``; ``static -= lr * buf`` --
    is checked bit for bit."""
    tr = cpu_steps["tr"]
    assert tr.steps_done == STEPS and tr.static.shape == (C * SPC, 3, HW, HW) and tr.buf.shape == tr.static.shape and tr.ipc == tr.spc == SPC
    assert torch.equal(cpu_steps["rec"][0]["before"][0], cpu_steps["static0"])
    for it, r in enumerate(cpu_steps["rec"]):
        static_b, buf_b = r["before"]
        loss_ref, g_ref, g_frames = autograd_dm_step(it, cpu_steps["stills"], static_b)
        assert r["loss"] == loss_ref, it
        assert float(g_ref.abs().max()) > 0
        bound = LR * (T - 1) * 2.0 ** -24 * g_frames.double().abs().sum(1)
        d = LR * (r["g"].double() - g_ref.double())
        print("still DM step %d: loss %.9g; max |d| %.3e, max bound %.3e, elements with d != 0: %d of %d"
              % (it, loss_ref, float(d.abs().max()), float(bound.max()), int((d != 0).sum()), d.numel()))
        assert bool((d.abs() <= bound).all()), it
        buf = r["g"].clone() if it == 0 else buf_b * MU + r["g"]
        assert torch.equal(r["buf"], buf) and torch.equal(r["static"], static_b - LR * buf), it
        assert torch.equal(r["clips"], r["static"].unsqueeze(1).expand(-1, T, -1, -1, -1)), it          # the next step's clips
    assert torch.equal(cpu_steps["rec"][0]["buf"], cpu_steps["rec"][0]["g"])          # first step: the buffer IS the gradient
    assert torch.equal(tr.gather_syn(), tr.image_syn) and tr.gather_static() is tr.static


def test_fp32_oracle_is_well_inside_the_gpu_bars_against_fp64(cpu_steps):
    """tests/test_gpu_still_dm.py compares HIP with this fp32 oracle run (loss 1e-3 relative at every step, image update 5e-2
    rel-l2 per class).  The seed is not a chaotic one if the fp32 oracle itself stays at least ten times inside both bars
    against the same three steps, momentum included, in float64."""
    static = cpu_steps["static0"].double()
    buf = None
    rel_loss = []
    for it in range(STEPS):
        loss64, g64, _ = autograd_dm_step(it, cpu_steps["stills"], static, dtype=torch.float64)
        buf = g64 if buf is None else MU * buf + g64
        static = static - LR * buf
        rel_loss.append(abs(cpu_steps["rec"][it]["loss"] - loss64) / abs(loss64))
    up32, up64 = cpu_steps["tr"].static.double() - cpu_steps["static0"].double(), static - cpu_steps["static0"].double()
    per = [float((up32[c * SPC:(c + 1) * SPC] - up64[c * SPC:(c + 1) * SPC]).norm() / up64[c * SPC:(c + 1) * SPC].norm()) for c in range(C)]
    print("fp32 oracle vs float64, %d steps: loss rel %s, image update rel-l2 per class %s"
          % (STEPS, ["%.3e" % e for e in rel_loss], ["%.3e" % e for e in per]))
    assert max(rel_loss) < 1e-4 and max(per) < 5e-3


# ---- DMTrainer's hooks -----------------------------------------------------------------------------------------------------

def test_dm_trainer_hooks_default_to_the_expressions_they_replaced():
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(4, T, 3, HW, HW, generator=g)
    be = OracleBackend()
    tr = distill.DMTrainer(be, distill.RealPool(clips, [2, 2], [0, 2]), 2, 1, batch_real=2, lr_img=0.5)
    be.set_weights(be.new_network(0))
    idx = torch.tensor([1, 0, 3, 2])
    assert torch.equal(tr._embed_real(idx), be.embed_pool(clips, idx))
    assert torch.equal(tr._embed_real(idx, [(2, 2)]), be.embed_pool(clips, idx))          # (a backend without embed_pool_segments)
    assert torch.equal(tr._real_features(idx), be.embed_pool(clips, idx))
    grad = torch.randn(tr.image_syn.shape, generator=g)
    x, buf = tr.image_syn.clone(), tr.buf.clone()
    for first in (True, False):
        tr._apply_pixel_grad(grad, first)
        OracleBackend.sgd(None, x, buf, grad, 0.5, 0.5, first)
        assert torch.equal(tr.image_syn, x) and torch.equal(tr.buf, buf)
    assert distill.StillDMTrainer._embed_real is not distill.DMTrainer._embed_real
    assert distill.StillDMTrainer._apply_pixel_grad is not distill.DMTrainer._apply_pixel_grad
    assert distill.StillDMTrainer.step is distill.DMTrainer.step and distill.StillDMTrainer._flush_backward is distill.DMTrainer._flush_backward


def test_still_dm_trainer_refusals_and_init_real():
    geo = plan.NetGeometry(T, HW, HW)
    be = OracleBackend()
    with pytest.raises(ValueError, match="pool of stills"):
        distill.StillDMTrainer(be, distill.RealPool(torch.zeros(2, T, 3, HW, HW), [1, 1], [0, 1]), geo, 2, 1, 1, 0.1)
    with pytest.raises(ValueError, match="rows 1..3 of a pool of 2"):
        distill.StillDMTrainer(be, distill.RealPool(torch.zeros(2, 3, HW, HW), [1, 2], [0, 1]), geo, 2, 1, 1, 0.1)
    stills = torch.arange(6.).view(6, 1, 1, 1).expand(6, 3, HW, HW).contiguous()
    with pytest.raises(ValueError, match="allreduce"):
        distill.StillDMTrainer(be, distill.RealPool(stills, [3, 3], [0, 3]), geo, 2, 2, 1, 0.1, exchange="allreduce")
    with pytest.raises(ValueError, match="static"):
        distill.StillDMTrainer(be, distill.RealPool(stills, [3, 3], [0, 3]), geo, 2, 2, 1, 0.1, static=torch.zeros(3, 3, HW, HW))
    tr = distill.StillDMTrainer(be, distill.RealPool(stills, [3, 3], [0, 3]), geo, 2, 2, 1, 0.1)
    assert tr.static[:, 0, 0, 0].tolist() == [0.0, 1.0, 3.0, 4.0] and tr.ipc == tr.spc == 2          # --init real: the first spc stills
    assert tr.image_syn.shape == (4, T, 3, HW, HW) and tr.buf.shape == tr.static.shape and not tr.buf.any()


# ---- sharding: two ranks reproduce one -------------------------------------------------------------------------------------

def _dm_run(rank, world, shard):
    stills, static0 = still_dm_case()
    lo, hi = distill.class_range(C, rank, world)          # (the rows of a rank's memories: class blocks under 'class' and 'batch')
    tr = still_dm_trainer(OracleBackend(), "cpu", stills, static0[lo * SPC:hi * SPC], rank=rank, world=world, shard=shard)
    assert tr.owned_classes() == list(range(lo, hi))
    losses = [float(tr.global_loss(tr.step(it))) for it in range(2)]
    return losses, tr.gather_static(), tr.gather_syn()


def _worker_dm(rank, world, port, q, shard):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        losses, static, clips = _dm_run(rank, world, shard)
        if rank == 0:
            q.put((losses, static.numpy(), clips.numpy()))
    finally:
        dist.destroy_process_group()


def _worker_dm_class(rank, world, port, q):
    _worker_dm(rank, world, port, q, "class")


def _worker_dm_batch(rank, world, port, q):
    _worker_dm(rank, world, port, q, "batch")


@pytest.fixture(scope="module")
def one_rank_run():
    torch.set_num_threads(4)
    return _dm_run(0, 1, "class")


@pytest.mark.parametrize("worker", [_worker_dm_class, _worker_dm_batch], ids=["class", "batch"])
def test_still_dm_trainer_sharding_identity_two_ranks_gloo(worker, one_rank_run):
    """Two steps on two ranks -- one class each ('class'), or half of every class's real batch each with the feature sums
    all-reduced ('batch') -- reproduce the one-rank run: summed loss, gathered images in class order, gathered clips = the images
    repeated.  Bars: the identity bars of tests/test_distributed_cpu.py (loss rtol 2e-5; memories rtol 1e-4, atol 1e-6 -- the
    oracle's summation order depends on the thread count and on how the batch is cut)."""
    from tests.test_distributed_cpu import _spawn
    want_l, want_s, _ = one_rank_run
    got_l, got_s, got_c = _spawn(worker, 2)
    np.testing.assert_allclose(got_l, want_l, rtol=2e-5)
    np.testing.assert_allclose(got_s, want_s.numpy(), rtol=1e-4, atol=1e-6)
    assert got_s.shape == (C * SPC, 3, HW, HW) and got_c.shape == (C * SPC, T, 3, HW, HW)
    assert all(np.array_equal(got_c[:, t], got_s) for t in range(T))
    assert not np.allclose(want_s.numpy(), still_dm_case()[1].numpy())


# ---- the driver ------------------------------------------------------------------------------------------------------------

def _args(tmp_path, *extra):
    return run_dm.build_parser().parse_args([
        "--memories", "static", "--dataset", "synthetic", "--num_classes", "2", "--pool_per_class", "3", "--spc", "2", "--Iteration", "1",
        "--batch_real", "2", "--frames", "8", "--im_size", "64", "--lr_img", "0.1", "--eval_it", "2", "--num_eval", "1",
        "--epoch_eval_train", "1", "--batch_train", "4", "--save_path", str(tmp_path), "--no_eval"] + list(extra))


def test_run_dm_static_mode_on_the_oracle_backend(tmp_path):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    log = []
    tr = run_dm.run(_args(tmp_path), backend=OracleBackend(), log=log)
    losses = [r["Loss"] for r in log if "Loss" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[0] > 0
    assert type(tr) is distill.StillDMTrainer and tr.steps_done == 2
    assert tr.static.shape == (4, 3, 64, 64) and tr.image_syn.shape == (4, 8, 3, 64, 64)
    path = os.path.join(tmp_path, "Static_DM", "synthetic_spc2_0.1", "static_0.pt")
    static = checkpoint.load_static(path)
    assert static.shape == (4, 3, 64, 64) and static.dtype == torch.float32
    pool = run_dm_pool(_args(tmp_path))
    assert torch.equal(static, pool.clips[[0, 1, 3, 4]])          # --init real, saved before the first step
    assert not torch.equal(tr.static, static)
    with pytest.raises(ValueError, match="single\\*"):
        run_dm.run(_args(tmp_path, "--dataset", "miniUCF101"), backend=OracleBackend(), log=[])
    with pytest.raises(ValueError, match="allreduce"):
        run_dm.run(_args(tmp_path), backend=OracleBackend(), log=[], exchange="allreduce")


def run_dm_pool(args):
    from video_distillation_amd import run_dc
    return run_dc.load_stills(args, 0, 1, torch.device("cpu"))[0]


def test_run_dm_static_noise_comes_from_the_seed_and_ipc_is_not_read(tmp_path):
    args = _args(tmp_path, "--init", "noise", "--seed", "3", "--Iteration", "0", "--ipc", "7")
    tr = run_dm.run(args, backend=OracleBackend(), log=[])
    noise = torch.randn((4, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    assert tr.ipc == 2 and tr.steps_done == 1
    assert torch.allclose(tr.static + LR * tr.buf, noise, rtol=0, atol=1e-6)          # one step from the noise: static = noise - lr * g
    saved = checkpoint.load_static(os.path.join(tmp_path, "Static_DM", "synthetic_spc2_0.1", "static_0.pt"))
    assert torch.equal(saved, noise)          # drawn in full on the host from --seed, saved before the first step


def test_flags_of_the_static_mode():
    args = run_dm.build_parser().parse_args([])
    assert (args.memories, args.spc, args.seed) == ("images", 2, 0)
    with pytest.raises(SystemExit):
        run_dm.build_parser().parse_args(["--memories", "s2d"])
    from video_distillation_amd import run_dc
    assert callable(run_dc.load_stills) and callable(run_dc.StillTestLoader)
