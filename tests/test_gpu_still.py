"""The ``vds_`` kernels of csrc/still.hip through the C ABI against the torch expression / a host loop of float adds, one
``distill.StillGMTrainer`` step on the HIP ops against the oracle ops, the tie argument of its docstring against clips without
ties, and ``run_dc --memories static`` end to end into an ``S2DTrainer`` step.

Shapes: (5, 7) has 3*H*W = 105, no multiple of 4: the scalar kernels; (6, 6) = 108 floats = 27 float4, less than one workgroup
of the vector kernels, whose bound check cuts the block; (64, 64) = 3072 float4 = 12 workgroups per image; the same (6, 6) from
a base 4 bytes off a 16-byte boundary takes the scalar kernels again.  T = 1 (no add at all), 8, 16; n = 1, 3.  Two more sizes
reach the loops no small shape enters: 65 537 images of (2, 2) (grid y is capped at 65 535: the image loop of the vector kernels
takes a second turn) and 40 001 of (5, 7) (4.2 M elements, past the 16 384 x 256 the scalar grid covers in one pass).

Tolerances: expand copies, reduce adds in a stated order: both are compared bit for bit.  Against fp64 the T-term fp32 sum is
within (T-1) * 2^-24 * sum_t |g_t| (one rounding of at most half an ulp of a partial sum, itself at most the sum of the
magnitudes, per add).  The trainer tests take their bars from test_gm_trainer_hip_matches_oracle_trainer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(5, 7), (6, 6), (64, 64)]


def _call(name, *args):
    from video_distillation_amd import hip
    rc = getattr(hip.lib(), name)(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _guarded(numel, offset=0):
    """A device buffer of ``numel`` floats starting ``offset`` floats into an allocation, NaN-filled, with ``GUARD`` floats of a
    sentinel behind it -> (the allocation, the view to hand to the kernel)."""
    whole = torch.full((offset + numel + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    whole[offset + numel:] = -777.0
    return whole, whole[offset:offset + numel]


def _guard_intact(whole, numel, offset=0):
    return bool((whole[offset + numel:] == -777.0).all()) and (offset == 0 or bool(torch.isnan(whole[:offset]).all()))


def _expand_case(n_src, index, T, H, W, offset=0):
    g = torch.Generator().manual_seed(1000 * H + 10 * T + n_src)
    images = torch.randn(n_src, 3, H, W, generator=g)
    src_whole = torch.zeros(offset + images.numel(), dtype=torch.float32, device="cuda")
    src = src_whole[offset:]
    src.copy_(images.reshape(-1))
    idx = None if index is None else torch.as_tensor(index, dtype=torch.int64).cuda()
    n = n_src if index is None else len(index)
    whole, out = _guarded(n * T * 3 * H * W, offset)
    assert (src.data_ptr() % 16 == 0) == (offset == 0) and (out.data_ptr() % 16 == 0) == (offset == 0)
    rc = _call("vds_still_expand", src.data_ptr(), 0 if idx is None else idx.data_ptr(), n, T, H, W, out.data_ptr())
    assert rc == 0
    want = (images if index is None else images[torch.as_tensor(index)]).unsqueeze(1).expand(-1, T, -1, -1, -1).contiguous()
    assert torch.equal(out.cpu().view(n, T, 3, H, W), want)
    assert _guard_intact(whole, out.numel(), offset)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("T", [1, 8, 16])
def test_expand_is_the_torch_expression_bit_for_bit(T, H, W):
    for n in (1, 3):
        _expand_case(n, None, T, H, W)
    _expand_case(3, [2, 0, 1], T, H, W)          # a permutation
    _expand_case(3, [1, 1, 2, 1, 0], T, H, W)          # repeated rows, more clips than images
    _expand_case(1, [0, 0], T, H, W)


def _ascending_sum(g):
    """(n, T, ...) float32 -> the host loop of ascending np.float32 adds over T."""
    out = g[:, 0].copy()
    for t in range(1, g.shape[1]):
        out = (out + g[:, t]).astype(np.float32)
    return out


def _reduce_case(n, T, H, W, offset=0):
    rng = np.random.default_rng(1000 * H + 10 * T + n)
    g = (rng.normal(0.0, 1.0, (n, T, 3, H, W)) * 10.0 ** rng.integers(-3, 3, (n, T, 1, 1, 1))).astype(np.float32)
    src_whole = torch.zeros(offset + g.size, dtype=torch.float32, device="cuda")
    src = src_whole[offset:]
    src.copy_(torch.from_numpy(g).reshape(-1))
    outs = []
    for _ in range(2):
        whole, out = _guarded(n * 3 * H * W, offset)
        assert _call("vds_still_reduce", src.data_ptr(), n, T, H, W, out.data_ptr()) == 0
        assert _guard_intact(whole, out.numel(), offset)
        outs.append(out.cpu().numpy().reshape(n, 3, H, W))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))          # a second run: identical bits
    assert np.array_equal(outs[0].view(np.uint32), _ascending_sum(g).view(np.uint32))
    exact = g.astype(np.float64).sum(1)
    bound = (T - 1) * 2.0 ** -24 * np.abs(g.astype(np.float64)).sum(1)
    assert (np.abs(outs[0].astype(np.float64) - exact) <= bound).all()


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("T", [1, 8, 16])
def test_reduce_is_the_ascending_float_sum_bit_for_bit_and_repeatable(T, H, W):
    for n in (1, 3):
        _reduce_case(n, T, H, W)


def test_bases_off_a_16_byte_boundary_take_the_scalar_kernels():
    _expand_case(3, [2, 2, 0], 8, 6, 6, offset=1)
    _reduce_case(3, 8, 6, 6, offset=1)


@pytest.mark.parametrize("n,H,W", [(65537, 2, 2), (40001, 5, 7)])
def test_the_loops_past_one_pass_of_the_grid(n, H, W):
    _expand_case(n, None, 2, H, W)
    _reduce_case(n, 2, H, W)
    index = np.random.default_rng(n).integers(0, 5, n)
    _expand_case(5, index.tolist(), 1, H, W)


@pytest.mark.parametrize("H,W", SHAPES)
def test_frame_order_reduce_of_weighted_expand(H, W):
    """reduce(expand(x) * w_t) = the ascending sum of w_t * x: a kernel that walked the frames in another order, or wrote frame t
    to another slot, would add the same terms in another order -- with weights spread over six decades that shows in the bits."""
    from video_distillation_amd import hip
    T, n = 8, 3
    g = torch.Generator().manual_seed(H)
    x = torch.randn(n, 3, H, W, generator=g)
    w = torch.tensor([3.0e-3, 1.0e3, -7.0, 0.11, 9.0e2, -1.0e-2, 5.0, -1.0e3]).view(1, T, 1, 1, 1)
    clips = hip.still_expand(x.cuda(), None, T)
    assert torch.equal(clips.cpu(), x.unsqueeze(1).expand(-1, T, -1, -1, -1))
    got = hip.still_reduce((clips * w.cuda()).contiguous()).cpu().numpy()
    terms = (x.unsqueeze(1) * w).numpy()          # (one fp32 product per term, as on the device)
    assert np.array_equal(got.view(np.uint32), _ascending_sum(terms).view(np.uint32))
    assert not np.array_equal(got, _ascending_sum(terms[:, ::-1]))          # (the order is visible at these weights)


def test_python_wrappers_check_the_index_on_the_host():
    from video_distillation_amd import hip
    x = torch.randn(3, 3, 5, 7).cuda()
    for bad in ([0, 3], [-1], torch.tensor([1, 5]), torch.tensor([3]).cuda()):
        with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
            hip.still_expand(x, bad, 4)
    out = hip.still_expand(x, np.array([2, 2]), 4)
    assert torch.equal(out.cpu(), x.cpu()[[2, 2]].unsqueeze(1).expand(-1, 4, -1, -1, -1))
    assert hip.still_expand(x, [], 4).shape == (0, 4, 3, 5, 7) and hip.still_reduce(torch.zeros(0, 4, 3, 5, 7).cuda()).shape == (0, 3, 5, 7)


# ---- trainer --------------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def still_steps():
    """One still step (outer_loop = 1) on the inputs of tests/test_still_cpu.py: oracle ops on the CPU, HIP ops on cuda:0.  The
    first step's momentum buffer is the image gradient."""
    from tests.cpu_backend import OracleGMOps
    from tests.test_still_cpu import still_case, still_trainer
    from video_distillation_amd import distill
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    stills, static0, init = still_case()
    out = {"stills": stills, "static0": static0, "init": init}
    for name, ops, dev in (("cpu", OracleGMOps("ours"), "cpu"), ("hip", distill.HipGMOps("cuda:0", "ours"), "cuda:0")):
        tr = still_trainer(ops, dev, stills, static0, init)
        loss = float(tr.step(0))
        out[name] = dict(loss=loss, g=tr.buf.cpu().clone(), static=tr.static.cpu().clone(), clips=tr.image_syn.cpu().clone())
    return out


def test_still_step_hip_matches_oracle(still_steps):
    """Bars of test_gm_trainer_hip_matches_oracle_trainer: loss within 1e-3 relative, image update within 5e-2 rel-l2 per class
    (arg-max flips allowed).  The seed is not a chaotic one: on the CPU the fp32 oracle is, against the same computation in
    float64, 1.5e-8 off on the loss and 1.6e-5 / 8.3e-6 rel-l2 off on the two classes' updates
    (tests/test_still_cpu.py::test_fp32_oracle_is_well_inside_the_gpu_bars_against_fp64 asserts ten times inside both bars)."""
    from tests.test_still_cpu import C, T
    cpu, hip_ = still_steps["cpu"], still_steps["hip"]
    static0 = still_steps["static0"]
    rel_loss = abs(hip_["loss"] - cpu["loss"]) / cpu["loss"]
    per = [_rel(hip_["static"][k] - static0[k], cpu["static"][k] - static0[k]) for k in range(C)]
    print("still step: loss HIP %.6f oracle %.6f (rel %.1e); image update rel-l2 per class %s"
          % (hip_["loss"], cpu["loss"], rel_loss, ["%.1e" % e for e in per]))
    assert rel_loss < 1e-3
    assert max(per) < 5e-2
    assert torch.equal(hip_["clips"], hip_["static"].unsqueeze(1).expand(-1, T, -1, -1, -1))          # re-expanded after the update


def test_ties_do_not_move_the_image_gradient(still_steps):
    """The frames of a still clip are equal, so the temporal max-pools see exact ties; the docstring of StillGMTrainer argues
    that the pick among equal frames cannot change the image gradient.  Here: the same step by plain ``GMTrainer`` on clips
    whose frames are the stills plus per-frame noise (no two frames equal: no exact ties), its clip gradient summed over T by
    ``still_reduce``, against the still step's image gradient -- within the rel-l2 bar of the test above, 5e-2 per class.
    The noise's own effect, measured on the oracle (tests/test_still_cpu.py::test_frame_noise_moves_the_gradient_far_less_than_
    the_bar): 3.8e-3 / 1.5e-3 rel-l2 at the amplitude 1e-4 used here, under a tenth of the bar (the issue's 1e-3 gave 1.8e-2 /
    2.9e-2 there, so the amplitude was lowered, not the bar)."""
    from tests.test_still_cpu import C, T, HW, LR, still_noise
    from video_distillation_amd import distill, hip, plan
    stills, static0, init = still_steps["stills"], still_steps["static0"], still_steps["init"]
    noise = still_noise()
    clips = stills.unsqueeze(1).expand(-1, T, -1, -1, -1) + noise
    syn0 = static0.unsqueeze(1).expand(-1, T, -1, -1, -1) + noise[[0, 3]]
    assert all(not torch.equal(clips[:, t], clips[:, t + 1]) for t in range(T - 1))
    pool = distill.RealPool(clips.contiguous().cuda(), [3] * C, [0, 3])
    tr = distill.GMTrainer(distill.HipGMOps("cuda:0", "ours"), pool, plan.NetGeometry(T, HW, HW), C, 1, batch_real=2, lr_img=LR,
                           lr_net=0.01, image_syn=syn0.contiguous().cuda(), outer_loop=1, inner_loop=1, dropout_p=0.0, net_init=init)
    loss = float(tr.step(0))
    g_noisy = hip.still_reduce(tr.buf.contiguous()).cpu()          # first step: buf is the clip gradient
    g_still = still_steps["hip"]["g"]
    per = [_rel(g_noisy[k], g_still[k]) for k in range(C)]
    print("ties: loss without ties %.6f, with %.6f; image gradient rel-l2 per class %s" % (loss, still_steps["hip"]["loss"], ["%.1e" % e for e in per]))
    assert max(per) < 5e-2


def test_run_dc_static_end_to_end_feeds_an_s2d_step(tmp_path):
    """``run_dc --memories static --dataset synthetic`` at 8x64x64, 2 classes, Iteration 2 with one evaluation of 2 epochs: finite
    numbers in the log, and the ``static_0.pt`` it writes is the ``--path_static`` of one ``S2DTrainer`` step (``run_s2d``,
    Iteration 0)."""
    from video_distillation_amd import checkpoint, distill, run_dc, run_s2d
    common = ["--dataset", "synthetic", "--num_classes", "2", "--frames", "8", "--im_size", "64", "--pool_per_class", "4", "--batch_real", "2",
              "--save_path", str(tmp_path)]
    log = []
    args = run_dc.build_parser().parse_args(common + [
        "--memories", "static", "--spc", "2", "--Iteration", "2", "--eval_it", "3", "--num_eval", "1", "--epoch_eval_train", "2",
        "--lr_img", "0.01", "--lr_net", "0.01", "--batch_train", "4"])
    tr = run_dc.run(args, log=log)
    torch.cuda.synchronize()
    assert type(tr) is distill.StillGMTrainer and tr.steps_done == 3
    losses = [r["Loss"] for r in log if "Loss" in r]
    accs = [r for r in log if "Accuracy/ConvNet3D" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and len(accs) == 1
    assert all(np.isfinite([accs[0][k] for k in ("Accuracy/ConvNet3D", "Max_Accuracy/ConvNet3D", "Std/ConvNet3D", "Max_Std/ConvNet3D")]))
    assert 0.0 <= accs[0]["Accuracy/ConvNet3D"] <= 1.0 and torch.isfinite(tr.static).all()
    path = os.path.join(tmp_path, "Static_DC", "synthetic_spc2_0.01", "static_0.pt")
    static = checkpoint.load_static(path)
    assert static.shape == (4, 3, 64, 64) and torch.isfinite(static).all()
    log2 = []
    s2d = run_s2d.build_parser().parse_args(common + [
        "--path_static", path, "--no_train_static", "--vpc", "1", "--spc", "2", "--dpc", "2", "--Iteration", "0", "--no_eval"])
    tr2 = run_s2d.run(s2d, log=log2)
    torch.cuda.synchronize()
    assert torch.equal(tr2.static.cpu(), static) and tr2.steps_done == 1
    assert [np.isfinite(r["Loss"]) for r in log2 if "Loss" in r] == [True]
