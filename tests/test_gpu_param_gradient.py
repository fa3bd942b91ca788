"""The PARAMETER side of one level -- bias and weight gradient -- as the linear operator it is, against fp64.

A random pooled gradient in the layout the level really receives (layout 0 at level 2, channels-last below), random arg-max bytes
(ReLU-dead windows among them) and a random source (fp32 pixels at level 0, channels-last 16-bit slots in the forward format's planes
below) go through exactly what train.py runs for a level: ``EmbedEngine.level_unpool(dense=False)`` for the power-of-two scale,
then ``TrainEngine.level_param_grads`` -- vd_bias_grad_pooled[_ordered], vd_clip_minor_*, the fused vd_unpool_relu_bwd_packed, the
weight-gradient tile program (plan.plan_wgrad) and vd_replica_sum.  The reference is fp64 on the host (tests/param_gradient_cases.py):
dense dy by index arithmetic, dW by autograd of F.conv3d with respect to the weight, db = dy summed.  Nothing is decided anywhere.

g_w / g_b are ACCUMULATED into: they start from seeded non-zero tensors at the front of larger NaN-filled allocations, whose tails
must still be all NaN afterwards.

Weight gradient: rel-L2 of the whole tensor and the worst rel-L2 over three families of slices -- per tap (147 slices over (cout,
cin)), per output channel, per input channel -- for three input patterns: everything random; the source non-zero only on its border
shell (dW then depends on the padding taps and box edges alone); the pooled gradient non-zero only in the last pooled row and
column (the ragged boxes).  A slice whose reference is identically zero must be exactly zero (at level 2, 39 of the 147 taps see
only padding at 64 x 66 x 4, 65 x 63 x 4, 64 x 64 x 8 and 96 x 80 x 12, 57 at 70 x 58 x 4; with one clip every output channel whose only window is dead).
Bias gradient: element-wise within AO.gamma(k) x the sum of the absolute terms, k as tests/test_gpu_aux_kernels.py derives it.

Clip sizes: 64 x 66 x 4, 65 x 63 x 4 and 70 x 58 x 4 (conv grids 32 x 33, 33 x 32, 35 x 29 and 9 x 7: ragged last boxes, rows / columns no
pool window covers), 64 x 64 x 8 (also with exactly 8 and with 17 clips at level 1: one full clip chunk; three, the last holding one
clip), 96 x 80 x 12 and 112 x 112 x 16.  The block of positions, the number of boxes and of accumulation copies the planner chose are
asserted per case (PLANNED), so that a planner change is a named failure and not a silently different test.

Bounds: what tests/test_gpu_wgrad.py holds a single linear conv program to -- f16x3 2e-5, bf16x3 1e-4, f16 2e-3 -- applied to every
slice family and every input pattern.  tests/test_wgrad_emulation_cpu.py recomputes what the operand rounding ALONE costs for these
inputs and asserts that each bar leaves a factor of four over it (worst floors, all three patterns alike: f16 4.9e-4, bf16x3 6.5e-6,
f16x3 1.3e-6, each per output channel at level 2 with one clip; per tap / per input channel / whole: 3.8e-4, 4.4e-6, 9.2e-8 at most).
They are NOT tightened from the measured error here; that is a later change with these figures in hand.
MEASURED on an MI355X, worst over all cases and patterns (the ordered, dense-entry, magnitude 1e-7 / 1e4 and odd-block runs included):
                     whole      per tap    per cout   per cin
    f16x3   level 0  3.35e-07   3.90e-07   3.80e-07   3.37e-07
            level 1  2.60e-07   2.89e-07   2.73e-07   2.65e-07
            level 2  1.15e-07   1.34e-07   1.97e-06   1.21e-07
    bf16x3  level 0  4.47e-06   5.35e-06   5.06e-06   4.50e-06
            level 1  4.44e-06   4.63e-06   5.18e-06   4.58e-06
            level 2  4.57e-06   5.46e-06   8.38e-06   5.51e-06
    f16     level 0  3.00e-04   3.76e-04   3.55e-04   3.05e-04
            level 1  2.96e-04   3.06e-04   3.45e-04   3.01e-04
            level 2  2.96e-04   3.59e-04   4.94e-04   3.73e-04
(the level-2 per-output-channel figures are the one-clip cases: a slice of a single pool window, where the format's own floor is
1.3e-6 / 6.5e-6 / 4.9e-4.)  Bias gradient: the worst |error| is 0.008 of its bound.  Dense entry against the pooled one: 4.9e-08."""
import pytest
import torch

from tests import aux_oracle as AO
from tests import param_gradient_cases as C
from tests.test_gpu_wgrad import _slots_from_dense

pytestmark = pytest.mark.gpu

WORST = {}          # (format, level) -> {family: worst rel-L2 so far}
_TRAINERS = {}

# (clip size, level, clips) -> (block of positions, boxes, accumulation copies); the same for one and two operand planes
PLANNED = {
    (C.G_A, 0, 1): ((1, 2, 14), 192, 6), (C.G_A, 0, 3): ((1, 2, 14), 192, 6), (C.G_A, 1, 9): ((2, 2, 8), 8, 1),
    (C.G_A, 2, 9): ((1, 2, 2), 2, 1), (C.G_A, 2, 1): ((1, 2, 2), 2, 1),
    (C.G_B, 0, 1): ((1, 2, 14), 204, 7), (C.G_B, 0, 3): ((1, 2, 14), 204, 7), (C.G_B, 1, 9): ((2, 2, 8), 8, 1),
    (C.G_B, 2, 9): ((1, 2, 2), 2, 1), (C.G_B, 2, 1): ((1, 2, 2), 2, 1),
    (C.G_C, 0, 1): ((1, 2, 14), 216, 7), (C.G_C, 0, 3): ((1, 2, 14), 216, 7), (C.G_C, 1, 9): ((2, 2, 7), 10, 1),
    (C.G_C, 2, 9): ((1, 2, 2), 2, 1), (C.G_C, 2, 1): ((1, 2, 2), 2, 1),
    (C.SMALL, 0, 1): ((2, 4, 4), 256, 9), (C.SMALL, 0, 3): ((2, 4, 4), 256, 9), (C.SMALL, 1, 9): ((4, 2, 8), 8, 1),
    (C.SMALL, 1, 8): ((8, 4, 4), 4, 1), (C.SMALL, 1, 17): ((4, 2, 8), 8, 1), (C.SMALL, 2, 9): ((1, 2, 2), 4, 1),
    (C.SMALL, 2, 1): ((2, 2, 2), 2, 1),
    (C.ODD, 0, 2): ((4, 4, 4), 360, 12), (C.ODD, 1, 2): ((4, 4, 10), 9, 1), (C.ODD, 2, 2): ((2, 3, 3), 3, 1),
    (C.FULL, 0, 2): ((4, 2, 14), 448, 16), (C.FULL, 1, 2): ((8, 2, 14), 14, 1), (C.FULL, 2, 2): ((4, 4, 4), 2, 1),
}


def _trainer(geom, fmt):
    """One training engine per (clip size, backward format); the forward runs hi+lo pairs of the same 16-bit type, as in
    tests/test_gpu_input_gradient.py::_engine."""
    from video_distillation_amd import plan, train
    if (geom, fmt) not in _TRAINERS:
        _TRAINERS[(geom, fmt)] = train.TrainEngine(plan.NetGeometry(*geom), 4, (1, 1, 1), "cuda:0", prec="f16x3" if fmt == "f16" else fmt,
                                                   prec_bwd=fmt)
    return _TRAINERS[(geom, fmt)]


def _guarded(start, extra):
    """``start`` at the front of a NaN-filled allocation: (whole allocation, view of the front in ``start``'s shape)."""
    big = torch.full((start.numel() + extra,), float("nan"), dtype=torch.float32, device="cuda")
    big[:start.numel()] = start.reshape(-1).cuda()
    return big, big[:start.numel()].view(start.shape)


def _source(eng, li, x):
    """The level's source as the trainer holds it: -> (tensor, is_pixels, slots per plane)"""
    if li == 0:
        return x.permute(0, 2, 1, 3, 4).contiguous().cuda(), True, 0          # (nb, T, 3, H, W) fp32 pixels
    slots = _slots_from_dense(x, eng.prec_name, eng.planes).cuda()
    return slots, False, int(slots[0].numel() // 8)


def _run_level(te, li, nb, inp, entry="pooled"):
    """``level_unpool`` for the scale, then the parameter side, into guarded g_w / g_b that start from w0 / b0.
    ``entry`` = "dense": WgradOp.run on the dense slots of ``level_unpool(dense=True)`` instead (what ``_down_sweep`` uses; no bias).
    -> (g_w - w0, g_b, both fp64 on the host)"""
    g, am, layout, x, w0, b0 = inp
    eng = te.eng
    gd, amd = g.cuda(), am.cuda()
    src, is_pix, plane = _source(eng, li, x)
    wbig, g_w = _guarded(w0, 4096)
    bbig, g_b = _guarded(b0, 256)
    if entry == "dense":
        slots, nslots, sc, inv = eng.level_unpool(li, nb, gd, layout, amd, dense=True)
        te._wgrad(li, nb).run(src, is_pix, plane, slots, nslots, g_w, out_scale=inv)
    else:
        _, _, sc, inv = eng.level_unpool(li, nb, gd, layout, amd, dense=False)
        te.level_param_grads(li, nb, gd, layout, amd, src, is_pix, plane, sc, inv, g_w, g_b)
    torch.cuda.synchronize()
    wres, bres = wbig.cpu(), bbig.cpu()
    assert bool(torch.isnan(wres[w0.numel():]).all()), "level %d wrote behind its weight gradient" % li
    assert bool(torch.isnan(bres[b0.numel():]).all()), "level %d wrote behind its bias gradient" % li
    assert bool(torch.isfinite(wres[:w0.numel()]).all()) and bool(torch.isfinite(bres[:b0.numel()]).all())
    return wres[:w0.numel()].view(w0.shape).double() - w0.double(), bres[:b0.numel()].double()


def _check_weights(dw, want, fmt, li, label):
    worst, zeros = C.slice_errors(dw, want)
    rec = WORST.setdefault((fmt, li), {k: 0.0 for k in C.FAMILIES})
    for k in C.FAMILIES:
        rec[k] = max(rec[k], worst[k][0])
    print("weight gradient %s level %d %s: %s | zero slices %s | so far %s" % (
        fmt, li, label, ", ".join("%s %.2e at %d" % (k, worst[k][0], worst[k][1]) for k in C.FAMILIES),
        {k: v for k, v in zeros.items() if v}, " / ".join("%.2e" % rec[k] for k in C.FAMILIES)))
    for k in C.FAMILIES:
        assert worst[k][0] < C.BAR[fmt], (k, worst[k])
    return zeros


def _check_bias(db, ref, terms, b0, li, nb, geom, ordered, label):
    """|db - (b0 + ref)| <= gamma(k) x (sum |terms| + |b0|).  A workgroup owns 256 pooled positions of one clip: <= 256 adds inside
    it, then (atomic) one add per (clip, block) onto db, or (ordered) the partial sums folded in index order: <= ceil(rows / 32) adds
    per fold lane, 32 lanes, the add onto db (tests/test_gpu_aux_kernels.py::test_bias_grad_pooled)."""
    To, Ho, Wo = C.layer_dims(geom, li)[8:11]
    rows = nb * (-(-(To * Ho * Wo) // 256))
    k = 256 + (-(-rows // 32) + 33 if ordered else rows)
    bound = AO.gamma(k) * (terms + b0.double().abs())
    err = (db - (ref + b0.double())).abs()
    slack = float((err / bound.clamp_min(1e-300)).max())
    print("bias gradient level %d %s: worst |error| / bound %.3f (k = %d)" % (li, label, slack, k))
    assert bool((err <= bound).all()), (int((err > bound).sum()), slack)


def _check_case(te, geom, fmt, li, nb, patterns=C.PATTERNS, mag=1.0, ordered=False, label=""):
    out = {}
    for name in patterns:
        inp = C.pattern(geom, li, nb, name, mag)
        want, db_ref, db_terms = C.reference(geom, li, nb, name, mag)
        dw, db = _run_level(te, li, nb, inp)
        tag = "%s x %d clips, %s%s" % (geom, nb, name, label)
        zeros = _check_weights(dw, want, fmt, li, tag)
        _check_bias(db, db_ref, db_terms, inp[5], li, nb, geom, ordered, tag)
        out[name] = (dw, db, zeros)
    return out


@pytest.mark.parametrize("geom,fmt,li,nb", C.level_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_level_parameter_gradients_are_the_fp64_ones(geom, fmt, li, nb):
    te = _trainer(geom, fmt)
    op = te._wgrad(li, nb)
    assert (tuple(op.plan.meta["box"]), op.plan.nbox, op.replicas) == PLANNED[(geom, li, nb)]
    assert op.CCb == -(-nb // 8)
    res = _check_case(te, geom, fmt, li, nb)
    assert res["full"][2]["tap"] == C.padding_only_taps(geom, li)          # (level 2 of the 4-frame sizes: 39 and, at 70 x 58, 57 of 147)
    if li == 2 and geom[0] == 4 and nb == 1:
        assert res["full"][2]["cout"] > 0           # one window per output channel: the dead ones


@pytest.mark.parametrize("li,nb", [(0, 3), (1, 9)])
def test_ordered_mode_is_reproducible_and_as_exact(li, nb):
    """hip.set_deterministic(True): one accumulation copy per box folded in index order, the bias partial sums folded in index
    order -- the same bounds, and two runs bitwise equal."""
    from video_distillation_amd import hip
    te = _trainer(C.G_C, "f16x3")
    was = hip.deterministic()
    hip.set_deterministic(True)
    try:
        op = te._wgrad(li, nb)
        assert op.ordered and op.replicas == op.plan.nbox == PLANNED[(C.G_C, li, nb)][1]
        first = _check_case(te, C.G_C, "f16x3", li, nb, ordered=True, label=", ordered")
        again = _run_level(te, li, nb, C.pattern(C.G_C, li, nb, "full"))
    finally:
        hip.set_deterministic(was)
    assert torch.equal(first["full"][0], again[0]) and torch.equal(first["full"][1], again[1])


def test_dense_entry_gives_the_same_weight_gradient():
    """WgradOp.run on the dense slots of level_unpool(dense=True) with out_scale = inv: the same products as run_pooled in another
    summation order -- the same bounds, and within 1e-6 rel-L2 of it (the bar of test_weight_gradient_through_the_c_abi_alone)."""
    geom, li, nb = C.G_C, 1, 9
    te = _trainer(geom, "f16x3")
    inp = C.pattern(geom, li, nb, "full")
    want = C.reference(geom, li, nb, "full")[0]
    pooled, _ = _run_level(te, li, nb, inp)
    dense, _ = _run_level(te, li, nb, inp, entry="dense")
    _check_weights(dense, want, "f16x3", li, "%s x %d clips, dense entry" % (geom, nb))
    same = float((dense - pooled).norm() / pooled.norm())
    print("dense entry against the pooled one: rel-L2 %.1e" % same)
    assert same < 1e-6


@pytest.mark.parametrize("fmt", ["f16x3", "f16"])
@pytest.mark.parametrize("mag", [1e-7, 1e4])
def test_gradient_magnitudes_pass_through_the_power_of_two_scale(fmt, mag):
    """Pooled gradients far below fp16's smallest normal and far above 1 (the accumulated tensors start at the same magnitude):
    finite, and the same relative bounds."""
    g, _, _, _, w0, _ = C.inputs(C.SMALL, 1, 9, mag)
    g1, _, _, _, w1, _ = C.inputs(C.SMALL, 1, 9)
    assert torch.equal(g, g1 * mag) and torch.equal(w0, w1 * mag)
    _check_case(_trainer(C.SMALL, fmt), C.SMALL, fmt, 1, 9, patterns=("full",), mag=mag, label=" at |g| ~ %g" % mag)


@pytest.mark.parametrize("block,planned", [("1,3,3", (1, 3, 4)), ("1,7,7", (1, 7, 8))])
def test_odd_blocks_on_the_device(block, planned, monkeypatch):
    """VD_WG_BLOCK with an odd number of positions: the block grows by a column that the packed gradient masks with zeros."""
    geom, li, nb = C.G_C, 1, 9
    te = _trainer(geom, "f16x3")
    monkeypatch.setenv("VD_WG_BLOCK", block)
    kept = te._wg.pop((li, nb, False), None)          # (the engine keeps one program per (level, clips): plan this one afresh)
    try:
        assert tuple(te._wgrad(li, nb).plan.meta["box"]) == planned
        _check_case(te, geom, "f16x3", li, nb, label=", block %s" % (planned,))
    finally:
        te._wg.pop((li, nb, False), None)
        if kept is not None:
            te._wg[(li, nb, False)] = kept
