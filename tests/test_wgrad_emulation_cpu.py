"""The weight-gradient tile program (plan.plan_wgrad) on the CPU, before anything is launched on a GPU.

(1) tests/emulate.py::run_wgrad_plan interprets the program from the device's own tables -- row origins, position offsets, the
    gather table, the packed-dy layout, the accumulation copy of every box -- in fp64 and must equal fp64 autograd of F.conv3d
    with respect to the weight: max-abs error over max-abs reference below 1e-12.  fp64 against fp64: a dW element is a sum of at
    most ~1e5 products of O(1) values, each summation order is within ~n u of the exact sum relative to the sum of absolute
    terms, and u = 1.1e-16 -- 1e-12 leaves two orders of magnitude over that and is eleven orders below one misplaced term.
    All three levels of 64 x 66 x 4, 65 x 63 x 4, 70 x 58 x 4 (ragged last boxes, conv rows / columns no pool window covers) and
    64 x 64 x 8, with 1, 8 and 9 clips (one clip chunk, a full one, a second one holding one clip), atomic and ordered plans; and
    the explicit blocks (1,3,3) and (1,7,7), which take the odd-count branch of ``_plan_wgrad`` (an extra masked column).
(2) Structure at every size the GPU test launches: every conv position in exactly one (box, step position), positions outside
    the grid packed as zero, the patch within the LDS budget, one accumulation copy per box in ordered plans.
(3) What the operand FORMATS alone cost (tests/param_gradient_cases.py): both operands of every case of
    tests/test_gpu_param_gradient.py rounded as the format rounds them, everything accumulated in fp64, the same slice families and
    input patterns -- the bars of that test must leave a factor of four over these floors, or they would be testing the format
    and not the kernels.  Worst floors, whole / per tap / per output channel / per input channel (the three patterns agree to two
    digits): f16x3 7.2e-8 / 9.2e-8 / 1.3e-6 / 9.2e-8, bf16x3 3.6e-6 / 4.3e-6 / 6.5e-6 / 4.4e-6, f16 3.0e-4 / 3.8e-4 / 4.9e-4 / 3.7e-4
    against bars of 2e-5, 1e-4 and 2e-3; the per-output-channel worst is level 2 with one clip (a slice of one pool window)."""
import numpy as np
import pytest
import torch

from tests import emulate as E
from tests import param_gradient_cases as C
from tests.test_gpu_input_gradient import _dense_gradient
from video_distillation_amd import plan as P

SMALL_SIZES = (C.G_A, C.G_B, C.G_C, C.SMALL)
LDS_BUDGET = 3700                    # plan_wgrad's default, the one engine.WgradOp plans with
_REF = {}


def _level(geom, li, nclips):
    """Random source and dense gradient of one level and the fp64 weight gradient (shared by the atomic and the ordered plan)."""
    key = (geom, li, nclips)
    if key not in _REF:
        cin, cout, t, h, w, T, OH, OW = P.NetGeometry(*geom).layer_dims()[li][:8]
        gen = torch.Generator().manual_seed(31 * li + nclips + sum(geom))
        x = torch.randn(nclips, cin, t, h, w, generator=gen, dtype=torch.float64)
        dy = torch.randn(nclips, cout, T, OH, OW, generator=gen, dtype=torch.float64)
        _REF[key] = (x, dy, C.weight_gradient(x, dy))
    return _REF[key]


def _plan(geom, li, nclips, ordered=False, block=None):
    cin, cout, t, h, w = P.NetGeometry(*geom).layer_dims()[li][:5]
    return P.plan_wgrad("wgrad%dx%d" % (cin, cout), cin, cout, t, h, w, nclips, block=block, ordered=ordered)


def _assert_equal_to_autograd(pl, geom, li, nclips):
    x, dy, want = _level(geom, li, nclips)
    got = E.run_wgrad_plan(pl, x.numpy(), dy.numpy(), nclips)
    err = float(np.abs(got - want.numpy()).max() / want.abs().max())
    print("%s %s level %d, %d clips, box %s, %d boxes, %d copies: max-abs error / max-abs reference %.1e"
          % (pl.name, geom, li, nclips, pl.meta["box"], pl.nbox, pl.meta["replicas"], err))
    assert err < 1e-12


@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("nclips", [1, 8, 9])
@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom", SMALL_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_weight_gradient_program_equals_fp64_autograd(geom, li, nclips, ordered):
    pl = _plan(geom, li, nclips, ordered)
    if ordered:
        assert pl.meta["replicas"] == pl.nbox and sorted(int(b[5]) for b in pl.boxes) == list(range(pl.nbox))
    _assert_equal_to_autograd(pl, geom, li, nclips)


@pytest.mark.parametrize("block,now", [((1, 3, 3), 4), ((1, 7, 7), 8)])
def test_odd_blocks_get_a_masked_extra_column(block, now):
    """An odd number of positions per block: K steps take position pairs, so the block grows by one column whose dy is zero."""
    pl = _plan(C.G_C, 1, 9, block=block)
    assert pl.meta["box"][2] == now and tuple(pl.meta["box"][:2]) == block[:2]
    _assert_equal_to_autograd(pl, C.G_C, 1, 9)


def _step_positions(pl):
    """(t, oh, ow) of every (box, step position) from the tables alone: box origin (t0 - 1, 2 oh0 - 3, 2 ow0 - 3) in source slots,
    step offset dt * pitch_f + 2 doh * pitch_h + 2 dow in patch slots.  -> int array [nbox, 2 S, 3]"""
    bt = pl.types[0]
    off = bt.tap_off.astype(np.int64) // P.SLOT_BYTES
    dt, r = np.divmod(off, bt.pitch_f)
    dh2, dw2 = np.divmod(r, bt.pitch_h)
    assert not (dh2 % 2).any() and not (dw2 % 2).any() and (dw2 < bt.pw).all() and (dh2 < bt.ph).all() and (dt < bt.pf).all()
    b = pl.boxes.astype(np.int64)
    assert not ((b[:, 2] + 3) % 2).any() and not ((b[:, 3] + 3) % 2).any()
    t0, oh0, ow0 = b[:, 1] + 1, (b[:, 2] + 3) // 2, (b[:, 3] + 3) // 2
    return np.stack([t0[:, None] + dt[None, :], oh0[:, None] + dh2[None, :] // 2, ow0[:, None] + dw2[None, :] // 2], axis=-1)


@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom,nclips", [(C.G_A, 9), (C.G_B, 3), (C.G_C, 9), (C.SMALL, 17), (C.ODD, 2), (C.FULL, 2)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_structure_of_the_weight_gradient_program(geom, nclips, li, ordered):
    pl = _plan(geom, li, nclips, ordered)
    cin, cout, t, h, w, T, OH, OW = P.NetGeometry(*geom).layer_dims()[li][:8]
    assert tuple(pl.meta["grid"]) == (T, OH, OW) and pl.CC == -(-nclips // 8) and len(pl.types) == 1
    bt = pl.types[0]
    assert bt.pitch_c <= LDS_BUDGET and pl.gather_table().shape[1] >= bt.pitch_c
    if ordered:
        assert pl.meta["replicas"] == pl.nbox and (pl.boxes[:, 5] == np.arange(pl.nbox)).all()
    else:
        assert 1 <= pl.meta["replicas"] <= 16 and (pl.boxes[:, 5] >= 0).all() and (pl.boxes[:, 5] < pl.meta["replicas"]).all()
    pos = _step_positions(pl)                                            # [nbox, 2S, 3]
    inside = (pos[..., 0] < T) & (pos[..., 1] < OH) & (pos[..., 2] < OW) & (pos >= 0).all(axis=-1)
    lin = (pos[..., 0] * OH + pos[..., 1]) * OW + pos[..., 2]
    count = np.bincount(lin[inside], minlength=T * OH * OW)
    assert count.size == T * OH * OW and (count == 1).all(), "conv positions covered %d..%d times" % (count.min(), count.max())
    # the packed dy: clip 0 / output channel 0 of every (box, step position) names exactly that position, all else follows from it
    idx = P.wgrad_pack_index(pl)                                         # [nbox, CCb, S, NT, 64, 8]
    first = idx[:, 0, :, 0, :, 0][:, :, [0, 32]].reshape(pl.nbox, 2 * pl.S)
    assert (first[~inside] == -1).all(), "a position outside the grid is packed from dy"
    assert (first[inside] == lin[inside] * cout).all()
    out = idx.reshape(pl.nbox, pl.CC, pl.S, pl.NT, 2, 32, 8).transpose(0, 2, 4, 1, 3, 5, 6).reshape(pl.nbox, 2 * pl.S, pl.CC, pl.NT, 32, 8)
    assert (out[~inside] == -1).all()
    clip = (np.arange(pl.CC)[:, None, None, None] * 8 + np.arange(8)[None, None, None, :])
    n = np.arange(pl.NT)[None, :, None, None] * 32 + np.arange(32)[None, None, :, None]
    want = np.where(clip < nclips, (clip * T * OH * OW + lin[inside][:, None, None, None, None]) * cout + n, -1)
    assert (out[inside] == want).all()


# ---- (3) the floors of the operand formats -------------------------------------------------------------------------------------------
def _floor_cases():
    seen, out = set(), []
    for geom, fmt, li, nb in C.level_cases():
        if (geom, li, nb) not in seen:
            seen.add((geom, li, nb))
            out.append((geom, li, nb, tuple(f for g, f, l, n in C.level_cases() if (g, l, n) == (geom, li, nb))))
    return out


FLOOR = {}          # (format, family, pattern) -> worst simulated rel-L2 so far


@pytest.mark.parametrize("geom,li,nb,fmts", _floor_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bars_leave_four_times_the_rounding_of_the_operands(geom, li, nb, fmts):
    """Both operands rounded as the format rounds them (hi, or hi + lo), products and sums in fp64: the rel-L2 of every slice
    family, for every input pattern, must be at most a quarter of the bar the device is held to."""
    dims = C.layer_dims(geom, li)
    for name in C.PATTERNS:
        g, am, layout, x, _, _ = C.pattern(geom, li, nb, name)
        want = C.reference(geom, li, nb, name)[0]
        for fmt in fmts:
            dy = _dense_gradient(C.rounded(g, fmt), am, dims, layout)          # (fp64 in, fp64 out: .double() keeps it)
            got = C.weight_gradient(C.rounded(x, fmt), dy)
            worst, zeros = C.slice_errors(got, want)
            if name == "full":
                assert zeros["tap"] == C.padding_only_taps(geom, li), (zeros, C.padding_only_taps(geom, li))
            for fam, (v, i) in worst.items():
                key = (fmt, fam, name)
                FLOOR[key] = max(FLOOR.get(key, 0.0), v)
                assert 4 * v <= C.BAR[fmt], "%s level %d x %d clips, %s / %s / %s: floor %.2e at slice %d, bar %.0e" % (
                    geom, li, nb, fmt, fam, name, v, i, C.BAR[fmt])
    print("floors so far, worst pattern, per format (%s): %s" % (" / ".join(C.FAMILIES), {f: " / ".join(
        "%.1e" % max(v for k, v in FLOOR.items() if k[:2] == (f, fam)) for fam in C.FAMILIES) for f in sorted({k[0] for k in FLOOR})}))

