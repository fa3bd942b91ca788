"""CPU companion of tests/test_gpu_forward_level.py (no GPU): the data and the checker of tests/forward_level_cases.py themselves.

THE BOUNDS ARE ATTAINABLE.  For the small clip sizes, every level and every format: the fp64 conv of the operands as the format
holds them (hi, or hi + lo; f16x3 weights under their x 2^8 shift), with the output rounded to the level's output format, stays
within ONE QUARTER of the bound the GPU test uses -- rel-L2 whole and on the border shell, and the max-abs ratio within a quarter of
4 x the bound.  Worst floors over these cases (rel-L2 / shell / max-abs ratio), printed per case:
    f16x3   6.10e-08 / 6.10e-08 / 1.50e-07    bf16x3  3.02e-06 / 3.02e-06 / 6.87e-06
    f16     2.61e-04 / 2.61e-04 / 4.96e-04    bf16    2.08e-03 / 2.08e-03 / 4.10e-03
against bounds of 3.2e-6, 1.4e-5, 2e-3 and 2e-2: no bound had to be raised for its format's sake.  (f16 and bf16: two operand
roundings per product, and the output rounding of levels 0 and 1.)  The select epilogue likewise: f16x3 5.91e-08, bf16x3 3.54e-06
against 4.4e-6 and 1.8e-5.  The near-tie rule of the decisions at tie_tol = 2e-5 is attainable in hi+lo pairs only, which is
asserted too -- see forward_level_cases.format_reference.
THE PLANNER REACHES THE FAMILIES the GPU test asserts, at the clip sizes it uses (the same tables, without a device).
THE EXACT CASES ARE EXACT: the sum condition, a reference on the 2^-6 grid, ties, exact zeros, every conv position a winner.
THE CHECKER CATCHES WHAT IT IS FOR: the reference itself passes; with one deliberate corruption at a time it fails.
THE LAYOUT HELPERS ROUND-TRIP."""
import copy
from types import SimpleNamespace

import pytest
import torch

from tests import aux_oracle as AO
from tests import forward_level_cases as C

SIZES = (C.G_A, C.G_B, C.G_C, C.SMALL)
FORMATS = ("f16x3", "bf16x3", "f16", "bf16")
_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)          # noqa: E731


def _nb(li):
    return 3 if li == 0 else 2


@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom", SIZES, ids=_IDS)
def test_the_formats_alone_stay_within_a_quarter_of_the_bounds(geom, li):
    case = C.random_case(geom, li, _nb(li))
    for fmt in FORMATS:
        floor = C.format_floor(case, fmt)
        print("format floor %s level %d %s: rel-L2 %.2e, border shell %.2e, max-abs ratio %.2e | bound %.1e" % (
            fmt, li, geom, floor[0], floor[1], floor[2], C.BOUND[fmt]))
        assert floor[0] <= C.BOUND[fmt] / 4 and floor[1] <= C.BOUND[fmt] / 4 and floor[2] <= C.BOUND[fmt], (fmt, floor)
        assert floor[0] > 0 or fmt == "f16x3"


def test_the_near_tie_rule_is_attainable_in_hi_lo_pairs_only():
    """Exact arithmetic on the operands as the format holds them, decisions against the free fp64 reference at tie_tol = 2e-5 x rms:
    the hi+lo formats route no window otherwise that is no near-tie; the single-pass formats do, by their operand bits alone --
    which is why tests/test_gpu_forward_level.py states their near-tie rule against forward_level_cases.format_reference."""
    far = {fmt: 0 for fmt in FORMATS}
    worst = {fmt: 0.0 for fmt in FORMATS}
    for geom in SIZES:
        case = C.random_case(geom, 0, 3)
        for fmt in FORMATS:
            fr = C.format_reference(case, fmt)
            stats = C.compare_decisions(fr.idx, fr.dead, case.ref)
            far[fmt] += stats["not_near_tie"]
            worst[fmt] = max(worst[fmt], stats["worst_margin"])
            own = C.compare_decisions(fr.idx, fr.dead, fr)
            assert own["mismatch"] == 0
    print("windows of level 0 the format alone routes otherwise, no near-tie: %s, worst margin / rms %s" % (far, {k: "%.1e" % v for k, v in worst.items()}))
    assert far["f16x3"] == 0 and far["bf16x3"] == 0
    assert far["f16"] > 0 and far["bf16"] > far["f16"] and worst["f16"] > 10 * C.TIE_TOL and worst["bf16"] > 100 * C.TIE_TOL


def test_the_planner_reaches_the_families_of_the_gpu_test():
    """tests/test_gpu_forward_level.py::FAMILY / LATENCY / SELECT_FAMILY, planned as EmbedEngine and GradMatchEngine plan them."""
    from tests import test_gpu_forward_level as G
    from video_distillation_amd import plan as P
    fam = lambda pl: (pl.NTW, pl.MTW, pl.MW, pl.ncl, pl.nbox, len(pl.types))          # noqa: E731
    def forward_plan(geom, li, balanced, batch_hint=None):
        """Level 1 / 2 of the larger sizes as plan.plan_network chooses them, without planning their first level and input gradients
        (seconds each); the small sizes go through plan_network itself."""
        if geom not in (C.ODD, C.FULL):
            return P.plan_network(P.NetGeometry(*geom), ntw=2, ntw0=1, balanced=balanced, batch_hint=batch_hint)["fwd"][li]
        import dataclasses
        cin, cout, t, h, w = C.layer_dims(geom, li)[:5]
        make = lambda **kw: P.plan_forward_cl("fwd%d" % li, cin, cout, t, h, w, 2, feat_out=(li == 2), **kw)          # noqa: E731
        pl, pl2 = make(), make(ntw=2)
        if pl2.rows_total <= pl.rows_total:
            pl = pl2
        elif balanced and (pl.NT, pl.MW, pl.MTW) == (4, 1, 7) and all(t.mt == 7 for t in pl.types):
            pl = dataclasses.replace(pl, MW=2, MTW=3, NTW=2)
        return P.latency_variant(pl, batch_hint, lambda opts: make(mtw_options=opts))

    for (geom, li, x3), want in G.FAMILY.items():
        for hilo in ((False,) if x3 is None else (x3,)):          # (``balanced`` only matters where a 7-tile layout is in reach)
            assert fam(forward_plan(geom, li, not hilo)) == want, (geom, li, hilo, fam(forward_plan(geom, li, not hilo)), want)
    assert {li: fam(forward_plan(C.FULL, li, True, 8)) for li in (1, 2)} == G.LATENCY
    assert fam(forward_plan(C.FULL, 1, True)) == (2, 3, 2, 1, 14, 1) and fam(forward_plan(C.FULL, 1, False)) == (1, 7, 1, 1, 14, 1)
    for (geom, li), want in G.SELECT_FAMILY.items():
        cin, cout, t, h, w = C.layer_dims(geom, li)[:5]
        assert fam(P.plan_forward_cl("sel%d" % li, 2 * cin, cout, t, h, w, 2, feat_out=(li == 2))) == want, (geom, li)


def test_the_bounds_come_from_the_single_program_bars():
    """Never wider than what they started from."""
    for fmt in FORMATS:
        assert 0 < C.BOUND[fmt] <= C.BAR[fmt]
    for fmt in C.SELECT_BAR:
        assert 0 < C.SELECT_BOUND[fmt] <= C.SELECT_BAR[fmt]


@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom", SIZES, ids=_IDS)
def test_the_exact_cases_are_exact(geom, li):
    for nb in ((1, 3) if li == 0 else (1, 2)):
        case = C.exact_case(geom, li, nb)          # (asserts the sum condition, the grid, ties, zeros and the winners itself)
        ref = case.ref
        assert float(C.conv64(case.x.abs(), case.w.abs()).max()) * 64 < 2.0 ** 24
        for v in (case.z0, ref.value, case.b.double(), case.w.double(), case.x.double()):
            assert bool(((v * 64) == (v * 64).round()).all())
        for fmt in FORMATS:          # every operand survives every operand format, the x 2^8 weight shift included
            assert torch.equal(C.rounded(case.x, fmt), case.x.double())
            assert torch.equal(C.rounded(case.w, fmt, C.WSHIFT.get(fmt, 1.0)), case.w.double())
            assert bool(torch.isfinite((case.w * C.WSHIFT.get(fmt, 1.0)).to(AO.dtype16(C.PREC[fmt])).float()).all())
        assert bool((ref.margin == 0).any()) and bool(((ref.margin == 0) & ~ref.dead).any()), "no LIVE window with tied maxima"
        assert bool((ref.top == 0).any()) and bool(ref.dead[ref.top == 0].all())
        assert C.winners_cover_the_grid(ref)
        # the first-maximum rule is a rule: some tied window's first maximum is not its last
        tied = (ref.margin == 0) & ~ref.dead
        last = (ref.win == ref.top.unsqueeze(-1)).long().cumsum(-1).argmax(-1)
        assert bool((last[tied] != ref.idx[tied]).any())
        assert bool((ref.idx[tied] > 0).any()) or tied.sum() < 8


def test_random_cases_have_live_and_dead_windows_and_hide_no_position():
    for geom in SIZES:
        for li in range(3):
            ref = C.random_case(geom, li, _nb(li)).ref
            assert bool(ref.dead.any()) and bool((~ref.dead).any()) and C.winners_cover_the_grid(ref)
            if li > 0:
                x = C.random_case(geom, li, _nb(li)).x
                assert bool((x >= 0).all()) and 0.25 < float((x == 0).float().mean()) < 0.42


# --------------------------------------------------------------------------------------------------------- the checker
def _perfect(kind, geom, li, nb, fmt, with_argmax=True, planes=None):
    case = C.get_case(kind, geom, li, nb)
    return case, C.perfect_output(case, fmt, planes or C.planes_of(fmt), with_argmax)


def _check(kind, out, case, fmt):
    if kind == "exact":
        C.check_exact(out, case, fmt)
    else:
        C.check_random(out, case, fmt, C.BOUND[fmt])


def _slot_index(dims, b, c, t, h, w):
    """Element index of (clip, channel, pooled position) in the channels-last slots -> (slot, lane)"""
    cout, To, Ho, Wo = dims[1], dims[8], dims[9], dims[10]
    return (((b * (cout // 8) + c // 8) * To + t) * Ho + h) * Wo + w, c % 8


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("geom,li,fmt", [(C.G_A, 0, "f16x3"), (C.G_C, 1, "f16x3"), (C.SMALL, 1, "f16"), (C.SMALL, 2, "f16x3"), (C.G_B, 0, "bf16")],
                         ids=_IDS)
def test_the_reference_passes_its_own_checker(kind, geom, li, fmt):
    for with_argmax in (True, False):
        case, out = _perfect(kind, geom, li, _nb(li), fmt, with_argmax)
        _check(kind, out, case, fmt)
    if li == 1 and fmt == "f16":          # the emit_lo = 1 plane of a single-pass level 1
        case, out = _perfect(kind, geom, li, _nb(li), fmt, False, planes=2)
        assert out.planes.shape[0] == 2
        _check(kind, out, case, fmt)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("li", [0, 1, 2])
def test_one_border_element_off_by_one_weight_times_one_pixel(kind, li):
    geom, fmt = C.G_B, "f16x3"
    case, out = _perfect(kind, geom, li, _nb(li), fmt)
    dims = C.layer_dims(geom, li)
    delta = 1.0 / 64.0 if kind == "exact" else float(case.w.abs().mean())          # weight 1/64 x pixel 1; a typical weight x pixel 1
    b, c, t, h, w = _nb(li) - 1, 9, 0, dims[9] - 1, dims[10] - 1                  # last clip, last row and column: a border window
    v = case.ref.value.clone()
    v[b, c, t, h, w] += delta
    if li == 2:
        out.feat[:case.nb] = C.to_feat(v.float())
    else:
        s = C.to_slots(v.float(), fmt)
        out.planes[:, :s.shape[1]] = s
    with pytest.raises(AssertionError):
        _check(kind, out, case, fmt)


@pytest.mark.parametrize("fmt", ["bf16x3", "f16x3", "f16"])
def test_two_channels_of_one_slot_swapped_in_the_lo_plane_only(fmt):
    """Exact data: the hi planes stay what they are, so nothing but the bit-for-bit comparison of the LOW plane can see it (on
    random data the two values move by 2^-12 of themselves, inside any norm).  The exact level-1 case holds sums of some hundreds in
    two channels, whose fp16 image needs the low plane; for the single-pass format this is the emit_lo = 1 plane."""
    geom, li = C.SMALL, 1
    case, out = _perfect("exact", geom, li, 2, fmt, False, 2)
    C.check_exact(out, case, fmt)
    lo = out.planes[1, :out.planes.shape[1] * 2 // 3]
    cand = torch.nonzero((lo[:, 2] != lo[:, 3]) & (out.planes[0, :lo.shape[0], 2] != C.SENT16)).flatten()
    assert cand.numel() > 0, "no slot whose third and fourth low parts differ"
    s = int(cand[cand.numel() // 2])
    a, b = int(out.planes[1, s, 2]), int(out.planes[1, s, 3])
    out.planes[1, s, 2], out.planes[1, s, 3] = b, a
    with pytest.raises(AssertionError, match="lo plane"):
        C.check_exact(out, case, fmt)


def _byte_view(out, case):
    dims = C.layer_dims(case.geom, case.li)
    return dims, (lambda b, c, t, h, w: (((b * dims[1] + c) * dims[8] + t) * dims[9] + h) * dims[10] + w) if case.li == 2 else \
        (lambda b, c, t, h, w: _slot_index(dims, b, c, t, h, w)[0] * 8 + c % 8)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("li", [0, 1, 2])
def test_one_live_argmax_byte_moved_to_a_non_tied_position(kind, li):
    geom, fmt = C.G_A, "f16x3"
    case, out = _perfect(kind, geom, li, _nb(li), fmt)
    ref = case.ref
    dims, at = _byte_view(out, case)
    clear = (~ref.dead) & (ref.margin / ref.rms > 1e-2)
    b, c, t, h, w = torch.nonzero(clear)[int(clear.sum()) // 2].tolist()
    i = at(b, c, t, h, w)
    assert int(out.am[i]) == int(ref.idx[b, c, t, h, w])
    out.am[i] = (int(out.am[i]) + 1) % ref.win.shape[-1]
    with pytest.raises(AssertionError):
        _check(kind, out, case, fmt)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dead_before", [False, True])
def test_one_dead_flag_flipped_on_a_window_with_a_clear_margin(kind, dead_before):
    geom, li, fmt = C.G_C, 1, "f16x3"
    case, out = _perfect(kind, geom, li, 2, fmt)
    ref = case.ref
    dims, at = _byte_view(out, case)
    clear = (ref.dead == dead_before) & (ref.top.abs() / ref.rms > 1e-2)
    b, c, t, h, w = torch.nonzero(clear)[int(clear.sum()) // 2].tolist()
    i = at(b, c, t, h, w)
    assert bool(out.am[i] & 0x80) == dead_before
    out.am[i] = int(out.am[i]) ^ 0x80
    with pytest.raises(AssertionError):
        _check(kind, out, case, fmt)


@pytest.mark.parametrize("li,fmt", [(0, "f16"), (1, "bf16x3"), (2, "f16x3")])
def test_one_owned_element_left_at_the_sentinel_and_one_guard_element_written(li, fmt):
    geom = C.G_B
    case, good = _perfect("exact", geom, li, _nb(li), fmt)
    dims = C.layer_dims(geom, li)
    n = dims[1] * dims[8] * dims[9] * dims[10]
    C.check_written(good, dims, li, case.nb)

    def corrupt(fn, match):
        out = copy.deepcopy(good)
        fn(out)
        with pytest.raises(AssertionError, match=match):
            C.check_written(out, dims, li, case.nb)
        with pytest.raises(AssertionError):
            C.check_exact(out, case, fmt)

    def set_value(t, i, v):
        t.view(-1)[i] = v

    if li == 2:
        corrupt(lambda o: set_value(o.feat, case.nb * n - 1, float("nan")), "unwritten")
        corrupt(lambda o: set_value(o.feat, case.nb * n, 0.0), "behind")
    else:
        last_plane = good.planes.shape[0] - 1
        corrupt(lambda o: set_value(o.planes[last_plane], case.nb * n - 1, C.SENT16), "unwritten")          # the LAST owned element of the last plane
        corrupt(lambda o: set_value(o.planes[0], 17, C.SENT16), "unwritten")
        corrupt(lambda o: set_value(o.planes[last_plane], case.nb * n, 0), "behind")                      # the FIRST guard element
    corrupt(lambda o: set_value(o.am, case.nb * n - 1, C.SENT_AM), "arg-max bytes unwritten")
    corrupt(lambda o: set_value(o.am, case.nb * n, 0), "behind")
    corrupt(lambda o: set_value(o.am, 5, int(o.am[5]) | 0x08), "bits outside")
    if dims[11] == 1:
        corrupt(lambda o: set_value(o.am, 5, int(o.am[5]) | 0x04), "bits outside")          # no frame bit where the level does not pool frames


# ------------------------------------------------------------------------------------------------------ layout helpers
@pytest.mark.parametrize("fmt", FORMATS)
def test_layout_helpers_round_trip(fmt):
    gen = torch.Generator().manual_seed(3)
    nb, Cc, t, h, w = 3, 24, 2, 5, 3
    x = torch.randn(nb, Cc, t, h, w, generator=gen)
    s = C.to_slots(x, fmt)
    assert s.shape == (C.planes_of(fmt), nb * 3 * t * h * w, 8) and s.dtype == torch.int16
    # slot order [clip][C/8][t][h][w][8]: element (b, c, t, h, w) by index arithmetic
    hi = AO.split16(x, C.PREC[fmt])[0]
    for (b, c, tt, hh, ww) in ((0, 0, 0, 0, 0), (2, 23, 1, 4, 2), (1, 9, 1, 0, 2)):
        slot = (((b * 3 + c // 8) * t + tt) * h + hh) * w + ww
        assert int(s[0, slot, c % 8]) == int(hi[b, c, tt, hh, ww])
    back = C.from_slots(s, nb, Cc, t, h, w)
    assert torch.equal(back[0], hi) and torch.equal(C.decode(back, fmt), C.rounded(x, fmt))
    assert torch.equal(C.from_slots(s, 2, Cc, t, h, w), back[:, :2])          # the first clips of a larger buffer
    a = torch.randint(0, 256, (nb, Cc, t, h, w), generator=gen).to(torch.uint8)
    assert torch.equal(C.from_slots(C.bytes_to_slots(a), nb, Cc, t, h, w), a)
    f = C.to_feat(x)
    assert f.shape == (nb, Cc * t * h * w) and float(f[1, ((7 * t + 1) * h + 2) * w + 1]) == float(x[1, 7, 1, 2, 1])
    assert torch.equal(C.from_feat(f, nb, Cc, t, h, w), x)


def test_layout_helpers_agree_with_the_projects_own():
    """to_slots is tests/test_gpu_wgrad.py::_slots_from_dense, the byte order is tests/argmax_tools.py::decode_argmax's, window
    elements are enumerated as tests/argmax_tools.py::oracle_windows does."""
    from tests import argmax_tools as A
    from tests.test_gpu_wgrad import _slots_from_dense
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 2, 3, 5, generator=gen)
    for fmt in ("f16x3", "bf16x3", "f16"):
        assert torch.equal(C.to_slots(x, fmt).reshape(-1), _slots_from_dense(x, fmt, C.planes_of(fmt)).reshape(-1))
    a = torch.randint(0, 8, (2, 16, 2, 3, 5), generator=gen).to(torch.uint8)
    a[0, 3, 1, 2, 4] |= 0x80
    pos, dead = A.decode_argmax(C.bytes_to_slots(a), 2, 16, 2, 3, 5, feat_layout=False)
    assert torch.equal(pos, (a & 7).long()) and torch.equal(dead, (a & 0x80) != 0)
    z = torch.randn(2, 8, 5, 7, 6, generator=gen).double()
    for pt in (1, 2):
        arg, margin, top1 = A.oracle_windows(z, pt)
        ref = C.reference(z, torch.zeros(8), pt)
        assert torch.equal(arg, ref.idx) and torch.equal(top1, ref.top) and torch.equal(margin, ref.margin)


# ------------------------------------------------------------------------------------------------------ the select epilogue
@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom", [C.SMALL, C.G_B], ids=_IDS)
def test_select_cases(geom, li):
    """The exact select case is exact (select_case asserts the doubled sum bound and the grid), its reference passes the checker in
    every output mode, one element off by 2^-8 (one weight x one pixel x the scale) or one dead window not zero fails it; the
    formats alone stay within a quarter of the select bounds."""
    nb = 2
    for fmt, mode in (("f16x3", "feat" if li == 2 else "f32"), ("bf16x3", "feat" if li == 2 else "planes")):
        exact = C.select_case(geom, li, nb, "exact")
        assert bool(((exact.value * 256) == (exact.value * 256).round()).all())
        good = C.perfect_select(exact, fmt, mode)
        C.check_select(good, exact, fmt, mode)
        dead = (exact.am & 0x80) != 0
        for pick, delta in ((torch.nonzero(~dead)[7], 2.0 ** -8), (torch.nonzero(dead)[3], 2.0 ** -8)):
            v = exact.value.clone()
            v[tuple(pick.tolist())] += delta
            bad = C.perfect_select(SimpleNamespace(**{**vars(exact), "value": v}), fmt, mode)
            with pytest.raises(AssertionError):
                C.check_select(bad, exact, fmt, mode)
        flat = good.clone()
        flat.view(-1)[-1] = 0          # a guard element written
        with pytest.raises(AssertionError, match="behind"):
            C.check_select(flat, exact, fmt, mode)
        rand = C.select_case(geom, li, nb, "random")
        C.check_select(C.perfect_select(rand, fmt, mode), rand, fmt, mode, C.SELECT_BOUND[fmt])
        floor = C.select_floor(rand, fmt, mode)
        print("select format floor %s level %d %s: %s | bound %.1e" % (fmt, li, geom, ["%.2e" % v for v in floor], C.SELECT_BOUND[fmt]))
        assert floor[0] <= C.SELECT_BOUND[fmt] / 4 and floor[1] <= C.SELECT_BOUND[fmt] / 4 and floor[2] <= C.SELECT_BOUND[fmt]
