"""What tests/test_gpu_down_sweep.py rests on, checked without a device (tests/down_sweep_cases.py):

* every input-gradient plan an EmbedEngine / TrainEngine / GradMatchEngine can hold at the six clip sizes names every output element
  EXACTLY ONCE -- over the boxes and clip groups of a program and over the programs of a level.  A storing program does not care
  about an element named twice; the accumulating instantiation of the down sweep would count it twice;
* the checkers pass a perfect fp64 result and fail each of the ways a down-sweep level can be subtly wrong;
* the operand formats alone (fp64 arithmetic on the operands as held at the scales the engine would choose) stay below the bars for
  every case the GPU test runs -- where they did not, the case's inputs would be wrong for the bar;
* the integer cases are exact in fp32: every partial sum of absolute terms stays below 2^24 quanta."""
import numpy as np
import pytest
import torch

from tests import down_sweep_cases as D

_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)          # noqa: E731


# ---- exactly once ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", D.SIZES, ids=_IDS)
def test_every_input_gradient_plan_names_every_output_element_exactly_once(geom):
    seen, programs = set(), 0
    for batch_hint, small in ((None, True), (1, True), (None, False), (1, False)):
        bwd = D.bwd_plans(geom, batch_hint, small)
        assert len(bwd) == 3
        for li, plans in enumerate(bwd):
            key = (li,) + tuple(id(pl) for pl in plans)
            if key in seen:          # (the planner's cache hands the same plan objects to several variants)
                continue
            seen.add(key)
            ncl = max(pl.ncl for pl in plans)
            for nclips in sorted({1, 3, ncl + 1}):
                total, per = D.named_counts(plans, geom, li, nclips)
                for pl, cnt in zip(plans, per):
                    assert int(cnt.max()) == 1, "%s names an element %d times at %d clips" % (pl.name, int(cnt.max()), nclips)
                assert bool((total == 1).all()), "level %d of %s at %d clips (batch_hint %s, bwd0_small %s): %d elements unnamed, %d named more than once" % (
                    li, geom, nclips, batch_hint, small, int((total == 0).sum()), int((total > 1).sum()))
            programs += len(plans)
    assert programs >= 3
    if geom == D.G_B:
        assert [len(p) for p in D.bwd_plans(geom)] == [4, 4, 4]          # odd H and W: four parity-class pixel programs at level 0
    if geom in (D.G_A, D.SMALL):
        small, big = D.bwd_plans(geom, None, True)[0], D.bwd_plans(geom, None, False)[0]
        assert len(small) == 1 and small[0].MTW == 4 and small[0].nbox > big[0].nbox          # bwd0_small really is another plan


def test_the_count_sees_an_element_named_twice():
    import dataclasses
    pl = D.bwd_plans(D.G_B)[1][0]
    boxes = np.asarray(pl.boxes).copy()
    twice = dataclasses.replace(pl, boxes=np.concatenate([boxes, boxes[-1:]]))
    cin, _, t, h, w = D.layer_dims(D.G_B, 1)[:5]
    cnt = D.count_named(twice, 1, np.zeros(cin * t * h * w, dtype=np.int32))
    assert int(cnt.max()) == 2


# ---- the checkers can fail --------------------------------------------------------------------------------------------------------
def _fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fmt", ["f16x3", "bf16x3"])
def test_abar_checker_passes_the_fp64_result_and_fails_every_mutant(fmt):
    c = D.case(D.G_B, 0, 1)          # 65 x 63: the last row and the last column belong to one parity class each
    want = c.t1 + c.t2
    D.check_abar(want.clone(), c, fmt, "perfect")
    D.check_abar(want.float().double(), c, fmt, "perfect, rounded to fp32")
    h, w = want.shape[3:]
    shifted = want.clone()
    shifted[0, :, :, 1::2, 0::2] = torch.roll(want[0, :, :, 1::2, 0::2], 1, dims=-1)
    last_row, last_col = want.clone(), want.clone()
    last_row[:, :, :, h - 1, :] = c.t1[:, :, :, h - 1, :]
    last_col[:, :, :, :, w - 1] = c.t1[:, :, :, :, w - 1]
    mutants = {"second term missing": c.t1, "second term twice (equally: dvscale off by two)": c.t1 + 2 * c.t2,
               "zscale off by two": 2 * c.t1 + c.t2, "zscale off by a half": 0.5 * c.t1 + c.t2, "dvscale off by a half": c.t1 + 0.5 * c.t2,
               "one parity class of one clip shifted": shifted, "last row at the first launch's value": last_row,
               "last column at the first launch's value": last_col}
    for name, got in mutants.items():
        assert _fails(D.check_abar, got, c, fmt, name), name
    # a level above, several clips: one clip's second term missing
    c1 = D.case(D.G_B, 1, 3)
    got = (c1.t1 + c1.t2).clone()
    got[2] = c1.t1[2]
    D.check_abar(c1.t1 + c1.t2, c1, fmt, "perfect")
    assert _fails(D.check_abar, got, c1, fmt, "second term missing in the last clip")


def test_guard_and_unwritten_elements_are_seen():
    c = D.case(D.G_B, 0, 1)
    buf = D.abar_buffer(c.geom, 0, 1)
    buf[:1] = D.to_abar_layout((c.t1 + c.t2).float(), 0)
    assert torch.equal(D.written_abar(buf, 0, 1), (c.t1 + c.t2).float().double())
    bad = buf.clone()
    bad[1, 0, 0, 0, 0] = 0.0
    assert _fails(D.written_abar, bad, 0, 1), "a guard element written"
    bad = buf.clone()
    bad[0, 3, 2, 64, 62] = float("nan")
    assert _fails(D.written_abar, bad, 0, 1), "an element left unwritten"
    big = D.guarded(c.hb0, 16)
    assert torch.equal(D.written_front(big, c.hb0, "hv_b"), torch.zeros(c.hb0.shape, dtype=torch.float64))
    big[c.hb0.numel()] = 1.0
    assert _fails(D.written_front, big, c.hb0, "hv_b")


@pytest.mark.parametrize("fmt", ["f16x3", "bf16x3"])
def test_parameter_checkers_pass_the_fp64_result_and_fail_every_mutant(fmt):
    c = D.case(D.G_B, 1, 3)
    D.check_hv_w(c.w1 + c.w2, c, fmt, "perfect")
    D.check_hv_b(c.hb, c, "perfect")
    assert _fails(D.check_hv_w, c.w1, c, fmt, "the gbar x dz term missing")
    assert _fails(D.check_hv_w, c.w1 + 2 * c.w2, c, fmt, "gdscale off by two")
    assert _fails(D.check_hv_w, 0.5 * c.w1 + c.w2, c, fmt, "zscale off by a half")
    dz_sum = D.dense(c.g1, c.am, c.geom, c.li, c.layout).sum(dim=(0, 2, 3, 4))
    assert _fails(D.check_hv_b, dz_sum, c, "summed over dz instead of zb")
    # a slice that is zero in both terms must stay exactly zero: level 2 of a 4-frame size has taps that see only padding
    c2 = D.case(D.G_B, 2, 1)
    want = c2.w1 + c2.w2
    dead = torch.nonzero(want.reshape(-1, 147).norm(dim=0) == 0).flatten()
    assert dead.numel() > 0
    got = want.clone()
    got.view(-1, 147)[5, int(dead[0])] = 1e-30
    D.check_hv_w(want, c2, fmt, "perfect")
    assert _fails(D.check_hv_w, got, c2, fmt, "a padding-only tap not exactly zero")


# ---- the format floor against the bars ---------------------------------------------------------------------------------------------
def _floor_cases():
    seen = {}
    for geom, fmt, li, nb, _ in D.level_cases():
        seen.setdefault((geom, li, nb, "full", D.ONES), []).append(fmt)
    for geom, fmt, li, nb, pattern in D.pattern_cases():
        seen.setdefault((geom, li, nb, pattern, D.ONES), []).append(fmt)
    for geom, fmt, li, nb, mags in D.magnitude_cases():
        seen.setdefault((geom, li, nb, "full", mags), []).append(fmt)
    return [k + (tuple(sorted(set(v))),) for k, v in seen.items()]


@pytest.mark.parametrize("geom,li,nb,pattern,mags,fmts", _floor_cases(), ids=_IDS)
def test_format_floor_lies_below_the_bars(geom, li, nb, pattern, mags, fmts):
    c = D.case(geom, li, nb, pattern, mags)
    for fmt in fmts:
        ab, hw, hb = D.floor(c, fmt)
        print("floor %s %s level %d x %d clips %s %s: abar %s, hv_w %s, hv_b %.3f of their allowances" % (
            fmt, geom, li, nb, pattern, mags, ["%.3f" % v for v in ab], {k: "%.3f" % v[0] for k, v in hw.items()}, hb))
        assert max(ab) < 1.0, (fmt, ab)
        assert max(v[0] for v in hw.values()) < 1.0, (fmt, hw)
        assert hb < 1.0, (fmt, hb)


# ---- the integer cases ---------------------------------------------------------------------------------------------------------------
def _exact_cases():
    seen = {}
    for geom, fmt, li, nb in D.exact_cases():
        seen.setdefault((geom, li, nb), []).append(fmt)
    return [k + (tuple(v),) for k, v in seen.items()]


@pytest.mark.parametrize("geom,li,nb,fmts", _exact_cases(), ids=_IDS)
def test_integer_cases_are_exact_in_fp32_and_in_the_operand_formats(geom, li, nb, fmts):
    c = D.case(geom, li, nb, kind="exact")
    print("exact %s level %d x %d clips: partial sums of absolute terms below %s quanta (2^24 = %d)" % (
        geom, li, nb, ["%d" % b for b in c.partial_sum_bounds], 2 ** 24))
    assert D.is_exact_in_fp32(c), c.partial_sum_bounds
    assert bool(((c.t1 + c.t2) != 0).any()) and bool(((c.w1 + c.w2) != 0).any()) and bool((c.hb != 0).any())
    for fmt in fmts:          # every operand is held exactly at the engine's scales: the floor of an exact case is zero
        ab, hw, hb = D.floor(c, fmt)
        assert max(ab) == 0.0 and max(v[0] for v in hw.values()) == 0.0 and hb == 0.0, (fmt, ab, hw, hb)
