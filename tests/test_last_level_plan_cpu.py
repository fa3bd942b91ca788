"""Which program the real side's LAST level runs (plan.plan_last_level), per geometry, form ("x3": fp16 hi+lo pairs, "c8": the
corrections on the fp8 matrix instruction) and ``VD_C8_POS`` -- the choice ``EmbedEngine(last_hilo=...)`` uploads, the ``ValueError``
``distill.HipBackend`` answers by falling back from "c8" to "x3", and the row-major program ``tests/test_gpu_c8.py`` compares the
position tiles against.  Planned as a single-pass f16 engine plans (``plan_network(geo, ntw=2, ntw0=1, balanced=True)``); no device."""
import copy

import pytest

from video_distillation_amd import plan as P

# what is asserted of a planned program: (epi, NTW, MTW, ncl, S); None = ValueError; "base" = the single-pass program's own shape
X3_BASE = "base"
CASES = {
    # geometry: (single-pass base (NTW, MTW, ncl), x3, c8, c8 with VD_C8_POS=0)
    (8, 64, 64): ((1, 2, 4), X3_BASE, (P.EPI_POS_FEAT, 1, 4, 8, 72), None),
    (16, 112, 112): ((2, 4, 2), (P.EPI_POOL_FEAT, 1, 4, 1, 74), (P.EPI_POS_FEAT, 1, 4, 4, 56), (P.EPI_POOL_FEAT, 1, 4, 1, 76)),
    (8, 80, 96): (None, X3_BASE, (P.EPI_POS_FEAT, 1, 4, 8, 64), None),
    (8, 112, 112): (None, X3_BASE, (P.EPI_POS_FEAT, 1, 4, 8, 56), None),
    (12, 96, 80): (None, X3_BASE, None, None),
    (6, 64, 64): (None, X3_BASE, None, None),
    (10, 48, 48): (None, X3_BASE, None, None),
}


def _shape(pl):
    return (pl.epi, pl.NTW, pl.MTW, pl.ncl, pl.S)


def _snapshot(pl):
    return (pl.name, _shape(pl), [t.tap_off.copy() for t in pl.types], copy.deepcopy(pl.meta))


def _same(a, b):
    return a[:2] == b[:2] and a[3] == b[3] and len(a[2]) == len(b[2]) and all((x == y).all() and x.shape == y.shape for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("geom", sorted(CASES))
def test_last_level_program_per_geometry_form_and_switch(monkeypatch, geom):
    base_shape, x3, c8, c8_rows = CASES[geom]
    net = P.plan_network(P.NetGeometry(*geom), ntw=2, ntw0=1, balanced=True)
    dims, base = net["dims"], net["fwd"][2]
    assert base.name == "fwd2" and base.epi == P.EPI_POOL_FEAT and base.S == 74
    if base_shape is not None:
        assert (base.NTW, base.MTW, base.ncl) == base_shape
    before = _snapshot(base)

    monkeypatch.delenv("VD_C8_POS", raising=False)
    got = P.plan_last_level(dims, base, "x3", "f16")
    assert got.name == "fwd2_hilo"
    assert _shape(got) == (_shape(base) if x3 == X3_BASE else x3)
    if x3 == X3_BASE:          # the base program itself under its new name: same tables, same operand gather
        assert got.types is base.types and got.widx is base.widx
    else:                      # the one-clip alternative replaces a two-clip 4 x 2-tile base
        assert (base.NTW, base.MTW, base.ncl) == (2, 4, 2) and got.rows_total <= base.rows_total
        assert 2 * got.gather_table().shape[1] * 16 <= 72 * 1024
    assert all(t.tap_off.size == 2 * got.S for t in got.types)          # no skip table in a hi+lo pair program

    for switch, want in ((None, c8), ("1", c8), ("0", c8_rows)):
        if switch is None:
            monkeypatch.delenv("VD_C8_POS", raising=False)
        else:
            monkeypatch.setenv("VD_C8_POS", switch)
        if want is None:
            with pytest.raises(ValueError, match="last_hilo='c8' needs the f16 format and either position tiles"):
                P.plan_last_level(dims, base, "c8", "f16")
            continue
        got = P.plan_last_level(dims, base, "c8", "f16")
        assert got.name == "fwd2_c8" and _shape(got) == want
        assert got.S % 4 == 0
        assert all(t.tap_off.size == 2 * got.S + got.S // 4 for t in got.types)      # tap offsets, then the tile skip masks
        if got.epi == P.EPI_POS_FEAT:
            assert got.w_box_stride > 0 and got.ncl == 32 // dims[2][5]          # rows = (clip, frame) pairs: 32 / frames clips per box
        else:                                                            # row-major: skips nothing, one shared operand set
            assert got.w_box_stride == 0 and all(not t.tap_off[2 * got.S:].any() for t in got.types)

    with pytest.raises(ValueError):          # the fp8-corrected form is an f16 program, whatever the switch says
        P.plan_last_level(dims, base, "c8", "bf16")
    monkeypatch.delenv("VD_C8_POS", raising=False)
    with pytest.raises(ValueError):
        P.plan_last_level(dims, base, "c8", "bf16")
    assert P.plan_last_level(dims, base, "x3", "bf16").name == "fwd2_hilo"

    assert _same(_snapshot(base), before), "plan_last_level changed the single-pass program it was given"
    assert net["fwd"][2] is base and base.name == "fwd2"


def test_row_major_c8_program_does_not_touch_the_planner_s_shared_program(monkeypatch):
    """The row-major fp8-corrected program is the one-clip 4 x 1-tile program plus a skip table; that program comes out of the
    planner's per-process cache, where the hi+lo form of the NEXT engine finds it again: the table goes into a copy."""
    geom = (16, 112, 112)
    net = P.plan_network(P.NetGeometry(*geom), ntw=2, ntw0=1, balanced=True)
    dims, base = net["dims"], net["fwd"][2]
    d2 = dims[2]
    shared = P.plan_forward_cl("fwd2", d2[0], d2[1], d2[2], d2[3], d2[4], d2[11], feat_out=True, ntw=1, mtw_options=(4,), step_multiple=4)
    sizes = [t.tap_off.size for t in shared.types]
    assert sizes == [2 * shared.S] * len(shared.types)
    monkeypatch.setenv("VD_C8_POS", "0")
    got = P.plan_last_level(dims, base, "c8", "f16")
    assert got.S == shared.S and [t.tap_off.size for t in got.types] == [2 * got.S + got.S // 4] * len(got.types)
    assert [t.tap_off.size for t in shared.types] == sizes and shared.name == "fwd2"
