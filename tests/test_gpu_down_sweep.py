"""The downward sweep of the second-order pass -- ``train.GradMatchEngine._down_sweep`` -- checked where nothing can excuse an error.

(B) ONE LEVEL, NOTHING DECIDED.  ``GradMatchEngine.down_level`` with the state filled exactly as the sweeps before it fill it, by the
    engine's own helpers: ``_pack_adjoint`` (V_l at its power-of-two scale, the storing and the accumulating programs' operands),
    ``level_unpool`` of a random pooled first-order gradient (dz_l and ``gscale``), the tangent gbar_l through ``_absmax_scale`` /
    ``_combine(.., 1)`` / vd_split_scaled as ``_up_sweep`` does, the source slots of a_l.  Random arg-max bytes (ReLU-dead windows
    among them) are an INPUT.  abar_l goes into a NaN-filled allocation with a guard clip behind it, hv_w / hv_b into the fronts of
    NaN-filled allocations that start from seeded values.  Reference, bars and checkers: tests/down_sweep_cases.py -- fp64 by index
    arithmetic and autograd of F.conv3d, per clip and input parity class, whole and on the border shell, four slice families of the
    weight adjoint.  The bars are DERIVED there (a single program's bound per term, one fp32 add), not measured here.
    Exact, without any tolerance: V = 0 leaves what the storing launch wrote; a zero incoming adjoint makes the accumulating launch
    the storing one, bit for bit; integer data equals fp64; the four accumulating pixel programs of an odd clip size give the same
    bits in one launch and in four.  The program families are asserted per (size, level, batch_hint) (PLANNED), and the engine's
    plans are the ones tests/test_down_sweep_cpu.py counted on the host.
(C) THE CONV LEVELS' WHOLE SECOND-ORDER PASS ON THE RECORDED DECISIONS: ``ag_feat_forward`` / ``ag_feat_backward(keep=True)`` /
    ``ag_feat_second_order`` against the fp64 double backward through tests/argmax_tools.py::routed_feature_layers, routed by the
    arg-max bytes the forward recorded.  No clip is exempt as a flip; every window the fp64 values would route otherwise must be a
    near-tie.  Adjoints of g_feat and x per clip, the six parameter adjoints per tensor.

Bars of (C): started from those of the free comparisons (2e-4 for the vjp, 1e-4 "tight" for gradients); a bar stays where the
measured worst is within ten times of it, otherwise it is four times the measured worst (kernels deterministic up to the atomics'
order, inputs seeded).

MEASURED on an MI355X, worst over all cases of this file (sparse patterns, magnitudes 1e-7 / 1e4 and batch_hint = 1 included).
(B) abar: error over ||t1|| + ||t2|| per clip and parity class (compares with B), then error over allowance whole / shell / max-abs:
    f16x3   level 0  5.30e-07 (B = 2.4e-6)  0.215 / 0.185 / 0.187    level 1  5.57e-07  0.226 / 0.206 / 0.195    level 2  3.69e-07  0.151 / 0.146 / 0.104
    bf16x3  level 0  3.27e-06 (B = 2.0e-5)  0.163 / 0.162 / 0.073    level 1  3.35e-06  0.167 / 0.168 / 0.078    level 2  3.40e-06  0.169 / 0.169 / 0.075
    hv_w: rel-L2 whole / per tap / per cout / per cin (bars 2e-5 / 1e-4), worst error over allowance of any family:
    f16x3   level 0  3.34e-07 / 4.02e-07 / 3.66e-07 / 3.35e-07  0.020    level 1  2.10e-07 / 2.24e-07 / 2.42e-07 / 2.14e-07  0.010
            level 2  1.14e-07 / 1.30e-07 / 1.72e-07 / 1.22e-07  0.008
    bf16x3  level 0  4.46e-06 / 5.53e-06 / 5.26e-06 / 4.51e-06  0.055    level 1  4.50e-06 / 4.66e-06 / 5.63e-06 / 4.59e-06  0.040
            level 2  4.41e-06 / 5.62e-06 / 8.47e-06 / 5.03e-06  0.078
    hv_b: the worst |error| is 0.007 of its bound.  The format floors (tests/test_down_sweep_cpu.py) are at most 0.022 of an allowance.
    The derived bars are NOT tightened here.  The four exact checks hold without tolerance in every case.
(C) against the routed fp64 oracle, no window routed otherwise at any level in any case:
                adjoint of g_feat (per clip)   adjoint of x (per clip)   parameter adjoints (per tensor)
    f16x3       1.84e-06                       8.14e-07                  1.70e-06 (w2; w0 6.8e-07, w1 5.1e-07, biases below)
       -> 1e-4 was 54 x: 7.4e-6            -> 2e-4 was 246 x: 3.3e-6   -> 1e-4 was 59 x: 6.8e-6
    bf16x3      5.89e-06                       7.85e-06                  7.77e-06
       -> 1e-4 was 17 x: 2.4e-5            -> 2e-4 was 25 x: 3.2e-5    -> 1e-4 was 13 x: 3.2e-5
    (b2's adjoint is identically zero in the reference -- the features are affine in b2 -- and exactly zero on the device.)
Run time of this file on an MI355X host: 120 cases in 45 s, the slowest 0.9 s (for the record; the fp64 references are most of it)."""
import functools

import pytest
import torch

from oracle import ref_cpu as R
from tests import argmax_tools as A
from tests import down_sweep_cases as D

pytestmark = pytest.mark.gpu

_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)          # noqa: E731
WORST_ABAR = {}          # (format, level) -> [error / (|t1| + |t2|), error / allowance whole, shell, max-abs]
WORST_HVW = {}           # (format, level) -> {family: rel-L2}
WORST = {}               # (C): (format, quantity) -> worst relative error
_MATCHERS = {}

# (clip size, level, batch_hint) -> per program (MTW, NT, MW, clips per box, boxes) of GradMatchEngine.bwdV[level] (= eng.bwd[level]'s plans)
PLANNED = {
    (D.G_A, 0, None): [(4, 1, 4, 1, 9)], (D.G_A, 1, None): [(8, 2, 2, 2, 1)] * 4, (D.G_A, 2, None): [(8, 4, 1, 32, 1)] * 4,
    (D.G_B, 0, None): [(2, 1, 4, 1, 17), (2, 1, 4, 1, 17), (8, 1, 4, 1, 4), (8, 1, 4, 1, 4)],
    (D.G_B, 1, None): [(8, 2, 2, 2, 1)] * 4, (D.G_B, 2, None): [(8, 4, 1, 32, 1)] * 4,
    (D.G_C, 0, None): [(4, 1, 4, 1, 9)], (D.G_C, 1, None): [(8, 2, 2, 2, 1), (8, 2, 2, 2, 1), (7, 2, 2, 2, 1), (7, 2, 2, 2, 1)],
    (D.G_C, 2, None): [(8, 4, 1, 32, 1), (4, 4, 1, 64, 2), (8, 4, 1, 32, 1), (2, 4, 1, 64, 4)],
    (D.SMALL, 0, None): [(4, 1, 4, 1, 12)], (D.SMALL, 1, None): [(8, 2, 2, 1, 1)] * 4, (D.SMALL, 2, None): [(8, 4, 1, 16, 1)] * 4,
    (D.ODD, 0, None): [(4, 1, 4, 1, 30)], (D.ODD, 1, None): [(8, 2, 2, 1, 3)] * 4,
    (D.ODD, 2, None): [(7, 4, 1, 4, 1), (8, 4, 1, 7, 1), (7, 4, 1, 4, 1), (8, 4, 1, 7, 1)],
    (D.FULL, 0, None): [(4, 1, 4, 1, 70)], (D.FULL, 1, None): [(7, 2, 2, 1, 7)] * 4,
    (D.FULL, 2, None): [(8, 4, 1, 2, 1), (2, 4, 1, 2, 3), (2, 4, 1, 2, 3), (7, 4, 1, 3, 1)],
    (D.G_B, 1, 1): [(2, 2, 2, 1, 2)] * 4, (D.SMALL, 1, 1): [(2, 2, 2, 1, 4)] * 4,
}


def _matcher(geom, fmt, batch_hint=None):
    from video_distillation_amd import plan, train
    key = (geom, fmt, batch_hint)
    if key not in _MATCHERS:
        _MATCHERS[key] = train.GradMatchEngine(plan.NetGeometry(*geom), 4, (1, 1, 1), "cuda:0", prec=fmt, batch_hint=batch_hint)
    return _MATCHERS[key]


def _assert_planned(gm, geom, li, batch_hint):
    """The planner's choice is the recorded one, the accumulating programs run the storing programs' plans, and those are the
    plans the host-side count walked."""
    fam = [(dp.plan.MTW, dp.plan.NT, dp.plan.MW, dp.plan.ncl, dp.plan.nbox) for dp in gm.bwdV[li]]
    assert fam == PLANNED[(geom, li, batch_hint)], (fam, PLANNED[(geom, li, batch_hint)])
    host = D.bwd_plans(geom, batch_hint, True)[li]
    assert len(host) == len(gm.bwdV[li]) == len(gm.eng.bwd[li])
    for dv, dp, pl in zip(gm.bwdV[li], gm.eng.bwd[li], host):
        assert dv.plan is dp.plan and D.plan_identity(dp.plan) == D.plan_identity(pl)
        assert dv.params.atomic == 1 and dp.params.atomic == 0


def _slot_order(v):
    """fp32 (nb, C, t, h, w) -> flat, in the order of the channels-last slots."""
    nb, C, t, h, w = v.shape
    return v.reshape(nb, C // 8, 8, t, h, w).permute(0, 1, 3, 4, 5, 2).contiguous().reshape(-1)


def _fill_state(gm, c, fmt, V=None, ab=None):
    """Inside ``gm.eng.workspace``: everything ``down_level`` reads, written as the sweeps before it write it.  The levels other than
    the case's carry the network's initial weights (packed, never run).  -> (incoming adjoint, arg-max bytes, pixels or None, V list)"""
    from video_distillation_amd import hip
    eng, li, nb = gm.eng, c.li, c.nb
    W = [p.cuda().float().contiguous() for p in R.init_params(11)[:6]]
    Vs = [p.cuda().float().contiguous() for p in R.init_params(23)[:6]]
    W[2 * li] = c.W.cuda()
    Vs[2 * li] = (c.V if V is None else V).cuda().contiguous()
    gm._pack_adjoint(W, Vs)
    am = c.am.cuda()
    eng.level_unpool(li, nb, c.g1.cuda(), c.layout, am, name="dy", scale_name="gscale")
    _, n1, n2, _, act1, act2, gbar1, gbar2 = gm._sweep_bufs(nb)
    x = None
    if li == 0:
        x = c.a.permute(0, 2, 1, 3, 4).contiguous().cuda()
    else:
        act, gb = (act1, gbar1) if li == 1 else (act2, gbar2)
        src = D.to_slots(c.a, fmt)
        assert tuple(src.shape) == tuple(act.shape), (src.shape, act.shape)
        act.copy_(src.cuda())
        if gm.scaled:          # the tangent as the level below wrote it (fp32, slot order): measured, the common scale with V_l, split
            g32 = _slot_order(c.gbar).cuda()
            sg = gm._absmax_scale(g32, "gscale_up%d" % li, gm.V_TARGET)
            s_l = gm._combine(sg, gm._sv[li], 1, "sscale%d" % li)
            gm._sg = [None, None, None]
            gm._sg[li] = s_l
            hip.run("vd_split_scaled", hip.ptr(g32), g32.numel(), hip.ptr(s_l), hip.ptr(gb[0]), hip.ptr(gb[1]), eng.prec,
                    hip.stream_ptr(eng.device))
        else:                  # (bf16x3: the select program writes the two planes itself)
            gb.copy_(D.to_slots(c.gbar, fmt).cuda())
    return (c.ab if ab is None else ab).cuda().contiguous(), am, x, Vs


def _run(gm, c, fmt, V=None, ab=None, with_hv=True, extra=None):
    """-> (abar (nb, cin, t, h, w) fp64, hv_w - start, hv_b - start, the raw abar buffer on the device).  ``extra(state)`` runs inside
    the same workspace after the level and returns whatever it computes there."""
    eng, li, nb = gm.eng, c.li, c.nb
    with eng.workspace({}):
        grad, am, x, Vs = _fill_state(gm, c, fmt, V, ab)
        big = D.abar_buffer(c.geom, li, nb).cuda()
        hv = wbig = bbig = None
        if with_hv:
            wbig, bbig = D.guarded(c.hw0, 4096).cuda(), D.guarded(c.hb0, 256).cuda()
            hv = [None] * 6
            hv[2 * li], hv[2 * li + 1] = wbig[:c.hw0.numel()].view(c.hw0.shape), bbig[:c.hb0.numel()]
        out = gm.down_level(li, nb, grad, c.layout, am, x, hv, out=big[:nb])
        assert out.data_ptr() == big.data_ptr()
        more = extra(dict(grad=grad, am=am, x=x, V=Vs)) if extra is not None else None
        torch.cuda.synchronize()
    got = D.written_abar(big.cpu(), li, nb)
    dw = db = None
    if with_hv:
        dw, db = D.written_front(wbig.cpu(), c.hw0, "hv_w"), D.written_front(bbig.cpu(), c.hb0, "hv_b")
    return got, dw, db, big, more


def _check(gm, c, fmt, label):
    got, dw, db, _, _ = _run(gm, c, fmt)
    D.check_abar(got, c, fmt, label, WORST_ABAR.setdefault((fmt, c.li), [0.0] * 4))
    D.check_hv_w(dw, c, fmt, label, WORST_HVW.setdefault((fmt, c.li), {}))
    D.check_hv_b(db, c, label)
    print("so far: hv_w rel-L2 %s" % {k: "%.2e" % v for k, v in WORST_HVW[(fmt, c.li)].items()})


# ---- (B) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,fmt,li,nb,batch_hint", D.level_cases(), ids=_IDS)
def test_one_level_of_the_down_sweep_is_the_fp64_one(geom, fmt, li, nb, batch_hint):
    gm = _matcher(geom, fmt, batch_hint)
    _assert_planned(gm, geom, li, batch_hint)
    if batch_hint:
        assert PLANNED[(geom, li, batch_hint)] != PLANNED[(geom, li, None)]
    if li == 2 and nb == 9:
        assert all(nb % dp.plan.ncl for dp in gm.bwdV[2]), "the last clip group of every level-2 program is ragged"
    _check(gm, D.case(geom, li, nb), fmt, "%s x %d clips%s" % (geom, nb, ", batch_hint %d" % batch_hint if batch_hint else ""))


@pytest.mark.parametrize("geom,fmt,li,nb,pattern", D.pattern_cases(), ids=_IDS)
def test_sparse_patterns(geom, fmt, li, nb, pattern):
    """The incoming adjoint only in the last pooled row and column; dz only on the border shell of the conv grid."""
    _check(_matcher(geom, fmt), D.case(geom, li, nb, pattern), fmt, "%s x %d clips, %s" % (geom, nb, pattern))


@pytest.mark.parametrize("geom,fmt,li,nb,mags", D.magnitude_cases(), ids=_IDS)
def test_magnitudes_pass_through_the_composed_scales(geom, fmt, li, nb, mags):
    """zscale, dvscale = gscale x vscale and gdscale = gscale x sscale with each factor 1e-7 or 1e4 away from the others: the same
    relative bars."""
    _check(_matcher(geom, fmt), D.case(geom, li, nb, "full", mags), fmt, "%s x %d clips, (ab, g1, V, gbar) x %s" % (geom, nb, mags))


@pytest.mark.parametrize("geom,fmt,li,nb", D.exact_cases(), ids=_IDS)
def test_integer_data_equals_fp64(geom, fmt, li, nb):
    c = D.case(geom, li, nb, kind="exact")
    got, dw, db, _, _ = _run(_matcher(geom, fmt), c, fmt)
    want = c.t1 + c.t2
    assert torch.equal(got, want), "abar: %d of %d elements differ from fp64" % (int((got != want).sum()), want.numel())
    assert torch.equal(dw, c.w1 + c.w2), "hv_w - start: %d elements differ from fp64" % int((dw != c.w1 + c.w2).sum())
    assert torch.equal(db, c.hb), "hv_b - start differs from fp64"


@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom", [D.G_A, D.G_B, D.G_C, D.SMALL], ids=_IDS)
def test_zero_adjoint_of_the_weights_leaves_the_storing_launch(geom, li):
    """V = 0: abar_l is what ``level_dgrad(eng.bwd[li], ...)`` alone writes, value for value -- the accumulating launch added zeros."""
    fmt, nb = "f16x3", (3 if li == 0 else 9)
    gm, c = _matcher(geom, fmt), D.case(geom, li, nb)
    eng = gm.eng

    def alone(state):
        big = D.abar_buffer(geom, li, nb).cuda()
        zb, nslots, _, inv_z = eng.level_unpool(li, nb, state["grad"], c.layout, state["am"], name="zb", scale_name="zscale")
        eng.level_dgrad(eng.bwd[li], zb, nslots, big[:nb], nb, inv_z)
        return big

    _, _, _, big, ref = _run(gm, c, fmt, V=torch.zeros_like(c.V), with_hv=False, extra=alone)
    assert torch.equal(big[:nb], ref[:nb])
    assert bool((big[:nb] != 0).any())


@pytest.mark.parametrize("li", [0, 1, 2])
@pytest.mark.parametrize("geom,fmt", [(D.G_A, "f16x3"), (D.G_B, "f16x3"), (D.G_B, "bf16x3"), (D.G_C, "f16x3"), (D.SMALL, "f16x3")], ids=_IDS)
def test_accumulating_onto_zeros_is_the_storing_program(geom, fmt, li):
    """Incoming adjoint = 0: abar_l equals, bit for bit, a plain storing ``_DevPlan`` of the same plan packed with the scaled V_l and
    run over dz with dvscale."""
    from video_distillation_amd import engine
    nb = 3 if li == 0 else 9
    gm, c = _matcher(geom, fmt), D.case(geom, li, nb)
    eng = gm.eng

    def plain(state):
        big = D.abar_buffer(geom, li, nb).cuda()
        progs = [engine._DevPlan(dp.plan, eng.device, eng.prec_bwd) for dp in eng.bwd[li]]
        for dp in progs:
            assert dp.params.atomic == 0
            dp.pack(gm._Vs[li] if gm.scaled else state["V"][2 * li])
        dy = eng.dy_buf(li, nb)
        inv = eng.scale_buf("dvscale%d" % li)[1:] if gm.scaled else None
        eng.level_dgrad(progs, dy, int(dy.shape[1]), big[:nb], nb, inv)
        torch.cuda.synchronize()          # (``progs`` own their tables: they must outlive their launches)
        return big

    _, _, _, big, ref = _run(gm, c, fmt, ab=torch.zeros_like(c.ab), with_hv=False, extra=plain)
    assert torch.equal(big[:nb].view(torch.int32), ref[:nb].view(torch.int32))
    assert bool((big[:nb] != 0).any())


def test_accumulating_pixel_programs_in_one_launch_and_in_four(monkeypatch):
    """65 x 63 x 4, level 0: the four parity-class programs in accumulating form as one launch (vd_conv_mfma_multi) and as four."""
    gm, c = _matcher(D.G_B, "f16x3"), D.case(D.G_B, 0, 3)
    assert len(gm.bwdV[0]) == 4
    outs = {}
    for multi in ("0", "1"):
        monkeypatch.setenv("VD_MULTI_LAUNCH", multi)
        outs[multi] = _run(gm, c, "f16x3", with_hv=False)[3]
    assert torch.equal(outs["0"][:3].view(torch.int32), outs["1"][:3].view(torch.int32))


# ---- (C) the conv levels' whole second-order pass on the recorded decisions -----------------------------------------------------------
VJP_BAR, TIGHT = 2e-4, 1e-4          # the free comparisons' bars: the starting point; every one was more than ten times the measured worst
BARS = {"f16x3": {"g_feat": 7.4e-6, "x": 3.3e-6, "params": 6.8e-6},           # ... so each is 4 x the measured worst (module docstring)
        "bf16x3": {"g_feat": 2.4e-5, "x": 3.2e-5, "params": 3.2e-5}}
P6 = ("w0", "b0", "w1", "b1", "w2", "b2")


@functools.lru_cache(maxsize=None)
def _whole_inputs(geom, nb):
    from video_distillation_amd import plan
    gen = torch.Generator().manual_seed(90 + sum(geom))
    x = torch.randn(nb, geom[0], 3, geom[1], geom[2], generator=gen)
    x = (x - x.mean()) / x.std()
    params = [p.contiguous() for p in R.init_params(4)[:6]]
    gf = torch.randn(nb, plan.NetGeometry(*geom).num_feat, generator=gen)
    v6 = [torch.randn(p.shape, generator=gen) for p in params]
    return x, params, gf, v6


def _routed_second_order(x, params, gf, v6, am, stats):
    """fp64: G = grad(routed feats, p6, g_feat, create_graph), s = sum <v_i, G_i>, grad(s, [g_feat, x, *p6])."""
    routes = A.routes_from_argmax([a.cpu() for a in am], tuple(x.shape), params)
    p64 = [p.double().clone().requires_grad_(True) for p in params]
    xr = x.double().permute(0, 2, 1, 3, 4).clone().requires_grad_(True)
    g64 = gf.double().clone().requires_grad_(True)
    feats = A.routed_feature_layers(xr, p64, routes, stats).reshape(x.shape[0], -1)
    G = torch.autograd.grad(feats, p64, g64, create_graph=True, allow_unused=True)
    s = sum((v.double() * g).sum() for v, g in zip(v6, G) if g is not None and v is not None)
    out = torch.autograd.grad(s, [g64, xr] + p64, allow_unused=True)
    gbar, xbar = out[0], out[1].permute(0, 2, 1, 3, 4)
    return gbar, xbar, [torch.zeros_like(p) if o is None else o for o, p in zip(out[2:], p64)]


def _rel(got, want):
    got, want = got.double().cpu(), want.double()
    n = float(want.norm())
    if n == 0.0:
        assert float(got.abs().max()) == 0.0, "a quantity whose reference is identically zero is not zero"
        return 0.0
    return float((got - want).norm()) / n


def _second_order(geom, fmt, nb, v6, label):
    x, params, gf, _ = _whole_inputs(geom, nb)
    gm = _matcher(geom, fmt)
    p_dev = [p.cuda() for p in params]
    feats, fs = gm.ag_feat_forward(x.cuda(), p_dev)
    _, _, bs = gm.ag_feat_backward(fs, gf.cuda(), p_dev, False, True, True)
    gbar3, xbar, hv = gm.ag_feat_second_order(fs, bs, [None if v is None else v.cuda() for v in v6], p_dev, True)
    torch.cuda.synchronize()
    stats = []
    want_g, want_x, want_p = _routed_second_order(x, params, gf, v6, fs["am"], stats)
    assert all(s["not_near_tie"] == 0 for s in stats), stats          # no clip is exempt: a window routed otherwise must be a near-tie
    per_g = [_rel(gbar3[i], want_g[i]) for i in range(nb)]
    per_x = [_rel(xbar[i], want_x[i]) for i in range(nb)]
    per_p = [_rel(h, w) for h, w in zip(hv, want_p)]
    for q, v in (("g_feat", max(per_g)), ("x", max(per_x)), ("params", max(per_p))):
        WORST[(fmt, q)] = max(WORST.get((fmt, q), 0.0), v)
    print("second order %s %s %s vs ROUTED fp64: adjoint of g_feat per clip %s, of x per clip %s, of %s %s | windows routed otherwise %s, "
          "no near-tie %s | WORST %s" % (fmt, geom, label, ["%.2e" % v for v in per_g], ["%.2e" % v for v in per_x], P6, ["%.2e" % v for v in per_p],
                                        [s["mismatch"] for s in stats], [s["not_near_tie"] for s in stats],
                                        {k: "%.2e" % v for k, v in WORST.items()}))
    bars = BARS[fmt]
    assert bool(torch.isfinite(xbar).all()) and bool(torch.isfinite(gbar3).all())
    assert max(per_g) < bars["g_feat"], ("adjoint of g_feat", per_g)
    assert max(per_x) < bars["x"], ("adjoint of x", per_x)
    assert max(per_p) < bars["params"], ("parameter adjoints", dict(zip(P6, per_p)))


@pytest.mark.parametrize("geom,nb,fmt", [(D.G_A, 3, "f16x3"), (D.G_B, 3, "f16x3"), (D.G_B, 3, "bf16x3"), (D.G_C, 3, "f16x3"), (D.SMALL, 2, "f16x3")],
                         ids=_IDS)
def test_whole_second_order_pass_on_the_recorded_decisions(geom, nb, fmt):
    _second_order(geom, fmt, nb, _whole_inputs(geom, nb)[3], "all six adjoints")


@pytest.mark.parametrize("li", [0, 1, 2])
def test_second_order_pass_for_one_level_s_weights_at_a_time(li):
    v6 = [v if k == 2 * li else None for k, v in enumerate(_whole_inputs(D.G_B, 3)[3])]
    _second_order(D.G_B, "f16x3", 3, v6, "v only for w%d" % li)


@pytest.mark.parametrize("mag", [1e-7, 1e4])
def test_second_order_pass_at_other_magnitudes_of_the_adjoints(mag):
    v6 = [v * mag for v in _whole_inputs(D.G_B, 3)[3]]
    _second_order(D.G_B, "f16x3", 3, v6, "v x %g" % mag)
