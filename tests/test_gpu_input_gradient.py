"""The input-gradient programs of csrc/conv_mfma.hip, checked where no pooling decision can excuse an error.

(B) ONE LEVEL AS THE LINEAR OPERATOR IT IS: a random pooled gradient and random arg-max bytes (ReLU-dead windows among them) go
    through exactly the two steps ``EmbedEngine.backward`` and train.py run for a level -- ``level_unpool`` (ReLU + max-pool
    backward, power-of-two scale, 16-bit split) and ``level_dgrad`` (the level's parity-class programs, or the merged pixel
    program) -- and the result is compared with fp64: the same scatter by index arithmetic, then autograd of ``F.conv3d``
    with respect to its input.  Nothing is decided anywhere, so every clip and every input parity class (h % 2, w % 2) of every
    clip is held to the bound of a single linear conv program (tests/test_gpu_wgrad.py), whole and on its border shell alone,
    and every output element must have been written exactly where the level owns it.
(C) THE WHOLE FIRST-ORDER GRADIENT ON THE RECORDED DECISIONS: forward(keep) + backward against the fp64 oracle routed by the
    arg-max bytes the forward recorded (tests/argmax_tools.py) -- no clip is exempt as an "arg-max flip" -- and the decisions
    themselves against the fp64 values: every window routed otherwise must be a near-tie.

Clip sizes: next to 64 x 64 x 8, 96 x 80 x 12 and 112 x 112 x 16 the three sizes whose program families no other GPU test
launches (tests/test_plan_emulation.py::test_clip_sizes_off_the_multiple_of_four states what each of them plans to): 64 x 66 x 4
(W = 2 mod 4), 65 x 63 x 4 (odd H and W) and 70 x 58 x 4.

Bounds.  (B) relative L2 per clip and parity class, whole and on the border shell; the largest absolute error over the largest
reference element of the same subset gets four times that (the ratio of test_embed_forward_small).  Starting point: what
tests/test_gpu_wgrad.py holds a single linear conv program to -- f16x3 2e-5, bf16x3 1e-4, f16 2e-3.  A bound stays where the
measured worst is within ten times of it; otherwise it is four times the measured worst (the kernels are deterministic and the
inputs seeded: the spread comes from the inputs alone).  MEASURED on an MI355X, worst over all cases (rel-L2 / shell / max-abs):
    f16x3   level 0  5.40e-07 / 4.59e-07 / 1.66e-06    level 1  6.00e-07 / 5.20e-07 / 1.56e-06    level 2  5.22e-07 / 5.06e-07 / 1.35e-06
            -> 2e-5 was 33 x the worst: bound 4 x 6.00e-07 = 2.4e-6
    bf16x3  level 0  4.62e-06 / 4.61e-06 / 5.32e-06    level 1  4.70e-06 / 4.71e-06 / 5.44e-06    level 2  4.93e-06 / 4.93e-06 / 6.44e-06
            -> 1e-4 was 20 x the worst: bound 4 x 4.93e-06 = 2.0e-5
    f16     level 0  3.03e-04 / 3.06e-04 / 4.08e-04    level 1  3.09e-04 / 3.09e-04 / 3.82e-04    level 2  3.35e-04 / 3.35e-04 / 4.53e-04
            -> 2e-3 is 6 x the worst: stays
(the three new clip sizes, the small-box and latency-oriented programs and the magnitudes 1e-7 / 1e4 all lie inside these figures).
(C) whole gradient, f16x3, per clip against the ROUTED fp64 oracle: measured 7.3e-07 .. 8.14e-07 over the twelve clips of the four
sizes, no window routed otherwise at any level -> the "tight" 1e-4 of the free comparisons was 120 x the worst: bound
4 x 8.14e-07 = 3.3e-6.  With the single-pass f16 backward at 65 x 63 x 4: 5.14e-04 worst, bound 2e-3 (4 x) stays.  Features against
the free fp64 oracle: f16x3 8.1e-07 .. 9.9e-07 (bound 3e-5), f16 2.7e-04 .. 2.9e-04 (bound 2e-3): the bounds of tests/test_gpu_embed.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import argmax_tools as A
from tests import aux_oracle as AO

pytestmark = pytest.mark.gpu

G_A, G_B, G_C = (4, 64, 66), (4, 65, 63), (4, 70, 58)
SMALL, ODD, FULL = (8, 64, 64), (12, 96, 80), (16, 112, 112)

BOUND = {"f16x3": 2.4e-6, "bf16x3": 2.0e-5, "f16": 2e-3}      # relative L2 of one level against fp64 (module docstring: 4 x measured worst / kept)
ROUTED_TIGHT = 3.3e-6                                         # whole gradient, f16x3, per clip, against the ROUTED fp64 oracle
ROUTED_F16 = 2e-3                                             # ... with the single-pass f16 backward
FWD_TOL = {"f16x3": 3e-5, "f16": 2e-3}                        # features against the free fp64 oracle (tests/test_gpu_embed.py TOL)

WORST = {}                                                    # (format, level) -> [rel-L2, shell rel-L2, max-abs ratio] seen so far
_ENGINES = {}


def _engine(geom, fmt, batch_hint=None, bwd0_small=False, seed=11):
    """One engine per (clip size, backward format, options), weights packed for the input-gradient programs."""
    from video_distillation_amd import engine, plan
    key = (geom, fmt, batch_hint, bwd0_small, seed)
    if key not in _ENGINES:
        eng = engine.EmbedEngine(plan.NetGeometry(*geom), prec="f16x3" if fmt == "f16" else fmt, prec_bwd=fmt, device="cuda:0",
                                 batch_hint=batch_hint, bwd0_small=bwd0_small)
        eng.set_weights([p.cuda() for p in R.init_params(seed)])
        eng._pack_bwd()
        _ENGINES[key] = eng
    return _ENGINES[key]


def _dense_gradient(g, am, dims, layout):
    """fp64 backward of ReLU + MaxPool3d((pool_t, 2, 2)) by index arithmetic: pooled element (clip, n, pt, pr, pc) with arg-max byte
    a sends its gradient to conv position (pt * pool_t + a.bit2, 2 pr + a.bit1, 2 pc + a.bit0); bit 7 (dead window) sends nothing.
    g / am in the layouts vd_unpool_relu_bwd takes (0: (C,T,H,W) features order, 1: channels-last); -> (nb, C, T, OH, OW)."""
    cout, T, OH, OW, To, Ho, Wo, pt = dims[1], *dims[5:12]
    nb, npos = g.shape[0], To * Ho * Wo
    if layout == 0:
        gd, a = g.double().reshape(nb, cout, npos), am.reshape(nb, cout, npos)
    else:
        gd = g.double().reshape(nb, npos, cout).permute(0, 2, 1)
        a = am.reshape(nb, cout // 8, npos, 8).permute(0, 1, 3, 2).reshape(nb, cout, npos)
    a = a.to(torch.int64)
    clip, n, pos = torch.meshgrid(torch.arange(nb), torch.arange(cout), torch.arange(npos), indexing="ij")
    t = (pos // (Ho * Wo)) * pt + ((a >> 2) & 1)
    oh, ow = 2 * ((pos // Wo) % Ho) + ((a >> 1) & 1), 2 * (pos % Wo) + (a & 1)
    ok = a < (8 if pt == 2 else 4)
    dense = torch.zeros(nb, cout, T, OH, OW, dtype=torch.float64)
    dense[clip[ok], n[ok], t[ok], oh[ok], ow[ok]] = gd[ok]
    return dense


@functools.lru_cache(maxsize=None)
def _case(geom, li, nb, mag=1.0, seed=11):
    """Inputs of one level and the fp64 input gradient, shared by the formats: (g fp32, arg-max bytes, layout, want (nb,cin,t,h,w))."""
    from video_distillation_amd import plan
    dims = plan.NetGeometry(*geom).layer_dims()[li]
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = dims
    layout = 0 if li == 2 else 1
    gen = torch.Generator().manual_seed(1000 * li + nb + sum(geom))
    shape = (nb, cout, To, Ho, Wo) if layout == 0 else (nb, To, Ho, Wo, cout)
    g = (torch.randn(shape, generator=gen) * mag).contiguous()
    am = AO.argmax_bytes(77 + li + nb, (nb, cout, To, Ho, Wo) if layout == 0 else (nb, cout // 8, To, Ho, Wo, 8), pt)
    assert bool((am & 0x80 != 0).any()) and bool((am & 0x80 == 0).any())
    dy = _dense_gradient(g, am, dims, layout)
    wt = R.init_params(seed)[2 * li].double()
    xin = torch.zeros(nb, cin, t, h, w, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv3d(xin, wt, None, stride=(1, 2, 2), padding=(1, 3, 3)), xin, dy)
    return g, am, layout, want


def _run_level(eng, li, nb, g, am, layout):
    """The level's two steps as EmbedEngine.backward runs them, into a NaN-filled output with one guard clip behind it.
    -> (nb, cin, t, h, w) fp64 on the host; asserts that every element of the nb clips was written and none of the guard."""
    cin, _, t, h, w = eng.dims[li][:5]
    if li == 0:
        big = torch.full((nb + 1, t, cin, h, w), float("nan"), dtype=torch.float32, device="cuda")
        out = big[:nb]
    else:
        big = eng.dx_buf(li, nb + 1)
        big.fill_(float("nan"))
        out = eng.dx_buf(li, nb)
        assert out.data_ptr() == big.data_ptr()
    dy, nslots, _, inv = eng.level_unpool(li, nb, g.cuda(), layout, am.cuda())
    eng.level_dgrad(eng.bwd[li], dy, nslots, out, nb, inv)
    torch.cuda.synchronize()
    res = big.cpu()
    assert bool(torch.isnan(res[nb]).all()), "level %d wrote behind its last clip" % li
    unwritten = int(torch.isnan(res[:nb]).sum())
    assert unwritten == 0, "level %d left %d of %d output elements unwritten (or wrote NaN)" % (li, unwritten, res[:nb].numel())
    got = res[:nb].double()
    return got.permute(0, 2, 1, 3, 4) if li == 0 else got.permute(0, 4, 1, 2, 3)


def _check_level(got, want, fmt, li, label):
    """Per clip and per parity class (h % 2, w % 2): rel-L2 whole and on the border shell (within 3 of a spatial edge, or first / last
    frame) below the format's bound, largest absolute error over the largest reference element of the subset below 4 x the bound."""
    nb, _, t, h, w = want.shape
    tt, hh, ww = torch.arange(t), torch.arange(h), torch.arange(w)
    shell = (((tt == 0) | (tt == t - 1))[:, None, None] | ((hh < 3) | (hh >= h - 3))[None, :, None] | ((ww < 3) | (ww >= w - 3))[None, None, :])
    worst, where = [0.0, 0.0, 0.0], [None, None, None]
    for b in range(nb):
        for ph in range(min(2, h)):
            for pw in range(min(2, w)):
                d, r = (got[b] - want[b])[:, :, ph::2, pw::2], want[b][:, :, ph::2, pw::2]
                s = shell[:, ph::2, pw::2].expand_as(r)
                vals = (float(d.norm() / r.norm()), float(d[s].norm() / r[s].norm()), float(d.abs().max() / r.abs().max()))
                for k, v in enumerate(vals):
                    if not v <= worst[k]:
                        worst[k], where[k] = v, (b, ph, pw)
    rec = WORST.setdefault((fmt, li), [0.0, 0.0, 0.0])
    for k in range(3):
        rec[k] = max(rec[k], worst[k])
    print("input gradient %s level %d %s: worst rel-L2 %.2e at (clip, ph, pw) %s, border shell %.2e at %s, max-abs ratio %.2e at %s | so far %s"
          % (fmt, li, label, worst[0], where[0], worst[1], where[1], worst[2], where[2], ["%.2e" % v for v in rec]))
    bound = BOUND[fmt]
    assert worst[0] < bound, ("rel-L2", worst[0], where[0])
    assert worst[1] < bound, ("border shell rel-L2", worst[1], where[1])
    assert worst[2] < 4 * bound, ("max-abs ratio", worst[2], where[2])


def _clips(eng, li, nb):
    """"ncl+1": one clip more than the largest clip group of the level's programs -- every program's last group is ragged."""
    if nb != "ncl+1":
        return nb
    return max(dp.plan.ncl for dp in eng.bwd[li]) + 1


def _level_cases():
    out = []
    for geom, fmts in ((G_A, ("f16x3", "f16")), (G_B, ("f16x3", "f16")), (G_C, ("f16x3", "f16")), (SMALL, ("f16x3", "f16", "bf16x3"))):
        for fmt in fmts:
            out += [(geom, fmt, 0, 1), (geom, fmt, 0, 3), (geom, fmt, 1, "ncl+1"), (geom, fmt, 2, "ncl+1")]
    out += [(ODD, "f16x3", 0, 2), (ODD, "f16x3", 1, "ncl+1"), (ODD, "f16x3", 2, 8)]
    out += [(FULL, "f16x3", 0, 1), (FULL, "f16x3", 1, 3), (FULL, "f16x3", 2, 3)]
    return out


@pytest.mark.parametrize("geom,fmt,li,nb", _level_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_level_input_gradient_is_the_fp64_transposed_convolution(geom, fmt, li, nb):
    eng = _engine(geom, fmt)
    nb = _clips(eng, li, nb)
    if geom == G_C and li == 2:
        assert nb == 65 and sorted(dp.plan.ncl for dp in eng.bwd[2]) == [32, 32, 64, 64]
    if geom == G_A and li == 2:
        assert nb == 33
    if geom == G_B and li == 0:
        assert len(eng.bwd[0]) == 4 and all(dp.plan.col_off is None for dp in eng.bwd[0])      # four parity-class programs, pixel output
    if geom in (G_A, G_C) and li == 0:
        assert len(eng.bwd[0]) == 1 and eng.bwd[0][0].plan.meta["block_w"] == 2                # the merged program in 2 x 2 pixel blocks
    g, am, layout, want = _case(geom, li, nb)
    got = _run_level(eng, li, nb, g, am, layout)
    _check_level(got, want, fmt, li, "%s x %d clips" % (geom, nb))


@pytest.mark.parametrize("li", [1, 2])
def test_latency_oriented_input_gradient_programs(li):
    """batch_hint = 8 at 112 x 112 x 16 re-plans the parity-class programs of levels 1 and 2 for short workgroups
    (plan.latency_variant): the same operator against fp64."""
    base, eng = _engine(FULL, "f16x3"), _engine(FULL, "f16x3", batch_hint=8)
    shape = lambda e: [(dp.plan.MTW, dp.plan.ncl, dp.plan.nbox) for l in (1, 2) for dp in e.bwd[l]]          # noqa: E731
    assert shape(base) != shape(eng), "the hint did not change any program of levels 1 and 2"
    g, am, layout, want = _case(FULL, li, 3)
    _check_level(_run_level(eng, li, 3, g, am, layout), want, "f16x3", li, "%s x 3 clips, batch_hint 8" % (FULL,))


@pytest.mark.parametrize("geom", [SMALL, G_A])
def test_first_level_input_gradient_in_small_boxes(geom):
    """bwd0_small (the training engines): the merged pixel program in boxes of 4 M tiles per wave within 1800 LDS slots."""
    base, eng = _engine(geom, "f16x3"), _engine(geom, "f16x3", bwd0_small=True)
    pl = eng.bwd[0][0].plan
    assert len(eng.bwd[0]) == 1 and pl.MTW == 4 and pl.lds_slots <= 1800 and pl.nbox > base.bwd[0][0].plan.nbox
    for nb in (1, 3):
        g, am, layout, want = _case(geom, 0, nb)
        _check_level(_run_level(eng, 0, nb, g, am, layout), want, "f16x3", 0, "%s x %d clips, small boxes" % (geom, nb))


@pytest.mark.parametrize("fmt", ["f16x3", "f16"])
@pytest.mark.parametrize("mag", [1e-7, 1e4])
def test_gradient_magnitudes_pass_through_the_power_of_two_scale(fmt, mag):
    """vd_absmax_scale's scale goes in through level_unpool and comes out through ``inv``: gradients far below fp16's smallest
    normal and far above 1 are reproduced as exactly as O(1) ones (magnitude 1 is the case of the table above)."""
    eng = _engine(SMALL, fmt)
    nb = _clips(eng, 1, "ncl+1")
    g, am, layout, want = _case(SMALL, 1, nb, mag)
    g1, _, _, want1 = _case(SMALL, 1, nb)
    assert torch.equal(g, g1 * mag) and float(want.abs().max()) > 0.5 * mag * float(want1.abs().max())
    got = _run_level(eng, 1, nb, g, am, layout)
    assert bool(torch.isfinite(got).all())
    _check_level(got, want, fmt, 1, "%s x %d clips at |g| ~ %g" % (SMALL, nb, mag))


# ---- (C) the whole first-order gradient on the recorded decisions ------------------------------------------------------------------
def _routed_gradient(x, gf, params, am):
    """fp64 gradient of (routed features * gf).sum() with every pooling decision taken from the arg-max bytes ``am``."""
    p64 = [p.double() for p in params[:6]]
    routes = A.routes_from_argmax([a.cpu() for a in am], tuple(x.shape), params)
    xr = x.double().permute(0, 2, 1, 3, 4).clone().requires_grad_(True)
    feats = A.routed_feature_layers(xr, p64, routes)
    (feats.reshape(x.shape[0], -1) * gf.double()).sum().backward()
    return xr.grad.permute(0, 2, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def _whole(geom):
    from video_distillation_amd import plan
    params = R.init_params(4)
    gen = torch.Generator().manual_seed(60 + sum(geom))
    x = torch.randn(3, geom[0], 3, geom[1], geom[2], generator=gen)
    gf = torch.randn(3, plan.NetGeometry(*geom).num_feat, generator=gen)
    with torch.no_grad():
        feats64 = R.convnet3d_embed(x.double(), [p.double() for p in params])
    return params, x, gf, feats64


def _per_clip(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return [float((got[i] - want[i]).norm() / want[i].norm()) for i in range(want.shape[0])]


@pytest.mark.parametrize("geom", [G_A, G_B, G_C, SMALL], ids=lambda v: "x".join(map(str, v)))
def test_whole_input_gradient_on_the_recorded_decisions(geom):
    from video_distillation_amd import engine, plan
    params, x, gf, feats64 = _whole(geom)
    eng = engine.EmbedEngine(plan.NetGeometry(*geom), prec="f16x3", device="cuda:0")
    eng.set_weights([p.cuda() for p in params])
    feats, saved = eng.forward(x.cuda(), keep=True)
    dx = eng.backward(saved, gf.cuda())
    torch.cuda.synchronize()
    assert len(saved) == 1
    am = [a.cpu() for a in saved[0][2:5]]
    # forward, both precision families, against the FREE fp64 oracle
    e16 = engine.EmbedEngine(plan.NetGeometry(*geom), prec="f16", device="cuda:0")
    e16.set_weights([p.cuda() for p in params])
    if geom == G_C:
        assert len(e16.fwd[0].plan.types) == 4 and not e16.fwd[0].breg_ok       # four box types: the generic kernel, single pass too
    fwd = {"f16x3": feats.double().cpu(), "f16": e16.forward(x.cuda()).double().cpu()}
    rel = {k: (float((v - feats64).norm() / feats64.norm()), float((v - feats64).abs().max() / feats64.abs().max())) for k, v in fwd.items()}
    # decisions: every window the fp64 values route otherwise is a near-tie of those values
    dec = A.compare_decisions(x, params, am)
    # arithmetic: every clip against the oracle routed by the recorded decisions
    per = _per_clip(dx, _routed_gradient(x, gf, params, am))
    print("whole gradient %s f16x3 vs ROUTED fp64, per clip: %s | windows routed otherwise per level %s, no near-tie %s, worst margin %s | "
          "features vs free fp64 (rel-L2, rel-max): %s" % (geom, ["%.2e" % v for v in per], [d["mismatch"] for d in dec],
                                                          [d["not_near_tie"] for d in dec], ["%.1e" % d["worst_margin"] for d in dec],
                                                          {k: "%.2e %.2e" % v for k, v in rel.items()}))
    assert all(d["not_near_tie"] == 0 for d in dec), dec
    assert max(per) < ROUTED_TIGHT, per
    for k, (l2, mx) in rel.items():
        assert l2 < FWD_TOL[k] and mx < 4 * FWD_TOL[k], (k, l2, mx)


@pytest.mark.parametrize("geom", [G_A, G_B], ids=lambda v: "x".join(map(str, v)))
def test_first_layer_kernel_variants_are_bitwise_equal_off_the_multiple_of_four(monkeypatch, geom):
    """VD_L0_BREG = 0 / 4 / 5 (generic tile program, register-resident B with the plain K loop, the same with shared A fragments)
    at pixel rows of width 66 and 63: bitwise equal features, and 4 / 5 really ran vd_conv0_breg's program."""
    from video_distillation_amd import engine, plan
    params, x, _, _ = _whole(geom)
    outs = {}
    for variant in ("0", "4", "5"):
        monkeypatch.setenv("VD_L0_BREG", variant)
        eng = engine.EmbedEngine(plan.NetGeometry(*geom), prec="f16", device="cuda:0", ntw0=1)
        assert eng.fwd[0].breg_ok == (variant != "0") and eng.fwd[0].breg_variant == int(variant)
        assert eng.fwd[0].plan.meta.get("frame_tiles") == 1 and len(eng.fwd[0].plan.types) == 1
        eng.set_weights([p.cuda() for p in params])
        outs[variant] = eng.forward(x.cuda())
    torch.cuda.synchronize()
    assert torch.equal(outs["0"], outs["4"]) and torch.equal(outs["0"], outs["5"])


def test_single_pass_backward_on_the_recorded_decisions_at_an_odd_clip_size():
    """prec_bwd = 'f16' at 65 x 63 x 4 (four parity-class pixel programs at level 0), per clip against the routed fp64 oracle."""
    from video_distillation_amd import engine, plan
    params, x, gf, _ = _whole(G_B)
    eng = engine.EmbedEngine(plan.NetGeometry(*G_B), prec="f16x3", prec_bwd="f16", device="cuda:0")
    eng.set_weights([p.cuda() for p in params])
    _, saved = eng.forward(x.cuda(), keep=True)
    dx = eng.backward(saved, gf.cuda())
    torch.cuda.synchronize()
    per = _per_clip(dx, _routed_gradient(x, gf, params, [a.cpu() for a in saved[0][2:5]]))
    print("whole gradient %s f16 backward vs ROUTED fp64, per clip: %s" % (G_B, ["%.2e" % v for v in per]))
    assert bool(torch.isfinite(dx).all()) and max(per) < ROUTED_F16, per
