"""Seeded inputs, fp64 references, format floors and checkers of ONE level of the second-order DOWN sweep (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_gpu_down_sweep.py (``train.GradMatchEngine.down_level`` on the device) and tests/test_down_sweep_cpu.py (the
box plans name every output element exactly once, the checkers catch what they are for, the operand formats alone stay below the
bars, the integer cases are exact in fp32), so that both speak about the same data.  torch and numpy on the CPU only; of the product
package only ``plan`` (the planner is host code).

A level computes, from the pooled incoming adjoint ``ab`` and the pooled first-order gradient ``g1`` (both scattered to the conv grid by
the SAME arg-max bytes: zb = P^T ab, dz = P^T g1), the level's weights W and their adjoints V, its source a and tangent gbar:

    abar  = convT(zb, W) + convT(dz, V)           t1 + t2: a storing launch, then an accumulating one (fp32 atomic adds)
    hv_w += dW(a, zb) + dW(gbar, dz)              w1 + w2: two accumulations into one tensor (gbar_0 = 0: one at level 0)
    hv_b += sum zb

Bars.  Nothing here is measured from the code under test.  With B the bound a single input-gradient program is held to
(tests/test_gpu_input_gradient.py BOUND) a subset S of abar passes when
    ||got - want||_S <= B (||t1||_S + ||t2||_S) + 2^-24 ||want||_S
-- each launch within its own bound (triangle inequality) plus the one fp32 add of the accumulation -- and its largest absolute
error is at most 4 B x its largest reference element.  hv_w: the same form with BAR of tests/param_gradient_cases.py over its four
slice families; a slice that is zero in both terms must be exactly zero.  hv_b: within gamma(k) x the sum of the absolute terms.

Magnitudes multiply the unit case's tensors: ab, g1 and gbar are randn there, V has the weights' own distribution (so that the two
terms of abar are of one size in the unit case and neither hides under the other's allowance).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import aux_oracle as AO
from tests import param_gradient_cases as PG
from tests.forward_level_cases import to_slots          # noqa: F401  (the GPU test writes a_l and reads slot layouts with it)
from tests.test_gpu_input_gradient import BOUND, _dense_gradient

G_A, G_B, G_C, SMALL, ODD, FULL = PG.G_A, PG.G_B, PG.G_C, PG.SMALL, PG.ODD, PG.FULL
SIZES = (G_A, G_B, G_C, SMALL, ODD, FULL)
BAR = PG.BAR
U32 = AO.U32
ONES = (1.0, 1.0, 1.0, 1.0)                        # magnitudes of (incoming adjoint, g1, V, gbar)
PATTERNS = ("full", "last", "dzshell")
GRAD_TARGET, V_TARGET = 1024.0, 128.0              # engine.GRAD_TARGET(), train.GradMatchEngine.V_TARGET
WSHIFT = {"f16x3": 256.0}                          # hip.F16X3_WSHIFT
layer_dims = PG.layer_dims


# ------------------------------------------------------------------------------------------------------------------- the case lists
def level_cases():
    """(clip size, format, level, clips, batch_hint) of part (B).  9 clips leave the last clip group of every level-2 program
    ragged (8, 32 or 64 clips per box)."""
    out = []
    for geom, fmts in ((G_A, ("f16x3",)), (G_B, ("f16x3", "bf16x3")), (G_C, ("f16x3",))):
        for li, nb in ((0, 1), (0, 3), (1, 9), (2, 9), (2, 1)):
            out += [(geom, fmt, li, nb, None) for fmt in fmts]
    for li, nb in ((0, 3), (1, 9), (2, 9), (2, 1)):
        out += [(SMALL, fmt, li, nb, None) for fmt in ("f16x3", "bf16x3")]
    out += [(ODD, "f16x3", 0, 2, None), (ODD, "f16x3", 1, 2, None), (ODD, "f16x3", 2, 9, None)]
    out += [(FULL, "f16x3", li, 2, None) for li in range(3)]
    out += [(G_B, "f16x3", 1, 3, 1), (SMALL, "f16x3", 1, 3, 1)]
    return out


def pattern_cases():
    """(clip size, format, level, clips, pattern): the two sparse patterns where they reach what they are for -- the ragged last boxes
    and the four parity-class pixel programs of the three sizes off the multiple of four, and one case per level above."""
    base = [(G_A, 0, 3), (G_B, 0, 3), (G_C, 0, 3), (G_B, 1, 9), (G_B, 2, 9)]
    return [(geom, "f16x3", li, nb, p) for geom, li, nb in base for p in ("last", "dzshell")]


def magnitude_cases():
    """(clip size, format, level, clips, magnitudes): each of ab, g1, V, gbar at 1e-7 and at 1e4, one at a time, and all at 1e-7
    (no tangent at level 0)."""
    out = []
    for geom, li, nb in ((G_B, 1, 9), (SMALL, 0, 3)):
        n = 4 if li else 3
        for k in range(n):
            for m in (1e-7, 1e4):
                out.append((geom, "f16x3", li, nb, tuple(m if j == k else 1.0 for j in range(4))))
        out.append((geom, "f16x3", li, nb, tuple(1e-7 if j < n else 1.0 for j in range(4))))
    return out


def exact_cases():
    """(clip size, format, level, clips) of the integer variant: every level of the sizes whose programs differ."""
    out = []
    for geom, fmts in ((G_A, ("f16x3",)), (G_B, ("f16x3", "bf16x3")), (G_C, ("f16x3",)), (SMALL, ("f16x3", "bf16x3"))):
        out += [(geom, fmt, li, nb) for li, nb in ((0, 3), (1, 9), (2, 9)) for fmt in fmts]
    return out + [(ODD, "f16x3", 2, 9), (FULL, "f16x3", 0, 2)]


# ------------------------------------------------------------------------------------------------------------------------ reference
def dense(g, am, geom, li, layout):
    """fp64 P^T g on the conv grid (nb, cout, T, OH, OW) by index arithmetic."""
    return _dense_gradient(g, am, layer_dims(geom, li), layout)


def conv_t(dy, w, in_shape):
    """fp64 autograd of F.conv3d with respect to its input."""
    xin = torch.zeros(in_shape, dtype=torch.float64, requires_grad=True)
    (out,) = torch.autograd.grad(F.conv3d(xin, w.double(), None, stride=R.CONV_STRIDE, padding=R.CONV_PAD), xin, dy.double())
    return out


def _pooled_keep(am, geom, li, layout, shape, mask):
    """0 / 1 per pooled element: 1 where its arg-max position lies inside ``mask`` (T, OH, OW) of the conv grid."""
    ids = torch.arange(1, int(np.prod(shape)) + 1, dtype=torch.float64).reshape(shape)
    where = dense(ids, am, geom, li, layout)                     # the id of the pooled element that lands on each conv position
    hit = where[mask.expand_as(where) & (where > 0)].long() - 1
    keep = torch.zeros(int(np.prod(shape)))
    keep[hit] = 1.0
    return keep.reshape(shape)


@functools.lru_cache(maxsize=12)
def case(geom, li, nb, pattern="full", mags=ONES, kind="random"):
    """Inputs and fp64 reference of one level; shared by the formats.  ``kind`` "exact": small integers and k/64 everywhere."""
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = layer_dims(geom, li)
    layout = 0 if li == 2 else 1
    exact = kind == "exact"
    gen = torch.Generator().manual_seed((40000 if exact else 20000) + 1000 * li + nb + sum(geom))
    shape = (nb, cout, To, Ho, Wo) if layout == 0 else (nb, To, Ho, Wo, cout)
    src_shape = (nb, cin, t, h, w)
    thin = lambda: (torch.rand(src_shape, generator=gen) >= 1.0 / 3.0)          # noqa: E731
    m_ab, m_g1, m_v, m_gb = mags
    if exact:
        assert mags == ONES
        ab = torch.randint(-3, 4, shape, generator=gen).float()
        g1 = torch.randint(-3, 4, shape, generator=gen).float()
        W = (torch.randint(-4, 5, (cout, cin, 3, 7, 7), generator=gen).float() / 64.0).contiguous()
        V = (torch.randint(-4, 5, (cout, cin, 3, 7, 7), generator=gen).float() / 64.0).contiguous()
        a = torch.randint(-3, 4, src_shape, generator=gen).float() if li == 0 else torch.randint(0, 4, src_shape, generator=gen).float() * thin()
        gbar = torch.randint(-3, 4, src_shape, generator=gen).float() if li else None
    else:
        ab = torch.randn(shape, generator=gen) * m_ab
        g1 = torch.randn(shape, generator=gen) * m_g1
        W = R.init_params(11)[2 * li].contiguous()
        V = (R.init_params(23)[2 * li] * m_v).contiguous()
        a = torch.randn(src_shape, generator=gen) if li == 0 else torch.randn(src_shape, generator=gen).abs() * thin()
        gbar = (torch.randn(src_shape, generator=gen) * m_gb) if li else None
    am = AO.argmax_bytes(277 + li + nb, (nb, cout, To, Ho, Wo) if layout == 0 else (nb, cout // 8, To, Ho, Wo, 8), pt)
    assert bool((am & 0x80 != 0).any()) and bool((am & 0x80 == 0).any()), "live and ReLU-dead windows"
    if pattern == "last":          # the incoming adjoint only in the last pooled row and column: the ragged boxes
        keep = torch.zeros(Ho, Wo)
        keep[Ho - 1, :] = 1
        keep[:, Wo - 1] = 1
        ab = (ab * (keep[None, None, None] if layout == 0 else keep[None, None, :, :, None])).contiguous()
    elif pattern == "dzshell":     # dz only on the border shell of the conv grid: the padding taps and box edges of the accumulating launch
        g1 = (g1 * _pooled_keep(am, geom, li, layout, shape, PG.shell_mask(T, OH, OW))).contiguous()
    else:
        assert pattern == "full"
    zb, dz = dense(ab, am, geom, li, layout), dense(g1, am, geom, li, layout)
    if pattern == "dzshell":
        assert bool((dz[:, :, ~PG.shell_mask(T, OH, OW)] == 0).all()) and bool((dz != 0).any())
    t1, t2 = conv_t(zb, W, src_shape), conv_t(dz, V, src_shape)
    w1 = PG.weight_gradient(a, zb)
    w2 = PG.weight_gradient(gbar, dz) if li else torch.zeros_like(w1)
    hb, hb_terms = zb.sum(dim=(0, 2, 3, 4)), zb.abs().sum(dim=(0, 2, 3, 4))
    if exact:
        hw0 = torch.randint(-3, 4, w1.shape, generator=gen).float()
        hb0 = torch.randint(-3, 4, (cout,), generator=gen).float()
    else:          # (at the gradients' magnitude: an fp32 sum keeps 2^-24 of its LARGER term)
        hw0 = torch.randn(w1.shape, generator=gen) * (float((w1 + w2).pow(2).mean().sqrt()) / 8.0)
        hb0 = torch.randn(cout, generator=gen) * m_ab
    assert bool((hw0 != 0).any()) and bool((hb0 != 0).any())
    c = SimpleNamespace(geom=geom, li=li, nb=nb, pattern=pattern, mags=mags, kind=kind, layout=layout, ab=ab, g1=g1, am=am, W=W, V=V,
                        a=a, gbar=gbar, hw0=hw0.contiguous(), hb0=hb0.contiguous(), t1=t1, t2=t2, w1=w1, w2=w2, hb=hb, hb_terms=hb_terms)
    if exact:
        c.partial_sum_bounds = _partial_sum_bounds(c, zb, dz)
    return c


def _partial_sum_bounds(c, zb, dz):
    """Upper bounds, from the fp64 dense zb / dz, of every partial sum of ABSOLUTE terms of an exact case, in units of the results'
    quantum (2^-6 for abar, 1 for hv_w and hv_b): -> (abar, hv_w, hv_b).  abar: max |zb| x the largest absolute row sum of W over
    (cout, taps), the same for dz and V.  hv_w: per output channel, max |a| x sum |zb| + max |gbar| x sum |dz| + max |start|."""
    rows = lambda wt: float(wt.double().abs().sum(dim=(0, 2, 3, 4)).max())          # noqa: E731
    abar = 64.0 * (float(zb.abs().max()) * rows(c.W) + float(dz.abs().max()) * rows(c.V))
    per = lambda v: v.abs().sum(dim=(0, 2, 3, 4))                                     # noqa: E731
    hv_w = float((float(c.a.abs().max()) * per(zb) + (float(c.gbar.abs().max()) if c.li else 0.0) * per(dz)).max()) + float(c.hw0.abs().max())
    hv_b = float(per(zb).max()) + float(c.hb0.abs().max())
    return abar, hv_w, hv_b


def is_exact_in_fp32(c):
    """The 2^24 condition: every partial sum of every accumulation order is an integer multiple of the quantum below 2^24."""
    q = (c.t1 + c.t2) * 64.0
    ok = bool((q == q.round()).all()) and bool(((c.w1 + c.w2) == (c.w1 + c.w2).round()).all()) and bool((c.hb == c.hb.round()).all())
    return ok and all(b < 2.0 ** 24 for b in c.partial_sum_bounds)


# ------------------------------------------------------------------------------------------------------ output buffers and checkers
def abar_buffer(geom, li, nb):
    """NaN-filled fp32 output of nb clips with one guard clip behind them, in the level's layout: pixels (clip, t, cin, h, w) at
    level 0, channels-last (clip, t, h, w, cin) above."""
    cin, _, t, h, w = layer_dims(geom, li)[:5]
    return torch.full((nb + 1, t, cin, h, w) if li == 0 else (nb + 1, t, h, w, cin), float("nan"), dtype=torch.float32)


def to_abar_layout(v, li):
    """(nb, cin, t, h, w) -> the level's output layout."""
    return (v.permute(0, 2, 1, 3, 4) if li == 0 else v.permute(0, 2, 3, 4, 1)).contiguous()


def written_abar(buf, li, nb):
    """Every element of the nb clips is written, the guard clip is still NaN -> (nb, cin, t, h, w) fp64."""
    assert buf.shape[0] == nb + 1
    assert bool(torch.isnan(buf[nb]).all()), "level %d wrote behind its last clip" % li
    left = int(torch.isnan(buf[:nb]).sum())
    assert left == 0, "level %d left %d of %d output elements unwritten (or wrote NaN)" % (li, left, buf[:nb].numel())
    got = buf[:nb].double()
    return got.permute(0, 2, 1, 3, 4) if li == 0 else got.permute(0, 4, 1, 2, 3)


def guarded(start, extra):
    """``start`` at the front of a NaN-filled flat fp32 allocation."""
    big = torch.full((start.numel() + extra,), float("nan"), dtype=torch.float32)
    big[:start.numel()] = start.reshape(-1)
    return big


def written_front(big, start, what):
    """The tail is still NaN and the front finite -> front - start, fp64, in ``start``'s shape."""
    n = start.numel()
    assert bool(torch.isnan(big[n:]).all()), "wrote behind %s" % what
    assert bool(torch.isfinite(big[:n]).all()), "%s is not finite" % what
    return big[:n].view(start.shape).double() - start.double()


def _ratio(err, allow):
    return 0.0 if err == 0.0 else (float("inf") if allow == 0.0 else err / allow)


def abar_ratios(got, c, fmt):
    """Per clip and input parity class (h % 2, w % 2), whole and on the border shell: error over allowance (module docstring), and
    the largest absolute error over 4 B x the largest reference element.  -> (worst of each, where, worst error over
    ||t1|| + ||t2||: the figure that compares with B)"""
    B = BOUND[fmt]
    want = c.t1 + c.t2
    nb, _, t, h, w = want.shape
    shell = PG.shell_mask(t, h, w)
    worst, where, rel = [0.0, 0.0, 0.0], [None, None, None], 0.0
    for b in range(nb):
        for ph in range(min(2, h)):
            for pw in range(min(2, w)):
                sub = lambda v: v[b][:, :, ph::2, pw::2]          # noqa: E731
                d, r, a1, a2 = sub(got) - sub(want), sub(want), sub(c.t1), sub(c.t2)
                s = shell[:, ph::2, pw::2].expand_as(r)
                vals = (_ratio(float(d.norm()), B * (float(a1.norm()) + float(a2.norm())) + U32 * float(r.norm())),
                        _ratio(float(d[s].norm()), B * (float(a1[s].norm()) + float(a2[s].norm())) + U32 * float(r[s].norm())),
                        _ratio(float(d.abs().max()), 4.0 * B * float(r.abs().max())))
                rel = max(rel, _ratio(float(d.norm()), float(a1.norm()) + float(a2.norm())))
                for k, v in enumerate(vals):
                    if not v <= worst[k]:
                        worst[k], where[k] = v, (b, ph, pw)
    return worst, where, rel


def check_abar(got, c, fmt, label="", record=None):
    worst, where, rel = abar_ratios(got, c, fmt)
    if record is not None:
        record[0] = max(record[0], rel)
        for k in range(3):
            record[k + 1] = max(record[k + 1], worst[k])
    print("down sweep %s level %d %s: abar error / allowance %.3f at (clip, ph, pw) %s, border shell %.3f at %s, max-abs %.3f at %s; "
          "error / (|t1| + |t2|) %.2e against B = %.1e | so far %s" % (fmt, c.li, label, worst[0], where[0], worst[1], where[1], worst[2],
                                                                       where[2], rel, BOUND[fmt], ["%.2e" % v for v in record] if record else "-"))
    assert worst[0] <= 1.0, ("abar", worst[0], where[0])
    assert worst[1] <= 1.0, ("abar, border shell", worst[1], where[1])
    assert worst[2] <= 1.0, ("abar, max-abs", worst[2], where[2])
    return worst


def _families(v):
    cout, cin = v.shape[:2]
    return {"whole": v.reshape(1, -1), "tap": v.reshape(cout * cin, 147).t(), "cout": v.reshape(cout, -1),
            "cin": v.permute(1, 0, 2, 3, 4).reshape(cin, -1)}


def hv_w_ratios(dw, c, fmt):
    """``dw`` = hv_w - start.  Per slice of the four families of tests/param_gradient_cases.py: ||dw - want|| over
    BAR (||w1|| + ||w2||) + 2^-24 ||want||; a slice that is zero in both terms must be exactly zero.  -> {family: (worst, index)}"""
    want = c.w1 + c.w2
    fd, f1, f2, fw = _families(dw.double() - want), _families(c.w1), _families(c.w2), _families(want)
    out = {}
    for k in PG.FAMILIES:
        en, n1, n2, nw = fd[k].norm(dim=1), f1[k].norm(dim=1), f2[k].norm(dim=1), fw[k].norm(dim=1)
        dead = (n1 == 0) & (n2 == 0)
        assert bool((en[dead] == 0).all()), "%s slices %s are zero in both terms and not in the result" % (k, torch.nonzero(dead & (en != 0)).flatten().tolist())
        allow = BAR[fmt] * (n1 + n2) + U32 * nw
        ratio = torch.where(en == 0, torch.zeros_like(en), en / allow)
        assert not bool(torch.isnan(ratio).any()), k
        i = int(ratio.argmax())
        out[k] = (float(ratio[i]), i)
    return out


def check_hv_w(dw, c, fmt, label="", record=None):
    ratios = hv_w_ratios(dw, c, fmt)
    rel, zeros = PG.slice_errors(dw, c.w1 + c.w2)          # (its own zero-slice assertion, and the rel-L2 figures of the predecessor)
    if record is not None:
        for k in PG.FAMILIES:
            record[k] = max(record.get(k, 0.0), rel[k][0])
    print("down sweep %s level %d %s: hv_w error / allowance %s | rel-L2 %s | zero slices %s" % (
        fmt, c.li, label, ", ".join("%s %.3f at %d" % (k, ratios[k][0], ratios[k][1]) for k in PG.FAMILIES),
        ", ".join("%.2e" % rel[k][0] for k in PG.FAMILIES), {k: v for k, v in zeros.items() if v}))
    for k in PG.FAMILIES:
        assert ratios[k][0] <= 1.0, ("hv_w", k, ratios[k])
    return ratios


def hv_b_ratio(db, c):
    """``db`` = hv_b - start.  |db - sum zb| over gamma(k) x (sum |zb| + |start|): a workgroup of vd_bias_grad_pooled owns 256 pooled
    positions of one clip (<= 256 adds), then one atomic add per (clip, block) onto hv_b
    (tests/test_gpu_aux_kernels.py::test_bias_grad_pooled)."""
    To, Ho, Wo = layer_dims(c.geom, c.li)[8:11]
    rows = c.nb * (-(-(To * Ho * Wo) // 256))
    bound = AO.gamma(256 + rows) * (c.hb_terms + c.hb0.double().abs())
    err = (db.double() - c.hb).abs()
    assert bool((err[bound == 0] == 0).all())
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def check_hv_b(db, c, label=""):
    r = hv_b_ratio(db, c)
    print("down sweep level %d %s: hv_b worst |error| / bound %.3f" % (c.li, label, r))
    assert r <= 1.0, ("hv_b", r)
    return r


# ----------------------------------------------------------------------------------------------------------------- the format floor
def pow2_scale(absmax, target):
    """The power of two vd_absmax_scale chooses: the largest 2^k with absmax x 2^k < target (1 for an all-zero tensor)."""
    if absmax == 0.0:
        return 1.0
    fm, em = math.frexp(absmax)
    ft, et = math.frexp(target)
    return 2.0 ** max(-126, min(126, et - em - (0 if ft > fm else 1)))


def scales(c, fmt):
    """The scales the engine would choose: zscale, gscale (engine.GRAD_TARGET), vscale and sscale = min(scale of gbar, vscale)
    (train.GradMatchEngine.V_TARGET); bf16x3 runs unscaled."""
    if fmt != "f16x3":
        return SimpleNamespace(z=1.0, g=1.0, v=1.0, s=1.0)
    sv = pow2_scale(float(c.V.abs().max()), V_TARGET)
    ss = min(pow2_scale(float(c.gbar.abs().max()), V_TARGET), sv) if c.li else 1.0
    return SimpleNamespace(z=pow2_scale(float(c.ab.abs().max()), GRAD_TARGET), g=pow2_scale(float(c.g1.abs().max()), GRAD_TARGET), v=sv, s=ss)


def floor(c, fmt):
    """What the operand FORMAT alone costs the case: fp64 arithmetic on the operands as held after the hi+lo split at the scales
    the engine would choose (f16x3 weights under their x 2^8 shift), every stored or accumulated result rounded to fp32.
    -> (abar ratios, hv_w ratios, hv_b ratio) as the checkers compute them"""
    sc, ws = scales(c, fmt), WSHIFT.get(fmt, 1.0)
    zb = PG.rounded(dense(c.ab, c.am, c.geom, c.li, c.layout).float(), fmt, sc.z)
    dz = PG.rounded(dense(c.g1, c.am, c.geom, c.li, c.layout).float(), fmt, sc.g)
    W = PG.rounded(c.W, fmt, ws)
    V = PG.rounded((c.V * sc.v).contiguous(), fmt, ws) / sc.v
    f32 = lambda v: v.float().double()          # noqa: E731
    abar = f32(f32(conv_t(zb, W, c.a.shape)) + conv_t(dz, V, c.a.shape))
    hw = f32(c.hw0.double() + PG.weight_gradient(PG.rounded(c.a, fmt), zb))
    if c.li:
        hw = f32(hw + PG.weight_gradient(PG.rounded(c.gbar, fmt, sc.s), dz))
    hb = f32(c.hb0.double() + zb.sum(dim=(0, 2, 3, 4)))
    return abar_ratios(abar, c, fmt)[0], hv_w_ratios(hw - c.hw0.double(), c, fmt), hv_b_ratio(hb - c.hb0.double(), c)


# ------------------------------------------------------------------------------------------------------------ the exactly-once count
def bwd_plans(geom, batch_hint=None, bwd0_small=True):
    """The input-gradient plans of the hi+lo engines, built as ``EmbedEngine`` builds them (TrainEngine / GradMatchEngine pass
    bwd0_small=True, a plain EmbedEngine does not)."""
    from video_distillation_amd import plan
    return plan.plan_network(plan.NetGeometry(*geom), ntw=2, ntw0=1, balanced=False, batch_hint=batch_hint, bwd0_small=bwd0_small)["bwd"]


def plan_identity(pl):
    return pl.name, pl.MTW, np.asarray(pl.boxes).tolist()


def count_named(pl, nclips, count):
    """Adds to ``count`` (flat, nclips x elements per clip) how often the row-output epilogue of ``pl`` names each output element,
    walking ``flat_tables()`` and ``boxes`` over the clip groups as tests/emulate.py::run_plan does."""
    descs, tables = pl.flat_tables()
    n = np.arange(pl.NT * 32)
    valid = n < pl.n_out
    coff = (np.asarray(pl.col_off)[n[valid]] if pl.col_off is not None else n[valid] * pl.n_stride).astype(np.int64)
    named = []
    for grp in range(-(-nclips // pl.ncl)):
        clip0 = grp * pl.ncl
        for box in np.asarray(pl.boxes):
            ty, out_rel = int(box[0]), int(box[4])
            mt, o_ofs = int(descs[ty][6]), int(descs[ty][8])
            o = tables[o_ofs:o_ofs + mt * 32].astype(np.int64)
            o = o[o >= 0]
            o = o[clip0 + o // pl.out_clip_stride < nclips]
            idx = (clip0 * pl.out_clip_stride + out_rel + o)[:, None] + coff[None, :]
            assert idx.size == 0 or (idx.min() >= 0 and idx.max() < count.size), "%s names an element outside the %d clips" % (pl.name, nclips)
            named.append(idx.reshape(-1))
    if named:
        count += np.bincount(np.concatenate(named), minlength=count.size).astype(count.dtype)
    return count


def named_counts(plans, geom, li, nclips):
    """-> (count over all programs of the level, [count per program])"""
    cin, _, t, h, w = layer_dims(geom, li)[:5]
    per = [count_named(pl, nclips, np.zeros(nclips * cin * t * h * w, dtype=np.int32)) for pl in plans]
    return sum(per), per
