"""Seeded inputs, fp64 references, layout helpers and the checker of ONE forward level (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_gpu_forward_level.py (a level's tile program alone on the device) and tests/test_forward_level_cpu.py (what
the operand formats alone cost, that the exact cases are exact, that the checker catches what it is for), so that both speak
about the same data.  torch on the CPU only.

A level is Conv3d(stride (1,2,2), padding (1,3,3)) + bias, then ReLU and MaxPool3d((pool_t,2,2)) -- in the kernel's order: the
maximum of the window first (bias is per channel, ReLU monotone).  The reference is fp64 ``F.conv3d`` and, per pooled window
(positions enumerated dt*4 + dh*2 + dw as tests/argmax_tools.py::oracle_windows does): the FIRST maximum, its index, its margin
to the second, and the dead flag ``max + bias <= 0``.

Two kinds of inputs.  RANDOM: randn clips at level 0, half-normal values with a third exact zeros above (every source there is the
output of a ReLU and pool); weights of ``oracle.ref_cpu.init_params``; its biases scaled to max |b| = 2 x rms of the conv output,
so that a visible share of the windows is dead.  EXACT: integer pixels in -3..3 (0..3 with a third zeros above level 0), weights
k/64 with |k| <= 4, biases j/64 with |j| <= 64 -- every operand is exact in bf16, in fp16 and under the x 2^8 weight shift of
VD_PREC_F16X3, and every partial sum of every accumulation order is a multiple of 2^-6 below 18816 * 3 * 4 / 64 = 3528, far inside
fp32's 24 bits: the device result must EQUAL the fp64 one, in every format.  ``exact_case`` asserts that per case from
conv(|x|, |w|).  Ties between window elements are frequent in such data (and three channels whose weights are a single tap hold
them in most windows); outputs of exactly zero are planted (the bias of every fourth channel is minus one of that channel's window
maxima where one lies in [-1, 1]).
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import aux_oracle as AO

G_A, G_B, G_C = (4, 64, 66), (4, 65, 63), (4, 70, 58)
SMALL, ODD, FULL = (8, 64, 64), (12, 96, 80), (16, 112, 112)
M7 = (4, 104, 112)          # a small clip size whose level 1 plans to the 7-tile families (3 boxes; 112 x 112 x 16: 14)

PREC = {"f16x3": AO.PREC_F16X3, "bf16x3": AO.PREC_BF16X3, "f16": AO.PREC_F16, "bf16": AO.PREC_BF16}
WSHIFT = {"f16x3": 256.0}                     # hip.F16X3_WSHIFT: the packed fp16 hi+lo weights are W x 2^8
SENT16, SENT_AM = 0x7FFF, 0x55                # a NaN in fp16 and in bf16; a byte with bits 4 and 6 set: no program writes either
TIE_TOL = 2e-5                                # tests/argmax_tools.py::compare_decisions

# what the project holds a single conv program to against fp64 (tests/test_gpu_wgrad.py, tests/test_gpu_embed.py): the STARTING point of
# tests/test_gpu_forward_level.py's bounds
BAR = {"f16x3": 2e-5, "bf16x3": 1e-4, "f16": 2e-3, "bf16": 2e-2}
# ... and the bounds derived from it by the rule and the measurements in that module's docstring (rel-L2; max-abs ratio 4 x)
BOUND = {"f16x3": 3.2e-6, "bf16x3": 1.4e-5, "f16": 2e-3, "bf16": 2e-2}


def planes_of(fmt):
    return 2 if AO.has_lo(PREC[fmt]) else 1


def layer_dims(geom, li):
    from video_distillation_amd import plan
    return plan.NetGeometry(*geom).layer_dims()[li]


# ------------------------------------------------------------------------------------------------------------ layout helpers
def to_slots(x, fmt, planes=None):
    """fp32 (nb, C, t, h, w) -> the channels-last operand slots [planes][nb * per][8] int16 a level reads, per = C/8 * t * h * w,
    slot order [clip][C/8][t][h][w][8]."""
    nb, C, t, h, w = x.shape
    cl = x.reshape(nb, C // 8, 8, t, h, w).permute(0, 1, 3, 4, 5, 2).contiguous()
    hi, lo = AO.split16(cl, PREC[fmt])
    return torch.stack([hi, lo][:planes or planes_of(fmt)]).reshape(-1, nb * (C // 8) * t * h * w, 8).contiguous()


def from_slots(slots, nb, C, t, h, w):
    """The inverse for the first nb clips of [planes][>= nb * per][8] (16-bit planes), or of a flat byte array in the same slot
    order (arg-max bytes): -> (planes, nb, C, t, h, w), resp. (nb, C, t, h, w)."""
    per = (C // 8) * t * h * w
    if slots.dim() == 1:
        return slots[:nb * per * 8].reshape(nb, C // 8, t, h, w, 8).permute(0, 1, 5, 2, 3, 4).reshape(nb, C, t, h, w)
    P = slots.shape[0]
    return slots[:, :nb * per].reshape(P, nb, C // 8, t, h, w, 8).permute(0, 1, 2, 6, 3, 4, 5).reshape(P, nb, C, t, h, w)


def bytes_to_slots(a):
    """(nb, C, t, h, w) bytes -> flat, slot order."""
    nb, C, t, h, w = a.shape
    return a.reshape(nb, C // 8, 8, t, h, w).permute(0, 1, 3, 4, 5, 2).reshape(-1).contiguous()


def to_feat(v):
    """(nb, C, T, H, W) -> (nb, C * T * H * W): the feature order of the last level."""
    return v.reshape(v.shape[0], -1).contiguous()


def from_feat(f, nb, C, t, h, w):
    return f.reshape(-1)[:nb * C * t * h * w].reshape(nb, C, t, h, w)


def decode(bits, fmt):
    """(planes, ...) int16 -> the fp64 value hi (+ lo)."""
    return sum(AO.decode16(b.contiguous(), PREC[fmt]) for b in bits)


def no_negative_zero(bits):
    """16-bit patterns with -0 (0x8000) written as +0: the one freedom of a bit-for-bit comparison."""
    return torch.where(bits == -32768, torch.zeros_like(bits), bits)


# --------------------------------------------------------------------------------------------------------------- reference
def conv64(x, w):
    return F.conv3d(x.double(), w.double(), None, stride=R.CONV_STRIDE, padding=R.CONV_PAD)


def windows(z, pt):
    """(nb, C, T, OH, OW) -> (nb, C, To, Ho, Wo, pt * 4), window elements in the order dt*4 + dh*2 + dw."""
    nb, C, T, H, W = z.shape
    To, Ho, Wo = T // pt, H // 2, W // 2
    w = z[:, :, :To * pt, :Ho * 2, :Wo * 2].reshape(nb, C, To, pt, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 6, 3, 5, 7)
    return w.reshape(nb, C, To, Ho, Wo, pt * 4)


def reference(z0, bias, pt):
    """fp64 conv output WITHOUT bias and the bias -> win (windows of z0 + bias), top (first maximum), idx (its index), margin (to
    the second), dead (top <= 0), value (the level's output: top, or 0 where dead), rms (of the conv output with bias)."""
    z = z0 + bias.double().view(1, -1, 1, 1, 1)
    win = windows(z, pt)
    top2 = win.topk(2, dim=-1).values
    top = top2[..., 0]
    K = win.shape[-1]
    idx = torch.where(win == top.unsqueeze(-1), torch.arange(K), torch.full((), K, dtype=torch.int64)).min(dim=-1).values
    dead = top <= 0
    return SimpleNamespace(win=win, top=top, idx=idx, margin=top2[..., 0] - top2[..., 1], dead=dead,
                           value=torch.where(dead, torch.zeros_like(top), top), rms=float(z.pow(2).mean().sqrt()), pt=pt)


def winners_cover_the_grid(ref):
    """Every conv position of the pooled part of the grid is the winner of a LIVE window of at least one channel, in every clip:
    pooling then hides no position from a comparison of the level's output."""
    won = F.one_hot(ref.idx, ref.win.shape[-1]).bool() & (~ref.dead).unsqueeze(-1)
    return bool(won.any(dim=1).all())


def _gen(geom, li, nb, salt):
    return torch.Generator().manual_seed(salt + 1000 * li + nb + sum(geom))


@functools.lru_cache(maxsize=None)
def random_case(geom, li, nb, seed=11):
    """-> x (nb, cin, t, h, w) fp32, w, b fp32, ref"""
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = layer_dims(geom, li)
    gen = _gen(geom, li, nb, 7000)
    x = torch.randn(nb, cin, t, h, w, generator=gen)
    if li > 0:
        x = x.abs() * (torch.rand(x.shape, generator=gen) >= 1.0 / 3.0)
    p = R.init_params(seed)
    wt, b = p[2 * li].contiguous(), p[2 * li + 1]
    z0 = conv64(x, wt)
    b = (b * (2.0 * float(z0.pow(2).mean().sqrt()) / float(b.abs().max()))).contiguous()
    ref = reference(z0, b, pt)
    assert bool(ref.dead.any()) and bool((~ref.dead).any()), "both live and dead windows"
    assert 0.02 < float(ref.dead.double().mean()) < 0.7, float(ref.dead.double().mean())
    assert winners_cover_the_grid(ref), "a conv position wins nowhere"
    return SimpleNamespace(x=x, w=wt, b=b, ref=ref, z0=z0, kind="random", geom=geom, li=li, nb=nb)


@functools.lru_cache(maxsize=None)
def exact_case(geom, li, nb):
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = layer_dims(geom, li)
    gen = _gen(geom, li, nb, 9000)
    if li == 0:
        x = torch.randint(-3, 4, (nb, cin, t, h, w), generator=gen).float()
    else:
        x = torch.randint(0, 4, (nb, cin, t, h, w), generator=gen).float() * (torch.rand((nb, cin, t, h, w), generator=gen) >= 1.0 / 3.0)
    wt = (torch.randint(-4, 5, (cout, cin, 3, 7, 7), generator=gen).float() / 64.0).contiguous()
    if li > 0:          # two channels with weights |k|/64 on non-negative pixels: sums of some hundreds, whose fp16 image needs the low plane too
        wt[2], wt[cout - 2] = wt[2].abs(), wt[cout - 2].abs()
    b = torch.randint(-64, 65, (cout,), generator=gen).float() / 64.0
    # tie channels: three output channels see ONE tap of ONE input channel -- their conv values are 4/64 resp. -3/64 x a pixel, four
    # or seven levels: most of their windows hold tied maxima at varying positions, whatever the size of the case
    for c, k in ((1, 4.0), (cout - 3, -3.0), (5, -3.0)):
        wt[c] = 0.0
        wt[c, 0, 1, 3, 3] = k / 64.0
    # the sum condition: every partial sum of every order is bounded by the sum of the absolute terms
    bound = float(conv64(x.abs(), wt.abs()).max()) + 1.0
    assert bound * 64.0 < 2.0 ** 24, bound
    z0 = conv64(x, wt)
    assert bool((z0 * 64.0 == (z0 * 64.0).round()).all()), "the fp64 reference is no multiple of 2^-6"
    # planted zeros: every fourth channel's bias is minus one of its window maxima, where one lies within the biases' range
    m0 = windows(z0, pt).max(dim=-1).values.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    for c in range(0, cout, 4):
        cand = m0[c][m0[c].abs() <= 1.0]
        if cand.numel():
            b[c] = -float(cand[cand.numel() // 2])
    b[1] = b[cout - 3] = 0.5          # (the tie channels are live: their conv values are >= 0 resp. <= 0 above level 0, small at it)
    b[5] = 0.0                        # ... and a third one's maximum is exactly zero wherever its window sees a zero pixel
    b = b.contiguous()
    assert bool((b * 64.0 == (b * 64.0).round()).all()) and float(b.abs().max()) <= 1.0
    ref = reference(z0, b, pt)
    assert bool((ref.margin == 0).any()), "no window with tied maxima"
    assert bool((ref.top == 0).any()), "no output of exactly zero"
    assert bool(ref.dead.any()) and bool((~ref.dead).any())
    assert winners_cover_the_grid(ref), "a conv position wins nowhere"
    for fmt in ("f16x3", "bf16x3"):          # the hi+lo formats hold the level's output without rounding
        v32 = ref.value.float()
        assert torch.equal(decode(torch.stack(AO.split16(v32, PREC[fmt])), fmt), ref.value), fmt
    return SimpleNamespace(x=x, w=wt, b=b, ref=ref, z0=z0, kind="exact", geom=geom, li=li, nb=nb)


def get_case(kind, geom, li, nb):
    return exact_case(geom, li, nb) if kind == "exact" else random_case(geom, li, nb)


# ----------------------------------------------------------------------------------------- a level's output and its checker
def output_buffers(dims, li, nb, planes, with_argmax):
    """The sentinel-filled buffers of nb clips and one guard clip behind them (CPU tensors; the GPU test moves them to the device):
    16-bit planes [planes][(nb + 1) * per][8] (0x7FFF) below the last level, fp32 features (nb + 1, C * To * Ho * Wo) (NaN) at it,
    arg-max bytes (0x55)."""
    cout, To, Ho, Wo = dims[1], dims[8], dims[9], dims[10]
    n = cout * To * Ho * Wo
    out = SimpleNamespace(planes=None, feat=None, am=None)
    if li == 2:
        out.feat = torch.full((nb + 1, n), float("nan"), dtype=torch.float32)
    else:
        out.planes = torch.full((planes, (nb + 1) * (n // 8), 8), SENT16, dtype=torch.int16)
    if with_argmax:
        out.am = torch.full(((nb + 1) * n,), SENT_AM, dtype=torch.uint8)
    return out


def perfect_output(case, fmt, planes, with_argmax):
    """What an exact device would leave in ``output_buffers`` for this case (the CPU test corrupts it, one element at a time)."""
    dims = layer_dims(case.geom, case.li)
    out = output_buffers(dims, case.li, case.nb, planes, with_argmax)
    v32 = case.ref.value.float()
    if case.li == 2:
        out.feat[:case.nb] = to_feat(v32)
    else:
        s = to_slots(v32, fmt, planes)
        out.planes[:, :s.shape[1]] = s
    if with_argmax:
        a = (case.ref.idx | (case.ref.dead.long() << 7)).to(torch.uint8)
        flat = a.reshape(-1) if case.li == 2 else bytes_to_slots(a)
        out.am[:flat.numel()] = flat
    return out


def check_written(out, dims, li, nb):
    """The guard clip is untouched; no sentinel remains in any element the nb clips own, in any plane; every arg-max byte has bits
    3..6 clear, and bit 2 as well where the level does not pool frames."""
    cout, To, Ho, Wo, pt = dims[1], dims[8], dims[9], dims[10], dims[11]
    n = cout * To * Ho * Wo
    if out.planes is not None:
        per = n // 8
        assert out.planes.shape[1] == (nb + 1) * per
        assert bool((out.planes[:, nb * per:] == SENT16).all()), "level %d wrote behind its last clip" % li
        left = int((out.planes[:, :nb * per] == SENT16).sum())
        assert left == 0, "level %d left %d 16-bit elements unwritten" % (li, left)
    if out.feat is not None:
        assert bool(torch.isnan(out.feat[nb:]).all()), "level %d wrote behind its last clip's features" % li
        left = int(torch.isnan(out.feat[:nb]).sum())
        assert left == 0, "level %d left %d features unwritten (or wrote NaN)" % (li, left)
    if out.am is not None:
        assert bool((out.am[nb * n:] == SENT_AM).all()), "level %d wrote arg-max bytes behind its last clip" % li
        a = out.am[:nb * n]
        bad = int(((a & (0x78 if pt == 2 else 0x7C)) != 0).sum())
        assert bad == 0, "level %d: %d arg-max bytes unwritten or with bits outside the position and the dead flag" % (li, bad)


def decoded(out, dims, li, nb, fmt):
    """-> (value fp64 (nb, C, To, Ho, Wo), 16-bit planes (planes, nb, C, To, Ho, Wo) or None, (position, dead flag) or None)"""
    cout, To, Ho, Wo = dims[1], dims[8], dims[9], dims[10]
    if li == 2:
        bits, value = None, from_feat(out.feat, nb, cout, To, Ho, Wo).double()
    else:
        bits = from_slots(out.planes, nb, cout, To, Ho, Wo)
        value = decode(bits, fmt)
    dec = None
    if out.am is not None:
        a = (out.am[:nb * cout * To * Ho * Wo].reshape(nb, cout, To, Ho, Wo) if li == 2 else from_slots(out.am, nb, cout, To, Ho, Wo)).long()
        dec = (a & 7, (a & 0x80) != 0)
    return value, bits, dec


def check_exact(out, case, fmt):
    """(A) of tests/test_gpu_forward_level.py: the value, every 16-bit plane, the fp32 features, the live positions (first maximum,
    ties included) and the dead flags of an EXACT case, bit for bit."""
    dims = layer_dims(case.geom, case.li)
    li, nb, ref = case.li, case.nb, case.ref
    check_written(out, dims, li, nb)
    value, bits, dec = decoded(out, dims, li, nb, fmt)
    v32 = ref.value.float()
    if li == 2:
        assert torch.equal(value.float(), v32), "features: %d of %d differ from the fp64 value" % (int((value.float() != v32).sum()), v32.numel())
    else:
        want = torch.stack(AO.split16(v32, PREC[fmt]))[:bits.shape[0]]
        for k in range(bits.shape[0]):
            diff = no_negative_zero(bits[k]) != no_negative_zero(want[k])
            assert not bool(diff.any()), "%s plane of level %d: %d of %d elements differ from split16 of the fp64 value, first at %s" % (
                ("hi", "lo")[k], li, int(diff.sum()), diff.numel(), torch.nonzero(diff)[0].tolist())
        if bits.shape[0] == 2:           # hi + lo hold the value itself (exact_case asserts that the format can)
            assert torch.equal(value, ref.value), "level %d: hi + lo is not the fp64 value" % li
    if dec is not None:
        pos, dead = dec
        assert torch.equal(dead, ref.top <= 0), "level %d: %d dead flags differ from value <= 0" % (li, int((dead != (ref.top <= 0)).sum()))
        wrong = (~dead) & (pos != ref.idx)
        assert not bool(wrong.any()), "level %d: %d live windows do not record the FIRST maximum, first at %s" % (
            li, int(wrong.sum()), torch.nonzero(wrong)[0].tolist())


def shell_mask(To, Ho, Wo):
    """Pooled positions in the first or last frame, row or column."""
    tt, hh, ww = torch.arange(To), torch.arange(Ho), torch.arange(Wo)
    return (((tt == 0) | (tt == To - 1))[:, None, None] | ((hh == 0) | (hh == Ho - 1))[None, :, None]
            | ((ww == 0) | (ww == Wo - 1))[None, None, :])


def value_errors(got, want):
    """Per clip: rel-L2 of the whole output and of its border shell, largest absolute error over the largest reference element.
    -> the worst of each over the clips, and which clip"""
    nb, C, To, Ho, Wo = want.shape
    s = shell_mask(To, Ho, Wo).expand(C, To, Ho, Wo)
    worst, where = [0.0, 0.0, 0.0], [None, None, None]
    for b in range(nb):
        d, r = got[b] - want[b], want[b]
        vals = (float(d.norm() / r.norm()), float(d[s].norm() / r[s].norm()), float(d.abs().max() / r.abs().max()))
        for k, v in enumerate(vals):
            if not v <= worst[k]:
                worst[k], where[k] = v, b
    return worst, where


def compare_decisions(pos, dead, ref, tie_tol=TIE_TOL):
    """tests/argmax_tools.py::compare_decisions for one level: a live window routed otherwise, or a differing dead flag, counts as
    a near-tie when the reference's margin (top1 - top2, resp. |top1| for the flag) is below tie_tol x rms of the conv output.  In
    a dead window the position bits are not part of the contract."""
    flag_diff = dead != ref.dead
    pos_diff = (~dead) & (~ref.dead) & (pos != ref.idx)
    slack = torch.where(flag_diff, ref.top.abs(), ref.margin) / ref.rms
    mism = flag_diff | pos_diff
    return {"windows": int(mism.numel()), "mismatch": int(mism.sum()), "not_near_tie": int((mism & (slack > tie_tol)).sum()),
            "worst_margin": float(slack[mism].max()) if bool(mism.any()) else 0.0}


def routed_value(pos, dead, ref):
    """The fp64 conv value at the RECORDED position (0 where the window was recorded dead)."""
    sel = ref.win.gather(-1, pos.unsqueeze(-1)).squeeze(-1)
    return torch.where(dead, torch.zeros_like(sel), sel)


def check_random(out, case, fmt, bound, label="", record=None, ref=None, decisions_ref=None):
    """(B): the output as values against the free fp64 value (the maximum over a window is 1-Lipschitz: no routing allowance), and,
    with arg-max bytes, against the fp64 conv value at the recorded position, and the decisions against the near-tie rule
    (against ``decisions_ref`` where given: ``format_reference`` for the single-pass formats).
    rel-L2 whole / border shell / routed below ``bound``, max-abs ratio below 4 x ``bound``.  -> the decoded value"""
    dims = layer_dims(case.geom, case.li)
    li, nb = case.li, case.nb
    ref = ref or case.ref
    check_written(out, dims, li, nb)
    value, _, dec = decoded(out, dims, li, nb, fmt)
    assert bool(torch.isfinite(value).all())
    worst, where = value_errors(value, ref.value)
    figures = list(worst) + [0.0]
    text = ""
    if dec is not None:
        pos, dead = dec
        rw, _ = value_errors(value, routed_value(pos, dead, ref))
        figures[3] = max(rw[0], rw[1])
        stats = compare_decisions(pos, dead, decisions_ref or ref)
        text = " | at the recorded positions %.2e | routed otherwise %d of %d, no near-tie %d, worst margin %.1e" % (
            figures[3], stats["mismatch"], stats["windows"], stats["not_near_tie"], stats["worst_margin"])
        if decisions_ref is not None:
            free = compare_decisions(pos, dead, ref)
            text += " (against the unrounded operands: %d, %d, %.1e)" % (free["mismatch"], free["not_near_tie"], free["worst_margin"])
    if record is not None:
        for k in range(4):
            record[k] = max(record[k], figures[k])
    print("forward %s level %d %s: rel-L2 %.2e (clip %s), border shell %.2e (clip %s), max-abs ratio %.2e (clip %s)%s | so far %s" % (
        fmt, li, label, worst[0], where[0], worst[1], where[1], worst[2], where[2], text,
        ["%.2e" % v for v in record] if record is not None else "-"))
    assert worst[0] < bound, ("rel-L2", worst[0], where[0])
    assert worst[1] < bound, ("border shell rel-L2", worst[1], where[1])
    assert worst[2] < 4 * bound, ("max-abs ratio", worst[2], where[2])
    if dec is not None:
        assert figures[3] < bound, ("rel-L2 at the recorded positions", figures[3])
        assert stats["not_near_tie"] == 0, stats
    return value


def rounded(v, fmt, scale=1.0):
    """tests/param_gradient_cases.py::rounded for the four forward formats: fp32 values as the operand format holds them (hi, or
    hi + lo), in fp64; ``scale``: the power of two applied before rounding."""
    hi, lo = AO.split16((v * scale).contiguous(), PREC[fmt])
    return decode(torch.stack([hi, lo])[:planes_of(fmt)], fmt) / scale


_FORMAT_REFERENCES = {}


def format_reference(case, fmt):
    """The fp64 level on the operands AS THE FORMAT HOLDS THEM (hi, or hi + lo; f16x3 weights under their x 2^8 shift) and the fp32
    bias: what a program of that format is to compute, in exact arithmetic.  The near-tie rule of the single-pass formats is stated
    against it: their 11 resp. 8 operand bits alone move the conv values by 3e-4 resp. 2e-3 of their rms and route some 2e-4
    resp. 2e-3 of the windows otherwise, with margins up to 7e-4 resp. 6e-3 x rms -- tie_tol = 2e-5 x rms against the UNROUNDED
    operands is not attainable by any program of such a format (tests/test_forward_level_cpu.py asserts that), and is what the
    free and the routed value comparisons already cover: a window routed otherwise has margin <= the error of the value at the
    recorded position + the error at the reference's position.  Against the rounded operands only the fp32 accumulation is
    left, and tie_tol = 2e-5 stands."""
    key = (case.kind, case.geom, case.li, case.nb, fmt)
    if key not in _FORMAT_REFERENCES:
        z0 = conv64(rounded(case.x, fmt), rounded(case.w, fmt, WSHIFT.get(fmt, 1.0)))
        _FORMAT_REFERENCES[key] = reference(z0, case.b, case.ref.pt)
    return _FORMAT_REFERENCES[key]


def format_floor(case, fmt, out_fmt=None):
    """What the operand FORMAT alone costs: fp64 conv of the operands as the format holds them (hi, or hi + lo; f16x3 weights under
    their x 2^8 shift), the fp32 bias, and the output rounded to the level's output format (fp32 features at the last level).
    -> worst (rel-L2, border shell, max-abs ratio) over the clips against the free fp64 value"""
    out_fmt = out_fmt or fmt
    v32 = format_reference(case, fmt).value.float()
    got = v32.double() if case.li == 2 else decode(torch.stack(AO.split16(v32, PREC[out_fmt]))[:planes_of(out_fmt)], out_fmt)
    return value_errors(got, case.ref.value)[0]


# ------------------------------------------------------------------------------- (C) the select epilogue (train.GradMatchEngine.sel)
SELECT_BAR = {"f16x3": 2e-5, "bf16x3": 1e-4}          # the single-linear-program bars again: the starting point
SELECT_BOUND = {"f16x3": 4.4e-6, "bf16x3": 1.8e-5}    # ... and what the rule makes of them (tests/test_gpu_forward_level.py docstring)
SELECT_SCALE = 0.25                                   # the power-of-two out_scale of every select case


@functools.lru_cache(maxsize=None)
def select_case(geom, li, nb, kind):
    """One level of the upward sweep as the linear operator it is: sources a (activation-like; clips at level 0) and gbar (a signed
    tangent; none at level 0), operands V and W (packed as torch.cat([V, W], dim=1)), bias vb, arg-max bytes am (nb, cout, To, Ho,
    Wo) with dead windows as an INPUT.  value = P(conv(a, V) + conv(gbar, W)) * SELECT_SCALE + vb, 0 where dead, in fp64.
    Exact kind: integers and k/64 as in ``exact_case``; the sum bound doubles and is still asserted below 2^24 / 64."""
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = layer_dims(geom, li)
    exact = kind == "exact"
    gen = _gen(geom, li, nb, 11000 if exact else 13000)
    shape = (nb, cin, t, h, w)
    zeros = lambda: (torch.rand(shape, generator=gen) >= 1.0 / 3.0)          # noqa: E731
    if exact:
        a = torch.randint(-3, 4, shape, generator=gen).float() if li == 0 else torch.randint(0, 4, shape, generator=gen).float() * zeros()
        g = torch.randint(-3, 4, shape, generator=gen).float() if li > 0 else None
        V = (torch.randint(-4, 5, (cout, cin, 3, 7, 7), generator=gen).float() / 64.0).contiguous()
        W = (torch.randint(-4, 5, (cout, cin, 3, 7, 7), generator=gen).float() / 64.0).contiguous() if li > 0 else None
        vb = (torch.randint(-64, 65, (cout,), generator=gen).float() / 64.0).contiguous()
        bound = float(conv64(a.abs(), V.abs()).max()) + (float(conv64(g.abs(), W.abs()).max()) if li > 0 else 0.0) + 1.0
        assert bound * 64.0 < 2.0 ** 24, bound
    else:
        a = torch.randn(shape, generator=gen) if li == 0 else torch.randn(shape, generator=gen).abs() * zeros()
        g = torch.randn(shape, generator=gen) if li > 0 else None
        V = R.init_params(21)[2 * li].contiguous()
        W = R.init_params(22)[2 * li].contiguous() if li > 0 else None
        vb = None
    z = conv64(a, V) + (conv64(g, W) if li > 0 else 0.0)
    if vb is None:          # (a bias of the selected values' own magnitude: a larger one would hide their error in every norm)
        vb = (torch.randn(cout, generator=gen) * (float(z.pow(2).mean().sqrt()) * SELECT_SCALE)).contiguous()
    if exact:
        assert bool((z * 64.0 == (z * 64.0).round()).all())
    am = AO.argmax_bytes(300 + li + nb + sum(geom), (nb, cout, To, Ho, Wo), pt)
    dead = (am & 0x80) != 0
    assert bool(dead.any()) and bool((~dead).any())
    sel = windows(z, pt).gather(-1, (am & 7).long().unsqueeze(-1)).squeeze(-1)
    value = torch.where(dead, torch.zeros_like(sel), sel * SELECT_SCALE + vb.double().view(1, -1, 1, 1, 1))
    return SimpleNamespace(a=a, g=g, V=V, W=W, vb=vb, am=am, value=value, kind=kind, geom=geom, li=li, nb=nb)


def select_buffers(dims, li, nb, mode):
    """Sentinel-filled output of a select program with a guard clip: mode "f32" (select = 2: fp32 in the slot order, NaN), "planes"
    (select = 1: hi and lo, 0x7FFF) or "feat" (the last level: fp32 features, NaN)."""
    n = dims[1] * dims[8] * dims[9] * dims[10]
    if mode == "planes":
        return torch.full((2, (nb + 1) * (n // 8), 8), SENT16, dtype=torch.int16)
    return torch.full(((nb + 1) * n,), float("nan"), dtype=torch.float32)


def perfect_select(case, fmt, mode):
    dims = layer_dims(case.geom, case.li)
    buf = select_buffers(dims, case.li, case.nb, mode)
    v32 = case.value.float()
    if mode == "planes":
        s = to_slots(v32, fmt, 2)
        buf[:, :s.shape[1]] = s
    elif mode == "f32":
        nb, C, t, h, w = v32.shape
        buf[:v32.numel()] = v32.reshape(nb, C // 8, 8, t, h, w).permute(0, 1, 3, 4, 5, 2).reshape(-1)
    else:
        buf[:v32.numel()] = v32.reshape(-1)
    return buf


def check_select(buf, case, fmt, mode, bound=None, label="", record=None):
    """Guard and sentinels, then: exact kind -- the fp32 output is the fp32 cast of the fp64 value, the 16-bit planes are split16 of
    it, bit for bit (sign of a zero apart); random kind -- per clip rel-L2 whole / border shell below ``bound``, max-abs ratio below
    4 x ``bound``.  A dead window is exactly zero in both."""
    dims = layer_dims(case.geom, case.li)
    cout, To, Ho, Wo = dims[1], dims[8], dims[9], dims[10]
    nb, n = case.nb, cout * To * Ho * Wo
    v32 = case.value.float()
    if mode == "planes":
        assert bool((buf[:, nb * (n // 8):] == SENT16).all()), "the select program wrote behind its last clip"
        assert not bool((buf[:, :nb * (n // 8)] == SENT16).any()), "the select program left 16-bit elements unwritten"
        bits = from_slots(buf, nb, cout, To, Ho, Wo)
        got = decode(bits, fmt)
    else:
        assert bool(torch.isnan(buf[nb * n:]).all()), "the select program wrote behind its last clip"
        assert not bool(torch.isnan(buf[:nb * n]).any()), "the select program left elements unwritten (or wrote NaN)"
        got32 = from_feat(buf, nb, cout, To, Ho, Wo) if mode == "feat" else from_slots(buf, nb, cout, To, Ho, Wo)
        got = got32.double()
    dead = (case.am & 0x80) != 0
    assert bool((got[dead] == 0).all()), "a dead window is not zero"
    if case.kind == "exact":
        if mode == "planes":
            want = torch.stack(AO.split16(v32, PREC[fmt]))
            for k in range(2):
                diff = no_negative_zero(bits[k]) != no_negative_zero(want[k])
                assert not bool(diff.any()), "%s plane: %d of %d elements differ from split16 of the fp64 value" % (("hi", "lo")[k], int(diff.sum()), diff.numel())
        else:
            assert torch.equal(got32, v32), "%d of %d fp32 outputs differ from the fp64 value" % (int((got32 != v32).sum()), v32.numel())
        return got
    worst, where = value_errors(got, case.value)
    if record is not None:
        for k in range(3):
            record[k] = max(record[k], worst[k])
    print("select %s level %d %s: rel-L2 %.2e (clip %s), border shell %.2e (clip %s), max-abs ratio %.2e (clip %s) | so far %s" % (
        fmt, case.li, label, worst[0], where[0], worst[1], where[1], worst[2], where[2], ["%.2e" % v for v in record] if record is not None else "-"))
    assert worst[0] < bound and worst[1] < bound and worst[2] < 4 * bound, (worst, where)
    return got


def select_floor(case, fmt, mode):
    """What the operand format alone costs a select level (fp64 arithmetic on the operands as held, fp32 or hi + lo output)."""
    z = conv64(rounded(case.a, fmt), rounded(case.V, fmt, WSHIFT.get(fmt, 1.0)))
    if case.li > 0:
        z = z + conv64(rounded(case.g, fmt), rounded(case.W, fmt, WSHIFT.get(fmt, 1.0)))
    dead = (case.am & 0x80) != 0
    sel = windows(z, layer_dims(case.geom, case.li)[11]).gather(-1, (case.am & 7).long().unsqueeze(-1)).squeeze(-1)
    v32 = torch.where(dead, torch.zeros_like(sel), sel * SELECT_SCALE + case.vb.double().view(1, -1, 1, 1, 1)).float()
    got = decode(torch.stack(AO.split16(v32, PREC[fmt])), fmt) if mode == "planes" else v32.double()
    return value_errors(got, case.value)[0]
