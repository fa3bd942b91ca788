"""Seeded inputs, fp64 references and slice metrics of one level's PARAMETER gradients (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_gpu_param_gradient.py (the device against fp64) and tests/test_wgrad_emulation_cpu.py (what the operand formats
alone cost, on the CPU), so that both speak about the same inputs.  torch on the CPU only.
"""
import functools

import torch
import torch.nn.functional as F

from tests import aux_oracle as AO
from tests.test_gpu_input_gradient import _dense_gradient

G_A, G_B, G_C = (4, 64, 66), (4, 65, 63), (4, 70, 58)
SMALL, ODD, FULL = (8, 64, 64), (12, 96, 80), (16, 112, 112)

# what tests/test_gpu_wgrad.py holds a single linear conv program to (rel-L2 against fp64), applied to every slice family
BAR = {"f16x3": 2e-5, "bf16x3": 1e-4, "f16": 2e-3}
PREC = {"f16x3": AO.PREC_F16X3, "bf16x3": AO.PREC_BF16X3, "f16": AO.PREC_F16}
FAMILIES = ("whole", "tap", "cout", "cin")
PATTERNS = ("full", "shell", "last")


def level_cases():
    """(clip size, format, level, clips) of the per-level test: the smallest shapes that reach each program family."""
    out = []
    for geom, fmts in ((G_A, ("f16x3", "f16")), (G_B, ("f16x3", "f16")), (G_C, ("f16x3", "f16")), (SMALL, ("f16x3", "f16", "bf16x3"))):
        for fmt in fmts:
            out += [(geom, fmt, 0, 1), (geom, fmt, 0, 3), (geom, fmt, 1, 9), (geom, fmt, 2, 9), (geom, fmt, 2, 1)]
            if geom == SMALL:
                out += [(geom, fmt, 1, 8), (geom, fmt, 1, 17)]
    for geom in (ODD, FULL):
        out += [(geom, "f16x3", li, 2) for li in range(3)]
    return out


def layer_dims(geom, li):
    from video_distillation_amd import plan
    return plan.NetGeometry(*geom).layer_dims()[li]


@functools.lru_cache(maxsize=None)
def inputs(geom, li, nb, mag=1.0):
    """The level's random inputs: pooled gradient g (fp32, layout 0 at level 2, channels-last below), arg-max bytes with dead
    windows, source x (nb, cin, t, h, w) fp32, and the seeded start values of the accumulated g_w / g_b."""
    cin, cout, t, h, w, T, OH, OW, To, Ho, Wo, pt = layer_dims(geom, li)
    layout = 0 if li == 2 else 1
    gen = torch.Generator().manual_seed(5000 + 1000 * li + nb + sum(geom))
    shape = (nb, cout, To, Ho, Wo) if layout == 0 else (nb, To, Ho, Wo, cout)
    g = (torch.randn(shape, generator=gen) * mag).contiguous()
    am = AO.argmax_bytes(177 + li + nb, (nb, cout, To, Ho, Wo) if layout == 0 else (nb, cout // 8, To, Ho, Wo, 8), pt)
    assert bool((am & 0x80 != 0).any()) and bool((am & 0x80 == 0).any())
    x = torch.randn(nb, cin, t, h, w, generator=gen)
    w0 = torch.randn(cout, cin, 3, 7, 7, generator=gen) * mag          # (at the gradient's magnitude: an fp32 sum keeps 2^-24 of its LARGER term)
    b0 = torch.randn(cout, generator=gen) * mag
    return g, am, layout, x, w0, b0


def shell_mask(t, h, w):
    """First and last frame, and within 3 of a spatial edge."""
    tt, hh, ww = torch.arange(t), torch.arange(h), torch.arange(w)
    return (((tt == 0) | (tt == t - 1))[:, None, None] | ((hh < 3) | (hh >= h - 3))[None, :, None] | ((ww < 3) | (ww >= w - 3))[None, None, :])


def pattern(geom, li, nb, name, mag=1.0):
    """Inputs of one pattern: 'full'; 'shell' (source non-zero only on its border shell: dW depends on the padding taps and box
    edges alone); 'last' (pooled gradient non-zero only in the last pooled row and column: the ragged boxes)."""
    g, am, layout, x, w0, b0 = inputs(geom, li, nb, mag)
    _, _, t, h, w, _, _, _, To, Ho, Wo, _ = layer_dims(geom, li)
    if name == "shell":
        x = x * shell_mask(t, h, w).to(x.dtype)
    elif name == "last":
        keep = torch.zeros(Ho, Wo)
        keep[Ho - 1, :] = 1
        keep[:, Wo - 1] = 1
        g = (g * (keep[None, None, None] if layout == 0 else keep[None, None, :, :, None])).contiguous()
    else:
        assert name == "full"
    return g, am, layout, x, w0, b0


def padding_only_taps(geom, li):
    """How many of the 147 taps multiply nothing but padding at this level: tap k of an axis is live if some conv position o of the
    POOLED part of the grid (only there dy can be non-zero) has stride * o + k - pad inside the source."""
    _, _, t, h, w, _, _, _, To, Ho, Wo, pt = layer_dims(geom, li)
    live = lambda n_in, n_out, k, s, p: sum(any(0 <= s * o + kk - p < n_in for o in range(n_out)) for kk in range(k))          # noqa: E731
    return 147 - live(t, To * pt, 3, 1, 1) * live(h, 2 * Ho, 7, 2, 3) * live(w, 2 * Wo, 7, 2, 3)


def weight_gradient(x, dy):
    """fp64 autograd of F.conv3d with respect to the weight."""
    cout, cin = dy.shape[1], x.shape[1]
    wt = torch.zeros(cout, cin, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), wt, None, stride=(1, 2, 2), padding=(1, 3, 3))
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (dw,) = torch.autograd.grad(y, wt, dy.double())
    return dw


@functools.lru_cache(maxsize=None)
def reference(geom, li, nb, name, mag=1.0):
    """fp64 on the host: dense dy by index arithmetic, dW by autograd, db = dy summed over clips and positions, and the sum of the
    absolute terms of db.  -> (dW, db, |db| terms)"""
    g, am, layout, x, _, _ = pattern(geom, li, nb, name, mag)
    dy = _dense_gradient(g, am, layer_dims(geom, li), layout)
    return weight_gradient(x, dy), dy.sum(dim=(0, 2, 3, 4)), dy.abs().sum(dim=(0, 2, 3, 4))


def rounded(v, fmt, scale=1.0):
    """fp32 values as the operand format holds them (hi, or hi + lo), in fp64; ``scale``: the power of two applied before rounding."""
    hi, lo = AO.split16((v * scale).contiguous(), PREC[fmt])
    out = AO.decode16(hi, PREC[fmt])
    if AO.has_lo(PREC[fmt]):
        out = out + AO.decode16(lo, PREC[fmt])
    return out / scale


def slice_errors(got, want):
    """Rel-L2 of the whole tensor and the worst rel-L2 over the slices of three families -- per tap (147 slices over (cout, cin)), per
    output channel, per input channel -- with where the worst is.  A slice whose reference is identically zero must be exactly
    zero in the result (its count is returned): -> ({family: (worst, index)}, {family: zero slices})"""
    d = got.double() - want
    cout, cin = want.shape[:2]
    fam = {"whole": (d.reshape(1, -1), want.reshape(1, -1)),
           "tap": (d.reshape(cout * cin, 147).t(), want.reshape(cout * cin, 147).t()),
           "cout": (d.reshape(cout, -1), want.reshape(cout, -1)),
           "cin": (d.permute(1, 0, 2, 3, 4).reshape(cin, -1), want.permute(1, 0, 2, 3, 4).reshape(cin, -1))}
    worst, zeros = {}, {}
    for k, (dd, ww) in fam.items():
        en, wn = dd.norm(dim=1), ww.norm(dim=1)
        dead = wn == 0
        assert bool((en[dead] == 0).all()), "%s slices %s have a zero reference and a non-zero result" % (k, torch.nonzero(dead & (en != 0)).flatten().tolist())
        rel = torch.where(dead, torch.zeros_like(en), en / torch.where(dead, torch.ones_like(wn), wn))
        assert bool(torch.isfinite(rel).all()), k
        i = int(rel.argmax())
        worst[k], zeros[k] = (float(rel[i]), i), int(dead.sum())
    return worst, zeros
