"""fp64 restatements of the helper entry points of include/vd_hip.h (TEST INFRASTRUCTURE ONLY).

One plain function per operation, written from the header's contract and the reference lines it cites -- not from the HIP
source.  torch on the CPU only, nothing from the product package.  Differentiable operations are stated as their FORWARD;
tests/test_gpu_aux_kernels.py obtains gradients and double-backward from fp64 autograd.  The bit-level operations are built from
torch's float16 / bfloat16 casts (round to nearest even, like the hardware conversion) and compared as integer bit patterns.
The seeded input generators of the GPU tests live here too, so that tests/test_aux_oracle_cpu.py can check them without a GPU.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

PREC_BF16, PREC_F16, PREC_BF16X3, PREC_F16X3 = 0, 1, 2, 3          # VD_PREC_* of vd_hip.h
U32 = 2.0 ** -24                                                     # unit roundoff of fp32


def gamma(k: float) -> float:
    """k roundings of relative size 2^-24 each compound to at most k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1)."""
    return k * U32 / (1.0 - k * U32)


def dtype16(prec: int) -> torch.dtype:
    return torch.bfloat16 if prec in (PREC_BF16, PREC_BF16X3) else torch.float16


def has_lo(prec: int) -> bool:
    return prec >= 2


# ---------------------------------------------------------------------------------------------- bit-level operations
def split16(v: torch.Tensor, prec: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """hi = rn16(v), lo = rn16(v - hi) (the subtraction in fp32, where it is exact) as int16 bit patterns."""
    assert v.dtype == torch.float32
    dt = dtype16(prec)
    hi = v.to(dt)
    lo = (v - hi.float()).to(dt)
    return hi.view(torch.int16), lo.view(torch.int16)


def decode16(bits: torch.Tensor, prec: int) -> torch.Tensor:
    return bits.view(dtype16(prec)).double()


def round_operand(w: torch.Tensor, prec: int) -> torch.Tensor:
    """(float) rn16(w)"""
    return w.to(dtype16(prec)).float()


def split_scaled(src: torch.Tensor, scale: Optional[float], prec: int):
    v = src if scale is None else src * torch.tensor(scale, dtype=torch.float32)
    return split16(v, prec)


def resplit(src_hi: torch.Tensor, src_lo: Optional[torch.Tensor], src_prec: int, dst_prec: int):
    """16-bit elements of one format (hi, optionally + lo, summed in fp32) split again in another."""
    v = src_hi.view(dtype16(src_prec)).float()
    if src_lo is not None:
        v = v + src_lo.view(dtype16(src_prec)).float()
    return split16(v, dst_prec)


def pix2rows(x: torch.Tensor, clip_index: Optional[torch.Tensor], prec: int):
    """(B,T,3,H,W) fp32 -> [nclips][T*3][H][pitch] 16-bit rows, pitch = roundup8(W + 8), row = 3 zeros, the W pixels, zeros."""
    B, T, ch, H, W = x.shape
    assert ch == 3
    src = x if clip_index is None else x[clip_index]
    pitch = (W + 8 + 7) // 8 * 8
    rows = torch.zeros(src.shape[0], T * 3, H, pitch, dtype=torch.float32)
    rows[..., 3:3 + W] = src.reshape(src.shape[0], T * 3, H, W)
    return split16(rows, prec)


def unpool_relu_bwd(g: torch.Tensor, argmax: torch.Tensor, nclips: int, C: int, To: int, Ho: int, Wo: int, pool_t: int, T: int,
                    OH: int, OW: int, g_layout: int, prec: int, scale: Optional[float]):
    """Backward of ReLU + MaxPool3d((pool_t,2,2)) as a SCATTER by index arithmetic: pooled output (clip, n, pt, pr, pc) with arg-max
    byte a sends its gradient (x scale) to dense position (pt*pool_t + a.bit2, 2 pr + a.bit1, 2 pc + a.bit0); a byte with bit 7 set
    (ReLU-dead window) or naming a position outside the window / the grid sends nothing.  Result: channels-last slots
    [clip][C/8][T][OH][OW][8] as (hi, lo) bit patterns."""
    npos = To * Ho * Wo
    if g_layout == 0:
        gd = g.reshape(nclips, C, npos)
        am = argmax.reshape(nclips, C, npos)
    else:
        gd = g.reshape(nclips, npos, C).permute(0, 2, 1)
        am = argmax.reshape(nclips, C // 8, npos, 8).permute(0, 1, 3, 2).reshape(nclips, C, npos)
    gd = gd if scale is None else gd * torch.tensor(scale, dtype=torch.float32)
    am = am.to(torch.int64)
    clip, n, pos = torch.meshgrid(torch.arange(nclips), torch.arange(C), torch.arange(npos), indexing="ij")
    pt, pr, pc = pos // (Ho * Wo), (pos // Wo) % Ho, pos % Wo
    t = pt * pool_t + ((am >> 2) & 1)
    oh, ow = 2 * pr + ((am >> 1) & 1), 2 * pc + (am & 1)
    ok = (am < (8 if pool_t == 2 else 4)) & (t < T) & (oh < OH) & (ow < OW)
    dense = torch.zeros(nclips, C, T, OH, OW, dtype=torch.float32)
    dense[clip[ok], n[ok], t[ok], oh[ok], ow[ok]] = gd[ok]
    slots = dense.reshape(nclips, C // 8, 8, T, OH, OW).permute(0, 1, 3, 4, 5, 2).contiguous()
    return split16(slots, prec)


# ---------------------------------------------------------------------------------------------- reductions
def dm_loss(feat_real: torch.Tensor, feat_syn: torch.Tensor) -> torch.Tensor:
    """loss[c] = sum_d (mean_b real[c,b,d] - mean_b syn[c,b,d])^2 ; inputs [nclass][n][dim] fp64."""
    diff = feat_real.mean(dim=1) - feat_syn.mean(dim=1)
    return (diff * diff).sum(dim=1)


def group_sum(x: torch.Tensor, groups: int, per: int, scale: float) -> torch.Tensor:
    return x.reshape(groups, per, -1).sum(dim=1) * scale


def sgd_step(x, buf, g, lr, mu, wd, first):
    """torch.optim.SGD(momentum, dampening 0, weight_decay): g' = g + wd x; buf = first ? g' : mu buf + g'; x -= lr buf.
    Works in the dtype of its arguments, one operation at a time (fp64 oracle, or the fp32 formula bit for bit)."""
    gp = g if wd is None else g + wd * x
    nb = gp.clone() if first else buf * mu + gp
    return x - lr * nb, nb


def bias_grad_dense(dy_bits: torch.Tensor, prec: int, N: int, scale_inv: Optional[float]) -> torch.Tensor:
    """dy_bits [planes][clip][N/8][npos][8] int16 -> scale_inv * sum over planes, clips, positions, per channel."""
    v = decode16(dy_bits, prec).sum(dim=(0, 1, 3)).reshape(N)
    return v if scale_inv is None else v * scale_inv


def _pooled_cn(g, argmax, nclips, C, npos, g_layout):
    if g_layout == 0:
        return g.reshape(nclips, C, npos), argmax.reshape(nclips, C, npos)
    return (g.reshape(nclips, npos, C).permute(0, 2, 1),
            argmax.reshape(nclips, C // 8, npos, 8).permute(0, 1, 3, 2).reshape(nclips, C, npos))


def bias_grad_pooled(g: torch.Tensor, argmax: torch.Tensor, nclips: int, C: int, npos: int, g_layout: int) -> torch.Tensor:
    """sum of g over clips and pooled positions whose window was alive (bit 7 of the arg-max byte clear); g fp64."""
    gd, am = _pooled_cn(g, argmax, nclips, C, npos, g_layout)
    return (gd * ((am.to(torch.int64) & 0x80) == 0)).sum(dim=(0, 2))


def replica_sum(rep: torch.Tensor) -> torch.Tensor:
    """rep [replicas][rows][cols] -> [cols][rows]"""
    return rep.sum(dim=0).t()


def standardize(x: torch.Tensor) -> torch.Tensor:
    """(x - mean) / std, batch-global scalars, unbiased std; x fp64."""
    n = x.numel()
    mean = x.sum() / n
    var = ((x - mean) ** 2).sum() / (n - 1)
    return (x - mean) / var.sqrt()


# ---------------------------------------------------------------------------------------------- head, loss, match rows (forward only)
def head_forward(feats: torch.Tensor, w: torch.Tensor, b: torch.Tensor, kt: int, kh: int, kw: int,
                 mask: Optional[torch.Tensor] = None):
    """AvgPool3d((kt,kh,kw), stride 1) over (B,C,To,Ho,Wo) with Ho == kh, Wo == kw; dropout mask (B,C,Tp) of 0 or 1/(1-p);
    1x1x1 conv (w [K][C], b [K]); max over T.  Returns logits (B,K), dropped (B,Tp,C), arg-max frame (B,K), z (B,K,Tp)."""
    B, C, To, Ho, Wo = feats.shape
    assert Ho == kh and Wo == kw
    Tp = To - kt + 1
    pooled = torch.stack([feats[:, :, t:t + kt].sum(dim=(2, 3, 4)) for t in range(Tp)], dim=2) / (kt * kh * kw)
    if mask is not None:
        pooled = pooled * mask
    z = torch.einsum("bct,kc->bkt", pooled, w) + b[None, :, None]
    logits, amax = z.max(dim=2)
    return logits, pooled.permute(0, 2, 1), amax, z


def ce_per_clip(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss per clip: log sum_k exp(z_k) - z_y (the mean over clips is the loss)."""
    m = logits.max(dim=1, keepdim=True).values
    lse = m.squeeze(1) + (logits - m).exp().sum(dim=1).log()
    return lse - logits.gather(1, labels[:, None]).squeeze(1)


def match_sums(gr: torch.Tensor, gs: torch.Tensor) -> torch.Tensor:
    """The five sums of one gradient tensor viewed as [rows][len]."""
    d, a, b = (gr * gs).sum(-1), (gr * gr).sum(-1), (gs * gs).sum(-1)
    cos = (1 - d / (gr.norm(dim=-1) * gs.norm(dim=-1) + 0.000001)).sum()
    return torch.stack([cos, ((gs - gr) ** 2).sum(), d.sum(), a.sum(), b.sum()])


def match_metric(gr: torch.Tensor, gs: torch.Tensor, mode: int) -> torch.Tensor:
    """mode 0 'ours' (row cosine), 1 'mse', 2 'cos' (global) of utils.py:634-687."""
    if mode == 0:
        return (1 - (gr * gs).sum(-1) / (gr.norm(dim=-1) * gs.norm(dim=-1) + 0.000001)).sum()
    if mode == 1:
        return ((gs - gr) ** 2).sum()
    return 1 - (gr * gs).sum() / (gr.norm() * gs.norm() + 0.000001)


# ---------------------------------------------------------------------------------------------- scales
def absmax_exponent(m: float, target: float) -> Optional[int]:
    """The k of vd_absmax_scale: max|g| 2^k in [target/2, target), clamped to [-126, 126]; None = scale 1 (nothing to scale)."""
    if not (m > 0.0 and math.isfinite(m) and target > 0.0 and math.isfinite(target)):
        return None
    fm, em = math.frexp(m)          # exact: both are floats
    ft, et = math.frexp(target)
    k = et - em - (0 if ft > fm else 1)
    return max(-126, min(126, k))


def scale_combine(a, b, mode: int) -> float:
    """a, b: (scale, 1/scale, absmax word) triples or None (b)."""
    x, y = a[0], (1.0 if b is None else b[0])
    if mode == 0:
        return x * y
    a_empty, b_empty = a[2] == 0, (b is None or b[2] == 0)
    return (1.0 if b_empty else y) if a_empty else (x if b_empty else min(x, y))


# ---------------------------------------------------------------------------------------------- seeded inputs
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def head_inputs(seed: int, B: int, C: int, To: int, Ho: int, Wo: int, kt: int, K: int, with_mask: bool):
    """feats, w, b, mask (fp32).  The draw is repeated with the next seed until no two frames of a (clip, class) are closer than
    HEAD_TIE_MARGIN of the logit scale, so that fp32 rounding cannot decide an arg-max."""
    Tp = To - kt + 1
    for s in range(seed, seed + 64):
        g = gen(s)
        feats = torch.randn(B, C, To, Ho, Wo, generator=g)
        w = torch.randn(K, C, generator=g) / math.sqrt(C)
        b = torch.randn(K, generator=g) * 0.1
        mask = ((torch.rand(B, C, Tp, generator=g) < 0.5).float() * 2.0) if with_mask else None
        if head_tie_gap(feats, w, b, kt, Ho, Wo, mask) > HEAD_TIE_MARGIN:
            return feats, w, b, mask
    raise AssertionError("no tie-free draw")


HEAD_TIE_MARGIN = 1e-4          # >> gamma(C + 20) * sum|terms| ~ 1e-5 * O(1) of these inputs


def head_tie_gap(feats, w, b, kt, kh, kw, mask) -> float:
    """smallest distance between the best and the second-best frame of any (clip, class), relative to max |z| (inf for one frame)"""
    z = head_forward(feats.double(), w.double(), b.double(), kt, kh, kw, None if mask is None else mask.double())[3]
    if z.shape[2] < 2:
        return math.inf
    top = z.topk(2, dim=2).values
    return float((top[..., 0] - top[..., 1]).min() / z.abs().max())


def ce_inputs(seed: int, B: int, K: int, spread: float = 60.0, bad_label: Optional[Tuple[int, int]] = None):
    """logits with a range of about `spread` and labels in [0, K); bad_label = (clip, value) plants one out-of-range label."""
    g = gen(seed)
    logits = (torch.rand(B, K, generator=g) - 0.5) * spread
    labels = torch.randint(0, K, (B,), generator=g)
    if bad_label is not None:
        labels[bad_label[0]] = bad_label[1]
    return logits, labels


def argmax_bytes(seed: int, shape, pool_t: int, dead_fraction: float = 0.25) -> torch.Tensor:
    """arg-max bytes of a pooled level: window code 0..3 (pool_t 1) or 0..7 (pool_t 2), bit 7 set on dead windows (their low bits
    still hold a code: the dead bit alone must silence them)."""
    g = gen(seed)
    code = torch.randint(0, 8 if pool_t == 2 else 4, shape, generator=g)
    dead = torch.rand(shape, generator=g) < dead_fraction
    return (code | (dead.long() << 7)).to(torch.uint8)


def edge_values16(seed: int, n: int) -> torch.Tensor:
    """fp32 values that stress the 16-bit splits: +-0, the fp16 subnormal range (< 6.1e-5), exact rounding ties of both
    formats, values near 1 and near 6e4 (finite in fp16), and seeded noise over 20 binades; length n."""
    g = gen(seed)
    special = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 5e-6, -3e-5, 6.0e-5, 6.2e-5,
               1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -11), 1.0, -1.0,
               1.0 - 2.0 ** -12, 0.999, 1.001, 2048.0 + 1.0, 2048.0 + 3.0, 6.0e4, -6.0e4, 59999.5, 60001.7, 0.1, -0.3333333]
    noise = torch.randn(max(n - len(special), 0), generator=g) * torch.exp2(torch.randint(-16, 5, (max(n - len(special), 0),), generator=g).float())
    v = torch.cat([torch.tensor(special, dtype=torch.float32), noise])[:n]
    return v[torch.randperm(v.numel(), generator=g)].contiguous()


def standardize_input(seed: int, n: int, mean: float, std: float) -> torch.Tensor:
    return torch.randn(n, generator=gen(seed)) * std + mean


STANDARDIZE_ROWS = ((1.5, 3.0), (0.45, 0.25), (10.0, 0.1), (100.0, 1.0), (100.0, 0.1), (1000.0, 1.0))


def standardize_bound(x: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(bound, yardstick): 4 x the error of the reference's own fp32 expression on this input, or 2e-6, whichever is larger."""
    y32 = (x - x.mean()) / x.std()
    yard = float((y32.double() - ref).abs().max())
    return max(4.0 * yard, 2e-6), yard
