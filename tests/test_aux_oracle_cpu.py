"""Checks the checker: every fp64 oracle of tests/aux_oracle.py agrees with an independent torch formulation to 1e-12, the bit-level
oracles with hand-computed patterns, and the seeded input generators deliver what the GPU tests rely on (no arg-max decided by
a tie, no label out of range except the planted one).  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import aux_oracle as O

TOL = 1e-12


def close(a, b, tol=TOL):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert a.shape == b.shape and err <= tol * scale, (err, scale)


def r64(*shape, seed=0):
    return torch.randn(*shape, generator=O.gen(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ reductions
def test_dm_loss_oracle_is_the_reference_class_term():
    fr, fs = r64(3, 7, 33, seed=1), r64(3, 2, 33, seed=2)
    got = O.dm_loss(fr, fs)
    close(got, torch.stack([R.dm_class_term(fr[c], fs[c]) for c in range(3)]))
    fs2 = fs.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(O.dm_loss(fr, fs2).sum(), fs2)
    close(g, (-2.0 / 2) * (fr.mean(1) - fs.mean(1))[:, None, :].expand(3, 2, 33))


def test_group_sum_and_replica_sum_and_bias_oracles():
    x = r64(6 * 5, 17, seed=3)
    want = torch.stack([sum(x[g * 5 + b] for b in range(5)) for g in range(6)]) * 0.125
    close(O.group_sum(x, 6, 5, 0.125), want)
    rep = r64(4, 5, 3, seed=4)
    want = torch.zeros(3, 5, dtype=torch.float64)
    for r in range(4):
        for i in range(5):
            for j in range(3):
                want[j, i] += rep[r, i, j]
    close(O.replica_sum(rep), want)
    # pooled bias gradient, both layouts, against a loop
    nclips, C, npos = 2, 16, 5
    g0 = r64(nclips, C, npos, seed=5)
    am0 = O.argmax_bytes(6, (nclips, C, npos), 2, 0.4)
    want = torch.zeros(C, dtype=torch.float64)
    for b in range(nclips):
        for n in range(C):
            for p in range(npos):
                if int(am0[b, n, p]) < 128:
                    want[n] += g0[b, n, p]
    close(O.bias_grad_pooled(g0, am0, nclips, C, npos, 0), want)
    g1 = g0.permute(0, 2, 1).contiguous()
    am1 = am0.reshape(nclips, C // 8, 8, npos).permute(0, 1, 3, 2).contiguous()
    close(O.bias_grad_pooled(g1, am1, nclips, C, npos, 1), want)
    assert 0 < int((am0 >= 128).sum()) < am0.numel()
    # dense bias gradient: decode + sum
    v = torch.randn(2, nclips, C // 8, npos, 8, generator=O.gen(7))
    for prec in (O.PREC_BF16, O.PREC_F16):
        bits = v.to(O.dtype16(prec)).view(torch.int16)
        want = v.to(O.dtype16(prec)).double().permute(2, 4, 0, 1, 3).reshape(C, -1).sum(1) * 0.25
        close(O.bias_grad_dense(bits, prec, C, 0.25), want)


@pytest.mark.parametrize("wd", [None, 5e-4])
def test_sgd_oracle_is_torch_optim_sgd(wd):
    x0, g = r64(50, seed=8), [r64(50, seed=9 + i) for i in range(3)]
    p = x0.clone().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=0.0 if wd is None else wd)
    x, buf = x0.clone(), None
    for i in range(3):
        p.grad = g[i].clone()
        opt.step()
        x, buf = O.sgd_step(x, buf, g[i], 0.1, 0.9, wd, i == 0)
        close(x, p.detach())
        close(buf, opt.state[p]["momentum_buffer"])
    # and the reference's own restatement (no weight decay)
    if wd is None:
        xr, br = R.sgd_momentum_step(x0, g[0], None, 0.1, 0.9)
        close(O.sgd_step(x0, None, g[0], 0.1, 0.9, None, True)[0], xr)


def test_standardize_oracle_is_the_reference_expression():
    x = r64(4097, seed=10) * 3 + 1.5
    close(O.standardize(x), R.standardise_batch(x))
    for mean, std in O.STANDARDIZE_ROWS:
        x32 = O.standardize_input(11, 4097, mean, std)
        ref = O.standardize(x32.double())
        bound, yard = O.standardize_bound(x32, ref)
        assert bound >= 2e-6 and bound >= 4 * yard and yard < 1e-3
        assert abs(float(x32.double().mean()) - mean) < 0.2 * std and abs(float(x32.double().std()) / std - 1) < 0.1


# ------------------------------------------------------------------------------------------------ head, loss
@pytest.mark.parametrize("C,K,To,Ho,kt,with_mask", [(8, 3, 2, 1, 1, False), (16, 5, 6, 2, 2, True), (24, 65, 3, 3, 2, True)])
def test_head_oracle_is_avgpool_conv_max(C, K, To, Ho, kt, with_mask):
    feats, w, b, mask = [None if t is None else t.double() for t in O.head_inputs(20, 3, C, To, Ho, Ho, kt, K, with_mask)]
    logits, dropped, amax, z = O.head_forward(feats, w, b, kt, Ho, Ho, mask)
    pooled = torch.nn.AvgPool3d((kt, Ho, Ho), stride=1)(feats)
    if mask is not None:
        pooled = pooled * mask[:, :, :, None, None]
    conv = torch.nn.Conv3d(C, K, 1).double()
    with torch.no_grad():
        conv.weight.copy_(w.reshape(K, C, 1, 1, 1))
        conv.bias.copy_(b)
        out = conv(pooled).squeeze(3).squeeze(3)
    close(logits, out.max(dim=2).values)
    assert torch.equal(amax, out.argmax(dim=2))
    close(dropped, pooled.squeeze(3).squeeze(3).permute(0, 2, 1))
    close(z, out)


def test_head_oracle_is_the_reference_head():
    """R.convnet3d_logits after its feature layers: (2,1,1) average pooling, mask, 1x1x1 conv, max over frames."""
    feats, w, b, mask = [t.double() for t in O.head_inputs(21, 2, 128, 4, 1, 1, 2, 7, True)]
    pooled = F.avg_pool3d(feats, kernel_size=(2, 1, 1), stride=1) * mask[:, :, :, None, None]
    want = F.conv3d(pooled, w.reshape(7, 128, 1, 1, 1), b).squeeze(3).squeeze(3).max(dim=2).values
    close(O.head_forward(feats, w, b, 2, 1, 1, mask)[0], want)


@pytest.mark.parametrize("B,K", [(1, 1), (9, 2), (9, 65), (4, 300)])
def test_ce_oracle_is_cross_entropy(B, K):
    logits, labels = O.ce_inputs(30, B, K)
    assert int(labels.min()) >= 0 and int(labels.max()) < K
    assert float(logits.max() - logits.min()) > (40 if K * B >= 18 else -1)
    close(O.ce_per_clip(logits.double(), labels), F.cross_entropy(logits.double(), labels, reduction="none"))
    close(O.ce_per_clip(logits.double(), labels).mean(), F.cross_entropy(logits.double(), labels))


def test_ce_inputs_plant_exactly_one_bad_label():
    for bad in (-1, 65):
        _, labels = O.ce_inputs(31, 9, 65, bad_label=(4, bad))
        out = (labels < 0) | (labels >= 65)
        assert out.nonzero().flatten().tolist() == [4]


def test_head_inputs_have_no_near_ties():
    """An arg-max may not hinge on rounding: the gap between the two best frames exceeds twice the fp32 forward bound."""
    for (B, C, To, Ho, kt, K, m) in ((5, 136, 6, 2, 2, 300, True), (1, 8, 2, 1, 1, 1, False), (5, 128, 5, 3, 1, 65, True)):
        feats, w, b, mask = O.head_inputs(40, B, C, To, Ho, Ho, kt, K, m)
        z = O.head_forward(feats.double(), w.double(), b.double(), kt, Ho, Ho, None if mask is None else mask.double())[3]
        zabs = O.head_forward(feats.double().abs(), w.double().abs(), b.double().abs(), kt, Ho, Ho,
                              None if mask is None else mask.double().abs())[3]
        bound = O.gamma(C + kt * Ho * Ho + 5) * float(zabs.max())
        top = z.topk(2, dim=2).values
        assert float((top[..., 0] - top[..., 1]).min()) > 2 * bound
        if mask is not None:
            assert set(mask.unique().tolist()) == {0.0, 2.0}
    assert O.head_tie_gap(*O.head_inputs(41, 2, 8, 1, 1, 1, 1, 3, False)[:3], 1, 1, 1, None) == math.inf


# ------------------------------------------------------------------------------------------------ match rows
def test_match_oracle_is_the_reference_match_loss():
    gr, gs = r64(6, 4, 3, 7, 7, seed=50), r64(6, 4, 3, 7, 7, seed=51)
    rows_r, rows_s = gr.reshape(-1, 7), gs.reshape(-1, 7)          # 5-D tensors: cosine over the LAST axis
    close(O.match_metric(rows_r, rows_s, 0), R.distance_wb(gr, gs))
    close(O.match_sums(rows_r, rows_s)[0], R.match_loss([gs], [gr], "ours"))
    close(O.match_metric(rows_r, rows_s, 1), R.match_loss([gs], [gr], "mse"))
    close(O.match_metric(rows_r, rows_s, 2), R.match_loss([gs], [gr], "cos"))
    s = O.match_sums(rows_r, rows_s)
    close(s[1], R.match_loss([gs], [gr], "mse"))
    close(1 - s[2] / (s[3].sqrt() * s[4].sqrt() + 1e-6), R.match_loss([gs], [gr], "cos"))
    # a trailing unit axis: every element its own row, cosine = sign agreement
    a, b = r64(9, 1, seed=52), r64(9, 1, seed=53)
    close(O.match_sums(a, b)[0], (1 - (a * b) / ((a * b).abs() + 1e-6)).sum())
    # an all-zero s row has gradient zero (the reference's norm backward), not NaN
    b0 = b.clone()
    b0[3] = 0
    b0.requires_grad_(True)
    (g,) = torch.autograd.grad(O.match_metric(a, b0, 0), b0)
    assert torch.isfinite(g).all() and float(g[3].abs()) == pytest.approx(float(a[3].abs() / 1e-6), rel=1e-9)


# ------------------------------------------------------------------------------------------------ scales
def test_absmax_exponent_puts_the_product_into_the_half_open_interval():
    f32 = lambda v: float(np.float32(v))
    below, above = f32(np.nextafter(np.float32(0.25), np.float32(0))), f32(np.nextafter(np.float32(0.25), np.float32(1)))
    for m in (1.0, 0.25, below, above, 3.0, 1e-3, f32(3e38), f32(1e-40), f32(2.0 ** -149), 1024.0, 1023.99994, 512.0):
        for target in (1024.0, 1.0, 100.0, f32(2.0 ** -100)):
            k = O.absmax_exponent(m, target)
            free = math.floor(math.log2(target / m)) if m > 1e-30 else None
            if -126 < k < 126:
                assert target / 2 <= m * 2.0 ** k < target, (m, target, k)
                assert free is None or k in (free, free - 1)
            else:
                assert (m * 2.0 ** k < target / 2) if k == 126 else (m * 2.0 ** k >= target)
    assert O.absmax_exponent(1.0, 1024.0) == 9 and O.absmax_exponent(0.5, 1024.0) == 10 and O.absmax_exponent(below * 4, 1024.0) == 10
    assert O.absmax_exponent(0.0, 1024.0) is None and O.absmax_exponent(math.inf, 1024.0) is None
    assert O.scale_combine((4.0, 0.25, 1), (8.0, 0.125, 1), 0) == 32.0 and O.scale_combine((4.0, 0.25, 1), None, 0) == 4.0
    assert O.scale_combine((4.0, 0.25, 1), (8.0, 0.125, 1), 1) == 4.0 and O.scale_combine((4.0, 0.25, 0), (8.0, 0.125, 1), 1) == 8.0
    assert O.scale_combine((4.0, 0.25, 1), (8.0, 0.125, 0), 1) == 4.0 and O.scale_combine((4.0, 0.25, 0), (8.0, 0.125, 0), 1) == 1.0
    assert O.scale_combine((4.0, 0.25, 0), None, 1) == 1.0 and O.scale_combine((4.0, 0.25, 1), None, 1) == 4.0


# ------------------------------------------------------------------------------------------------ bit-level
def test_split16_bit_patterns():
    v = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 65504.0, 1.0 + 2.0 ** -8,
                      1.0 + 3 * 2.0 ** -8], dtype=torch.float32)
    hi, lo = O.split16(v, O.PREC_F16X3)
    h = lambda t: [x & 0xffff for x in t.tolist()]
    # fp16: ties to even (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9), smallest subnormal 2^-24 = 0x0001, 2^-25 ties to 0
    assert h(hi)[:8] == [0x0000, 0x8000, 0x3c00, 0x3c00, 0x3c02, 0x0001, 0x0000, 0x7bff]
    assert h(lo)[:8] == [0x0000, 0x0000, 0x0000, 0x1000, 0x9000, 0x0000, 0x0000, 0x0000]      # 2^-11 = 0x1000; -2^-11; 2^-25 lost
    hi, lo = O.split16(v, O.PREC_BF16X3)
    assert h(hi)[8:] == [0x3f80, 0x3f82] and h(lo)[8:] == [0x3b80, 0xbb80]                    # bf16 ties at 2^-8: +-2^-8 = 0x3b80
    # hi + lo reproduces a normal-range input to the pair precision 2^-22 (fp16: while lo stays normal, |v| >= 2^-2; bf16: 2^-16)
    x = O.edge_values16(60, 4096)
    big = x.abs() >= 0.25
    for prec, rel in ((O.PREC_F16X3, 2.0 ** -22), (O.PREC_BF16X3, 2.0 ** -16)):
        hi, lo = O.split16(x, prec)
        back = O.decode16(hi, prec) + O.decode16(lo, prec)
        assert float(((back - x.double()).abs() / x.double().abs())[big].max()) <= rel
        assert torch.equal(O.round_operand(x, prec).double(), O.decode16(hi, prec))
    # the generator covers what it promises
    assert (x == 0).sum() >= 2 and ((x.abs() > 0) & (x.abs() < 6.1e-5)).any() and (x.abs() > 5.9e4).any() and torch.isfinite(x).all()
    assert torch.isfinite(x.to(torch.float16).float()).all()
    assert (torch.signbit(x) & (x == 0)).any()


def test_resplit_split_scaled_pix2rows_oracles():
    x = O.edge_values16(61, 512)
    hi, lo = O.split16(x, O.PREC_F16X3)
    dhi, dlo = O.resplit(hi, lo, O.PREC_F16X3, O.PREC_BF16X3)
    want = (hi.view(torch.float16).float() + lo.view(torch.float16).float())
    assert torch.equal(dhi, want.to(torch.bfloat16).view(torch.int16))
    shi, _ = O.split_scaled(x, 0.5, O.PREC_F16)
    assert torch.equal(shi, (x * 0.5).to(torch.float16).view(torch.int16))
    clips = torch.randn(3, 2, 3, 4, 13, generator=O.gen(62))
    idx = torch.tensor([2, 0, 2, 1])
    hi, lo = O.pix2rows(clips, idx, O.PREC_BF16X3)
    assert hi.shape == (4, 6, 4, 24)
    for b in range(4):
        for p in range(6):
            for r in range(4):
                row = torch.zeros(24)
                row[3:16] = clips[idx[b], p // 3, p % 3, r]
                assert torch.equal(hi[b, p, r], row.to(torch.bfloat16).view(torch.int16))
    assert int(hi[..., :3].abs().max()) == 0 and int(hi[..., 16:].abs().max()) == 0 and int(lo[..., 16:].abs().max()) == 0


@pytest.mark.parametrize("g_layout,pool_t,T,OH,OW", [(0, 2, 5, 4, 6), (1, 2, 4, 5, 3), (1, 1, 3, 4, 4), (0, 1, 2, 3, 5)])
def test_unpool_oracle_against_a_loop(g_layout, pool_t, T, OH, OW):
    nclips, C = 2, 16
    To, Ho, Wo = T // pool_t, OH // 2, OW // 2
    npos = To * Ho * Wo
    g = torch.randn(nclips * C * npos, generator=O.gen(70))
    am = O.argmax_bytes(71, (nclips * C * npos,), pool_t)
    hi, _ = O.unpool_relu_bwd(g, am, nclips, C, To, Ho, Wo, pool_t, T, OH, OW, g_layout, O.PREC_F16X3, 0.5)
    dense = torch.zeros(nclips, C // 8, T, OH, OW, 8)
    for b in range(nclips):
        for n in range(C):
            for p in range(npos):
                i = (b * C + n) * npos + p if g_layout == 0 else (b * npos + p) * C + n
                ai = i if g_layout == 0 else ((b * (C // 8) + n // 8) * npos + p) * 8 + n % 8
                a = int(am[ai])
                if a >= 128:
                    continue
                pt, pr, pc = p // (Ho * Wo), (p // Wo) % Ho, p % Wo
                dense[b, n // 8, pt * pool_t + (a >> 2), 2 * pr + ((a >> 1) & 1), 2 * pc + (a & 1), n % 8] = g[i] * 0.5
    assert torch.equal(hi, dense.to(torch.float16).view(torch.int16))
    assert int((am >= 128).sum()) > 0
