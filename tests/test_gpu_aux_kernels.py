"""Every helper entry point of csrc/aux_kernels.hip, called straight through the C ABI (ctypes on hip.lib(), no trainer, no
engine) and compared with the fp64 restatements of tests/aux_oracle.py at the shapes where kernels go wrong: unroll tails, grid
caps, one-element rows, block boundaries, odd grids.

Tolerances (none hand-tuned):
  * bit-level operations, integer outputs and "bitwise the same" claims are compared exactly;
  * fp32 reductions against fp64 use the forward bound |err| <= gamma(k) * sum|terms|, gamma(k) = k u / (1 - k u), u = 2^-24, the
    sum of absolute terms evaluated in fp64 and k = the fp32 roundings on the kernel's longest path, counted in a comment at
    each use (fused multiply-adds only lower the count);
  * where such a bound is not practical (second-order head pass, cosine rows) the yardstick is the error of the same expression
    evaluated by torch in fp32 on the CPU against the fp64 oracle: the kernel may be at most 4 x that + 4 ulp of the output's scale.
Every check prints its measured error beside its bound; with VD_AUX_PARITY_OUT=<path> the pairs are also written there as JSON,
stamped with hip.sources_hash() (the file meant for it is profiles/aux_kernels_parity.json).  Each launch runs once; all inputs are seeded and small."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import aux_oracle as O

pytestmark = pytest.mark.gpu

I64, F32, VP = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
ULP = 2.0 ** -23
RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    path = os.environ.get("VD_AUX_PARITY_OUT")
    if path and RECORDS:
        from video_distillation_amd import hip
        with open(path, "w") as f:
            json.dump({"sources_hash": hip.sources_hash(), "library_stamp": hip.loaded_stamp(),
                       "device": torch.cuda.get_device_name(0), "note": "max |error| beside its bound per check of "
                       "tests/test_gpu_aux_kernels.py (forward bound gamma(k) sum|terms|, or 4 x fp32-torch error + 4 ulp)",
                       "checks": RECORDS}, f, indent=1)


def call(name, *args):
    """One launch on the current stream, then wait; returns the entry point's code."""
    from video_distillation_amd import hip
    rc = getattr(hip.lib(), name)(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def ok(name, *args):
    assert call(name, *args) == 0, name


def P(t):
    return VP(0 if t is None else t.data_ptr())


KEEP = []


@pytest.fixture(autouse=True)
def _release_device_inputs():
    yield
    KEEP.clear()


def dev(t):
    """device copy of an input, kept alive until the test ends (a temporary would hand its memory to the next upload)"""
    if t is None:
        return None
    KEEP.append(t.contiguous().cuda())
    return KEEP[-1]


def d64(t):
    return None if t is None else t.double()


def report(label, got, ref, bound):
    """max |got - ref| against an elementwise (or scalar) bound; prints and records the worst pair."""
    got, ref = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).detach().cpu().reshape(-1)
    if bound.numel() == 1:
        bound = bound.expand_as(ref)
    assert got.shape == ref.shape == bound.shape, (label, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), label
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    i = int(ratio.argmax())
    print("%-58s err %.3e  bound %.3e  (max err %.3e)" % (label, float(err[i]), float(bound[i]), float(err.max())))
    RECORDS.append({"check": label, "error": float(err[i]), "bound": float(bound[i]), "max_error": float(err.max())})
    assert float(ratio[i]) <= 1.0, "%s: error %.3e exceeds bound %.3e" % (label, float(err[i]), float(bound[i]))


def report_yard(label, got, ref, ref32):
    """the yardstick rule: max error <= 4 x (max error of the fp32 torch evaluation) + 4 ulp of the output's scale"""
    got, ref, ref32 = [torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, ref, ref32)]
    assert torch.isfinite(got).all(), label
    err, yard = float((got - ref).abs().max()), float((ref32 - ref).abs().max())
    bound = 4.0 * yard + 4.0 * ULP * float(ref.abs().max())
    print("%-58s err %.3e  bound %.3e  (fp32 torch %.3e)" % (label, err, bound, yard))
    RECORDS.append({"check": label, "error": err, "bound": bound, "fp32_torch_error": yard})
    assert err <= bound, "%s: error %.3e exceeds 4 x %.3e + 4 ulp = %.3e" % (label, err, yard, bound)


def bits_equal(label, got, want):
    got, want = got.cpu().reshape(-1), want.cpu().reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    bad = int((got != want).sum())
    print("%-58s %d of %d elements differ" % (label, bad, want.numel()))
    RECORDS.append({"check": label, "error": bad, "bound": 0})
    assert bad == 0, "%s: %d elements differ, first at %d" % (label, bad, int((got != want).nonzero()[0]))


# ================================================================================================ vd_dm_loss
@pytest.mark.parametrize("nclass,nreal,nsyn,dim,with_g", [(5, 64, 3, 2048, True), (1, 1, 1, 1, True), (5, 7, 1, 63, True),
                                                          (1, 8, 3, 1024, True), (5, 9, 3, 1025, True), (1, 64, 1, 2048, False)])
def test_dm_loss(nclass, nreal, nsyn, dim, with_g):
    g = O.gen(100 + dim + nreal)
    fr, fs = torch.randn(nclass, nreal, dim, generator=g) + 0.3, torch.randn(nclass, nsyn, dim, generator=g)
    loss = torch.full((nclass,), 7.0).cuda()
    gs = torch.full((nclass, nsyn, dim), 7.0).cuda() if with_g else None
    ok("vd_dm_loss", P(dev(fr)), P(dev(fs)), nclass, nreal, nsyn, dim, P(loss), P(gs))
    fs64 = fs.double().requires_grad_(True)
    ref = O.dm_loss(fr.double(), fs64)
    (gref,) = torch.autograd.grad(ref.sum(), fs64)
    # a column mean: at most n adds, the rounded 1/n and the multiplication by it (n + 2 roundings); the difference of the two
    # means one more: k = max(nreal, nsyn) + 3 on |mean| terms A + S.  loss = sum_d diff^2: the error e of diff enters as
    # 2 |diff| e + e^2; the square, <= ceil(dim / 1024) adds per thread, a 6-level wave tree and 16 adds over the waves: k2.
    e = O.gamma(max(nreal, nsyn) + 3) * (fr.double().abs().mean(1) + fs.double().abs().mean(1))
    diff = (fr.double().mean(1) - fs.double().mean(1)).abs()
    k2 = 1 + math.ceil(dim / 1024) + 6 + 16
    report("dm_loss loss %s" % ((nclass, nreal, nsyn, dim),), loss, ref.detach(),
           (2 * diff * e + e * e).sum(1) + O.gamma(k2) * ((diff + e) ** 2).sum(1))
    if with_g:      # g = -2 diff / nsyn: the rounded 1 / nsyn and one multiplication on top of diff's error
        report("dm_loss g_syn %s" % ((nclass, nreal, nsyn, dim),), gs, gref,
               ((2.0 / nsyn) * e + O.gamma(2) * 2.0 / nsyn * (diff + e))[:, None, :].expand(nclass, nsyn, dim))


# ================================================================================================ vd_group_sum
@pytest.mark.parametrize("groups,per,dim", [(6, 4, 256), (1, 1, 1), (6, 3, 255), (1, 5, 257), (6, 5, 1), (1, 4, 255), (6, 1, 257)])
def test_group_sum(groups, per, dim):
    x = torch.randn(groups * per, dim, generator=O.gen(200 + per + dim))
    out = torch.full((groups, dim), 7.0).cuda()
    scale = 0.375          # != 1, exact in fp32
    ok("vd_group_sum", P(dev(x)), groups, per, dim, F32(scale), P(out))
    # at most `per` adds and the multiplication by scale: k = per + 1
    report("group_sum %s" % ((groups, per, dim),), out, O.group_sum(x.double(), groups, per, scale),
           O.gamma(per + 1) * O.group_sum(x.double().abs(), groups, per, scale))


# ================================================================================================ vd_sgd_momentum(_wd)
@pytest.mark.parametrize("wd", [None, 5e-4])
@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 3])
def test_sgd_momentum(n, wd):
    g = O.gen(300 + (n % 1000))
    x0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    lr, mu = np.float32(0.1), np.float32(0.9)
    wd32 = None if wd is None else np.float32(wd)
    x, buf = x0.cuda(), torch.full((n,), 7.0).cuda()          # `first` must overwrite whatever the buffer holds
    x32, b32 = x0.clone(), None
    x64, b64, xa, ba = x0.double(), None, x0.double().abs(), None
    t32 = lambda v: torch.tensor(v, dtype=torch.float32)
    for step in range(3):
        first = 1 if step == 0 else 0
        gd = grads[step].cuda()
        if wd is None:
            ok("vd_sgd_momentum", P(x), P(buf), P(gd), I64(n), F32(lr), F32(mu), first)
        else:
            ok("vd_sgd_momentum_wd", P(x), P(buf), P(gd), I64(n), F32(lr), F32(mu), F32(wd32), first)
        # the header's formula in fp32, one rounded operation after the other (0-dim fp32 coefficients)
        x32, b32 = O.sgd_step(x32, b32, grads[step], t32(lr), t32(mu), None if wd is None else t32(wd32), bool(first))
        # fp64 with the same (fp32-representable) coefficients, and the same recursion over absolute values for the bound
        c = (float(lr), float(mu), None if wd is None else float(wd32))
        x64, b64 = O.sgd_step(x64, b64, grads[step].double(), *c, bool(first))
        xa, ba = O.sgd_step(xa, ba, grads[step].double().abs(), -c[0], c[1], c[2], bool(first))
    bits_equal("sgd%s n=%d x vs fp32 formula" % ("" if wd is None else "_wd", n), x.view(torch.int32), x32.view(torch.int32))
    bits_equal("sgd%s n=%d buf vs fp32 formula" % ("" if wd is None else "_wd", n), buf.view(torch.int32), b32.view(torch.int32))
    # six rounded operations per step (wd x, + g, mu buf, + g', lr buf, x -), three steps: k = 18 on the recursion's absolute terms
    report("sgd%s n=%d x vs fp64 SGD" % ("" if wd is None else "_wd", n), x, x64, O.gamma(18) * xa)
    report("sgd%s n=%d buf vs fp64 SGD" % ("" if wd is None else "_wd", n), buf, b64, O.gamma(18) * ba)


# ================================================================================================ classifier head
#              B   C    K   To Ho kt  mask      (Ho = Wo = kh = kw; Tp = To - kt + 1)
HEAD_CASES = [(5, 128, 64, 3, 1, 2, True),      # typical: Tp 2
              (1, 8, 1, 1, 1, 1, False),        # Tp 1, one class
              (5, 136, 300, 6, 2, 2, True),     # Tp 5, more than one class per thread, C not a multiple of 64
              (1, 128, 65, 5, 3, 1, False),     # Tp 5, kt 1, 3 x 3 window
              (5, 8, 3, 2, 2, 1, True),         # Tp 2
              (1, 136, 3, 2, 3, 2, True)]       # Tp 1 out of two frames


def head_setup(case, seed=400):
    B, C, K, To, Ho, kt, with_mask = case
    feats, w, b, mask = O.head_inputs(seed + C + K, B, C, To, Ho, Ho, kt, K, with_mask)
    return feats, w, b, mask, To - kt + 1


def head_bounds(case, feats, w, b, mask):
    """|z| terms and the forward bounds.  pooled: n_win adds, the rounded 1 / n_win, the multiplication by it and by the mask:
    k = n_win + 3.  z = b + sum_c w pooled: C products and C adds on top: k = C + n_win + 5 (the longest path of any term)."""
    B, C, K, To, Ho, kt, _ = case
    nwin = kt * Ho * Ho
    _, drop_abs, _, z_abs = O.head_forward(d64(feats).abs(), d64(w).abs(), d64(b).abs(), kt, Ho, Ho, None if mask is None else d64(mask).abs())
    return O.gamma(nwin + 3) * drop_abs, O.gamma(C + nwin + 5) * z_abs.max(dim=2).values, drop_abs, nwin


def run_head_train_fwd(case, feats, w, b, mask, Tp):
    B, C, K, To, Ho, kt, _ = case
    dropped = torch.full((B, Tp, C), 7.0).cuda()
    logits = torch.full((B, K), 7.0).cuda()
    amax = torch.full((B, K), -9, dtype=torch.int32).cuda()
    ok("vd_head_train_fwd", P(dev(feats)), P(dev(mask)), P(dev(w)), P(dev(b)), I64(B), C, To, Ho, Ho, kt, Ho, Ho, K, P(dropped),
       P(logits), P(amax))
    return dropped, logits, amax


@pytest.mark.parametrize("case", HEAD_CASES, ids=str)
def test_head_forward(case):
    B, C, K, To, Ho, kt, _ = case
    feats, w, b, mask, Tp = head_setup(case)
    # inference head: no mask.  Only its logits are compared: a maximum over frames is continuous at a tie, so the unmasked
    # logits need no tie-free draw (the draw's guarantee covers the masked logits, whose arg-max is compared below)
    b_drop, b_logit, _, _ = head_bounds(case, feats, w, b, None)
    ref_logits, _, _, z = O.head_forward(d64(feats), d64(w), d64(b), kt, Ho, Ho, None)
    out = torch.full((B, K), 7.0).cuda()
    ok("vd_head_fwd", P(dev(feats)), P(dev(w)), P(dev(b)), I64(B), C, To, Ho, Ho, kt, Ho, Ho, K, P(out))
    report("head_fwd logits %s" % (case,), out, ref_logits, b_logit)
    # training head
    b_drop, b_logit, _, _ = head_bounds(case, feats, w, b, mask)
    ref_logits, ref_drop, ref_amax, _ = O.head_forward(d64(feats), d64(w), d64(b), kt, Ho, Ho, d64(mask))
    dropped, logits, amax = run_head_train_fwd(case, feats, w, b, mask, Tp)
    report("head_train_fwd logits %s" % (case,), logits, ref_logits, b_logit)
    report("head_train_fwd dropped %s" % (case,), dropped, ref_drop, b_drop)
    bits_equal("head_train_fwd amax_t %s" % (case,), amax, ref_amax.to(torch.int32))


@pytest.mark.parametrize("case", HEAD_CASES, ids=str)
def test_head_backward(case):
    B, C, K, To, Ho, kt, _ = case
    feats, w, b, mask, Tp = head_setup(case)
    dropped, logits, amax = run_head_train_fwd(case, feats, w, b, mask, Tp)
    g = O.gen(450 + C + K)
    dl = torch.randn(B, K, generator=g) / B
    gw0, gb0 = torch.randn(K, C, generator=g) * 0.1, torch.randn(K, generator=g) * 0.1          # the parameter gradients ACCUMULATE
    f64, w64, b64 = d64(feats).requires_grad_(True), d64(w).requires_grad_(True), d64(b).requires_grad_(True)
    ref_logits, _, ref_amax, _ = O.head_forward(f64, w64, b64, kt, Ho, Ho, d64(mask))
    bits_equal("head_bwd: amax_t of the forward %s" % (case,), amax, ref_amax.to(torch.int32))
    r_gw, r_gb, r_gf = torch.autograd.grad((ref_logits * dl.double()).sum(), (w64, b64, f64))
    # bounds.  g_w[k][c] = g_w0 + sum_clip dl * dropped: dropped carries its own n_win + 3 roundings (it is the forward's fp32
    # output), one product, B adds (atomics, any order): k = n_win + 4 + B.  g_b: B adds.  g_feats = (1 / n_win) sum over <= kt
    # windows of mask * sum_k dl w: K products and K adds, the mask, kt adds, the rounded 1 / n_win and its product: k = K + kt + 4.
    _, _, drop_abs, nwin = head_bounds(case, feats, w, b, mask)
    onehot = (ref_amax[:, :, None] == torch.arange(Tp)[None, None, :]).double()                  # (B, K, Tp)
    t_gw = gw0.double().abs() + torch.einsum("bkt,bk,btc->kc", onehot, dl.double().abs(), drop_abs)
    t_gb = gb0.double().abs() + dl.double().abs().sum(0)
    dp_abs = torch.einsum("bkt,bk,kc->btc", onehot, dl.double().abs(), d64(w).abs())
    if mask is not None:
        dp_abs = dp_abs * d64(mask).abs().permute(0, 2, 1)
    t_gf = torch.zeros(B, C, To, dtype=torch.float64)
    for t in range(To):
        for tp in range(max(0, t - kt + 1), min(t, Tp - 1) + 1):
            t_gf[:, :, t] += dp_abs[:, tp, :] / nwin
    t_gf = t_gf[:, :, :, None, None].expand(B, C, To, Ho, Ho)
    outs = {}
    for form in ("vd_head_train_bwd", "vd_head_train_bwd_ordered", "vd_head_train_bwd_ordered"):
        gw, gb, gf = gw0.clone().cuda(), gb0.clone().cuda(), torch.full((B, C, To, Ho, Ho), 7.0).cuda()
        ok(form, P(dev(dl)), P(amax), P(dropped), P(dev(mask)), P(dev(w)), I64(B), C, To, Ho, Ho, kt, Ho, Ho, K, P(gw), P(gb), P(gf))
        outs.setdefault(form, []).append((gw, gb, gf))
    for form, runs in outs.items():
        gw, gb, gf = runs[0]
        report("%s g_w %s" % (form[8:], case), gw, r_gw + gw0.double(), O.gamma(nwin + 4 + B) * t_gw)
        report("%s g_b %s" % (form[8:], case), gb, r_gb + gb0.double(), O.gamma(B + 1) * t_gb)
        report("%s g_feats %s" % (form[8:], case), gf, r_gf, O.gamma(K + kt + 4) * t_gf)
    (a_gw, a_gb, a_gf), (o1, o2) = outs["vd_head_train_bwd"][0], outs["vd_head_train_bwd_ordered"]
    for name, x, y in zip(("g_w", "g_b", "g_feats"), o1, o2):
        bits_equal("head_train_bwd_ordered %s run 1 == run 2 %s" % (name, case), x.view(torch.int32), y.view(torch.int32))
    # ordered against atomic, same fp32 inputs: they differ by the summation order over the B clips and by the rounding of each
    # product (the gather fuses it into its add): twice k = B + 2
    report("head bwd ordered vs atomic g_w %s" % (case,), o1[0], a_gw.double().cpu(), 2 * O.gamma(B + 2) * t_gw)
    report("head bwd ordered vs atomic g_b %s" % (case,), o1[1], a_gb.double().cpu(), 2 * O.gamma(B + 1) * t_gb)
    bits_equal("head bwd ordered vs atomic g_feats %s" % (case,), o1[2].view(torch.int32), a_gf.view(torch.int32).cpu())


def test_head_rejects_windows_that_do_not_collapse():
    """Ho - kh + 1 != 1 (or Wo, or no frame left): -2 before any launch, from all five head entry points."""
    n = VP(0)
    assert call("vd_head_fwd", n, n, n, I64(1), 8, 2, 2, 2, 1, 1, 2, 3, n) == -2
    assert call("vd_head_train_fwd", n, n, n, n, I64(1), 8, 2, 2, 2, 1, 2, 1, 3, n, n, n) == -2
    assert call("vd_head_train_bwd", n, n, n, n, n, I64(1), 8, 2, 2, 2, 1, 1, 2, 3, n, n, n) == -2
    assert call("vd_head_train_bwd_ordered", n, n, n, n, n, I64(1), 8, 1, 1, 1, 2, 1, 1, 3, n, n, n) == -2
    assert call("vd_head_second_order", n, n, n, n, n, n, n, n, n, I64(1), 8, 2, 2, 2, 1, 1, 2, 3, n, n, n, n) == -2


# ================================================================================================ vd_ce_loss
def run_ce(logits, labels):
    B, K = logits.shape
    loss, dl = torch.full((B,), 7.0).cuda(), torch.full((B, K), 7.0).cuda()
    ok("vd_ce_loss", P(dev(logits)), P(dev(labels)), B, K, P(loss), P(dl))
    return loss.cpu(), dl.cpu()


def ce_check(tag, logits, labels, loss, dl, rows):
    B, K = logits.shape
    z = logits.double()[rows].requires_grad_(True)
    y = labels[rows]
    per = O.ce_per_clip(z, y)
    (gref,) = torch.autograd.grad(per.sum() / B, z)
    # the kernel evaluates in fp64 and rounds ONCE to fp32: k = 1 on |lse| + |z_y| (which also covers the fp64 evaluation itself)
    lse = (per + z.gather(1, y[:, None]).squeeze(1)).detach()
    report("ce_loss loss %s" % (tag,), loss[rows], per.detach(), O.gamma(1) * (lse.abs() + z.detach().gather(1, y[:, None]).squeeze(1).abs()))
    # dlogits = (p - onehot) / B rounded once; a second unit covers exp(z - lse) in fp64 with |z - lse| <= 60
    p = (z.detach() - lse[:, None]).exp()
    onehot = torch.nn.functional.one_hot(y, K).double()
    report("ce_loss dlogits %s" % (tag,), dl[rows], gref, O.gamma(2) * (p + onehot) / B)
    # probabilities recovered from dlogits sum to one within 2 ulp of fp32
    psum = (dl[rows].double() * B + onehot).sum(1)
    print("%-58s |sum p - 1| %.3e  bound %.3e" % ("ce_loss softmax sums %s" % (tag,), float((psum - 1).abs().max()), 2 * ULP))
    RECORDS.append({"check": "ce_loss softmax sums %s" % (tag,), "error": float((psum - 1).abs().max()), "bound": 2 * ULP})
    assert float((psum - 1).abs().max()) <= 2 * ULP


@pytest.mark.parametrize("B,K", [(9, 64), (1, 1), (9, 2), (1, 63), (9, 65), (9, 300), (1, 300)])
def test_ce_loss(B, K):
    logits, labels = O.ce_inputs(500 + K, B, K, spread=60.0)
    loss, dl = run_ce(logits, labels)
    ce_check((B, K), logits, labels, loss, dl, torch.arange(B))


@pytest.mark.parametrize("bad", [-1, 65])
def test_ce_loss_label_out_of_range_is_nan_for_that_clip_only(bad):
    """The documented behaviour (torch raises; without a host sync the loud failure is NaN): not a fault."""
    logits, labels = O.ce_inputs(501, 9, 65, bad_label=(4, bad))
    loss, dl = run_ce(logits, labels)
    assert math.isnan(float(loss[4])) and bool(torch.isnan(dl[4]).all())
    rows = torch.tensor([0, 1, 2, 3, 5, 6, 7, 8])
    assert bool(torch.isfinite(loss[rows]).all()) and bool(torch.isfinite(dl[rows]).all())
    ce_check("(9, 65) label %d" % bad, logits, labels, loss, dl, rows)


# ================================================================================================ vd_head_second_order
def second_order_reference(dtype, case, feats, w, b, mask, labels, dl_free, v_w, v_b, gbar):
    """S = <v_w, dL/dw> + <v_b, dL/db> + <gbar, dL/dfeats> differentiated once more, by autograd in `dtype`.  labels given: L = mean
    CE of the oracle head (the loss Hessian included).  dl_free given: the caller's own loss -- the first derivatives are the
    head's vector-Jacobian products with the cotangent dl_free, which is also differentiated (dlogbar)."""
    B, C, K, To, Ho, kt, _ = case
    c = lambda t: None if t is None else t.to(dtype)
    f, ww, bb = c(feats).requires_grad_(True), c(w).requires_grad_(True), c(b).requires_grad_(True)
    logits = O.head_forward(f, ww, bb, kt, Ho, Ho, c(mask))[0]
    if labels is not None:
        g_w, g_b, g_f = torch.autograd.grad(O.ce_per_clip(logits, labels).mean(), (ww, bb, f), create_graph=True)
        dl = None
    else:
        dl = c(dl_free).requires_grad_(True)
        g_w, g_b, g_f = torch.autograd.grad(logits, (ww, bb, f), grad_outputs=dl, create_graph=True)
    S = (g_w * c(v_w)).sum() + (g_b * c(v_b)).sum() + (g_f * c(gbar)).sum()
    wanted = (f, ww, bb) + (() if dl is None else (dl,))
    grads = torch.autograd.grad(S, wanted, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, wanted)]
    return {"abar": grads[0], "wbar": grads[1], "bbar": grads[2], "dlogbar": grads[3] if dl is not None else None}


@pytest.mark.parametrize("with_logits,with_pbar", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("case", [HEAD_CASES[0], HEAD_CASES[2], HEAD_CASES[3], HEAD_CASES[5]], ids=str)
def test_head_second_order(case, with_logits, with_pbar):
    B, C, K, To, Ho, kt, _ = case
    feats, w, b, mask, Tp = head_setup(case)
    g = O.gen(600 + C + K)
    labels = torch.randint(0, K, (B,), generator=g)
    v_w, v_b = torch.randn(K, C, generator=g), torch.randn(K, generator=g)
    gbar = torch.randn(B, C, To, Ho, Ho, generator=g)
    dl_free = torch.randn(B, K, generator=g) / B
    dropped, logits, amax = run_head_train_fwd(case, feats, w, b, mask, Tp)
    if with_logits:
        loss, dl = torch.empty(B).cuda(), torch.empty(B, K).cuda()
        ok("vd_ce_loss", P(logits), P(dev(labels)), B, K, P(loss), P(dl))
    else:
        dl = dev(dl_free)
    abar = torch.full((B, C, To, Ho, Ho), 7.0).cuda()
    wbar, bbar = (torch.zeros(K, C).cuda(), torch.zeros(K).cuda()) if with_pbar else (None, None)
    dlogbar = None if with_logits else torch.full((B, K), 7.0).cuda()
    ok("vd_head_second_order", P(logits if with_logits else None), P(dl), P(amax), P(dropped), P(dev(mask)), P(dev(w)), P(dev(v_w)),
       P(dev(v_b)), P(dev(gbar)), I64(B), C, To, Ho, Ho, kt, Ho, Ho, K, P(abar), P(wbar), P(bbar), P(dlogbar))
    args = (case, feats, w, b, mask, labels if with_logits else None, dl_free, v_w, v_b, gbar)
    r64, r32 = second_order_reference(torch.float64, *args), second_order_reference(torch.float32, *args)
    tag = "%s logits=%d pbar=%d" % (case, with_logits, with_pbar)
    report_yard("head_second_order abar_feats " + tag, abar, r64["abar"], r32["abar"])
    if with_pbar:
        report_yard("head_second_order wbar " + tag, wbar, r64["wbar"], r32["wbar"])
        if with_logits:
            report_yard("head_second_order bbar " + tag, bbar, r64["bbar"], r32["bbar"])
        else:          # no loss Hessian: the head's parameter gradients do not depend on its bias
            bits_equal("head_second_order bbar (no Hessian) " + tag, bbar.view(torch.int32), torch.zeros(K, dtype=torch.int32))
    if not with_logits:
        report_yard("head_second_order dlogbar " + tag, dlogbar, r64["dlogbar"], r32["dlogbar"])


# ================================================================================================ vd_match_rows_fwd / _bwd
MATCH_CASES = [(300, 7), (1, 1), (63, 2), (64, 8), (65, 9), (300, 64), (30000, 1), (30000, 7), (63, 65), (300, 1000), (1, 1000),
               (64, 1), (65, 1), (1, 8), (300, 2)]


def match_inputs(rows, length):
    g = O.gen(700 + rows + length)
    gr, gs = torch.randn(rows, length, generator=g), torch.randn(rows, length, generator=g)
    if rows > 1:
        gs[rows // 2] = 0.0          # an all-zero s row: the ns > 0 guard of the backward, 1 - 0 / (0 + 1e-6) = 1 in the forward
    return gr, gs


def match_batch(gr, gs, gout_buf, rows, length):
    from video_distillation_amd import hip
    b = hip.VdMatchBatch()
    b.nseg, b.reserved = 1, 0
    b.seg[0].gr, b.seg[0].gs, b.seg[0].g = gr.data_ptr(), gs.data_ptr(), 0 if gout_buf is None else gout_buf.data_ptr()
    b.seg[0].rows, b.seg[0].len, b.seg[0].reserved = rows, length, 0
    return b


def match_sum_bounds(gr, gs, acc0):
    """sums 1..4 are plain sums of products.  Longest path of one term: its product (and the subtraction of 'mse'), <= len adds
    within the row, <= ceil(rows / 64) adds in the thread's running sum (a wave owns at least 64 rows per round, so no thread sees
    more), the 6-level wave tree and <= 16 adds over the waves of a block, <= min(rows, 1024) same-address atomics -- which also
    round the value acc held before the call."""
    rows, length = gr.shape
    k = 2 + length + math.ceil(rows / 64) + 6 + 16 + min(rows, 1024)
    r, s = gr.double().abs(), gs.double().abs()
    return O.gamma(k) * (torch.stack([((s + r) ** 2).sum(), (r * s).sum(), (r * r).sum(), (s * s).sum()]) + acc0.double().abs()[1:])


@pytest.mark.parametrize("rows,length", MATCH_CASES)
def test_match_rows_forward(rows, length):
    """All five sums of the single-tensor form and of the _multi form on the same data.  [rows][len] is a ROW view for every len:
    with len == 1 each element is its own cosine row (acc[0] = sum of 1 - sign agreement), as the header says and as
    vd_match_rows_bwd mode 0 differentiates."""
    from video_distillation_amd import hip
    gr, gs = match_inputs(rows, length)
    ref = O.match_sums(gr.double(), gs.double())
    ref32 = O.match_sums(gr, gs)
    acc0 = torch.tensor([0.5, -1.0, 2.0, 0.25, 3.0])          # the sums ACCUMULATE onto acc
    bounds = match_sum_bounds(gr, gs, acc0)
    a, b = dev(gr), dev(gs)
    single = acc0.clone().cuda()
    ok("vd_match_rows_fwd", P(a), P(b), I64(rows), length, P(single))
    multi = acc0.clone().cuda()
    ok("vd_match_rows_fwd_multi", ctypes.byref(match_batch(a, b, None, rows, length)), P(multi))
    for tag, acc in (("single", single), ("multi", multi)):
        got = acc.cpu().double() - acc0.double()
        report("match_rows_fwd %s sums 1..4 (%d, %d)" % (tag, rows, length), got[1:], ref[1:], bounds)
        # the cosine sum: yardstick (near-zero norms make a term-wise bound impractical)
        report_yard("match_rows_fwd %s cosine sum (%d, %d)" % (tag, rows, length), got[:1], ref[:1], ref32[:1])
    # equality of the two forms to summation error: both lie within the bounds above of the same fp64 sums
    report("match_rows_fwd single vs multi (%d, %d)" % (rows, length), single[1:], multi[1:].double().cpu(), 2 * bounds)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rows,length", MATCH_CASES)
def test_match_rows_backward(rows, length, mode):
    gr, gs = match_inputs(rows, length)
    gout = 0.75
    s64 = gs.double().requires_grad_(True)
    (gref,) = torch.autograd.grad(O.match_metric(gr.double(), s64, mode) * gout, s64)
    s32 = gs.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(O.match_metric(gr, s32, mode) * gout, s32)
    acc = O.match_sums(gr.double(), gs.double()).float()          # mode 2 reads the forward's global sums
    a, b = dev(gr), dev(gs)
    g1, g2 = torch.full((rows, length), 7.0).cuda(), torch.full((rows, length), 7.0).cuda()
    go = torch.tensor([gout]).cuda()
    ok("vd_match_rows_bwd", P(a), P(b), I64(rows), length, mode, P(dev(acc)), P(go), P(g1))
    ok("vd_match_rows_bwd_multi", ctypes.byref(match_batch(a, b, g2, rows, length)), mode, P(dev(acc)), P(go))
    for tag, got in (("single", g1.cpu()), ("multi", g2.cpu())):
        label = "match_rows_bwd %s mode %d (%d, %d)" % (tag, mode, rows, length)
        if mode == 1:      # gout * 2 * (s - r): the subtraction and one product (2 x is exact): k = 2
            report(label, got, gref, O.gamma(2) * 2 * gout * (gs.double().abs() + gr.double().abs()))
            continue
        zero = torch.zeros(rows, dtype=torch.bool)
        if mode == 0 and rows > 1:      # the all-zero s row has gradient -gout r / 1e-6: a scale of its own
            zero[rows // 2] = True
            report_yard(label + " zero-norm row", got[zero], gref[zero], g32[zero])
        if int((~zero).sum()):
            report_yard(label, got[~zero], gref[~zero], g32[~zero])


# ================================================================================================ vd_absmax_scale / vd_scale_combine
def f32(v):
    return float(np.float32(v))


def float_bits(v):
    return int(np.float32(v).view(np.uint32))


def run_absmax(x, target):
    out = torch.full((4,), 7.0).cuda()
    ok("vd_absmax_scale", P(dev(x)), I64(x.numel()), F32(target), P(out))
    o = out.cpu()
    return float(o[0]), float(o[1]), int(o.view(torch.int32)[2]) & 0xffffffff


def absmax_check(label, x, target, must_hold=True):
    s, inv, word = run_absmax(x, target)
    m = float(x.double().abs().max()) if x.numel() else 0.0
    k = O.absmax_exponent(m, f32(target))
    print("%-58s max|g| %.9g target %g -> scale %g (want 2^%s), max|g| * scale %.9g" % (label, m, target, s, k, m * s))
    RECORDS.append({"check": label, "error": 0 if (k is None and s == 1.0) or (k is not None and s == 2.0 ** k) else 1, "bound": 0})
    assert word == float_bits(m), "%s: absmax word %#x, max|g| has bits %#x" % (label, word, float_bits(m))
    assert s > 0 and math.frexp(s)[0] == 0.5, "%s: scale %r is not a power of two" % (label, s)
    assert inv == 1.0 / s and s * inv == 1.0, "%s: out[1] = %r is not 1 / %r" % (label, inv, s)
    if k is None:
        assert s == 1.0, label
        return
    if must_hold:      # exact: a float times a power of two is exact in fp64
        assert f32(target) / 2 <= m * s < f32(target), "%s: max|g| * scale = %.9g outside [%g, %g)" % (label, m * s, target / 2, target)
    assert s == 2.0 ** k, "%s: scale 2^%d, want 2^%d" % (label, round(math.log2(s)), k)


def noise(n, seed, amp=0.2):
    return (torch.rand(n, generator=O.gen(seed)) - 0.5) * amp


@pytest.mark.parametrize("n,pos", [(1, 0), (2047, 0), (2049, 2048), (1024 * 2048 + 5, 1024 * 2048 + 3), (1024 * 2048 + 5, 0), (2049, 1000)])
def test_absmax_scale_sizes_and_position_of_the_maximum(n, pos):
    x = noise(n, 800 + n)
    x[pos] = -3.0 if pos % 2 == 0 else 3.0          # (a negative maximum too)
    absmax_check("absmax_scale n=%d max at %d" % (n, pos), x, 1024.0)


def test_absmax_scale_at_and_around_powers_of_two():
    """target / max|g| an exact power of two lands ON target with floor(log2(target / m)); one ulp either side of it the result
    hinges on log2f's rounding.  The interval is half-open: 0.25 -> 2^11 (512), not 2^12 (1024 = target)."""
    quarter = np.float32(0.25)
    for name, m in (("exact power of two", quarter), ("one ulp below", np.nextafter(quarter, np.float32(0))),
                    ("one ulp above", np.nextafter(quarter, np.float32(1))), ("max == target", np.float32(1024.0)),
                    ("one ulp below target", np.nextafter(np.float32(1024.0), np.float32(0))), ("target / 2", np.float32(512.0))):
        x = noise(300, 810)
        x[17] = float(m)
        absmax_check("absmax_scale %s (max %.9g)" % (name, float(m)), x, 1024.0)
    x = noise(300, 811)
    x[5] = -0.75
    absmax_check("absmax_scale target 100 (not a power of two)", x, 100.0)
    x[5] = -0.78125          # 100 / 0.78125 = 128
    absmax_check("absmax_scale target 100, target / max = 128", x, 100.0)


def test_absmax_scale_extreme_values():
    absmax_check("absmax_scale all zero", torch.zeros(5000), 1024.0)
    x = noise(300, 820, amp=1e37)
    x[299] = f32(3e38)
    absmax_check("absmax_scale max 3e38", x, 1024.0)
    x[299] = -f32(3e38)
    absmax_check("absmax_scale max -3e38", x, 1024.0)
    sub = torch.zeros(300)
    sub[7] = f32(1e-40)
    sub[8] = -f32(2.0 ** -149)
    absmax_check("absmax_scale subnormal max, target 2^-100", sub, 2.0 ** -100)
    # out of reach: 2^k would have to be 2^142; the documented clamp (k <= 126: 2^k and 2^-k stay normal floats) applies
    absmax_check("absmax_scale subnormal max, target 1024 (clamped)", sub, 1024.0, must_hold=False)


@pytest.mark.parametrize("mode", [0, 1])
def test_scale_combine(mode):
    def blk(s, word):          # a 4-float block as vd_absmax_scale leaves it: scale, 1 / scale, the float bits of max|g|
        arr = np.array([s, 1.0 / s, 0.0, 0.0], dtype=np.float32)
        arr.view(np.uint32)[2] = word
        return torch.from_numpy(arr)
    live, empty = float_bits(0.37), 0
    for a, b in (((4.0, live), (0.125, live)), ((0.125, live), (4.0, live)), ((4.0, live), None), ((4.0, empty), (0.125, live)),
                 ((0.125, live), (4.0, empty)), ((4.0, empty), (0.125, empty)), ((4.0, empty), None), ((2.0 ** 60, live), (2.0 ** -90, live))):
        out = torch.full((4,), 7.0).cuda()
        ta, tb = dev(blk(*a)), None if b is None else dev(blk(*b))
        ok("vd_scale_combine", P(ta), P(tb), mode, P(out))
        want = O.scale_combine((a[0], 1 / a[0], a[1]), None if b is None else (b[0], 1 / b[0], b[1]), mode)
        o = out.cpu()
        print("scale_combine mode %d a=%s b=%s -> %g (want %g)" % (mode, a, b, float(o[0]), want))
        RECORDS.append({"check": "scale_combine mode %d a=%s b=%s" % (mode, a, b),
                        "error": 0 if float(o[0]) == want and float(o[1]) == 1.0 / want else 1, "bound": 0})
        assert float(o[0]) == want and float(o[1]) == 1.0 / want
    assert call("vd_scale_combine", P(ta), P(tb), 2, P(out)) == -2 and call("vd_scale_combine", VP(0), P(tb), 0, P(out)) == -2


# ================================================================================================ 16-bit operand formats
PRECS = [O.PREC_BF16, O.PREC_F16, O.PREC_BF16X3, O.PREC_F16X3]


def tiled_edges(n, seed):
    base = O.edge_values16(seed, min(n, 1 << 16))
    return base.repeat((n + base.numel() - 1) // base.numel())[:n].contiguous()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_round_operand(n, prec):
    x = tiled_edges(n, 900 + n)
    out = torch.full((n,), 7.0).cuda()
    ok("vd_round_operand", P(dev(x)), I64(n), prec, P(out))
    bits_equal("round_operand n=%d prec %d" % (n, prec), out.view(torch.int32), O.round_operand(x, prec).view(torch.int32))
    xin = dev(x)          # in place: out may alias w
    ok("vd_round_operand", P(xin), I64(n), prec, P(xin))
    bits_equal("round_operand in place n=%d prec %d" % (n, prec), xin.view(torch.int32), O.round_operand(x, prec).view(torch.int32))


# n: one float4, a partial last block, exactly the grid cap of 8192 blocks x 256 threads x 4 elements, and one float4 past it
@pytest.mark.parametrize("n,prec,with_lo,scale", [(4, O.PREC_F16X3, True, None), (1020, O.PREC_BF16X3, True, 0.5), (1028, O.PREC_F16, False, 3.0),
                                                  (1024, O.PREC_BF16, False, None), (4096, O.PREC_F16X3, True, 2.0 ** -3),
                                                  (8192 * 256 * 4, O.PREC_F16X3, True, None), (8192 * 256 * 4 + 4, O.PREC_BF16X3, True, 0.75),
                                                  (4096, O.PREC_F16X3, False, 1.7), (4096, O.PREC_BF16, True, None)])
def test_split_scaled(n, prec, with_lo, scale):
    x = tiled_edges(n, 910 + (n % 977))
    if scale is not None and scale > 1:
        x = x.clamp(-6.0e4 / scale, 6.0e4 / scale)          # the scaled value stays finite in fp16 (no Inf anywhere)
    hi = torch.full((n,), 0x5555, dtype=torch.int16).cuda()
    lo = torch.full((n,), 0x5555, dtype=torch.int16).cuda() if with_lo else None
    sc = None if scale is None else torch.tensor([scale]).cuda()
    ok("vd_split_scaled", P(dev(x)), I64(n), P(sc), P(hi), P(lo), prec)
    whi, wlo = O.split_scaled(x, scale, prec)
    bits_equal("split_scaled hi n=%d prec %d scale %s" % (n, prec, scale), hi, whi)
    if with_lo:
        bits_equal("split_scaled lo n=%d prec %d scale %s" % (n, prec, scale), lo, wlo)
        # hi + lo reproduces the (scaled) input to the pair precision: 2^-22 relative while lo is a normal fp16 number
        # (|v| >= 2^-2); a bf16 pair carries 16 bits: 2^-16
        v = x.double() * (1.0 if scale is None else f32(scale))
        back = O.decode16(hi.cpu(), prec) + O.decode16(lo.cpu(), prec)
        big = v.abs() >= 0.25
        rel = float(((back - v).abs() / v.abs().clamp_min(1e-30))[big].max()) if bool(big.any()) else 0.0
        bound = 2.0 ** -22 if prec == O.PREC_F16X3 or prec == O.PREC_F16 else 2.0 ** -16
        print("split_scaled hi + lo pair precision: %.3e (bound %.3e)" % (rel, bound))
        RECORDS.append({"check": "split_scaled hi + lo relative pair precision n=%d prec %d scale %s" % (n, prec, scale),
                        "error": rel, "bound": bound})
        assert rel <= bound


def test_split_scaled_rejects_bad_sizes_and_alignment_before_any_launch():
    x = torch.zeros(16).cuda()
    hi, lo = torch.zeros(16, dtype=torch.int16).cuda(), torch.zeros(16, dtype=torch.int16).cuda()
    for n in (1, 2, 3, 5, 7):
        assert call("vd_split_scaled", P(x), I64(n), VP(0), P(hi), P(lo), O.PREC_F16X3) == -2
    assert call("vd_split_scaled", VP(x.data_ptr() + 4), I64(8), VP(0), P(hi), P(lo), O.PREC_F16X3) == -2
    assert call("vd_split_scaled", P(x), I64(8), VP(0), VP(hi.data_ptr() + 2), P(lo), O.PREC_F16X3) == -2
    assert call("vd_split_scaled", P(x), I64(8), VP(0), P(hi), VP(lo.data_ptr() + 4), O.PREC_F16X3) == -2
    assert call("vd_split_scaled", P(x), I64(8), VP(0), P(hi), P(lo), 4) == -2
    assert call("vd_split_scaled", VP(0), I64(8), VP(0), P(hi), P(lo), 0) == -2
    assert int(hi.abs().max()) == 0 and int(lo.abs().max()) == 0


# n: one element, a partial block, and three past the grid cap of 16384 blocks x 256 threads (the grid-stride tail)
@pytest.mark.parametrize("n,sprec,dprec,src_lo,dst_lo", [(4097, O.PREC_F16X3, O.PREC_BF16X3, True, True), (1, O.PREC_BF16X3, O.PREC_F16X3, True, True),
                                                         (255, O.PREC_F16, O.PREC_BF16X3, False, True), (257, O.PREC_BF16X3, O.PREC_F16, True, False),
                                                         (16384 * 256 + 3, O.PREC_F16X3, O.PREC_BF16X3, True, True),
                                                         (4097, O.PREC_BF16, O.PREC_F16, False, False), (4097, O.PREC_F16X3, O.PREC_F16X3, True, True)])
def test_resplit_slots(n, sprec, dprec, src_lo, dst_lo):
    x = tiled_edges(n, 920 + (n % 977))
    shi, slo = O.split16(x, sprec)
    dhi = torch.full((n,), 0x5555, dtype=torch.int16).cuda()
    dlo = torch.full((n,), 0x5555, dtype=torch.int16).cuda() if dst_lo else None
    ok("vd_resplit_slots", P(dev(shi)), P(dev(slo) if src_lo else None), I64(n), sprec, P(dhi), P(dlo), dprec)
    whi, wlo = O.resplit(shi, slo if src_lo else None, sprec, dprec)
    bits_equal("resplit hi n=%d %d->%d" % (n, sprec, dprec), dhi, whi)
    if dst_lo:
        bits_equal("resplit lo n=%d %d->%d" % (n, sprec, dprec), dlo, wlo)


# ================================================================================================ vd_pix2rows
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("W", [8, 12, 13, 37, 64])
def test_pix2rows(W, prec):
    """W % 4 == 0 takes the float4 path, the others the scalar one; with clip_index (repeats and a permutation) and without."""
    T, H, pool = 2, 3, 4
    x = tiled_edges(pool * T * 3 * H * W, 930 + W).reshape(pool, T, 3, H, W)
    pitch = (W + 8 + 7) // 8 * 8
    for idx in (None, torch.tensor([2, 0, 3, 3, 1, 0])):
        nclips = pool if idx is None else idx.numel()
        hi = torch.full((nclips, T * 3, H, pitch), 0x5555, dtype=torch.int16).cuda()
        lo = torch.full((nclips, T * 3, H, pitch), 0x5555, dtype=torch.int16).cuda() if O.has_lo(prec) else None
        ok("vd_pix2rows", P(dev(x)), P(dev(idx)), I64(nclips), T, H, W, P(hi), P(lo), prec)
        whi, wlo = O.pix2rows(x, idx, prec)
        bits_equal("pix2rows hi W=%d prec %d index %s" % (W, prec, idx is not None), hi, whi)
        if lo is not None:
            bits_equal("pix2rows lo W=%d prec %d index %s" % (W, prec, idx is not None), lo, wlo)


# ================================================================================================ vd_unpool_relu_bwd
#                g_layout pool_t T  OH OW  scale  prec            (layout 1 + even OH, OW: the window form; otherwise the slot form)
UNPOOL_CASES = [(1, 2, 4, 6, 8, None, O.PREC_F16X3), (1, 1, 3, 4, 4, 0.5, O.PREC_BF16X3), (1, 2, 5, 6, 4, 3.0, O.PREC_F16),
                (1, 2, 4, 5, 7, None, O.PREC_BF16), (1, 1, 2, 6, 5, 0.5, O.PREC_F16X3), (0, 2, 4, 6, 8, None, O.PREC_F16X3),
                (0, 2, 5, 5, 6, 0.25, O.PREC_BF16X3), (0, 1, 3, 4, 7, None, O.PREC_F16), (0, 1, 1, 2, 2, 2.0, O.PREC_BF16),
                (1, 2, 1, 2, 2, None, O.PREC_F16X3)]


@pytest.mark.parametrize("g_layout,pool_t,T,OH,OW,scale,prec", UNPOOL_CASES)
def test_unpool_relu_bwd(g_layout, pool_t, T, OH, OW, scale, prec):
    nclips, C = 3, 16
    To, Ho, Wo = T // pool_t, OH // 2, OW // 2
    npos = To * Ho * Wo
    n = nclips * C * npos
    g = tiled_edges(max(n, 1), 940 + T + OH + OW).clamp(-2.0e4, 2.0e4)[:n]
    am = O.argmax_bytes(941 + T + OH, (n,), pool_t)
    slots = nclips * (C // 8) * T * OH * OW
    hi = torch.full((slots, 8), 0x5555, dtype=torch.int16).cuda()
    lo = torch.full((slots, 8), 0x5555, dtype=torch.int16).cuda() if O.has_lo(prec) else None
    sc = None if scale is None else torch.tensor([scale]).cuda()
    gd, amd = (dev(g), dev(am)) if n else (torch.zeros(4).cuda(), torch.zeros(8, dtype=torch.uint8).cuda())
    ok("vd_unpool_relu_bwd", P(gd), P(amd), I64(nclips), C, To, Ho, Wo, pool_t, T, OH, OW, g_layout, P(hi), P(lo), prec, P(sc))
    whi, wlo = O.unpool_relu_bwd(g, am, nclips, C, To, Ho, Wo, pool_t, T, OH, OW, g_layout, prec, scale)
    tag = "layout %d pool_t %d T %d grid %dx%d scale %s prec %d" % (g_layout, pool_t, T, OH, OW, scale, prec)
    bits_equal("unpool_relu_bwd hi " + tag, hi, whi)
    if lo is not None:
        bits_equal("unpool_relu_bwd lo " + tag, lo, wlo)
    assert n == 0 or (int((am >= 128).sum()) > 0 and int((whi != 0).sum()) > 0)
    assert call("vd_unpool_relu_bwd", P(gd), P(amd), I64(nclips), 12, To, Ho, Wo, pool_t, T, OH, OW, g_layout, P(hi), P(lo), prec, P(sc)) == -2
    assert call("vd_unpool_relu_bwd", P(gd), P(amd), I64(nclips), C, To, Ho, Wo, 3, T, OH, OW, g_layout, P(hi), P(lo), prec, P(sc)) == -2


# ================================================================================================ bias gradients
@pytest.mark.parametrize("nclips,C,npos,g_layout", [(3, 128, 5000, 1), (1, 8, 1, 0), (3, 64, 255, 0), (1, 256, 256, 1), (3, 8, 257, 1),
                                                    (1, 128, 257, 0), (3, 256, 5000, 0), (1, 64, 1, 1), (3, 128, 256, 0)])
def test_bias_grad_pooled(nclips, C, npos, g_layout):
    from video_distillation_amd import hip
    gen = O.gen(1000 + C + npos)
    g = torch.randn(nclips * C * npos, generator=gen)
    am = O.argmax_bytes(1001 + C + npos, (nclips * C * npos,), 2, dead_fraction=0.3)
    db0 = torch.randn(C, generator=gen)          # accumulation onto a non-zero db
    ref = O.bias_grad_pooled(g.double(), am, nclips, C, npos, g_layout) + db0.double()
    terms = O.bias_grad_pooled(g.double().abs(), am, nclips, C, npos, g_layout) + db0.double().abs()
    nblk = (npos + 255) // 256
    tag = "(%d, %d, %d) layout %d" % (nclips, C, npos, g_layout)
    db = db0.clone().cuda()
    ok("vd_bias_grad_pooled", P(dev(g)), P(dev(am)), I64(nclips), C, I64(npos), g_layout, P(db))
    # a workgroup owns 256 positions of one clip: <= 256 adds inside it, then one atomic per (clip, block) onto db: k = 256 + nclips nblk
    report("bias_grad_pooled " + tag, db, ref, O.gamma(256 + nclips * nblk) * terms)
    want = hip.lib().vd_bias_grad_pooled_scratch_floats(I64(nclips), C, I64(npos))
    assert want == nclips * nblk * C          # one row of C partial sums per (clip, block of 256 positions)
    runs = []
    for _ in range(2):
        scratch = torch.full((want + 64,), 1234.5).cuda()          # exactly the advertised size, and a guard behind it
        db = db0.clone().cuda()
        ok("vd_bias_grad_pooled_ordered", P(dev(g)), P(dev(am)), I64(nclips), C, I64(npos), g_layout, P(scratch), P(db))
        assert bool((scratch[want:] == 1234.5).all()), "the ordered form wrote past vd_bias_grad_pooled_scratch_floats"
        runs.append(db)
    # the same partial sums folded in index order: <= ceil(rows / 32) adds per fold lane, 32 lanes, the add onto db
    report("bias_grad_pooled_ordered " + tag, runs[0], ref, O.gamma(256 + math.ceil(nclips * nblk / 32) + 33) * terms)
    bits_equal("bias_grad_pooled_ordered run 1 == run 2 " + tag, runs[0].view(torch.int32), runs[1].view(torch.int32).cpu())


def test_bias_grad_pooled_rejects_channel_counts_it_cannot_tile():
    n = VP(0)
    for C in (24, 512):          # 256 % C != 0, C > 256
        assert call("vd_bias_grad_pooled", n, n, I64(1), C, I64(4), 0, n) == -2
        assert call("vd_bias_grad_pooled_ordered", n, n, I64(1), C, I64(4), 0, n, n) == -2


@pytest.mark.parametrize("nclips,N,npos,planes,prec,scale_inv", [(3, 64, 5000, 2, O.PREC_F16X3, 0.125), (1, 8, 1, 1, O.PREC_BF16, None),
                                                                 (3, 128, 255, 2, O.PREC_BF16X3, None), (1, 256, 256, 1, O.PREC_F16, 4.0),
                                                                 (3, 8, 257, 2, O.PREC_F16X3, None), (1, 64, 5000, 1, O.PREC_BF16, 0.5)])
def test_bias_grad_dense(nclips, N, npos, planes, prec, scale_inv):
    gen = O.gen(1100 + N + npos)
    v = torch.randn(nclips, N // 8, npos, 8, generator=gen)
    hi, lo = O.split16(v, prec)
    dy = torch.stack([hi, lo])[:planes].contiguous()          # [planes][clip][N/8][npos][8]
    db0 = torch.randn(N, generator=gen)
    db = db0.clone().cuda()
    sc = None if scale_inv is None else torch.tensor([scale_inv]).cuda()
    ok("vd_bias_grad", P(dev(dy)), I64(nclips * (N // 8) * npos), planes, I64(nclips), N, I64(npos), prec, P(sc), P(db))
    ref = O.bias_grad_dense(dy, prec, N, scale_inv) + db0.double()
    terms = O.decode16(dy, prec).abs().sum(dim=(0, 1, 3)).reshape(N) * (1.0 if scale_inv is None else scale_inv) + db0.double().abs()
    # the launch has zb = min(64, ceil(npos / 2048)) position blocks of 256 threads per (clip, channel chunk): a thread adds
    # planes * ceil(npos / (256 zb)) values, then the 6-level wave tree, 4 waves, the product with scale_inv (11), then one atomic
    # per (clip, position block) onto db: k = planes ceil(npos / (256 zb)) + 11 + zb nclips
    zb = min(64, math.ceil(npos / 2048))
    k = planes * math.ceil(npos / (256 * zb)) + 11 + zb * nclips
    report("bias_grad dense (%d, %d, %d) planes %d prec %d scale %s" % (nclips, N, npos, planes, prec, scale_inv), db, ref, O.gamma(k) * terms)
    assert call("vd_bias_grad", P(dev(dy)), I64(1), planes, I64(nclips), 12, I64(npos), prec, P(sc), P(db)) == -2


# ================================================================================================ vd_standardize(_ordered)
def run_standardize(x, ordered):
    xd = dev(x)
    out = torch.full((x.numel(),), 7.0).cuda()
    scratch = torch.full((4096,), 3.0, dtype=torch.float64).cuda()          # the plain form must zero its two doubles itself
    ok("vd_standardize_ordered" if ordered else "vd_standardize", P(xd), I64(x.numel()), P(scratch), P(out))
    return out


STD_CASES = [(4097, r) for r in range(6)] + [(300000, r) for r in range(6)] + [(2, 0), (2, 5), (4095, 0), (4095, 5),
                                                                                 (2048 * 4096 + 5, 0), (2048 * 4096 + 5, 5)]


@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("n,row", STD_CASES)
def test_standardize(n, row, ordered):
    """Every (mean, std) of the table up to mean / std = 1000: the bound is 4 x the error of the reference's own fp32 expression
    (x - x.mean()) / x.std() on that input, or 2e-6, whichever is larger.  (With fp32 partial sums of x and x^2 the one-pass
    variance loses (mean / std)^2 ulps to cancellation: 2.5e-2 of the output at mean 1000, std 1.)"""
    mean, std = O.STANDARDIZE_ROWS[row]
    x = O.standardize_input(1200 + n % 1000 + row, n, mean, std)
    ref = O.standardize(x.double())
    bound, yard = O.standardize_bound(x, ref)
    out = run_standardize(x, ordered)
    tag = "standardize%s n=%d mean %g std %g" % ("_ordered" if ordered else "", n, mean, std)
    print("%-58s fp32 torch error %.3e" % (tag, yard))
    report(tag, out, ref, bound)
    if ordered:
        bits_equal(tag + " run 1 == run 2", out.view(torch.int32), run_standardize(x, True).view(torch.int32).cpu())


def test_standardize_rejects_fewer_than_two_elements():
    x, out, scratch = torch.ones(4).cuda(), torch.zeros(4).cuda(), torch.zeros(4096, dtype=torch.float64).cuda()
    for n in (0, 1, -3):
        assert call("vd_standardize", P(x), I64(n), P(scratch), P(out)) == -2
        assert call("vd_standardize_ordered", P(x), I64(n), P(scratch), P(out)) == -2
    assert float(out.abs().max()) == 0.0


# ================================================================================================ vd_replica_sum
@pytest.mark.parametrize("replicas", [1, 2, 33, 64, 65, 200])
def test_replica_sum(replicas):
    rows, cols = 147, 37          # neither a multiple of the 32 x 32 tile
    gen = O.gen(1300 + replicas)
    rep = torch.randn(replicas, rows, cols, generator=gen)
    out0 = torch.randn(cols, rows, generator=gen)          # accumulation onto a non-zero dW
    runs = []
    for _ in range(2):
        out = out0.clone().cuda()
        ok("vd_replica_sum", P(dev(rep)), replicas, rows, cols, P(out))          # (the copies are scratch: a fresh upload per run)
        runs.append(out)
    # <= replicas adds over the copies (in groups of 32 and then the group heads above 64 copies: fewer) and the add onto out
    report("replica_sum %d copies" % replicas, runs[0], O.replica_sum(rep.double()) + out0.double(),
           O.gamma(replicas + 1) * (O.replica_sum(rep.double().abs()) + out0.double().abs()))
    bits_equal("replica_sum %d copies run 1 == run 2" % replicas, runs[0].view(torch.int32), runs[1].view(torch.int32).cpu())
