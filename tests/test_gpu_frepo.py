"""FRePo on the GPU, at 64x64x8: the two ``vdf_`` kernels through the C ABI against fp64 and, bit for bit, against the float32
restatement (tests/frepo_oracle.py); the regression train step against the fp64 route of tests/test_gpu_train.py with the loss
replaced; ``embed_exact`` and ``nfr.nfr(exact=True)``; one ``FRePoTrainer.step`` against the hand composition of the public
pieces; FRePo's ``evaluate_synset``."""
import copy
import ctypes
import math
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import frepo_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 8
CANARY = np.float32(-777.0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- vdf_mse_loss --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(1, 1), (5, 7), (50, 50), (500, 400)])
def test_mse_loss_through_the_c_abi_against_fp64_twice_bit_for_bit(B, K):
    """dlogits = (l - y) * (float)(2 / BK): two roundings and a rounded constant, 3 x 2^-24 relative; the loss is an fp64 sum
    rounded once (and the fp64 sum of BK positive terms is itself exact to ~BK x 2^-53): 2^-23 relative."""
    from video_distillation_amd import hip
    g = torch.Generator().manual_seed(B * 1000 + K)
    l, y = torch.randn(B, K, generator=g), torch.randn(B, K, generator=g) * 0.3
    want_loss, want_d = O.mse_f64(l.numpy(), y.numpy())
    ld, yd = l.cuda(), y.cuda()
    outs = []
    for _ in range(2):
        whole = torch.full((GUARD + 1 + GUARD + B * K + GUARD,), float(CANARY), dtype=torch.float32, device="cuda")
        loss, dlog = whole[GUARD:GUARD + 1], whole[2 * GUARD + 1:2 * GUARD + 1 + B * K]
        code = hip.lib().vdf_mse_loss(ld.data_ptr(), yd.data_ptr(), B, K, loss.data_ptr(), dlog.data_ptr(), hip.stream_ptr("cuda"))
        assert code == 0
        torch.cuda.synchronize()
        host = whole.cpu().numpy()
        assert np.all(host[:GUARD] == CANARY) and np.all(host[GUARD + 1:2 * GUARD + 1] == CANARY) and np.all(host[-GUARD:] == CANARY)
        outs.append((host[GUARD], host[2 * GUARD + 1:-GUARD].reshape(B, K).copy()))
    (loss_a, d_a), (loss_b, d_b) = outs
    assert np.array_equal(_bits(loss_a), _bits(loss_b)) and np.array_equal(_bits(d_a), _bits(d_b))
    err_d = np.abs(d_a.astype(np.float64) - want_d)
    print("(%d, %d): loss %.9g (fp64 %.9g, rel %.2e); dlogits worst %.2f x 2^-24 relative"
          % (B, K, loss_a, want_loss, abs(float(loss_a) - want_loss) / want_loss, float(np.max(err_d / np.abs(want_d))) / O.U))
    assert np.all(err_d <= 3 * O.U * np.abs(want_d))
    assert abs(float(loss_a) - want_loss) <= 2.0 ** -23 * want_loss
    got_loss, got_d = hip.mse_loss(ld, yd)          # the wrapper: the same launch
    assert np.array_equal(_bits(got_loss.cpu().numpy()), _bits(loss_a)) and np.array_equal(_bits(got_d.cpu().numpy()), _bits(d_a))


# ---- vdf_adam_multi ------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 1023, 1025, 28224]
KINDS = ["randn", "zero", "tiny"]


def _layout(sizes, shifts):
    """Offsets (in floats) of the segments inside one flat buffer per stream: segment k starts ``shifts[k][s]`` floats past a
    16-byte boundary in stream s (0: p, 1: m, 2: v, 3: g), with at least GUARD canary floats before and after every segment."""
    offs, at = [], [0, 0, 0, 0]
    for n, sh in zip(sizes, shifts):
        row = []
        for s in range(4):
            start = (at[s] + GUARD + 3) // 4 * 4 + sh[s]
            row.append(start)
            at[s] = start + n
        offs.append(row)
    return offs, [a + GUARD for a in at]


def _adam_case(sizes, t):
    """Host state, layout and expectation of one launch: per segment its own learning rate, every other one AdamW's decay, the
    gradient kinds in turn.  Segment 1 starts one float past a 16-byte boundary in all four streams (the 16-byte body with a
    head of three), segment 2 at different offsets in the four streams (4-byte accesses)."""
    shifts = [(0, 0, 0, 0)] * len(sizes)
    shifts[1] = (1, 1, 1, 1)
    shifts[2] = (0, 1, 2, 3)
    if len(sizes) > 5:
        shifts[5] = (3, 3, 3, 3)
    offs, totals = _layout(sizes, shifts)
    flats = [np.full(tot, CANARY, dtype=np.float32) for tot in totals]
    want, segs = [np.full(tot, CANARY, dtype=np.float32) for tot in totals], []
    for k, n in enumerate(sizes):
        lr, wd = 1e-3 * (k + 1), (5e-4 if k % 2 else 0.0)
        state = O.state(n, t, 100 + k, KINDS[k % 3])
        c = O.constants(lr, 0.9, 0.999, 1e-8, t, wd)
        new = O.adam_f32(*state, c) + (state[3],)
        for s in range(4):
            flats[s][offs[k][s]:offs[k][s] + n] = state[s]
            want[s][offs[k][s]:offs[k][s] + n] = new[s]
        segs.append((offs[k], n, lr, wd))
    return flats, want, segs


def _check_adam(dev, want):
    torch.cuda.synchronize()
    for name, d, w in zip("pmvg", dev, want):
        got = d.cpu().numpy()
        bad = np.flatnonzero(_bits(got) != _bits(w))
        assert bad.size == 0, "%s: %d floats differ from the restatement (or a canary moved), first at %d: %r != %r" % (
            name, bad.size, bad[0], got[bad[0]], w[bad[0]])


@pytest.mark.parametrize("t", O.T_VALUES)
@pytest.mark.parametrize("nseg", [7, 16])
def test_adam_multi_is_the_float32_restatement_bit_for_bit(nseg, t):
    from video_distillation_amd import hip
    sizes = (SIZES * 3)[:nseg]
    flats, want, segs = _adam_case(sizes, t)
    dev = [torch.from_numpy(f).cuda() for f in flats]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    b = hip.VdfAdamBatch()
    b.nseg = nseg
    b.beta1, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.eps = 0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-8
    b.bc2_sqrt = (1.0 - 0.999 ** t) ** 0.5
    for k, (off, n, lr, wd) in enumerate(segs):
        s = b.seg[k]
        s.p, s.m, s.v, s.g = (dev[i].data_ptr() + 4 * off[i] for i in range(4))
        s.n, s.step_size, s.lr_wd = n, lr / (1.0 - 0.9 ** t), lr * wd
    assert hip.lib().vdf_adam_multi(ctypes.addressof(b), hip.stream_ptr("cuda")) == 0
    _check_adam(dev, want)
    assert (dev[0].data_ptr() + 4 * segs[1][0][0]) % 16 == 4


def test_the_wrapper_takes_more_than_sixteen_tensors_in_two_launches():
    from video_distillation_amd import hip
    sizes, t = (SIZES * 3)[:17], 10
    flats, want, segs = _adam_case(sizes, t)
    dev = [torch.from_numpy(f).cuda() for f in flats]
    hip.adam_multi([tuple(dev[i][off[i]:off[i] + n] for i in range(4)) + (lr, wd) for off, n, lr, wd in segs], 0.9, 0.999, 1e-8, t)
    _check_adam(dev, want)


# ---- the regression train step -------------------------------------------------------------------
def _oracle_regress(x, targets, params, mask):
    p64 = [p.double().requires_grad_(True) for p in params]
    m = None if mask is None else mask.double()[:, :, :, None, None]
    logits = R.convnet3d_logits(x.double(), p64, drop_mask=m)
    loss = F.mse_loss(logits, targets.double())
    grads = torch.autograd.grad(loss, p64)
    return float(loss), logits.detach(), [g.detach() for g in grads]


def _rel(a, b):
    return float((a.cpu().double() - b).norm() / b.norm())


@pytest.mark.parametrize("B,K,use_mask", [(5, 7, False), (11, 4, True)])
def test_regress_and_grads_match_fp64_autograd(B, K, use_mask):
    """tests/test_gpu_train.py::test_loss_and_grads_match_fp64_autograd with ``F.mse_loss`` on soft targets for the
    cross-entropy: the same route (the batch against fp64; clip by clip tightly for all but the few clips whose pooling ties
    flip; the batch equal to the sum of the single-clip HIP gradients) and that file's bar for f16x3, 1e-4."""
    from video_distillation_amd import plan, train
    T, H, W, tight = 8, 64, 64, 1e-4
    g = torch.Generator().manual_seed(B * 100 + K + 1)
    x = R.standardise_batch(torch.randn(B, T, 3, H, W, generator=g))
    targets = F.one_hot(torch.randint(0, K, (B,), generator=g), K).float() - 1.0 / K + 0.05 * torch.randn(B, K, generator=g)
    params = R.init_params(950 + K, 3, K)
    te = train.TrainEngine(plan.NetGeometry(T, H, W), K, (2, 1, 1), "cuda:0", prec="f16x3", prec_bwd="f16x3")
    mask = (torch.rand(B, te.C, te.Tp, generator=g) < 0.5).float() * 2.0 if use_mask else None
    pc = [p.cuda() for p in params]
    loss_ref, logits_ref, grads_ref = _oracle_regress(x, targets, params, mask)
    loss, logits, grads = te.regress_and_grads(x.cuda(), targets.cuda(), pc, None if mask is None else mask.cuda())
    grads = [gr.clone() for gr in grads]
    torch.cuda.synchronize()
    assert loss.dim() == 0 and len(grads) == 8 and [tuple(a.shape) for a in grads] == [tuple(p.shape) for p in params]
    print("loss %.7f (fp64 %.7f)" % (float(loss), loss_ref))
    assert abs(float(loss) - loss_ref) / abs(loss_ref) < 1e-4
    np.testing.assert_allclose(logits.cpu().double().numpy(), logits_ref.numpy(), rtol=1e-3, atol=1e-4)
    errs = [_rel(got, ref) for got, ref in zip(grads, grads_ref)]
    print(B, K, "batch grad rel-l2 vs fp64:", " ".join("%.1e" % e for e in errs))
    assert max(errs) < 3e-2, errs
    acc, n_tight = [torch.zeros_like(gr) for gr in grads], 0
    for b in range(B):
        mb = None if mask is None else mask[b:b + 1]
        _, _, g1 = te.regress_and_grads(x[b:b + 1].cuda(), targets[b:b + 1].cuda(), pc, None if mb is None else mb.cuda())
        _, _, r1 = _oracle_regress(x[b:b + 1], targets[b:b + 1], params, mb)
        e1 = max(_rel(a_, r_) for a_, r_ in zip(g1, r1))
        n_tight += e1 < tight
        assert e1 < 5e-2, (b, e1)
        for a_, g_ in zip(acc, g1):
            a_ += g_ / B          # (a single clip's MSE divides by K, the batch's by B K)
    print("   clips matching fp64 within %.0e: %d of %d" % (tight, n_tight, B))
    assert n_tight >= B - max(2, B // 4)
    lin = [float((a_ - g_).norm() / g_.norm()) for a_, g_ in zip(acc, grads)]
    assert max(lin) < 2e-5, lin


def _net(seed, C):
    from video_distillation_amd import networks
    torch.manual_seed(seed)
    return networks.ConvNet3D(3, C, 128, 3, 'relu', 'none', 'maxpooling', 8, (64, 64)).cuda()


@pytest.mark.parametrize("decay", [False, True])
def test_hip_regress_step_three_steps_are_the_restatement_and_the_state_is_torchs(decay):
    from video_distillation_amd import networks
    C, B = 4, 6
    net = _net(11, C).train()
    make = (lambda ps: torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=5e-4)) if decay else \
        (lambda ps: torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999)))
    opt = make(net.parameters())
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=500)
    assert net.hip_regress_trainable(torch.zeros(1, 8, 3, 64, 64, device="cuda"), opt, torch.nn.MSELoss())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 8, 3, 64, 64, generator=g).cuda()
    y = (F.one_hot(torch.arange(B) % C, C).float() - 1.0 / C).cuda()
    te = net._train_engine(x)
    seen, orig = [], te.regress_and_grads

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append([t.detach().cpu().numpy().copy() for t in out[2]])
        return out
    te.regress_and_grads = spy
    try:
        params = list(net.parameters())
        m = [np.zeros(p.numel(), np.float32) for p in params]
        v = [np.zeros(p.numel(), np.float32) for p in params]
        for t in (1, 2, 3):
            before = [p.detach().cpu().numpy().ravel().copy() for p in params]
            versions = [p._version for p in params]
            lr = opt.param_groups[0]["lr"]          # read at the call: the scheduler drives it
            logits, loss = net.hip_regress_step(x, y, opt)
            sched.step()
            torch.cuda.synchronize()
            assert tuple(logits.shape) == (B, C) and math.isfinite(float(loss)) and len(seen) == t
            c = O.constants(lr, 0.9, 0.999, 1e-8, t, 5e-4 if decay else 0.0)
            for k, p in enumerate(params):
                wp, m[k], v[k] = O.adam_f32(before[k], m[k], v[k], seen[-1][k].ravel(), c)
                st = opt.state[p]
                for name, got, want in (("p", p, wp), ("exp_avg", st["exp_avg"], m[k]), ("exp_avg_sq", st["exp_avg_sq"], v[k])):
                    assert np.array_equal(_bits(got.detach().cpu().numpy().ravel()), _bits(want)), (t, k, name)
                assert float(st["step"]) == t and p._version > versions[k]
        assert opt.param_groups[0]["lr"] != lr
    finally:
        te.regress_and_grads = orig
    # torch's keys, dtypes and shapes: against one step of torch's own code on a host parameter
    ref_p = torch.nn.Parameter(torch.zeros(3, 2))
    ref = make([ref_p])
    ref_p.grad = torch.ones(3, 2)
    ref.step()
    for p in params:
        st = opt.state[p]
        assert set(st) == set(ref.state[ref_p]) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == ref.state[ref_p]["step"].dtype and st["step"].shape == ref.state[ref_p]["step"].shape
        assert st["step"].device.type == ref.state[ref_p]["step"].device.type == "cpu"
        for key in ("exp_avg", "exp_avg_sq"):
            assert st[key].dtype == p.dtype and st[key].shape == p.shape and st[key].device == p.device
    # a plain optimizer.step() with torch's own code continues from that state
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    assert all(float(opt.state[p]["step"]) == 4 for p in params)
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))          # and a state_dict round trip
    assert all(float(opt.state[p]["step"]) == 4 for p in params)


def test_hip_regress_trainable_is_false_for_what_the_step_does_not_restate():
    net = _net(12, 3)
    x, ps, mse = torch.zeros(1, 8, 3, 64, 64, device="cuda"), list(net.parameters()), torch.nn.MSELoss()
    assert net.hip_regress_trainable(x, torch.optim.Adam(ps), mse) and net.hip_regress_trainable(x, torch.optim.AdamW(ps), mse)
    assert not net.hip_regress_trainable(x, torch.optim.SGD(ps, lr=0.1), mse)
    assert not net.hip_regress_trainable(x, torch.optim.Adam(ps, amsgrad=True), mse)
    assert not net.hip_regress_trainable(x, torch.optim.Adam([{"params": ps[:6]}, {"params": ps[6:]}]), mse)
    assert not net.hip_regress_trainable(x, torch.optim.Adam(ps), torch.nn.MSELoss(reduction='sum'))
    assert not net.hip_regress_trainable(x, torch.optim.Adam(ps), torch.nn.CrossEntropyLoss())
    assert not net.hip_regress_trainable(x, torch.optim.Adam(ps, maximize=True), mse)
    assert not net.hip_regress_trainable(x, torch.optim.Adam(ps, weight_decay=1e-2), mse)          # coupled L2 decay
    assert not net.hip_regress_trainable(x.cpu(), torch.optim.Adam(ps), mse)
    assert not net.hip_trainable(x, torch.optim.Adam(ps), mse)          # and the cross-entropy step stays what it was


# ---- exact features --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
def test_embed_exact_meets_the_f16x3_bar_and_leaves_the_dither_memory_alone(n):
    net = _net(20 + n, 5).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 8, 3, 64, 64, generator=g)
    want = R.convnet3d_embed(x.double(), [p.detach().cpu().double() for p in list(net.parameters())[:6]])
    assert not hasattr(net, "_real_dithered_key")
    got = net.embed_exact(x.cuda())
    assert not hasattr(net, "_real_dithered_key") and not got.requires_grad
    rl2 = float((got.double().cpu() - want).norm() / want.norm())
    rmax = float((got.double().cpu() - want).abs().max() / want.abs().max())
    print("embed_exact, %d clips: rel-l2 %.3e rel-max %.3e" % (n, rl2, rmax))
    assert rl2 < 3e-5 and rmax < 4 * 3e-5          # tests/test_gpu_embed.py's f16x3 bar
    with torch.no_grad():
        net.embed(torch.randn(8, 8, 3, 64, 64, generator=g).cuda())          # a dithered batch: remembered
    key = net._real_dithered_key
    assert key is not None
    again = net.embed_exact(x.cuda())
    assert net._real_dithered_key == key and torch.equal(again, got)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.embed_exact(x)


def test_nfr_exact_is_nfr_pred_on_exact_features_and_the_default_is_unchanged():
    from video_distillation_amd import networks, nfr, plan
    n, m, C, reg = 3, 8, 3, 1e-6
    g = torch.Generator().manual_seed(41)
    net = _net(41, C)
    x_syn, x_tar = torch.randn(n, 8, 3, 64, 64, generator=g).cuda(), torch.randn(m, 8, 3, 64, 64, generator=g).cuda()
    y_syn = ((F.one_hot(torch.arange(n) % C, C).float() - 1.0 / C)).cuda()
    for mode in ("auto", False):
        net.real_dither = mode
        pred = nfr.nfr(net, x_syn.clone().requires_grad_(True), y_syn, x_tar, reg, exact=True)
        assert net.real_dither is mode or net.real_dither == mode
    net.real_dither = "auto"
    # by hand: embed_exact targets, exact-weight hi+lo synthetic features straight from the engine
    prec = networks.get_precision()
    eng = networks.get_engine(plan.NetGeometry(8, 64, 64), prec["syn"], x_syn.device, prec["bwd"])
    net._sync_engine(eng)
    feat_syn = eng.forward(x_syn)
    feat_tar = net.embed_exact(x_tar)
    want = nfr.nfr_pred(feat_syn, y_syn, feat_tar, reg)
    assert torch.equal(pred.detach(), want) and not net.training and not any(p.requires_grad for p in net.parameters())
    xs = x_syn.clone().requires_grad_(True)
    nfr.nfr(net, xs, y_syn, x_tar, reg, exact=True).square().sum().backward()
    assert xs.grad is not None and bool(torch.isfinite(xs.grad).all()) and float(xs.grad.abs().max()) > 0
    # the default path: without the keyword and with exact=False, the same bits -- and not those of the exact path
    a = nfr.nfr(net, x_syn.clone().requires_grad_(True), y_syn, x_tar, reg)
    b = nfr.nfr(net, x_syn.clone().requires_grad_(True), y_syn, x_tar, reg, exact=False)
    with torch.no_grad():
        f_t = net.embed(x_tar)
    c = nfr.nfr_pred(net.embed(x_syn.clone().requires_grad_(True)), y_syn, f_t, reg)
    assert torch.equal(a, b) and torch.equal(a.detach(), c.detach()) and not torch.equal(a.detach(), pred.detach())


# ---- the trainer -------------------------------------------------------------------------------------
C3, PER, M_TAR, POOL = 3, 2, 8, 3


def _make_trainer(memories, learn_label, seed=5):
    from video_distillation_amd import frepo, utils
    g = torch.Generator().manual_seed(seed)
    n = C3 * PER
    y0 = frepo.soft_labels(torch.arange(C3).repeat_interleave(PER), C3, frepo.y_scale(C3))
    if memories == "images":
        syn = frepo.SynData(torch.randn(n, 8, 3, 64, 64, generator=g), y0, learn_label).cuda()
    else:
        torch.manual_seed(seed)
        hals = torch.nn.ModuleList([utils.Conv3DNet() for _ in range(2)])
        syn = frepo.S2DSynData(torch.randn(n, 3, 64, 64, generator=g), torch.randn(C3, PER, 8, 1, 64, 64, generator=g), hals, y0,
                               learn_label).cuda()
    count = [0]

    def get_model():
        count[0] += 1
        return _net(1000 + count[0], C3)
    opt, sch = frepo.syn_optimizer(syn, 1e2, 1e-3, 100)          # the reference's learning rates
    pools = frepo.build_pool(get_model, 1e-3, 100, POOL, "cuda")
    return frepo.FRePoTrainer(syn, pools, opt, sch), g


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


@pytest.mark.parametrize("learn_label", [False, True])
@pytest.mark.parametrize("memories", ["images", "s2d"])
def test_one_trainer_step_is_the_hand_composition_of_the_public_pieces(memories, learn_label):
    from video_distillation_amd import frepo, nfr
    tr, g = _make_trainer(memories, learn_label)
    syn = tr.syndata
    x_t = torch.randn(M_TAR, 8, 3, 64, 64, generator=g).cuda()
    y_t = frepo.soft_labels(torch.arange(M_TAR) % C3, C3).cuda()
    assert [e.step for e in tr.pools] == [0, 33, 66]
    named = dict(syn.named_parameters())
    before = {k: p.detach().clone() for k, p in named.items()}
    nets_before = [copy.deepcopy(e.model.state_dict()) for e in tr.pools]
    lrs = {id(p): grp["lr"] for grp in tr.synopt.param_groups for p in grp["params"]}
    _seed(9)
    loss, ln_loss, lb_loss = tr.step(x_t, y_t)
    torch.cuda.synchronize()
    assert all(t.is_cuda and t.dim() == 0 and not t.requires_grad for t in (loss, ln_loss, lb_loss))
    # the hand composition under the same seeds, on copies of the state before the step
    _seed(9)
    if memories == "s2d":          # (the last composition is no leaf: deepcopy refuses it)
        syn.x_syn = None
    twin = copy.deepcopy(syn)
    with torch.no_grad():
        for k, p in twin.named_parameters():
            p.copy_(before[k])
    x2, y2 = twin()
    idx = int(np.random.randint(low=0, high=POOL))
    assert idx == tr.last_idx
    net2 = _net(0, C3)
    net2.load_state_dict(nets_before[idx])
    pred = nfr.nfr(net2, x2, y2, x_t, 1e-6, exact=True)
    ln2 = torch.nn.MSELoss(reduction='none')(pred, y_t).sum(dim=-1).mean(0)
    lb2 = frepo.lb_margin_th(y2).mean()
    assert torch.equal(ln_loss, ln2.detach()) and torch.equal(lb_loss, lb2.detach()) and torch.equal(loss, (ln2 + lb2).detach())
    # the synthetic parameters: the restatement applied to their autograd gradients (step 1 from zero moments)
    moved = []
    for k, p in named.items():
        if p.grad is None:
            assert torch.equal(p.detach(), before[k]), k
            continue
        moved.append(k)
        c = O.constants(lrs[id(p)], 0.9, 0.999, 1e-8, 1)
        zero = np.zeros(p.numel(), np.float32)
        want, wm, wv = O.adam_f32(before[k].cpu().numpy().ravel(), zero, zero, p.grad.cpu().numpy().ravel(), c)
        st = tr.synopt.state[p]
        assert np.array_equal(_bits(p.detach().cpu().numpy().ravel()), _bits(want)), k
        assert np.array_equal(_bits(st["exp_avg"].cpu().numpy().ravel()), _bits(wm)) and float(st["step"]) == 1, k
        assert np.array_equal(_bits(st["exp_avg_sq"].cpu().numpy().ravel()), _bits(wv)), k
    want_moved = (["x_syn"] if memories == "images" else ["dynamic", "hallucinator.0.encoder.weight", "hallucinator.0.encoder.bias",
                                                            "hallucinator.1.encoder.weight", "hallucinator.1.encoder.bias"])
    if memories == "s2d":          # a hallucinator no clip drew this step has no gradient, as with torch's own step
        want_moved = [k for k in want_moved if "hallucinator" not in k or int(k.split(".")[1]) in set(twin.last_draw)]
        assert torch.equal(syn.static.detach(), before["static"]) and syn.static.grad is None
    assert sorted(moved) == sorted(want_moved + (["y_syn"] if learn_label else []))
    assert torch.equal(syn.y_syn.detach(), before["y_syn"]) != learn_label
    assert tr.synopt.param_groups[0]["lr"] < 1e2 and tr.synopt.param_groups[1]["lr"] < 1e-3          # the cosine schedule was stepped
    # exactly the drawn element's step and weights changed
    assert [e.step for e in tr.pools] == [s + (k == idx) for k, s in enumerate((0, 33, 66))]
    for k, e in enumerate(tr.pools):
        same = all(torch.equal(e.model.state_dict()[name], t) for name, t in nets_before[k].items())
        assert same == (k != idx), k
        assert len(e.optimizer.state) == (8 if k == idx else 0)
    assert tr.pools[idx].model.training


@pytest.mark.parametrize("memories", ["images", "s2d"])
def test_twenty_steps_on_one_target_batch_stay_finite(memories):
    """Only finiteness is asserted: whether ``ln_loss`` falls at the reference's learning rates on noise has not been measured
    (the first and the last value are printed; on one MI355X: 0.678 -> 0.667 for images, 0.724 -> 0.667 for s2d, where 2/3 is
    the loss of predicting zero at C = 3)."""
    from video_distillation_amd import frepo
    tr, g = _make_trainer(memories, True, seed=6)
    x_t = torch.randn(M_TAR, 8, 3, 64, 64, generator=g).cuda()
    y_t = frepo.soft_labels(torch.arange(M_TAR) % C3, C3).cuda()
    _seed(10)
    out = [tr.step(x_t, y_t) for _ in range(20)]
    ln = [float(o[1]) for o in out]
    print("%s: ln_loss first %.6g last %.6g; all: %s" % (memories, ln[0], ln[-1], " ".join("%.4g" % v for v in ln)))
    assert all(math.isfinite(float(t)) for o in out for t in o)


def test_evaluate_synset_trains_the_net_with_adamw_on_soft_labels():
    from video_distillation_amd import frepo, networks
    C = 3
    g = torch.Generator().manual_seed(2)
    clips = torch.randn(6, 8, 3, 64, 64, generator=g)
    y = frepo.soft_labels(torch.arange(C).repeat_interleave(2), C, frepo.y_scale(C))
    test = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(clips[:4], torch.arange(4) % C), batch_size=4)
    net = _net(77, C)
    before = [p.detach().clone() for p in net.parameters()]
    calls, orig = [], networks.ConvNet3D.hip_regress_step

    def spy(self, x, lab, opt):
        calls.append((int(x.shape[0]), type(opt), opt.param_groups[0]["weight_decay"], opt.param_groups[0]["lr"]))
        return orig(self, x, lab, opt)
    networks.ConvNet3D.hip_regress_step = spy
    try:
        args = types.SimpleNamespace(device="cuda", lr_net=1e-3, epoch_eval_train=1, batch_train=6)
        out, acc_train, acc_test = frepo.evaluate_synset(0, net, clips, y, test, args, C)
    finally:
        networks.ConvNet3D.hip_regress_step = orig
    assert out is net and 0.0 <= acc_train <= 1.0 and 0.0 <= acc_test <= 1.0
    assert [c[:3] for c in calls] == [(6, torch.optim.AdamW, 0.0005)] * 2 and calls[0][3] == pytest.approx(1e-5)
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
