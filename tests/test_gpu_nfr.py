"""The kernel ridge predictor of csrc/nfr.hip (include/vd_nfr.h) through the C ABI, through ``nfr.nfr_pred`` and through
``nfr.nfr`` on a ConvNet3D, against the fp64 oracle of tests/nfr_oracle.py.

Cases (n, m, d, C): ``nfr_oracle.CASES`` -- the smallest of everything; sizes that are no multiple of 4 or 16; exactly one
matrix tile and one k step (n > d as well: cond 9.5e6); one past each tile edge and past a 32-wide LDS stage; configuration 1's
feature width; n > d (a rank-deficient K: cond 6.7e6 and 1.4e7 with these seeds); two duplicated rows (cond 6.1e6) at reg 1e-6
and 1e-3 (6.1e3); the workload's n, d and C at a
small m -- and n = VDN_LDS_SYN, VDN_LDS_SYN + 1 at (m, d, C) = (4, 8, 2), reg 1e-2: both sides of the LDS / streamed split.

Bar.  Every comparison of fp64 outputs: rel-L2 <= 16 * cond_2(A) * 2^-53 (``nfr_oracle.bar``, where it is derived), cond_2(A)
computed per case in fp64.  The Python surface returns the fp64 results rounded once: elementwise
|x - ref| <= 2^-23 |ref| + bar * max|ref|.  End to end through the network: the project's 1e-3 rel-L2 (tests/test_gpu_e2e.py)
against the hand composition with the ORACLE's feature gradient on the HIP features."""
import numpy as np
import pytest
import torch

from tests import nfr_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
SPLIT_CASES = [(128, 4, 8, 2, 1e-2, False), (129, 4, 8, 2, 1e-2, False)]


def _guarded(numel):
    """A NaN-filled device buffer of ``numel`` doubles with ``GUARD`` doubles of a sentinel on both sides -> (allocation, view)."""
    whole = torch.full((GUARD + numel + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    whole[:GUARD] = -777.0
    whole[GUARD + numel:] = -777.0
    return whole, whole[GUARD:GUARD + numel]


def _guard_intact(whole, numel):
    return bool((whole[:GUARD] == -777.0).all()) and bool((whole[GUARD + numel:] == -777.0).all())


def _abi(case, fs, ys, ft, R):
    """One forward and one backward call through the C ABI into guarded buffers -> (pred, g_feat_syn, g_y_syn, status) on the host."""
    from video_distillation_amd import hip
    n, m, d, C, reg, _ = case
    lib = hip.lib()
    nbytes = lib.vdn_nfr_workspace_bytes(n, m, d, C)
    assert nbytes >= 8 * (1 + n * n + n * C + m * n)
    ws_whole, ws = _guarded(nbytes // 8)
    dfs, dys, dft, dR = (t.cuda().contiguous() for t in (fs, ys, ft, R))
    p_whole, pred = _guarded(m * C)
    assert lib.vdn_nfr_forward(dfs.data_ptr(), dys.data_ptr(), dft.data_ptr(), n, m, d, C, reg, ws.data_ptr(), pred.data_ptr(),
                               hip.stream_ptr()) == 0
    gf_whole, g_fs = _guarded(n * d)
    gy_whole, g_ys = _guarded(n * C)
    keep = ws.clone()
    assert lib.vdn_nfr_backward(dfs.data_ptr(), dft.data_ptr(), dR.data_ptr(), n, m, d, C, reg, ws.data_ptr(), g_fs.data_ptr(),
                                g_ys.data_ptr(), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _guard_intact(ws_whole, nbytes // 8) and _guard_intact(p_whole, m * C) and _guard_intact(gf_whole, n * d) \
        and _guard_intact(gy_whole, n * C)
    assert torch.equal(ws.view(torch.int64), keep.view(torch.int64))          # backward only reads the workspace
    return (pred.cpu().reshape(m, C), g_fs.cpu().reshape(n, d), g_ys.cpu().reshape(n, C), hip.nfr_status(ws))


@pytest.mark.parametrize("case", O.CASES + SPLIT_CASES, ids=O.case_id)
def test_c_abi_against_the_fp64_oracle_twice_bit_for_bit(case):
    from video_distillation_amd import hip
    assert (hip.VDN_LDS_SYN, hip.VDN_MAX_SYN) == (128, 1024) and SPLIT_CASES[0][0] == hip.VDN_LDS_SYN
    fs, ys, ft, R = O.inputs(case)
    assert float(fs.abs().max()) > 0
    want = O.by_autograd(fs, ys, ft, R, case[4])
    c = O.cond(fs, case[4])
    first = _abi(case, fs, ys, ft, R)
    again = _abi(case, fs, ys, ft, R)
    assert first[3] == 0 and again[3] == 0
    errs = [O.rel_l2(got, ref) for got, ref in zip(first[:3], want)]
    print("%s: cond %.3e, bar %.3e; rel-L2 pred %.3e, g_feat_syn %.3e, g_y_syn %.3e (in units of cond * 2^-53: %s)"
          % (O.case_id(case), c, O.bar(c), errs[0], errs[1], errs[2], ["%.2f" % (e / (c * 2.0 ** -53)) for e in errs]))
    for got in first[:3]:
        assert bool(torch.isfinite(got).all())
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))          # a second run: identical bits
    assert max(errs) <= O.bar(c), errs


def test_all_zero_features_give_a_status_and_nan_never_a_number():
    case = (5, 6, 7, 3, 1e-6, False)
    fs, ys, ft, R = O.inputs(case)
    pred, g_fs, g_ys, status = _abi(case, torch.zeros_like(fs), ys, ft, R)
    assert status == 1
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(g_fs).all()) and bool(torch.isnan(g_ys).all())
    bad = fs.clone()
    bad[2, 3] = float("inf")
    pred, g_fs, g_ys, status = _abi(case, bad, ys, ft, R)
    assert status != 0
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(g_fs).all()) and bool(torch.isnan(g_ys).all())


def _loss(pred, y):
    """The reference's loss line (distill_s2d.py: criterion = MSELoss(reduction='none'))."""
    return torch.nn.MSELoss(reduction='none')(pred, y).sum(-1).mean(0)


def _within_one_rounding(got, ref, b):
    ref = ref.double()
    return bool(((got.double().cpu() - ref).abs() <= 2.0 ** -23 * ref.abs() + b * float(ref.abs().max())).all())


@pytest.mark.parametrize("case", [O.CASES[1], O.CASES[7], O.CASES[10]], ids=O.case_id)
def test_nfr_pred_loss_and_backward_are_the_oracle_rounded_once(case):
    from video_distillation_amd import nfr
    fs, ys, ft, _ = O.inputs(case)
    y_tar = torch.randn(ft.shape[0], ys.shape[1], generator=torch.Generator().manual_seed(7))
    dfs, dys = fs.cuda().requires_grad_(True), ys.cuda().requires_grad_(True)
    pred = nfr.nfr_pred(dfs, dys, ft.cuda(), case[4])
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (case[1], case[3])
    pred.retain_grad()
    _loss(pred, y_tar.cuda()).backward()
    # the oracle takes the upstream gradient the op was handed: what is compared is the op, not the loss line
    want = O.by_autograd(fs, ys, ft, pred.grad.cpu(), case[4])
    b = O.bar(O.cond(fs, case[4]))
    assert _within_one_rounding(pred.detach(), want[0], b)
    assert _within_one_rounding(dfs.grad, want[1], b)
    assert _within_one_rounding(dys.grad, want[2], b)
    with pytest.raises(ValueError):
        nfr.nfr_pred(dfs, dys, ft.cuda().requires_grad_(True), case[4])
    only_labels = nfr.nfr_pred(dfs.detach(), dys, ft.cuda(), case[4])          # a gradient for the labels alone
    assert only_labels.requires_grad and torch.equal(only_labels, pred.detach())


def _net(seed, C):
    from video_distillation_amd import networks
    torch.manual_seed(seed)
    return networks.ConvNet3D(3, C, 128, 3, 'relu', 'none', 'maxpooling', 8, (64, 64)).cuda()


def _oracle_feature_gradient(feat_syn, y_syn, feat_tar, y_tar, reg):
    """d loss / d feat_syn and d loss / d y_syn of the reference's loss line over form (a) in fp64, on the given features."""
    fs = feat_syn.detach().cpu().double().requires_grad_(True)
    ys = y_syn.detach().cpu().double().requires_grad_(True)
    ft = feat_tar.detach().cpu().double()
    kss, kts = fs @ fs.t(), ft @ fs.t()
    n = kss.shape[0]
    pred = kts @ torch.linalg.solve(kss + abs(reg) * torch.trace(kss) * torch.eye(n, dtype=torch.float64) / n, ys)
    return torch.autograd.grad(_loss(pred, y_tar.cpu().double()), (fs, ys))


@pytest.mark.parametrize("memories", ["pixels", "hallucinator"])
def test_nfr_through_the_network_equals_the_hand_composition(memories):
    """64x64x8, 3 synthetic and 4 target clips, C = 3.  ``nfr(net, ...)`` against the same two ``embed`` calls made by hand:
    ``pred`` is ``nfr_pred`` of the net's own features, and the gradient that reaches the pixels (or the dynamic memory and the
    hallucinator) is ``autograd.grad(net.embed(x_syn), leaves, g_feat)`` with the oracle's g_feat on those features.  A missing
    no_grad, a sign or a transposed operand moves either by O(1)."""
    from video_distillation_amd import nfr, utils
    n, m, C, reg = 3, 4, 3, 1e-6
    g = torch.Generator().manual_seed(31)
    net = _net(5, C)
    x_tar = torch.randn(m, 8, 3, 64, 64, generator=g).cuda()
    y_tar = torch.nn.functional.one_hot(torch.arange(m) % C, C).float().cuda()
    y_syn = (torch.nn.functional.one_hot(torch.arange(n) % C, C).float() - 1.0 / C).cuda().requires_grad_(True)
    if memories == "pixels":
        leaves = [torch.randn(n, 8, 3, 64, 64, generator=g).cuda().requires_grad_(True)]
        make = lambda: leaves[0]          # noqa: E731
    else:
        torch.manual_seed(6)
        hal = utils.Conv3DNet(img_size=64).cuda()
        static = torch.randn(n, 3, 64, 64, generator=g).cuda()
        dynamic = torch.randn(n, 8, 1, 64, 64, generator=g).cuda().requires_grad_(True)
        leaves = [dynamic] + list(hal.parameters())
        make = lambda: hal(static, dynamic)          # noqa: E731
    pred = nfr.nfr(net, make(), y_syn, x_tar, reg)
    _loss(pred, y_tar).backward()
    got = [t.grad.clone() for t in leaves]
    got_y = y_syn.grad.clone()
    assert all(not p.requires_grad for p in net.parameters()) and not net.training
    # by hand: the same two embed calls in the same order
    with torch.no_grad():
        feat_tar = net.embed(x_tar)
    feat_syn = net.embed(make())
    assert not feat_tar.requires_grad and feat_syn.requires_grad
    assert torch.equal(pred.detach(), nfr.nfr_pred(feat_syn.detach(), y_syn.detach(), feat_tar, reg))
    g_feat, g_y = _oracle_feature_gradient(feat_syn, y_syn, feat_tar, y_tar, reg)
    want = torch.autograd.grad(feat_syn, leaves, g_feat.float().cuda())
    for a, b in zip(got, want):
        err = O.rel_l2(a.cpu(), b.cpu())
        print("%s: gradient of shape %s, rel-L2 to the hand composition %.3e" % (memories, tuple(a.shape), err))
        assert float(b.abs().max()) > 0 and err <= 1e-3
    assert O.rel_l2(got_y.cpu(), g_y) <= 1e-3


def test_use_flip_doubles_the_synthetic_set_by_its_mirror():
    from video_distillation_amd import nfr
    n, m, C, reg = 3, 4, 3, 1e-6
    g = torch.Generator().manual_seed(32)
    net = _net(7, C)
    x_syn = torch.randn(n, 8, 3, 64, 64, generator=g).cuda()
    x_tar = torch.randn(m, 8, 3, 64, 64, generator=g).cuda()
    y_syn = torch.randn(n, C, generator=g).cuda()
    pred = nfr.nfr(net, x_syn, y_syn, x_tar, reg, use_flip=True)
    with torch.no_grad():
        feat_tar = net.embed(x_tar)
        feat_syn = net.embed(torch.cat((x_syn, torch.flip(x_syn, dims=[-1])), 0))
    assert tuple(feat_syn.shape) == (2 * n, 256)
    assert torch.equal(pred, nfr.nfr_pred(feat_syn, torch.cat((y_syn, y_syn), 0), feat_tar, reg))
    assert not torch.equal(pred, nfr.nfr(net, x_syn, y_syn, x_tar, reg))
