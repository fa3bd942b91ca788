"""Multi-static batches composed on the device: ``vd_hallucinator_fwd_multi`` through the C ABI against the fp64 ``conv3d`` of its
contract and, bit for bit, against ``vd_hallucinator_fwd`` called once per item; ``utils.MultiStaticBatches`` against the host
``DataLoader`` over ``MultiStaticSharedDataset`` under equal seeds (every batch ``torch.equal``, generators left in the same
state); which of the two ``evaluate_synset(mode='multi-static')`` picks; and ``run_s2d`` end to end with evaluation on."""
import os
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.aux_oracle import gamma

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _poison(shape):
    """Leave a NaN-filled block of the output's size in the caching allocator, so that an element the kernel does not write
    cannot look right by accident."""
    t = torch.full(tuple(shape), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del t


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.fixture
def poisoned_batches(monkeypatch):
    """Poison the allocator before EVERY ``hip.hallucinate_multi`` call (the loader's batches, whoever iterates it): the NaN
    block has the size of the batch about to be composed, and the output is the binding's first device allocation, so it is
    the block the caching allocator hands back -- not the previous batch's, which holds valid clips.  -> the list of the batch
    sizes seen."""
    from video_distillation_amd import hip
    orig, seen = hip.hallucinate_multi, []

    def multi(static, dynamic, sidx, *a, **k):
        seen.append(len(sidx))
        _poison((len(sidx), dynamic.shape[1], 3, dynamic.shape[3], dynamic.shape[4]))
        return orig(static, dynamic, sidx, *a, **k)
    monkeypatch.setattr(hip, "hallucinate_multi", multi)
    return seen


# ------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------
def _multi(stat, dyn, sidx, didx, hidx, w, b, n):
    from video_distillation_amd import hip
    T, H, W = dyn.shape[1], dyn.shape[3], dyn.shape[4]
    _poison((n, T, 3, H, W))
    out = torch.empty((n, T, 3, H, W), dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vd_hallucinator_fwd_multi(hip.ptr(stat), hip.ptr(dyn), hip.ptr(sidx), hip.ptr(didx), hip.ptr(hidx), hip.ptr(w),
                                                  hip.ptr(b), int(w.shape[0]), n, T, H, W, hip.ptr(out), hip.stream_ptr(out.device)),
              "vd_hallucinator_fwd_multi")
    torch.cuda.synchronize()
    return out


def _single(stat, dyn, s, d, w, b):
    """vd_hallucinator_fwd for one item with its own set."""
    from video_distillation_amd import hip
    T, H, W = dyn.shape[1], dyn.shape[3], dyn.shape[4]
    _poison((1, T, 3, H, W))
    out = torch.empty((1, T, 3, H, W), dtype=torch.float32, device=DEV)
    hip.check(hip.lib().vd_hallucinator_fwd(hip.ptr(stat[s]), hip.ptr(dyn[d]), None, None, hip.ptr(w), hip.ptr(b), 1, T, H, W,
                                            hip.ptr(out), hip.stream_ptr(out.device)), "vd_hallucinator_fwd")
    return out[0]


def _check_kernel(seed, n, T, H, W, nh, ns, nd, sidx, didx, hidx):
    g = torch.Generator().manual_seed(seed)
    stat, dyn = torch.randn(ns, 3, H, W, generator=g), torch.randn(nd, T, 1, H, W, generator=g)
    w, b = torch.randn(nh, 3, 4, 3, 3, 3, generator=g) * 0.3, torch.randn(nh, 3, generator=g)
    si = list(range(n)) if sidx is None else sidx
    di = list(range(n)) if didx is None else didx
    hi = [0] * n if hidx is None else hidx
    dev = [t.to(DEV) for t in (stat, dyn, w, b)]
    tables = [None if t is None else torch.tensor(t, dtype=dt, device=DEV)
              for t, dt in ((sidx, torch.int64), (didx, torch.int64), (hidx, torch.int32))]
    got = _multi(dev[0], dev[1], tables[0], tables[1], tables[2], dev[2], dev[3], n)
    assert got.shape == (n, T, 3, H, W)
    # (a) the contract in fp64 on the host: conv3d(cat(static over T, dynamic), w[h], b[h]); every output is a sum of at most 108
    #     products and a bias, 109 roundings in any order -> |got - ref| <= gamma(112) (sum |w||x| + |b|)
    for i in range(n):
        vol = torch.cat([stat[si[i]].unsqueeze(1).expand(3, T, H, W), dyn[di[i]].transpose(0, 1)], 0).double()[None]
        ref = F.conv3d(vol, w[hi[i]].double(), b[hi[i]].double(), padding=1)[0].transpose(0, 1)
        mag = F.conv3d(vol.abs(), w[hi[i]].double().abs(), b[hi[i]].double().abs(), padding=1)[0].transpose(0, 1)
        err = (got[i].cpu().double() - ref).abs()
        assert bool((err <= gamma(112) * mag).all()), "clip %d: worst error / bound %.3g" % (i, float((err / (gamma(112) * mag)).max()))
    # (b) bit for bit what the single-set entry gives for each item alone
    for i in range(n):
        one = _single(dev[0], dev[1], si[i], di[i], dev[2][hi[i]], dev[3][hi[i]])
        torch.cuda.synchronize()
        assert np.array_equal(_u32(got[i]), _u32(one)), "clip %d differs from vd_hallucinator_fwd" % i


def test_multi_sets_and_repeated_gathers_in_less_than_one_wave():
    _check_kernel(1, n=5, T=3, H=6, W=10, nh=3, ns=4, nd=3, sidx=[1, 1, 3, 0, 1], didx=[2, 0, 2, 2, 1], hidx=[2, 0, 1, 2, 0])


@pytest.mark.parametrize("T", [1, 2])
def test_clips_without_a_temporal_neighbour(T):
    _check_kernel(10 + T, n=3, T=T, H=6, W=10, nh=2, ns=3, nd=4, sidx=[2, 0, 1], didx=[3, 3, 0], hidx=[1, 0, 1])


def test_two_blocks_per_clip_the_second_partial():
    _check_kernel(3, n=3, T=3, H=15, W=20, nh=2, ns=2, nd=3, sidx=[1, 0, 1], didx=[0, 2, 1], hidx=[0, 1, 1])


def test_null_tables_mean_identity_and_set_zero():
    _check_kernel(4, n=6, T=8, H=64, W=64, nh=2, ns=6, nd=6, sidx=None, didx=None, hidx=None)


def test_argument_errors_are_reported_before_any_launch():
    from video_distillation_amd import hip
    L = hip.lib()
    f = torch.zeros(648, device=DEV)
    p, st = hip.ptr(f), hip.stream_ptr(f.device)
    assert L.vd_hallucinator_fwd_multi(p, p, None, None, None, p, p, 0, 1, 1, 2, 2, p, st) == -1
    assert L.vd_hallucinator_fwd_multi(p, p, None, None, None, p, p, -3, 1, 1, 2, 2, p, st) == -1
    for hole in range(5):          # stat, dyn, w, b, out
        a = [p, p, None, None, None, p, p, 1, 1, 1, 2, 2, p, st]
        a[(0, 1, 5, 6, 12)[hole]] = None
        assert L.vd_hallucinator_fwd_multi(*a) == -1
    assert L.vd_hallucinator_fwd_multi(p, p, None, None, None, p, p, 1, 65536, 1, 2, 2, p, st) == -2
    assert L.vd_hallucinator_fwd_multi(p, p, None, None, None, p, p, 1, 0, 1, 2, 2, p, st) == 0
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------------------------------
def _memories(n_c, per_s, dpc, T=2, H=6, W=10, seed=7):
    from video_distillation_amd import utils
    g = torch.Generator().manual_seed(seed)
    static = torch.randn(n_c * per_s, 3, H, W, generator=g).to(DEV)
    dynamic = torch.randn(n_c, dpc, T, 1, H, W, generator=g).to(DEV)
    torch.manual_seed(seed)
    hals = [utils.Conv3DNet().to(DEV), utils.Conv3DNet(mode='add').to(DEV)]
    return static, dynamic, hals


def _seed():
    np.random.seed(5); random.seed(7); torch.manual_seed(3)


def _states():
    return (random.getstate(), torch.get_rng_state().tolist())


def _two_epochs(loader):
    out = []
    for _ in range(2):
        for clips, labels in loader:
            out.append((clips.detach().clone(), labels.cpu().clone()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_c,per_s,dpc,own_generator", [(3, 2, 2, False), (2, 10, 10, False), (2, 10, 10, True)])
def test_batches_equal_the_host_loader_and_leave_the_generators_alike(n_c, per_s, dpc, own_generator, poisoned_batches):
    from video_distillation_amd import utils
    static, dynamic, hals = _memories(n_c, per_s, dpc)
    n = n_c if per_s == 2 else n_c * 5
    gens = [torch.Generator().manual_seed(21) if own_generator else None for _ in range(2)]
    _seed()
    host = _two_epochs(torch.utils.data.DataLoader(utils.MultiStaticSharedDataset(static, dynamic, hals), batch_size=4, shuffle=True,
                                                   num_workers=0, generator=gens[0]))
    after_host = _states()
    _seed()
    loader = utils.MultiStaticBatches(static, dynamic, hals, 4, shuffle=True, generator=gens[1])
    assert len(loader) == (n + 3) // 4
    mine = _two_epochs(loader)
    assert poisoned_batches == [c.shape[0] for c, _ in mine]          # (every batch was composed over a NaN block)
    assert _states() == after_host
    if own_generator:
        assert gens[0].get_state().tolist() == gens[1].get_state().tolist()
    assert [c.shape[0] for c, _ in mine] == ([4] * (n // 4) + ([n % 4] if n % 4 else [])) * 2          # the last batch is short
    assert len(mine) == len(host)
    for (c0, l0), (c1, l1) in zip(host, mine):
        assert c1.dtype == torch.float32 and c1.is_cuda and l1.dtype == torch.int64 and not c1.requires_grad
        assert torch.equal(l0, l1) and np.array_equal(_u32(c0), _u32(c1))
    assert sorted(torch.cat([l for _, l in mine[:len(mine) // 2]]).tolist()) == sorted(list(range(n_c)) * (n // n_c))
    if per_s == 10:          # (the two epochs were shuffled apart)
        assert not torch.equal(torch.cat([l for _, l in mine[:3]]), torch.cat([l for _, l in mine[3:]]))


def test_labels_arrive_on_the_device(poisoned_batches):
    from video_distillation_amd import utils
    static, dynamic, hals = _memories(3, 2, 2)
    _seed()
    clips, labels = next(iter(utils.MultiStaticBatches(static, dynamic, hals, 4)))
    assert labels.is_cuda and labels.dtype == torch.int64 and sorted(labels.tolist()) == [0, 1, 2] and clips.shape == (3, 2, 3, 6, 10)


# ------------------------------------------------------------------------------------------------------------------------
# which loader evaluate_synset takes
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the launches of the two bindings: hip.hallucinate_multi and the library's single-set vd_hallucinator_fwd."""

    def __init__(self, monkeypatch):
        from video_distillation_amd import hip
        self.multi, self.single = [], 0
        L = hip.lib()
        orig_multi, orig_single = hip.hallucinate_multi, L.vd_hallucinator_fwd

        def multi(*a, **k):
            self.multi.append(len(a[2]))
            return orig_multi(*a, **k)

        def single(*a):
            self.single += 1
            return orig_single(*a)
        monkeypatch.setattr(hip, "hallucinate_multi", multi)
        monkeypatch.setattr(L, "vd_hallucinator_fwd", single)


def _convnet(seed, num_classes):
    from video_distillation_amd import networks
    torch.manual_seed(seed)
    return networks.ConvNet3D(channel=3, num_classes=num_classes, net_width=128, net_depth=3, net_act='relu', net_norm='none',
                              net_pooling='maxpooling', im_size=(64, 64), frames=8)


def test_g11_runs_on_the_device_loader_and_keeps_its_losses(golden_dir, monkeypatch, poisoned_batches):
    from video_distillation_amd import utils
    z = np.load(os.path.join(golden_dir, "g11_multi_static_eval.npz"))
    C, n_test, epochs = int(z["C"]), int(z["n_test"]), int(z["epochs"])
    g = torch.Generator().manual_seed(int(z["data_seed"]))
    static = torch.randn(C * 2, 3, 64, 64, generator=g)
    dynamic = torch.randn(C, 2, 8, 1, 64, 64, generator=g)
    test_x = torch.randn(n_test, 8, 3, 64, 64, generator=g)
    hals = []
    for k in range(2):
        h = utils.Conv3DNet(img_size=64)
        h.load_state_dict({"encoder.weight": torch.tensor(z["hal_w"][k]), "encoder.bias": torch.tensor(z["hal_b"][k])})
        hals.append(h.cuda())
    net = _convnet(int(z["net_seed"]), C)
    net.dropout.p = 0.0
    args = types.SimpleNamespace(device="cuda", lr_net=float(z["lr_net"]), epoch_eval_train=epochs, batch_train=256,
                                 model="ConvNet3D", eval_mode="SS")
    testloader = torch.utils.data.DataLoader(utils.TensorDataset(test_x, torch.arange(n_test) % C), batch_size=4)
    losses, orig_epoch = [], utils.epoch

    def record(mode, *a):
        out = orig_epoch(mode, *a)
        if mode == 'train':
            losses.append(out[0])
        return out
    monkeypatch.setattr(utils, "epoch", record)
    spy = _Spy(monkeypatch)
    torch.manual_seed(int(z["rng_seed"])); random.seed(int(z["rng_seed"]))
    utils.evaluate_synset(0, net, (static.cuda(), dynamic.cuda(), hals), None, testloader, args, mode='multi-static')
    per_epoch = (C + 255) // 256
    assert spy.single == 0 and spy.multi == [min(256, C - 256 * k) for k in range(per_epoch)] * (epochs + 1)
    print("multi-static train losses on the device loader", losses, "golden", z["train_loss"])
    np.testing.assert_allclose(losses, z["train_loss"], rtol=1e-3)


def test_a_plain_callable_among_the_hallucinators_takes_the_host_loader(monkeypatch, poisoned_batches):
    from video_distillation_amd import utils
    C = 3
    g = torch.Generator().manual_seed(2)
    static, dynamic = torch.randn(C * 2, 3, 64, 64, generator=g).cuda(), torch.randn(C, 2, 8, 1, 64, 64, generator=g).cuda()
    test_x = torch.randn(C, 8, 3, 64, 64, generator=g)
    torch.manual_seed(4)
    hal = utils.Conv3DNet().cuda()
    hals = [hal, lambda s, d: hal(s, d)]
    assert not utils.MultiStaticBatches.device_composable(static, dynamic, hals)
    assert utils.MultiStaticBatches.device_composable(static, dynamic, [hal])
    assert not utils.MultiStaticBatches.device_composable(static.cpu(), dynamic.cpu(), [hal])
    assert isinstance(utils.multi_static_loader(static, dynamic, hals, 2), torch.utils.data.DataLoader)
    args = types.SimpleNamespace(device="cuda", lr_net=0.01, epoch_eval_train=0, batch_train=2, model="ConvNet3D", eval_mode="SS")
    testloader = torch.utils.data.DataLoader(utils.TensorDataset(test_x, torch.arange(C)), batch_size=4)
    spy = _Spy(monkeypatch)
    random.seed(1); torch.manual_seed(1)
    utils.evaluate_synset(0, _convnet(5, C), (static, dynamic, hals), None, testloader, args, mode='multi-static')
    assert spy.multi == [] and poisoned_batches == [] and spy.single == C          # one epoch, one single-clip launch per item


# ------------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------------
def test_run_s2d_with_evaluation_on(tmp_path, poisoned_batches):
    from video_distillation_amd import distill, plan, run_s2d, utils
    C, per, T, HW, seed = 3, 5, 8, 64, 13
    g = torch.Generator().manual_seed(6)
    clips, labels = torch.randn(C * per, T, 3, HW, HW, generator=g), torch.arange(C).repeat_interleave(per)
    test_clips, test_labels = torch.randn(30, T, 3, HW, HW, generator=g), torch.arange(30) % C
    torch.save({"clips": clips, "labels": labels, "test_clips": test_clips, "test_labels": test_labels}, tmp_path / "toy.pt")
    args = run_s2d.build_parser().parse_args(
        ["--method", "DM", "--dataset", "toy", "--data_file", str(tmp_path / "toy.pt"), "--save_path", str(tmp_path / "out"),
         "--im_size", str(HW), "--frames", str(T), "--vpc", "1", "--spc", "2", "--dpc", "2", "--batch_real", "4", "--Iteration", "2",
         "--eval_it", "2", "--num_eval", "1", "--epoch_eval_train", "1", "--no_train_static", "--seed", str(seed),
         "--lr_dynamic=0.01", "--lr_hal=1e-06", "--eval_mode", "SS"])
    log = []
    run_s2d.run(args, log=log)
    torch.cuda.synchronize()
    acc = [r for r in log if "Accuracy/ConvNet3D" in r]
    assert poisoned_batches == [C] * 4          # two evaluations of one network, epoch_eval_train + 1 = 2 epochs of one batch
    assert [r["step"] for r in acc] == [0, 2]
    assert all(0.0 <= r["Accuracy/ConvNet3D"] <= 1.0 and r["Max_Accuracy/ConvNet3D"] >= r["Accuracy/ConvNet3D"] for r in acc)
    loss = {r["step"]: r["Loss"] for r in log if "Loss" in r}
    assert sorted(loss) == [0, 2] and all(np.isfinite(v) for v in loss.values())
    # iteration 0 by hand on the same tensors: the loss is forward only (no atomics)
    static, dynamic, hals = run_s2d.initial_state(args, C)
    be = distill.HipBackend(plan.NetGeometry(T, HW, HW), DEV, prec_real=args.prec_real, prec_syn=args.prec_syn)
    pool = distill.RealPool(clips.to(DEV), [per] * C, [per * c for c in range(C)])
    tr = distill.S2DTrainer(be, pool, C, 1, 2, 2, 4, static.to(DEV), dynamic.to(DEV), hals[0].encoder.weight.detach().to(DEV),
                            hals[0].encoder.bias.detach().to(DEV), lr_dynamic=0.01, lr_hal=1e-6, lr_static=100.0, train_static=False)
    want = float(tr.step(0)) / C
    tr.sync()
    print("run_s2d Loss at iteration 0: %.9g, S2DTrainer.step(0) by hand: %.9g" % (loss[0], want))
    assert abs(loss[0] / want - 1) < 1e-6
    d = os.path.join(str(tmp_path / "out"), "S2D_multis_DM", "toy_ipc1_0.01_1e-06")
    files = sorted(os.listdir(d))
    assert "dynamic_best.pt" in files and "weights_best.pt" in files and "dynamic_0.pt" in files and "hal_0.pt" in files
    assert not any(f.startswith("images_") for f in files)
    assert tuple(torch.load(os.path.join(d, "dynamic_best.pt")).shape) == (C * 2, T, 1, HW, HW)
