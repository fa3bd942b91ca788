"""Device half of the resident video store: vd_clips_sample against its numpy restatement (tests/resident_oracle.py, bit for
bit), ``ResidentClipLoader`` against the host ``DataLoader`` under equal seeds (every batch ``torch.equal``, generators left in
the same state), the same through ``utils.epoch('test')``, and the two driver flags on the committed JPEG tree."""
import os
import random
import types

import numpy as np
import pytest
import torch

from tests import resident_oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UCF = os.path.join(GOLD, "frames", "UCF101")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _seed():
    np.random.seed(5); random.seed(7); torch.manual_seed(3)


def _states():
    return (np.random.get_state()[1].tolist(), np.random.get_state()[2], random.getstate(), torch.get_rng_state().tolist())


def _store(nframes, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (nframes, h, w, 3), dtype=torch.uint8, generator=g)
    k = min(256, u8.numel())
    u8.view(-1)[:k] = torch.arange(k, dtype=torch.uint8)                     # every byte value
    return u8


def _poison(shape):
    """Leave a NaN-filled block of the output's size in the caching allocator, so that an element the kernel does not write
    cannot look right by accident."""
    t = torch.full(shape, float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    del t


def _check(u8, dev, rows, flip, crops, t, out_hw):
    from video_distillation_amd import dataset as D
    want = O.clips_sample(u8.numpy(), rows, flip, crops, t, out_hw, MEAN, STD)
    _poison(want.shape)
    got = D.sample_clips(dev, rows, flip, crops, t, out_hw, MEAN, STD)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))       # bit-equal


@pytest.mark.parametrize("h,w,nclips,t", [(112, 112, 5, 4), (7, 5, 3, 2), (8, 12, 4, 3)])
def test_clips_sample_is_bit_equal_to_the_oracle_without_crop(h, w, nclips, t):
    u8 = _store(9, h, w, 100 + h)
    rng = np.random.RandomState(h * 7 + w)
    rows = rng.randint(0, 9, size=nclips * t)
    rows[:t] = rows[t:2 * t]                                                 # two clips share all their frames ...
    flip = np.arange(nclips) % 2                                             # ... one mirrored, one not
    _check(u8, u8.to("cuda:0"), rows, flip, None, t, (h, w))
    _check(u8, u8.to("cuda:0"), rows, np.zeros(nclips, dtype=np.uint8), None, t, (h, w))
    _check(u8, u8.to("cuda:0"), rows, np.ones(nclips, dtype=np.uint8), None, t, (h, w))


def test_clips_sample_resize_store_with_crops():
    u8 = _store(6, 100, 80, 31)
    nclips, t = 4, 3
    rng = np.random.RandomState(9)
    rows = rng.randint(0, 6, size=nclips * t)
    crops = np.stack([rng.randint(0, 37, size=nclips * t), rng.randint(0, 17, size=nclips * t)], 1)
    crops[0], crops[1], crops[2], crops[3] = (0, 0), (36, 16), (36, 0), (0, 16)          # the corners of the slack
    _check(u8, u8.to("cuda:0"), rows, np.array([0, 1, 1, 0]), crops, t, (64, 64))
    # a crop of the full stored size is no crop
    _check(u8, u8.to("cuda:0"), rows, np.array([1, 0, 1, 0]), np.zeros((nclips * t, 2), dtype=np.int64), t, (100, 80))


def test_clips_sample_unaligned_store_takes_the_scalar_path():
    base = torch.randint(0, 256, (5 * 8 * 8 * 3 + 1,), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    u8 = base[1:].view(5, 8, 8, 3)
    dev = base.to("cuda:0")[1:].view(5, 8, 8, 3)                             # 1-byte offset: not dword aligned on the device
    assert dev.data_ptr() % 4 != 0
    _check(u8, dev, np.array([4, 0, 2, 2, 1, 3]), np.array([1, 0, 1]), None, 2, (8, 8))


def test_clips_sample_of_no_clips_and_refused_tables():
    from video_distillation_amd import dataset as D
    dev = _store(3, 8, 8, 5).to("cuda:0")
    out = D.sample_clips(dev, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8), None, 4, (8, 8), MEAN, STD)
    assert out.shape == (0, 4, 3, 8, 8)
    with pytest.raises(ValueError):
        D.sample_clips(dev, [0, 3], [0], None, 2, (8, 8), MEAN, STD)         # refused on the host: nothing is launched
    with pytest.raises(ValueError):
        D.sample_clips(dev, [0, 1], [0], [(0, 0), (5, 0)], 2, (4, 4), MEAN, STD)


LOADER_CASES = {
    "ucf_test": (lambda D: D.UCF101(UCF, "test"), False, 3),
    "ucf_train_shuffled": (lambda D: D.UCF101(UCF, "train"), True, 2),
    "mini_seg": (lambda D: D.miniUCF101(UCF, "train", sample="split-random"), True, 2),
    "mini_seg_test": (lambda D: D.miniUCF101(UCF, "test", sample="split-random"), False, 3),
    "ucf_test_64": (lambda D: D.UCF101(UCF, "test", D.FrameTransform((64, 64))), False, 3),
    "ucf_train_64_shuffled": (lambda D: D.UCF101(UCF, "train", D.FrameTransform((64, 64))), True, 2),
}


@pytest.mark.parametrize("case", sorted(LOADER_CASES))
def test_resident_loader_equals_the_host_dataloader(case):
    from video_distillation_amd import dataset as D
    make, shuffle, passes = LOADER_CASES[case]
    ds = make(D)
    _seed()
    ref = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=shuffle, num_workers=0)
    want = [[(x.clone(), y.clone()) for x, y in ref] for _ in range(passes)]
    want_state = _states()
    ds2 = make(D)
    loader = D.resident_loader(ds2, "cuda:0", batch_size=2, shuffle=shuffle, workers=3)
    assert loader.store.frames.shape[0] == sum(loader.store.length) and loader.store.frames.dtype == torch.uint8
    assert loader.store.frames.numel() == loader.store.nbytes and len(loader) == len(ref)
    _seed()
    got = [[(x, y) for x, y in loader] for _ in range(passes)]
    assert _states() == want_state
    assert ds2.start == ds.start
    distinct = set()
    for gp, wp in zip(got, want):
        assert len(gp) == len(wp)
        for (gx, gy), (wx, wy) in zip(gp, wp):
            assert gx.is_cuda and gy.is_cuda and gy.dtype == torch.int64 and gx.dtype == torch.float32
            assert torch.equal(gx.cpu(), wx) and torch.equal(gy.cpu(), wy)
        distinct.add(tuple(float(gx.double().sum()) for gx, _ in gp))
    assert len(distinct) > 1                                                 # the passes differ: nothing was frozen


def test_store_over_a_subset_of_the_items():
    from video_distillation_amd import dataset as D
    ds = D.UCF101(UCF, "train")
    _seed()
    want = [ds[i][0] for i in (2, 0)]
    ds2 = D.UCF101(UCF, "train")
    store = D.ResidentVideos.from_dataset(ds2, "cuda:0", indices=[2, 0], workers=2)
    assert len(store) == 2 and store.labels.tolist() == [ds.labels[2], ds.labels[0]]
    _seed()
    x, y = store.batch([store.draw(2), store.draw(0)])
    assert torch.equal(x.cpu(), torch.stack(want)) and y.tolist() == [ds.labels[2], ds.labels[0]]


def _net(num_classes, size=112, frames=16):
    from video_distillation_amd import networks
    torch.manual_seed(11)
    return networks.ConvNet3D(3, num_classes, 128, 3, 'relu', 'none', 'maxpooling', frames, (size, size)).to("cuda:0")


def test_epoch_test_gives_the_same_result_on_either_loader():
    from video_distillation_amd import dataset as D, utils
    args = types.SimpleNamespace(device="cuda:0", model="ConvNet3D", eval_mode="SS")
    crit = torch.nn.CrossEntropyLoss()
    net = _net(2)
    ds = D.UCF101(UCF, "test")
    _seed()
    with torch.no_grad():
        loss_h, acc_h, per_h = utils.epoch('test', torch.utils.data.DataLoader(ds, batch_size=2), net, None, crit, args)
    loader = D.resident_loader(D.UCF101(UCF, "test"), "cuda:0", batch_size=2)
    _seed()
    with torch.no_grad():
        loss_r, acc_r, per_r = utils.epoch('test', loader, net, None, crit, args)
    print("epoch('test'): host loss %.9g acc %.4f, resident loss %.9g acc %.4f" % (loss_h, acc_h, loss_r, acc_r))
    assert acc_r == acc_h and per_r == per_h
    assert abs(loss_r - loss_h) <= 1e-3 * abs(loss_h)                        # (bit-equal inputs; the eval parity band on the loss)


def test_run_dm_test_videos_resident_feeds_evaluate_synset():
    from video_distillation_amd import dataset as D, hip, plan, run_dm, utils
    root = os.path.join(GOLD, "frames")
    prev = hip.set_deterministic(True)               # (the one training epoch in front of the test pass: the same net both times)
    try:
        res = _evaluate_on_both_loaders(D, plan, run_dm, utils, root)
    finally:
        hip.set_deterministic(prev)
    print("evaluate_synset test pass: host acc %.4f loss %.9g, resident acc %.4f loss %.9g" % (res["host"][0], res["host"][1],
                                                                                               res["resident"][0], res["resident"][1]))
    assert res["resident"][0] == res["host"][0]
    assert abs(res["resident"][1] - res["host"][1]) <= 1e-3 * abs(res["host"][1])
    assert res["resident"][2] == res["host"][2]


def _evaluate_on_both_loaders(D, plan, run_dm, utils, root):
    common = ["--dataset", "miniUCF101", "--data_path", root, "--num_workers", "2"]
    geo = plan.NetGeometry(16, 112, 112)
    res = {}
    for mode in ("host", "resident"):
        args = run_dm.build_parser().parse_args(common + ["--test_videos", mode])
        _seed()
        pool, num_classes, _, testloader = run_dm.load_data(args, 0, 1, geo, torch.device("cuda:0"))
        assert num_classes == 50 and pool.clips.shape[0] == 3 and len(testloader) == 1
        assert isinstance(testloader, D.ResidentClipLoader) == (mode == "resident")
        eargs = types.SimpleNamespace(device="cuda:0", lr_net=0.01, epoch_eval_train=0, batch_train=256, model="ConvNet3D", eval_mode="SS")
        net = _net(num_classes)
        net.dropout.p = 0.0
        syn = torch.randn(2, 16, 3, 112, 112, generator=torch.Generator().manual_seed(1)).cuda()
        rec = []
        orig = utils.epoch

        def spy(m, *a):
            out = orig(m, *a)
            rec.append((m, out[0], out[1]))
            return out
        utils.epoch = spy
        try:
            _, _, acc_test, _ = utils.evaluate_synset(0, net, syn, torch.tensor([0, 1]).cuda(), testloader, eargs, mode="none")
        finally:
            utils.epoch = orig
        res[mode] = (acc_test, [r for r in rec if r[0] == "test"][0][1], _states())
    return res


def test_buffer_train_videos_resident_writes_a_buffer(tmp_path):
    from video_distillation_amd import buffer, checkpoint
    args = buffer.build_parser().parse_args(["--dataset", "miniUCF101", "--data_path", os.path.join(GOLD, "frames"), "--num_experts", "1",
                                             "--train_epochs", "2", "--batch_train", "2", "--lr_teacher", "0.01", "--save_interval", "1",
                                             "--num_workers", "2", "--buffer_path", str(tmp_path), "--train_videos", "resident"])
    _seed()
    files = buffer.run(args, log=lambda *_: None)
    assert [os.path.basename(f) for f in files] == ["replay_buffer_0.pt"]
    back = checkpoint.load_expert_buffers(str(tmp_path))
    assert len(back) == 1 and len(back[0]) == 3 and len(back[0][0]) == 8
    moved = [float((a - b).abs().max()) for a, b in zip(back[0][0], back[0][2])]
    assert all(np.isfinite(moved)) and max(moved) > 0
