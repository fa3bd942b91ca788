"""Host half of the device-resident video store (dataset.ResidentVideos / ResidentClipLoader, vd_clips_sample): the per-read
draws against ``FrameFolderVideos.draw`` on the committed JPEG tree, the flip / resize commutation the store rests on, and the
argument checks that must fire before anything reaches a device.  No GPU: the tables are built from directory listings."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from video_distillation_amd import dataset as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UCF = os.path.join(GOLD, "frames", "UCF101")
SSV2 = os.path.join(GOLD, "frames", "SSv2_64x8")


def _seed():
    np.random.seed(5); random.seed(7); torch.manual_seed(3)


def _states():
    return (np.random.get_state()[1].tolist(), np.random.get_state()[2], random.getstate(), torch.get_rng_state().tolist())


CASES = {
    "ucf_test": lambda: D.UCF101(UCF, "test"),
    "ucf_train": lambda: D.UCF101(UCF, "train"),
    "mini_seg": lambda: D.miniUCF101(UCF, "train", sample="split-random"),
    "mini_seg_test": lambda: D.miniUCF101(UCF, "test", sample="split-random"),
    "ucf_test_64": lambda: D.UCF101(UCF, "test", D.FrameTransform((64, 64))),
    "ucf_train_64": lambda: D.UCF101(UCF, "train", D.FrameTransform((64, 64))),
}


def _host_passes(ds, passes=3):
    _seed()
    out = [[ds.draw(i) for i in range(len(ds))] for _ in range(passes)]
    return out, _states()


def _resident_passes(ds, passes=3):
    store = D.ResidentVideos(ds)                      # listing only: no decode, no device
    _seed()
    out = []
    for _ in range(passes):
        draws = [store.draw(i) for i in range(len(ds))]
        out.append((draws, store.tables(draws)))
    return store, out, _states()


@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_draws_equal_the_host_draws_over_three_passes(case):
    host, host_state = _host_passes(CASES[case]())
    ds = CASES[case]()
    store, mine, my_state = _resident_passes(ds)
    assert my_state == host_state                                 # numpy, random and torch generators advanced identically
    cropped = ds.transform.resize is not None
    for want, (draws, (rows, flips, crops)) in zip(host, mine):
        rows = rows.reshape(len(ds), D.NUM_FRAMES)
        assert flips.dtype == np.uint8 and rows.dtype == np.int64
        for i, w in enumerate(want):
            # the rows of the table, resolved back to files through frame_offset
            numbers = rows[i] - store.frame_offset[i] + 1
            files = [os.path.join(ds.video_dirs[i], "frame%06d.jpg" % n) for n in numbers]
            assert files == w.files and all(os.path.exists(f) for f in files)
            assert draws[i].numbers == numbers.tolist()
            assert bool(flips[i]) == w.flip
            if cropped:
                assert crops.dtype == np.int32
                assert [tuple(c) for c in crops.reshape(len(ds), D.NUM_FRAMES, 2)[i].tolist()] == w.crops
            else:
                assert crops is None and w.crops == [None] * D.NUM_FRAMES


def test_the_seeds_make_the_passes_differ():
    """A frozen preload must not pass the equivalence tests: under seeds 5 / 7 / 3 the test items restart on every pass and the
    flips change, while a training item keeps its start."""
    ds = D.UCF101(UCF, "test")
    store, mine, _ = _resident_passes(ds)
    starts = [tuple(d.numbers[0] for d in draws) for draws, _ in mine]
    assert starts == [(2, 3), (2, 2), (1, 3)]
    assert [draws[0].flip for draws, _ in mine] == [False, True, True]
    ds = D.UCF101(UCF, "train")
    store, mine, _ = _resident_passes(ds)
    assert [tuple(d.numbers[0] for d in draws) for draws, _ in mine] == [(3, 7, 1)] * 3 and ds.start == [3, 7, 1]
    flips = [tuple(d.flip for d in draws) for draws, _ in mine]
    assert len(set(flips)) > 1


def test_host_and_resident_reads_share_the_cached_start():
    ds = D.UCF101(UCF, "train")
    store = D.ResidentVideos(ds)
    _seed()
    first = store.draw(1).numbers[0]
    assert ds.start[1] == first
    assert int(os.path.basename(ds.draw(1).files[0])[5:11]) == first         # the host read reuses it
    ds.start[2] = 4
    assert store.draw(2).numbers[0] == 4                                     # and the other way round


def test_flip_and_resize_commute_on_every_golden_frame():
    """The store keeps resized, UNFLIPPED frames and mirrors on the device; the host flips first and resizes then."""
    from PIL import Image
    root = os.path.join(UCF, "jpegs_112")
    n = differing = 0
    for d in sorted(os.listdir(root)):
        for f in sorted(os.listdir(os.path.join(root, d))):
            with Image.open(os.path.join(root, d, f)) as im:
                im = im.convert("RGB")
                a = np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT).resize((80, 100), Image.BILINEAR))
                b = np.asarray(im.resize((80, 100), Image.BILINEAR))[:, ::-1]
            differing += int((a != b).sum())
            n += 1
    assert n == 207 and differing == 0


def test_stored_pixels_is_the_deterministic_part_of_the_transform():
    from PIL import Image
    ds = D.UCF101(UCF, "test", D.FrameTransform((64, 64)))
    _seed()
    d = ds.draw(0)
    u8 = ds.read_u8(d)
    for k in (0, 7):
        with Image.open(d.files[k]) as im:
            stored = ds.transform.stored_pixels(im)
        assert stored.shape == (100, 80, 3)
        i, j = d.crops[k]
        xs = np.arange(j, j + 64)
        xs = 80 - 1 - xs if d.flip else xs
        np.testing.assert_array_equal(u8[k], stored[i:i + 64][:, xs])


@pytest.mark.parametrize("case", ["ucf_test", "ucf_test_64", "mini_seg"])
def test_oracle_over_stored_frames_equals_the_host_items(case):
    """The chain the GPU tests rest on, closed on the host: stored (resized, unflipped) frames + the tables of a draw, through
    the numpy restatement of vd_clips_sample, give ``dataset[i]`` bit for bit."""
    from PIL import Image
    from tests import resident_oracle as O
    ds = CASES[case]()
    _seed()
    want = [ds[i][0].numpy() for i in range(len(ds))]
    ds = CASES[case]()
    store = D.ResidentVideos(ds)
    frames = []
    for k in range(len(store)):
        for n in range(1, store.length[k] + 1):
            with Image.open(store._file(k, n)) as im:
                frames.append(ds.transform.stored_pixels(im))
    frames = np.stack(frames)
    assert frames.shape == (store.num_frames,) + store.frame_hw + (3,) and frames.nbytes == store.nbytes
    _seed()
    rows, flips, crops = store.tables([store.draw(i) for i in range(len(ds))])
    tf = ds.transform
    got = O.clips_sample(frames, rows, flips, crops, D.NUM_FRAMES, tf.im_size, tf.mean.tolist(), tf.std.tolist())
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_sizes_come_from_the_listing_and_max_bytes_refuses():
    ds = D.UCF101(UCF, "test")
    store = D.ResidentVideos(ds)
    lengths = [len(os.listdir(d)) for d in ds.video_dirs]
    assert store.length == lengths and store.frame_offset.tolist() == [0] + np.cumsum(lengths).tolist()
    assert store.frame_hw == (112, 112) and store.nbytes == sum(lengths) * 112 * 112 * 3
    assert store.labels.tolist() == ds.labels and store.frames is None
    with pytest.raises(ValueError) as e:
        D.ResidentVideos.from_dataset(ds, "cuda:0", max_bytes=1000)          # refused before any decode or device call
    assert str(store.nbytes) in str(e.value) and "1000" in str(e.value)
    with pytest.raises(ValueError):
        D.resident_loader(ds, "cuda:0", max_bytes=1000)
    small = D.ResidentVideos(D.UCF101(UCF, "test", D.FrameTransform((64, 64))), indices=[1])
    assert small.frame_hw == (100, 80) and small.nbytes == lengths[1] * 100 * 80 * 3 and len(small) == 1
    with pytest.raises(ValueError):
        small.draw(0)                                                        # not in the store


def test_unsupported_datasets_point_to_preload():
    with pytest.raises(ValueError, match="preload"):
        D.ResidentVideos(D.SSv2(SSV2, "train"))                              # an 'all' family
    with pytest.raises(ValueError, match="preload"):
        D.ResidentVideos(D.staticUCF101(UCF, "train"))                       # still frames
    with pytest.raises(RuntimeError):
        D.ResidentVideos(D.UCF101(UCF, "test")).load("cpu")


def test_bad_tables_raise_before_upload():
    ds = D.UCF101(UCF, "test", D.FrameTransform((64, 64)))
    store = D.ResidentVideos(ds)
    _seed()
    good = store.draw(0)
    store.tables([good])
    for numbers in ([0] + good.numbers[1:], good.numbers[:-1] + [store.length[0] + 1]):
        with pytest.raises(ValueError, match="out of range"):
            store.tables([D.ResidentDraw(0, numbers, False, good.crops)])
    for crop in ((37, 0), (0, 17), (-1, 0)):                                 # 100 - 64 = 36 rows, 80 - 64 = 16 columns of slack
        with pytest.raises(ValueError, match="past the edge"):
            store.tables([D.ResidentDraw(0, good.numbers, False, [crop] + good.crops[1:])])
    store.tables([D.ResidentDraw(0, good.numbers, True, [(36, 16)] * 16)])   # the last origin that fits
    # the generic check of sample_clips' tables
    with pytest.raises(ValueError, match="outside the store"):
        D.check_clip_tables(10, (8, 8), (8, 8), [0, 10], [0], None, 2)
    with pytest.raises(ValueError, match="outside the store"):
        D.check_clip_tables(10, (8, 8), (8, 8), [-1, 3], [0], None, 2)
    with pytest.raises(ValueError, match="no crop"):
        D.check_clip_tables(10, (8, 8), (4, 4), [0, 1], [0], None, 2)
    with pytest.raises(ValueError, match="larger"):
        D.check_clip_tables(10, (8, 8), (9, 8), [0, 1], [0], [(0, 0), (0, 0)], 2)
    with pytest.raises(ValueError):
        D.check_clip_tables(10, (8, 8), (8, 8), [0, 1, 2], [0], None, 2)     # 3 rows for 1 clip of 2 frames


def test_clips_sample_argument_errors_come_before_any_device_call():
    from video_distillation_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    fn = hip.bind(hip.LIB_PATH).vd_clips_sample
    p = ctypes.c_void_p(4096)                            # never dereferenced: every call below returns before a launch
    null = ctypes.c_void_p(0)
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    std = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    zero_std = (ctypes.c_float * 3)(0.229, 0.0, 0.225)
    i64 = ctypes.c_int64

    def call(frames=p, store=i64(10), sh=8, sw=8, rows=p, crop=null, flip=p, n=i64(2), t=4, oh=8, ow=8, dst=p, m=mean, s=std):
        return fn(frames, store, sh, sw, rows, crop, flip, n, t, oh, ow, dst, m, s, null)

    assert call(n=i64(0)) == 0                                               # nothing to do
    assert call(n=i64(0), frames=null, rows=null, flip=null, dst=null) == 0
    for kw in (dict(frames=null), dict(rows=null), dict(flip=null), dict(dst=null), dict(m=null), dict(s=null)):
        assert call(**kw) == -1, kw                                          # null pointers with non-zero work
    for kw in (dict(store=i64(-1)), dict(sh=-1), dict(sw=-1), dict(n=i64(-1)), dict(t=-1), dict(oh=-1), dict(ow=-1)):
        assert call(**kw) == -1, kw                                          # negative sizes
    assert call(s=zero_std) == -1
    assert call(oh=9, crop=p) == -1 and call(ow=9, crop=p) == -1             # out > src
    assert call(oh=4, ow=4) == -1                                            # out != src needs crop_yx
    assert call(oh=4) == -1 and call(ow=4) == -1


def test_loader_length_and_dataset_match_the_dataloader():
    ds = D.UCF101(UCF, "train")
    loader = D.ResidentClipLoader(D.ResidentVideos(ds), batch_size=2)
    ref = torch.utils.data.DataLoader(ds, batch_size=2)
    assert len(loader) == len(ref) == 2 and loader.dataset is ref.dataset
    with pytest.raises(RuntimeError):
        next(iter(loader))                                                   # not loaded: an error, not a host fallback


def test_driver_flags_default_to_today():
    from video_distillation_amd import buffer, run_coreset, run_dm
    assert run_dm.build_parser().parse_args([]).test_videos == "host"
    assert run_coreset.build_parser().parse_args([]).test_videos == "host"
    assert buffer.build_parser().parse_args([]).train_videos == "preload"
    assert run_dm.build_parser().parse_args(["--test_videos", "resident"]).test_videos == "resident"
    with pytest.raises(SystemExit):
        buffer.build_parser().parse_args(["--train_videos", "host"])
