#!/usr/bin/env python3
"""Resident whole videos against the host loader: one JSON document (``--out``, default profiles/resident_videos_bench.json).

No dataset is assumed: the tool writes its own UCF101-layout JPEG tree from a seed into a temporary directory (``--videos``
test videos of ``--min_frames`` .. ``--max_frames`` frames, 112x112, smooth moving patterns + noise so that the JPEGs cost what
real frames cost to decode) and removes it at the end.  Measured, all on the device the store lives on:

  * ``store``: ``ResidentVideos.from_dataset`` -- seconds, frames/s (decode threads + H2D), bytes;
  * ``epoch_test``: one ``utils.epoch('test')`` (three passes, ConvNet3D) over the tree through the host ``DataLoader``
    (num_workers=0, 16 JPEG decodes per read) and through ``ResidentClipLoader``, alternated ``--rounds`` times in one process,
    wall clock ending in a device synchronise; the ratio with both absolute times, and that the two give the same accuracy;
  * ``kernel``: ``vd_clips_sample`` (no flip / every clip flipped / half of them; and the cropped scalar path out of a 100x80
    store) against ``vd_frames_normalize`` over the same number of frames: device events around ``--launches`` launches after a
    warm-up, the kernels alternated, ``--reps`` repetitions; median, min..max, GB/s (15 bytes per output pixel + the tables) and
    the share of the 8 TB/s HBM peak.

    python tools/bench_resident_videos.py [--videos 240] [--out profiles/resident_videos_bench.json]
"""
import argparse
import csv
import json
import os
import random
import shutil
import sys
import tempfile
import time
import types
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

HBM_PEAK = 8.0e12          # bytes/s, spec


def write_tree(root, videos, classes, min_frames, max_frames, seed, threads=16):
    """root/ucf101_splits1.csv + root/jpegs_112/<video>/frame%06d.jpg (all in the 'test' split) -> total frames."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    lengths = rng.randint(min_frames, max_frames + 1, size=videos)
    os.makedirs(os.path.join(root, "jpegs_112"))
    with open(os.path.join(root, "ucf101_splits1.csv"), "w", newline="") as fp:
        w = csv.writer(fp)
        w.writerow(["folder_name", "label", "split"])
        for v in range(videos):
            w.writerow(["v_%04d" % v, "class%02d" % (v % classes), "test"])

    def one(v):
        r = np.random.RandomState(seed * 7919 + v)
        d = os.path.join(root, "jpegs_112", "v_%04d" % v)
        os.makedirs(d)
        base = np.asarray(Image.fromarray(r.randint(0, 256, (14, 24, 3), dtype=np.uint8)).resize((192, 112), Image.BICUBIC), dtype=np.int16)
        for n in range(1, int(lengths[v]) + 1):
            shift = (n * 80) // int(lengths[v])
            img = base[:, shift:shift + 112] + r.randint(-12, 13, (112, 112, 3))
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(d, "frame%06d.jpg" % n), quality=90)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(videos)))
    return int(lengths.sum())


def seed_all():
    np.random.seed(5); random.seed(7); torch.manual_seed(3)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def timed_launches(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def bench_kernels(D, dev, clips, launches, reps):
    """vd_clips_sample against vd_frames_normalize over clips * 16 frames."""
    import ctypes
    from video_distillation_amd import hip
    T, H, W = 16, 112, 112
    nf = clips * T
    g = torch.Generator().manual_seed(1)
    store_frames = 3 * nf                                        # the sampler gathers out of a store three times the batch
    store = torch.randint(0, 256, (store_frames, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    store100 = torch.randint(0, 256, (nf, 100, 80, 3), dtype=torch.uint8, generator=g).to(dev)
    rng = np.random.RandomState(2)
    starts = rng.randint(0, store_frames - 4 * T, size=clips)
    rows = torch.from_numpy((starts[:, None] + 4 * np.arange(T)[None, :]).reshape(-1).astype(np.int64)).to(dev)      # a window, stride 4
    rows100 = torch.from_numpy(rng.randint(0, nf, size=nf).astype(np.int64)).to(dev)
    crops = torch.from_numpy(np.stack([rng.randint(0, 37, size=nf), rng.randint(0, 17, size=nf)], 1).astype(np.int32)).to(dev)
    flips = {"no_flip": torch.zeros(clips, dtype=torch.uint8), "all_flipped": torch.ones(clips, dtype=torch.uint8),
             "half_flipped": torch.from_numpy((rng.rand(clips) > 0.5).astype(np.uint8))}
    flips = {k: v.to(dev) for k, v in flips.items()}
    out = torch.empty((clips, T, 3, H, W), dtype=torch.float32, device=dev)
    out64 = torch.empty((clips, T, 3, 64, 64), dtype=torch.float32, device=dev)
    m = (ctypes.c_float * 3)(*D.IMAGENET_MEAN)
    s = (ctypes.c_float * 3)(*D.IMAGENET_STD)
    st = hip.stream_ptr(dev)

    def sample(flip):
        return lambda: hip.run("vd_clips_sample", hip.ptr(store), store_frames, H, W, hip.ptr(rows), None, hip.ptr(flip), clips, T,
                               H, W, hip.ptr(out), m, s, st)

    def sample_cropped():
        hip.run("vd_clips_sample", hip.ptr(store100), nf, 100, 80, hip.ptr(rows100), hip.ptr(crops), hip.ptr(flips["half_flipped"]),
                clips, T, 64, 64, hip.ptr(out64), m, s, st)

    def normalise():
        hip.run("vd_frames_normalize", hip.ptr(store), hip.ptr(out), nf, H, W, m, s, st)

    legs = {"frames_normalize": normalise, "clips_sample_cropped_100x80_to_64x64": sample_cropped}
    legs.update({"clips_sample_" + k: sample(v) for k, v in flips.items()})
    for fn in legs.values():                                     # warm-up: code objects, clocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():                               # alternated within every repetition
            times[k].append(timed_launches(fn, launches))
    res = {}
    for k, v in times.items():
        px = nf * (64 * 64 if "cropped" in k else H * W)
        byt = px * 15 + (0 if k == "frames_normalize" else nf * 8 + clips + (nf * 8 if "cropped" in k else 0))
        r = stats(v)
        r.update({"bytes": byt, "GBps": byt / (r["median_ms"] * 1e-3) / 1e9, "share_of_hbm_peak": byt / (r["median_ms"] * 1e-3) / HBM_PEAK})
        res[k] = r
    base = res["frames_normalize"]
    for k, r in res.items():
        if k.startswith("clips_sample") and "cropped" not in k:
            r["over_frames_normalize"] = r["median_ms"] / base["median_ms"]
    res["_shape"] = {"clips": clips, "frames": nf, "launches_per_rep": launches,
                     "yardstick": "frames_normalize median with its min..max as margin (same pixels, no tables)"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=240)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--min_frames", type=int, default=100)
    ap.add_argument("--max_frames", type=int, default=200)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernel_clips", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resident_videos_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident_videos: needs the GPU (nothing here is a CPU measurement)")
    from video_distillation_amd import dataset as D, hip, utils
    dev = torch.device("cuda:0")
    doc = {"_source": {"tool": "tools/bench_resident_videos.py", "kernel_sources_sha256_16": hip.sources_hash(),
                       "device": torch.cuda.get_device_name(dev), "args": {k: v for k, v in vars(a).items() if k != "out"}}}
    tmp = tempfile.mkdtemp(prefix="resident_videos_")
    try:
        t0 = time.time()
        total = write_tree(tmp, a.videos, a.classes, a.min_frames, a.max_frames, a.seed)
        doc["tree"] = {"videos": a.videos, "frames": total, "frame_size": [112, 112], "write_seconds": time.time() - t0}
        print("tree: %d videos, %d frames, written in %.1f s" % (a.videos, total, time.time() - t0), flush=True)
        ds = D.UCF101(tmp, "test")
        store = D.ResidentVideos.from_dataset(ds, dev, workers=a.workers)
        doc["store"] = {"build_seconds": store.build_seconds, "frames_per_second": store.num_frames / store.build_seconds,
                        "bytes": store.nbytes, "frames": store.num_frames, "decode_threads": min(a.workers, 16)}
        print("store: %.2f s, %.0f frames/s, %.3f GB" % (store.build_seconds, store.num_frames / store.build_seconds, store.nbytes / 1e9), flush=True)
        torch.manual_seed(11)
        net = utils.get_network('ConvNet3D', 3, a.classes, (112, 112), frames=16, dist=False).to(dev)
        args = types.SimpleNamespace(device=str(dev), model="ConvNet3D", eval_mode="SS")
        crit = torch.nn.CrossEntropyLoss()
        loaders = {"host": torch.utils.data.DataLoader(ds, batch_size=64, shuffle=False, num_workers=0),
                   "resident": D.ResidentClipLoader(store, batch_size=64)}
        with torch.no_grad():
            utils.epoch('test', loaders["resident"], net, None, crit, args)        # warm-up of the eval programs
            torch.cuda.synchronize()
            secs, accs = {"host": [], "resident": []}, {}
            for _ in range(a.rounds):
                for k in ("host", "resident"):
                    seed_all()
                    torch.cuda.synchronize()
                    t0 = time.time()
                    loss, acc, _ = utils.epoch('test', loaders[k], net, None, crit, args)
                    torch.cuda.synchronize()
                    secs[k].append(time.time() - t0)
                    accs[k] = (loss, acc)
                    print("epoch('test') %s: %.2f s (loss %.6f acc %.4f)" % (k, secs[k][-1], loss, acc), flush=True)
        h, r = float(np.median(secs["host"])), float(np.median(secs["resident"]))
        doc["epoch_test"] = {"clips_read": 3 * len(ds), "host_seconds": secs["host"], "resident_seconds": secs["resident"],
                             "host_median_s": h, "resident_median_s": r, "host_over_resident": h / r,
                             "host_ms_per_clip": h / (3 * len(ds)) * 1e3, "resident_ms_per_clip": r / (3 * len(ds)) * 1e3,
                             "same_accuracy": accs["host"][1] == accs["resident"][1],
                             "loss": {"host": accs["host"][0], "resident": accs["resident"][0]}}
        del store, loaders
        torch.cuda.empty_cache()
        doc["kernel"] = bench_kernels(D, dev, a.kernel_clips, a.launches, a.reps)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
