#!/usr/bin/env python3
"""The two key-frame kernels (csrc/keyframes.hip) next to the still kernels, and the DM step they feed: one JSON line.

Kernel leg.  n = 256 clips of 16x3x112x112 (617 MB, more than the 256 MB Infinity Cache: HBM rates) through the C ABI, the tables
(16, 4, linear), (16, 4, nearest) and (16, 1), alternated in one process with ``vds_still_expand`` / ``vds_still_reduce`` on the
same clip bytes.  No allocation in a window; device events around windows of back-to-back launches sized to run at least
``--window_s`` after a warm-up, median of ``--reps`` windows with min..max.  Algorithmic bytes, stated per entry: expand reads
the K key frames once and writes T frames, n * (K + T) * 3HW * 4; reduce reads a gradient frame once per key that references it
and writes K frames, n * (reads + K) * 3HW * 4 with reads = T for nearest and K = 1, and the count of (frame, key) pairs with
a non-zero weight for linear (28 at T = 16, K = 4: every frame but the first of a segment and the last is read by two keys).
``unique_bytes`` counts every gradient frame once.  Peak: 8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches on this chip.
Results are compared with the torch expressions before anything is timed.

Step leg.  ``distill.DMTrainer`` and ``distill.KeyframeDMTrainer`` (K = 4, linear) at configuration 2's shape (50 classes,
batch_real 64, ipc 1, 16x112x112, 93 clips per class) on the shipped mixed mode: windows of ``--steps`` overlapped steps,
alternated, steps/s of each as median of ``--reps`` with min..max.

    python tools/bench_keyframes.py [--reps 7] [--out profiles/keyframes_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_GBPS = 8000.0          # HBM3E spec
COPY_GBPS = 6290.0          # measured float4 copy on MI355X


def _window(call, launches):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(launches):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / launches          # us per launch


def kernel_leg(a, hip, dev):
    from video_distillation_amd import keyframes
    n, T, H = a.n, a.frames, a.im_size
    frame = 3 * H * H * 4          # bytes
    g = torch.Generator(device=dev).manual_seed(0)
    keys = torch.randn((n, T, 3, H, H), device=dev, generator=g)          # (the first K frames of a row are a table's keys: K <= T)
    grads = torch.randn((n, T, 3, H, H), device=dev, generator=g)
    clips = torch.empty((n, T, 3, H, H), device=dev)
    g_keys = torch.empty((n, T, 3, H, H), device=dev)
    lib, st = hip.lib(), hip.stream_ptr(dev)
    calls, byt, uniq = {}, {}, {}
    tables = {"k4_linear": keyframes.table(T, 4, "linear"), "k4_nearest": keyframes.table(T, 4, "nearest"), "k1": keyframes.table(T, 1, "linear")}
    for name, tab in tables.items():
        K, ct = tab.K, hip.vdk_table(tab)
        src = keys[:, :K].contiguous()
        reads = sum(len(tab.terms(k)) for k in range(K))
        calls["expand_" + name] = lambda src=src, ct=ct: lib.vdk_keyframe_expand(src.data_ptr(), n, ctypes.addressof(ct), H, H, clips.data_ptr(), st)
        calls["reduce_" + name] = lambda ct=ct: lib.vdk_keyframe_reduce(grads.data_ptr(), n, ctypes.addressof(ct), H, H, g_keys.data_ptr(), st)
        byt["expand_" + name] = uniq["expand_" + name] = n * (K + T) * frame
        byt["reduce_" + name], uniq["reduce_" + name] = n * (reads + K) * frame, n * (T + K) * frame
        # results first
        assert calls["expand_" + name]() == 0 and torch.equal(clips, keyframes.expand_torch(src, tab)), name
        assert calls["reduce_" + name]() == 0 and torch.equal(g_keys.view(-1)[:n * K * 3 * H * H].view(n, K, 3, H, H), keyframes.reduce_torch(grads, tab)), name
    still = keys[:, 0].contiguous()
    calls["still_expand"] = lambda: lib.vds_still_expand(still.data_ptr(), 0, n, T, H, H, clips.data_ptr(), st)
    calls["still_reduce"] = lambda: lib.vds_still_reduce(grads.data_ptr(), n, T, H, H, g_keys.data_ptr(), st)
    for name in ("still_expand", "still_reduce"):
        byt[name] = uniq[name] = n * (1 + T) * frame
        assert calls[name]() == 0
    launches = {}
    for name, call in calls.items():
        for _ in range(5):
            call()
        launches[name] = max(3, int(np.ceil(a.window_s * 1e6 / _window(call, 3))))
    us = {name: [] for name in calls}
    for _ in range(a.reps):          # alternated: all see the same clocks and the same neighbours
        for name, call in calls.items():
            us[name].append(_window(call, launches[name]))
    out = {}
    for name, v in us.items():
        med = float(np.median(v))
        out[name] = {"us_per_launch": med, "us_min": float(min(v)), "us_max": float(max(v)), "launches_per_window": launches[name],
                     "window_ms": med * launches[name] / 1e3, "algorithmic_bytes": byt[name], "unique_bytes": uniq[name],
                     "GBps": byt[name] / med / 1e3, "frac_of_peak": byt[name] / med / 1e3 / PEAK_GBPS,
                     "frac_of_float4_copy": byt[name] / med / 1e3 / COPY_GBPS, "us_per_clip_MB": med / (n * T * frame / 1e6)}
    for name in tables:          # per clip byte (both kinds move the same n * T frames on their larger side): time against the still kernel's
        out["expand_" + name]["time_vs_still"] = out["expand_" + name]["us_per_launch"] / out["still_expand"]["us_per_launch"]
        out["reduce_" + name]["time_vs_still"] = out["reduce_" + name]["us_per_launch"] / out["still_reduce"]["us_per_launch"]
    return out


def step_leg(a, dev):
    from video_distillation_amd import distill, plan
    C, per, T, H = a.classes, a.per_class, a.frames, a.im_size
    geo = plan.NetGeometry(T, H, H)
    pool = distill.RealPool.synthetic(C, list(range(C)), per, geo, dev)
    trainers = {"clips": distill.DMTrainer(distill.HipBackend(geo, dev), pool, C, a.ipc, a.batch_real, 1.0),
                "keyframes_k4": distill.KeyframeDMTrainer(distill.HipBackend(geo, dev), pool, geo, C, a.ipc, a.batch_real, 1.0, key_frames=4)}
    rate = {k: [] for k in trainers}
    it = 0
    for rep in range(-1, a.reps):          # (rep -1: warm-up of both, not recorded)
        for key, tr in trainers.items():
            tr.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(it, overlap=True)
                it += 1
            tr.sync()
            torch.cuda.synchronize()
            if rep >= 0:
                rate[key].append(a.steps / (time.perf_counter() - t0))
    assert bool(torch.isfinite(trainers["keyframes_k4"].keys).all())
    out = {k: {"steps_per_s": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in rate.items()}
    out.update(shape={"classes": C, "batch_real": a.batch_real, "ipc": a.ipc, "clips_per_class": per, "frames": T, "im_size": H},
               steps_per_window=a.steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--im_size", type=int, default=112)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--per_class", type=int, default=93)
    ap.add_argument("--batch_real", type=int, default=64)
    ap.add_argument("--ipc", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--window_s", type=float, default=0.25)
    ap.add_argument("--legs", type=str, default="kernel,step")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from video_distillation_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyframes.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rec = {"shape": {"n": a.n, "frames": a.frames, "im_size": a.im_size}, "reps": a.reps, "window_s": a.window_s, "peak_GBps": PEAK_GBPS,
           "float4_copy_GBps": COPY_GBPS, "sources": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev)}
    if "kernel" in a.legs:
        rec["kernel"] = kernel_leg(a, hip, dev)
        torch.cuda.empty_cache()
    if "step" in a.legs:
        rec["step"] = step_leg(a, dev)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
