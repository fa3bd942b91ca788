#!/usr/bin/env python3
"""The two still-clip kernels (csrc/still.hip) at n = 256 clips of 16x112x112: GB/s against the HBM peak, one JSON line.

  * ``expand``: 256 images (3,112,112) -> 256 clips (16,3,112,112), identity and through a random ``index`` with repeats
    (a gather out of a pool of 4 650 stills, the UCF50 shape).  Algorithmic bytes: n * 3HW * 4 read + n * T * 3HW * 4 written.
  * ``reduce``: 256 clip gradients -> 256 image gradients.  n * T * 3HW * 4 read + n * 3HW * 4 written.

Timed with device events around ``--launches`` back-to-back launches through the C ABI (no Python wrapper, no allocation in the
window) after a warm-up of the same shape, median of ``--reps`` windows; the window is sized to run for tenths of a second.  The
buffers of the larger side are 617 MB, more than the 256 MB Infinity Cache, so the figure is an HBM rate.  Peak: 8.0 TB/s spec;
6.29 TB/s is what a float4 copy reaches on this chip (the achievable bound, also recorded).  Results are checked against the torch
expressions before anything is timed.

    python tools/bench_still.py [--reps 7] [--launches 2000] [--out profiles/still_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_GBPS = 8000.0          # HBM3E spec
COPY_GBPS = 6290.0          # measured float4 copy on MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--im_size", type=int, default=112)
    ap.add_argument("--pool", type=int, default=4650)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from video_distillation_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_still.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    n, T, H = a.n, a.frames, a.im_size
    chw = 3 * H * H
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randn((a.pool, 3, H, H), device=dev, generator=g)
    index = torch.as_tensor(np.random.default_rng(0).integers(0, a.pool, n), device=dev)
    clips = torch.empty((n, T, 3, H, H), device=dev)
    images = torch.empty((n, 3, H, H), device=dev)
    grads = torch.randn((n, T, 3, H, H), device=dev, generator=g)
    lib, st = hip.lib(), hip.stream_ptr(dev)

    calls = {
        "expand_identity": lambda: lib.vds_still_expand(pool.data_ptr(), 0, n, T, H, H, clips.data_ptr(), st),
        "expand_gather": lambda: lib.vds_still_expand(pool.data_ptr(), index.data_ptr(), n, T, H, H, clips.data_ptr(), st),
        "reduce": lambda: lib.vds_still_reduce(grads.data_ptr(), n, T, H, H, images.data_ptr(), st),
    }
    # results first
    assert calls["expand_identity"]() == 0 and torch.equal(clips, pool[:n].unsqueeze(1).expand(-1, T, -1, -1, -1))
    assert calls["expand_gather"]() == 0 and torch.equal(clips, pool[index].unsqueeze(1).expand(-1, T, -1, -1, -1))
    assert calls["reduce"]() == 0
    want = grads[:, 0].clone()
    for t in range(1, T):
        want = want + grads[:, t]
    assert torch.equal(images, want)
    byt = n * chw * 4 * (T + 1)
    rec = {"shape": {"n": n, "frames": T, "im_size": H, "pool": a.pool}, "algorithmic_bytes": byt, "launches_per_window": a.launches,
           "reps": a.reps, "peak_GBps": PEAK_GBPS, "float4_copy_GBps": COPY_GBPS, "kernels": {},
           "sources": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev)}
    for name, call in calls.items():
        for _ in range(10):
            call()
        us = []
        for _ in range(a.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.launches):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3 / a.launches)
        med = float(np.median(us))
        rec["kernels"][name] = {"us_per_launch": med, "us_min": float(min(us)), "us_max": float(max(us)), "window_ms": med * a.launches / 1e3,
                                "GBps": byt / med / 1e3, "frac_of_peak": byt / med / 1e3 / PEAK_GBPS,
                                "frac_of_float4_copy": byt / med / 1e3 / COPY_GBPS}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
