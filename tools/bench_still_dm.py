#!/usr/bin/env python3
"""Still clips as first-level operand rows (csrc/still_rows.hip) and the still DM step they feed: one JSON line.

Kernel leg.  n = 3200 still clips of 16x112x112 (configuration 2's real batch: 50 classes x 64) gathered with repeats out of
4 650 stills, into the first level's 16-bit rows: ``vdsr_still_rows`` against ``vds_still_expand`` followed by ``vd_pix2rows``,
alternated in one process, for ``prec`` F16 (one plane) and F16X3 (two planes).  Through the C ABI, no allocation in a window;
device events around windows of back-to-back launches sized to run at least ``--window_s`` after a warm-up, median of ``--reps``
windows with min..max.  Algorithmic bytes: the gathered stills read once (n * 3HW * 4) + the rows written (planes * n * T * 3 * H *
pitch * 2); the composition also writes and reads the fp32 clips (2 * n * T * 3HW * 4), which is reported as its own traffic.
Peak: 8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches on this chip.  The two results are compared bit for bit first.

Step leg.  ``distill.StillDMTrainer`` at configuration 2's shape (50 classes, batch_real 64, spc 2, 16x112x112, 93 stills per
class) on the shipped mixed mode: windows of ``--steps`` overlapped steps, the real side through the new kernel and through the
two-launch composition (``HipBackend.still_rows_fused``) alternated, steps/s of each as median of ``--reps`` with min..max.

    python tools/bench_still_dm.py [--reps 7] [--out profiles/still_dm_bench.json]
"""
import argparse
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


def _stats(us):
    return {"us_per_launch": float(np.median(us)), "us_min": float(min(us)), "us_max": float(max(us))}


def kernel_leg(a, hip, dev):
    n, T, H = a.n, a.frames, a.im_size
    chw, cpr = 3 * H * H, (H + 8 + 7) // 8
    slots = n * T * 3 * H * cpr
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randn((a.pool, 3, H, H), device=dev, generator=g)
    index = torch.as_tensor(np.random.default_rng(0).integers(0, a.pool, n), device=dev)
    clips = torch.empty((n, T, 3, H, H), device=dev)
    rows = torch.empty((2, slots, 8), dtype=torch.int16, device=dev)
    want = torch.empty((2, slots, 8), dtype=torch.int16, device=dev)
    lib, st = hip.lib(), hip.stream_ptr(dev)
    out = {}
    for name, prec, planes in (("f16", hip.PREC["f16"], 1), ("f16x3", hip.PREC["f16x3"], 2)):
        def fused(dst=rows):
            return lib.vdsr_still_rows(pool.data_ptr(), index.data_ptr(), n, T, H, H, dst[0].data_ptr(),
                                       dst[1].data_ptr() if planes == 2 else 0, prec, st)

        def composed(dst=rows):
            rc = lib.vds_still_expand(pool.data_ptr(), index.data_ptr(), n, T, H, H, clips.data_ptr(), st)
            return rc or lib.vd_pix2rows(clips.data_ptr(), 0, n, T, H, H, dst[0].data_ptr(), dst[1].data_ptr() if planes == 2 else 0, prec, st)

        rows.fill_(-1)
        want.fill_(-2)
        assert fused(rows) == 0 and composed(want) == 0
        assert torch.equal(rows[:planes], want[:planes]), "vdsr_still_rows differs from vd_pix2rows(vds_still_expand) at prec %s" % name
        byt = n * chw * 4 + planes * slots * 16
        staged = 2 * n * T * chw * 4
        res = {}
        launches = {}
        for key, call in (("fused", fused), ("composed", composed)):
            for _ in range(3):
                call()
            launches[key] = max(3, int(np.ceil(a.window_s * 1e6 / _window(call, 3))))
        us = {"fused": [], "composed": []}
        for _ in range(a.reps):          # alternated: both see the same clocks and the same neighbours
            for key, call in (("fused", fused), ("composed", composed)):
                us[key].append(_window(call, launches[key]))
        for key in us:
            s = _stats(us[key])
            s.update(launches_per_window=launches[key], window_ms=s["us_per_launch"] * launches[key] / 1e3,
                     GBps=byt / s["us_per_launch"] / 1e3, frac_of_peak=byt / s["us_per_launch"] / 1e3 / PEAK_GBPS,
                     frac_of_float4_copy=byt / s["us_per_launch"] / 1e3 / COPY_GBPS)
            if key == "composed":
                s["traffic_bytes"] = byt + staged
                s["traffic_GBps"] = (byt + staged) / s["us_per_launch"] / 1e3
            res[key] = s
        res["algorithmic_bytes"] = byt
        res["speedup_median"] = res["composed"]["us_per_launch"] / res["fused"]["us_per_launch"]
        res["fused_median_below_composed_min"] = bool(res["fused"]["us_per_launch"] < res["composed"]["us_min"])
        out[name] = res
    return out


def step_leg(a, dev):
    from video_distillation_amd import distill, plan
    C, per, T, H = a.classes, a.pool // a.classes, a.frames, a.im_size
    geo = plan.NetGeometry(T, H, H)
    pool = distill.RealPool.synthetic(C, list(range(C)), per, plan.NetGeometry(1, H, H), dev)
    pool.clips = pool.clips[:, 0].contiguous()
    be = distill.HipBackend(geo, dev)
    tr = distill.StillDMTrainer(be, pool, geo, C, a.spc, a.batch_real, 1.0)
    it = 0
    rate = {"fused": [], "composed": []}
    for rep in range(-1, a.reps):          # (rep -1: warm-up of both paths, not recorded)
        for key in ("fused", "composed"):
            be.still_rows_fused = key == "fused"
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
    assert bool(torch.isfinite(tr.static).all())
    out = {k: {"steps_per_s": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in rate.items()}
    out.update(shape={"classes": C, "batch_real": a.batch_real, "spc": a.spc, "stills_per_class": per, "frames": T, "im_size": H},
               steps_per_window=a.steps, dither=be._dither, real_last=be.real_last)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3200)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--im_size", type=int, default=112)
    ap.add_argument("--pool", type=int, default=4650)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--batch_real", type=int, default=64)
    ap.add_argument("--spc", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--window_s", type=float, default=0.25)
    ap.add_argument("--legs", type=str, default="kernel,step")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from video_distillation_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_still_dm.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rec = {"shape": {"n": a.n, "frames": a.frames, "im_size": a.im_size, "pool": a.pool}, "reps": a.reps, "window_s": a.window_s,
           "peak_GBps": PEAK_GBPS, "float4_copy_GBps": COPY_GBPS, "sources": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev)}
    if "kernel" in a.legs:
        rec["kernel"] = kernel_leg(a, hip, dev)
        torch.cuda.empty_cache()
    if "step" in a.legs:
        rec["step"] = step_leg(a, dev)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
