#!/usr/bin/env python3
"""What the MTT driver's two switches cost or save, measured in one process: one JSON document (``--out``, default
profiles/mtt_driver_bench.json).

At bench configuration 5's shape (C = 400, 256 hallucinator-composed clips 64x64x8 per student step x 10 steps, static frozen,
synthetic random-walk expert buffer; ``--classes`` / ``--batch`` / ``--syn_steps``):

  * ``iteration``: ``S2DMTTTrainer.step`` with ``fused_flat`` off and on -- the legs alternated ``--rounds`` (3) times after a
    warm-up of each, ``--iters`` iterations per timing between two device events; per leg every timing, median and min..max.
    The min..max range of the OFF leg is the noise floor; "on slower beyond the noise floor" = median(on) - median(off) exceeds it;
  * ``fetch``: start + target parameters of one iteration as ``MTTTrainer.step`` gets them from the list form of a buffer file
    (16 pageable tensors host -> device and two ``torch.cat``), from ``ExpertStore(mode="host")`` (two pinned rows, asynchronous)
    and from ``mode="resident"`` (two views): host clock from the call to the end of a device synchronise, per fetch;
  * ``kernels``: the three ``vdt_`` entry points at that P next to ``vd_sgd_momentum`` at the same n (the yardstick of a
    streaming kernel of this class on this box), alternated, device events around ``--launches`` launches; GB/s over the
    algorithmic bytes (step 3n, loss 6n -- two passes --, adjoint 5n, sgd 5n floats).

Nothing here is a pass/fail threshold.

    python tools/bench_mtt_driver.py [--out profiles/mtt_driver_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

T, H, W = 8, 64, 64


def stats(v, unit="ms"):
    v = sorted(v)
    return {"median_" + unit: float(np.median(v)), "min_" + unit: v[0], "max_" + unit: v[-1], "reps": len(v), "all_" + unit: v}


def bench_iteration(distill, plan, dev, C, batch, syn_steps, iters, rounds):
    geo = plan.NetGeometry(T, H, W)
    gen = torch.Generator(device=dev); gen.manual_seed(99)
    traj = [distill.fresh_full_network(5, C, dev)]
    for _ in range(11):
        traj.append([p + 0.01 * p.abs().mean() * torch.randn(p.shape, device=dev, generator=gen) for p in traj[-1]])
    ops = distill.HipMTTOps(geo, C, dev, dropout_p=0.5, batch_hint=batch, fused_flat=True)
    chain = ops.flat
    trainers = {}
    for leg in ("off", "on"):
        g2 = torch.Generator(device=dev); g2.manual_seed(7)
        static = torch.randn(C * 2, 3, H, W, device=dev, generator=g2)
        dynamic = torch.randn(C, 2, T, 1, H, W, device=dev, generator=g2)
        hal_w = torch.empty(3, 4, 3, 3, 3, device=dev).uniform_(-0.096, 0.096, generator=g2)
        hal_b = torch.empty(3, device=dev).uniform_(-0.096, 0.096, generator=g2)
        trainers[leg] = distill.S2DMTTTrainer(ops, C, 1, 2, 2, static, dynamic, hal_w, hal_b, syn_lr=0.01, lr_dynamic=0.01, lr_hal=0.01,
                                              lr_lr=1e-5, syn_steps=syn_steps, batch_syn=batch, expert_epochs=1, max_start_epoch=10)
    times, last, it = {"off": [], "on": []}, {}, {"off": 0, "on": 0}
    for rnd in range(rounds + 1):          # round 0: warm-up of both legs
        for leg in ("off", "on"):
            ops.flat = chain if leg == "on" else None
            tr = trainers[leg]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                grand = tr.step(it[leg], traj)
                it[leg] += 1
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / iters
            if rnd:
                times[leg].append(ms)
            last[leg] = float(grand)
            print("fused_flat %s round %d: %.2f ms / iteration (grand loss %.6f)" % (leg, rnd, ms, last[leg]), flush=True)
    ops.flat = chain
    res = {"off": stats(times["off"]), "on": stats(times["on"]), "iterations_per_timing": iters, "grand_loss_last": last}
    floor = res["off"]["max_ms"] - res["off"]["min_ms"]
    diff = res["on"]["median_ms"] - res["off"]["median_ms"]
    res.update({"noise_floor_ms": floor, "on_minus_off_median_ms": diff, "on_slower_beyond_noise_floor": bool(diff > floor),
                "on_over_off": res["on"]["median_ms"] / res["off"]["median_ms"]})
    return res


def bench_fetch(distill, experts, checkpoint, dev, C, reps):
    d = tempfile.mkdtemp(prefix="mtt_buffer_")
    try:
        g = torch.Generator().manual_seed(3)
        walk = []
        for _ in range(2):
            cur = [0.05 * torch.randn(s, generator=g) for s in distill.FULL_SHAPES(C)]
            tr = [cur]
            for _ in range(3):
                cur = [p + 0.01 * p.abs().mean() * torch.randn(p.shape, generator=g) for p in cur]
                tr.append(cur)
            walk.append(tr)
        checkpoint.save_expert_buffer(d, walk)
        listed = torch.load(os.path.join(d, "replay_buffer_0.pt"), map_location="cpu")

        def from_list(k):
            t = listed[k % 2]
            start = [p.to(dev, torch.float32) for p in t[k % 3]]
            target = distill.flatten_params([p.to(dev, torch.float32) for p in t[k % 3 + 1]])
            return distill.flatten_params(start), target
        # (walk="reference": the one file is never read again, so a fetch times the rows only)
        stores = {m: experts.ExpertStore(d, C, dev, mode=m, walk="reference", seed=1) for m in ("host", "resident")}

        def from_store(m):
            def fetch(k):
                t = stores[m].next()
                return t.row(k % 3), t.row(k % 3 + 1)
            return fetch
        legs = {"list": from_list, "host": from_store("host"), "resident": from_store("resident")}
        times = {k: [] for k in legs}
        for rep in range(reps + 2):          # two warm-up rounds
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a, b = fn(rep)
                t_issue = time.perf_counter() - t0
                torch.cuda.synchronize()
                t_all = time.perf_counter() - t0
                if rep >= 2:
                    times[name].append((t_issue * 1e3, t_all * 1e3))
                del a, b
        res = {"row_floats": stores["host"].P, "bytes_per_fetch": 2 * 4 * stores["host"].P}
        for name, v in times.items():
            res[name] = {"host_blocked_ms": stats([x[0] for x in v]), "until_on_device_ms": stats([x[1] for x in v])}
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def bench_kernels(hip, dev, n, launches, reps):
    g = torch.Generator(device=dev); g.manual_seed(11)
    theta, theta0, target, grad, hv, tbar, v, out, buf = (0.05 * torch.randn(n, device=dev, generator=g) for _ in range(9))
    lr = torch.tensor(0.01, device=dev)
    scratch = torch.empty(hip.lib().vdt_traj_scratch_doubles(n), dtype=torch.float64, device=dev)
    rec, g_lr = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    st = hip.stream_ptr(dev)
    legs = {
        "vdt_traj_step": (3, lambda: hip.run("vdt_traj_step", hip.ptr(theta), hip.ptr(grad), hip.ptr(lr), n, hip.ptr(out), st)),
        "vdt_traj_loss": (6, lambda: hip.run("vdt_traj_loss", hip.ptr(theta), hip.ptr(theta0), hip.ptr(target), n, hip.ptr(scratch),
                                             hip.ptr(rec), hip.ptr(tbar), st)),
        "vdt_traj_adjoint": (5, lambda: hip.run("vdt_traj_adjoint", hip.ptr(tbar), hip.ptr(hv), hip.ptr(grad), hip.ptr(lr), 1.0, n,
                                                hip.ptr(scratch), hip.ptr(g_lr), hip.ptr(v), st)),
        "vd_sgd_momentum": (5, lambda: hip.run("vd_sgd_momentum", hip.ptr(out), hip.ptr(buf), hip.ptr(grad), n, 1e-6, 0.5, 0, st)),
    }
    for _, fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, (_, fn) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / launches)
    res = {"n": n, "launches_per_rep": launches}
    for k, tv in times.items():
        byt = legs[k][0] * n * 4
        r = stats(tv)
        r.update({"bytes": byt, "GBps": byt / (r["median_ms"] * 1e-3) / 1e9, "GBps_min": byt / (r["max_ms"] * 1e-3) / 1e9,
                  "GBps_max": byt / (r["min_ms"] * 1e-3) / 1e9})
        res[k] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--syn_steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fetch_reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mtt_driver_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mtt_driver: needs the GPU (nothing here is a CPU measurement)")
    from video_distillation_amd import checkpoint, distill, experts, hip, plan
    dev = torch.device("cuda:0")
    doc = {"_source": {"tool": "tools/bench_mtt_driver.py", "kernel_sources_sha256_16": hip.sources_hash(),
                       "library_stamp": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev), "geometry": [T, H, W],
                       "args": {k: v for k, v in vars(a).items() if k != "out"}}}
    doc["kernels"] = bench_kernels(hip, dev, experts.param_count(a.classes), a.launches, a.reps)
    doc["fetch"] = bench_fetch(distill, experts, checkpoint, dev, a.classes, a.fetch_reps)
    torch.cuda.empty_cache()
    doc["iteration"] = bench_iteration(distill, plan, dev, a.classes, min(a.batch, a.classes), a.syn_steps, a.iters, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
