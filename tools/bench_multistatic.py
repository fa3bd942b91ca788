#!/usr/bin/env python3
"""Multi-static training epochs composed on the device against the host loader: one JSON document (``--out``, default
profiles/multistatic_bench.json).

At 112x112x16 with C = 50 (``--classes``), on the two workloads of the reference's launchers -- ``vpc 1 / spc 2 / dpc 2`` (50 items
an epoch) and ``vpc 5 / spc 10 / dpc 10`` (250 items) -- and seeded noise memories:

  * ``epochs``: ``utils.epoch('train')`` -- what ``evaluate_synset(mode='multi-static')`` runs ``epoch_eval_train + 1`` times per
    network -- over ``utils.MultiStaticBatches`` (one ``vd_hallucinator_fwd_multi`` launch per batch) and over the
    ``DataLoader`` of ``MultiStaticSharedDataset`` (one single-clip launch per item + ``torch.stack``), which this tool
    constructs directly; ``--epochs`` epochs per timing, the two alternated ``--rounds`` times in one process after a warm-up
    of each, host clock ending in a device synchronise; per leg every timing, median and min..max, and the last epoch's loss of
    both under equal seeds; "slower beyond the spread" = the difference of the medians exceeds the wider of the two legs'
    min..max ranges;
  * ``kernel``: ``vd_hallucinator_fwd_multi`` (``--n_hal`` sets, a set per clip) against ``vd_hallucinator_fwd`` over the same
    gathers at ``n = 250``: device events around ``--launches`` launches after a warm-up, the kernels alternated, ``--reps``
    repetitions; median, min..max, GB/s over the algorithmic bytes (3 + T + 3T floats per pixel column).

    python tools/bench_multistatic.py [--out profiles/multistatic_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

HBM_PEAK = 8.0e12          # bytes/s, spec
T, H, W = 16, 112, 112
WORKLOADS = {"vpc1_spc2_dpc2": (2, 2), "vpc5_spc10_dpc10": (10, 10)}          # name -> (spc, dpc)


def seed_all():
    np.random.seed(5); random.seed(7); torch.manual_seed(3)


def stats(v, unit):
    v = sorted(v)
    return {"median_" + unit: float(np.median(v)), "min_" + unit: v[0], "max_" + unit: v[-1], "reps": len(v)}


def beyond_spread(a, b, name):
    """Is leg ``a`` slower than leg ``b`` beyond the spread?  The MEDIANS are compared (one lucky repetition decides nothing),
    and the spread is the wider of the two legs' observed min..max ranges."""
    diff = a["median_ms"] - b["median_ms"]
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return {name: {"median_difference_ms": diff, "spread_ms": spread, "beyond_spread": bool(diff > spread)}}


def bench_epochs(utils, dev, classes, spc, dpc, n_hal, batch_train, epochs, rounds):
    g = torch.Generator().manual_seed(1)
    static = torch.randn(classes * spc, 3, H, W, generator=g).to(dev)
    dynamic = torch.randn(classes, dpc, T, 1, H, W, generator=g).to(dev)
    torch.manual_seed(2)
    hals = [utils.Conv3DNet().to(dev) for _ in range(n_hal)]
    loaders = {"device": utils.MultiStaticBatches(static, dynamic, hals, batch_train, shuffle=True),
               "host": torch.utils.data.DataLoader(utils.MultiStaticSharedDataset(static, dynamic, hals), batch_size=batch_train,
                                                   shuffle=True, num_workers=0)}
    args = types.SimpleNamespace(device=str(dev), model="ConvNet3D", eval_mode="SS")
    crit = torch.nn.CrossEntropyLoss().to(dev)
    from video_distillation_amd import evalpool
    make_net = evalpool.convnet3d_factory(classes, (H, W), T)          # (utils.get_network would reseed from the clock)
    secs, last = {k: [] for k in loaders}, {}
    for rnd in range(rounds + 1):                                  # round 0: warm-up of both legs (programs, allocator, clocks)
        for k in ("device", "host"):
            seed_all()                                             # (the same network, shuffles and draws on both legs)
            net = make_net(0).to(dev)
            opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0005)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(epochs):
                loss, acc, _ = utils.epoch('train', loaders[k], net, opt, crit, args)
            torch.cuda.synchronize()
            if rnd:
                secs[k].append((time.time() - t0) / epochs)
            last[k] = loss
            print("%s round %d: %.1f ms / epoch (loss %.6f)" % (k, rnd, (time.time() - t0) / epochs * 1e3, loss), flush=True)
    n = len(loaders["host"].dataset)
    res = {"items_per_epoch": n, "batches_per_epoch": len(loaders["device"]), "epochs_per_timing": epochs,
           "device": stats([s * 1e3 for s in secs["device"]], "ms"), "host": stats([s * 1e3 for s in secs["host"]], "ms"),
           "device_ms_per_epoch": [s * 1e3 for s in secs["device"]], "host_ms_per_epoch": [s * 1e3 for s in secs["host"]]}
    res["last_epoch_loss"] = last
    res["host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
    res.update(beyond_spread(res["device"], res["host"], "device_minus_host"))
    res["device_not_slower_beyond_spread"] = not res["device_minus_host"]["beyond_spread"]
    return res


def timed_launches(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def bench_kernels(hip, dev, n, n_hal, launches, reps):
    g = torch.Generator().manual_seed(4)
    ns, nd = 500, 500                                              # the vpc 5 memories of 50 classes
    static = torch.randn(ns, 3, H, W, generator=g).to(dev)
    dynamic = torch.randn(nd, T, 1, H, W, generator=g).to(dev)
    w, b = (torch.randn(n_hal, 3, 4, 3, 3, 3, generator=g) * 0.2).to(dev), torch.randn(n_hal, 3, generator=g).to(dev)
    sidx = torch.randint(0, ns, (n,), generator=g).to(dev)
    didx = torch.randint(0, nd, (n,), generator=g).to(dev)
    hidx = torch.randint(0, n_hal, (n,), generator=g).to(torch.int32).to(dev)
    out = torch.empty((n, T, 3, H, W), dtype=torch.float32, device=dev)
    st = hip.stream_ptr(dev)

    def multi():
        hip.run("vd_hallucinator_fwd_multi", hip.ptr(static), hip.ptr(dynamic), hip.ptr(sidx), hip.ptr(didx), hip.ptr(hidx),
                hip.ptr(w), hip.ptr(b), n_hal, n, T, H, W, hip.ptr(out), st)

    def single():
        hip.run("vd_hallucinator_fwd", hip.ptr(static), hip.ptr(dynamic), hip.ptr(sidx), hip.ptr(didx), hip.ptr(w), hip.ptr(b), n,
                T, H, W, hip.ptr(out), st)
    legs = {"vd_hallucinator_fwd": single, "vd_hallucinator_fwd_multi": multi}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():                                 # alternated within every repetition
            times[k].append(timed_launches(fn, launches))
    byt = n * (3 + T + 3 * T) * H * W * 4
    res = {}
    for k, v in times.items():
        r = stats(v, "ms")
        r.update({"bytes": byt, "GBps": byt / (r["median_ms"] * 1e-3) / 1e9, "GBps_min": byt / (r["max_ms"] * 1e-3) / 1e9,
                  "GBps_max": byt / (r["min_ms"] * 1e-3) / 1e9, "share_of_hbm_peak": byt / (r["median_ms"] * 1e-3) / HBM_PEAK})
        res[k] = r
    res["multi_over_single_time"] = res["vd_hallucinator_fwd_multi"]["median_ms"] / res["vd_hallucinator_fwd"]["median_ms"]
    res.update(beyond_spread(res["vd_hallucinator_fwd_multi"], res["vd_hallucinator_fwd"], "multi_minus_single"))
    res["multi_not_below_single_beyond_spread"] = not res["multi_minus_single"]["beyond_spread"]
    res["_shape"] = {"n": n, "T": T, "H": H, "W": W, "n_hal": n_hal, "launches_per_rep": launches}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--n_hal", type=int, default=1, help="hallucinators of the epoch legs (the reference's default)")
    ap.add_argument("--batch_train", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel_clips", type=int, default=250)
    ap.add_argument("--kernel_n_hal", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "multistatic_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multistatic: needs the GPU (nothing here is a CPU measurement)")
    from video_distillation_amd import hip, utils
    dev = torch.device("cuda:0")
    doc = {"_source": {"tool": "tools/bench_multistatic.py", "kernel_sources_sha256_16": hip.sources_hash(),
                       "device": torch.cuda.get_device_name(dev), "geometry": [T, H, W],
                       "args": {k: v for k, v in vars(a).items() if k != "out"}}, "epochs": {}}
    for name, (spc, dpc) in WORKLOADS.items():
        print("workload %s" % name, flush=True)
        doc["epochs"][name] = bench_epochs(utils, dev, a.classes, spc, dpc, a.n_hal, a.batch_train, a.epochs, a.rounds)
        torch.cuda.empty_cache()
    doc["kernel"] = bench_kernels(hip, dev, a.kernel_clips, a.kernel_n_hal, a.launches, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
