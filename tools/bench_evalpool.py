#!/usr/bin/env python3
"""evalpool.evaluate_pool on ONE GPU at config-2 shapes: the per-network train and test times DESIGN section 6 derives the
expected N-rank evaluation time from, and the vd_eval_stats kernel time.

50 synthetic clips (C = 50, ipc 1) of 112x112x16, 501 training epochs in one batch of 50, 200 test clips in batches of 64,
three passes; randn data (the times do not depend on the values).  The first network of a process also pays for planning
and loading the training programs, so ``--num_eval`` 3 and the LAST network's times are the ones to read.

    python tools/bench_evalpool.py --out profiles/evalpool_1gpu.json [--trace <kernel_trace.csv>]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o evalstats -- python tools/bench_evalpool.py --kernel-only

``--kernel-only`` launches vd_eval_stats 30 times at (B, K) = (64, 50) and 30 times at (256, 400) and nothing else; ``--trace``
reads the kernel trace of such a run and adds the per-shape median durations to the JSON.  VD_DETERMINISTIC=1 times the ordered
training step (what bench.py's eval leg runs).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

KERNEL_SHAPES = ((64, 50), (256, 400))
KERNEL_REPS = 30


def kernel_loop():
    from video_distillation_amd import hip
    for B, K in KERNEL_SHAPES:
        z = torch.randn(B, K, device="cuda")
        y = torch.randint(0, K, (B,), device="cuda")
        rec = hip.eval_stats_record(K, "cuda")
        for _ in range(KERNEL_REPS):
            hip.eval_stats(z, y, rec)
        torch.cuda.synchronize()
        assert float(rec[0]) == B * KERNEL_REPS


def kernel_times(trace):
    rows = [r for r in csv.DictReader(open(trace)) if "eval_stats_kernel" in r["Kernel_Name"]]
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    assert len(ns) == KERNEL_REPS * len(KERNEL_SHAPES), len(ns)
    return {"%dx%d" % s: {"median_us": statistics.median(ns[k * KERNEL_REPS:(k + 1) * KERNEL_REPS]) / 1e3,
                          "min_us": min(ns[k * KERNEL_REPS:(k + 1) * KERNEL_REPS]) / 1e3,
                          "max_us": max(ns[k * KERNEL_REPS:(k + 1) * KERNEL_REPS]) / 1e3, "launches": KERNEL_REPS}
            for k, s in enumerate(KERNEL_SHAPES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_eval", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        kernel_loop()
        return
    from video_distillation_amd import evalpool, hip
    C, T, S = 50, 16, 112
    g = torch.Generator().manual_seed(1)
    syn = torch.randn(C, T, 3, S, S, generator=g).cuda()
    labels = torch.arange(C).cuda()
    test_x = torch.randn(4 * C, T, 3, S, S, generator=g).cuda()
    test_y = torch.arange(C).repeat_interleave(4).cuda()
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test_x, test_y), batch_size=64, shuffle=False)
    eargs = types.SimpleNamespace(device="cuda:0", lr_net=0.01, epoch_eval_train=a.epochs, batch_train=256, model="ConvNet3D", eval_mode="SS")
    t0 = time.time()
    got = evalpool.evaluate_pool(None, syn, labels, loader, eargs, num_eval=a.num_eval, seed=5, num_classes=C)
    out = {"what": "evalpool.evaluate_pool, world 1, C = 50 ipc 1 112x112x16, %d epochs, 200 test clips x 3 passes" % (a.epochs + 1),
           "device": torch.cuda.get_device_name(0), "sources_hash": hip.sources_hash(), "library_stamp": hip.loaded_stamp(),
           "deterministic": hip.deterministic(), "num_eval": a.num_eval, "wall_s": time.time() - t0, "times": got["times"],
           "train_s_per_network": got["times"]["train_s"][-1], "test_pass_s": got["times"]["test_pass_s"][-1][-1]}
    if a.trace:
        out["vd_eval_stats_kernel"] = dict(kernel_times(a.trace), source="rocprofv3 --kernel-trace --stats, tools/bench_evalpool.py --kernel-only")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
