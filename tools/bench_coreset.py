#!/usr/bin/env python3
"""Coreset selection at UCF50 shape: one JSON line.

50 classes x 93 clips of 112x112x16 (a ``templates`` synthetic pool, distill.RealPool.synthetic), D = 2048.  Measured:
  * ``embed_ms``: f16x3 features of all 4 650 clips (coreset.class_features, exact weights);
  * ``select_ms[method][ipc]``: one ``coreset.select`` call -- the means + centred Gram launch and the selection launch of all
    50 classes -- for herding and k-center at ipc 1, 10, 50 (median of ``--reps``, device events; the split between the two
    kernels comes from a ``rocprofv3 --kernel-trace --stats`` run of this tool);
  * ``torch_loop_ms[method][ipc]``: for comparison only, the reference's per-step loop (distill_coreset.py:72-105, one
    ``.item()`` per pick) restated with torch ops on the same device features -- herding as written there, k-center as the
    greedy farthest-point loop it intends.

    python tools/bench_coreset.py [--reps 5] [--out profiles/coreset_bench.json]
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


def torch_loop(feats, counts, offsets, ipc, method):
    picks = []
    for n, o in zip(counts, offsets):
        f = feats[o:o + n]
        mean = torch.mean(f, dim=0, keepdim=True)
        if method == "herding":
            sel, left = [], list(range(n))
            for i in range(ipc):
                det = mean * (i + 1) - torch.sum(f[sel], dim=0) if sel else mean * (i + 1)
                j = torch.argmin(torch.norm(det - f[left], dim=1)).item()
                sel.append(left.pop(j))
        else:
            sel = [torch.argmin(torch.norm(f - mean, dim=1)).item()]
            for _ in range(ipc - 1):
                d = torch.cdist(f, f[sel]).min(dim=1).values
                sel.append(torch.argmax(d).item())
        picks.append(sel)
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--per_class", type=int, default=93)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from video_distillation_amd import coreset, distill, hip, plan, utils
    dev = torch.device("cuda:0")
    geo = plan.NetGeometry(16, 112, 112)
    C = a.classes
    pool = distill.RealPool.synthetic(C, list(range(C)), a.per_class, geo, dev, kind="templates")
    net = utils.get_network('ConvNet3D', 3, C, (112, 112), frames=16, dist=False).to(dev)
    for p in net.parameters():
        p.requires_grad = False
    classes = list(range(C))

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        r = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), r

    coreset.class_features(net, pool, classes)          # warm-up (engine planning, weight packing)
    embed = [timed(lambda: coreset.class_features(net, pool, classes))[0] for _ in range(a.reps)]
    feats, counts, offsets = coreset.class_features(net, pool, classes)
    rec = {"shape": {"classes": C, "per_class": a.per_class, "frames": 16, "im_size": 112, "dim": int(feats.shape[1])},
           "embed_ms": float(np.median(embed)), "embed_clips": int(feats.shape[0]), "select_ms": {}, "torch_loop_ms": {},
           "picks_equal_torch_loop": {}, "sources": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev)}
    for method in ("herding", "k-center"):
        rec["select_ms"][method], rec["torch_loop_ms"][method], rec["picks_equal_torch_loop"][method] = {}, {}, {}
        for ipc in (1, 10, 50):
            coreset.select(feats, counts, offsets, ipc, method)
            ts = [timed(lambda: coreset.select(feats, counts, offsets, ipc, method))[0] for _ in range(a.reps)]
            rec["select_ms"][method][str(ipc)] = float(np.median(ts))
            got = coreset.select(feats, counts, offsets, ipc, method).view(C, ipc).cpu()
            t0 = time.perf_counter()
            ref = torch_loop(feats, counts, offsets, ipc, method)
            torch.cuda.synchronize()
            rec["torch_loop_ms"][method][str(ipc)] = (time.perf_counter() - t0) * 1e3
            # (the torch loop decides in fp32: a differing class is a near-tie of that arithmetic, not counted as an error here)
            rec["picks_equal_torch_loop"][method][str(ipc)] = int(sum(
                (got[c] - offsets[c]).tolist() == ref[c] for c in range(C)))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
