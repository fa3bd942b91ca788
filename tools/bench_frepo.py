#!/usr/bin/env python3
"""FRePo's two hot pieces at 64x64x8 and at configuration 2's shape (112x112x16): one JSON line.

  * the pool step: ``ConvNet3D.hip_regress_step`` (50 clips, C = 50, Adam) against the route that existed before it --
    ``net(x)``, ``nn.MSELoss()``, ``backward()``, ``torch.optim.Adam.step()`` on the same device, i.e. the twice-differentiable
    autograd Functions followed by torch's own optimiser (``pool_hip_ms`` / ``pool_fallback_ms``);
  * one whole ``FRePoTrainer.step`` at ipc 1 (50 synthetic clips, 512 targets, pool of 2, ``--memories images``):
    ``trainer_step_ms``.

Per shape the median over ``--rounds`` (at least 7) windows of ``--inner`` iterations each, device events around a window, every
variant warmed up first and the variants alternated window by window in one process; ``*_spread_ms`` is [min, max] of the
windows.  The figure of merit: ``pool_hip_ms`` is not above ``pool_fallback_ms`` by more than the spread of the fallback's own
windows (``pool_hip_not_slower``).  Per-kernel times belong to a kernel-trace run of its own, not to this tool.

    python tools/bench_frepo.py [--rounds 7] [--inner 10] [--shapes 64x64x8,112x112x16] [--out profiles/frepo_bench.json]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

C, N_SYN, M_TAR = 50, 50, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shapes", type=str, default="64x64x8,112x112x16")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7 windows")
    from video_distillation_amd import frepo, hip, networks
    assert torch.cuda.is_available(), "bench_frepo.py measures on the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    rec = {"rounds": a.rounds, "inner": a.inner, "C": C, "pool_clips": N_SYN, "targets": M_TAR, "shapes": {},
           "sources": hip.loaded_stamp(), "device": torch.cuda.get_device_name(dev), "torch": torch.__version__}

    def window(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.inner

    def make_net(seed, hw, frames):
        torch.manual_seed(seed)
        return networks.ConvNet3D(3, C, 128, 3, 'relu', 'none', 'maxpooling', frames, (hw, hw)).to(dev).train()

    for shape in a.shapes.split(","):
        H, W, T = (int(v) for v in shape.split("x"))
        random.seed(0); np.random.seed(0)
        g = torch.Generator().manual_seed(H + T)
        x = torch.randn(N_SYN, T, 3, H, W, generator=g).to(dev)
        y = frepo.soft_labels(torch.arange(N_SYN) % C, C, frepo.y_scale(C)).to(dev)
        mse = torch.nn.MSELoss()
        net_hip, net_ref = make_net(1, H, T), make_net(1, H, T)
        opt_hip = torch.optim.Adam(net_hip.parameters(), lr=1e-3, betas=(0.9, 0.999))
        opt_ref = torch.optim.Adam(net_ref.parameters(), lr=1e-3, betas=(0.9, 0.999))
        assert net_hip.hip_regress_trainable(x, opt_hip, mse)

        def pool_hip():
            net_hip.hip_regress_step(x, y, opt_hip)

        def pool_fallback():
            opt_ref.zero_grad(set_to_none=True)
            mse(net_ref(x), y).backward()
            opt_ref.step()

        syn = frepo.SynData(torch.randn(N_SYN, T, 3, H, W, generator=g), y.cpu().clone(), learn_label=False).to(dev)
        synopt, synsch = frepo.syn_optimizer(syn, 1e2, 1e-3, 10000)
        count = [0]

        def get_model():
            count[0] += 1
            return make_net(10 + count[0], H, T)
        # (max_online_updates beyond the run: no reset -- a reset builds a network -- falls into a window)
        trainer = frepo.FRePoTrainer(syn, frepo.build_pool(get_model, 1e-3, 1 << 30, 2, dev), synopt, synsch)
        x_t = torch.randn(M_TAR, T, 3, H, W, generator=g).to(dev)
        y_t = frepo.soft_labels(torch.arange(M_TAR) % C, C).to(dev)

        def trainer_step():
            trainer.step(x_t, y_t)

        variants = {"pool_hip_ms": pool_hip, "pool_fallback_ms": pool_fallback, "trainer_step_ms": trainer_step}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(a.rounds):          # alternated window by window
            for name, fn in variants.items():
                times[name].append(window(fn))
        entry = {"H": H, "W": W, "T": T}
        for name, ts in times.items():
            entry[name] = float(np.median(ts))
            entry[name.replace("_ms", "_spread_ms")] = [float(min(ts)), float(max(ts))]
        lo, hi = entry["pool_fallback_spread_ms"]
        entry["pool_hip_not_slower"] = bool(entry["pool_hip_ms"] <= entry["pool_fallback_ms"] + (hi - lo))
        entry["pool_speedup"] = entry["pool_fallback_ms"] / entry["pool_hip_ms"]
        rec["shapes"][shape] = entry
        del trainer, syn, net_hip, net_ref, x_t
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
