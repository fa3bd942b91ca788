#!/usr/bin/env python3
"""The kernel ridge predictor (nfr.nfr_pred, csrc/nfr.hip) at the shapes a FRePo run has: one JSON line.

Shapes (n, m, d, C), m = the FRePo script's 512-clip batch: (50, 512, 2048, 50) is ipc 1 and (250, 512, 2048, 50) ipc 5 at
112x112x16, (400, 512, 256, 400) is K400 at 64x64x8.  Features relu(randn), labels and targets randn, reg 1e-6.  Per shape, the
median over ``--rounds`` windows of ``--inner`` iterations each, device events around a window, every variant warmed up first and
the variants alternated window by window in one process:
  * ``op_ms``        : ``nfr_pred`` + the reference's loss line + ``backward()`` (what a trainer calls: the autograd Function,
                       its allocations, the fp32 roundings);
  * ``op_abi_ms``    : ``vdn_nfr_forward`` + ``vdn_nfr_backward`` alone, buffers allocated once (``op_abi_fwd_ms`` /
                       ``op_abi_bwd_ms``: each direction in a window of its own);
  * ``torch64_ms`` / ``torch32_ms``: the torch expressions of distill_s2d.py:133-136 with autograd on the same device in fp64 /
                       fp32, the same loss line and ``backward()``; the error text instead when this torch build cannot run
                       ``torch.linalg.solve`` on the device.
``kernels``: VGPRs, AGPRs, LDS, scratch and occupancy of every kernel of csrc/nfr.hip as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; dynamic LDS is not in that figure), when a compiler is there.

    python tools/bench_nfr.py [--rounds 7] [--inner 20] [--out profiles/nfr_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

SHAPES = [("ipc1", 50, 512, 2048, 50), ("ipc5", 250, 512, 2048, 50), ("k400_64x64x8", 400, 512, 256, 400)]


def kernel_resources():
    """{kernel: {vgprs, agprs, sgprs, scratch_bytes_per_lane, occupancy_waves_per_simd, static_lds_bytes}} of csrc/nfr.hip, or
    the reason there is none."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "video_distillation_amd", "csrc", "nfr.hip")
    with tempfile.TemporaryDirectory() as tmp:
        try:
            p = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-fPIC", "-c", src, "-o", os.path.join(tmp, "nfr.o"),
                                "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        except OSError as e:
            return {"error": str(e)}
    if p.returncode != 0:
        return {"error": p.stderr[-400:]}
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "static_lds_bytes"}
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            short = re.search(r"nfr_[a-z]+_kernel", mangled).group(0)
            flags = re.search(r"kernelIL(b[01](?:ELb[01])*)E", mangled)
            name = short + ("<%s>" % ",".join(flags.group(1).replace("ELb", " ").replace("b", "").split()) if flags else "")
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def loss_line(pred, y):
    return torch.nn.functional.mse_loss(pred, y, reduction='none').sum(-1).mean(0)


def torch_expression(fs, ys, ft, y_tar, reg):
    kss = torch.mm(fs, fs.t())
    kts = torch.mm(ft, fs.t())
    kss_reg = kss + abs(reg) * torch.trace(kss) * torch.eye(kss.shape[0], device=kss.device, dtype=kss.dtype) / kss.shape[0]
    pred = torch.mm(kts, torch.linalg.solve(kss_reg, ys))
    loss_line(pred, y_tar).backward()
    return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from video_distillation_amd import hip, nfr
    assert torch.cuda.is_available(), "bench_nfr.py measures on the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    reg = 1e-6
    rec = {"reg": reg, "rounds": a.rounds, "inner": a.inner, "shapes": {}, "sources": hip.loaded_stamp(),
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__}

    def window(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.inner

    lib = hip.lib()
    for tag, n, m, d, C in SHAPES:
        g = torch.Generator().manual_seed(n + m + d + C)
        fs32 = torch.relu(torch.randn(n, d, generator=g)).to(dev)
        ys32 = torch.randn(n, C, generator=g).to(dev)
        ft32 = torch.relu(torch.randn(m, d, generator=g)).to(dev)
        yt32 = torch.randn(m, C, generator=g).to(dev)
        R32 = torch.randn(m, C, generator=g).to(dev)

        def op():
            fs, ys = fs32.detach().requires_grad_(True), ys32.detach().requires_grad_(True)
            loss_line(nfr.nfr_pred(fs, ys, ft32, reg), yt32).backward()
            return fs.grad

        ws = torch.empty(lib.vdn_nfr_workspace_bytes(n, m, d, C) // 8, dtype=torch.float64, device=dev)
        pred = torch.empty(m, C, dtype=torch.float64, device=dev)
        g_fs = torch.empty(n, d, dtype=torch.float64, device=dev)
        g_ys = torch.empty(n, C, dtype=torch.float64, device=dev)
        st = hip.stream_ptr(dev)

        def abi_fwd():
            hip.run("vdn_nfr_forward", hip.ptr(fs32), hip.ptr(ys32), hip.ptr(ft32), n, m, d, C, reg, hip.ptr(ws), hip.ptr(pred), st)

        def abi_bwd():
            hip.run("vdn_nfr_backward", hip.ptr(fs32), hip.ptr(ft32), hip.ptr(R32), n, m, d, C, reg, hip.ptr(ws), hip.ptr(g_fs), hip.ptr(g_ys), st)

        def abi():
            abi_fwd()
            abi_bwd()

        def torch_variant(dtype):
            ft, yt = ft32.to(dtype), yt32.to(dtype)

            def run():
                fs, ys = fs32.detach().to(dtype).requires_grad_(True), ys32.detach().to(dtype).requires_grad_(True)
                torch_expression(fs, ys, ft, yt, reg)
                return fs.grad
            return run

        variants = {"op_ms": op, "op_abi_ms": abi, "op_abi_fwd_ms": abi_fwd, "op_abi_bwd_ms": abi_bwd}
        entry = {"n": n, "m": m, "d": d, "C": C}
        for name, dtype in (("torch64_ms", torch.float64), ("torch32_ms", torch.float32)):
            fn = torch_variant(dtype)
            try:
                fn()
                torch.cuda.synchronize()
                variants[name] = fn
            except Exception as e:          # (this torch build cannot run the expression on the device: recorded, not timed)
                entry[name] = "not run: %s: %s" % (type(e).__name__, str(e)[:200])
        for fn in variants.values():          # warm-up of every variant at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(a.rounds):          # alternated window by window
            for name, fn in variants.items():
                times[name].append(window(fn))
        for name, ts in times.items():
            entry[name] = float(np.median(ts))
            entry[name.replace("_ms", "_spread_ms")] = [float(min(ts)), float(max(ts))]
        # the gradient the timed op computes against the fp64 torch expression, at this shape
        if "torch64_ms" in variants:
            entry["g_feat_syn_rel_l2_to_torch64"] = float((op().double() - variants["torch64_ms"]()).norm() / variants["torch64_ms"]().norm())
            if "torch32_ms" in variants:
                entry["torch32_g_feat_syn_rel_l2_to_torch64"] = float((variants["torch32_ms"]().double() - variants["torch64_ms"]()).norm()
                                                                      / variants["torch64_ms"]().norm())
        rec["shapes"][tag] = entry
    rec["kernels"] = kernel_resources()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
