#!/usr/bin/env python3
"""run_frepo's driver loop -- real batch, ``FRePoTrainer.step``, the log cadence -- with ``--train_videos host`` against
``preload``, on one MI355X: one JSON line (and ``--out``).

Per shape (64x64x8 and configuration 2's 112x112x16) a data file of 1024 noise clips in 50 classes is held in memory as
``run_mtt.load_data`` holds a ``--data_file``; C = 50, ipc 1, ``--memories images``, no evaluation.  Three loops, each warmed up,
alternated window by window in one process, ``--rounds`` (at least 7) windows of 10 iterations, wall time around a window that
ends with the loop's own flush (a device synchronisation and the float reads of the ten pending losses):

  * ``host_ms``      the parent's loop: ``run_frepo.real_batches`` (a host DataLoader over the blob: a gather of 512 clips and
                     their fp32 host-to-device copy per iteration) -- the yardstick;
  * ``preload_ms``   ``run_frepo.device_batches`` over the clips in HBM: one ``index_select`` per iteration;
  * ``floor_ms``     ``FRePoTrainer.step`` on one fixed pair of device tensors: what a loop cannot go below.

Median and [min, max] of the windows, per iteration.  No figure is promised.

``ranks3``: three ranks on this ONE device over gloo (children of this tool), 64x64x8, ``frepo.TargetExchange`` with its phase
clock on: per rank the seconds per iteration in the embedding of its slice, the feature gather and the weight broadcast.  Three
processes share one GPU and the exchange goes through host memory, so these are per-rank times of the protocol's phases, NOT a
speed-up and not what xGMI would give.  ``exchange_bytes`` are the sizes of the per-step messages.  Not run: more than one GPU.

    python tools/bench_frepo_driver.py [--rounds 7] [--shapes 64x64x8,112x112x16] [--no_ranks3] [--out profiles/frepo_driver_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np              # noqa: E402
import torch                    # noqa: E402

C, N_REAL, WINDOW, POOL = 50, 1024, 10, 10


def build(hw, frames, dev, seed):
    """-> a trainer of the run's shape: C synthetic clips, a pool of POOL networks, from explicit seeds."""
    from video_distillation_amd import evalpool, frepo
    g = torch.Generator().manual_seed(seed)
    syn = frepo.SynData(torch.randn(C, frames, 3, hw, hw, generator=g), frepo.soft_labels(torch.arange(C), C, frepo.y_scale(C))).to(dev)
    opt, sch = frepo.syn_optimizer(syn, 1e2, 1e-3, 10000)
    make = evalpool.convnet3d_factory(C, (hw, hw), frames)
    evalpool.seed_all(seed)
    pools = frepo.build_pool(lambda: make(0), 1e-3, 100, POOL, dev)
    return frepo.FRePoTrainer(syn, pools, opt, sch)


def loop(trainer, batches, dev):
    """One window of the driver's loop body: next batch, step, pending; the flush at the end -> seconds."""
    pending = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(WINDOW):
        got = next(batches)
        x, y = got[-2], got[-1]
        pending.append(trainer.step(x.to(dev), y.to(dev)))
    torch.cuda.synchronize(dev)
    for loss, ln, lb in pending:
        float(loss), float(ln), float(lb)
    return time.perf_counter() - t0


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def one_shape(hw, frames, rounds, dev):
    from video_distillation_amd import frepo, run_frepo
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(N_REAL, frames, 3, hw, hw, generator=g)
    labels = (torch.arange(N_REAL) % C).tolist()
    clips_of = lambda idx: clips[torch.as_tensor(idx, dtype=torch.int64)].float()          # run_mtt.load_data's, for a data file
    store = run_frepo.RealStore(C, clips.to(dev), labels)
    fixed = (clips[:run_frepo.REAL_BATCH].to(dev), frepo.soft_labels(torch.as_tensor(labels[:run_frepo.REAL_BATCH]), C).to(dev))

    def same():
        while True:
            yield fixed
    variants = {"host": (build(hw, frames, dev, 3), run_frepo.real_batches(clips_of, labels, C, 0)),
                "preload": (build(hw, frames, dev, 3), run_frepo.device_batches(store, 0)),
                "floor": (build(hw, frames, dev, 3), same())}
    times = {k: [] for k in variants}
    for k, (tr, it) in variants.items():          # warm-up: plans, engines, allocator
        loop(tr, it, dev)
    for _ in range(rounds):
        for k, (tr, it) in variants.items():
            times[k].append(loop(tr, it, dev) / WINDOW * 1e3)
    d = int(variants["floor"][0].pools[0].model.embed_exact(fixed[0][:1]).shape[1])
    params = sum(p.numel() for p in variants["floor"][0].pools[0].model.parameters())
    return {"host_ms": stats(times["host"]), "preload_ms": stats(times["preload"]), "floor_ms": stats(times["floor"]),
            "batch_bytes_fp32": run_frepo.REAL_BATCH * frames * 3 * hw * hw * 4,
            "exchange_bytes": {"table_int64": (frepo.HEADER + run_frepo.REAL_BATCH) * 8, "features_fp32": run_frepo.REAL_BATCH * d * 4,
                               "feature_width": d, "weights_fp32": (1 + params) * 4, "parameters": params}}


def rank_child(hw, frames, iters):
    """One rank of the three on device 0: TargetExchange with its clock on; rank 0 prints the per-rank seconds per iteration."""
    import torch.distributed as dist
    from video_distillation_amd import evalpool, frepo, run_frepo
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(1)
    clips = torch.randn(N_REAL, frames, 3, hw, hw, generator=g).to(dev)
    labels = torch.arange(N_REAL) % C
    store = run_frepo.RealStore(C, clips, labels.tolist())
    make = evalpool.convnet3d_factory(C, (hw, hw), frames)
    if rank == 0:
        tr = build(hw, frames, dev, 3)
        ex = frepo.TargetExchange(lambda i: tr.pools[i].model, store.clips, rank, world, dev, run_frepo.REAL_BATCH)
    else:
        shells = [make(i).to(dev) for i in range(POOL)]
        ex = frepo.TargetExchange(lambda i: shells[i], store.clips, rank, world, dev, run_frepo.REAL_BATCH)
    ex.sync_all_weights(POOL)
    stream = frepo.real_batch_indices(N_REAL, run_frepo.REAL_BATCH, torch.Generator().manual_seed(0))
    for it in range(2 + iters):
        if it == 2:
            ex.clock = {}
            t0 = time.perf_counter()
        if rank == 0:
            rows = store.table(next(stream))
            idx = tr.draw_pool_index()
            y = store.labels(rows)
            ex.lead(idx, rows, lambda feat: tr.step(None, y, feat_tar=feat, idx=idx), it)
        else:
            ex.follow(it)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    mine = torch.tensor([ex.clock.get("embed", 0.0), ex.clock.get("gather", 0.0), ex.clock.get("weights", 0.0), total], dtype=torch.float64) / iters
    every = [torch.zeros(4, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(every, mine)
    if rank == 0:
        ex.lead_stop()
        print("RANKS3 " + json.dumps({"world": world, "iterations": iters, "shape": "%dx%dx%d" % (hw, hw, frames),
                                      "per_rank_ms": [{"embed": round(float(v[0]) * 1e3, 3), "gather": round(float(v[1]) * 1e3, 3),
                                                       "weights": round(float(v[2]) * 1e3, 3), "iteration": round(float(v[3]) * 1e3, 3)}
                                                      for v in every]}), flush=True)
    else:
        ex.follow()
    dist.destroy_process_group()


def ranks3(hw, frames, iters=10, timeout=300):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="3", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--rank_child", "%dx%dx%d" % (hw, hw, frames), "--iters", str(iters)]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(3)]
    try:
        outs = [p.communicate(timeout=timeout) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (_, err) in zip(procs, outs):
        if p.returncode != 0:
            raise RuntimeError("a rank of the three-rank run failed: %s" % err[-2000:])
    line = [l for l in outs[0][0].splitlines() if l.startswith("RANKS3 ")][0]
    return json.loads(line[len("RANKS3 "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", type=str, default="64x64x8,112x112x16")
    ap.add_argument("--no_ranks3", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--rank_child", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=10, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frepo_driver.py measures on the GPU: there is no CPU timing"
    if a.rank_child:
        hw, _, frames = (int(v) for v in a.rank_child.split("x"))
        return rank_child(hw, frames, a.iters)
    if a.rounds < 7:
        ap.error("--rounds: at least 7 windows")
    from video_distillation_amd import hip
    dev = torch.device("cuda:0")
    rec = {"rounds": a.rounds, "window": WINDOW, "C": C, "real_clips": N_REAL, "pool": POOL, "shapes": {}, "sources": hip.loaded_stamp(),
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "not_run": "more than one GPU"}
    for shape in a.shapes.split(","):
        hw, _, frames = (int(v) for v in shape.split("x"))
        rec["shapes"][shape] = one_shape(hw, frames, a.rounds, dev)
        torch.cuda.empty_cache()
    if not a.no_ranks3:
        rec["ranks3_one_device"] = ranks3(64, 8)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
