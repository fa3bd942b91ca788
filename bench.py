#!/usr/bin/env python3
"""Headline benchmark: distillation steps/s on N MI355X, for the five BASELINE.json configurations.

    python bench.py                                   # config 2: DM, miniUCF101 shape, IPC=1, 112x112x16 (the headline)
    python bench.py --full                            # the same + CPU baseline, eval, sustained and extra legs, measured peak
    python bench.py --method s2d                      # config 3: DM + static/dynamic memories
    python bench.py --method dc  --classes 51 --ipc 5                       # config 4: gradient matching
    python bench.py --method mtt --classes 400 --frames 8 --size 64         # config 5: MTT + static/dynamic memories
    python bench.py --frames 8 --size 64              # config 1's shape (the reference's CPU-runnable case) on the GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8 --steps 10 --warmup 3

One step = one iteration of the reference's loop body (DM: distill_baseline.py:334-355; s2d: distill_s2d_ms.py:393-438;
MTT+Ours: distill_s2d_ms.py:189-300; DC: the upstream loop around match_loss, utils.py:655).  Synthetic data (no dataset
ships): randn clips standardised per channel, generated on the device; inputs resident in HBM before the timed region.

Rank 0 prints ONE JSON line (contract in the task description).  `value` = steps / wall time of the timed region
(barrier + synchronize on both sides, max over ranks); `ms_per_step_median` is the median of the per-step intervals
between HIP events recorded behind each step's last kernel.  A plain run does only what that line needs: set-up, warm-up,
the timed steps, --dump-outputs, and the figures taken from the timed region itself.  Extra objects:
  roofline      -- DM / s2d: the conv tile program with the largest share of the timed region's GPU time: algorithmic FLOP per
                   launch / mean launch time (HIP events on the launch stream, inside the timed region) against the 2.5 PFLOP/s
                   dense 16-bit MFMA peak; `traffic` = HBM bytes per launch from the committed PMC passes, quoted only while the
                   file's stamp equals the hash of this checkout's kernel sources (else null; see traffic_source);
  per_rank      -- every rank's real clips, own ms per step, wait at the closing barrier, real-side ms, exchange ms (N > 1:
                   what tells an unbalanced partition from a slow collective from a slow device).
With --full, whatever takes runs of its own after the timed region as well:
  roofline      -- `peak_measured` = this box's MFMA-saturating microbenchmark (vd_mfma_peak); DM: `alone` = the real side
                   launched with nothing else on the chip; DC / MTT: the whole object, from one extra profiled step;
  cpu_baseline  -- the CPU oracle (torch fp32 ops == what the reference runs on a CPU) timed on this host's cores on a
                   bounded sample of the same workload, extrapolated to steps/s; rank 0, N=1 only;
  eval          -- evaluate_synset on the synthetic clips (HIP train step + HIP inference): a reproducible SMOKE of that path, not
                   an accuracy metric (accuracy parity: fixture G16, tests/test_gpu_eval_parity.py);
  sustained     -- the same step loop run for --sustain-seconds: steps/s once clocks have settled;
  parity_mode, fast_mode, exchange_*  -- DM: short timed legs of the same workload in other precision / exchange modes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_TFLOPS = 2500.0        # dense 16-bit MFMA, MI355X_MICROARCH.md


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--ipc", type=int, default=1)
    ap.add_argument("--batch-real", type=int, default=64)
    ap.add_argument("--pool-per-class", type=int, default=None, help="real clips per class (default 93; 1 for --method mtt)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--prec-real", default=os.environ.get("VD_PREC_REAL", "f16"))
    ap.add_argument("--prec-syn", default=os.environ.get("VD_PREC_SYN", "f16x3"))
    ap.add_argument("--prec-bwd", default=os.environ.get("VD_PREC_BWD", "f16x3"),
                    help="operand precision of the input-gradient passes (f16x3: hi+lo pairs; f16: single pass; both with per-layer "
                         "power-of-two scaling)")
    ap.add_argument("--real-last", default=None, choices=["x1", "x3", "c8"],
                    help="real side's last conv level: x3 = hi+lo operand pairs (default, VD_REAL_LAST), c8 = hi+lo with the two correction "
                         "products on the fp8 matrix instruction (two MFMA-equivalents per product), x1 = single pass like the others")
    ap.add_argument("--chunk", type=int, default=3200, help="real clips per launch (all of a single-GPU step by default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-classes", type=int, default=10, help="dm/s2d: class terms timed for the CPU baseline")
    ap.add_argument("--shard", default="auto", choices=["auto", "class", "batch", "hybrid"],
                    help="multi-GPU decomposition of dm: whole classes per rank (uneven blocks, no data-path collective); 1/N of every "
                         "class's real batch per rank (+ all-reduce of the per-class feature sums); hybrid = equal blocks of whole "
                         "classes + the left-over classes' batches split N ways (+ all-reduce of THEIR sums, 8 KB per class); "
                         "auto = hybrid when it balances better than class blocks, else class")
    ap.add_argument("--exchange", default="owner", choices=["owner", "allreduce"],
                    help="dm: what the timed steps do with the pixel gradients -- owner (default: a rank owns its classes' synthetic clips, "
                         "nothing crosses xGMI) or allreduce (the task's literal 'all-reduce of the matching-loss gradient': the full "
                         "C*ipc-clip gradient tensor, 120 MB at config 2, summed over the ranks through vd_comm_allreduce_f32 = RCCL).  "
                         "With more than one rank the mode that is NOT timed runs as a short extra leg (exchange_allreduce / exchange_owner)")
    ap.add_argument("--exchange-leg", action="store_true", help="dm, --full: run the other exchange mode's short leg even with --no-extra-legs")
    ap.add_argument("--vd-comm", choices=["auto", "on", "off"], default="auto",
                    help="the library's own RCCL communicator (hip.Comm -> vd_comm_*) for the pixel-gradient all-reduce and the `rccl` "
                         "block of the line.  auto: on one rank (where it has been exercised on every GPU test run), OFF on more than "
                         "one -- a SECOND communicator beside torch's, created and used for the first time on N devices, is not "
                         "something a scaling run should depend on: the all-reduce then goes through torch.distributed's group (the "
                         "same RCCL), and `rccl` reports that group.  on: use it at any world size")
    ap.add_argument("--syn-steps", type=int, default=10, help="--method mtt: unrolled student steps (sh/s2d/s2d_MTT_ms_K400.sh)")
    ap.add_argument("--batch-syn", type=int, default=256, help="--method mtt: composed clips per student step")
    ap.add_argument("--mtt-raw", action="store_true", help="--method mtt: raw synthetic clips (distill_baseline.py MTT) instead of "
                                                           "the static/dynamic composition of config 5")
    ap.add_argument("--method", default="dm", choices=["dm", "s2d", "dc", "mtt"])
    ap.add_argument("--pool-kind", default="templates", choices=["templates", "randn"],
                    help="synthetic real pool: class template + noise (learnable: eval top-1 is informative) or plain randn clips "
                         "(SURVEY 8(d); top-1 is chance by construction).  Same value statistics, same timings.")
    ap.add_argument("--pool-noise", type=float, default=1.5, help="--pool-kind templates: noise amplitude next to the template (rms 0.67)")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="dm, --full: skip the two short extra timed legs (parity_mode = all hi+lo pairs, fast_mode = round 2's single-pass mode)")
    ap.add_argument("--seed", type=int, default=0, help="seed of torch's global generators (dropout masks of DC / MTT, loader shuffles)")
    ap.add_argument("--no-alone", action="store_true", help="dm, --full: skip the stand-alone launches of the real side after the timed region "
                    "(roofline.alone); profiling runs use it so that the kernel statistics hold in-step launches only")
    ap.add_argument("--eval-atomic", action="store_true", help="dm: run the eval leg's training steps in the default (fp32-atomic) accumulation "
                    "mode instead of the fixed-order one (then top1_per_seed moves in its last digits from run to run)")
    ap.add_argument("--eval-seeds", type=int, default=5, help="dm: networks (fixed seeds) the eval leg trains; top1 is their mean")
    ap.add_argument("--eval-epochs", type=int, default=500,
                    help="dm, --full: after the timed steps run evaluate_synset on the synthetic clips for this many epochs (0 = skip); 500 "
                         "epochs take ~4 s on the HIP train step (the reference's default is 1000) and fit the 50 clips")
    ap.add_argument("--sustain-seconds", type=float, default=5.0, help="--full: length of the sustained leg (0 = skip)")
    ap.add_argument("--dis-metric", default="ours", choices=["ours", "mse", "cos"], help="match_loss metric of --method dc")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step computed (the global loss and the trainer's learnable "
                         "state, gathered over the ranks) as DIR/<name>.npy: float64 scalars, float32 arrays; an array above "
                         "2**22 elements is written as a fixed seeded sample of its flattened values (same shape -> same positions)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline does not need: the CPU baseline, the eval and sustained legs, "
                         "dm's extra precision and exchange legs, the measured MFMA peak, the stand-alone real side and DC / MTT's "
                         "profiling step (the --no-* switches above then skip single legs).  Without it a run sets up, warms up, "
                         "times the steps, dumps its outputs and prints the line")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
def conv_layer_macs(geo):
    return [d[1] * d[5] * d[6] * d[7] * d[0] * 147 for d in geo.layer_dims()]


def pmc_traffic(name, clips_per_launch):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (separate FETCH_SIZE / WRITE_SIZE
    runs, corrected as MI355X_MICROARCH.md prescribes) over tools/run_real_side.py, i.e. over the very launches of one step of
    THIS benchmark's default configuration (3200 clips per launch, index gather, dithered operand sets, low-plane output).
    Counters cannot be read from inside the timed run (rocprofv3 --pmc serialises the kernels), so the figure is carried in a
    file -- STAMPED with the hash of the kernel sources it was measured on (``hip.sources_hash``): a file whose stamp differs
    from this checkout's sources is refused (traffic null, the reason in ``traffic_source``), as is any other launch size.
    tools/refresh_profiles.sh re-measures the file.  -> (bytes or None, source label)."""
    from video_distillation_amd import hip
    mine = hip.sources_hash()
    for fn in ("r06_pmc_traffic.json", "r05_pmc_traffic.json"):
        path = os.path.join(ROOT, "profiles", fn)
        if not os.path.exists(path):
            continue
        doc = json.load(open(path))
        rec, src = doc.get(name), doc.get("_source", {})
        if not rec:
            continue
        stamp = src.get("kernel_sources_sha256_16")
        if stamp != mine:
            return None, "profiles/%s was measured on other kernel sources (stamp %s, this checkout %s): not quoted; re-measure with " \
                         "tools/refresh_profiles.sh" % (fn, stamp, mine)
        if int(round(clips_per_launch)) != int(rec["clips_per_launch"]):
            return None, "profiles/%s holds %d clips per launch, this run launches %d: not quoted" % (
                fn, rec["clips_per_launch"], int(round(clips_per_launch)))
        return rec["hbm_bytes_per_launch"], "profiles/%s: PMC passes over %s, %d clips per launch = this run's launch shape, kernel sources %s " \
            "= this checkout's (measured, unscaled)" % (fn, src.get("command", "tools/run_real_side.py"), rec["clips_per_launch"], stamp)
    return None, None


def mfma_peak(device):
    """This box's measured dense f16 MFMA rate (TFLOP/s): vd_mfma_peak, best of 3 launches of ~10 ms."""
    from video_distillation_amd import hip
    blocks, iters = 256 * 8, 4000
    out = torch.empty(blocks * 256, dtype=torch.float32, device=device)
    best = 0.0
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.check(hip.lib().vd_mfma_peak(blocks, iters, 0, hip.ptr(out), hip.stream_ptr(device)), "vd_mfma_peak")
        e1.record()
        torch.cuda.synchronize()
        best = max(best, blocks * 4 * iters * 8 * 32768.0 / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    return best


def real_side_alone(trainer, backend, args, macs, it):
    """The real side's three launches with NOTHING else on the chip (same run, after the timed region; 3 repetitions): inside a
    step the synthetic-clip stream's kernels share the CUs with whichever real-side launch is running -- which one they land on is
    a matter of LDS fit and dispatch order, the step time is what counts -- so `roofline.achieved` (in-step, the contract) moves by
    +-10 % between builds with the kernel unchanged.  This is the kernel by itself."""
    from video_distillation_amd import distill, engine
    dev = trainer.image_syn.device
    idx = distill.sample_real_indices(it, trainer.pool.counts, trainer.pool.offsets, args.batch_real, trainer.classes)
    idx_t = torch.as_tensor(idx, device=dev)
    trainer.sync(); torch.cuda.synchronize()
    backend.set_real_weights(backend.new_network(seed=it), trainer._per_class())
    trainer._real_features(idx_t); torch.cuda.synchronize()
    engine.LAUNCH_PROFILE = []
    try:
        for _ in range(3):
            trainer._real_features(idx_t)
        torch.cuda.synchronize()
        prof = engine.LAUNCH_PROFILE
    finally:
        engine.LAUNCH_PROFILE = None
    ms = {}
    for name, prec, flop, e0, e1 in prof:
        ms.setdefault(name, []).append(e0.elapsed_time(e1))
    out = {k + "_ms": sum(v) / len(v) for k, v in ms.items()}
    if "fwd1" in ms:
        clips = len(trainer.classes) * args.batch_real
        t = out["fwd1_ms"] * 1e-3
        out["achieved"] = 2.0 * macs[1] * clips / t / 1e12
        out["frac"] = out["achieved"] / 2500.0
        out["note"] = "level-1 forward launched with no other stream active (TFLOP/s, fraction of the 2.5 PFLOP/s spec peak)"
    return out


def best_threads(fn):
    """Thread count for the CPU baseline: the fastest of a short calibration (all logical CPUs is NOT the fastest on the
    GPU box's 2 x 64-core host: 256 threads ran 10x slower than 32)."""
    ncpu = os.cpu_count() or 1
    best = (None, 1)
    for th in sorted({t for t in (8, 16, 32, 64, 128, ncpu) if t <= ncpu}):
        torch.set_num_threads(th)
        fn()
        tc = time.perf_counter()
        fn()
        tc = time.perf_counter() - tc
        if best[0] is None or tc < best[0]:
            best = (tc, th)
    torch.set_num_threads(best[1])
    return best[1], ncpu


class Harness:
    def __init__(self, args, device, rank, world):
        self.args, self.device, self.rank, self.world = args, device, rank, world
        self.comm = None

    def open_comm(self):
        """An RCCL communicator over the ranks behind the C ABI (hip.Comm -> vd_comm_*), when the process group runs on RCCL
        (backend nccl: one device per rank); None otherwise (one process without a group, or the one-device gloo logic mode)."""
        import torch.distributed as dist
        want = self.args.vd_comm == "on" or (self.args.vd_comm == "auto" and self.world == 1)
        if self.comm is None and want and dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            from video_distillation_amd import hip
            self.comm = hip.Comm(self.rank, self.world)
        return self.comm

    def topology(self, clips_per_step):
        """Proof of the N-rank run for the JSON line (every rank calls): ``ranks_seen`` = an all-reduce of ones over the process
        group; ``clips_per_step`` = every rank's real clips per step (all-gather); ``rccl`` = version and rank count as RCCL
        itself reports them (ncclGetVersion / ncclCommCount of a communicator created over the ranks through vd_comm_*)."""
        import torch.distributed as dist
        rec = {"ranks_seen": 1, "clips_per_step": [int(clips_per_step)], "rccl": None,
               "launched_by": "bench.py spawn_ranks" if os.environ.get("VD_BENCH_SPAWNED") == "1" else
                              ("torch.distributed.run / external launcher" if "WORLD_SIZE" in os.environ else "single process")}
        if dist.is_available() and dist.is_initialized():
            ones = torch.ones(1, device=self.device)
            dist.all_reduce(ones)
            rec["ranks_seen"] = int(ones.item())
            mine = torch.tensor([int(clips_per_step)], device=self.device, dtype=torch.int64)
            parts = [torch.zeros_like(mine) for _ in range(self.world)]
            dist.all_gather(parts, mine)
            rec["clips_per_step"] = [int(p.item()) for p in parts]
            rec["backend"] = dist.get_backend()
            comm = self.open_comm()
            if comm is not None:
                from video_distillation_amd import hip
                v = hip.Comm.version()
                rec["rccl"] = {"version_code": v, "version": None if v is None else "%d.%d.%d" % (v // 10000, v // 100 % 100, v % 100),
                               "nranks": comm.size(), "torch_nccl_version": ".".join(str(x) for x in torch.cuda.nccl.version())}
            elif dist.get_backend() == "nccl":
                rec["rccl"] = {"through": "torch.distributed process group (backend nccl = RCCL); the library's own communicator is off "
                                          "at world > 1 unless --vd-comm on", "nranks": dist.get_world_size(),
                               "torch_nccl_version": ".".join(str(x) for x in torch.cuda.nccl.version())}
            else:
                rec["rccl"] = {"note": "process group on gloo (all ranks share device 0: RCCL refuses two ranks on one device)"}
        return rec

    def barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def run(self, step, sync, mark, profile=True):
        """W untimed + K timed steps; -> (wall seconds [max over ranks], per-step ms list, launch profile).  ``profile``:
        record two HIP events around every tile-program launch INSIDE the timed region (DM / s2d: ~25 launches per step,
        this is where `roofline.achieved` comes from).  The loops that issue thousands of small launches per step (DC, MTT)
        are host-issue sensitive: they are timed with the hook off and profiled in extra untimed steps (``profile_steps``)."""
        from video_distillation_amd import engine
        a = self.args
        for it in range(a.warmup):
            step(it)
        sync()
        self.barrier()
        engine.LAUNCH_PROFILE = [] if profile else None
        marks = [mark()]
        t0 = time.perf_counter()
        losses = []
        for it in range(a.warmup, a.warmup + a.steps):
            losses.append(step(it))
            marks.append(mark())
        sync()
        torch.cuda.synchronize()
        t_own = time.perf_counter() - t0          # this rank's own work of the timed region is done ...
        self.barrier()
        dt = time.perf_counter() - t0             # ... and everybody else's
        prof, engine.LAUNCH_PROFILE = engine.LAUNCH_PROFILE or [], None
        self.rank_diag = {"rank": self.rank, "own_ms_per_step": t_own / a.steps * 1e3, "wait_at_barrier_ms": (dt - t_own) * 1e3}
        if self.world > 1:
            import torch.distributed as dist
            tmax = torch.tensor([dt], device=self.device, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax)
        per_step = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(marks) - 1)]
        return dt, per_step, prof, losses

    def per_rank(self, prof, clips, extra=None):
        """Every rank's view of the timed region, gathered for the JSON line (every rank calls): real clips per step, its own time
        per step (up to its own synchronisation), how long it then waited at the closing barrier (the slowest rank waits ~0), the
        time of its real-side launches per step (HIP events of the launch profile: programs fwd0 / fwd1 / fwd2* in the real side's
        operand format) and, where the step has an exchange, its time per step -- what tells an unbalanced partition from a slow
        collective from a slow device when N > 1 runs for the first time."""
        a = self.args
        from video_distillation_amd import hip
        real = [e0.elapsed_time(e1) for name, prec, flop, e0, e1 in prof
                if name.startswith("fwd") and prec in (hip.PREC[a.prec_real], hip.PREC["f16c8"])]
        rec = dict(getattr(self, "rank_diag", {"rank": self.rank}), clips_per_step=int(clips),
                   real_side_ms_per_step=sum(real) / max(a.steps, 1), device=torch.cuda.get_device_name(self.device))
        rec.update(extra or {})
        out = [rec]
        if self.world > 1:
            import torch.distributed as dist
            out = [None] * self.world
            dist.all_gather_object(out, rec)
        return out

    def profile_steps(self, step, sync, first_it, n=1):
        """``n`` extra untimed steps with the launch hook on, on EVERY rank (a step may contain collectives)."""
        from video_distillation_amd import engine
        sync()
        torch.cuda.synchronize()
        engine.LAUNCH_PROFILE = []
        try:
            for k in range(n):
                step(first_it + k)
            sync()
            torch.cuda.synchronize()
        finally:
            prof, engine.LAUNCH_PROFILE = engine.LAUNCH_PROFILE, None
        return prof

    def sustained(self, step, sync, first_it):
        a = self.args
        if a.sustain_seconds <= 0:
            return None
        self.barrier()
        t0 = time.perf_counter()
        n = 0
        while True:
            for _ in range(max(1, a.steps // 4)):
                step(first_it + n)
                n += 1
            sync()
            torch.cuda.synchronize()
            stop = torch.tensor([1.0 if time.perf_counter() - t0 >= a.sustain_seconds else 0.0], device=self.device)
            if self.world > 1:
                import torch.distributed as dist
                dist.all_reduce(stop, op=dist.ReduceOp.MAX)
            if float(stop) > 0:
                break
        self.barrier()
        dt = time.perf_counter() - t0
        return {"seconds": dt, "steps": n, "value": n / dt, "unit": "steps/s"}


def roofline_from_profile(prof, device, kernel_labels, only_prec=None):
    """Aggregate the launch profile by tile program; the program with the largest total time is the dominant kernel.
    ``only_prec``: rank only programs of that operand precision (DM / s2d: the real-clip stream -- the small synthetic-clip
    launches run concurrently on a second stream, and their event-to-event times stretch to the length of the kernels
    they share the CUs with, so their summed durations are not GPU time)."""
    from video_distillation_amd import hip
    agg = {}
    for name, prec, flop, e0, e1 in prof:
        rec = agg.setdefault((name, prec), [0.0, 0, 0.0])
        rec[0] += e0.elapsed_time(e1) * 1e-3
        rec[1] += 1
        rec[2] += flop
    if not agg:
        return None
    inv = {v: k for k, v in hip.PREC.items()}
    total = sum(v[0] for v in agg.values())
    ranked = sorted(agg.items(), key=lambda kv: -kv[1][0])
    first = [kv for kv in ranked if only_prec is None or kv[0][1] == hip.PREC[only_prec]] or ranked
    (name, prec), (secs, n, flop) = first[0]
    achieved = flop / secs / 1e12
    x3 = hip.is_x3(prec)
    return {"bound": "mfma", "kernel": "%s, tile program '%s', operands %s" % (kernel_labels.get(name, "conv_mfma_kernel"), name, inv[prec]),
            "achieved": achieved, "peak": PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_TFLOPS,
            "launches": n, "mean_launch_ms": secs / n * 1e3, "flop_per_launch": flop / n,
            "share_of_conv_time": secs / total,
            "note": ("hi+lo operand pairs: 3 MFMAs per algorithmic product, so 1/3 of peak is this program's ceiling" if x3 else None),
            "programs": [{"program": k[0], "operands": inv[k[1]], "launches": v[1], "ms_total": v[0] * 1e3,
                          "tflops": v[2] / v[0] / 1e12 if v[0] > 0 else None} for k, v in ranked[:8]]}


_REAL_STDOUT = None


def quiet_stdout():
    """Everything that writes to fd 1 while the benchmark runs -- RCCL's version banner, evaluate_synset's progress
    line -- is sent to stderr; the ONE JSON line is written to the real stdout at the very end (``finish``)."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def finish(h, out, extra_rank0=None):
    import torch.distributed as dist
    from video_distillation_amd import distill
    refused = None
    if out is not None:     # data-path collectives this rank's trainers issued over the whole run (warm-up, timed, sustained, eval)
        out["collectives"] = dict(distill.COLLECTIVE_CALLS, backend=(dist.get_backend() if dist.is_initialized() else None),
                                  forced_on_one_rank=(h.world == 1 and distill.collectives_on(1)))
        from video_distillation_amd import hip
        out["library"] = {"sources_hash": hip.loaded_stamp(), "checkout_sources_hash": hip.sources_hash(), "abi": int(hip.lib().vd_abi_version())}
        refused = refuse_unproven(out, h.world)
    if h.comm is not None:
        h.comm.free()
        h.comm = None
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    if h.rank == 0:
        line = (json.dumps(out) + "\n").encode()
        if _REAL_STDOUT is not None:
            os.write(_REAL_STDOUT, line)
        else:
            sys.stdout.write(line.decode())
    if refused:
        print("bench.py: value withheld -- " + refused, file=sys.stderr)
        sys.exit(4)


def refuse_unproven(out, world):
    """An N-rank line must PROVE its N ranks: ``ranks_seen`` (an all-reduce of ones over the process group) and, where RCCL
    itself reported a rank count (``rccl.nranks`` = ncclCommCount, or the process group's size), both must equal ``n_gpus``.
    Otherwise ``value`` is withheld (null, the reason in ``refused``) and the run exits non-zero: a throughput of N GPUs that
    fewer ranks produced must never be printed.  Returns the reason or None."""
    why = []
    if out.get("n_gpus") != world:
        why.append("n_gpus %r but world size %d" % (out.get("n_gpus"), world))
    if out.get("ranks_seen") != world:
        why.append("ranks_seen %r != %d" % (out.get("ranks_seen"), world))
    rccl = out.get("rccl")
    if isinstance(rccl, dict) and "nranks" in rccl and rccl["nranks"] != world:
        why.append("rccl.nranks %r != %d" % (rccl["nranks"], world))
    cps = out.get("clips_per_step")
    if isinstance(cps, list) and len(cps) != world:
        why.append("clips_per_step lists %d ranks, not %d" % (len(cps), world))
    if not why:
        return None
    reason = "; ".join(why)
    for key in ("value", "value_median"):
        if key in out:
            out[key] = None
    out["refused"] = reason
    return reason


def base_record(args, h, metric, dt, per_step, dtype, workload, parallelism, precision):
    med = float(np.median(per_step))
    return {"metric": metric, "value": args.steps / dt, "unit": "steps/s", "n_gpus": h.world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "ms_per_step_median": med,
            "value_median": 1e3 / med, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": dtype,
            "data": "synthetic", "config": {"workload": workload, "precision": precision, "parallelism": parallelism}}


DUMP_SAMPLE = 1 << 22          # elements written per array at most (16 MB of float32; four such arrays stay under 64 MB)


def dump_outputs(args, h, loss, state):
    """--dump-outputs: ``loss`` (the global loss of the last timed step) and ``state`` (name -> tensor: what the trainer hands
    its caller after that step) as DIR/<name>.npy, on rank 0.  Every input of a run is seeded from the command line, so two
    builds given the same arguments can be compared file for file.  -> summary for the JSON line, or None."""
    if not args.dump_outputs or h.rank != 0:
        return None
    os.makedirs(args.dump_outputs, exist_ok=True)
    arrays = {"loss": np.asarray(float(loss), dtype=np.float64)}
    for name, t in state.items():
        arrays[name] = t.detach().float().cpu().numpy()
    rec, nbytes = {}, 0
    for name, a in arrays.items():
        shape = list(a.shape)
        if a.size > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False))
            a = a.reshape(-1)[idx]
        nbytes += a.nbytes
        assert nbytes <= 64 << 20, "--dump-outputs writes 64 MB at most"
        np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
        rec[name] = {"shape": shape, "written": int(a.size)}
    return {"dir": args.dump_outputs, "arrays": rec}


def trainer_state(trainer, world):
    """The learnable state a trainer holds after its latest step, whole (every rank calls: collectives where it is sharded by
    class).  DM / DC: the synthetic clips; s2d: dynamic memories + hallucinator (the static memories are frozen); MTT: the
    synthetic clips or memories + syn_lr (replicated over the ranks)."""
    if hasattr(trainer, "sync"):
        trainer.sync()
    torch.cuda.synchronize()
    if hasattr(trainer, "hal_w"):
        dyn = trainer.dynamic
        if world > 1 and hasattr(trainer, "c_lo"):          # S2DTrainer: every rank owns the dynamic rows of its classes
            import torch.distributed as dist
            parts = [None] * world
            dist.all_gather_object(parts, dyn.cpu())
            dyn = torch.cat(parts, 0)
        state = {"dynamic": dyn, "hal_w": trainer.hal_w, "hal_b": trainer.hal_b}
    else:
        state = {"image_syn": trainer.gather_syn() if hasattr(trainer, "gather_syn") else trainer.image_syn}
    if hasattr(trainer, "syn_lr"):
        state["syn_lr"] = trainer.syn_lr
    return state


# ------------------------------------------------------------------------------------------------------------------------
# DM / s2d (configs 1-3)
# ------------------------------------------------------------------------------------------------------------------------
def cpu_baseline_dm(args, trainer, backend, it, s2d=None):
    """The oracle on `cpu_classes` whole class terms (fwd 64 real + ipc syn, bwd to pixels -- for s2d through the
    hallucinator to the memories) with the SAME weights and clips the GPU uses for iteration `it`; also the loss parity of
    those class terms in the shipped precision mode."""
    from oracle import ref_cpu as R
    from video_distillation_amd import distill
    ncls = min(args.cpu_classes, len(trainer.classes))
    classes = trainer.classes[:ncls]
    weights = backend.new_network(seed=it)
    params = [w.cpu() for w in weights]
    idx = distill.sample_real_indices(it, trainer.pool.counts, trainer.pool.offsets, args.batch_real, classes)
    dev = trainer.pool.clips.device
    real = trainer.pool.clips[torch.as_tensor(idx, device=dev)].cpu()
    if s2d is None:
        syn = trainer.image_syn[:ncls * args.ipc].detach().clone()
    else:
        sidx, didx = (torch.as_tensor(t, device=dev) for t in trainer.indices(it))
        n = ncls * trainer.vpc
        syn = backend.hallucinate(trainer.static, trainer.dynamic, sidx[:n], didx[:n], trainer.hal_w, trainer.hal_b)
    backend.set_real_weights(weights, args.batch_real)
    f_real = backend.embed_pool(trainer.pool.clips, torch.as_tensor(idx, device=dev), args.batch_real)
    f_syn, _ = backend.embed_syn(syn, weights)
    loss_gpu = float(backend.dm_loss(f_real, f_syn, ncls)[0].sum())
    reals = [real[c * args.batch_real:(c + 1) * args.batch_real] for c in range(ncls)]

    def probe():
        with torch.no_grad():
            R.convnet3d_embed(reals[0][:8], params)
    threads, ncpu = best_threads(probe)
    per_cls = syn.shape[0] // ncls
    t0 = time.perf_counter()
    if s2d is None:
        loss_cpu, _ = R.dm_loss_and_grad(params, reals, syn.cpu(), per_cls)
    else:
        st = trainer.static.cpu().requires_grad_(False)
        dy = trainer.dynamic.cpu().requires_grad_(True)
        w, b = trainer.hal_w.cpu().requires_grad_(True), trainer.hal_b.cpu().requires_grad_(True)
        img = R.hallucinator(st[sidx[:n].cpu()], dy[didx[:n].cpu()], w, b)
        if os.environ.get("VD_BENCH_DEBUG"):
            print("debug s2d: |img cpu| %g |syn gpu| %g |st| %g |dy| %g |w| %g diff %g" % (
                float(img.norm()), float(syn.norm()), float(st.norm()), float(dy.norm()), float(w.norm()),
                float((img.detach() - syn.cpu()).norm())), file=sys.stderr)
        loss_cpu = torch.zeros(())
        for c in range(ncls):
            loss_cpu = loss_cpu + R.dm_class_term(R.convnet3d_embed(reals[c], params).detach(),
                                                  R.convnet3d_embed(img[c * per_cls:(c + 1) * per_cls], params))
        torch.autograd.grad(loss_cpu, [dy, w, b])
        loss_cpu = loss_cpu.detach()
    dt = time.perf_counter() - t0
    per_step = dt / ncls * args.classes
    return {"value": 1.0 / per_step, "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": "%d of %d class terms (%d real + %d syn clips %dx%dx%d each, fwd + bwd to %s), %.1f s, extrapolated x%.1f; "
                      "threads = fastest of a calibration over 8..%d (host has %d logical CPUs)" % (
                          ncls, args.classes, args.batch_real, per_cls, args.size, args.size, args.frames,
                          "pixels" if s2d is None else "dynamic memories + hallucinator", dt, args.classes / ncls, ncpu, ncpu),
            "loss_cpu_sample": float(loss_cpu), "loss_gpu_sample": loss_gpu,
            "loss_rel_err_vs_gpu": abs(loss_gpu - float(loss_cpu)) / abs(float(loss_cpu))}


def run_eval(args, trainer, pool, device, rank):
    """evaluate_synset (utils.py:848-886) on the current synthetic clips: a fresh ConvNet3D trained for --eval-epochs
    epochs with the HIP train step (ordered accumulation mode unless --eval-atomic), tested (3 passes, HIP inference) on the
    LAST 4 pool clips of every class, which main() took out of the range real batches and initial synthetic clips are drawn
    from.  Networks are built directly from fixed seeds (not through get_network, which reseeds from the wall clock), so the
    per-seed accuracies repeat from run to run.  On the default template pool the accuracy is informative; on --pool-kind
    randn it is chance level by construction."""
    import types
    from video_distillation_amd import networks, utils
    C = args.classes
    syn = trainer.gather_syn().detach().clone()            # (collective: every rank calls)
    if rank != 0:
        return None
    labels = torch.arange(C, device=device).repeat_interleave(args.ipc)
    resident = set(trainer.classes) | set(trainer.__dict__.get("split", []))       # classes whose real clips this rank holds
    call = getattr(pool, "counts_all", pool.counts)
    held_out = all(call[c] - pool.counts[c] == 4 for c in range(C) if call[c] > 0)
    have = [c for c in range(C) if call[c] > 4 and (c in resident or trainer.__dict__.get("shard") == "batch")]
    idx = torch.as_tensor([pool.offsets[c] + call[c] - 1 - k for c in have for k in range(4)], device=device)
    test = utils.TensorDataset(pool.clips[idx], torch.as_tensor(have, device=device).repeat_interleave(4))
    loader = torch.utils.data.DataLoader(test, batch_size=64, shuffle=False)
    eargs = types.SimpleNamespace(device=device, lr_net=0.01, epoch_eval_train=args.eval_epochs, batch_train=256,
                                  model="ConvNet3D", eval_mode="SS")
    # The outcome of 500 SGD epochs on 50 clips depends strongly on the network's initial weights and dropout masks (0.55 .. 0.97
    # top-1 between unseeded runs of one build, an occasional collapsed run at chance): --eval-seeds networks are trained from fixed
    # seeds and the MEAN top-1 is reported next to the per-seed values.
    import contextlib
    tops, trains = [], []
    from video_distillation_amd import hip
    prev_det = hip.set_deterministic(not args.eval_atomic)     # fixed summation order: the same top-1 per seed in every run
    try:            # (the library's accumulation mode is process-wide: restored even if a training run raises)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for sd in range(max(1, args.eval_seeds)):
            # (NOT utils.get_network: like the reference's it reseeds torch's global generator from the wall clock on every call
            #  -- SURVEY Q5 --, which is what made rounds 1-3's "fixed-seed" networks differ from run to run: initial weights,
            #  dropout masks and shuffles all came from the clock.  The module is constructed directly, as get_network does inside.)
            torch.manual_seed(1000 + sd)
            net = networks.ConvNet3D(channel=3, num_classes=C, net_width=128, net_depth=3, net_act='relu', net_norm='none',
                                     net_pooling='maxpooling', im_size=(args.size, args.size), frames=args.frames).to(device)
            with contextlib.redirect_stdout(sys.stderr):        # evaluate_synset prints its own progress line, like the reference
                _, acc_train, acc_test, _ = utils.evaluate_synset(sd, net, syn, labels, loader, eargs, mode="none")
            tops.append(float(acc_test)); trains.append(float(acc_train))
        torch.cuda.synchronize()
    finally:
        hip.set_deterministic(prev_det)
    dt = (time.perf_counter() - t0) / len(tops)
    return {"deterministic": not args.eval_atomic, "test_split": "held out (never drawn as real or initial synthetic clips)" if held_out else
            "last 4 clips of each class (drawable as real clips)",
            "top1": sum(tops) / len(tops), "acc_train": sum(trains) / len(trains), "top1_per_seed": tops, "epochs": args.eval_epochs + 1,
            "seconds": dt, "ms_per_epoch": dt / (args.eval_epochs + 1) * 1e3, "test_clips": int(idx.numel()),
            "note": (("class template + noise pool: chance is %.3f.  " % (1.0 / C)) if args.pool_kind == "templates" else
                     ("synthetic noise pool: top-1 is chance (%.3f) by construction.  " % (1.0 / C))) +
                    "A SMOKE of evaluate_synset on the HIP path (5 networks x %d epochs on 50 clips that are %d DM steps from a real clip), "
                    "reproducible per command line but not a metric: two DM steps more move a seed from 0.85 to 0.3.  Accuracy parity with "
                    "the reference is fixture G16 (tests/test_gpu_eval_parity.py: mean top-1 0.6135 vs 0.6110)" % (
                        args.eval_epochs + 1, args.warmup + args.steps)}


def exchange_record(trainer, args, geo, h):
    """What a DMTrainer's pixel-gradient exchange moved: nothing under owner-computes; for ``exchange='allreduce'`` the bytes of
    the full gradient tensor per step and the mean time of the all-reduce call itself (HIP events around it on the
    synthetic-clip stream: the collective plus whatever it waits for inside RCCL; this rank's view)."""
    if trainer.exchange != "allreduce":
        return {"pixel_gradient_bytes_per_step": 0, "note": "owner-computes: a rank updates the synthetic clips of its own classes"}
    import torch.distributed as dist
    torch.cuda.synchronize()
    through = "vd_comm_allreduce_f32 (RCCL) on the synthetic-clip stream" if trainer.comm is not None else \
        ("torch.distributed all_reduce (%s)" % dist.get_backend() if dist.is_initialized() else "no process group: identity")
    ms = [e0.elapsed_time(e1) for e0, e1 in trainer.exchange_events]
    nbytes = args.classes * args.ipc * args.frames * 3 * args.size * args.size * 4
    return {"pixel_gradient_bytes_per_step": nbytes, "allreduce_calls": len(ms), "allreduce_ms_mean": (sum(ms) / len(ms)) if ms else None,
            "allreduce_GBps_algorithmic": (nbytes / (sum(ms) / len(ms) * 1e-3) / 1e9) if ms and sum(ms) > 0 else None,
            "through": through}


def bench_dm(args, h, distill, plan, geo, pool, backend, shard):
    device, rank, world = h.device, h.rank, h.world
    s2d = args.method == "s2d"
    if not s2d:
        trainer = distill.DMTrainer(backend, pool, args.classes, args.ipc, args.batch_real, lr_img=1.0, momentum=0.5,
                                    rank=rank, world=world, shard=shard, exchange=args.exchange,
                                    comm=h.open_comm() if args.exchange == "allreduce" else None)
    else:   # sh/s2d/s2d_DM_ms.sh: vpc 1, spc 2, dpc 2, static frozen, SGD(.95) on dynamic memory + hallucinator
        gen = torch.Generator(device=device); gen.manual_seed(77)
        static_syn = torch.randn(args.classes * 2, 3, args.size, args.size, device=device, generator=gen)
        dynamic_syn = torch.randn(args.classes, 2, args.frames, 1, args.size, args.size, device=device, generator=gen)
        hal_w = torch.empty(3, 4, 3, 3, 3, device=device).uniform_(-0.096, 0.096, generator=gen)
        hal_b = torch.empty(3, device=device).uniform_(-0.096, 0.096, generator=gen)
        trainer = distill.S2DTrainer(backend, pool, args.classes, 1, 2, 2, args.batch_real, static_syn, dynamic_syn,
                                     hal_w, hal_b, lr_dynamic=0.01, lr_hal=1e-9, rank=rank, world=world)
        # (lr_dynamic = the reference's default, distill_s2d_ms.py:477; lr_hal scaled down from its 0.01: on the synthetic noise
        #  pool the hallucinator gradient is ~1e7 and the default diverges within three steps)
    gl = trainer.global_loss if hasattr(trainer, "global_loss") else (lambda l: l)

    def step(it):
        return gl(trainer.step(it, overlap=True))
    dt, per_step, prof, losses = h.run(step, trainer.sync, trainer.mark)
    dumped = dump_outputs(args, h, losses[-1], trainer_state(trainer, world)) if args.dump_outputs else None
    # the evaluation runs on the synthetic clips as they are after EXACTLY warmup + steps iterations (before the sustained leg,
    # whose step count is set by the clock): DM steps are free of atomics, the evaluation's training steps run in the fixed-order
    # mode, so `eval.top1_per_seed` is the same in every run of the same command line
    ev = None
    if args.full and args.eval_epochs > 0 and not s2d:
        ev = run_eval(args, trainer, pool, device, rank)
    sustained = h.sustained(step, trainer.sync, args.warmup + args.steps) if args.full else None
    # Two short extra legs of the same workload, on record next to the headline: the fp32-grade mode (every operand a hi+lo pair)
    # and round 2's fast mode (single pass on every real level and in the input gradient).  Every rank runs them.
    legs = {}
    if args.full and not s2d and not args.no_extra_legs:
        from video_distillation_amd.networks import _batch_hint
        for name, kw in (("parity_mode", dict(prec_real=args.prec_syn, prec_syn=args.prec_syn, prec_bwd=args.prec_syn)),
                         ("fast_mode", dict(prec_real=args.prec_real, prec_syn=args.prec_syn, prec_bwd=args.prec_real, real_last="x1"))):
            be2 = distill.HipBackend(geo, device, chunk=args.chunk, syn_batch_hint=_batch_hint(len(trainer.classes) * args.ipc), **kw)
            tr2 = distill.DMTrainer(be2, pool, args.classes, args.ipc, args.batch_real, lr_img=1.0, momentum=0.5, rank=rank, world=world,
                                    shard=shard)
            n_leg, warm = (5, 2)
            for it in range(warm):
                tr2.global_loss(tr2.step(it, overlap=True))
            tr2.sync(); h.barrier()
            t0 = time.perf_counter()
            for it in range(warm, warm + n_leg):
                last = tr2.global_loss(tr2.step(it, overlap=True))
            tr2.sync(); h.barrier()
            dt2 = time.perf_counter() - t0
            if world > 1:
                import torch.distributed as dist
                tmax = torch.tensor([dt2], device=device, dtype=torch.float64)
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                dt2 = float(tmax)
            legs[name] = {"value": n_leg / dt2, "unit": "steps/s", "ms_per_step": dt2 / n_leg * 1e3, "steps": n_leg, "warmup": warm,
                          "precision": {"real_clips": kw["prec_real"], "real_clips_last_level": be2.real_last,
                                        "syn_clips_fwd": kw["prec_syn"], "input_gradient": kw["prec_bwd"],
                                        "real_weight_dither_groups": be2._dither},
                          "loss_last": float(last) / args.classes}
            del tr2, be2
            torch.cuda.empty_cache()
    # The exchange mode that is NOT the timed one, as a short leg of the same workload in the shipped precision mode: with
    # --exchange owner (default) this is the literal pixel-gradient all-reduce, so that its cost stands next to owner-computes
    # the first time more than one GPU is available.  Every rank runs it (it contains the collective).
    if args.full and not s2d and (world > 1 or os.environ.get("VD_BENCH_EXCHANGE_LEG") == "1") and (args.exchange_leg or not args.no_extra_legs):
        other = "allreduce" if args.exchange == "owner" else "owner"
        tr3 = distill.DMTrainer(backend, pool, args.classes, args.ipc, args.batch_real, lr_img=1.0, momentum=0.5, rank=rank, world=world,
                                shard=shard, exchange=other, comm=h.open_comm() if other == "allreduce" else None)
        n_leg, warm = (5, 2)
        for it in range(warm):
            tr3.global_loss(tr3.step(it, overlap=True))
        tr3.sync(); h.barrier()
        tr3.exchange_events.clear()
        t0 = time.perf_counter()
        for it in range(warm, warm + n_leg):
            last = tr3.global_loss(tr3.step(it, overlap=True))
        tr3.sync(); h.barrier()
        dt3 = time.perf_counter() - t0
        if world > 1:
            import torch.distributed as dist
            tmax = torch.tensor([dt3], device=device, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt3 = float(tmax)
        ex = exchange_record(tr3, args, geo, h)
        legs["exchange_" + other] = dict({"value": n_leg / dt3, "unit": "steps/s", "ms_per_step": dt3 / n_leg * 1e3, "steps": n_leg,
                                          "warmup": warm, "loss_last": float(last) / args.classes}, **ex)
        del tr3
    if s2d or trainer.shard == "class":
        clips = args.batch_real * len(trainer.classes)
    elif trainer.shard == "hybrid":
        clips = args.batch_real * len(trainer.block) + (args.batch_real // world) * len(trainer.split)
    else:
        clips = (args.batch_real // world) * args.classes
    topo = h.topology(clips)
    ex_ms = [e0.elapsed_time(e1) for e0, e1 in getattr(trainer, "exchange_events", [])]
    per_rank = h.per_rank(prof, clips, {"exchange_ms_per_step": (sum(ex_ms) / len(ex_ms)) if ex_ms else None,
                                        "classes_owned": len(trainer.classes)})
    out = None
    if rank == 0:
        macs = conv_layer_macs(geo)
        nsyn = args.ipc if not s2d else 1
        step_flop = 2.0 * sum(macs) * (args.classes * (args.batch_real + nsyn) + args.classes * nsyn)
        name = "DM" if not s2d else "DM+Ours s2d"
        out = base_record(
            args, h, "distillation steps/sec (%s, miniUCF101 IPC=%d)" % (name, args.ipc), dt, per_step,
            args.prec_real, "miniUCF101-shaped %s IPC=%d: C=%d classes x (%d real + %d syn) clips %dx%dx%d, ConvNet3D depth 3, "
            "fresh net per step%s" % (name, args.ipc, args.classes, args.batch_real, nsyn, args.size, args.size, args.frames,
                                      "; vpc 1 / spc 2 / dpc 2, static memories frozen" if s2d else ""),
            ("real batch sharded x%d + all-reduce of per-class feature sums (410 KB); synthetic clips class-owned, no gradient "
             "exchange" % world) if trainer.__dict__.get("shard") == "batch" else
            ("hybrid x%d: %d whole classes per rank + the real batches of %d left-over classes split %d ways (all-reduce of their "
             "feature sums, %d KB); synthetic clips class-owned, no gradient exchange" % (
                 world, args.classes // world, args.classes % world, world, (args.classes % world) * 8)) if trainer.__dict__.get("shard") == "hybrid" else
            "class-sharded x%d (owner-computes, no gradient exchange%s)" % (world, "; 1.3 KB all-reduce of the hallucinator gradient" if s2d else ""),
            {"real_clips": args.prec_real, "real_clips_last_level": backend.real_last, "syn_clips_fwd": args.prec_syn, "input_gradient": args.prec_bwd, "accumulate": "f32",
             "real_weight_dither_groups": backend._dither, "syn_value_pass": None if backend._dither else backend.weight_format,
             "real_clips_last_level_program": (None if backend.eng_real.fwd2x is None else
                                               "position tiles" if backend.eng_real.fwd2x.plan.epi == 3 else "row-major")})
        out["config"]["pool_per_class"] = args.pool_per_class
        out["config"]["pool_kind"] = args.pool_kind
        out["config"]["real_pool"] = ("resident in HBM: fp32 clips + the same clips converted once to the first layer's 16-bit pixel "
                                      "rows; a real batch is an index list, no per-step conversion") if backend.resident_rows else \
            "resident in HBM as fp32, converted per step"
        out["loss_last"] = float(losses[-1]) / args.classes
        if dumped:
            out["dump_outputs"] = dumped
        if getattr(trainer, "real_range", None) is not None:      # what the fp8-corrected last level's producer saw (distill.HipBackend.check_real_range)
            out["config"]["precision"]["real_last_level_activation_range"] = trainer.real_range
        out["step_tflops"] = step_flop / (dt / args.steps) / 1e12
        out["step_frac_of_mfma_peak"] = out["step_tflops"] / PEAK_TFLOPS
        labels = {"fwd1": "conv_mfma_kernel<PREC, 3, false, 2, 1> (balanced 7-tile layout; conv layer 1 forward, real clips)",
                  "fwd0": "conv0_breg_kernel<PREC> (conv layer 0 forward)"}
        roof = roofline_from_profile(prof, device, labels, only_prec=args.prec_real)
        if roof:
            clips = roof["flop_per_launch"] / (2.0 * macs[1]) if "fwd1" in roof["kernel"] else None
            roof["traffic"], roof["traffic_source"] = pmc_traffic("conv1_fwd_f16", clips) if clips else (None, None)
            if args.full:
                roof["peak_measured"] = mfma_peak(device)
                roof["frac_of_measured"] = roof["achieved"] / roof["peak_measured"]
            if args.full and not s2d and world == 1 and not args.no_alone:
                roof["alone"] = real_side_alone(trainer, backend, args, macs, args.warmup + args.steps + 8)
            for p in roof["programs"]:
                if p["program"] in ("fwd0", "fwd2") and p["operands"] == args.prec_real:
                    roof[p["program"] + "_tflops"] = p["tflops"]
                if p["program"] in ("fwd2_hilo", "fwd2_c8"):      # the real side's last level in hi+lo pairs: 3 MFMAs per algorithmic product
                    #                                                (fwd2_c8: the corrections on the fp8 instruction: 2 MFMA-equivalents)
                    roof["fwd2_tflops"] = p["tflops"]
                    roof["fwd2_ms_per_launch"] = p["ms_total"] / max(p["launches"], 1)
            out["roofline"] = roof
        if sustained:
            out["sustained"] = sustained
        if ev:
            out["eval"] = ev
        for name, leg in legs.items():
            out[name] = leg
        out.update(topo)
        out["per_rank"] = per_rank
        out["exchange"] = dict({"mode": args.exchange}, **(exchange_record(trainer, args, geo, h) if not s2d else {}))
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_dm(args, trainer, backend, args.warmup + args.steps, s2d if s2d else None)
    finish(h, out)


# ------------------------------------------------------------------------------------------------------------------------
# gradient matching (config 4)
# ------------------------------------------------------------------------------------------------------------------------
def cpu_baseline_dc(args, trainer, geo, it):
    """The oracle on 2 class terms of the same step: dCE/dparams on the real batch (detached), on the synthetic clips with
    create_graph, match_loss, backward to the pixels."""
    from oracle import ref_cpu as R
    from video_distillation_amd import distill
    import torch.nn.functional as F
    ncls = min(2, len(trainer.classes))
    dev = trainer.image_syn.device
    params = [p.cpu().requires_grad_(True) for p in distill.fresh_full_network(it, args.classes, dev)]
    idx = distill.sample_real_indices(it, trainer.pool.counts, trainer.pool.offsets, args.batch_real, trainer.classes[:ncls])
    real = trainer.pool.clips[torch.as_tensor(idx, device=dev)].cpu()

    def probe():
        with torch.no_grad():
            R.convnet3d_embed(real[:8], params)
    threads, ncpu = best_threads(probe)
    t0 = time.perf_counter()
    total = 0.0
    for k in range(ncls):
        c = trainer.classes[k]
        xr = real[k * args.batch_real:(k + 1) * args.batch_real]
        gw_real = [g.detach() for g in torch.autograd.grad(
            F.cross_entropy(R.convnet3d_logits(xr, params), torch.full((xr.shape[0],), c)), params)]
        xs = trainer.image_syn[k * args.ipc:(k + 1) * args.ipc].detach().cpu().requires_grad_(True)
        gw_syn = torch.autograd.grad(F.cross_entropy(R.convnet3d_logits(xs, params), torch.full((args.ipc,), c)), params,
                                     create_graph=True)
        loss = R.match_loss(gw_syn, gw_real, args.dis_metric)
        torch.autograd.grad(loss, xs)
        total += float(loss)
    dt = time.perf_counter() - t0
    # the same class terms on the HIP path (same weights, clips and labels, dropout off): loss parity of the sample
    ops = trainer.ops
    net = ops.make_net([p.detach().to(dev) for p in params], geo, args.classes)
    net.dropout.p = 0.0
    for p in net.parameters():
        p.requires_grad_(True)
    total_gpu = 0.0
    for k in range(ncls):
        c = trainer.classes[k]
        xr = real[k * args.batch_real:(k + 1) * args.batch_real].to(dev)
        gw_real = [t.detach() for t in ops.param_grads(net, xr, torch.full((xr.shape[0],), c, dtype=torch.int64, device=dev), False)]
        xs = trainer.image_syn[k * args.ipc:(k + 1) * args.ipc].detach().clone().requires_grad_(True)
        gw_syn = ops.param_grads(net, xs, torch.full((args.ipc,), c, dtype=torch.int64, device=dev), True)
        total_gpu += float(ops.match_loss(gw_syn, gw_real))
    return {"value": 1.0 / (dt / ncls * args.classes), "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": "%d of %d class terms (%d real clips first-order + %d syn clips double backward, %dx%dx%d, dropout off), "
                      "%.1f s, extrapolated x%.1f; threads = fastest of a calibration over 8..%d" % (
                          ncls, args.classes, args.batch_real, args.ipc, args.size, args.size, args.frames, dt,
                          args.classes / ncls, ncpu),
            "loss_cpu_sample": total, "loss_gpu_sample": total_gpu, "loss_rel_err_vs_gpu": abs(total_gpu - total) / abs(total)}


def bench_dc(args, h, distill, geo, pool):
    """Config 4: one step = one `for it` iteration of distill.GMTrainer with get_loops(ipc) (ipc 1 / 5 -> outer 1, inner 1)."""
    from video_distillation_amd import networks, utils
    device, rank, world = h.device, h.rank, h.world
    outer, inner = utils.get_loops(args.ipc)
    ops = distill.HipGMOps(device, args.dis_metric)
    trainer = distill.GMTrainer(ops, pool, geo, args.classes, args.ipc, args.batch_real, lr_img=0.1, rank=rank, world=world,
                                outer_loop=outer, inner_loop=inner)

    def mark():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def step(it):
        return trainer.global_loss(trainer.step(it))
    dt, per_step, _, losses = h.run(step, lambda: None, mark, profile=False)
    dumped = dump_outputs(args, h, losses[-1], trainer_state(trainer, h.world)) if args.dump_outputs else None
    sustained = h.sustained(step, lambda: None, args.warmup + args.steps) if args.full else None
    # per-program times: under the class lanes every launch shares the GPU with seven others, so its event-to-event time is
    # not GPU time; one extra step on ONE lane (outside the timed region, on every rank: the step ends in a collective)
    # attributes the conv time to the programs
    prof1 = []
    if args.full:
        lanes_env = os.environ.get("VD_GM_LANES")
        os.environ["VD_GM_LANES"] = "1"
        try:
            prof1 = h.profile_steps(step, lambda: None, args.warmup + args.steps)
        finally:
            if lanes_env is None:
                del os.environ["VD_GM_LANES"]
            else:
                os.environ["VD_GM_LANES"] = lanes_env
    topo = h.topology(args.batch_real * len(trainer.classes))
    out = None
    if rank == 0:
        macs = sum(conv_layer_macs(geo))
        # per class term: real batch fwd + bwd (dgrad + wgrad = 2 x fwd), synthetic clips fwd + bwd + second-order sweep
        # (up: 2 x fwd, down: 2 x dgrad) -- algorithmic products, every pass counted once
        step_flop = 2.0 * macs * len(range(args.classes)) * (args.batch_real * 3 + args.ipc * (3 + 4)) * outer
        out = base_record(args, h, "distillation steps/sec (DC gradient matching '%s', IPC=%d)" % (args.dis_metric, args.ipc),
                          dt, per_step, networks.get_precision()["match"],
                          "HMDB51-shaped gradient matching: C=%d classes x (%d real + %d syn) clips %dx%dx%d, fresh net per step, "
                          "outer_loop %d inner_loop %d" % (args.classes, args.batch_real, args.ipc, args.size, args.size,
                                                           args.frames, outer, inner),
                          "class-sharded x%d (owner-computes, no gradient exchange)" % world, networks.get_precision())
        out["loss_last"] = float(losses[-1]) / args.classes
        if dumped:
            out["dump_outputs"] = dumped
        out["step_tflops"] = step_flop / (dt / args.steps) / 1e12
        out["step_frac_of_mfma_peak"] = out["step_tflops"] / PEAK_TFLOPS
        roof = roofline_from_profile(prof1, device, {})
        if roof:
            roof["traffic"], roof["traffic_source"] = None, None
            roof["peak_measured"] = mfma_peak(device)
            roof["measured_on"] = "one extra step with a single class lane (launches do not overlap); the timed steps run 8 lanes"
            out["roofline"] = roof
        if sustained:
            out["sustained"] = sustained
        out.update(topo)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_dc(args, trainer, geo, args.warmup + args.steps + 1)
    finish(h, out)


# ------------------------------------------------------------------------------------------------------------------------
# trajectory matching (config 5)
# ------------------------------------------------------------------------------------------------------------------------
def cpu_baseline_mtt(args, tr, traj, C, s2d):
    """The oracle on a reduced iteration: 2 unrolled student steps of 32 clips each (create_graph), grand loss, backward to
    the clips / syn_lr -- extrapolated by (syn_steps / 2) x (batch_syn / 32)."""
    from oracle import ref_cpu as R
    steps, nb = 2, min(32, tr.batch_syn)
    dev = tr.image_syn.device
    if s2d:
        these = torch.arange(nb, device=dev)
        label, sidx, didx = tr.indices(these, 0, 0)
        x = tr.ops.hallucinate(tr.static, tr.dynamic, sidx, didx, tr.hal_w, tr.hal_b).cpu()
        labels = label.cpu()
    else:
        x, labels = tr.image_syn[:nb].cpu(), tr.label_syn[:nb].cpu()
    start = [p.cpu() for p in traj[0]]
    target = [p.cpu() for p in traj[1]]

    def probe():
        with torch.no_grad():
            R.convnet3d_embed(x[:8], start)
    threads, ncpu = best_threads(probe)
    t0 = time.perf_counter()
    grand_cpu, _, _ = R.mtt_step(start, target, x, labels, 0.01, [torch.arange(nb)] * steps)
    dt = time.perf_counter() - t0
    scale = (tr.syn_steps / steps) * (tr.batch_syn / nb)
    # the same reduced iteration on the HIP path (same clips, labels, expert segment; dropout off): grand-loss parity of the sample
    from video_distillation_amd import distill, plan
    ops0 = distill.HipMTTOps(plan.NetGeometry(args.frames, args.size, args.size), C, dev, dropout_p=0.0, batch_hint=nb)
    tr0 = distill.MTTTrainer(ops0, C, x.to(dev), labels.to(dev), syn_lr=0.01, lr_img=1.0, lr_lr=1e-6, syn_steps=steps, batch_syn=nb,
                             expert_epochs=1, max_start_epoch=1)
    grand_gpu = float(tr0.step(0, traj, start_epoch=0, index_chunks=[torch.arange(nb)] * steps, update=False))
    del tr0, ops0
    return {"value": 1.0 / (dt * scale), "unit": "steps/s", "cores": threads, "kind": "port",
            "loss_cpu_sample": float(grand_cpu), "loss_gpu_sample": grand_gpu,
            "loss_rel_err_vs_gpu": abs(grand_gpu - float(grand_cpu)) / abs(float(grand_cpu)),
            "sample": "%d unrolled student steps x %d clips %dx%dx%d (create_graph) + backward of the grand loss, %.1f s, "
                      "extrapolated x%.0f to %d steps x %d clips (hallucinator excluded); threads = fastest of a calibration "
                      "over 8..%d" % (steps, nb, args.size, args.size, args.frames, dt, scale, tr.syn_steps, tr.batch_syn, ncpu)}


def bench_mtt(args, h, distill, geo):
    """Config 5 ("Kinetics-400 MTT+Ours"): one iteration = syn_steps unrolled student steps on batch_syn hallucinator-composed
    clips + the reverse sweep to dynamic memories, hallucinator and syn_lr (static frozen, sh/s2d/s2d_MTT_ms_K400.sh); expert
    buffer = random-walk parameter lists shared by all ranks; every step's batch is split over the ranks."""
    from video_distillation_amd import networks
    device, rank, world = h.device, h.rank, h.world
    C = args.classes
    gen = torch.Generator(device=device); gen.manual_seed(99)
    traj = [distill.fresh_full_network(5, C, device)]
    for e in range(11):
        traj.append([p + 0.01 * p.abs().mean() * torch.randn(p.shape, device=device, generator=gen) for p in traj[-1]])
    s2d = not args.mtt_raw
    if s2d:
        vpc, spc, dpc = 1, 2, 2
        batch = min(args.batch_syn, C * vpc)
        ops = distill.HipMTTOps(geo, C, device, dropout_p=0.5, batch_hint=batch // max(world, 1))
        static = torch.randn(C * spc, 3, args.size, args.size, device=device, generator=gen)
        dynamic = torch.randn(C, dpc, args.frames, 1, args.size, args.size, device=device, generator=gen)
        hal_w = torch.empty(3, 4, 3, 3, 3, device=device).uniform_(-0.096, 0.096, generator=gen)
        hal_b = torch.empty(3, device=device).uniform_(-0.096, 0.096, generator=gen)
        tr = distill.S2DMTTTrainer(ops, C, vpc, spc, dpc, static, dynamic, hal_w, hal_b, syn_lr=0.01, lr_dynamic=0.01, lr_hal=0.01,
                                   lr_lr=1e-5, syn_steps=args.syn_steps, batch_syn=batch, expert_epochs=1, max_start_epoch=10,
                                   rank=rank, world=world)
    else:
        batch = min(args.batch_syn, C * args.ipc)
        ops = distill.HipMTTOps(geo, C, device, dropout_p=0.5, batch_hint=batch // max(world, 1))
        image_syn = torch.randn(C * args.ipc, args.frames, 3, args.size, args.size, device=device, generator=gen)
        label_syn = torch.arange(C, device=device).repeat_interleave(args.ipc)
        tr = distill.MTTTrainer(ops, C, image_syn, label_syn, syn_lr=0.01, lr_img=1.0, lr_lr=1e-6, syn_steps=args.syn_steps,
                                batch_syn=batch, expert_epochs=1, max_start_epoch=10, rank=rank, world=world)

    def mark():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def step(it):
        return tr.step(it, traj)
    dt, per_step, _, losses = h.run(step, lambda: None, mark, profile=False)
    dumped = dump_outputs(args, h, losses[-1], trainer_state(tr, h.world)) if args.dump_outputs else None
    sustained = h.sustained(step, lambda: None, args.warmup + args.steps) if args.full else None
    prof = h.profile_steps(step, lambda: None, args.warmup + args.steps) if args.full else []
    topo = h.topology(len(range(rank, tr.batch_syn, max(world, 1))) * tr.syn_steps)      # this rank's share of every student batch
    out = None
    if rank == 0:
        macs = sum(conv_layer_macs(geo))
        # per student step and clip: fwd + first-order bwd (2 x fwd) + second-order sweep with parameter adjoints
        # (up 2 x fwd, down 2 x dgrad + 2 x wgrad)
        step_flop = 2.0 * macs * tr.syn_steps * tr.batch_syn * (3 + 6)
        out = base_record(args, h, "distillation steps/sec (MTT%s, syn_steps=%d)" % ("+Ours s2d" if s2d else "", args.syn_steps), dt,
                          per_step, networks.get_precision()["match"],
                          "Kinetics-400-shaped trajectory matching%s: C=%d classes, %d clips %dx%dx%d per student step x %d steps, "
                          "expert_epochs 1, synthetic random-walk expert buffer" % (
                              " over static+dynamic memories (vpc 1 / spc 2 / dpc 2, static frozen)" if s2d else "", C, tr.batch_syn,
                              args.size, args.size, args.frames, args.syn_steps),
                          "student batch split x%d, all-reduce of flat gradient + Hessian-vector product per inner step" % world,
                          networks.get_precision())
        out["grand_loss_last"] = float(losses[-1])
        if dumped:
            out["dump_outputs"] = dumped
        out["syn_lr"] = float(tr.syn_lr)
        out["operand_format_of_the_twice_differentiable_passes"] = {
            "format": networks.get_precision()["match"],
            "note": "f16x3 = fp16 hi+lo pairs, 22 bits, every gradient-like operand at a measured power-of-two scale, weights x 2^8 "
                    "(round 6); bf16x3 = bf16 pairs, 16 bits, unscaled (rounds 1 - 5; VD_PREC_MATCH=bf16x3).  Parity at this "
                    "configuration's own unroll length: profiles/r06_parity_mtt10*.json; same-box cost of the format: "
                    "profiles/r06_bench_mtt.json vs profiles/r06_bench_mtt_bf16x3.json (tools/refresh_profiles.sh runs both)"}
        out["step_tflops"] = step_flop / (dt / args.steps) / 1e12
        out["step_frac_of_mfma_peak"] = out["step_tflops"] / PEAK_TFLOPS
        roof = roofline_from_profile(prof, device, {})
        if roof:
            roof["traffic"], roof["traffic_source"] = None, None
            roof["peak_measured"] = mfma_peak(device)
            roof["measured_on"] = "one extra untimed step with the launch hook on (the timed steps run without it)"
            out["roofline"] = roof
        if sustained:
            out["sustained"] = sustained
        out.update(topo)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_mtt(args, tr, traj, C, s2d)
    finish(h, out)


# ------------------------------------------------------------------------------------------------------------------------
def spawn_ranks(args):
    """``python bench.py --gpus N`` with no launcher in front: start the N ranks HERE -- N fresh child processes of this very
    command line with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment (what torch.distributed.run would set) --
    from a parent that has made no HIP call (``torch.cuda.device_count()`` does not start the runtime on this image), relay rank
    0's JSON line (the children inherit this process's stdout; ranks other than 0 print nothing to it) and return non-zero if
    any rank fails, ending the others by their exact PIDs.  The reference's counterpart is single-process nn.DataParallel over
    the visible devices (reference utils.py:615-623)."""
    import socket
    import subprocess
    n = args.gpus
    one_device = os.environ.get("VD_BENCH_ONE_DEVICE") == "1"
    ndev = torch.cuda.device_count()
    if ndev < n and not one_device:
        raise SystemExit("--gpus %d but %d HIP device(s) visible (VD_BENCH_ONE_DEVICE=1 shares device 0 over gloo: a logic check, "
                         "not a timing)" % (n, ndev))
    port = os.environ.get("MASTER_PORT")
    if port is None:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = str(s.getsockname()[1])
    from video_distillation_amd import hip
    hip.build()          # a stale library is rebuilt ONCE, here (hipcc makes no HIP call), not by N ranks racing on the same object files
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, VD_BENCH_SPAWNED="1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    live = list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                print("bench.py: rank %d exited with code %d; stopping the other ranks" % (procs.index(p), code), file=sys.stderr)
                for q in live:
                    q.terminate()                       # exact PIDs of our own children
    return rc if rc >= 0 else 1


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    quiet_stdout()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device")
    # VD_BENCH_ONE_DEVICE=1 (tests/test_gpu_collectives.py): all ranks share device 0 and exchange over gloo (RCCL refuses two ranks
    # on one device) -- the N-rank data path of the trainers with the HIP kernels underneath, on a one-GPU box; not a timing mode
    one_device = os.environ.get("VD_BENCH_ONE_DEVICE") == "1"
    dev_index = 0 if one_device else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1 or os.environ.get("VD_BENCH_FORCE_DIST") == "1":      # (the env: exercise the RCCL calls on a one-GPU box)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if one_device:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", device_id=device, rank=rank, world_size=world)
    if os.environ.get("VD_BENCH_FAIL_RANK") == str(rank) and world > 1:       # fault injection of tests/test_gpu_collectives.py
        raise SystemExit(3)
    torch.manual_seed(args.seed)        # dropout masks of the DC / MTT class terms and the eval networks' shuffles: reproducible runs
    if args.pool_per_class is None:
        args.pool_per_class = 1 if args.method == "mtt" else 93

    from video_distillation_amd import distill, plan
    from video_distillation_amd.networks import _batch_hint
    geo = plan.NetGeometry(args.frames, args.size, args.size)
    h = Harness(args, device, rank, world)
    if args.method == "mtt":
        return bench_mtt(args, h, distill, geo)
    c_lo, c_hi = distill.class_range(args.classes, rank, world)
    shard = args.shard
    if shard == "auto":
        # (distill.choose_shard: the hybrid where the class blocks are more than 8 % uneven and the real batch divides by the number of
        #  ranks, whole-class blocks otherwise.  Single-GPU proxy of one rank's step in the shipped mode -- tools/rank_proxy.py,
        #  profiles/r03_rank_proxy.txt; exchange not included --: N = 2: class 18.3 / batch 18.4 ms; N = 4: class 9.65 / batch 9.68 /
        #  hybrid 9.66; N = 8: class 5.7 / batch 4.9 / hybrid 4.9, i.e. 6.2x / 7.35x / 7.3x of one GPU)
        shard = distill.choose_shard(args.classes, args.batch_real, world, args.method)
    if shard == "hybrid" and args.method != "dm":
        raise SystemExit("--shard hybrid is a decomposition of --method dm")
    if shard == "batch":   # every rank holds the whole pool (11 GB) and embeds its slice of each class batch
        pool = distill.RealPool.synthetic(args.classes, list(range(args.classes)), args.pool_per_class, geo, device, seed=1234,
                                          kind=args.pool_kind, noise=args.pool_noise)
    elif shard == "hybrid":   # the rank's block of whole classes + every split class
        block, split, _ = distill.hybrid_partition(args.classes, rank, world)
        pool = distill.RealPool.synthetic(args.classes, block + split, args.pool_per_class, geo, device, seed=1234, kind=args.pool_kind, noise=args.pool_noise)
    else:
        pool = distill.RealPool.synthetic(args.classes, list(range(c_lo, c_hi)), args.pool_per_class, geo, device, seed=1234,
                                          kind=args.pool_kind, noise=args.pool_noise)
    if args.method == "dc":
        return bench_dc(args, h, distill, geo, pool)
    # dm: the LAST 4 clips of every class are the evaluation's test split and are taken out of the range the real batches (and the
    # initial synthetic clips) are drawn from -- held-out data (they used to be drawable as real clips)
    pool.counts_all = list(pool.counts)
    if args.method == "dm" and all(n == 0 or n - 4 >= args.batch_real for n in pool.counts):
        pool.counts = [max(0, n - 4) for n in pool.counts]
    nsyn = (c_hi - c_lo) * (args.ipc if args.method == "dm" else 1)
    if shard == "hybrid":
        nsyn = (args.classes // world + 1) * args.ipc
    backend = distill.HipBackend(geo, device, prec_real=args.prec_real, prec_syn=args.prec_syn, chunk=args.chunk,
                                 prec_bwd=args.prec_bwd, real_last=args.real_last,
                                 syn_batch_hint=_batch_hint(nsyn) if os.environ.get("VD_SYN_HINT", "1") == "1" else None)
    return bench_dm(args, h, distill, plan, geo, pool, backend, shard)


if __name__ == "__main__":
    main()
