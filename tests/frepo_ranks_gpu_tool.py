"""Child processes of tests/test_gpu_frepo_ranks.py (one per rank, started directly with RANK / WORLD_SIZE set; all ranks on device
0, exchange over gloo -- RCCL refuses two ranks on one device, as in tests/evalpool_gpu_tool.py).

    trainer   --memories images|s2d --out PREFIX [--fail_rank R]    three iterations of FRePoTrainer on the toy problem below: at
                                                                    world 1 plain ``step(x, y)``, otherwise under
                                                                    ``frepo.TargetExchange``; every rank writes PREFIX.rank<r>.json.
                                                                    ``--fail_rank R``: rank R raises (on the host) in its second embed
    run_frepo --data_file F --log_file L --save_path S --eval_seed E   run_frepo --train_videos preload --target_ranks all
                                                                    --eval_ranks all on a toy data file
    pool_on   --data_file F --syn X --y_syn Y --eval_seed E --out PREFIX   evaluate_pool(recipe=frepo.EVAL_RECIPE), one rank, on a
                                                                    saved synthetic set
"""
import argparse
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np              # noqa: E402
import torch                    # noqa: E402
import torch.distributed as dist      # noqa: E402

C, PER, T, S, REAL, POOL = 3, 2, 8, 64, 8, 2
BATCHES = ([0, 1, 2, 3, 4, 5, 6, 7], [6, 1, 3], [5, 2])          # 8, 3 and 2 clips: slices 2/3/3, 1/1/1 and 0/1/1 at three ranks
FREPO_ARGS = ["--memories", "images", "--init", "noise", "--dataset", "toy", "--im_size", str(S), "--frames", str(T), "--Iteration", "2",
              "--num_nn_state", "2", "--max_online_updates", "4", "--seed", "4", "--train_videos", "preload", "--target_ranks", "all",
              "--eval_ranks", "all", "--num_eval", "2", "--epoch_eval_train", "1", "--eval_it", "2", "--startIt", "1"]
EVAL = dict(lr_net=0.001, epoch_eval_train=1, batch_train=C, num_eval=2)          # what FREPO_ARGS make of eargs


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def toy_problem(memories):
    """C = 3 at 8 x 64 x 64, two synthetic clips per class, 8 real clips, from explicit seeds."""
    from video_distillation_amd import frepo, utils
    g = torch.Generator().manual_seed(31)
    real = torch.randn(REAL, T, 3, S, S, generator=g)
    labels = torch.arange(REAL) % C
    y_syn = frepo.soft_labels(torch.arange(C).repeat_interleave(PER), C, frepo.y_scale(C))
    if memories == "images":
        syn = frepo.SynData(torch.randn(C * PER, T, 3, S, S, generator=g), y_syn, learn_label=True)
    else:
        static, dynamic = torch.randn(C * PER, 3, S, S, generator=g), torch.randn(C, PER, T, 1, S, S, generator=g)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(32)
            hals = torch.nn.ModuleList([utils.Conv3DNet() for _ in range(2)])
        syn = frepo.S2DSynData(static, dynamic, hals, y_syn, learn_label=True)
    return real.cuda(), labels.cuda(), syn.cuda()


def trainer_job(a, rank, world):
    from video_distillation_amd import evalpool, frepo
    real, labels, syn = toy_problem(a.memories)
    make = evalpool.convnet3d_factory(C, (S, S), T)
    fetch = lambda rows: real.index_select(0, rows.reshape(-1).to(real.device))
    out = {"rank": rank, "world": world}
    if rank != 0:
        shells = [make(i).cuda() for i in range(POOL)]
        ex = frepo.TargetExchange(lambda i: shells[i], fetch, rank, world, "cuda:0", batch=REAL)
        if a.fail_rank == rank:
            def inject(r, calls):
                if calls == 2:
                    raise OSError("injected on rank %d" % r)
            ex.inject = inject
        ex.sync_all_weights(POOL)
        done = 0
        while ex.follow(done + 1) == frepo.STEP:
            done += 1
        out["steps"] = done
        out["weights"] = [sha(m.parameters()) for m in shells]
    else:
        evalpool.seed_all(77)          # rank 0 holds every draw: the pool's initial weights, the pool index, the hallucinators
        # the element at index 1 starts at step 1 of 2: its first train step resets it, and the reset weights travel
        pools = frepo.build_pool(lambda: make(0), 1e-3, 2, POOL, "cuda:0")
        opt, sch = frepo.syn_optimizer(syn, 1e2, 1e-3, 10)
        tr = frepo.FRePoTrainer(syn, pools, opt, sch)
        ex = None
        if world > 1:
            ex = frepo.TargetExchange(lambda i: pools[i].model, fetch, rank, world, "cuda:0", batch=REAL)
            ex.sync_all_weights(POOL)
        losses, picked = [], []
        for it, batch in enumerate(BATCHES, 1):
            rows = torch.tensor(batch, dtype=torch.int64).reshape(-1, 1)
            y = frepo.soft_labels(labels.index_select(0, rows[:, 0].cuda()), C)
            if ex is None:
                got = tr.step(fetch(rows), y)
            else:
                idx = tr.draw_pool_index()
                got = ex.lead(idx, rows, lambda feat: tr.step(None, y, feat_tar=feat, idx=idx), it)
            picked.append(tr.last_idx)
            losses.append([float(v).hex() for v in got])
        if ex is not None:
            ex.lead_stop()
        out.update(losses=losses, picked=picked, syn=sha(syn.parameters()), weights=[sha(e.model.parameters()) for e in pools],
                   finite=all(np.isfinite(float.fromhex(v)) for row in losses for v in row))
    torch.cuda.synchronize()
    with open("%s.rank%d.json" % (a.out, rank), "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["trainer", "run_frepo", "pool_on"])
    ap.add_argument("--memories", default="images"); ap.add_argument("--out"); ap.add_argument("--fail_rank", type=int, default=-1)
    ap.add_argument("--data_file"); ap.add_argument("--log_file"); ap.add_argument("--save_path")
    ap.add_argument("--syn"); ap.add_argument("--y_syn"); ap.add_argument("--eval_seed", type=int, default=23)
    a = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    os.environ["LOCAL_RANK"] = "0"             # every rank on device 0
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from video_distillation_amd import driver, evalpool, frepo, hip
    assert hip.deterministic(), "run with VD_DETERMINISTIC=1: the comparison is bit for bit"
    if a.what == "trainer":
        trainer_job(a, rank, world)
    elif a.what == "run_frepo":
        from video_distillation_amd import run_frepo
        if rank != 0:
            def refuse(*args, **kw):
                raise AssertionError("rank %d writes a file" % rank)
            run_frepo.save = refuse
        run_frepo.run(run_frepo.build_parser().parse_args(FREPO_ARGS + ["--data_file", a.data_file, "--log_file", a.log_file,
                                                                        "--save_path", a.save_path, "--eval_seed", str(a.eval_seed)]))
    else:
        blob = torch.load(a.data_file, map_location="cpu")
        eargs = types.SimpleNamespace(device="cuda:0", lr_net=EVAL["lr_net"], epoch_eval_train=EVAL["epoch_eval_train"],
                                      batch_train=EVAL["batch_train"])
        x, y = torch.load(a.syn, map_location="cpu").cuda(), torch.load(a.y_syn, map_location="cpu").cuda()
        got = evalpool.evaluate_pool(evalpool.convnet3d_factory(C, (S, S), T), x, y, driver.file_test_loader(blob), eargs,
                                     num_eval=EVAL["num_eval"], seed=a.eval_seed, num_classes=C, recipe=frepo.EVAL_RECIPE)
        with open("%s.rank0.json" % a.out, "w") as f:
            json.dump({"mean": got["mean"], "std": got["std"], "acc_test": got["acc_test"], "loss_test": got["loss_test"],
                       "test_clips": got["test_clips"], "assignment": got["assignment"]}, f)
    torch.cuda.synchronize()
    if world > 1:          # (a rank that raised leaves without it: its peers have raised too, nobody waits for a farewell)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
