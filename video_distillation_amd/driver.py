"""What the drivers (``run_dm``, ``run_s2d``, ``run_mtt``, ``run_coreset``) share: the process setup, the JSON-lines log, the seed
of ``--eval_ranks all``, one evaluation of the current memories, the project's own flags and the test loaders.  Plain functions
that each driver's own loop calls; what a method does differently (when it evaluates, what it saves, what it logs per step)
stays in its driver."""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch


def start(use_cuda: bool):
    """-> (rank, world, device) from ``RANK`` / ``WORLD_SIZE`` / ``LOCAL_RANK``; the process group (nccl on the GPU, gloo on the
    host) is created when there are several ranks and the launcher has not done it."""
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device("cuda", local_rank) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group(backend="nccl" if use_cuda else "gloo")
    return rank, world, device


class JsonLog:
    """Rank 0 writes every record as one JSON line to stdout, to ``log_file`` (appended) and into the list ``sink``; the other
    ranks write nothing."""

    def __init__(self, log_file, rank: int, sink=None):
        self.rank, self.sink = rank, sink
        self.out = open(log_file, "a") if (log_file and rank == 0) else None

    def emit(self, rec: dict) -> None:
        if self.rank != 0:
            return
        line = json.dumps(rec)
        if self.sink is not None:
            self.sink.append(rec)
        print(line, flush=True)
        if self.out:
            self.out.write(line + "\n"); self.out.flush()

    def close(self) -> None:
        if self.out:
            self.out.close()


def draw_eval_seed(given, rank: int, world: int) -> int:
    """``--eval_seed``, or a clock value drawn on rank 0 and broadcast (a collective: every rank calls it or none does)."""
    if given is not None:
        return int(given)
    box = [int(time.time() * 1000) % 100000 if rank == 0 else None]
    if world > 1:
        import torch.distributed as dist
        dist.broadcast_object_list(box, src=0)
    return int(box[0])


def evaluate_round(args, it: int, memories, labels, mode: str, lr_net: float, testloader, eval_pool, best_acc: dict, best_std: dict,
                   log: JsonLog, *, rank: int, world: int, device, num_classes: int, pool_seed=None, test_freq=None):
    """One evaluation of the current memories at iteration ``it``: clips and ``labels`` with ``mode='none'``, ``[static, dynamic,
    hallucinators]`` and ``None`` with ``mode='multi-static'``.  Every model of ``eval_pool`` trains ``--num_eval`` networks with
    learning rate ``lr_net`` -- dealt over all ranks with the seed ``pool_seed`` when one is given (``--eval_ranks all``:
    ``evalpool.evaluate_pool``, every rank calls this), otherwise one after the other on rank 0 while the other ranks pass
    through -- and logs the reference's four accuracy keys; ``best_acc`` / ``best_std`` are updated in place.
    -> (a new best was reached, what ``evaluate_pool`` returned for each model)."""
    from . import evalpool, utils
    hw = (args.im_size, args.im_size)
    eargs = argparse.Namespace(device=str(device), lr_net=lr_net, epoch_eval_train=args.epoch_eval_train, batch_train=args.batch_train,
                               model=args.model, eval_mode=args.eval_mode)
    new_best, pooled = False, []
    for model_eval in eval_pool:
        if pool_seed is not None:
            if model_eval != 'ConvNet3D':
                raise NotImplementedError("--eval_ranks all evaluates ConvNet3D (the hot path's network), not %s" % model_eval)
            got = evalpool.evaluate_pool(evalpool.convnet3d_factory(num_classes, hw, args.frames), memories, labels, testloader, eargs,
                                         num_eval=args.num_eval, seed=pool_seed, mode=mode, rank=rank, world=world,
                                         num_classes=num_classes)
            pooled.append(got)
            mean, std = got["mean"], got["std"]           # (the same numbers on every rank: best_* stay in step)
        elif rank == 0:
            accs = []
            for it_eval in range(args.num_eval):
                net_eval = utils.get_network(model_eval, 3, num_classes, hw, frames=args.frames, dist=False).to(device)
                own = memories.clone() if mode == 'none' else memories          # every network trains on clips of its own
                _, _, acc_test, _ = utils.evaluate_synset(it_eval, net_eval, own, labels, testloader, eargs, mode=mode, test_freq=test_freq)
                accs.append(acc_test)
            mean, std = float(np.mean(accs)), float(np.std(accs))
        else:
            continue
        if mean > best_acc[model_eval]:
            best_acc[model_eval], best_std[model_eval], new_best = mean, std, True
        log.emit({"step": it, "Accuracy/%s" % model_eval: mean, "Max_Accuracy/%s" % model_eval: best_acc[model_eval],
                  "Std/%s" % model_eval: std, "Max_Std/%s" % model_eval: best_std[model_eval]})
    return new_best, pooled


def add_data_flags(p) -> None:
    """The project's own data flags, which every driver has."""
    p.add_argument('--data_file', type=str, default=None)
    p.add_argument('--im_size', type=int, default=112)
    p.add_argument('--num_classes', type=int, default=50, help='synthetic data only')
    p.add_argument('--test_videos', type=str, default='host', choices=['host', 'resident'],
                   help="host: the test loader decodes JPEGs per read; resident: whole test videos in HBM, clips drawn per read "
                        "on the device (dataset.ResidentVideos; 'window' datasets only)")


def add_eval_flags(p) -> None:
    """The project's own log and evaluation flags of the distillation drivers."""
    p.add_argument('--log_file', type=str, default=None)
    p.add_argument('--no_eval', action='store_true')
    p.add_argument('--eval_ranks', type=str, default='rank0', choices=['rank0', 'all'],
                   help="rank0: rank 0 trains and tests the num_eval networks one after the other; all: the networks and their "
                        "three test passes are dealt over all ranks (evalpool.evaluate_pool)")
    p.add_argument('--eval_seed', type=int, default=None,
                   help="--eval_ranks all: seed of the evaluation networks (default: a clock value drawn on rank 0); the "
                        "evaluation at iteration `it` uses eval_seed + it")


def folder_test_loader(args, rank: int, device, dst_test, host_loader):
    """The test loader of a frame-folder dataset: ``get_dataset``'s, or with ``--test_videos resident`` on the ranks that
    evaluate (rank 0; with ``--eval_ranks all`` every rank) whole test videos in HBM.  ``args`` may lack either flag."""
    if getattr(args, 'test_videos', 'host') == 'resident' and (rank == 0 or getattr(args, 'eval_ranks', 'rank0') == 'all'):
        from . import dataset as D
        return D.resident_loader(dst_test, device, batch_size=host_loader.batch_size, workers=args.num_workers)
    return host_loader


def file_test_loader(blob):
    """The test loader of a ``--data_file``, None when it holds no ``test_clips``."""
    if "test_clips" not in blob:
        return None
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(blob["test_clips"].float(), blob["test_labels"].long()),
                                       batch_size=64, shuffle=False)
