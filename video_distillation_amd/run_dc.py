#!/usr/bin/env python3
"""Gradient-matching (DC) driver over the HIP hot path, with two kinds of memory.

    python -m video_distillation_amd.run_dc --memories images --dataset miniUCF101 --data_path D --ipc 1
    python -m video_distillation_amd.run_dc --memories static --dataset singleUCF50 --data_path D --spc 2
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m video_distillation_amd.run_dc ...

``--memories images`` is the ``--method DC`` branch the reference's distill_baseline.py promises -- its parser defaults to DC and
has ``--outer_loop`` / ``--inner_loop`` / ``--dis_metric`` for it (:366-415), ``get_loops`` and ``match_loss`` are in its utils,
the loop body itself is absent: ``distill.GMTrainer`` on synthetic CLIPS, written as ``images_{it}.pt`` /
``images_best.pt`` at ``run_dm``'s cadence.

``--memories static`` is the static-learning stage of the static + dynamic method (the reference's README, step 4: "Static
Learning", for which it offers a download): ``distill.StillGMTrainer`` on synthetic still IMAGES, ``--spc`` per class, written as
``static_{it}.pt`` / ``static_best.pt`` = ``{"image": (C*spc,3,H,W)}`` -- what ``run_s2d`` / ``run_mtt --memories s2d`` read
with ``--path_static`` and the reference reads with ``torch.load(path)["image"]``.

    DEVIATION.  Upstream DC matches the gradients of a 2-D ConvNet on single frames.  This project has no 2-D network on the
    HIP path; the static stage matches the gradients of the hot path's own ConvNet3D on STILL CLIPS, one image repeated over
    ``--frames`` frames.  That is what the reference's ``static*`` datasets hand to ConvNet3D (distill_utils/dataset.py:626-633)
    and what the hallucinator's static branch feeds the network in the next stage.  DESIGN section 16.

Data.  ``images``: as ``run_dm`` (``run_dm.load_data``).  ``static``: the reference's ``single*`` dataset names with
``--data_path`` (items are (3,H,W) images), ``--data_file f.pt`` holding {"images": (N,3,H,W), "labels": (N,), optionally
"test_images", "test_labels"}, or ``--dataset synthetic``.  ``--init real`` starts from the first ``ipc`` clips / ``spc`` stills of
each class, ``--init noise`` from a generator seeded ``--seed``.  Unset ``--outer_loop`` / ``--inner_loop`` come from
``utils.get_loops(ipc)`` (distill_baseline.py:22-26).  Classes shard over ranks as ``GMTrainer`` does.  Evaluation in static
mode trains ConvNet3D on the expanded stills (``mode='none'``); test batches are expanded on the device by the same kernel.

Logging: JSON lines with ``Loss`` (the matching loss summed over classes and the outer loop / ``num_classes``) and the accuracy keys
of the other drivers.  Process setup, log, evaluation round and the project's own flags are ``driver.py``'s.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import driver


def build_parser():
    p = argparse.ArgumentParser(description="Gradient-matching (DC) distillation on MI355X")
    # the reference parser's names and defaults for what a DC loop reads (distill_baseline.py:366-415)
    p.add_argument('--dataset', type=str, default='miniUCF101')
    p.add_argument('--method', type=str, default='DC', choices=['DC'])
    p.add_argument('--model', type=str, default='ConvNet3D')
    p.add_argument('--ipc', type=int, default=1)
    p.add_argument('--eval_mode', type=str, default='S')
    p.add_argument('--outer_loop', type=int, default=None)
    p.add_argument('--inner_loop', type=int, default=None)
    p.add_argument('--num_eval', type=int, default=5)
    p.add_argument('--eval_it', type=int, default=50)
    p.add_argument('--epoch_eval_train', type=int, default=1000)
    p.add_argument('--Iteration', type=int, default=1000)
    p.add_argument('--lr_net', type=float, default=0.001)
    p.add_argument('--lr_img', type=float, default=1)
    p.add_argument('--batch_real', type=int, default=256)
    p.add_argument('--batch_train', type=int, default=256)
    p.add_argument('--init', type=str, default='real', choices=['noise', 'real'])
    p.add_argument('--data_path', type=str, default='distill_utils/data')
    p.add_argument('--dis_metric', type=str, default='ours')
    p.add_argument('--num_workers', type=int, default=8, help='decode threads of the preload')
    p.add_argument('--preload', action='store_true', help='accepted; no effect (the real pool is always resident)')
    p.add_argument('--save_path', type=str, default='./logged_files')
    p.add_argument('--frames', type=int, default=16)
    # the project's own
    p.add_argument('--memories', type=str, default='images', choices=['images', 'static'],
                   help="images: synthetic clips (images_{it}.pt); static: synthetic still images (static_{it}.pt)")
    p.add_argument('--spc', type=int, default=2, help='--memories static: images per class')
    p.add_argument('--seed', type=int, default=0, help='seed of --init noise')
    p.add_argument('--pool_per_class', type=int, default=93, help='synthetic data only')
    driver.add_data_flags(p)
    driver.add_eval_flags(p)
    return p


class StillTestLoader:
    """A loader of (B,3,H,W) test images as a loader of (B,T,3,H,W) still clips: every batch goes to ``device`` and is repeated
    over ``frames`` there (``distill.still_expand``: the kernel of the training side).  Everything else is the wrapped
    loader's."""

    def __init__(self, loader, ops, device, frames: int):
        self.loader, self.ops, self.device, self.frames = loader, ops, device, int(frames)

    def __iter__(self):
        from . import distill
        for x, y in self.loader:
            yield distill.still_expand(self.ops, x.float().to(self.device).contiguous(), None, self.frames), y

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):
        return getattr(self.loader, name)


def _pool_of_sorted(items: torch.Tensor, labels: torch.Tensor, rank: int, world: int, device):
    """Items ordered by class, this rank's classes on ``device`` -> (RealPool, num_classes, (c_lo, c_hi))."""
    from . import distill
    num_classes = int(labels.max()) + 1
    c_lo, c_hi = distill.class_range(num_classes, rank, world)
    order = torch.argsort(labels, stable=True)
    items, labels = items[order], labels[order]
    counts = torch.bincount(labels, minlength=num_classes).tolist()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    a, b = int(starts[c_lo]), int(starts[c_hi])
    return distill.RealPool(items[a:b].to(device), counts, [int(s) - a for s in starts[:-1]]), num_classes, (c_lo, c_hi)


def load_stills(args, rank, world, device):
    """-> (RealPool whose ``clips`` are this rank's classes' stills (N,3,H,W) on ``device``, num_classes, (c_lo, c_hi), a loader
    of test images or None)."""
    from . import distill, plan
    hw = (args.im_size, args.im_size)
    if args.data_file is not None:
        blob = torch.load(args.data_file, map_location="cpu")
        if "images" not in blob:
            raise KeyError('--memories static reads {"images": (N,3,H,W), "labels": (N,)} from --data_file')
        images, labels = blob["images"].float(), blob["labels"].long()
        if images.dim() != 4 or tuple(images.shape[1:]) != (3,) + hw:
            raise ValueError("%s holds images of shape %s; --im_size %d needs (N, 3, %d, %d)"
                             % (args.data_file, tuple(images.shape), args.im_size, hw[0], hw[1]))
        loader = None
        if "test_images" in blob:
            loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(blob["test_images"].float(), blob["test_labels"].long()),
                                                 batch_size=64, shuffle=False)
        return _pool_of_sorted(images, labels, rank, world, device) + (loader,)
    if args.dataset == 'synthetic':
        geo1 = plan.NetGeometry(1, hw[0], hw[1])
        c_lo, c_hi = distill.class_range(args.num_classes, rank, world)
        pool = distill.RealPool.synthetic(args.num_classes, list(range(c_lo, c_hi)), args.pool_per_class, geo1, device)
        pool.clips = pool.clips[:, 0].contiguous()
        per = max(1, min(8, args.pool_per_class))          # a small test set of the same distribution, every class, other seed
        test = distill.RealPool.synthetic(args.num_classes, list(range(args.num_classes)), per, geo1, device, seed=4321)
        loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(
            test.clips[:, 0].cpu(), torch.arange(args.num_classes).repeat_interleave(per)), batch_size=64, shuffle=False)
        return pool, args.num_classes, (c_lo, c_hi), loader
    from . import dataset as D
    if not args.dataset.startswith('single'):
        raise ValueError("--memories static reads still images: --dataset single* (singleUCF50, singleUCF101, singleHMDB51, "
                         "singleKinetics400, singleSSv2), synthetic, or a --data_file with \"images\"; not %s" % args.dataset)
    _, im_size, num_classes, _, _, _, dst_train, _, loader = D.get_dataset(args.dataset, args.data_path, img_size=hw)
    if tuple(im_size) != hw:
        raise ValueError("--dataset %s has %dx%d images; pass --im_size %d" % (args.dataset, im_size[0], im_size[1], im_size[0]))
    c_lo, c_hi = distill.class_range(num_classes, rank, world)
    classes = list(range(c_lo, c_hi))
    if torch.device(device).type == "cuda":
        pool = distill.RealPool.from_dataset(dst_train, num_classes, classes, device, workers=args.num_workers)
    else:          # (the host logic without a GPU: the same items in the same order, read one by one)
        per_class = D.indices_class(dst_train.labels, num_classes)
        order = [i for c in classes for i in per_class[c]]
        stills = torch.stack([dst_train[i][0] for i in order]) if order else torch.empty((0, 3) + hw)
        counts = [len(per_class[c]) for c in range(num_classes)]
        offsets, o = [0] * num_classes, 0
        for c in classes:
            offsets[c] = o
            o += counts[c]
        pool = distill.RealPool(stills, counts, offsets)
    return pool, num_classes, (c_lo, c_hi), loader


def run(args, ops=None, log=None):
    from . import checkpoint, distill, plan, utils
    static_mode = args.memories == 'static'
    per_class = args.spc if static_mode else args.ipc
    if per_class < 1:
        raise ValueError("--%s %d: at least one memory per class" % ("spc" if static_mode else "ipc", per_class))
    outer_loop, inner_loop = args.outer_loop, args.inner_loop
    if outer_loop is None or inner_loop is None:          # distill_baseline.py:22-26
        table = utils.get_loops(args.ipc)
        outer_loop = table[0] if outer_loop is None else outer_loop
        inner_loop = table[1] if inner_loop is None else inner_loop
    rank, world, device = driver.start(use_cuda=ops is None)
    geo = plan.NetGeometry(args.frames, args.im_size, args.im_size)
    if ops is None:
        ops = distill.HipGMOps(device, args.dis_metric)
    if static_mode:
        pool, num_classes, (c_lo, c_hi), testloader = load_stills(args, rank, world, device)
        if testloader is not None:
            testloader = StillTestLoader(testloader, ops, device, args.frames)
    else:
        from .run_dm import load_data
        pool, num_classes, (c_lo, c_hi), testloader = load_data(args, rank, world, geo, device)
    init = None
    if args.init == 'noise':
        gen = torch.Generator().manual_seed(args.seed)          # drawn in full on the host: every sharding starts from the same state
        shape = (num_classes * per_class,) + (() if static_mode else (args.frames,)) + (3, args.im_size, args.im_size)
        init = torch.randn(shape, generator=gen)[c_lo * per_class:c_hi * per_class].to(device)
    common = dict(lr_net=args.lr_net, momentum=0.5, rank=rank, world=world, outer_loop=outer_loop, inner_loop=inner_loop,
                  batch_train=args.batch_train)
    if static_mode:
        trainer = distill.StillGMTrainer(ops, pool, geo, num_classes, args.spc, args.batch_real, args.lr_img, static=init, **common)
    else:
        trainer = distill.GMTrainer(ops, pool, geo, num_classes, args.ipc, args.batch_real, args.lr_img, image_syn=init, **common)
    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    save_dir = os.path.join(args.save_path, "Static_DC" if static_mode else "Baseline_DC",
                            "%s_%s%d_%s" % (args.dataset, "spc" if static_mode else "ipc", per_class, args.lr_img))
    log = driver.JsonLog(args.log_file, rank, log)
    evaluate = not args.no_eval and testloader is not None
    eval_seed = None
    if args.eval_ranks == 'all' and evaluate:
        eval_seed = driver.draw_eval_seed(args.eval_seed, rank, world)
        log.emit({"eval_ranks": "all", "eval_seed": eval_seed, "world": world})
    label_syn = torch.arange(num_classes).repeat_interleave(per_class)
    eval_its = set(np.arange(0, args.Iteration + 1, args.eval_it).tolist())
    t0 = time.time()
    for it in range(args.Iteration + 1):
        if it in eval_its and (evaluate or it % 1000 == 0):
            syn_all = trainer.gather_syn()          # (collectives: every rank, whoever evaluates or saves)
            memory_all = trainer.gather_static() if static_mode else syn_all
            save_best = False
            if evaluate:
                save_best, _ = driver.evaluate_round(
                    args, it, syn_all.detach().clone(), label_syn, 'none', args.lr_net, testloader, eval_pool, best_acc, best_std, log,
                    rank=rank, world=world, device=device, num_classes=num_classes,
                    pool_seed=None if eval_seed is None else eval_seed + it)
            if rank == 0 and (save_best or it % 1000 == 0):
                (checkpoint.save_static if static_mode else checkpoint.save_images)(save_dir, it, memory_all, best=save_best)
        loss = trainer.global_loss(trainer.step(it))
        if it % 10 == 0 or it == args.Iteration:
            log.emit({"step": it, "Loss": float(loss) / num_classes, "elapsed_s": round(time.time() - t0, 3)})
    log.close()
    return trainer


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)


if __name__ == "__main__":
    main()
