#!/usr/bin/env python3
"""DM distillation driver over the HIP hot path (the ``--method DM`` branch of the reference's
distill_baseline.py:292-361, with its flag names for everything that branch reads).

    python -m video_distillation_amd.run_dm --dataset synthetic --ipc 1 --Iteration 100 --eval_it 50
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m video_distillation_amd.run_dm ...

Data: ``--dataset synthetic`` (randn clips); ``--dataset miniUCF101|UCF101|HMDB51|Kinetics400 --data_path D``
(the reference's frame folders, decoded once and kept in HBM: dataset.py; ``--test_videos resident`` keeps the test split's
whole videos there too, so that evaluation draws its clips per read without decoding JPEGs); or ``--data_file f.pt`` holding
{"clips": (N,T,3,H,W), "labels": (N,), "test_clips", "test_labels"}.  Logging: JSON lines with the reference's wandb keys
(``Loss``, ``Accuracy/<model>``, ``Max_Accuracy/<model>``, ``Std/<model>``, ``Max_Std/<model>``).  Process setup, log, the
evaluation round and the project's own flags are shared with the other drivers (``driver.py``).

``--memories static`` learns the static memory of the static + dynamic method by distribution matching on STILL clips
(``distill.StillDMTrainer``; ``run_dc --memories static`` is the same stage by gradient matching): ``--spc`` still images per
class, each fed to ConvNet3D repeated over ``--frames`` frames.

    python -m video_distillation_amd.run_dm --memories static --dataset singleUCF50 --data_path D --spc 2

Data as ``run_dc --memories static`` (``run_dc.load_stills``: the ``single*`` datasets, a ``--data_file`` with "images", or
``synthetic``); ``--init noise`` is drawn in full on the host from ``--seed`` and sliced per rank; ``--ipc`` is not read.
Evaluation trains on the expanded stills; files are ``static_{it}.pt`` / ``static_best.pt`` = ``{"image": (C*spc,3,H,W)}`` under
``save_path/Static_DM/{dataset}_spc{spc}_{lr_img}`` -- what ``run_s2d`` / ``run_mtt --memories s2d`` read with ``--path_static``.
They are written at ``--memories images``' cadence (a new best, or an evaluation iteration that is a multiple of 1000) with ONE
deviation, which is ``run_dc --memories static``'s: with ``--no_eval``, or data without test images, the evaluation iterations
that are multiples of 1000 still write their file (``--memories images`` writes nothing then) -- the file is this stage's
product, and a run that cannot evaluate would otherwise leave none.

``--memories keyframes`` learns KEY-FRAME memories (``distill.KeyframeDMTrainer``): ``--key_frames K`` frames per synthetic clip,
brought to ``--frames`` frames on the device by repeating them over segments (``--interp nearest``) or by linear interpolation
along T (``--interp linear``); K = 1 is a still, K = ``--frames`` the clip.  Real clips, data, sharding and evaluation are those of
``--memories images`` (evaluation trains on the expanded clips); ``--init noise`` is drawn in full on the host from ``--seed`` and
sliced per rank.  Files: ``keyframes_{it}.pt`` / ``keyframes_best.pt`` = ``{"frames": (C*ipc,K,3,H,W), "interp", "T"}`` under
``save_path/Keyframes_DM/{dataset}_ipc{ipc}_k{K}_{interp}_{lr_img}``, at ``--memories images``' cadence;
``checkpoint.keyframes_to_images(path)`` gives the ``images_*.pt`` tensor of such a file.

    python -m video_distillation_amd.run_dm --memories keyframes --key_frames 4 --interp linear --dataset miniUCF101 --data_path D
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import driver


def build_parser():
    p = argparse.ArgumentParser(description="DM distillation on MI355X")
    p.add_argument('--dataset', type=str, default='synthetic')
    p.add_argument('--data_path', type=str, default='distill_utils/data')
    p.add_argument('--num_workers', type=int, default=8, help='decode threads of the preload')
    p.add_argument('--method', type=str, default='DM', choices=['DM'])
    p.add_argument('--model', type=str, default='ConvNet3D')
    p.add_argument('--ipc', type=int, default=1)
    p.add_argument('--eval_mode', type=str, default='SS')
    p.add_argument('--num_eval', type=int, default=5)
    p.add_argument('--eval_it', type=int, default=500)
    p.add_argument('--epoch_eval_train', type=int, default=500)
    p.add_argument('--Iteration', type=int, default=5000)
    p.add_argument('--lr_net', type=float, default=0.01)
    p.add_argument('--lr_img', type=float, default=1.0)
    p.add_argument('--batch_real', type=int, default=64)
    p.add_argument('--batch_train', type=int, default=256)
    p.add_argument('--init', type=str, default='real', choices=['noise', 'real'])
    p.add_argument('--save_path', type=str, default='./logged_files')
    p.add_argument('--frames', type=int, default=16)
    p.add_argument('--pool_per_class', type=int, default=93, help='synthetic data only')
    p.add_argument('--prec_real', type=str, default='f16')
    p.add_argument('--prec_syn', type=str, default='f16x3')
    p.add_argument('--memories', type=str, default='images', choices=['images', 'static', 'keyframes'],
                   help="images: synthetic clips (images_{it}.pt); static: synthetic still images (static_{it}.pt; unlike images, "
                        "also written at evaluation iterations that are multiples of 1000 when nothing is evaluated); keyframes: "
                        "--key_frames learned frames per clip, expanded to --frames on the device (keyframes_{it}.pt)")
    p.add_argument('--spc', type=int, default=2, help='--memories static: images per class')
    p.add_argument('--seed', type=int, default=0, help='--memories static / keyframes: seed of --init noise')
    p.add_argument('--key_frames', type=int, default=4, help='--memories keyframes: learned frames per synthetic clip (1 .. --frames)')
    p.add_argument('--interp', type=str, default='linear', choices=['linear', 'nearest'],
                   help='--memories keyframes: linear interpolation along T, or each key repeated over its segment')
    driver.add_data_flags(p)
    driver.add_eval_flags(p)
    return p


def load_data(args, rank, world, geo, device):
    """-> (RealPool with this rank's classes resident on `device`, num_classes, (c_lo, c_hi), testloader)."""
    from . import distill
    if args.data_file is None and args.dataset != 'synthetic':
        from . import dataset as D
        _, im_size, num_classes, _, _, _, dst_train, dst_test, testloader = D.get_dataset(args.dataset, args.data_path,
                                                                                          img_size=(args.im_size, args.im_size))
        testloader = driver.folder_test_loader(args, rank, device, dst_test, testloader)
        c_lo, c_hi = distill.class_range(num_classes, rank, world)
        pool = distill.RealPool.from_dataset(dst_train, num_classes, list(range(c_lo, c_hi)), device, workers=args.num_workers)
        return pool, num_classes, (c_lo, c_hi), testloader
    if args.data_file is None:
        c_lo, c_hi = distill.class_range(args.num_classes, rank, world)
        pool = distill.RealPool.synthetic(args.num_classes, list(range(c_lo, c_hi)), args.pool_per_class, geo, device)
        return pool, args.num_classes, (c_lo, c_hi), None
    blob = torch.load(args.data_file, map_location="cpu")
    clips, labels = blob["clips"].float(), blob["labels"].long()
    num_classes = int(labels.max()) + 1
    c_lo, c_hi = distill.class_range(num_classes, rank, world)
    order = torch.argsort(labels, stable=True)
    clips, labels = clips[order], labels[order]
    counts = torch.bincount(labels, minlength=num_classes).tolist()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    a, b = int(starts[c_lo]), int(starts[c_hi])
    offsets = [int(s) - a for s in starts[:-1]]
    pool = distill.RealPool(clips[a:b].to(device), counts, offsets)
    return pool, num_classes, (c_lo, c_hi), driver.file_test_loader(blob)


def run(args, backend=None, log=None, shard: str = "class", exchange: str = "owner"):
    """``--memories`` decides the set-up -- data, trainer, ``per_class``, ``gather``, ``save`` and ``like_run_dc`` -- and nothing in
    the loop below it, which serves all three modes."""
    from . import checkpoint, distill, keyframes, plan, utils
    memories = getattr(args, 'memories', 'images')
    # the refusals that need no data, before any is loaded
    if memories == 'static' and args.spc < 1:
        raise ValueError("--spc %d: at least one memory per class" % args.spc)
    if memories == 'keyframes':
        keyframes.table(args.frames, args.key_frames, args.interp)
    rank, world, device = driver.start(use_cuda=backend is None)
    geo = plan.NetGeometry(args.frames, args.im_size, args.im_size)
    if memories == 'static':
        from .run_dc import StillTestLoader, load_stills
        pool, num_classes, (c_lo, c_hi), testloader = load_stills(args, rank, world, device)
    else:
        pool, num_classes, (c_lo, c_hi), testloader = load_data(args, rank, world, geo, device)
    if backend is None:
        backend = distill.HipBackend(geo, device, prec_real=args.prec_real, prec_syn=args.prec_syn)
    common = dict(momentum=0.5, rank=rank, world=world, shard=shard, exchange=exchange)
    hw = (3, args.im_size, args.im_size)

    def host_noise(per, *item):
        """``--init noise`` of the static and key-frame modes: drawn in full on the host from ``--seed``, so that every sharding
        starts from the same state, then the rows of this rank's memories (``DMTrainer.owned_classes``).  INTENDED to differ from
        the images mode, which draws its own rows on the device from ``4321 + rank``."""
        if args.init != 'noise':
            return None
        owned = list(range(c_lo, c_hi))
        if shard == "hybrid" and world > 1:
            block, _, split_owned = distill.hybrid_partition(num_classes, rank, world)
            owned = block + split_owned
        full = torch.randn((num_classes * per,) + item, generator=torch.Generator().manual_seed(args.seed))
        return full[[c * per + j for c in owned for j in range(per)]].to(device)

    # gather: () -> (all synthetic clips, all memories as the mode's file holds them), collectives on every rank;
    # save: (it, memories, best) -> the mode's file(s) of iteration ``it``
    like_run_dc = memories == 'static'
    per_class = args.spc if like_run_dc else args.ipc
    if memories == 'static':
        if testloader is not None:
            testloader = StillTestLoader(testloader, backend, device, args.frames)
        trainer = distill.StillDMTrainer(backend, pool, geo, num_classes, args.spc, args.batch_real, args.lr_img,
                                         static=host_noise(args.spc, *hw), **common)
        save_dir = os.path.join(args.save_path, "Static_DM", "%s_spc%d_%s" % (args.dataset, args.spc, args.lr_img))
        gather = lambda: (trainer.gather_syn(), trainer.gather_static())
        save = lambda it, static, best: checkpoint.save_static(save_dir, it, static, best=best)
    elif memories == 'keyframes':
        K = args.key_frames
        trainer = distill.KeyframeDMTrainer(backend, pool, geo, num_classes, args.ipc, args.batch_real, args.lr_img, key_frames=K,
                                            interp=args.interp, keys=host_noise(args.ipc, K, *hw), **common)
        save_dir = os.path.join(args.save_path, "Keyframes_DM", "%s_ipc%d_k%d_%s_%s" % (args.dataset, args.ipc, K, args.interp, args.lr_img))
        gather = lambda: (trainer.gather_syn(), trainer.gather_keys())
        save = lambda it, keys, best: checkpoint.save_keyframes(save_dir, it, keys, args.interp, args.frames, best=best)
    else:
        image_syn = None
        if args.init == 'noise':
            gen = torch.Generator(device=device); gen.manual_seed(4321 + rank)
            image_syn = torch.randn((c_hi - c_lo) * args.ipc, args.frames, *hw, device=device, generator=gen)
        trainer = distill.DMTrainer(backend, pool, num_classes, args.ipc, args.batch_real, args.lr_img, image_syn=image_syn, **common)
        save_dir = os.path.join(args.save_path, "Baseline_DM", "%s_ipc%d_%s" % (args.dataset, args.ipc, args.lr_img))
        gather = lambda: (trainer.gather_syn(),) * 2          # (the clips are the memories)
        save = lambda it, images, best: checkpoint.save_images(save_dir, it, images, best=best)

    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    log = driver.JsonLog(args.log_file, rank, log)
    evaluate = not args.no_eval and testloader is not None
    # Two cadences, both INTENDED.  Images and key frames: a round (the gathers; a file at a new best or a multiple of 1000) at every
    # evaluation iteration unless --no_eval, with or without test clips, and the seed is drawn and logged on the same condition;
    # --no_eval writes nothing.  Static is run_dc --memories static's: rounds and seed only where something is evaluated, but the
    # evaluation iterations that are multiples of 1000 write their file regardless -- the file is that stage's product.
    rounds = evaluate if like_run_dc else not args.no_eval
    eval_seed = None
    if args.eval_ranks == 'all' and rounds:
        eval_seed = driver.draw_eval_seed(args.eval_seed, rank, world)
        log.emit({"eval_ranks": "all", "eval_seed": eval_seed, "world": world})
    label_syn = torch.arange(num_classes).repeat_interleave(per_class)
    eval_its = set(np.arange(0, args.Iteration + 1, args.eval_it).tolist())
    t0 = time.time()
    for it in range(args.Iteration + 1):
        if it in eval_its and (rounds or (like_run_dc and it % 1000 == 0)):
            syn_all, memory_all = gather()
            if not like_run_dc:
                # INTENDED (run_dc has none): the gathers have waited already, but on a c8 two-stream backend every sync() counts
                # towards VD_RANGE_CHECK_EVERY, so this one decides when the real side's range is read
                trainer.sync()
            save_best = False
            if evaluate:
                save_best, pooled = driver.evaluate_round(
                    args, it, syn_all.detach().clone(), label_syn, 'none', args.lr_net, testloader, eval_pool, best_acc, best_std, log,
                    rank=rank, world=world, device=device, num_classes=num_classes,
                    pool_seed=None if eval_seed is None else eval_seed + it)
                for got in pooled:
                    log.emit({"step": it, "eval_pool": {"train_s": got["times"]["train_s"], "test_pass_s": got["times"]["test_pass_s"],
                                                        "assignment": got["assignment"]}})
            if rank == 0 and (save_best or it % 1000 == 0):
                save(it, memory_all, save_best)
        loss = trainer.global_loss(trainer.step(it, overlap=True))
        if it % 10 == 0 or it == args.Iteration:
            trainer.sync()
            log.emit({"step": it, "Loss": float(loss) / num_classes, "elapsed_s": round(time.time() - t0, 3)})
    trainer.sync()
    log.close()
    return trainer


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)


if __name__ == "__main__":
    main()
