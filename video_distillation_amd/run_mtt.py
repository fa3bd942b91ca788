#!/usr/bin/env python3
"""Trajectory-matching (MTT) distillation driver over the HIP hot path: the ``--method MTT`` branches of the reference's
distill_baseline.py:117-290 (``--memories images``: raw synthetic clips) and distill_s2d_ms.py:113-310 (``--memories s2d``:
static + dynamic memories and a hallucinator, "MTT+Ours"), each with its own parser's flag names and defaults for what that
branch reads.

    python -m video_distillation_amd.buffer  --dataset miniUCF101 --data_path D --buffer_path B --num_experts 30
    python -m video_distillation_amd.run_mtt --memories images --dataset miniUCF101 --data_path D --buffer_path B --ipc 1 \\
        --syn_steps 10 --expert_epochs 1 --max_start_epoch 10 --lr_img 1e4 --lr_teacher 0.01 --train_lr
    python -m video_distillation_amd.run_mtt --memories s2d --dataset miniUCF101 --data_path D --buffer_path B --vpc 1 --spc 2 \\
        --dpc 2 --path_static static.pt --no_train_static --lr_dynamic 1e4 --lr_hal 1e-3 --train_lr
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m video_distillation_amd.run_mtt ...

``static.pt``: ``python -m video_distillation_amd.run_dc --memories static --dataset singleUCF50 --data_path D --spc 2`` writes it
as ``static_best.pt`` / ``static_{it}.pt``; ``run_dm --memories static`` with the same flags learns it by distribution matching.

The expert trajectories of ``--buffer_path`` (``replay_buffer_N.pt`` of buffer.py) are served by ``experts.ExpertStore``:
``--expert_store host`` keeps one file at a time in pinned host memory, ``resident`` all of them in HBM; ``--buffer_walk all``
visits every file, ``reference`` only the first of the shuffle, as the reference's loops do (they never load a second file);
``--max_files`` bounds the files looked at.  ``--fused_flat on`` runs the flat-parameter arithmetic of an iteration on the
``vdt_`` kernels (include/vd_hip.h), ``off`` on torch expressions.  The walk is seeded (``--seed``) and the same on every rank;
every rank holds all memories and takes its share of each student batch (distill.MTTTrainer).

Data as ``run_dm`` (``--dataset synthetic``, the reference's frame folders, or ``--data_file f.pt``; the test loaders, like the
process setup, the log, the evaluation round and the project's own flags, are ``driver.py``'s); the real training clips are
read for ``--memories images --init real`` only: ``ipc`` random clips per class, drawn from ``--seed`` -- no resident pool of
the training set is built.  ``syn_lr`` starts at ``--lr_teacher`` and is trained only with ``--train_lr`` (``--lr_lr``);
evaluation trains its networks with ``lr_net = float(syn_lr)`` of that iteration (distill_baseline.py:157,
distill_s2d_ms.py:153), images with ``mode='none'`` testing every 200 epochs (at the end when ``--epoch_eval_train`` is below
200, where the reference's loop would never test), s2d with ``mode='multi-static'``.

Files (checkpoint.py): ``images_{it}.pt`` / ``images_best.pt`` under ``save_path/Baseline_MTT/{dataset}_ipc{ipc}_{lr_img}``;
``dynamic_{it}.pt``, ``hal_{it}.pt``, ``dynamic_best.pt`` / ``weights_best.pt`` -- and ``images_*`` when the static memory is
trained -- under ``save_path/S2D_multis_MTT/{dataset}_ipc{vpc}_{lr_dynamic}_{lr_hal}``; at evaluation iterations with a new best
accuracy and at multiples of 1000.  Logging: JSON lines with the reference's wandb keys (``Grand_Loss``,
``Grand_Loss/{start_epoch}``, ``Start_Epoch``, ``Synthetic_LR``, ``Accuracy/<model>``, ``Max_Accuracy/<model>``,
``Std/<model>``, ``Max_Std/<model>``); the grand losses stay on the device and are written out every 10 iterations and at the end.

Not here: the ``syn_{it}.png`` grid, wandb, evaluation architectures other than the hot path's.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import driver

# what the two parsers disagree on (distill_baseline.py:367-413, distill_s2d_ms.py:453-502)
DEFAULTS = {
    "images": {"eval_it": 50, "Iteration": 1000, "lr_teacher": 0.001, "buffer_path": None},
    "s2d": {"eval_it": 100, "Iteration": 15000, "lr_teacher": 0.01, "buffer_path": "./buffers"},
}


def build_parser(memories: str = "images"):
    d = DEFAULTS[memories]
    p = argparse.ArgumentParser(description="MTT distillation on MI355X (--memories %s)" % memories)
    p.add_argument('--memories', type=str, default=memories, choices=[memories],
                   help="images: the MTT branch of distill_baseline.py; s2d: that of distill_s2d_ms.py (main() reads this flag "
                        "first and builds the parser with that script's defaults)")
    p.add_argument('--dataset', type=str, default='miniUCF101')
    p.add_argument('--method', type=str, default='MTT', choices=['MTT'])
    p.add_argument('--model', type=str, default='ConvNet3D')
    p.add_argument('--eval_mode', type=str, default='S')
    p.add_argument('--num_eval', type=int, default=5)
    p.add_argument('--eval_it', type=int, default=d["eval_it"])
    p.add_argument('--epoch_eval_train', type=int, default=1000)
    p.add_argument('--Iteration', type=int, default=d["Iteration"])
    p.add_argument('--lr_lr', type=float, default=1e-5, help='learning rate of syn_lr (with --train_lr)')
    p.add_argument('--lr_teacher', type=float, default=d["lr_teacher"], help='initial syn_lr')
    p.add_argument('--train_lr', action='store_true', help='train syn_lr')
    p.add_argument('--batch_syn', type=int, default=None, help='student batch (default: num_classes * ipc, or * vpc)')
    p.add_argument('--batch_train', type=int, default=256)
    p.add_argument('--expert_epochs', type=int, default=3)
    p.add_argument('--syn_steps', type=int, default=64)
    p.add_argument('--max_start_epoch', type=int, default=25)
    p.add_argument('--buffer_path', type=str, default=d["buffer_path"])
    p.add_argument('--data_path', type=str, default='distill_utils/data')
    p.add_argument('--num_workers', type=int, default=8)
    p.add_argument('--preload', action='store_true', help='accepted; no effect (the loop reads no real clips)')
    p.add_argument('--save_path', type=str, default='./logged_files')
    p.add_argument('--frames', type=int, default=16)
    if memories == "images":
        p.add_argument('--ipc', type=int, default=1)
        p.add_argument('--lr_img', type=float, default=1)
        p.add_argument('--init', type=str, default='real', choices=['noise', 'real'])
    else:
        p.add_argument('--vpc', type=int, default=5, help='synthetic videos per class composed in a step')
        p.add_argument('--spc', type=int, default=10, help='static memories per class')
        p.add_argument('--dpc', type=int, default=1, help="dynamic memories per class (the reference's default; needs >= 2 * vpc)")
        p.add_argument('--lr_static', type=float, default=100)
        p.add_argument('--lr_dynamic', type=float, default=0.01)
        p.add_argument('--lr_hal', type=float, default=0.01)
        p.add_argument('--no_train_static', action='store_true', help='do not train the static memory')
        p.add_argument('--path_static', type=str, default=None, help='static memory file: {"image": (C*spc,3,H,W)}')
        p.add_argument('--n_hal', type=int, default=1, help='number of hallucinators (the first is trained)')
        p.add_argument('--startIt', type=int, default=0, help='first evaluation iteration')
    # the project's own
    driver.add_data_flags(p)
    driver.add_eval_flags(p)
    p.add_argument('--seed', type=int, default=0, help='seed of the expert walk, the noise memories, the real-clip draw and the hallucinators')
    p.add_argument('--expert_store', type=str, default='host', choices=['host', 'resident'],
                   help="host: one buffer file at a time in pinned host memory, two rows copied per iteration; resident: every "
                        "file of the walk in HBM")
    p.add_argument('--buffer_walk', type=str, default='all', choices=['all', 'reference'],
                   help="all: every buffer file in shuffled order; reference: only the first file of the shuffle, as the "
                        "reference's loops do")
    p.add_argument('--max_files', type=int, default=None, help='use the first N buffer files only')
    p.add_argument('--fused_flat', type=str, default='on', choices=['on', 'off'],
                   help="on: the flat-parameter chain on the vdt_ kernels (fp64 fixed-order sums); off: torch expressions")
    return p


def load_data(args, rank: int, device):
    """-> (num_classes, clips_of(indices) or None, labels of the training items or None, testloader or None).  Nothing of
    the training set is decoded or uploaded here: ``clips_of`` reads the few items ``--init real`` asks for."""
    if args.data_file is None and args.dataset != 'synthetic':
        from . import dataset as D
        _, _, num_classes, _, _, _, dst_train, dst_test, testloader = D.get_dataset(args.dataset, args.data_path,
                                                                                    img_size=(args.im_size, args.im_size))
        if not args.no_eval:
            testloader = driver.folder_test_loader(args, rank, device, dst_test, testloader)
        return num_classes, (lambda idx: torch.stack([dst_train[int(i)][0] for i in idx])), list(dst_train.labels), testloader
    if args.data_file is None:
        C = args.num_classes

        def randn_clips(idx):          # the synthetic data set is randn clips; item i is seeded by i
            return torch.stack([torch.randn((args.frames, 3, args.im_size, args.im_size),
                                            generator=torch.Generator().manual_seed(1234 + int(i))) for i in idx])
        return C, randn_clips, [c for c in range(C) for _ in range(4)], None
    blob = torch.load(args.data_file, map_location="cpu")
    labels = blob["labels"].long()
    num_classes = int(labels.max()) + 1
    return (num_classes, (lambda idx: blob["clips"][torch.as_tensor(idx, dtype=torch.int64)].float()), labels.tolist(),
            driver.file_test_loader(blob))


def real_init(clips_of, labels, num_classes: int, ipc: int, seed: int) -> torch.Tensor:
    """``ipc`` random training clips per class, class after class (distill_baseline.py:84-100) -- drawn from ``seed``, so every
    rank starts from the same clips."""
    from .dataset import indices_class
    per_class = indices_class(labels, num_classes)
    rng = np.random.default_rng([seed, 41])
    chosen = []
    for c in range(num_classes):
        if len(per_class[c]) < ipc:
            raise ValueError("--init real --ipc %d: class %d has %d training clips" % (ipc, c, len(per_class[c])))
        chosen += [int(i) for i in rng.permutation(per_class[c])[:ipc]]
    return clips_of(chosen)


def run(args, ops=None, log=None):
    from . import checkpoint, distill, experts, plan, run_s2d, utils
    s2d = args.memories == "s2d"
    if s2d:
        run_s2d.check_settings(args)
    if args.buffer_path is None:
        raise ValueError("--buffer_path: the directory of the expert trajectories (replay_buffer_N.pt, written by "
                         "video_distillation_amd.buffer)")
    rank, world, device = driver.start(use_cuda=ops is None)
    geo = plan.NetGeometry(args.frames, args.im_size, args.im_size)
    num_classes, clips_of, train_labels, testloader = load_data(args, rank, device)
    per_class = args.vpc if s2d else args.ipc
    batch_syn = args.batch_syn if args.batch_syn is not None else num_classes * per_class
    # every rank builds the same store: the walk comes from --seed alone
    store = experts.ExpertStore(args.buffer_path, num_classes, device, mode=args.expert_store, walk=args.buffer_walk,
                                seed=args.seed, max_files=args.max_files)
    store.check(args.max_start_epoch, args.expert_epochs)
    if ops is None:
        ops = distill.HipMTTOps(geo, num_classes, device, batch_hint=max(1, batch_syn // max(world, 1)),
                                fused_flat=(args.fused_flat == 'on'))
    hw = (args.im_size, args.im_size)
    hals = None
    if s2d:
        static, dynamic, hals = run_s2d.initial_state(args, num_classes)
        hals = hals.to(device)
        train_static = not args.no_train_static
        trainer = distill.S2DMTTTrainer(ops, num_classes, args.vpc, args.spc, args.dpc, static.to(device), dynamic.to(device),
                                        hals[0].encoder.weight.detach(), hals[0].encoder.bias.detach(), syn_lr=args.lr_teacher,
                                        lr_dynamic=args.lr_dynamic, lr_hal=args.lr_hal, lr_lr=args.lr_lr, syn_steps=args.syn_steps,
                                        batch_syn=batch_syn, expert_epochs=args.expert_epochs, max_start_epoch=args.max_start_epoch,
                                        lr_static=args.lr_static, train_static=train_static, momentum=0.95, rank=rank, world=world,
                                        train_lr=args.train_lr)
        del static, dynamic
        save_dir = os.path.join(args.save_path, "S2D_multis_MTT", "%s_ipc%d_%s_%s" % (args.dataset, args.vpc, args.lr_dynamic, args.lr_hal))
        start_it = args.startIt
    else:
        if args.init == 'real':
            image_syn = real_init(clips_of, train_labels, num_classes, args.ipc, args.seed)
        else:
            image_syn = torch.randn((num_classes * args.ipc, args.frames, 3) + hw, generator=torch.Generator().manual_seed(args.seed))
        if tuple(image_syn.shape) != (num_classes * args.ipc, args.frames, 3) + hw:
            raise ValueError("the training clips are %s; --frames %d --im_size %d needs %s"
                             % (tuple(image_syn.shape[1:]), args.frames, args.im_size, (args.frames, 3) + hw))
        label_syn = torch.arange(num_classes).repeat_interleave(args.ipc)
        trainer = distill.MTTTrainer(ops, num_classes, image_syn.to(device), label_syn.to(device), syn_lr=args.lr_teacher,
                                     lr_img=args.lr_img, lr_lr=args.lr_lr, syn_steps=args.syn_steps, batch_syn=batch_syn,
                                     expert_epochs=args.expert_epochs, max_start_epoch=args.max_start_epoch, momentum=0.5,
                                     rank=rank, world=world, train_lr=args.train_lr)
        del image_syn
        save_dir = os.path.join(args.save_path, "Baseline_MTT", "%s_ipc%d_%s" % (args.dataset, args.ipc, args.lr_img))
        start_it = 0
    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    log = driver.JsonLog(args.log_file, rank, log)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    evaluate = not args.no_eval and testloader is not None
    eval_seed = None
    if args.eval_ranks == 'all' and evaluate:
        eval_seed = driver.draw_eval_seed(args.eval_seed, rank, world)
        log.emit({"eval_ranks": "all", "eval_seed": eval_seed, "world": world})
    log.emit({"expert_store": store.mode, "buffer_walk": store.walk, "buffer_files": len(store.files), "expert_epochs_per_trajectory": store.epochs,
          "fused_flat": getattr(ops, "flat", None) is not None, "batch_syn": batch_syn})
    test_freq = 200 if args.epoch_eval_train >= 200 else None          # (the reference's loop never tests below 200 epochs)
    eval_its = set(np.arange(start_it, args.Iteration + 1, args.eval_it).tolist())
    pending = []          # (it, start_epoch, grand loss on the device, syn_lr on the device before the step)
    t0 = time.time()

    def flush():
        sync()
        for it_, start_, grand_, lr_ in pending:
            g = float(grand_)
            log.emit({"step": it_, "Grand_Loss": g, "Grand_Loss/%d" % start_: g, "Start_Epoch": start_, "Synthetic_LR": float(lr_),
                      "elapsed_s": round(time.time() - t0, 3)})
        del pending[:]

    for it in range(args.Iteration + 1):
        if it in eval_its and (evaluate or it % 1000 == 0):
            flush()
            if s2d:
                static_all = trainer.static
                dynamic_all = trainer.dynamic.view((num_classes, args.dpc) + tuple(trainer.dynamic.shape[1:]))
                with torch.no_grad():          # the reference trains hals[0] only (:247) and evaluates / saves all n_hal
                    hals[0].encoder.weight.copy_(trainer.hal_w.view_as(hals[0].encoder.weight))
                    hals[0].encoder.bias.copy_(trainer.hal_b)
            save_this_it = False
            if evaluate:          # networks trained with the syn_lr of this iteration; images test every 200 epochs
                if s2d:
                    memories, labels_eval, mode = [static_all.detach().clone(), dynamic_all.detach().clone(), hals], None, 'multi-static'
                else:
                    memories, labels_eval, mode = trainer.image_syn.detach().clone(), label_syn, 'none'
                save_this_it, _ = driver.evaluate_round(
                    args, it, memories, labels_eval, mode, float(trainer.syn_lr), testloader, eval_pool, best_acc, best_std, log,
                    rank=rank, world=world, device=device, num_classes=num_classes,
                    pool_seed=None if eval_seed is None else eval_seed + it, test_freq=None if s2d else test_freq)
                del memories
            if rank == 0 and (save_this_it or it % 1000 == 0):
                if s2d:
                    checkpoint.save_s2d(save_dir, it, dynamic_all, [h.encoder.weight for h in hals], [h.encoder.bias for h in hals],
                                        best=save_this_it)
                    if train_static:
                        checkpoint.save_images(save_dir, it, static_all, best=save_this_it)
                else:
                    checkpoint.save_images(save_dir, it, trainer.image_syn, best=save_this_it)
        lr_before = trainer.syn_lr
        grand = trainer.step(it, store.next())
        pending.append((it, trainer.last_start_epoch, grand, lr_before))
        if it % 10 == 0 or it == args.Iteration:
            flush()
    flush()
    log.close()
    return trainer


def main(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--memories', type=str, default='images', choices=sorted(DEFAULTS))
    memories = pre.parse_known_args(argv)[0].memories
    run(build_parser(memories).parse_args(argv))


if __name__ == "__main__":
    main()
