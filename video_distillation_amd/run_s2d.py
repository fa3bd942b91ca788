#!/usr/bin/env python3
"""Static + dynamic memory (s2d) DM distillation driver over the HIP hot path: the ``--method DM`` branch of the reference's
distill_s2d_ms.py:312-445, with its flag names and defaults for everything that branch reads.

    python -m video_distillation_amd.run_s2d --dataset miniUCF101 --data_path D --path_static static.pt --no_train_static \\
        --vpc 1 --spc 2 --dpc 2 --lr_dynamic=1e-3 --lr_hal=1e-5
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m video_distillation_amd.run_s2d ...

``static.pt`` is what ``python -m video_distillation_amd.run_dc --memories static --dataset singleUCF50 --data_path D --spc 2``
writes as ``static_best.pt`` / ``static_{it}.pt`` -- or ``run_dm --memories static`` with the same flags, the same stage by
distribution matching -- (or the file the reference offers for download).

Data as ``run_dm`` (``run_dm.load_data``: ``--dataset synthetic``, the reference's frame folders, or ``--data_file f.pt``); process
setup, log, evaluation round and the project's own flags are ``driver.py``'s.  The static memory comes
from ``--path_static`` (a dict with key "image", (C*spc,3,H,W)) or seeded noise; the dynamic memory (C,dpc,T,1,H,W) is seeded
noise drawn in full on the host, the same on every rank, of which the trainer keeps its classes -- every sharding starts from
the same state.  ``n_hal`` hallucinators are created; as in the reference only the first is trained (``hal_idx = 0``,
:407), all are evaluated (``MultiStaticSharedDataset`` picks one per item) and saved.  Evaluation trains its networks with
``lr_net = --lr_teacher`` (the reference sets ``args.lr_net = syn_lr``, :341; its parser has no ``--lr_net``).

Files under ``save_path/S2D_multis_DM/{dataset}_ipc{vpc}_{lr_dynamic}_{lr_hal}`` (checkpoint.py): ``dynamic_{it}.pt``,
``hal_{it}.pt``, with a new best accuracy ``dynamic_best.pt`` / ``weights_best.pt``, and ``images_{it}.pt`` /
``images_best.pt`` (the static memory) only when it is trained.  Logging: JSON lines with the reference's wandb keys.

Not here: the MTT branch (its driver is ``video_distillation_amd.run_mtt --memories s2d``), the ``syn_{it}.png`` grid, wandb.  ``--train_lr`` /
``--lr_lr`` are left out: the DM branch steps ``optimizer_lr`` on a tensor no DM loss depends on.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import driver
from .run_dm import load_data


def build_parser():
    p = argparse.ArgumentParser(description="s2d (static + dynamic memory) DM distillation on MI355X")
    p.add_argument('--dataset', type=str, default='miniUCF101')
    p.add_argument('--method', type=str, default='DM', choices=['DM'])
    p.add_argument('--model', type=str, default='ConvNet3D')
    p.add_argument('--spc', type=int, default=10, help='static memories per class')
    p.add_argument('--dpc', type=int, default=1, help="dynamic memories per class (the reference's default; needs >= 2 * vpc)")
    p.add_argument('--vpc', type=int, default=5, help='synthetic videos per class composed in a step')
    p.add_argument('--eval_mode', type=str, default='S')
    p.add_argument('--num_eval', type=int, default=5)
    p.add_argument('--eval_it', type=int, default=100)
    p.add_argument('--epoch_eval_train', type=int, default=1000)
    p.add_argument('--Iteration', type=int, default=15000)
    p.add_argument('--no_train_static', action='store_true', help='do not train the static memory')
    p.add_argument('--path_static', type=str, default=None, help='static memory file: {"image": (C*spc,3,H,W)}')
    p.add_argument('--lr_static', type=float, default=100)
    p.add_argument('--lr_dynamic', type=float, default=0.01)
    p.add_argument('--lr_teacher', type=float, default=0.01, help='learning rate of the evaluation networks')
    p.add_argument('--lr_hal', type=float, default=0.01)
    p.add_argument('--batch_real', type=int, default=256)
    p.add_argument('--batch_train', type=int, default=256)
    p.add_argument('--data_path', type=str, default='distill_utils/data')
    p.add_argument('--preload', action='store_true', help='accepted; no effect (the real pool is always resident)')
    p.add_argument('--n_hal', type=int, default=1, help='number of hallucinators (the first is trained)')
    p.add_argument('--frames', type=int, default=16)
    p.add_argument('--num_workers', type=int, default=8, help='decode threads of the preload')
    p.add_argument('--startIt', type=int, default=0, help='first evaluation iteration')
    p.add_argument('--save_path', type=str, default='./logged_files')
    p.add_argument('--seed', type=int, default=0, help='seed of the noise memories and of the hallucinators')
    # the project's own
    p.add_argument('--pool_per_class', type=int, default=93, help='synthetic data only')
    p.add_argument('--prec_real', type=str, default='f16')
    p.add_argument('--prec_syn', type=str, default='f16x3')
    driver.add_data_flags(p)
    driver.add_eval_flags(p)
    return p


def check_settings(args) -> None:
    """Reject what the index formulas would run out of range on, before anything is loaded."""
    if args.vpc < 1 or args.dpc < 2 * args.vpc or args.spc < 2 * args.vpc:
        raise ValueError("--vpc %d --spc %d --dpc %d index out of range: a step composes video v of a class from dynamic memory "
                         "2*v + {0,1} and static memory spc*label + 2*v + {0,1} (distill_s2d_ms.py:405-406), so dpc >= 2*vpc and "
                         "spc >= 2*vpc are needed (the reference's default --dpc 1 with --vpc 5 indexes out of range)"
                         % (args.vpc, args.spc, args.dpc))
    if not args.no_eval:
        if args.spc not in (2, 10):
            raise ValueError("--spc %d: evaluation composes its clips with MultiStaticSharedDataset, which knows spc 2 (vpc 1) and "
                             "spc 10 (vpc 5) only (utils.py:462-496); pass one of those, or --no_eval -- also where the data has no test clips "
                             "(--dataset synthetic, a --data_file without test_clips): this check runs before the data is read"
                             % args.spc)
        if args.spc == 10 and args.dpc < 10:
            raise ValueError("--spc 10 --dpc %d index out of range in evaluation: MultiStaticSharedDataset reads dynamic memory "
                             "2*idx + {0,1}, idx < 5 (utils.py:475), so dpc >= 10 is needed" % args.dpc)
    if args.n_hal < 1:
        raise ValueError("--n_hal %d: at least one hallucinator" % args.n_hal)


def initial_state(args, num_classes: int):
    """-> (static (C*spc,3,H,W), dynamic (C,dpc,T,1,H,W), ModuleList of n_hal Conv3DNet), all on the host and the same on every
    rank: the dynamic memory from a generator seeded ``--seed``, the static memory from ``--path_static`` or a generator seeded
    ``--seed + 1``, the hallucinators created after ``torch.manual_seed(--seed)``."""
    from . import checkpoint, utils
    hw = (args.im_size, args.im_size)
    dynamic = torch.randn((num_classes, args.dpc, args.frames, 1) + hw, generator=torch.Generator().manual_seed(args.seed))
    if args.path_static is not None:
        static = checkpoint.load_static(args.path_static)
        if tuple(static.shape) != (num_classes * args.spc, 3) + hw:
            raise ValueError("%s holds a static memory of shape %s; --spc %d on %d classes at %dx%d needs %s"
                             % (args.path_static, tuple(static.shape), args.spc, num_classes, hw[0], hw[1],
                                (num_classes * args.spc, 3) + hw))
    else:
        static = torch.randn((num_classes * args.spc, 3) + hw, generator=torch.Generator().manual_seed(args.seed + 1))
    torch.manual_seed(args.seed)
    hals = torch.nn.ModuleList([utils.Conv3DNet() for _ in range(args.n_hal)])
    return static, dynamic, hals


def run(args, backend=None, log=None):
    from . import checkpoint, distill, plan, utils
    check_settings(args)
    rank, world, device = driver.start(use_cuda=backend is None)
    geo = plan.NetGeometry(args.frames, args.im_size, args.im_size)
    pool, num_classes, _, testloader = load_data(args, rank, world, geo, device)
    if backend is None:
        backend = distill.HipBackend(geo, device, prec_real=args.prec_real, prec_syn=args.prec_syn)
    static, dynamic, hals = initial_state(args, num_classes)
    hals = hals.to(device)
    train_static = not args.no_train_static
    trainer = distill.S2DTrainer(backend, pool, num_classes, args.vpc, args.spc, args.dpc, args.batch_real, static.to(device),
                                 dynamic.to(device), hals[0].encoder.weight.detach(), hals[0].encoder.bias.detach(),
                                 lr_dynamic=args.lr_dynamic, lr_hal=args.lr_hal, lr_static=args.lr_static,
                                 train_static=train_static, momentum=0.95, rank=rank, world=world)
    del static, dynamic
    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    save_dir = os.path.join(args.save_path, "S2D_multis_DM", "%s_ipc%d_%s_%s" % (args.dataset, args.vpc, args.lr_dynamic, args.lr_hal))
    log = driver.JsonLog(args.log_file, rank, log)
    evaluate = not args.no_eval and testloader is not None
    eval_seed = None
    if args.eval_ranks == 'all' and evaluate:
        eval_seed = driver.draw_eval_seed(args.eval_seed, rank, world)
        log.emit({"eval_ranks": "all", "eval_seed": eval_seed, "world": world})
    eval_its = set(np.arange(args.startIt, args.Iteration + 1, args.eval_it).tolist())
    t0 = time.time()
    for it in range(args.Iteration + 1):
        if it in eval_its and (evaluate or it % 1000 == 0):
            static_all, dynamic_all = trainer.gather_memories()          # (a collective: every rank, whoever evaluates or saves)
            with torch.no_grad():          # the reference trains hals[0] only (:407) and evaluates / saves all n_hal
                hals[0].encoder.weight.copy_(trainer.hal_w.view_as(hals[0].encoder.weight))
                hals[0].encoder.bias.copy_(trainer.hal_b)
            save_this_it = False
            if evaluate:
                save_this_it, _ = driver.evaluate_round(
                    args, it, [static_all.detach().clone(), dynamic_all.detach().clone(), hals], None, 'multi-static', args.lr_teacher,
                    testloader, eval_pool, best_acc, best_std, log, rank=rank, world=world, device=device, num_classes=num_classes,
                    pool_seed=None if eval_seed is None else eval_seed + it)
            if rank == 0 and (save_this_it or it % 1000 == 0):
                checkpoint.save_s2d(save_dir, it, dynamic_all, [h.encoder.weight for h in hals], [h.encoder.bias for h in hals],
                                    best=save_this_it)
                if train_static:
                    checkpoint.save_images(save_dir, it, static_all, best=save_this_it)
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
