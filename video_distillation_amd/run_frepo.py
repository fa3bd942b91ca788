#!/usr/bin/env python3
"""FRePo(+Ours) distillation driver over the HIP hot path: the reference's FRePo/script/distill_s2d.py with its parser's flag
names and defaults (:393-428).

    python -m video_distillation_amd.run_frepo --memories s2d --dataset miniUCF101 --data_path D --path_static static.pt \\
        --num_prototypes_per_class 1 --dpc 1 --n_hal 1 --lr_d 1e2 --lr_h 1e-3
    python -m video_distillation_amd.run_frepo --memories images --dataset miniUCF101 --data_path D --init real

``--memories s2d`` is the script: a static memory (``--path_static``, or noise; never trained), a dynamic memory per class and
``--n_hal`` hallucinators compose the synthetic clips (frepo.S2DSynData); ``--memories images`` is plain FRePo on whole clips
(frepo.SynData, ``--init real|noise``).  A pool of ``--num_nn_state`` networks is trained online on the synthetic set
(frepo.PoolElement); per iteration one of them embeds 512 real clips and the synthetic set, the kernel ridge predictor
(nfr.nfr, fp64) gives the loss, Adam moves the synthetic set (frepo.FRePoTrainer).

Data as ``run_mtt`` (``--dataset synthetic``, the reference's frame folders, or ``--data_file f.pt`` under any ``--dataset``
name); the real batches are 512 clips, shuffled and infinite, labels ``one_hot - 1 / C``; the synthetic labels are
``(one_hot - 1 / C) / sqrt(C / 10)``.

Files: at ``it == 1`` and every 400 iterations ``dynamic_{it}.pt`` (C, dpc, T, 1, H, W), ``hal_{it}.pt`` (the ModuleList's
state dict, what ``checkpoint.load_hallucinators`` reads) and ``y_syn_{it}.pt`` under ``save_path/S2D_FRePo/{dataset}_ipc{n}_
{lr_d}_{lr_h}``; ``images_{it}.pt`` and ``y_syn_{it}.pt`` under ``save_path/Baseline_FRePo/...``; with a new best accuracy
``dynamic_best.pt`` / ``weights_best.pt`` / ``y_syn_best.pt``, or ``images_best.pt`` / ``y_syn_best.pt``.  Evaluation at
``np.arange(startIt, Iteration + 1, eval_it)``: ``--num_eval`` networks through FRePo's own ``evaluate_synset`` (AdamW, MSE on
the soft labels).  Logging: JSON lines (driver.JsonLog) with ``Loss``, ``ln_loss``, ``lb_loss`` and ``lr`` per step and the
reference's four ``Accuracy/...`` keys per evaluation; the losses stay on the device and are written out every 10 iterations.

Not here: more than one rank (refused), ``--eval_ranks all`` and ``--test_videos resident`` (refused), wandb, ``--init
real-all``, evaluation architectures other than the hot path's.  ``--data_path`` defaults to the other drivers' relative
directory, not to the reference author's absolute one.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import driver

STEPS_PER_SAVE = 400
STEPS_PER_EVAL = 10000
REAL_BATCH = 512


def build_parser():
    p = argparse.ArgumentParser(description="FRePo(+Ours) distillation on MI355X")
    p.add_argument('--memories', type=str, default='s2d', choices=['s2d', 'images'])
    p.add_argument('--dataset', type=str, default='miniUCF101')
    p.add_argument('--method', type=str, default='FRePo', choices=['FRePo'])
    p.add_argument('--model', type=str, default='ConvNet3D')
    p.add_argument('--num_prototypes_per_class', type=int, default=1, help='synthetic clip(s) per class')
    p.add_argument('--num_eval', type=int, default=5)
    p.add_argument('--eval_it', type=int, default=1000)
    p.add_argument('--eval_mode', type=str, default='S')
    p.add_argument('--epoch_eval_train', type=int, default=500)
    p.add_argument('--batch_train', type=int, default=None, help='default: min(number of synthetic clips, 500)')
    p.add_argument('--batch_syn', type=int, default=512, help='accepted; the script never reads it')
    p.add_argument('--init', type=str, default='real', choices=['noise', 'real'], help='--memories images: the initial clips')
    p.add_argument('--data_path', type=str, default='distill_utils/data')
    p.add_argument('--startIt', type=int, default=0)
    p.add_argument('--Iteration', type=int, default=10000)
    p.add_argument('--max_online_updates', type=int, default=100)
    p.add_argument('--num_nn_state', type=int, default=10)
    p.add_argument('--learn_label', action='store_true')
    p.add_argument('--lr_d', type=float, default=1e2, help='learning rate of the dynamic memory (images: of the clips)')
    p.add_argument('--lr_h', type=float, default=0.001, help='learning rate of the hallucinators and the labels')
    p.add_argument('--lr_net', type=float, default=0.001)
    p.add_argument('--num_workers', type=int, default=16)
    p.add_argument('--path_static', type=str, default=None, help='static memory file: {"image": (C*n,3,H,W)}')
    p.add_argument('--dpc', type=int, default=1)
    p.add_argument('--spc', type=int, default=1)
    p.add_argument('--n_hal', type=int, default=1)
    p.add_argument('--frames', type=int, default=16)
    # the project's own
    driver.add_data_flags(p)
    driver.add_eval_flags(p)
    p.add_argument('--seed', type=int, default=0, help='seed of the noise memories, the real-clip draw and the hallucinators')
    p.add_argument('--save_path', type=str, default='./logged_files')
    return p


def check_settings(args) -> None:
    """What the driver refuses, before anything touches a device."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("run_frepo runs on a single rank (WORLD_SIZE is %s)" % os.environ.get("WORLD_SIZE"))
    if args.eval_ranks != 'rank0':
        raise ValueError("run_frepo: --eval_ranks all is not built for FRePo's evaluate_synset")
    if args.test_videos != 'host':
        raise ValueError("run_frepo: --test_videos resident is not built for this driver")
    if args.memories == 's2d' and args.dpc != args.num_prototypes_per_class:
        raise ValueError("--memories s2d composes dpc clips per class from num_prototypes_per_class static memories each: "
                         "--dpc %d != --num_prototypes_per_class %d" % (args.dpc, args.num_prototypes_per_class))


class _RealItems(torch.utils.data.Dataset):
    def __init__(self, clips_of, labels, num_classes):
        from . import frepo
        self.clips_of = clips_of
        self.labels = frepo.soft_labels(torch.as_tensor(labels, dtype=torch.int64), num_classes)

    def __len__(self):
        return int(self.labels.shape[0])

    def __getitem__(self, i):
        return self.clips_of([i])[0].float(), self.labels[i]


def real_batches(clips_of, labels, num_classes: int, workers: int):
    """The reference's InfiniteDataLoader (:29-45, :260): shuffled batches of 512 (clips, soft labels), epoch after epoch."""
    loader = torch.utils.data.DataLoader(_RealItems(clips_of, labels, num_classes), batch_size=REAL_BATCH, shuffle=True,
                                         num_workers=workers)
    while True:
        for batch in loader:
            yield batch


def build_syndata(args, num_classes: int, clips_of, train_labels, device):
    from . import checkpoint, frepo, run_mtt, utils
    n, hw = num_classes * args.num_prototypes_per_class, (args.im_size, args.im_size)
    gen = torch.Generator().manual_seed(args.seed)
    y_syn = frepo.soft_labels(torch.arange(num_classes).repeat_interleave(args.num_prototypes_per_class), num_classes,
                              frepo.y_scale(num_classes))
    if args.memories == 'images':
        if args.init == 'real':
            x = run_mtt.real_init(clips_of, train_labels, num_classes, args.num_prototypes_per_class, args.seed).float()
        else:
            x = torch.randn((n, args.frames, 3) + hw, generator=gen)
        if tuple(x.shape) != (n, args.frames, 3) + hw:
            raise ValueError("the training clips are %s; --frames %d --im_size %d needs %s"
                             % (tuple(x.shape[1:]), args.frames, args.im_size, (args.frames, 3) + hw))
        return frepo.SynData(x, y_syn, learn_label=args.learn_label).to(device)
    static = torch.randn((n, 3) + hw, generator=gen)
    dynamic = torch.randn((num_classes, args.dpc, args.frames, 1) + hw, generator=gen)
    if args.path_static is not None:
        static = checkpoint.load_static(args.path_static)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(args.seed)
        hals = torch.nn.ModuleList([utils.Conv3DNet() for _ in range(args.n_hal)])
    return frepo.S2DSynData(static, dynamic, hals, y_syn, learn_label=args.learn_label).to(device)


def save(save_dir: str, tag, syndata, s2d: bool) -> None:
    os.makedirs(save_dir, exist_ok=True)
    best = tag == "best"
    if s2d:
        torch.save(syndata.dynamic.detach().cpu(), os.path.join(save_dir, "dynamic_%s.pt" % tag))
        torch.save({k: v.detach().cpu() for k, v in syndata.hallucinator.state_dict().items()},
                   os.path.join(save_dir, "weights_best.pt" if best else "hal_%s.pt" % tag))
    else:
        torch.save(syndata.x_syn.detach().cpu(), os.path.join(save_dir, "images_%s.pt" % tag))
    torch.save(syndata.y_syn.detach().cpu(), os.path.join(save_dir, "y_syn_%s.pt" % tag))


def run(args, log=None):
    check_settings(args)
    from . import frepo, run_mtt, utils
    rank, world, device = driver.start(use_cuda=True)
    s2d = args.memories == 's2d'
    num_classes, clips_of, train_labels, testloader = run_mtt.load_data(args, rank, device)
    hw = (args.im_size, args.im_size)
    num_prototypes = args.num_prototypes_per_class * num_classes
    batch_train = min(num_prototypes, 500) if args.batch_train is None else args.batch_train
    syndata = build_syndata(args, num_classes, clips_of, train_labels, device)
    synopt, synsch = frepo.syn_optimizer(syndata, args.lr_d, args.lr_h, args.Iteration)
    get_model = lambda: utils.get_network(args.model, 3, num_classes, hw, frames=args.frames, dist=False).to(device)
    pools = frepo.build_pool(get_model, args.lr_net, args.max_online_updates, args.num_nn_state, device)
    trainer = frepo.FRePoTrainer(syndata, pools, synopt, synsch)
    workers = args.num_workers if (args.data_file is None and args.dataset != 'synthetic') else 0
    batches = real_batches(clips_of, train_labels, num_classes, workers)
    save_dir = os.path.join(args.save_path, "S2D_FRePo" if s2d else "Baseline_FRePo",
                            "%s_ipc%d_%s_%s" % (args.dataset, args.num_prototypes_per_class, args.lr_d, args.lr_h))
    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    log = driver.JsonLog(args.log_file, rank, log)
    evaluate = not args.no_eval and testloader is not None
    eval_its = set(np.arange(args.startIt, args.Iteration + 1, args.eval_it).tolist())
    eargs = argparse.Namespace(device=str(device), lr_net=args.lr_net, epoch_eval_train=args.epoch_eval_train, batch_train=batch_train)
    pending = []          # (it, loss, ln_loss, lb_loss on the device, lr_h of the step)
    t0 = time.time()

    def flush():
        if pending:
            torch.cuda.synchronize(device)
        for it_, loss_, ln_, lb_, lr_ in pending:
            log.emit({"step": it_, "Loss": float(loss_), "ln_loss": float(ln_), "lb_loss": float(lb_), "lr": lr_,
                      "elapsed_s": round(time.time() - t0, 3)})
        del pending[:]

    for it in range(1, args.Iteration + 1):
        if evaluate and (it in eval_its or it % STEPS_PER_EVAL == 0):
            flush()
            for model_eval in eval_pool:
                accs = []
                for it_eval in range(args.num_eval):
                    net_eval = utils.get_network(model_eval, 3, num_classes, hw, frames=args.frames, dist=False).to(device)
                    with torch.no_grad():
                        x_eval, y_eval = syndata.value()          # (s2d: a fresh draw of the hallucinators, as the reference)
                    _, _, acc_test = frepo.evaluate_synset(it_eval, net_eval, x_eval.clone(), y_eval.clone(), testloader, eargs,
                                                           num_classes)
                    accs.append(acc_test)
                mean, std = float(np.mean(accs)), float(np.std(accs))
                if mean > best_acc[model_eval]:
                    best_acc[model_eval], best_std[model_eval] = mean, std
                    save(save_dir, "best", syndata, s2d)
                log.emit({"step": it, "Accuracy/%s" % model_eval: mean, "Max_Accuracy/%s" % model_eval: best_acc[model_eval],
                          "Std/%s" % model_eval: std, "Max_Std/%s" % model_eval: best_std[model_eval]})
        if it % STEPS_PER_SAVE == 0 or it == 1:
            save(save_dir, it, syndata, s2d)
        x_target, y_target = next(batches)
        lr_now = float(synsch.get_last_lr()[-1])
        loss, ln_loss, lb_loss = trainer.step(x_target.to(device), y_target.to(device))
        pending.append((it, loss, ln_loss, lb_loss, lr_now))
        if it % 10 == 0 or it == args.Iteration:
            flush()
    flush()
    log.close()
    return trainer


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
