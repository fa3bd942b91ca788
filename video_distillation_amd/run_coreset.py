#!/usr/bin/env python3
"""Coreset baselines (herding / k-center) over the HIP path: the reference's distill_coreset.py with its flags and defaults.

    python -m video_distillation_amd.run_coreset --dataset synthetic --method herding --ipc 10 --num_eval 1
    python -m video_distillation_amd.run_coreset --dataset miniUCF101 --data_path D --method k-center --ipc 1 \\
        --pretrained_path net.pt

Data as in run_dm (``run_dm.load_data``; the data flags, process setup and log are ``driver.py``'s): ``--dataset synthetic`` (``--num_classes``, ``--pool_per_class``, ``--im_size``),
a frame-folder dataset under ``--data_path`` (decoded once, resident in HBM -- ``--preload`` is accepted and always in
effect), or ``--data_file f.pt``.  Selection: ``coreset.build_synset`` (fp32-grade features, fp64 Gram, picks on the device);
``--kcenter reference`` reproduces the reference script's k-center output (ipc <= 2 only, see coreset.py).  Then
``utils.evaluate_synset`` ``--num_eval`` times with ``mode='none', test_freq=100`` as the reference does (at fewer than 100
training epochs, where that test frequency would never test, the net is tested after the last epoch).  Output: JSON lines
(``--log_file`` too): the picks per class as dataset indices with the embed / selection times, each ``acc_test``, then
``acc_test_mean`` / ``acc_test_std``.  One rank only.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import driver


def build_parser():
    p = argparse.ArgumentParser(description='Coreset baselines on MI355X')
    # distill_coreset.py's flags, with its defaults
    p.add_argument('--dataset', type=str, default='miniUCF101', help='dataset')
    p.add_argument('--method', type=str, default='k-center', help='k-center or herding')
    p.add_argument('--model', type=str, default='ConvNet3D', help='model')
    p.add_argument('--ipc', type=int, default=1, help='image(s) per class')
    p.add_argument('--eval_mode', type=str, default='S', help='eval_mode')
    p.add_argument('--num_eval', type=int, default=5, help='how many networks to evaluate on')
    p.add_argument('--epoch_eval_train', type=int, default=1000, help='epochs to train a model with synthetic data')
    p.add_argument('--lr_net', type=float, default=0.001, help='learning rate for network')
    p.add_argument('--batch_train', type=int, default=256, help='batch size for training networks')
    p.add_argument('--data_path', type=str, default='distill_utils/data', help='dataset path')
    p.add_argument('--pretrained_path', type=str, default=None, help='pretrained model path')
    p.add_argument('--num_workers', type=int, default=8, help='decode threads of the preload')
    p.add_argument('--save_path', type=str, default='.', help='path to save')
    p.add_argument('--frames', type=int, default=16, help='')
    p.add_argument('--preload', action='store_true', help='preload dataset (the pool is always resident)')
    # the project's data options (run_dm.load_data reads them)
    driver.add_data_flags(p)
    p.add_argument('--pool_per_class', type=int, default=93, help='synthetic data only')
    # this driver's own
    p.add_argument('--kcenter', type=str, default='greedy', choices=['greedy', 'reference'])
    p.add_argument('--log_file', type=str, default=None)
    return p


def _dataset_indices(args, pool, num_classes):
    """Pool row -> dataset index per class: load_data keeps each class's clips in dataset order."""
    if args.data_file is None and args.dataset == 'synthetic':
        return [list(range(pool.offsets[c], pool.offsets[c] + pool.counts[c])) for c in range(num_classes)]
    if args.data_file is not None:
        labels = torch.load(args.data_file, map_location="cpu")["labels"].long().tolist()
    else:
        from . import dataset as D
        labels = D.get_dataset(args.dataset, args.data_path, img_size=(args.im_size, args.im_size))[6].labels
    per = [[] for _ in range(num_classes)]
    for i, lab in enumerate(labels):
        per[int(lab)].append(i)
    return per


def run(args, log=None):
    from . import coreset, plan, utils
    from .run_dm import load_data
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_coreset runs on one rank: selection of a whole dataset takes seconds on one GPU "
                         "(launch it without torch.distributed.run)")
    if args.method not in coreset.METHODS:
        raise NotImplementedError("--method %s (the reference knows herding and k-center)" % args.method)
    _, _, device = driver.start(use_cuda=True)
    geo = plan.NetGeometry(args.frames, args.im_size, args.im_size)
    pool, num_classes, _, testloader = load_data(args, 0, 1, geo, device)
    im_size = (int(pool.clips.shape[3]), int(pool.clips.shape[4]))
    log = driver.JsonLog(args.log_file, 0, log)
    emit = log.emit
    net = utils.get_network(args.model, 3, num_classes, im_size, frames=args.frames, dist=False).to(device)
    net.train()
    for param in list(net.parameters()):
        param.requires_grad = False
    if args.pretrained_path is not None:
        net.load_state_dict(torch.load(args.pretrained_path, map_location=device))
    net.eval()

    stats = {}
    image_syn, label_syn, index = coreset.build_synset(net, pool, num_classes, args.ipc, args.method, kcenter=args.kcenter,
                                                       stats=stats)
    ds_index = _dataset_indices(args, pool, num_classes)
    picks = index.view(num_classes, args.ipc).cpu().tolist()
    emit({"method": args.method, "kcenter": args.kcenter if args.method == "k-center" else None, "ipc": args.ipc,
          "num_classes": num_classes, "embed_s": round(stats["embed_s"], 6), "select_s": round(stats["select_s"], 6),
          "picks": [[ds_index[c][p - pool.offsets[c]] for p in picks[c]] for c in range(num_classes)]})
    if testloader is None:
        emit({"eval": "skipped: the synthetic pool has no test split"})
    else:
        test_freq = 100 if args.epoch_eval_train >= 100 else None
        for model_eval in utils.get_eval_pool(args.eval_mode, args.model, args.model):
            accs = []
            for it_eval in range(args.num_eval):
                net_eval = utils.get_network(model_eval, 3, num_classes, im_size, frames=args.frames, dist=False).to(device)
                eargs = argparse.Namespace(device=str(device), lr_net=args.lr_net, epoch_eval_train=args.epoch_eval_train,
                                           batch_train=args.batch_train, model=args.model, eval_mode=args.eval_mode)
                _, acc_train, acc_test, _ = utils.evaluate_synset(it_eval, net_eval, image_syn.detach().clone(),
                                                                  label_syn.detach().clone(), testloader, eargs, mode='none',
                                                                  test_freq=test_freq)
                accs.append(float(acc_test))
                emit({"model": model_eval, "it_eval": it_eval, "acc_train": float(acc_train), "acc_test": float(acc_test)})
            emit({"model": model_eval, "acc_test_mean": float(np.mean(accs)), "acc_test_std": float(np.std(accs))})
    log.close()
    return image_syn, label_syn, index


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
