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

The expert trajectories of ``--buffer_path`` (``replay_buffer_N.pt`` of buffer.py) are served by ``experts.ExpertStore``:
``--expert_store host`` keeps one file at a time in pinned host memory, ``resident`` all of them in HBM; ``--buffer_walk all``
visits every file, ``reference`` only the first of the shuffle, as the reference's loops do (they never load a second file);
``--max_files`` bounds the files looked at.  ``--fused_flat on`` runs the flat-parameter arithmetic of an iteration on the
``vdt_`` kernels (include/vd_traj.h), ``off`` on torch expressions.  The walk is seeded (``--seed``) and the same on every rank;
every rank holds all memories and takes its share of each student batch (distill.MTTTrainer).

Data as ``run_dm`` (``--dataset synthetic``, the reference's frame folders, or ``--data_file f.pt``); the real training clips are
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
import json
import os
import time

import numpy as np
import torch

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
    p.add_argument('--data_file', type=str, default=None)
    p.add_argument('--im_size', type=int, default=112)
    p.add_argument('--num_classes', type=int, default=50, help='synthetic data only')
    p.add_argument('--log_file', type=str, default=None)
    p.add_argument('--no_eval', action='store_true')
    p.add_argument('--test_videos', type=str, default='host', choices=['host', 'resident'])
    p.add_argument('--eval_ranks', type=str, default='rank0', choices=['rank0', 'all'])
    p.add_argument('--eval_seed', type=int, default=None)
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
        if args.test_videos == 'resident' and (rank == 0 or args.eval_ranks == 'all') and not args.no_eval:
            testloader = D.resident_loader(dst_test, device, batch_size=testloader.batch_size, workers=args.num_workers)
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
    test = None
    if "test_clips" in blob:
        test = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(blob["test_clips"].float(), blob["test_labels"].long()),
                                           batch_size=64, shuffle=False)
    return num_classes, (lambda idx: blob["clips"][torch.as_tensor(idx, dtype=torch.int64)].float()), labels.tolist(), test


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
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = ops is None
    device = torch.device("cuda", local_rank) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group(backend="nccl" if use_cuda else "gloo")
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
    out = open(args.log_file, "a") if (args.log_file and rank == 0) else None

    def emit(rec):
        if rank == 0:
            line = json.dumps(rec)
            (log.append(rec) if log is not None else None)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    evaluate = not args.no_eval and testloader is not None
    eval_all = args.eval_ranks == 'all' and evaluate
    eval_seed = None
    if eval_all:
        eval_seed = args.eval_seed
        if eval_seed is None:
            box = [int(time.time() * 1000) % 100000 if rank == 0 else None]
            if world > 1:
                import torch.distributed as dist
                dist.broadcast_object_list(box, src=0)
            eval_seed = box[0]
        emit({"eval_ranks": "all", "eval_seed": int(eval_seed), "world": world})
    emit({"expert_store": store.mode, "buffer_walk": store.walk, "buffer_files": len(store.files), "expert_epochs_per_trajectory": store.epochs,
          "fused_flat": getattr(ops, "flat", None) is not None, "batch_syn": batch_syn})
    test_freq = 200 if args.epoch_eval_train >= 200 else None          # (the reference's loop never tests below 200 epochs)
    eval_its = set(np.arange(start_it, args.Iteration + 1, args.eval_it).tolist())
    pending = []          # (it, start_epoch, grand loss on the device, syn_lr on the device before the step)
    t0 = time.time()

    def flush():
        sync()
        for it_, start_, grand_, lr_ in pending:
            g = float(grand_)
            emit({"step": it_, "Grand_Loss": g, "Grand_Loss/%d" % start_: g, "Start_Epoch": start_, "Synthetic_LR": float(lr_),
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
                memories, labels_eval, mode = [static_all.detach().clone(), dynamic_all.detach().clone(), hals], None, 'multi-static'
            else:
                memories, labels_eval, mode = trainer.image_syn.detach().clone(), torch.arange(num_classes).repeat_interleave(args.ipc), 'none'
            save_this_it = False
            if evaluate:
                eargs = argparse.Namespace(device=str(device), lr_net=float(trainer.syn_lr), epoch_eval_train=args.epoch_eval_train,
                                           batch_train=args.batch_train, model=args.model, eval_mode=args.eval_mode)
                for model_eval in eval_pool:
                    if eval_all:
                        from . import evalpool
                        if model_eval != 'ConvNet3D':
                            raise NotImplementedError("--eval_ranks all evaluates ConvNet3D (the hot path's network), not %s" % model_eval)
                        make_net = evalpool.convnet3d_factory(num_classes, hw, args.frames)
                        got = evalpool.evaluate_pool(make_net, memories, labels_eval, testloader, eargs, num_eval=args.num_eval,
                                                     seed=int(eval_seed) + it, mode=mode, rank=rank, world=world,
                                                     num_classes=num_classes)
                        mean, std = got["mean"], got["std"]           # (the same numbers on every rank: best_* stay in step)
                    elif rank == 0:
                        accs = []
                        for it_eval in range(args.num_eval):
                            net_eval = utils.get_network(model_eval, 3, num_classes, hw, frames=args.frames, dist=False).to(device)
                            if s2d:
                                _, _, acc_test, _ = utils.evaluate_synset(it_eval, net_eval, memories, None, testloader, eargs,
                                                                          mode='multi-static')
                            else:
                                _, _, acc_test, _ = utils.evaluate_synset(it_eval, net_eval, memories.clone(), labels_eval, testloader,
                                                                          eargs, mode='none', test_freq=test_freq)
                            accs.append(acc_test)
                        mean, std = float(np.mean(accs)), float(np.std(accs))
                    else:
                        continue
                    if mean > best_acc[model_eval]:
                        best_acc[model_eval], best_std[model_eval], save_this_it = mean, std, True
                    emit({"step": it, "Accuracy/%s" % model_eval: mean, "Max_Accuracy/%s" % model_eval: best_acc[model_eval],
                          "Std/%s" % model_eval: std, "Max_Std/%s" % model_eval: best_std[model_eval]})
            if rank == 0 and (save_this_it or it % 1000 == 0):
                if s2d:
                    checkpoint.save_s2d(save_dir, it, dynamic_all, [h.encoder.weight for h in hals], [h.encoder.bias for h in hals],
                                        best=save_this_it)
                    if train_static:
                        checkpoint.save_images(save_dir, it, static_all, best=save_this_it)
                else:
                    checkpoint.save_images(save_dir, it, trainer.image_syn, best=save_this_it)
            del memories
        lr_before = trainer.syn_lr
        grand = trainer.step(it, store.next())
        pending.append((it, trainer.last_start_epoch, grand, lr_before))
        if it % 10 == 0 or it == args.Iteration:
            flush()
    flush()
    if out:
        out.close()
    return trainer


def main(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--memories', type=str, default='images', choices=sorted(DEFAULTS))
    memories = pre.parse_known_args(argv)[0].memories
    run(build_parser(memories).parse_args(argv))


if __name__ == "__main__":
    main()
