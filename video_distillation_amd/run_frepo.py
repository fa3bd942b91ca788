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
``(one_hot - 1 / C) / sqrt(C / 10)``.  ``--train_videos host`` reads them through a host ``DataLoader``; ``preload`` uploads the
training set once as fp32 clips and gathers a batch with one ``index_select``; ``resident`` keeps whole videos in HBM
(``dataset.ResidentVideos``, 'window' frame-folder datasets) and draws start frame and flip per read.  The two device modes take
their batch order from ``frepo.real_batch_indices`` under a private generator seeded from ``--seed``.

Ranks: one by default.  ``--target_ranks all`` (needs ``preload`` or ``resident``) keeps the synthetic set, the pool, the
optimisers and every random draw on rank 0 and deals the 512 target clips' ``embed_exact`` forward over all ranks
(``frepo.TargetExchange``); ``--eval_ranks all`` (needs ``--target_ranks all``) deals the evaluation networks over the ranks too
(``evalpool.evaluate_pool`` with ``frepo.EVAL_RECIPE``).  Files and log lines are rank 0's.

Files: at ``it == 1`` and every 400 iterations ``dynamic_{it}.pt`` (C, dpc, T, 1, H, W), ``hal_{it}.pt`` (the ModuleList's
state dict, what ``checkpoint.load_hallucinators`` reads) and ``y_syn_{it}.pt`` under ``save_path/S2D_FRePo/{dataset}_ipc{n}_
{lr_d}_{lr_h}``; ``images_{it}.pt`` and ``y_syn_{it}.pt`` under ``save_path/Baseline_FRePo/...``; with a new best accuracy
``dynamic_best.pt`` / ``weights_best.pt`` / ``y_syn_best.pt``, or ``images_best.pt`` / ``y_syn_best.pt``.  Evaluation at
``np.arange(startIt, Iteration + 1, eval_it)``: ``--num_eval`` networks through FRePo's own ``evaluate_synset`` (AdamW, MSE on
the soft labels).  Logging: JSON lines (driver.JsonLog) with ``Loss``, ``ln_loss``, ``lb_loss`` and ``lr`` per step and the
reference's four ``Accuracy/...`` keys per evaluation; the losses stay on the device and are written out every 10 iterations.

Not here: the synthetic side or the pool's training sharded over ranks, a host-mode loader under several ranks (refused), wandb,
``--init real-all``, evaluation architectures other than the hot path's.  ``--data_path`` defaults to the other drivers'
relative directory, not to the reference author's absolute one.
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
    p.add_argument('--train_videos', type=str, default='host', choices=['host', 'preload', 'resident'],
                   help="host: a DataLoader decodes / gathers the 512 real clips per iteration; preload: the training set in HBM as "
                        "fp32 clips, one index_select per batch; resident: whole training videos in HBM, clips drawn per read "
                        "(dataset.ResidentVideos; 'window' frame-folder datasets only)")
    p.add_argument('--target_ranks', type=str, default='rank0', choices=['rank0', 'all'],
                   help="rank0: a single rank; all: rank 0 leads, every rank embeds its share of the target clips "
                        "(needs --train_videos preload or resident)")
    return p


def check_settings(args) -> None:
    """What the driver refuses, before anything touches a device."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    folders = args.data_file is None and args.dataset != 'synthetic'
    if world > 1 and args.target_ranks != 'all':
        raise ValueError("run_frepo runs on a single rank (WORLD_SIZE is %d) unless --target_ranks all deals the target clips "
                         "over the ranks" % world)
    if args.target_ranks == 'all' and args.train_videos == 'host':
        raise ValueError("run_frepo: --target_ranks all needs --train_videos preload or resident (under --train_videos host every "
                         "rank would decode its own 512 clips per iteration)")
    if args.eval_ranks == 'all' and args.target_ranks != 'all':
        raise ValueError("run_frepo: --eval_ranks all needs --target_ranks all (the ranks that evaluate are the ranks that embed)")
    if args.eval_ranks == 'all' and world < 2:
        raise ValueError("run_frepo: --eval_ranks all at WORLD_SIZE 1: there is no second rank to deal the networks to")
    if args.test_videos == 'resident' and not folders:
        raise ValueError("run_frepo: --test_videos resident keeps the test videos of a frame-folder dataset in HBM; a --data_file "
                         "or --dataset synthetic has none")
    if args.train_videos == 'resident' and not folders:
        raise ValueError("run_frepo: --train_videos resident keeps the training videos of a frame-folder dataset in HBM; a "
                         "--data_file or --dataset synthetic has none (use preload)")
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


class RealStore:
    """The real clips in HBM and their batches, for ``--train_videos preload`` and ``resident``.  ``table(indices)`` is what
    rank 0 draws per batch -- one row of ``width`` int64 per clip, every random draw of the read inside -- and ``clips(rows)`` /
    ``labels(rows)`` turn rows of it into device tensors on any rank that holds the store.

      * preload:   ``clips`` (N, T, 3, H, W) fp32 and ``labels`` (N,) on the device; a row is the item number, a batch one
                   ``index_select``;
      * resident:  a ``dataset.ResidentVideos`` store; a row is ``[item, flip, T frame numbers, T crop rows, T crop columns]``
                   (crops -1 when the transform does not crop), drawn by ``store.draw`` from the global generators in batch
                   order as the host loader's items draw them; a batch is one ``vd_clips_sample`` launch (``store.batch``)."""

    def __init__(self, num_classes: int, clips=None, labels=None, videos=None):
        self.num_classes, self.dev_clips, self.videos = int(num_classes), clips, videos
        if videos is None:
            self.dev_labels = torch.as_tensor(labels, dtype=torch.int64).to(clips.device)
            self.n, self.width = int(clips.shape[0]), 1
        else:
            from . import dataset as D
            self.n, self.width = len(videos), 2 + 3 * D.NUM_FRAMES

    def table(self, indices: torch.Tensor) -> torch.Tensor:
        indices = indices.to(torch.int64).reshape(-1)
        if self.videos is None:
            return indices.reshape(-1, 1).clone()
        rows = torch.full((int(indices.numel()), self.width), -1, dtype=torch.int64)
        for b, k in enumerate(indices.tolist()):
            d = self.videos.draw(self.videos.indices[k])
            t = len(d.numbers)
            rows[b, 0], rows[b, 1] = d.index, int(d.flip)
            rows[b, 2:2 + t] = torch.as_tensor(d.numbers, dtype=torch.int64)
            if d.crops and d.crops[0] is not None:
                rows[b, 2 + t:2 + 3 * t] = torch.as_tensor(d.crops, dtype=torch.int64).t().reshape(-1)
        return rows

    def _draws(self, rows: torch.Tensor):
        from . import dataset as D
        t, out = D.NUM_FRAMES, []
        for r in rows.tolist():
            crops = [None] * t if r[2 + t] < 0 else [(int(y), int(x)) for y, x in zip(r[2 + t:2 + 2 * t], r[2 + 2 * t:2 + 3 * t])]
            out.append(D.ResidentDraw(int(r[0]), [int(v) for v in r[2:2 + t]], bool(r[1]), crops))
        return out

    def clips(self, rows: torch.Tensor) -> torch.Tensor:
        if self.videos is None:
            return self.dev_clips.index_select(0, rows.reshape(-1).to(self.dev_clips.device))
        return self.videos.batch(self._draws(rows))[0]

    def labels(self, rows: torch.Tensor) -> torch.Tensor:
        """The soft labels ``one_hot - 1 / C`` of the rows, on the device."""
        from . import frepo
        if self.videos is None:
            lab = self.dev_labels.index_select(0, rows.reshape(-1).to(self.dev_labels.device))
        else:
            lab = torch.as_tensor([self.videos.dataset.labels[int(i)] for i in rows[:, 0].tolist()],
                                  dtype=torch.int64).to(self.videos.frames.device)
        return frepo.soft_labels(lab, self.num_classes)


def load_data(args, rank: int, device):
    """``run_mtt.load_data`` and, for ``--train_videos preload | resident``, the ``RealStore`` of the training set.
    -> (num_classes, clips_of, labels, testloader, store or None)"""
    from . import run_mtt
    if args.train_videos == 'host':
        return run_mtt.load_data(args, rank, device) + (None,)
    if args.data_file is None and args.dataset != 'synthetic':
        from . import dataset as D
        _, _, num_classes, _, _, _, dst_train, dst_test, testloader = D.get_dataset(args.dataset, args.data_path,
                                                                                    img_size=(args.im_size, args.im_size))
        if not args.no_eval:
            testloader = driver.folder_test_loader(args, rank, device, dst_test, testloader)
        clips_of = lambda idx: torch.stack([dst_train[int(i)][0] for i in idx])
        if args.train_videos == 'resident':
            try:
                videos = D.ResidentVideos.from_dataset(dst_train, device, workers=args.num_workers)
            except ValueError as e:
                raise ValueError("run_frepo: --train_videos resident: %s" % e)
            store = RealStore(num_classes, videos=videos)
        else:
            clips, labels = D.preload(dst_train, device, workers=args.num_workers)
            store = RealStore(num_classes, clips, labels)
        return num_classes, clips_of, list(dst_train.labels), testloader, store
    num_classes, clips_of, labels, testloader = run_mtt.load_data(args, rank, device)
    if args.data_file is not None:
        clips = torch.load(args.data_file, map_location="cpu")["clips"].float().to(device)
    else:
        clips = clips_of(range(len(labels))).float().to(device)
    return num_classes, clips_of, labels, testloader, RealStore(num_classes, clips, labels)


def device_batches(store: RealStore, seed: int):
    """``--train_videos preload | resident``: for ever ``(table rows, clips, soft labels)`` of the next batch, the order from
    ``frepo.real_batch_indices`` under a private generator seeded from ``seed``."""
    from . import frepo
    for indices in frepo.real_batch_indices(store.n, REAL_BATCH, torch.Generator().manual_seed(int(seed))):
        rows = store.table(indices)
        yield rows, store.clips(rows), store.labels(rows)


def eval_shell(args, num_classes: int, device):
    """A synthetic set of the run's shapes with nothing in it: what a rank other than 0 loads rank 0's parameters into for an
    evaluation round."""
    from . import frepo, utils
    n, hw = num_classes * args.num_prototypes_per_class, (args.im_size, args.im_size)
    y = torch.zeros(n, num_classes)
    if args.memories == 'images':
        return frepo.SynData(torch.zeros((n, args.frames, 3) + hw), y).to(device)
    hals = torch.nn.ModuleList([utils.Conv3DNet() for _ in range(args.n_hal)])
    return frepo.S2DSynData(torch.zeros((n, 3) + hw), torch.zeros((num_classes, args.dpc, args.frames, 1) + hw), hals, y).to(device)


def evaluate_on_all_ranks(args, it: int, syndata, testloader, eargs, num_classes: int, rank: int, world: int, device, seed: int):
    """One evaluation round of ``--eval_ranks all``, entered by every rank: rank 0 broadcasts the synthetic set's parameters --
    for ``--memories images`` the clips and labels ``syndata.value()`` returns, for s2d the memories and hallucinators it is
    composed from, so that every network draws its own hallucinators as on one rank -- and ``evalpool.evaluate_pool`` deals the
    networks.  Network ``i``'s training set is ``syndata.value()`` on its owner, after the unit's seed.
    -> the result dict, the same on every rank."""
    import torch.distributed as dist
    from . import evalpool, frepo
    xdev = evalpool._exchange_device(device, True)
    flat = evalpool.flat_weights(syndata).to(xdev) if rank == 0 else \
        torch.empty(sum(p.numel() for p in syndata.parameters()), dtype=torch.float32, device=xdev)
    dist.broadcast(flat, src=0)
    if rank != 0:
        evalpool.load_flat_weights(syndata, flat.to(device))

    def data(i):
        with torch.no_grad():
            x, y = syndata.value()
        return x.clone(), y.clone()
    make_net = evalpool.convnet3d_factory(num_classes, (args.im_size, args.im_size), args.frames)
    return evalpool.evaluate_pool(make_net, None, None, testloader, eargs, num_eval=args.num_eval, seed=seed, rank=rank, world=world,
                                  num_classes=num_classes, recipe=frepo.EVAL_RECIPE.with_data(data))


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
    from . import frepo, utils
    rank, world, device = driver.start(use_cuda=True)
    s2d = args.memories == 's2d'
    num_classes, clips_of, train_labels, testloader, store = load_data(args, rank, device)
    hw = (args.im_size, args.im_size)
    num_prototypes = args.num_prototypes_per_class * num_classes
    batch_train = min(num_prototypes, 500) if args.batch_train is None else args.batch_train
    get_model = lambda: utils.get_network(args.model, 3, num_classes, hw, frames=args.frames, dist=False).to(device)
    eval_pool = utils.get_eval_pool(args.eval_mode, args.model, args.model)
    evaluate = not args.no_eval and testloader is not None
    eval_all = evaluate and args.eval_ranks == 'all'
    if eval_all and list(eval_pool) != ['ConvNet3D']:
        raise NotImplementedError("--eval_ranks all evaluates ConvNet3D (the hot path's network), not %s" % list(eval_pool))
    eval_seed = driver.draw_eval_seed(args.eval_seed, rank, world) if eval_all else None
    eargs = argparse.Namespace(device=str(device), lr_net=args.lr_net, epoch_eval_train=args.epoch_eval_train, batch_train=batch_train)
    exchange = None
    if rank != 0:
        # an embedder: the store, a shell per pool network, a shell of the synthetic set for the evaluation rounds
        shells = [get_model() for _ in range(args.num_nn_state)]
        exchange = frepo.TargetExchange(lambda idx: shells[idx], store.clips, rank, world, device, REAL_BATCH, store.width)
        if exchange.follow() != frepo.READY:          # (raises when rank 0 failed while it set up)
            raise RuntimeError("run_frepo: rank 0 did not announce its set-up")
        exchange.sync_all_weights(len(shells))
        syn_shell = eval_shell(args, num_classes, device) if eval_all else None
        done = 0
        while True:
            kind = exchange.follow(done + 1)
            if kind == frepo.STEP:
                done += 1
            elif kind == frepo.EVALUATE:          # (the round before iteration done + 1)
                evaluate_on_all_ranks(args, done + 1, syn_shell, testloader, eargs, num_classes, rank, world, device, eval_seed + done + 1)
            else:
                return None
    if args.target_ranks == 'all':
        exchange = frepo.TargetExchange(lambda idx: pools[idx].model, store.clips, rank, world, device, REAL_BATCH, store.width)
    try:
        syndata = build_syndata(args, num_classes, clips_of, train_labels, device)
        synopt, synsch = frepo.syn_optimizer(syndata, args.lr_d, args.lr_h, args.Iteration)
        pools = frepo.build_pool(get_model, args.lr_net, args.max_online_updates, args.num_nn_state, device)
        trainer = frepo.FRePoTrainer(syndata, pools, synopt, synsch)
    except BaseException:
        if exchange is not None:
            exchange.lead_abort()          # (the other ranks wait for the set-up's header)
        raise
    if store is None:
        workers = args.num_workers if (args.data_file is None and args.dataset != 'synthetic') else 0
        batches = real_batches(clips_of, train_labels, num_classes, workers)
    elif args.target_ranks != 'all':
        batches = device_batches(store, args.seed)
    if args.target_ranks == 'all':
        indices = frepo.real_batch_indices(store.n, REAL_BATCH, torch.Generator().manual_seed(int(args.seed)))      # (device_batches' order)
        exchange.lead_ready()
        exchange.sync_all_weights(len(pools))
    save_dir = os.path.join(args.save_path, "S2D_FRePo" if s2d else "Baseline_FRePo",
                            "%s_ipc%d_%s_%s" % (args.dataset, args.num_prototypes_per_class, args.lr_d, args.lr_h))
    best_acc = {m: 0.0 for m in eval_pool}; best_std = {m: 0.0 for m in eval_pool}
    log = driver.JsonLog(args.log_file, rank, log)
    eval_its = set(np.arange(args.startIt, args.Iteration + 1, args.eval_it).tolist())
    pending = []          # (it, loss, ln_loss, lb_loss on the device, lr_h of the step)
    t0 = time.time()

    def flush():
        if pending:
            torch.cuda.synchronize(device)
        for it_, loss_, ln_, lb_, lr_ in pending:
            log.emit({"step": it_, "Loss": float(loss_), "ln_loss": float(ln_), "lb_loss": float(lb_), "lr": lr_,
                      "elapsed_s": round(time.time() - t0, 3)})
        del pending[:]

    try:
        for it in range(1, args.Iteration + 1):
            if evaluate and (it in eval_its or it % STEPS_PER_EVAL == 0):
                flush()
                for model_eval in eval_pool:
                    if eval_all:
                        exchange.lead_evaluate()
                        got = evaluate_on_all_ranks(args, it, syndata, testloader, eargs, num_classes, rank, world, device, eval_seed + it)
                        exchange.waiting = True
                        mean, std = got["mean"], got["std"]
                    else:
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
            lr_now = float(synsch.get_last_lr()[-1])
            if store is None:
                x_target, y_target = next(batches)
                loss, ln_loss, lb_loss = trainer.step(x_target.to(device), y_target.to(device))
            elif exchange is None:
                _, x_target, y_target = next(batches)          # (device tensors: nothing crosses PCIe but the table)
                loss, ln_loss, lb_loss = trainer.step(x_target, y_target)
            else:
                rows = store.table(next(indices))
                idx = trainer.draw_pool_index()
                y_target = store.labels(rows)
                loss, ln_loss, lb_loss = exchange.lead(idx, rows, lambda feat: trainer.step(None, y_target, feat_tar=feat, idx=idx), it)
            pending.append((it, loss, ln_loss, lb_loss, lr_now))
            if it % 10 == 0 or it == args.Iteration:
                flush()
        flush()
    except BaseException:
        if exchange is not None:
            exchange.lead_abort()
        raise
    if exchange is not None:
        exchange.lead_stop()
    log.close()
    return trainer


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
