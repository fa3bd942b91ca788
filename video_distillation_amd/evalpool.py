"""Evaluation of a synthetic set dealt across ranks.

The reference trains the ``num_eval`` evaluation networks one after the other on a DataParallel model (utils.py:615-623, called
at distill_baseline.py:295-322); this build runs one process per GPU, and ``evaluate_synset`` on rank 0 left the other ranks
waiting.  The networks are independent of each other, and so are the three test passes of each network, so the evaluation is
``3 * num_eval`` units:

  * phase A: network ``i`` is created and trained by rank ``i % world`` -- ``evaluate_synset``'s loop without its test;
  * phase B: pass ``p`` of network ``i`` runs on rank ``(i + p * num_eval) % world``; a network with a pass on a foreign rank
    travels there from its owner as one flat fp32 tensor (nothing travels when no unit moved);
  * exchange: one fp64 tensor (num_eval, 4, 8 + 2K) -- rows 0..2 the passes' ``vd_eval_stats`` records, row 3 the owner's last
    training epoch -- zero except where this rank wrote, summed by one all-reduce.  Every slot has one writer: the sum is exact.

What a network trains on, how it is trained and how one pass is tested is a ``Recipe``.  The default one is the reference's
cross-entropy evaluation as above (SGD, three passes, ``vd_eval_stats``); ``frepo.EVAL_RECIPE`` is FRePo's regression evaluation
(AdamW on soft labels, ONE test pass through ``vdr_regress_stats``, whose record has the same slots): then there are
``passes + 1`` rows per network and ``(1 + passes) * num_eval`` units.

All global generators are seeded from (seed, i, 0) before network ``i`` is created and trained and from (seed, i, 1 + p) before
pass ``p`` of its test, so what a unit computes depends neither on the rank that runs it nor on what that rank ran before.
Every rank derives the same result from the reduced tensor.  A rank that raises inside a phase still takes part in the error
flag exchanged at the end of the phase; then every rank raises.
"""
from __future__ import annotations

import random
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import distill, hip, utils
from .networks import ConvNet3D

PASSES = 3                # epoch('test') reads the test set three times (utils.py:752-844)
TRAIN_ROW = PASSES        # row of the exchange tensor that carries the owner's last training epoch: [0] loss, [1] accuracy


def train_rank(i: int, world: int) -> int:
    """The rank that creates and trains network ``i``."""
    return i % world


def unit_rank(i: int, p: int, num_eval: int, world: int, passes: int = PASSES) -> int:
    """The rank that runs test pass ``p`` (of ``passes``) of network ``i``.  The units numbered ``i + p * num_eval`` are dealt
    round-robin: every unit has one rank, loads differ by at most one unit, and all passes stay with the owner when ``world``
    divides ``num_eval`` (and at ``world`` 1)."""
    if not 0 <= p < passes:
        raise ValueError("unit_rank: pass %d of %d" % (p, passes))
    return (i + p * num_eval) % world


def assignment(num_eval: int, world: int, passes: int = PASSES) -> Dict[str, list]:
    """{"train": [rank of network i], "test": [[rank of pass p of network i]]}"""
    return {"train": [train_rank(i, world) for i in range(num_eval)],
            "test": [[unit_rank(i, p, num_eval, world, passes) for p in range(passes)] for i in range(num_eval)]}


def unit_seed(seed: int, i: int, k: int) -> int:
    """63-bit seed of (seed, network i, k): k = 0 creation and training, k = 1 + p test pass p."""
    return int(np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(i), int(k)]).generate_state(1, dtype=np.uint64)[0] >> 1)


def seed_all(s: int) -> None:
    """python ``random``, numpy, torch CPU and every torch device generator."""
    random.seed(s)
    np.random.seed(s % (1 << 32))
    torch.manual_seed(s)


def convnet3d_factory(num_classes: int, im_size, frames: int, channel: int = 3) -> Callable[[int], nn.Module]:
    """The default ``make_net``: the hot path's ConvNet3D (utils.get_network's 'ConvNet3D', utils.py:608-609) constructed
    directly -- ``get_network`` reseeds the global generator from the wall clock, which would undo the seeding above."""
    width, depth, act, _, _ = utils.get_default_convnet_setting()

    def make_net(i: int) -> nn.Module:
        return ConvNet3D(channel=channel, num_classes=num_classes, net_width=width, net_depth=depth, net_act=act, net_norm='none',
                         net_pooling='maxpooling', im_size=tuple(im_size), frames=frames)
    return make_net


def flat_weights(net: nn.Module) -> torch.Tensor:
    return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in net.parameters()])


def load_flat_weights(net: nn.Module, flat: torch.Tensor) -> None:
    at = 0
    with torch.no_grad():
        for p in net.parameters():
            n = p.numel()
            p.copy_(flat[at:at + n].view_as(p))
            at += n
    if at != flat.numel():
        raise ValueError("flat weights hold %d values, the network %d" % (flat.numel(), at))


def train_network(net: nn.Module, images_train, labels_train, args, mode: str = 'none'):
    """``evaluate_synset``'s training loop (utils.py:848-886) without its test: ``Epoch + 1`` training epochs, learning rate x 0.1
    and a fresh optimiser after epoch ``Epoch // 2 + 1``.  -> (loss, accuracy) of the last epoch."""
    lr = float(args.lr_net)
    Epoch = int(args.epoch_eval_train)
    lr_schedule = [Epoch // 2 + 1]
    optimizer = torch.optim.SGD(net.parameters(), lr=lr, momentum=0.9, weight_decay=0.0005)
    criterion = nn.CrossEntropyLoss().to(args.device)
    if mode == 'none':
        trainloader = torch.utils.data.DataLoader(utils.TensorDataset(images_train, labels_train), batch_size=args.batch_train,
                                                  shuffle=True, num_workers=0)
    elif mode == 'multi-static':
        trainloader = utils.multi_static_loader(images_train[0], images_train[1], images_train[2], args.batch_train)
    else:
        raise NotImplementedError
    loss_train, acc_train = 0.0, 0.0
    for ep in range(Epoch + 1):
        loss_train, acc_train, _ = utils.epoch('train', trainloader, net, optimizer, criterion, args)
        if ep in lr_schedule:
            lr *= 0.1
            optimizer = torch.optim.SGD(net.parameters(), lr=lr, momentum=0.9, weight_decay=0.0005)
    if isinstance(acc_train, (list, tuple)):       # eval_mode 'top5': [acc, top-1, top-3, top-5]
        acc_train = acc_train[0]
    return float(loss_train), float(acc_train)


def test_pass(net: nn.Module, testloader, args, rec: torch.Tensor) -> torch.Tensor:
    """One iteration of ``testloader`` in eval mode without gradient, preprocessed as ``utils.epoch`` does; the statistics of
    every batch are accumulated into ``rec`` (on ``args.device``) by one ``vd_eval_stats`` launch."""
    net = net.to(args.device)
    net.eval()
    with torch.no_grad():
        for datum in testloader:
            img = datum[0].float().to(args.device)
            if 'Video' in args.model:
                img = img[:, :, :, 24:-24, 24:-24]
            img = utils._standardize(img)
            lab = datum[1].long().to(args.device)
            hip.eval_stats(net(img), lab, rec)
    return rec


class Recipe:
    """What ``evaluate_pool`` runs per network.

      * ``data(i)``                             -> (images_train, labels_train) of network ``i``; called by its owner after the
                                                   generators were seeded for the unit.  None: the arguments of ``evaluate_pool``
      * ``train(net, x, y, args)``              -> (loss, accuracy) of the last training epoch
      * ``test_pass(net, loader, args, rec)``   one iteration of the loader, accumulated into the record ``rec``
      * ``passes``                              test passes per network

    ``derive`` reads every record by the slots of ``vd_eval_stats``; ``loss_scale(K)`` divides slot 1 further (the regression
    record sums over the K classes of a clip, the mean-squared error divides by them)."""

    def __init__(self, train, test_pass, passes: int, data=None, loss_scale=None):
        if int(passes) < 1:
            raise ValueError("Recipe: at least one test pass")
        self.train, self.test_pass, self.passes, self.data, self.loss_scale = train, test_pass, int(passes), data, loss_scale

    def with_data(self, data) -> "Recipe":
        return Recipe(self.train, self.test_pass, self.passes, data, self.loss_scale)


def default_recipe(mode: str = 'none') -> Recipe:
    """The reference's cross-entropy evaluation: ``train_network`` in ``mode``, three passes of ``test_pass``."""
    return Recipe(lambda net, x, y, args: train_network(net, x, y, args, mode), test_pass, PASSES)


def _live(world: int) -> bool:
    if world <= 1:
        return False
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("evaluate_pool(world=%d) needs an initialised torch.distributed process group" % world)
    if dist.get_world_size() != world:
        raise RuntimeError("evaluate_pool(world=%d) under a process group of %d ranks" % (world, dist.get_world_size()))
    return True


def _exchange_device(device, live: bool):
    """Where the tensors that travel live: on the device under nccl (RCCL), on the host under gloo."""
    if live:
        import torch.distributed as dist
        if dist.get_backend() == "nccl":
            return torch.device(device)
    return torch.device("cpu")


def _end_of_phase(name: str, error: Optional[BaseException], live: bool, xdev) -> None:
    """Exchange the error flag of a phase; raise on every rank when any rank failed."""
    flag = torch.tensor([1.0 if error is not None else 0.0], dtype=torch.float32, device=xdev)
    if live:
        distill._all_reduce_max(flag)
    if error is not None:
        raise error
    if float(flag[0]) != 0.0:
        raise RuntimeError("evaluate_pool: another rank failed in the %s phase" % name)


def derive(records: torch.Tensor, num_eval: int, world: int, passes: int = PASSES, loss_scale: float = 1.0) -> dict:
    """The result every rank computes from the reduced (num_eval, passes + 1, 8 + 2K) tensor; ``loss_test`` is slot 1 over the
    clips seen and over ``loss_scale``."""
    if int(records.shape[1]) != passes + 1:
        raise ValueError("derive: %d rows per network for %d passes" % (int(records.shape[1]), passes))
    R = records.detach().cpu().to(torch.float64)
    K = (R.shape[2] - hip.EVAL_STATS_HEAD) // 2
    H = hip.EVAL_STATS_HEAD
    out = {"num_eval": num_eval, "world": world, "num_classes": K, "acc_test": [], "loss_test": [], "top1": [], "top3": [], "top5": [],
           "acc_per_class": [], "acc_train": [], "loss_train": [], "test_clips": [], "labels_out_of_range": []}
    for i in range(num_eval):
        tot = R[i, :passes].sum(0)              # (integers and the passes' loss sums, added in pass order)
        n = float(tot[0])
        if n <= 0:
            raise RuntimeError("evaluate_pool: network %d saw no test clip with a label in [0, %d)" % (i, K))
        out["test_clips"].append(int(n))
        out["labels_out_of_range"].append(int(tot[5]))
        out["loss_test"].append(float(tot[1]) / n / loss_scale if loss_scale != 1.0 else float(tot[1]) / n)
        out["acc_test"].append(float(tot[2]) / n)           # sum of top-1 hits / sum of clips over the three passes, as epoch()
        out["top1"].append(float(tot[2]) / n)
        out["top3"].append(float(tot[3]) / n)
        out["top5"].append(float(tot[4]) / n)
        hits, seen = tot[H:H + K].tolist(), tot[H + K:H + 2 * K].tolist()
        out["acc_per_class"].append([h / s if s > 0 else None for h, s in zip(hits, seen)])
        out["loss_train"].append(float(R[i, passes, 0]))          # (the training row follows the passes: TRAIN_ROW at three)
        out["acc_train"].append(float(R[i, passes, 1]))
    out["mean"] = float(np.mean(out["acc_test"]))
    out["std"] = float(np.std(out["acc_test"]))
    out["assignment"] = assignment(num_eval, world, passes)
    out["records"] = R
    return out


def evaluate_pool(make_net, images_train, labels_train, testloader, args, *, num_eval: int, seed: int, mode: str = 'none',
                  rank: int = 0, world: int = 1, num_classes: Optional[int] = None, on_trained=None,
                  recipe: Optional[Recipe] = None) -> dict:
    """Train ``num_eval`` networks on the synthetic set and test each three times, dealt over ``world`` ranks (module
    docstring).  Every rank calls it with the same arguments and its own ``rank`` and gets the same dict: per network
    ``acc_test``, ``loss_test``, ``top1`` / ``top3`` / ``top5``, ``acc_per_class`` (None for a class never seen),
    ``acc_train``, ``loss_train``; over the networks ``mean`` and ``std`` (np.mean / np.std, as the reference's drivers); the
    reduced ``records``; the unit-to-rank ``assignment``; and ``times`` (seconds: per network and pass, and per rank and phase).

    ``make_net(i)`` builds network ``i`` after the generators were seeded (None: ConvNet3D for the geometry of
    ``images_train``, mode 'none').  It must not reseed from the clock as ``utils.get_network`` does.  ``args`` is
    ``evaluate_synset``'s namespace.  ``num_classes``: width of the records (default: from the training labels).
    ``on_trained(i, net)`` is called by the owner of network ``i`` after its training.  ``recipe``: None is the reference's
    cross-entropy evaluation (``default_recipe(mode)``); another ``Recipe`` trains and tests its own way with its own number of
    passes, ``mode`` 'none' only."""
    if mode not in ('none', 'multi-static'):
        raise NotImplementedError
    if num_eval < 1 or not 0 <= rank < world:
        raise ValueError("evaluate_pool: num_eval >= 1 and 0 <= rank < world")
    if num_classes is None:
        num_classes = int(labels_train.max()) + 1 if mode == 'none' else int(images_train[1].shape[0])
    if make_net is None:
        if mode != 'none':
            raise ValueError("evaluate_pool: pass make_net for mode %r" % mode)
        make_net = convnet3d_factory(num_classes, images_train.shape[3:5], int(images_train.shape[1]))
    if recipe is None:
        recipe = default_recipe(mode)
    elif mode != 'none':
        raise ValueError("evaluate_pool: a recipe of its own runs in mode 'none'")
    PASSES, TRAIN_ROW = recipe.passes, recipe.passes          # (rows per network: the passes, then the owner's training epoch)
    K = int(num_classes)
    live = _live(world)
    xdev = _exchange_device(args.device, live)
    plan = assignment(num_eval, world, PASSES)
    records = torch.zeros((num_eval, PASSES + 1, hip.EVAL_STATS_HEAD + 2 * K), dtype=torch.float64, device=xdev)
    times = torch.zeros(num_eval * (PASSES + 1) + world * 3, dtype=torch.float64, device=xdev)
    net_times = times[:num_eval * (PASSES + 1)].view(num_eval, PASSES + 1)      # [i][p] test pass p, [i][3] training
    rank_times = times[num_eval * (PASSES + 1):].view(world, 3)                # [rank] train, move, test
    is_cuda = torch.device(args.device).type == "cuda"

    def sync():
        if is_cuda:
            torch.cuda.synchronize(args.device)

    # ---- phase A: create and train the networks this rank owns; build the shells of the foreign ones it will test
    nets: Dict[int, nn.Module] = {}
    error = None
    t_phase = time.time()
    try:
        for i in range(num_eval):
            mine = plan["train"][i] == rank
            if not mine and rank not in plan["test"][i]:
                continue
            seed_all(unit_seed(seed, i, 0))
            net = make_net(i).to(args.device)
            if mine:
                t0 = time.time()
                x_train, y_train = (images_train, labels_train) if recipe.data is None else recipe.data(i)
                loss_train, acc_train = recipe.train(net, x_train, y_train, args)
                sync()
                net_times[i, TRAIN_ROW] = time.time() - t0
                records[i, TRAIN_ROW, 0] = loss_train
                records[i, TRAIN_ROW, 1] = acc_train
                if on_trained is not None:
                    on_trained(i, net)
            nets[i] = net
    except Exception as e:          # noqa: BLE001 -- re-raised after the flag exchange
        error = e
    rank_times[rank, 0] = time.time() - t_phase
    _end_of_phase("train", error, live, xdev)

    # ---- the trained weights of a network travel to the foreign ranks that test it (library code only: nothing here raises
    #      on one rank alone)
    t_phase = time.time()
    if live:
        import torch.distributed as dist
        for i in range(num_eval):
            owner = plan["train"][i]
            needers = sorted(set(plan["test"][i]) - {owner})
            if rank == owner:
                if needers:
                    flat = flat_weights(nets[i]).to(xdev)
                    for dst in needers:
                        dist.send(flat, dst=dst)
            elif rank in needers:
                flat = torch.empty(sum(p.numel() for p in nets[i].parameters()), dtype=torch.float32, device=xdev)
                dist.recv(flat, src=owner)
                load_flat_weights(nets[i], flat.to(args.device))
    rank_times[rank, 1] = time.time() - t_phase

    # ---- phase B: the test passes dealt to this rank
    error = None
    t_phase = time.time()
    try:
        for i in range(num_eval):
            for p in range(PASSES):
                if plan["test"][i][p] != rank:
                    continue
                seed_all(unit_seed(seed, i, 1 + p))
                t0 = time.time()
                rec = recipe.test_pass(nets[i], testloader, args, hip.eval_stats_record(K, args.device))
                sync()
                records[i, p].copy_(rec)
                net_times[i, p] = time.time() - t0
    except Exception as e:          # noqa: BLE001
        error = e
    rank_times[rank, 2] = time.time() - t_phase
    _end_of_phase("test", error, live, xdev)

    # ---- exchange
    if live:
        distill._all_reduce(records)
        distill._all_reduce(times)
    out = derive(records, num_eval, world, PASSES, 1.0 if recipe.loss_scale is None else float(recipe.loss_scale(K)))
    tn, tr = net_times.cpu(), rank_times.cpu()
    out["times"] = {"train_s": tn[:, TRAIN_ROW].tolist(), "test_pass_s": tn[:, :PASSES].tolist(),
                    "rank_train_s": tr[:, 0].tolist(), "rank_move_s": tr[:, 1].tolist(), "rank_test_s": tr[:, 2].tolist()}
    return out
