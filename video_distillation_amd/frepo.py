"""FRePo(+Ours) on the HIP path: the method of the reference's FRePo/script/distill_s2d.py, with its names and semantics.

  * ``lb_margin_th``                    the label-margin loss (:21-26)
  * ``SynData`` / ``S2DSynData``        the synthetic set: clips, or static + dynamic memories and hallucinators (:47-86)
  * ``PoolElement``                     one network of the model pool with its Adam optimiser and chained schedule, trained
                                        online on the synthetic set and reset after ``max_online_updates`` steps (:90-178)
  * ``FRePoTrainer.step``               one iteration of the loop (:343-367)
  * ``evaluate_synset`` / ``epoch``     FRePo's own evaluation: AdamW, MSE on soft labels (lib_torch/utils.py:522-601)
  * ``soft_labels`` / ``y_scale``       the label construction (:253-263)
  * ``hip_adam_step``                   ``optimizer.step()`` of any torch Adam / AdamW in ``vdf_adam_multi`` launches
  * ``real_batch_indices``              the batch order of the real clips kept in HBM: the DataLoader's, from a private generator
  * ``TargetExchange``                  the target embedding dealt over ranks under a leader (``--target_ranks all``)
  * ``EVAL_RECIPE``                     the evaluation as an ``evalpool.Recipe``: dealt over ranks, one ``vdr_regress_stats`` pass

The numerically hard centre is ``nfr.nfr`` (csrc/nfr.hip, fp64); every network step is ``ConvNet3D.hip_regress_step`` (the MFMA
forward / backward passes of the cross-entropy step with ``vdf_mse_loss`` and one ``vdf_adam_multi`` launch, csrc/frepo.hip).
The label-margin loss and the loss line are a handful of torch expressions on (n, C) and (m, C) tensors.

Not here: the synthetic side or the pool's training sharded over ranks (only the target embedding and the evaluation are dealt),
wandb, the blocked Cholesky of DESIGN 19.
"""
from __future__ import annotations

import random
import time
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import evalpool, hip


# ---- labels (distill_s2d.py:253-263) ------------------------------------------------------------
def y_scale(num_classes: int) -> float:
    return float(np.sqrt(num_classes / 10))


def soft_labels(labels: torch.Tensor, num_classes: int, scale: float = 1.0) -> torch.Tensor:
    """``(one_hot(labels) - 1 / C) / scale`` as float32: ``scale = y_scale(C)`` for the synthetic labels, 1 for real and test
    labels."""
    return ((F.one_hot(labels.long(), num_classes=num_classes) - 1 / num_classes) / scale).float()


def lb_margin_th(y: torch.Tensor) -> torch.Tensor:
    """Per row of ``y`` (n, C): ``-min(top1 - top2, 1 / C)`` (distill_s2d.py:21-26, there under vmap)."""
    val = torch.topk(y, k=2, dim=-1).values
    bound = torch.tensor(1 / y.shape[-1], dtype=torch.float, device=y.device)
    return -torch.minimum(val[..., 0] - val[..., 1], bound)


# ---- the optimiser step -------------------------------------------------------------------------
def _adam_group_check(optimizer, group) -> None:
    from .networks import ConvNet3D
    if not isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)) or not ConvNet3D._adam_group_ok(optimizer, group):
        raise NotImplementedError("hip_adam_step: torch.optim.Adam / AdamW without amsgrad, maximize, capturable or fused, a host-number "
                                  "learning rate, and weight decay only in its decoupled form (there is no torch-op fallback)")


def adam_update(optimizer, group, params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor]) -> None:
    """One Adam / AdamW step of ``params`` (tensors of ``group``) with the gradients ``grads``, the state kept where torch
    keeps it: ``optimizer.state[p]`` gets ``step`` (a float32 host scalar), ``exp_avg`` and ``exp_avg_sq`` (zeros like ``p``) on
    first use and ``step`` is incremented, exactly as ``torch.optim.Adam`` does -- a later plain ``optimizer.step()``, a
    ``state_dict()`` round trip or a scheduler just work.  Tensors that share a step count share a ``vdf_adam_multi`` launch."""
    _adam_group_check(optimizer, group)
    decoupled = isinstance(optimizer, torch.optim.AdamW) or bool(group.get("decoupled_weight_decay"))
    lr, (beta1, beta2), eps = float(group["lr"]), group["betas"], float(group["eps"])
    wd = float(group.get("weight_decay", 0)) if decoupled else 0.0
    by_step = {}
    for p, g in zip(params, grads):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError("hip_adam_step has no CPU path: contiguous fp32 parameters on a HIP device")
        st = optimizer.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["step"] += 1
        by_step.setdefault(int(st["step"]), []).append(
            (p.data, st["exp_avg"], st["exp_avg_sq"], g.detach().to(torch.float32).contiguous(), lr, wd))
    for t, segs in by_step.items():
        hip.adam_multi(segs, float(beta1), float(beta2), eps, t)
    for p in params:
        torch.autograd.graph.increment_version(p)
    optimizer._opt_called = True          # (what torch's schedulers look at before they warn that no optimiser step came first)


def hip_adam_step(optimizer) -> None:
    """``optimizer.step()`` of a torch Adam / AdamW on the HIP path: every param group with its own learning rate, parameters
    whose ``.grad`` is None skipped as torch skips them, one launch per 16 tensors of one step count."""
    for group in optimizer.param_groups:
        live = [p for p in group["params"] if p.grad is not None]
        if live:
            adam_update(optimizer, group, live, [p.grad for p in live])


# ---- the synthetic set --------------------------------------------------------------------------
class SynData(nn.Module):
    def __init__(self, x_init, y_init, learn_label=False):
        super().__init__()
        self.x_syn = nn.Parameter(x_init, requires_grad=True)
        self.y_syn = nn.Parameter(y_init, requires_grad=learn_label)

    def forward(self):
        return self.x_syn, self.y_syn

    def value(self):
        return self.x_syn.detach(), self.y_syn.detach()


class S2DSynData(nn.Module):
    """Static (n_c * dpc, 3, H, W; not trained), dynamic (n_c, dpc, T, 1, H, W), a ModuleList of hallucinators and the labels.
    ``forward`` draws one hallucinator per clip with ``random.randint`` in the reference's order (clip 0 first) and composes clip
    ``i`` from ``dynamic[i // dpc, i % dpc]`` and ``static[i]`` -- with ONE call per hallucinator over the clips that drew it,
    not one per clip.  ``value()`` re-draws, as the reference does."""

    def __init__(self, static, dynamic, hallucinator, y_init, learn_label=False):
        super().__init__()
        self.n_c, self.dpc = int(dynamic.shape[0]), int(dynamic.shape[1])
        if dynamic.dim() != 6 or self.n_c * self.dpc != int(static.shape[0]):
            raise ValueError("S2DSynData: dynamic %s composes n_c * dpc = %d clips, the static memory holds %d (the reference "
                             "would index out of range)" % (tuple(dynamic.shape), self.n_c * self.dpc, int(static.shape[0])))
        self.static = nn.Parameter(static, requires_grad=False)
        self.dynamic = nn.Parameter(dynamic, requires_grad=True)
        self.hallucinator = hallucinator
        self.y_syn = nn.Parameter(y_init, requires_grad=learn_label)
        self.x_syn = None
        self.last_draw: List[int] = []

    def forward(self):
        n = self.n_c * self.dpc
        draw = [random.randint(0, len(self.hallucinator) - 1) for _ in range(n)]
        self.last_draw = draw
        dyn = self.dynamic.reshape((n,) + tuple(self.dynamic.shape[2:]))          # row i = dynamic[i // dpc, i % dpc]
        used = sorted(set(draw))
        if len(used) == 1:
            self.x_syn = self.hallucinator[used[0]](self.static, dyn)
            return self.x_syn, self.y_syn
        parts, order = [], []
        for h in used:
            idx = [i for i in range(n) if draw[i] == h]
            at = torch.as_tensor(idx, dtype=torch.int64, device=dyn.device)
            parts.append(self.hallucinator[h](self.static.index_select(0, at), dyn.index_select(0, at)))
            order += idx
        back = torch.empty(n, dtype=torch.int64)
        back[torch.as_tensor(order)] = torch.arange(n)
        self.x_syn = torch.cat(parts, 0).index_select(0, back.to(dyn.device))
        return self.x_syn, self.y_syn

    def value(self):
        self.forward()
        return self.x_syn.detach(), self.y_syn.detach()


# ---- the model pool -----------------------------------------------------------------------------
def chained_schedule(optimizer, warmup_iters: int, t_max: int, eta_min: float):
    """``ChainedScheduler([LinearLR(0.01, warmup_iters), CosineAnnealingLR(t_max, eta_min)])``: torch's own schedulers."""
    S = torch.optim.lr_scheduler
    return S.ChainedScheduler([S.LinearLR(optimizer, start_factor=0.01, total_iters=warmup_iters),
                               S.CosineAnnealingLR(optimizer, T_max=t_max, eta_min=eta_min)])


class PoolElement:
    def __init__(self, get_model, get_optimizer, get_scheduler, loss_fn, batch_size, max_online_updates, idx, device, step=0):
        self.get_model, self.get_optimizer, self.get_scheduler = get_model, get_optimizer, get_scheduler
        self.loss_fn = loss_fn.to(device)
        self.batch_size, self.max_online_updates, self.idx, self.device = batch_size, max_online_updates, idx, device
        self.model = self.optimizer = self.scheduler = None
        self.initialize()
        self.step = step          # (the schedule is not advanced to ``step``: the reference does not either)

    def initialize(self):
        self.model = self.get_model().to(self.device)
        self.optimizer = self.get_optimizer(self.model)
        self.scheduler = self.get_scheduler(self.optimizer)
        self.step = 0

    def __call__(self, x, no_grad=False):
        self.model.eval()
        if no_grad:
            with torch.no_grad():
                return self.model(x)
        return self.model(x)

    def nfr(self, x_syn, y_syn, x_tar, reg=1e-6, use_flip=False, feat_tar=None):
        """``feat_tar`` (m, d): the targets' ``embed_exact`` features, computed elsewhere; ``x_tar`` is then not embedded."""
        from . import nfr
        return nfr.nfr(self.model, x_syn, y_syn, x_tar, reg=reg, use_flip=use_flip, exact=True, feat_tar=feat_tar)

    def get_batch(self, xs, ys):
        if ys.shape[0] < self.batch_size:
            return xs, ys
        sample_idx = np.random.choice(ys.shape[0], size=(self.batch_size,), replace=False)
        at = torch.as_tensor(sample_idx, dtype=torch.int64, device=ys.device)
        return xs[at], ys[at]

    def train_steps(self, x_syn, y_syn, steps=1):
        self.model.train()
        self.model.requires_grad_(True)
        for _ in range(steps):
            x, y = self.get_batch(x_syn, y_syn)
            ok = getattr(self.model, "hip_regress_trainable", None)
            if ok is not None and not ok(x, self.optimizer, self.loss_fn):
                raise NotImplementedError("PoolElement.train_steps: the model, optimiser and loss are not the combination "
                                          "ConvNet3D.hip_regress_step runs (there is no torch-op fallback)")
            self.model.hip_regress_step(x, y, self.optimizer)
            self.scheduler.step()
        self.check_for_reset(steps=steps)

    def check_for_reset(self, steps=1):
        self.step += steps
        if self.step >= self.max_online_updates:
            self.initialize()


def build_pool(get_model, lr_net: float, max_online_updates: int, num_nn_state: int, device) -> List[PoolElement]:
    """The pool of distill_s2d.py:283-294: Adam(lr_net), the chained schedule with 500 warm-up steps, MSE, batches of 500,
    element ``idx`` starting at step ``(max_online_updates // num_nn_state) * idx``."""
    get_optimizer = lambda m: torch.optim.Adam(m.parameters(), lr=lr_net, betas=(0.9, 0.999))
    get_scheduler = lambda o: chained_schedule(o, 500, max_online_updates, lr_net * 0.01)
    return [PoolElement(get_model, get_optimizer, get_scheduler, nn.MSELoss(), 500, max_online_updates, idx, device,
                        step=(max_online_updates // num_nn_state) * idx) for idx in range(num_nn_state)]


def syn_optimizer(syndata: nn.Module, lr_d: float, lr_h: float, iterations: int):
    """Adam over the synthetic set in the reference's two groups (:268-272) -- parameters whose name holds 'dynamic' (or, for
    ``SynData``, the clips ``x_syn``) at ``lr_d``, everything else at ``lr_h`` -- and ``CosineAnnealingLR(T_max=iterations,
    eta_min=0.1 lr_h)``."""
    first = 'dynamic' if any('dynamic' in n for n, _ in syndata.named_parameters()) else 'x_syn'
    d_params = [p for n, p in syndata.named_parameters() if first in n]
    other = [p for n, p in syndata.named_parameters() if first not in n]
    opt = torch.optim.Adam([{"params": d_params, "lr": lr_d}, {"params": other, "lr": lr_h}])
    return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=iterations, eta_min=lr_h * 0.1)


class FRePoTrainer:
    """One iteration of distill_s2d.py:343-367 per ``step``.  Nothing is read on the host."""

    def __init__(self, syndata: nn.Module, pools: Sequence[PoolElement], synopt, synsch, reg: float = 1e-6):
        self.syndata, self.pools, self.synopt, self.synsch, self.reg = syndata, list(pools), synopt, synsch, reg
        self.criterion = nn.MSELoss(reduction='none')
        self.last_idx = None

    def draw_pool_index(self) -> int:
        """The pool element of an iteration, from numpy's global generator (distill_s2d.py:345)."""
        return int(np.random.randint(low=0, high=len(self.pools)))

    def step(self, x_target: Optional[torch.Tensor], y_target: torch.Tensor, feat_tar: Optional[torch.Tensor] = None,
             idx: Optional[int] = None):
        """-> (loss, ln_loss, lb_loss) as device scalars.  ``feat_tar`` (m, d): ``pools[idx].model.embed_exact(x_target)``
        computed by the caller (``TargetExchange``), who then also made this iteration's ``draw_pool_index()`` and passes it as
        ``idx``; ``x_target`` is not read.  The synthetic set draws from python's ``random`` and the pool index from numpy, so
        the order of the two draws does not matter to either stream."""
        if feat_tar is not None and idx is None:
            raise ValueError("FRePoTrainer.step: feat_tar comes from pools[idx]; pass the idx that was drawn for it")
        x_syn, y_syn = self.syndata()
        if idx is None:
            idx = self.draw_pool_index()
        self.last_idx = idx
        pool_m = self.pools[idx]
        y_pred = pool_m.nfr(x_syn, y_syn, x_target, reg=self.reg, use_flip=False, feat_tar=feat_tar)
        ln_loss = self.criterion(y_pred, y_target).sum(dim=-1).mean(0)
        lb_loss = lb_margin_th(y_syn).mean()
        loss = ln_loss + lb_loss
        self.synopt.zero_grad(set_to_none=True)
        loss.backward()
        hip_adam_step(self.synopt)
        x_syn, y_syn = self.syndata.value()
        pool_m.train_steps(x_syn, y_syn, steps=1)
        self.synsch.step()
        return loss.detach(), ln_loss.detach(), lb_loss.detach()


# ---- real batches from HBM ----------------------------------------------------------------------
def real_batch_indices(n: int, batch: int, generator: torch.Generator) -> Iterator[torch.Tensor]:
    """The item numbers of ``DataLoader(dataset of n items, batch, shuffle=True, generator=generator)`` iterated epoch after
    epoch, for ever, as int64 host tensors; the last batch of an epoch is short.  ``generator`` is consumed per epoch exactly as
    the DataLoader consumes it (``dataset.DeviceBatches.__iter__``): one int64 for the iterator's base seed, the permutation,
    and the sampler's second, unused permutation when the epoch ends."""
    n, batch = int(n), int(batch)
    if n < 1 or batch < 1:
        raise ValueError("real_batch_indices: n %d items in batches of %d" % (n, batch))
    while True:
        torch.empty((), dtype=torch.int64).random_(generator=generator)
        order = torch.randperm(n, generator=generator)
        for lo in range(0, n, batch):
            yield order[lo:lo + batch]
        torch.randperm(n, generator=generator)


# ---- the target embedding dealt over ranks ------------------------------------------------------
HEADER = 4                          # [kind, error, idx, m] in front of the table
STEP, STOP, EVALUATE, READY = 0, 1, 2, 3      # header[0]: an iteration follows; stop (rank 0 is done); an evaluation round follows; rank 0 is set up


def rank_slice(m: int, r: int, world: int) -> Tuple[int, int]:
    """Rows ``[r * m // world, (r + 1) * m // world)`` of a batch of ``m``: in rank order they partition ``[0, m)``; a slice may be
    empty (m < world)."""
    return (r * m) // world, ((r + 1) * m) // world


def pad_rows(m: int, world: int) -> int:
    """Rows per rank of the gathered buffer: ``ceil(m / world)``, what the longest slice needs."""
    return -(-int(m) // int(world))


def trim_gathered(gathered: torch.Tensor, m: int, world: int) -> torch.Tensor:
    """(world * pad_rows, d) as ``all_gather_into_tensor`` leaves it -> the (m, d) rows of the slices, in batch order."""
    pad = pad_rows(m, world)
    parts = []
    for r in range(world):
        lo, hi = rank_slice(m, r, world)
        parts.append(gathered[r * pad:r * pad + (hi - lo)])
    return torch.cat(parts, 0) if world > 1 else parts[0]


class TargetExchange:
    """The leader (rank 0) and the embedders of ``--target_ranks all``.

    Every rank holds the real clips (``fetch(rows)``: the (k, width) int64 rows of a table -> k clips on the device) and a shell
    of every pool network (``models``; on rank 0 the pool's own, looked up per call because a reset replaces them).  Rank 0 alone
    holds the synthetic set, the optimisers and every random draw.  Per iteration

      1. rank 0 broadcasts ONE int64 tensor: the header ``[kind, error, idx, m]`` and the table of the batch (``m`` rows of
         ``width`` columns in a buffer of ``batch`` rows);
      2. rank r embeds rows ``rank_slice(m, r, world)`` with ``models(idx).embed_exact``;
      3. one MAX all-reduce of ``[error flag, d]`` (a rank that failed or whose slice is empty does not know the feature width
         d, and the gather needs one shape everywhere), then one ``all_gather_into_tensor`` of (``pad_rows(m, world)``, d) fp32 per rank, trimmed to ``feat_tar`` (m, d);
      4. rank 0 runs ``step(feat_tar)`` -- ``FRePoTrainer.step`` with ``feat_tar=`` and ``idx=``;
      5. rank 0 broadcasts ``[error, flat fp32 weights of element idx]`` (it may have been reset), the others load them.

    A rank that raises still takes part in the collective that follows and carries the flag; then every rank raises.  The followers
    wait in step 1 only: ``lead_stop`` / ``lead_abort`` release them.  At ``world`` 1 nothing is exchanged.  Under nccl (RCCL)
    the tensors that travel live on the device, under gloo on the host (``evalpool._exchange_device``)."""

    def __init__(self, models: Callable[[int], nn.Module], fetch: Callable[[torch.Tensor], torch.Tensor], rank: int, world: int,
                 device, batch: int, width: int = 1):
        self.models, self.fetch, self.rank, self.world, self.device = models, fetch, int(rank), int(world), device
        self.batch, self.width = int(batch), int(width)
        self.live = evalpool._live(self.world)
        self.xdev = evalpool._exchange_device(device, self.live)
        self.waiting = True          # the followers are in (or on their way to) the header broadcast
        self.inject = None           # tests: called with (rank, iteration count) before the embed
        self.clock = None            # tools/bench_frepo_driver.py: a dict that collects seconds per phase (adds a device sync per phase)

    # -- collectives (no-ops at world 1) --------------------------------------------------------------------------------------
    def _tick(self, name: str, since: float) -> float:
        """With a ``clock``: wait for the device, add the seconds since ``since`` under ``name``; -> now."""
        if self.clock is None:
            return since
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.clock[name] = self.clock.get(name, 0.0) + (now - since)
        return now

    def _broadcast(self, t: torch.Tensor) -> torch.Tensor:
        if self.live:
            import torch.distributed as dist
            dist.broadcast(t, src=0)
        return t

    def _message(self, kind: int, error: int = 0, idx: int = 0, table: Optional[torch.Tensor] = None) -> torch.Tensor:
        msg = torch.zeros(HEADER + self.batch * self.width, dtype=torch.int64)
        m = 0 if table is None else int(table.shape[0])
        if m:
            msg[HEADER:HEADER + m * self.width] = table.reshape(-1)
        msg[0], msg[1], msg[2], msg[3] = int(kind), int(error), int(idx), m
        return msg.to(self.xdev)

    def _raise_if(self, flag: bool, error: Optional[BaseException], where: str):
        if error is not None:
            raise error
        if flag:
            raise RuntimeError("TargetExchange: another rank failed in %s" % where)

    # -- weights ------------------------------------------------------------------------------------------------------------------
    def sync_weights(self, idx: int, error: Optional[BaseException] = None) -> None:
        """Element ``idx`` of rank 0 -> every rank's shell, behind one status word (step 5)."""
        model = self.models(idx)
        if not self.live:
            self._raise_if(False, error, "the step")
            return
        t0 = self._tick("other", time.perf_counter())
        count = sum(p.numel() for p in model.parameters())
        if self.rank == 0:
            body = torch.zeros(count, dtype=torch.float32, device=self.xdev) if error is not None \
                else evalpool.flat_weights(model).to(self.xdev)
            flat = torch.cat([torch.tensor([0.0 if error is None else 1.0], dtype=torch.float32, device=self.xdev), body])
        else:
            flat = torch.empty(1 + count, dtype=torch.float32, device=self.xdev)
        self._broadcast(flat)
        self._raise_if(float(flat[0]) != 0.0, error, "the step")
        if self.rank != 0:
            evalpool.load_flat_weights(model, flat[1:].to(self.device))
        self._tick("weights", t0)

    def sync_all_weights(self, count: int) -> None:
        """Before the first iteration: every element once."""
        for idx in range(count):
            self.sync_weights(idx)

    # -- one iteration ------------------------------------------------------------------------------------------------------------
    def _embed(self, idx: int, table: torch.Tensor, calls: int) -> torch.Tensor:
        """Steps 2 and 3 on every rank -> ``feat_tar`` (m, d) fp32 on the device."""
        from . import distill
        m = int(table.shape[0])
        lo, hi = rank_slice(m, self.rank, self.world)
        pad, error, feat = pad_rows(m, self.world), None, None
        t0 = self._tick("other", time.perf_counter())
        try:
            model = self.models(idx)
            if self.inject is not None:
                self.inject(self.rank, calls)
            if hi > lo:
                model.eval()
                feat = model.embed_exact(self.fetch(table[lo:hi])).detach().to(torch.float32)
                if feat.dim() != 2 or int(feat.shape[0]) != hi - lo:
                    raise RuntimeError("TargetExchange: embed_exact gave %s for %d clips" % (tuple(feat.shape), hi - lo))
        except Exception as e:          # noqa: BLE001 -- re-raised after the exchange of the flag
            error, feat = e, None
        if not self.live:
            self._raise_if(False, error, "the embedding")
            return feat
        import torch.distributed as dist
        t0 = self._tick("embed", t0)
        word = torch.tensor([0 if error is None else 1, 0 if feat is None else int(feat.shape[1])], dtype=torch.int64, device=self.xdev)
        distill._all_reduce_max(word)
        self._raise_if(int(word[0]) != 0, error, "the embedding")
        d = int(word[1])
        if feat is not None and int(feat.shape[1]) != d:
            raise RuntimeError("TargetExchange: this rank's features are %d wide, another rank's %d" % (int(feat.shape[1]), d))
        mine = torch.zeros((pad, d), dtype=torch.float32, device=self.xdev)
        if feat is not None:
            mine[:hi - lo].copy_(feat)
        gathered = torch.empty((self.world * pad, d), dtype=torch.float32, device=self.xdev)
        dist.all_gather_into_tensor(gathered, mine)
        out = trim_gathered(gathered, m, self.world).to(self.device)
        self._tick("gather", t0)
        return out

    def lead(self, idx: int, table: torch.Tensor, step: Callable[[torch.Tensor], object], calls: int = 0):
        """Rank 0's iteration: ``table`` (m, width) int64 on the host -> what ``step(feat_tar)`` returns."""
        if not 1 <= int(table.shape[0]) <= self.batch or table.numel() != int(table.shape[0]) * self.width:
            raise ValueError("TargetExchange: a table of %s for batches of %d rows of %d" % (tuple(table.shape), self.batch, self.width))
        table = table.reshape(int(table.shape[0]), self.width)
        self._broadcast(self._message(STEP, 0, idx, table))
        self.waiting = False
        feat_tar = self._embed(idx, table, calls)
        out, error = None, None
        try:
            out = step(feat_tar)
        except Exception as e:          # noqa: BLE001
            error = e
        self.sync_weights(idx, error)
        self.waiting = True
        return out

    def lead_ready(self) -> None:
        """Rank 0 has built its side: the followers, who wait for this first, go on to ``sync_all_weights``."""
        self._broadcast(self._message(READY))

    def lead_evaluate(self) -> None:
        """Rank 0 announces an evaluation round; every rank then enters it."""
        self._broadcast(self._message(EVALUATE))
        self.waiting = False

    def lead_stop(self) -> None:
        self._broadcast(self._message(STOP))
        self.waiting = False

    def lead_abort(self) -> None:
        """Rank 0 failed outside an iteration: release the followers, if they are waiting for a header."""
        if self.live and self.waiting:
            self._broadcast(self._message(STOP, 1))
            self.waiting = False

    def follow(self, calls: int = 0) -> int:
        """A follower's turn: receive the header; embed and load the weights (-> STEP), or -> EVALUATE / STOP / READY.  Raises
        when rank 0 reports an error."""
        msg = self._broadcast(torch.zeros(HEADER + self.batch * self.width, dtype=torch.int64, device=self.xdev)).cpu()
        kind, error, idx, m = (int(v) for v in msg[:HEADER])
        if error:
            raise RuntimeError("TargetExchange: rank 0 failed")
        if kind != STEP:
            return kind
        self._embed(idx, msg[HEADER:HEADER + m * self.width].reshape(m, self.width), calls)
        self.sync_weights(idx)
        return STEP


# ---- evaluation (lib_torch/utils.py:522-601) ----------------------------------------------------
def epoch(mode, dataloader, net, optimizer, criterion, args, num_classes: int):
    """FRePo's ``epoch``: no batch standardisation, one pass, MSE on soft labels, accuracy argmax against argmax.  Integer
    labels of a loader are turned into ``one_hot - 1 / C``.  The train step is ``hip_regress_step``; the statistics stay on the
    device until the end of the pass.  -> (loss, accuracy)."""
    net.train() if mode == 'train' else net.eval()
    losses, hits, num_exp = [], [], 0
    for datum in dataloader:
        img = datum[0].float().to(args.device)
        lab = datum[1].to(args.device)
        if not lab.is_floating_point():
            lab = soft_labels(lab, num_classes)
        lab = lab.float()
        n_b = int(lab.shape[0])
        if mode == 'train':
            if not (hasattr(net, "hip_regress_trainable") and net.hip_regress_trainable(img, optimizer, criterion)):
                raise NotImplementedError("frepo.epoch: the train step runs ConvNet3D.hip_regress_step (AdamW, nn.MSELoss); there "
                                          "is no torch-op fallback")
            output, loss = net.hip_regress_step(img, lab, optimizer)
        else:
            with torch.no_grad():
                output = net(img)
                loss = criterion(output, lab)
        losses.append(loss.detach().reshape(1) * n_b)
        hits.append((output.detach().argmax(dim=-1) == lab.argmax(dim=-1)).sum().reshape(1))
        num_exp += n_b
    return float(torch.cat(losses).sum().cpu()) / num_exp, float(torch.cat(hits).sum().cpu()) / num_exp


def evaluate_synset(it_eval, net, images_train, labels_train, testloader, args, num_classes: int, test_freq=None):
    """FRePo's ``evaluate_synset``, mode 'none': ``epoch_eval_train + 1`` epochs of AdamW(lr_net, weight decay 5e-4) under the
    chained schedule (warm-up over a tenth of the epochs, cosine to 0.01 lr_net), MSE on the soft labels ``labels_train``; one
    test pass at the end (and every ``test_freq`` epochs).  -> (net, acc_train, acc_test)."""
    from .utils import TensorDataset, get_time
    net = net.to(args.device)
    lr, Epoch = float(args.lr_net), int(args.epoch_eval_train)
    optimizer = torch.optim.AdamW(net.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=0.0005)
    scheduler = chained_schedule(optimizer, int((Epoch + 1) * 0.1), Epoch + 1, lr * 0.01)
    criterion = nn.MSELoss().to(args.device)
    trainloader = torch.utils.data.DataLoader(TensorDataset(images_train.to(args.device), labels_train.to(args.device)),
                                              batch_size=args.batch_train, shuffle=True, num_workers=0)
    start = time.time()
    for ep in range(Epoch + 1):
        loss_train, acc_train = epoch('train', trainloader, net, optimizer, criterion, args, num_classes)
        if test_freq is not None and ep % test_freq == 0:
            epoch('test', testloader, net, optimizer, criterion, args, num_classes)
        scheduler.step()
    time_train = time.time() - start
    loss_test, acc_test = epoch('test', testloader, net, optimizer, criterion, args, num_classes)
    print('%s Evaluate_%02d: epoch = %04d train time = %d s train loss = %.6f train acc = %.4f, test acc = %.4f' % (
        get_time(), it_eval, Epoch, int(time_train), loss_train, acc_train, acc_test))
    return net, acc_train, acc_test


def train_network(net, images_train, labels_train, args):
    """``evaluate_synset``'s training loop without its test -> (loss, accuracy) of the last epoch; the number of classes is the
    width of the soft labels."""
    from .utils import TensorDataset
    net = net.to(args.device)
    num_classes = int(labels_train.shape[1])
    lr, Epoch = float(args.lr_net), int(args.epoch_eval_train)
    optimizer = torch.optim.AdamW(net.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=0.0005)
    scheduler = chained_schedule(optimizer, int((Epoch + 1) * 0.1), Epoch + 1, lr * 0.01)
    criterion = nn.MSELoss().to(args.device)
    trainloader = torch.utils.data.DataLoader(TensorDataset(images_train.to(args.device), labels_train.to(args.device)),
                                              batch_size=args.batch_train, shuffle=True, num_workers=0)
    loss_train, acc_train = 0.0, 0.0
    for ep in range(Epoch + 1):
        loss_train, acc_train = epoch('train', trainloader, net, optimizer, criterion, args, num_classes)
        scheduler.step()
    return float(loss_train), float(acc_train)


def test_pass(net, testloader, args, rec: torch.Tensor) -> torch.Tensor:
    """``epoch('test')`` as one ``vdr_regress_stats`` launch per batch into ``rec``: no standardisation, the integer labels
    straight from the loader (the kernel forms ``one_hot - 1 / K`` itself)."""
    net = net.to(args.device)
    net.eval()
    with torch.no_grad():
        for datum in testloader:
            img = datum[0].float().to(args.device)
            lab = datum[1].to(args.device)
            if lab.is_floating_point():
                raise ValueError("frepo.test_pass: the test loader yields integer labels")
            hip.regress_stats(net(img), lab, rec)
    return rec


# FRePo's evaluation for ``evalpool.evaluate_pool(recipe=)``: one test pass, loss = rec[1] / (K * clips)
EVAL_RECIPE = evalpool.Recipe(train_network, test_pass, 1, loss_scale=lambda K: float(K))
