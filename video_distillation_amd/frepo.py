"""FRePo(+Ours) on the HIP path: the method of the reference's FRePo/script/distill_s2d.py, with its names and semantics.

  * ``lb_margin_th``                    the label-margin loss (:21-26)
  * ``SynData`` / ``S2DSynData``        the synthetic set: clips, or static + dynamic memories and hallucinators (:47-86)
  * ``PoolElement``                     one network of the model pool with its Adam optimiser and chained schedule, trained
                                        online on the synthetic set and reset after ``max_online_updates`` steps (:90-178)
  * ``FRePoTrainer.step``               one iteration of the loop (:343-367)
  * ``evaluate_synset`` / ``epoch``     FRePo's own evaluation: AdamW, MSE on soft labels (lib_torch/utils.py:522-601)
  * ``soft_labels`` / ``y_scale``       the label construction (:253-263)
  * ``hip_adam_step``                   ``optimizer.step()`` of any torch Adam / AdamW in ``vdf_adam_multi`` launches

The numerically hard centre is ``nfr.nfr`` (csrc/nfr.hip, fp64); every network step is ``ConvNet3D.hip_regress_step`` (the MFMA
forward / backward passes of the cross-entropy step with ``vdf_mse_loss`` and one ``vdf_adam_multi`` launch, csrc/frepo.hip).
The label-margin loss and the loss line are a handful of torch expressions on (n, C) and (m, C) tensors.

Not here: more than one rank, wandb, ``--eval_ranks all``, the blocked Cholesky of DESIGN 19.
"""
from __future__ import annotations

import random
import time
from typing import List, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip


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

    def nfr(self, x_syn, y_syn, x_tar, reg=1e-6, use_flip=False):
        from . import nfr
        return nfr.nfr(self.model, x_syn, y_syn, x_tar, reg=reg, use_flip=use_flip, exact=True)

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

    def step(self, x_target: torch.Tensor, y_target: torch.Tensor):
        """-> (loss, ln_loss, lb_loss) as device scalars."""
        x_syn, y_syn = self.syndata()
        idx = int(np.random.randint(low=0, high=len(self.pools)))
        self.last_idx = idx
        pool_m = self.pools[idx]
        y_pred = pool_m.nfr(x_syn, y_syn, x_target, reg=self.reg, use_flip=False)
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
