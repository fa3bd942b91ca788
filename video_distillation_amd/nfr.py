"""FRePo's "neural feature regression" predictor (FRePo/script/distill_s2d.py:124-137, ``PoolElement.nfr``) on the HIP path.

``nfr_pred(feat_syn, y_syn, feat_tar, reg)`` is the kernel ridge predictor on given features,

    pred = K_ts (K_ss + |reg| tr(K_ss) / n  I)^-1 y_syn,      K_ss = feat_syn feat_syn^T,  K_ts = feat_tar feat_syn^T,

differentiable once with respect to ``feat_syn`` and ``y_syn``; ``nfr(net, x_syn, y_syn, x_tar, reg, use_flip)`` is what
``PoolElement.nfr`` computes for a ``get_network('ConvNet3D')`` network.  The reference's loss line
``criterion(pred, y).sum(-1).mean(0)`` and ``loss.backward()`` then run unchanged: the gradient reaches the synthetic pixels and
labels and, through ``utils.Conv3DNet``, a dynamic memory and a hallucinator.

The solve and every product around it run in fp64 in csrc/nfr.hip (include/vd_nfr.h has the algebra): the system's condition
number reaches 1e7 at reg = 1e-6, where the reference's fp32 solve loses the feature gradient.  ``pred`` and the gradients are
the fp64 results rounded to fp32 once.  One deliberate difference from the reference: its lambda passes through a float32
``torch.eye``; here lambda is an fp64 number.  There is no CPU and no torch-op path.

The model pool and its online training, the label-margin loss, the optimiser of the synthetic data and the trainer are
``frepo.py``; the driver and its file formats are ``run_frepo.py``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import hip


class _NfrFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_syn, y_syn, feat_tar, reg):
        fs, ys, ft = (t.detach().contiguous() for t in (feat_syn, y_syn, feat_tar))
        pred, workspace = hip.nfr_forward(fs, ys, ft, reg)
        ctx.save_for_backward(fs, ft, workspace)
        ctx.reg = reg
        return pred.to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pred):
        fs, ft, workspace = ctx.saved_tensors
        g_feat, g_y = hip.nfr_backward(fs, ft, g_pred.to(torch.float32).contiguous(), workspace, ctx.reg)
        return (g_feat.to(torch.float32) if ctx.needs_input_grad[0] else None,
                g_y.to(torch.float32) if ctx.needs_input_grad[1] else None, None, None)


def nfr_pred(feat_syn: torch.Tensor, y_syn: torch.Tensor, feat_tar: torch.Tensor, reg: float = 1e-6) -> torch.Tensor:
    """The kernel ridge predictor on features: ``feat_syn`` (n, d), ``y_syn`` (n, C), ``feat_tar`` (m, d), fp32 on one HIP
    device -> ``pred`` (m, C) fp32.  Differentiable once with respect to ``feat_syn`` and ``y_syn``; ``feat_tar`` carries no
    gradient (``ValueError`` when it requires one).  A system whose pivots are not all positive and finite (all-zero or
    non-finite features) gives NaN, never a plausible number; nothing is read on the host."""
    if feat_tar.requires_grad:
        raise ValueError("nfr_pred: feat_tar carries no gradient (the reference takes it under no_grad): detach it")
    for name, t in (("feat_syn", feat_syn), ("y_syn", y_syn), ("feat_tar", feat_tar)):
        if t.dtype != torch.float32:
            raise ValueError("nfr_pred: %s is %s, not float32" % (name, t.dtype))
    return _NfrFunction.apply(feat_syn, y_syn, feat_tar, float(reg))


def nfr(net, x_syn: torch.Tensor, y_syn: torch.Tensor, x_tar: torch.Tensor, reg: float = 1e-6, use_flip: bool = False,
        exact: bool = False, feat_tar: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``PoolElement.nfr`` (distill_s2d.py:124-137) with ``weight_grad=False``: the network in eval mode with frozen parameters,
    the target clips embedded under ``no_grad`` first, the synthetic clips with the graph kept; ``use_flip`` doubles the
    synthetic set by its mirror along W.  ``x_syn`` (n, T, 3, H, W), ``y_syn`` (n, C), ``x_tar`` (m, T, 3, H, W) -> ``pred``
    (m, C).

    ``exact``: both sides are multiplied by the exact weights in hi+lo pairs -- the targets through ``net.embed_exact`` (no
    dithered operand sets), the synthetic clips without the value pass that rounds the weights to the real side's format -- which
    is what the solve needs once two synthetic clips come close.  ``net.real_dither`` is afterwards as the caller
    left it.  The default is ``embed`` on both sides, as before.

    ``feat_tar`` (m, d): the target features, embedded elsewhere (``frepo.TargetExchange``: by other ranks); ``x_tar`` is then
    not read and may be None."""
    if use_flip:
        x_syn = torch.cat((x_syn, torch.flip(x_syn, dims=[-1])), dim=0)
        y_syn = torch.cat((y_syn, y_syn), dim=0)
    net.eval()
    if not exact:
        if feat_tar is None:
            with torch.no_grad():
                feat_tar = net.embed(x_tar)
        net.requires_grad_(False)
        feat_syn = net.embed(x_syn)
        return nfr_pred(feat_syn, y_syn, feat_tar, reg)
    if feat_tar is None:
        feat_tar = net.embed_exact(x_tar)
    net.requires_grad_(False)
    had, before = "real_dither" in vars(net), getattr(net, "real_dither", "auto")
    net.real_dither = True          # (the caller states that no undithered rn16 side exists: the value pass is never run)
    try:
        feat_syn = net.embed(x_syn)
    finally:
        if had:
            net.real_dither = before
        else:
            del net.real_dither
    return nfr_pred(feat_syn, y_syn, feat_tar, reg)
