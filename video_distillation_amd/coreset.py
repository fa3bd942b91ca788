"""Coreset baselines on the HIP path: herding and k-center selection of real clips (the reference's distill_coreset.py:59-109).

Both methods rank the clips of one class by distances between their features.  They are translation invariant, so the
selection runs on the centred Gram matrix of each class, ``G~ = (F - m)(F - m)^T``, built in fp64 from the fp32 features
(csrc/coreset.hip: one launch for the class means and G~, one for all ``ipc`` greedy steps of every class; no host
synchronisation per step):

* herding (exactly the reference): pick ``argmin_{j not chosen} ||(i+1) m - sum_chosen f - f_j||``, i.e.
  ``argmin G~[j,j] + 2 sum_chosen G~[s,j]``;
* k-center (``kcenter="greedy"``, the default): greedy farthest point -- first the clip closest to the class mean (the
  reference's first pick), then the clip farthest from its nearest chosen clip (chosen clips are not picked again).  The
  reference's loop intends this algorithm (DatasetCondensation issue #21) but its broadcasting breaks it from the second pick
  on: ``kcenter="reference"`` reproduces what the reference script outputs at ipc <= 2 (its second pick is always the class's
  first clip) and refuses ipc >= 3, where the reference raises.

Ties go to the lowest index, as torch's ``argmin`` / ``argmax`` do.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import torch

METHODS = ("herding", "k-center")
KCENTER_MODES = ("greedy", "reference")
_WORKSPACE_BUDGET = 256 << 20          # bytes of fp64 Gram blocks per launch pair; larger selections run in class groups
_ENGINES: Dict[tuple, object] = {}


def _host_ints(v) -> List[int]:
    if isinstance(v, torch.Tensor):
        return [int(x) for x in v.detach().cpu().tolist()]
    return [int(x) for x in v]


def _check_args(counts: Sequence[int], ipc: int, method: str, kcenter: str, allow_short: bool) -> None:
    if method not in METHODS:
        raise NotImplementedError("coreset method %r (the reference knows 'herding' and 'k-center')" % (method,))
    if kcenter not in KCENTER_MODES:
        raise ValueError("kcenter must be one of %s, not %r" % (KCENTER_MODES, kcenter))
    if int(ipc) < 1:
        raise ValueError("ipc must be >= 1, not %d" % ipc)
    if method == "k-center" and kcenter == "reference" and ipc >= 3:
        raise ValueError("kcenter='reference' reproduces distill_coreset.py's k-center, which fails at ipc >= 3: "
                         "`features - features[idx_centers]` broadcasts (N, D) against (ipc - 1, D) and raises; "
                         "use kcenter='greedy' (the farthest-point algorithm that loop intends)")
    if not allow_short:
        for c, n in enumerate(counts):
            if n < ipc:
                raise ValueError("class %d has %d clips, fewer than ipc = %d (the reference's argmin fails on an empty "
                                 "tensor there)" % (c, n, ipc))


def select(features: torch.Tensor, counts, offsets, ipc: int, method: str, kcenter: str = "greedy",
           allow_short: bool = False) -> torch.Tensor:
    """Picks of every class, class-major and in selection order: LongTensor (C * ipc,) on the features' device, entry
    ``c * ipc + t`` = the row of ``features`` of class c's pick t.  ``features`` (rows, D) fp32; class c owns rows
    ``offsets[c] .. offsets[c] + counts[c] - 1``.  ``allow_short``: a class with fewer than ``ipc`` rows gets -1 for its
    picks instead of a ValueError."""
    counts, offsets = _host_ints(counts), _host_ints(offsets)
    _check_args(counts, ipc, method, kcenter, allow_short)
    if len(counts) != len(offsets) or not counts:
        raise ValueError("counts and offsets must be non-empty and of equal length")
    if features.dim() != 2:
        raise ValueError("features must be (rows, D), not %s" % (tuple(features.shape),))
    for n, o in zip(counts, offsets):
        if n < 0 or o < 0 or o + n > features.shape[0]:
            raise ValueError("class rows %d .. %d lie outside the %d feature rows" % (o, o + n, features.shape[0]))
    from . import hip
    if not features.is_cuda:
        raise RuntimeError("coreset.select runs on a HIP device (no CPU path)")
    if method == "k-center" and kcenter == "reference":
        first = select(features, counts, offsets, 1, "k-center", allow_short=allow_short)
        if ipc == 1:
            return first
        # the reference's second pick: argmax of a 0-d tensor, i.e. the class's first clip
        second = torch.tensor([o if n >= ipc else -1 for n, o in zip(counts, offsets)], dtype=torch.int64, device=features.device)
        first = torch.where(second < 0, second, first)
        return torch.stack([first, second], 1).reshape(-1)
    feats = features.detach().to(torch.float32).contiguous()
    dev = feats.device
    C, D = len(counts), int(feats.shape[1])
    out = torch.empty(C * ipc, dtype=torch.int64, device=dev)
    L = hip.lib()
    code = hip.CORESET_METHOD[method]
    # classes in groups whose Gram blocks (group size x max count^2 fp64) stay within the workspace budget
    c0 = 0
    while c0 < C:
        c1, mc = c0, 0
        while c1 < C:
            m = max(mc, counts[c1], 1)
            if c1 > c0 and (c1 - c0 + 1) * m * m * 8 > _WORKSPACE_BUDGET:
                break
            mc, c1 = m, c1 + 1
        nb = int(L.vd_coreset_workspace_bytes(c1 - c0, mc))
        if nb < 0:
            raise ValueError("a class of %d clips exceeds the selection kernel's limit" % mc)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        cnt = torch.tensor(counts[c0:c1], dtype=torch.int32).to(dev)
        ofs = torch.tensor(offsets[c0:c1], dtype=torch.int64).to(dev)
        hip.run("vd_coreset_select", hip.ptr(feats), D, hip.ptr(ofs), hip.ptr(cnt), c1 - c0, mc, int(ipc), code,
                hip.ptr(out[c0 * ipc:]), hip.ptr(ws), nb, hip.stream_ptr(dev))
        c0 = c1
    return out


def _engine(geo, device):
    from . import engine
    device = torch.device(device)
    key = (geo.frames, geo.height, geo.width, device.index if device.index is not None else torch.cuda.current_device())
    eng = _ENGINES.get(key)
    if eng is None:
        eng = engine.EmbedEngine(geo, prec="f16x3", device=device)
        _ENGINES[key] = eng
    return eng


def _feature_params(net) -> List[torch.Tensor]:
    if hasattr(net, "module"):
        net = net.module
    return [p.detach() for p in net._feature_params()]


def class_features(net, pool, classes: Sequence[int], chunk: int = 512) -> Tuple[torch.Tensor, List[int], List[int]]:
    """Features of every clip of ``classes`` of the resident ``pool`` (distill.RealPool): (rows, D) fp32 on the pool's device,
    class ``classes[k]`` in rows ``offsets[k] .. offsets[k] + counts[k] - 1``; returns (features, counts, offsets).

    The clips run through an ``engine.EmbedEngine`` in f16x3 (hi+lo fp16 pairs, fp32-grade) with the net's EXACT weights --
    the format ``net.embed`` gives clips that carry a gradient.  ``net.embed`` on a frozen net without gradient is not used: it
    takes the DM real side's single-pass f16 path and, for batches of >= 4 clips, deals clip j to dithered weight set j mod G.
    That keeps a class MEAN unbiased, but every clip then carries its own rounding perturbation of ~1e-4 .. 1e-3 of |f|, and
    selection ranks single clips by distance, where such perturbations decide near-ties.  The clips are read out of
    ``pool.clips`` through an index (gather fused into the first layer's conversion), ``chunk`` clips per forward, without a
    copy per class."""
    from . import plan as P
    clips = pool.clips
    geo = P.NetGeometry(int(clips.shape[1]), int(clips.shape[3]), int(clips.shape[4]))
    eng = _engine(geo, clips.device)
    eng.set_weights([p.to(clips.device, torch.float32) for p in _feature_params(net)])
    counts = [int(pool.counts[c]) for c in classes]
    offsets, o = [], 0
    for n in counts:
        offsets.append(o)
        o += n
    feats = torch.empty((o, eng.num_feat), dtype=torch.float32, device=clips.device)
    index = torch.cat([torch.arange(pool.offsets[c], pool.offsets[c] + n, dtype=torch.int64) for c, n in zip(classes, counts)]) \
        if classes else torch.zeros(0, dtype=torch.int64)
    index = index.to(clips.device)
    for r0 in range(0, o, int(chunk)):
        r1 = min(o, r0 + int(chunk))
        feats[r0:r1] = eng.forward(clips, index=index[r0:r1])
    return feats, counts, offsets


def build_synset(net, pool, num_classes: int, ipc: int, method: str, kcenter: str = "greedy", chunk: int = 512,
                 group_clips: int = 16384, stats: Optional[dict] = None):
    """The reference's ``image_syn`` / ``label_syn`` (distill_coreset.py:67-105) from the resident pool: returns
    (image_syn (num_classes * ipc, T, 3, H, W), label_syn [0]*ipc + [1]*ipc + ..., index) where ``index`` holds the pool rows
    picked, class-major in selection order, and ``image_syn`` rows are those pool clips bit for bit.  Classes are embedded and
    selected in groups of about ``group_clips`` clips, so the features of a large pool are never all resident.  ``stats``
    (a dict) receives ``embed_s`` and ``select_s`` (wall time, device-synchronised)."""
    counts = [int(pool.counts[c]) for c in range(num_classes)]
    _check_args(counts, ipc, method, kcenter, allow_short=False)
    dev = pool.clips.device
    index = torch.empty(num_classes * ipc, dtype=torch.int64, device=dev)
    t_embed = t_sel = 0.0
    c0 = 0
    while c0 < num_classes:
        c1, n = c0, 0
        while c1 < num_classes and (c1 == c0 or n + counts[c1] <= group_clips):
            n, c1 = n + counts[c1], c1 + 1
        classes = list(range(c0, c1))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        feats, cnt, ofs = class_features(net, pool, classes, chunk=chunk)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        rows = select(feats, cnt, ofs, ipc, method, kcenter=kcenter)
        # feature row -> pool row: class k's rows start at ofs[k] in feats and at pool.offsets[c] in the pool
        shift = torch.tensor([pool.offsets[c] - o for c, o in zip(classes, ofs)], dtype=torch.int64, device=dev)
        index[c0 * ipc:c1 * ipc] = rows + shift.repeat_interleave(ipc)
        torch.cuda.synchronize(dev)
        t_embed, t_sel = t_embed + (t1 - t0), t_sel + (time.perf_counter() - t1)
        del feats
        c0 = c1
    image_syn = pool.clips[index]
    label_syn = torch.arange(num_classes, dtype=torch.long, device=dev).repeat_interleave(ipc)
    if stats is not None:
        stats["embed_s"], stats["select_s"] = t_embed, t_sel
    return image_syn, label_syn, index
