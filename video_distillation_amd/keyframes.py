"""Key-frame memories: the one definition of the temporal tables (``table``), the frames ``--init real`` starts the keys from
(``init_frames``) and the torch expressions of expand / reduce in the kernels' operation order (csrc/keyframes.hip).

A memory is K frames (K, 3, H, W); frame t of its clip of T frames is ``w0[t] * key i0[t] + w1[t] * key i1[t]``.

``nearest`` (the paper's segments) and K == 1:  ``i0[t] = i1[t] = (t*K) // T``, ``w0 = 1``, ``w1 = 0``.
``linear`` with K >= 2 (T >= 2), ``num = t*(K-1)``, ``den = T-1``:  ``i0 = min(num // den, K-2)``, ``i1 = i0 + 1``,
``w1 = float32((num - i0*den) / den)`` (the quotient in fp64, then rounded), ``w0 = float32(1 - float64(w1))`` -- linear
interpolation along T with aligned end points: the first frame is the first key, the last frame the last key (``w1 = 1``,
``w0 = 0``).  At K == T both kinds are the identity (one weight of exactly 1 per frame); K == 1 is the still clip.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MAX_FRAMES = 64          # include/vd_keyframes.h VDK_MAX_FRAMES
INTERPS = ("linear", "nearest")


@dataclass(eq=False)
class Table:
    """The four length-T arrays (``i0``, ``i1`` int32; ``w0``, ``w1`` float32) with T, K and the kind; unpacks into the arrays."""
    T: int
    K: int
    interp: str
    i0: np.ndarray
    i1: np.ndarray
    w0: np.ndarray
    w1: np.ndarray
    _vdk: object = field(default=None, repr=False)          # hip.vdk_table's ctypes mirror, built when a kernel is first called

    def __iter__(self):
        return iter((self.i0, self.i1, self.w0, self.w1))

    def terms(self, k: int):
        """The non-zero terms of key ``k`` in the order reduce adds them: [(t, w)], ascending t, i0 before i1."""
        out = []
        for t in range(self.T):
            for idx, w in ((self.i0[t], self.w0[t]), (self.i1[t], self.w1[t])):
                if int(idx) == k and float(w) != 0.0:
                    out.append((t, float(w)))
        return out


def table(T: int, K: int, interp: str = "linear") -> Table:
    T, K = int(T), int(K)
    if interp not in INTERPS:
        raise ValueError("key frames: interp %r is none of %s" % (interp, INTERPS))
    if K < 1 or K > T or T > MAX_FRAMES:
        raise ValueError("key frames: 1 <= K (%d) <= T (%d) <= %d" % (K, T, MAX_FRAMES))
    if interp == "linear" and K > 1 and T < 2:
        raise ValueError("key frames: linear interpolation between %d keys needs T >= 2" % K)
    t = np.arange(T, dtype=np.int64)
    if interp == "nearest" or K == 1:
        i0 = (t * K) // T
        i1 = i0.copy()
        w0, w1 = np.ones(T, dtype=np.float32), np.zeros(T, dtype=np.float32)
    else:
        num, den = t * (K - 1), T - 1
        i0 = np.minimum(num // den, K - 2)
        i1 = i0 + 1
        w1 = ((num - i0 * den).astype(np.float64) / float(den)).astype(np.float32)
        w0 = (1.0 - w1.astype(np.float64)).astype(np.float32)
    return Table(T, K, interp, i0.astype(np.int32), i1.astype(np.int32), w0, w1)


def init_frames(T: int, K: int, interp: str = "linear"):
    """The frame of a real clip that key k starts from (``--init real``): for linear with K >= 2 the frame nearest to where
    the key sits on the time axis, ``(k*(T-1) + (K-1)//2) // (K-1)``; for nearest or K == 1 the first frame of its segment,
    ``(k*T + K - 1) // K``.  K == T: frame k either way."""
    table(T, K, interp)          # (the refusals)
    if interp == "linear" and K >= 2:
        return [(k * (T - 1) + (K - 1) // 2) // (K - 1) for k in range(K)]
    return [(k * T + K - 1) // K for k in range(K)]


def expand_torch(keys, tab: Table):
    """(n, K, 3, H, W) -> (n, T, 3, H, W) in torch, operation for operation what ``vdk_keyframe_expand`` computes: a zero weight's
    term is skipped, a weight of 1 copies, every product and the add are separate fp32 operations."""
    import torch
    if keys.dim() != 5 or int(keys.shape[1]) != tab.K:
        raise ValueError("keyframe expand: keys (n, %d, 3, H, W), not %s" % (tab.K, tuple(keys.shape)))
    out = torch.empty((keys.shape[0], tab.T) + tuple(keys.shape[2:]), dtype=keys.dtype, device=keys.device)
    for t in range(tab.T):
        r = None
        for idx, w in ((int(tab.i0[t]), float(tab.w0[t])), (int(tab.i1[t]), float(tab.w1[t]))):
            if w == 0.0:
                continue
            p = keys[:, idx] if w == 1.0 else keys[:, idx] * w
            r = p if r is None else r + p
        if r is None:
            out[:, t].zero_()
        else:
            out[:, t] = r
    return out


def reduce_torch(g, tab: Table):
    """(n, T, 3, H, W) -> (n, K, 3, H, W) in torch, operation for operation what ``vdk_keyframe_reduce`` computes: per key the
    products of its terms in ascending t (i0 before i1), the accumulator started from the first product, 0 without a term."""
    import torch
    if g.dim() != 5 or int(g.shape[1]) != tab.T:
        raise ValueError("keyframe reduce: g (n, %d, 3, H, W), not %s" % (tab.T, tuple(g.shape)))
    out = torch.zeros((g.shape[0], tab.K) + tuple(g.shape[2:]), dtype=g.dtype, device=g.device)
    for k in range(tab.K):
        acc = None
        for t, w in tab.terms(k):
            p = g[:, t] if w == 1.0 else g[:, t] * w
            acc = p if acc is None else acc + p
        if acc is not None:
            out[:, k] = acc
    return out
