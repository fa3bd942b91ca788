"""fp64 NumPy restatement of the coreset selection criteria on a class's centred Gram matrix (the test oracle of
video_distillation_amd/coreset.py; tests/test_coreset_cpu.py pins it to the reference's picks in tests/golden/g18_coreset.npz).

Each function returns (picks, gaps, own): ``gaps[t]`` is the relative margin of the oracle's own choice ``own[t]`` at step t
over the runner-up under the criterion (|best - second| / the largest |G[j,j]|), which is what decides whether a differing pick
is a near-tie.  Without ``follow``, ``picks == own``."""
import numpy as np


def centred_gram(f: np.ndarray) -> np.ndarray:
    f = np.asarray(f, dtype=np.float64)
    f = f - f.mean(0, keepdims=True)
    return f @ f.T


def _argmin(v: np.ndarray, ok: np.ndarray, scale: float):
    idx = np.flatnonzero(ok)
    vals = v[idx]
    k = int(np.argmin(vals))           # first occurrence: the lowest index among ties
    s = np.sort(vals)
    gap = (s[1] - s[0]) / scale if len(s) > 1 else np.inf
    return int(idx[k]), gap


def herding(G: np.ndarray, ipc: int, follow=None):
    """argmin_{j not chosen} G[j,j] + 2 sum_chosen G[s,j].  ``follow``: a pick sequence to route the oracle on (its own pick is
    replaced by follow[t] from step t on, so that a near-tie decided otherwise does not end the comparison)."""
    n = G.shape[0]
    diag, acc, ok = np.diag(G).copy(), np.zeros(n), np.ones(n, bool)
    scale = max(float(np.abs(diag).max()), 1e-300)
    picks, gaps, own = [], [], []
    for t in range(ipc):
        p, gap = _argmin(diag + 2 * acc, ok, scale)
        own.append(p)
        if follow is not None:
            p = int(follow[t])
        picks.append(p)
        gaps.append(gap)
        ok[p] = False
        acc += G[p]
    return picks, gaps, own


def kcenter_greedy(G: np.ndarray, ipc: int, follow=None):
    """First argmin_j G[j,j] (closest to the mean), then argmax_{j not chosen} min_{c chosen} |f_j - f_c|^2."""
    n = G.shape[0]
    diag, ok = np.diag(G).copy(), np.ones(n, bool)
    mind = np.full(n, np.inf)
    scale = max(float(np.abs(diag).max()), 1e-300)
    picks, gaps, own = [], [], []
    for t in range(ipc):
        p, gap = _argmin(diag if t == 0 else -mind, ok, scale)
        own.append(p)
        if follow is not None:
            p = int(follow[t])
        picks.append(p)
        gaps.append(gap)
        ok[p] = False
        mind = np.minimum(mind, diag + diag[p] - 2 * G[p])
    return picks, gaps, own


def kcenter_reference(G: np.ndarray, ipc: int):
    """What distill_coreset.py's k-center branch outputs: the clip closest to the mean, then (ipc 2) the class's first clip;
    ipc >= 3 raises there."""
    if ipc >= 3:
        raise ValueError("the reference's k-center fails at ipc >= 3")
    first, gaps, _ = kcenter_greedy(G, 1)
    picks = (first + [0])[:ipc]
    return picks, (gaps + [np.inf])[:ipc], picks


def select(G: np.ndarray, ipc: int, method: str, kcenter: str = "greedy", follow=None):
    if method == "herding":
        return herding(G, ipc, follow)
    if kcenter == "reference":
        return kcenter_reference(G, ipc)
    return kcenter_greedy(G, ipc, follow)
