"""numpy fp64 restatement of the vd_eval_stats record (include/vd_hip.h) and the planted cases its CPU and GPU tests share.
Written clip by clip from the definitions, with no torch: independent of both hip.eval_stats branches."""
import numpy as np

HEAD = 8
SHAPES = ((1, 3), (4, 5), (64, 50), (7, 400))
RTOL_CE = 1e-12          # rec[1]: <= 256 fp64 terms summed in another order move it by about 256 * 2^-53 = 3e-14


def record(logits, labels, rec=None):
    """rec (8 + 2K doubles, accumulated) for fp32 logits (B, K) and int64 labels (B,)."""
    z = np.asarray(logits, dtype=np.float32)
    B, K = z.shape
    rec = np.zeros(HEAD + 2 * K, dtype=np.float64) if rec is None else rec
    ce = []
    for b in range(B):
        y = int(labels[b])
        if y < 0 or y >= K:
            rec[5] += 1
            continue
        row = z[b].astype(np.float64)
        rank = sum(1 for k in range(K) if row[k] > row[y] or (row[k] == row[y] and k < y))
        m = row.max()
        ce.append(m + np.log(np.exp(row - m).sum()) - row[y])
        rec[0] += 1
        rec[2] += rank < 1
        rec[3] += rank < 3
        rec[4] += rank < 5
        rec[HEAD + y] += rank < 1
        rec[HEAD + K + y] += 1
    rec[1] += float(np.sum(np.asarray(ce, dtype=np.float64))) if ce else 0.0
    return rec


def planted(B, K, seed=0):
    """fp32 logits and labels of shape (B, K) with, where B allows: exact ties of the label's logit at the row maximum with a
    class below it, above it and on both sides (the tie decides top-1), a tie in the middle of the ranking (it decides top-3 /
    top-5), a label of -1 and a label of K.  B = 1: one clip whose K logits are all equal, label in the middle."""
    rng = np.random.default_rng(1000 * B + K + seed)
    z = (rng.standard_normal((B, K)) * 3).astype(np.float32)
    y = rng.integers(0, K, size=B).astype(np.int64)
    if B == 1:
        z[0, :] = np.float32(0.5)
        y[0] = K // 2
        return z, y
    top = np.float32(z.max() + 1)
    y[0] = K // 2; z[0, y[0]] = top; z[0, y[0] - 1] = top                      # equal maximum BELOW the label: rank 1
    y[1] = K // 2; z[1, y[1]] = top; z[1, y[1] + 1] = top                      # equal maximum ABOVE the label: rank 0
    y[2] = -1
    y[3] = K
    if B > 6:
        y[4] = K // 2; z[4, y[4] - 1:y[4] + 2] = top                         # both sides
        order = np.argsort(-z[5], kind="stable")
        y[5] = order[2]                                                        # the third largest ...
        lower = [k for k in range(K) if k < y[5] and k not in order[:2]]
        if lower:
            z[5, lower[0]] = z[5, y[5]]                                        # ... tied with a lower index: rank 3, out of top-3
        order = np.argsort(-z[6], kind="stable")
        y[6] = order[4]
        higher = [k for k in range(K) if k > y[6] and k not in order[:4]]
        if higher:
            z[6, higher[0]] = z[6, y[6]]                                       # tied with a higher index: rank 4, still top-5
    return z, y


def assert_record(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    ce_err = abs(got[1] - want[1]) / max(abs(want[1]), 1e-300)
    print("%s: clips %d, CE sum %.17g (oracle %.17g, rel %.2e)" % (what, want[0], got[1], want[1], ce_err))
    counts = np.arange(got.size) != 1
    assert np.array_equal(got[counts], want[counts]), (what, got[:HEAD], want[:HEAD])
    assert got[6] == 0 and got[7] == 0
    assert ce_err <= RTOL_CE or got[1] == want[1], (what, got[1], want[1])
