"""An fp64 torch restatement of FRePo's kernel ridge predictor (distill_s2d.py:133-136) and of its gradient, in two independent
forms, for tests/test_nfr_cpu.py and tests/test_gpu_nfr.py.  Not a test module.

  (a) ``by_autograd``: the defining expressions, the gradient by autograd through ``torch.linalg.solve``.
  (b) ``by_formulas``: the explicit forward and backward formulas of include/vd_nfr.h with a Cholesky factor.

Both take lambda = |reg| tr(K) / n as an fp64 number (the reference rounds it to fp32 through a float32 ``torch.eye``: form (a)
meets the fixture tests/golden/nfr/values.npz, written by the reference's own ``PoolElement.nfr`` on double inputs, to about
1e-6, not to fp64).

The bar of every comparison of two fp64 evaluations is ``bar(cond) = 16 * cond_2(A) * 2^-53`` in rel-L2: two correct fp64
evaluations in different summation orders differ by a multiple of cond_2(A) * 2^-53; that multiple, measured on the CPU between a
hand-rolled Cholesky with 4-wide chunked Gram sums and (a) over ``CASES``, was 0.1 - 0.6.  At the worst-conditioned case
(cond 1.5e7) the bar is 2.7e-8, below fp32's 2^-24: an fp32 accumulation, solve or intermediate anywhere fails every case.
"""
import numpy as np
import torch

# (n, m, d, C, reg, duplicate rows)
CASES = [
    (1, 1, 1, 1, 1e-6, False),              # the smallest of everything
    (3, 5, 7, 3, 1e-6, False),              # nothing is a multiple of 4 or 16
    (16, 16, 4, 2, 1e-6, False),            # exactly one matrix tile and one k step
    (17, 33, 36, 5, 1e-6, False),           # one past each tile edge and one past a 32-wide LDS stage
    (33, 40, 256, 5, 1e-6, False),          # configuration 1's feature width
    (65, 70, 100, 7, 1e-6, False),
    (12, 9, 8, 3, 1e-6, False),             # n > d: a rank-deficient K, only the regulariser makes A positive definite
    (40, 32, 24, 6, 1e-6, False),
    (16, 20, 64, 4, 1e-6, True),            # rows 1 and 5 of F_s copied from rows 0 and 4
    (16, 20, 64, 4, 1e-3, True),
    (50, 64, 2048, 50, 1e-6, False),        # the workload's n, d and C at a small m
]


def case_id(case) -> str:
    n, m, d, C, reg, dup = case
    return "n%d-m%d-d%d-C%d-reg%g%s" % (n, m, d, C, reg, "-dup" if dup else "")


def inputs(case):
    """Seeded fp32 inputs of a case: features relu(randn), labels and g_pred randn -> (feat_syn, y_syn, feat_tar, g_pred)."""
    n, m, d, C, reg, dup = case
    seed = 1000003 * n + 10007 * m + 101 * d + C
    while True:          # (relu(randn) of a 1 x 1 matrix is zero every other seed: the first seed that gives a feature)
        g = torch.Generator().manual_seed(seed)
        fs = torch.relu(torch.randn(n, d, generator=g))
        if float(fs.max()) > 0:
            break
        seed += 1
    ys = torch.randn(n, C, generator=g)
    ft = torch.relu(torch.randn(m, d, generator=g))
    R = torch.randn(m, C, generator=g)
    if dup:
        fs[1], fs[5] = fs[0].clone(), fs[4].clone()
    return fs, ys, ft, R


def system(feat_syn, reg):
    """A = K + |reg| tr(K) / n I in fp64."""
    F = feat_syn.double()
    K = F @ F.t()
    n = K.shape[0]
    return K + (abs(float(reg)) * torch.trace(K) / n) * torch.eye(n, dtype=torch.float64)


def cond(feat_syn, reg) -> float:
    """cond_2(A), from the singular values in fp64."""
    s = torch.linalg.svdvals(system(feat_syn, reg))
    return float(s.max() / s.min())


def bar(c: float) -> float:
    return 16.0 * c * 2.0 ** -53


def by_autograd(feat_syn, y_syn, feat_tar, g_pred, reg):
    """(a): -> (pred, g_feat_syn, g_y_syn) in fp64; the gradient is that of sum(pred * g_pred)."""
    fs = feat_syn.double().clone().requires_grad_(True)
    ys = y_syn.double().clone().requires_grad_(True)
    ft = feat_tar.double()
    kss = torch.mm(fs, fs.t())
    kts = torch.mm(ft, fs.t())
    n = kss.shape[0]
    kss_reg = kss + abs(float(reg)) * torch.trace(kss) * torch.eye(n, dtype=torch.float64) / n
    pred = torch.mm(kts, torch.linalg.solve(kss_reg, ys))
    g_fs, g_ys = torch.autograd.grad(pred, (fs, ys), g_pred.double())
    return pred.detach(), g_fs, g_ys


def by_formulas(feat_syn, y_syn, feat_tar, g_pred, reg):
    """(b): the formulas of include/vd_nfr.h with a Cholesky factor, no autograd -> (pred, g_feat_syn, g_y_syn) in fp64."""
    Fs, Ys, Ft, R = feat_syn.double(), y_syn.double(), feat_tar.double(), g_pred.double()
    n = Fs.shape[0]
    K, Kt = Fs @ Fs.t(), Ft @ Fs.t()
    lam = abs(float(reg)) * torch.trace(K) / n
    L = torch.linalg.cholesky(K + lam * torch.eye(n, dtype=torch.float64))
    Z = torch.cholesky_solve(Ys, L)
    pred = Kt @ Z
    Q = torch.cholesky_solve(Kt.t() @ R, L)
    G = -Q @ Z.t()
    Gb = G + (abs(float(reg)) / n) * torch.trace(G) * torch.eye(n, dtype=torch.float64)
    g_fs = (Gb + Gb.t()) @ Fs + (Z @ R.t()) @ Ft
    return pred, g_fs, Q


def rel_l2(a, b) -> float:
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / b.norm())
