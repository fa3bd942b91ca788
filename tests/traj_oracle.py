"""Numpy restatements of the flat-parameter chain of include/vd_hip.h (``vdt_``; TEST INFRASTRUCTURE ONLY): the elementwise parts in
float32 with every operation rounded on its own -- what the kernels promise bit for bit --, the sums with ``math.fsum`` over the
fp64 terms the kernels form (fp64 difference then fp64 square; the fp64 product of two float32 values, which is exact)."""
import math

import numpy as np

F = np.float32


def traj_step(theta, g, lr):
    theta, g = np.asarray(theta, F), np.asarray(g, F)
    return (theta - (F(lr) * g).astype(F)).astype(F)


def traj_dists(theta, theta0, target):
    """-> (dist, dist0): fsum of the fp64 squares of the fp64 differences."""
    t = np.asarray(target, np.float64)
    d1 = np.asarray(theta, np.float64) - t
    d0 = np.asarray(theta0, np.float64) - t
    return math.fsum((d1 * d1).tolist()), math.fsum((d0 * d0).tolist())


def traj_tbar(theta, target, dist0):
    """(2.0f * (theta - target)) / (float)dist0 in float32; ``dist0`` is the double the kernel (or ``traj_dists``) produced."""
    theta, target = np.asarray(theta, F), np.asarray(target, F)
    diff = (theta - target).astype(F)
    return ((F(2.0) * diff).astype(F) / F(np.float64(dist0))).astype(F)


def traj_adjoint(tbar, hv, g, lr, share):
    """-> (tbar after ``+= hv`` (None: unchanged), the fsum of (double)tbar * (double)g, the absolute sum of those terms,
    v = (-(lr * share)) * tbar)."""
    tbar, g = np.asarray(tbar, F), np.asarray(g, F)
    t = tbar.copy() if hv is None else (tbar + np.asarray(hv, F)).astype(F)
    terms = t.astype(np.float64) * g.astype(np.float64)
    c = F(-(F(lr) * F(share)))
    return t, math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist()), (c * t).astype(F)
