"""Restatements for the FRePo tests: the Adam formula of include/vd_frepo.h in numpy float32 (every operation rounded on its
own, in the header's order), the same step in fp64 from the same float32 state, the derived bound between the two, and the
mean-squared error in fp64.  Nothing here imports the package under test."""
import numpy as np

F = np.float32
U = 2.0 ** -24          # unit roundoff of float32
TINY = 2.0 ** -149          # the smallest float32 subnormal: what a rounding may lose in absolute terms when a result underflows
# Roundings of the header's formula, as written, on the path to the quotient u = (step_size * m) / (sqrt(v) / bc2_sqrt + eps):
#   m = m + one_minus_beta1 * (g - m)                 3   (difference, product, sum)
#   v = beta2 * v + one_minus_beta2 * (g * g)         4   (product, square, product, sum)
#   u                                                  5   (square root, quotient, sum, product, quotient)
R_M, R_V, R_U = 3, 4, 5
R = R_M + R_V + R_U


def constants(lr, beta1, beta2, eps, step, weight_decay=0.0):
    """The float32 constants of one launch, computed as the host computes them: in double, each rounded to float once."""
    return dict(beta1=F(beta1), one_minus_beta1=F(1.0 - beta1), beta2=F(beta2), one_minus_beta2=F(1.0 - beta2),
                bc2_sqrt=F((1.0 - beta2 ** step) ** 0.5), eps=F(eps), step_size=F(lr / (1.0 - beta1 ** step)), lr_wd=F(lr * weight_decay))


def adam_f32(p, m, v, g, c):
    """include/vd_frepo.h, line by line, on float32 arrays -> (p, m, v)."""
    p, m, v, g = (np.asarray(a, dtype=F) for a in (p, m, v, g))
    with np.errstate(under="ignore"):
        if c["lr_wd"] != 0:
            p = (p * F(F(1.0) - c["lr_wd"])).astype(F)
        dm = (g - m).astype(F)
        tm = (c["one_minus_beta1"] * dm).astype(F)
        mn = (m + tm).astype(F)
        av = (c["beta2"] * v).astype(F)
        gg = (g * g).astype(F)
        bv = (c["one_minus_beta2"] * gg).astype(F)
        vn = (av + bv).astype(F)
        s = np.sqrt(vn).astype(F)
        q = (s / c["bc2_sqrt"]).astype(F)
        den = (q + c["eps"]).astype(F)
        num = (c["step_size"] * mn).astype(F)
        u = (num / den).astype(F)
        return (p - u).astype(F), mn, vn


def adam_f64(p, m, v, g, c):
    """The same step in fp64 from the same float32 state and the same float32 constants -> (p, m, v, u, denom, decayed p)."""
    p, m, v, g = (np.asarray(a, dtype=F).astype(np.float64) for a in (p, m, v, g))
    k = {name: float(val) for name, val in c.items()}
    pw = p * (1.0 - k["lr_wd"]) if k["lr_wd"] != 0 else p
    mn = m + k["one_minus_beta1"] * (g - m)
    vn = k["beta2"] * v + k["one_minus_beta2"] * (g * g)
    den = np.sqrt(vn) / k["bc2_sqrt"] + k["eps"]
    u = k["step_size"] * mn / den
    return pw - u, mn, vn, u, den, pw


def bounds(p, m, v, g, c):
    """(bound on |p32 - p64|, on |m32 - m64|, on |v32 - v64|) for one step from the float32 state (p, m, v, g).

    m: three roundings, each relative to a term no larger than M = |m| + (1-b1)|g - m|: 3 U M.
    v: four roundings of non-negative terms: 4 U v64, plus TINY where g * g leaves the normal range (|g| = 1e-20: the square
       is a float32 subnormal or zero, and what is lost there is absolute, at most one subnormal spacing after the sum).
    p: the final subtraction rounds once, U |p64|; with AdamW's decay the factor 1 - lr_wd and the product round too, 2 U |p|
       more; the quotient u carries the R roundings on its path (R_M of them relative to M, not to |m64|, hence M in the bound;
       the R_V of v are halved by the square root, which only loosens the bound) and 2 more for the terms of second order:
       (R + 2) U step_size M / denom64."""
    p64, m64, v64, u, den, pw = adam_f64(p, m, v, g, c)
    m_, g_ = np.asarray(m, dtype=F).astype(np.float64), np.asarray(g, dtype=F).astype(np.float64)
    M = np.abs(m_) + float(c["one_minus_beta1"]) * np.abs(g_ - m_)
    decay = 2 if c["lr_wd"] != 0 else 0
    step = float(c["step_size"])
    bp = U * np.abs(p64) + decay * U * np.abs(pw) + (R + 2) * U * step * M / den
    bm = R_M * U * M
    bv = R_V * U * v64 + TINY
    return bp, bm, bv


T_VALUES = (1, 2, 10, 1000)


def state(n, t, seed, g_kind="randn"):
    """A float32 state (p, m, v, g) of ``n`` elements as it may stand before step ``t``: at t = 1 both moments are zero."""
    rng = np.random.default_rng([seed, t, n])
    p = rng.standard_normal(n).astype(F)
    g = {"randn": lambda: rng.standard_normal(n) * 0.1, "zero": lambda: np.zeros(n), "tiny": lambda: np.where(rng.random(n) < 0.5, 1e-20, -1e-20)}[g_kind]().astype(F)
    if t == 1:
        return p, np.zeros(n, F), np.zeros(n, F), g
    m = (rng.standard_normal(n) * 0.05).astype(F)
    v = (rng.random(n) * 0.01 + 1e-6).astype(F)
    return p, m, v, g


def mse_f64(logits, targets):
    """(loss, dlogits) of nn.MSELoss() in fp64 from float32 inputs."""
    l, y = np.asarray(logits, dtype=F).astype(np.float64), np.asarray(targets, dtype=F).astype(np.float64)
    d = l - y
    return float((d * d).sum() / d.size), 2.0 * d / d.size
