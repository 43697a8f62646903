"""The site-rate moves restated from their definitions (reference core/run.cpp:1105-1235) with exact_model's arithmetic: sums of
products of doubles are Fractions, log / lgamma / exp come from mpmath at 60 digits, and every quantity is an `Exact` with its
condition magnitude S and term count n, so that a float64 evaluation in any order lies within (n + 8) u S of it.

Rules for the terms, on top of exact_model's:
- lgamma(x) counts |lgamma x| + |x psi(x)| + 1: a relative error e of x is an absolute error |x psi(x)| e of lgamma(x);
- a product c log(y) counts |c| (|log y| + 1), y's own roundings (mu T + alpha: one product, one sum, all terms positive) being
  relative errors of y and so absolute errors of log y of the same size;
- a difference of two separately formed sums (sum of the new rates minus sum of the old ones) counts both sums.

Nothing here calls the engine.  Inputs may be float64 values or Fractions (exact statistics of exact_model.stats).
"""
from __future__ import annotations

from fractions import Fraction as F

import mpmath

from exact_model import _DPS, _ZERO, Exact, _frac, _log, _mp

NU_FLOOR = 1e-50
SCALE_LO, SCALE_HI = 0.9, 1.0 / 0.9


def _F(x) -> F:
    return x if isinstance(x, F) else F(float(x))


def _lgamma(x):
    """(lgamma(x), its S) for x > 0."""
    with mpmath.workdps(_DPS):
        m = _mp(x)
        v = _frac(mpmath.loggamma(m))
        s = _frac(abs(m * mpmath.digamma(m)))
    return v, abs(v) + s + 1


def log_p_alpha(alpha, mu_l, Ttwiddle_l, num_muts_l) -> Exact:
    """calc_log_p_alpha (run.cpp:1157-1181): sum over sites of [M_l > 0] lgamma(M_l + alpha) - (M_l + alpha) log(mu_l Ttwiddle_l + alpha),
    minus n_plus lgamma(alpha), plus L alpha log(alpha); n_plus = sites with mutations."""
    a = _F(alpha)
    L = len(num_muts_l)
    v, S, n_plus = _ZERO, _ZERO, 0
    lg_cache, log_cache = {}, {}
    for l in range(L):
        M = int(num_muts_l[l])
        if M > 0:
            n_plus += 1
            if M not in lg_cache:
                lg_cache[M] = _lgamma(M + a)
            lg, lgS = lg_cache[M]
            v += lg; S += lgS
        y = _F(mu_l[l]) * _F(Ttwiddle_l[l]) + a
        if y not in log_cache:
            log_cache[y] = _log(y)
        ly = log_cache[y]
        v -= (M + a) * ly
        S += (M + a) * (abs(ly) + 1)
    lg, lgS = _lgamma(a)
    la = _log(a)
    v += -n_plus * lg + L * a * la
    S += n_plus * lgS + L * a * (abs(la) + 1)
    return Exact(v, S, 2 * L + 6)


def log_metropolis(old_alpha, new_alpha, log_p_old, log_p_new) -> Exact:
    """run.cpp:1203-1209 with mean_alpha = 1: -(new - old) + (log p(new) - log p(old)) + log(old / new), from the numbers given."""
    o, nw, po, pn = _F(old_alpha), _F(new_alpha), _F(log_p_old), _F(log_p_new)
    lr = _log(o / nw)
    return Exact(-(nw - o) + pn - po + lr, abs(nw - o) + abs(pn) + abs(po) + abs(lr) + 1, 4)


def accepts(log_mh: float, u: float) -> bool:
    """run.cpp:1210, from the float64 log_metropolis the engine reports and its uniform."""
    import math
    return log_mh > 0.0 or u < math.exp(log_mh)


def delta_log_G(mu_l, Ttwiddle_l, num_muts_l, nu_old, nu_new) -> Exact:
    """run.cpp:1144 over the sites: -mu_l (new - old) Ttwiddle_l + M_l log(new / old)."""
    v, S = _ZERO, _ZERO
    L = len(num_muts_l)
    for l in range(L):
        o, nw, M = _F(nu_old[l]), _F(nu_new[l]), int(num_muts_l[l])
        t = _F(mu_l[l]) * (nw - o) * _F(Ttwiddle_l[l])
        v -= t; S += abs(t)
        if M:
            lr = _log(nw / o)
            v += M * lr; S += M * (abs(lr) + 1)
    return Exact(v, S, 2 * L)


def delta_log_prior_nu(alpha, nu_old, nu_new) -> Exact:
    """run.cpp:1148 over the sites, then :1151: sum of (alpha - 1) log(new / old), minus alpha (sum new - sum old)."""
    a = _F(alpha)
    v, S, so, sn = _ZERO, _ZERO, _ZERO, _ZERO
    for o, nw in zip(nu_old, nu_new):
        o, nw = _F(o), _F(nw)
        lr = _log(nw / o)
        v += (a - 1) * lr; S += abs(a - 1) * (abs(lr) + 1)
        so += o; sn += nw
    v -= a * (sn - so)
    S += a * (sn + so)
    return Exact(v, S, 3 * len(nu_old) + 2)


def delta_log_prior_alpha(alpha_before, alpha_after, nu_old) -> Exact:
    """run.cpp:1226-1231 with mean_alpha = 1, from the rates as they were before the draw."""
    a0, a1 = _F(alpha_before), _F(alpha_after)
    L = len(nu_old)
    s_nu, s_log, s_log_S = _ZERO, _ZERO, _ZERO
    for x in nu_old:
        x = _F(x)
        lx = _log(x)
        s_nu += x; s_log += lx; s_log_S += abs(lx) + 1
    l0, l1 = _log(a0), _log(a1)
    (g0, g0S), (g1, g1S) = _lgamma(a0), _lgamma(a1)
    d = a1 - a0
    v = -d + L * (a1 * l1 - a0 * l0) - L * (g1 - g0) + d * s_log - d * s_nu
    S = abs(d) + L * (a1 * (abs(l1) + 1) + a0 * (abs(l0) + 1)) + L * (g1S + g0S) + abs(d) * (s_log_S + s_nu)
    return Exact(v, S, 2 * L + 10)


def alpha_posterior_quadrature(mu_l, Ttwiddle_l, num_muts_l, splits, want_mean=True):
    """(normaliser, mean) of the alpha steps' target exp(log p(alpha) - alpha) (exponential prior of mean 1), by mpmath quadrature over
    the pieces `splits` cuts (0, inf) into; the density is taken relative to its value at alpha = 1 so that it stays in range."""
    ref = log_p_alpha(1.0, mu_l, Ttwiddle_l, num_muts_l).value - 1
    counts, L = {}, len(num_muts_l)
    for l in range(L):
        k = (int(num_muts_l[l]), _F(mu_l[l]) * _F(Ttwiddle_l[l]))
        counts[k] = counts.get(k, 0) + 1
    n_plus = sum(c for (M, _), c in counts.items() if M > 0)
    with mpmath.workdps(30):
        terms = [(M, _mp(b), c) for (M, b), c in counts.items()]
        ref_m = _mp(ref)

        def dens(a):
            s = -n_plus * mpmath.loggamma(a) + L * a * mpmath.log(a) - a
            for M, b, c in terms:
                if M > 0:
                    s += c * mpmath.loggamma(M + a)
                s -= c * (M + a) * mpmath.log(b + a)
            return mpmath.exp(s - ref_m)

        Z = mpmath.quad(dens, splits)
        if not want_mean:
            return Z, None
        m = mpmath.quad(lambda a: a * dens(a), splits)
        return Z, m / Z
