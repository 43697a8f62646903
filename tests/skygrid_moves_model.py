"""The Skygrid population moves restated on exact_model's arithmetic: the gradient of the curve, the whole-tree statistics the moves
read, and every number a round of the three moves reports (reference core/run.cpp:1321-1358, 1360-2014, 2016-2189;
core/pop_model.cpp:206-245, 333-523; core/scalable_coalescent.cpp:163-187).  A third party for the HIP kernels
(csrc/emat_skygrid_kernels.hpp): Fractions, mpmath at 60 digits, and every quantity an `Exact` with its condition magnitude S and term
count n (exact_model's docstring), so that a float64 evaluation of the reference's formula in any order lies within (n + 8) u S.

The gradient here is the EXACT derivative of log(integral of N), not the reference's series: where a log-linear piece has
|Delta| < 1e-5 the reference replaces expm1(Delta) / Delta by 1 + Delta / 2 and J(Delta) by 1/2 + Delta / 3 (pop_model.cpp:491-494),
which truncates the piece's integral by at most Delta^2 / 6 and its J by at most Delta^2 / 4 relative: 3e-11 of the piece's
magnitude at the branch's edge.  `d_log_int_N_d_gamma` returns that allowance next to the Exact; it is zero for every other piece.

Nothing here draws random numbers or runs a trajectory: the moves' draws and states are INPUTS (the device's own, taken from its result and
trace), and each function restates one line of the reference from the state before it.
"""
from __future__ import annotations

import math
from fractions import Fraction as F

import mpmath

import exact_model as X
from exact_model import Exact, _exp, _expm1, _fl, _frac, _log, _mp

SERIES_EDGE = 1e-5              # pop_model.cpp:491
SERIES_TRUNCATION = 3e-11       # max(Delta^2 / 6, Delta^2 / 4) at |Delta| = 1e-5, rounded up


def _fr(v) -> F:
    """A float64 (or numpy scalar) or a Fraction, as a Fraction."""
    return v if isinstance(v, F) else _fl(v)


_Q = 1 << 260


def _rd(v: F) -> F:
    """v rounded to a multiple of 2^-260 (far below anything a check here resolves): a quotient's denominator would otherwise grow with
    every term a sum takes in, and a thousand cells would cost seconds."""
    return F((v.numerator * _Q) // v.denominator, _Q)


def _J(D: F) -> F:
    """J(D) = (D e^D - (e^D - 1)) / D^2 (pop_model.cpp:440), 1/2 at 0; a series below 1e-20, where 60 digits no longer carry the difference."""
    if abs(D) < F(1, 10 ** 20):
        return F(1, 2) + D / 3 + D * D / 8
    return (D * _exp(D) - _expm1(D)) / (D * D)


def d_log_N_d_gamma(pop: X.Pop, t, k: int) -> F:
    """pop_model.cpp:206-225, exactly (a 0, a 1 or a ratio of differences of times)."""
    t = t if isinstance(t, F) else _fl(t)
    kk, M = pop._sky_interval(t), len(pop.x) - 1
    if kk == 0:
        return F(int(k == 0))
    if kk > M:
        return F(int(k == M))
    if not pop.log_linear:
        return F(int(k == kk))
    c = (t - pop.x[kk - 1]) / (pop.x[kk] - pop.x[kk - 1])
    return 1 - c if k == kk - 1 else c if k == kk else F(0)


def support_of_d_log_N_d_gamma(pop: X.Pop, k: int):
    """pop_model.cpp:227-245: (lo, hi) as floats, -inf / +inf at the ends."""
    M = len(pop.x) - 1
    lo = -math.inf if k == 0 else float(pop.x[k - 1])
    hi = math.inf if k == M else float(pop.x[k] if not pop.log_linear else pop.x[k + 1])
    return lo, hi


def _pieces(pop: X.Pop, a: F, b: F):
    """The pieces of [a, b], one per knot interval it meets, with what every knot's derivative shares: (I, S_I, allow_I, {k: record},
    number of pieces).  Kept with `pop` (a Pop is one set of gammas): the force asks for the same cell once per knot."""
    cache = pop.__dict__.setdefault("_pieces_cache", {})
    if (a, b) in cache:
        return cache[(a, b)]
    x, gm, M = pop.x, pop.gamma, len(pop.x) - 1
    ka, kb = pop._sky_interval(a), pop._sky_interval(b)
    bias = max(gm[max(ka - 1, 0): min(kb, M) + 1])
    I, S_I, allow_I, recs = F(0), F(0), F(0), {}
    for k in range(ka, kb + 1):
        lo = max(a, x[k - 1]) if k > 0 else a
        hi = min(b, x[k]) if k <= M else b
        if hi <= lo:
            continue
        if k == 0 or k == M + 1 or not pop.log_linear:
            kg = 0 if k == 0 else M if k == M + 1 else k
            v = _exp(gm[kg]) * (hi - lo)
            cond = 2 + abs(gm[kg]) + abs(bias)
            I += v; S_I += v * cond
            recs[k] = ("flat", kg, v, cond)
            continue
        w = x[k] - x[k - 1]
        c_lo, c_hi = (lo - x[k - 1]) / w, (hi - x[k - 1]) / w
        G_lo = (1 - c_lo) * gm[k - 1] + c_lo * gm[k]
        G_hi = (1 - c_hi) * gm[k - 1] + c_hi * gm[k]
        D = G_hi - G_lo
        series = abs(D) < F(SERIES_EDGE)
        v = _exp(G_lo) * (hi - lo) * (_expm1(D) / D if D != 0 else 1)
        cond = 4 + 3 * (abs(gm[k - 1]) + abs(gm[k])) + abs(D) + abs(bias)
        I += v; S_I += v * cond
        if series:
            allow_I += v
        recs[k] = ("linear", hi - lo, c_lo, c_hi, G_lo, G_hi, D, series, cond)
    cache[(a, b)] = (I, S_I, allow_I, recs, kb - ka + 1)
    return cache[(a, b)]


def d_log_int_N_d_gamma(pop: X.Pop, a, b, kp: int):
    """(d log(integral of N over [a, b]) / d gamma_kp as an Exact, the allowance for the reference's series branch).  a < b.
    S: each piece's share of the derivative and of the integral with the condition of the exponentials it is made of (exact_model's
    _sky_integral rule), J counted by the two terms the reference subtracts, (|D e^D| + |expm1 D|) / D^2, which is what its float64
    form loses just above the series' edge."""
    a, b = (v if isinstance(v, F) else _fl(v) for v in (a, b))
    assert a < b
    M = len(pop.x) - 1
    I, S_I, allow_I, recs, npieces = _pieces(pop, a, b)
    dI, S_dI, allow_dI = F(0), F(0), F(0)
    touching = {kp, kp + 1} | ({0} if kp == 0 else set()) | ({M + 1} if kp == M else set())
    for k in sorted(touching & set(recs)):
        rec = recs[k]
        if rec[0] == "flat":
            _, kg, v, cond = rec
            if kp == kg:
                dI += v; S_dI += v * cond
            continue
        _, width, c_lo, c_hi, G_lo, G_hi, D, series, cond = rec
        if kp != k and kp != k - 1:
            continue
        Jp, Jm = _J(D), _J(-D)
        if series:
            SJp = SJm = F(1)
        else:
            SJp = (abs(D * _exp(D)) + abs(_expm1(D))) / (D * D)
            SJm = (abs(D * _exp(-D)) + abs(_expm1(-D))) / (D * D)
        w_hi, w_lo = (c_hi, c_lo) if kp == k else (1 - c_hi, 1 - c_lo)
        t1 = width * w_hi * _exp(G_lo) * Jp
        t2 = width * w_lo * _exp(G_hi) * Jm
        dI += t1 + t2
        # the weights of knot k - 1 are formed as 1 - c: each counts the 1 and the c it subtracts (a cell that ends just short of x_k has
        # 1 - c_lo of 1e-10 carrying the rounding of a number of size 1)
        m_hi, m_lo = (c_hi, c_lo) if kp == k else (1 + c_hi, 1 + c_lo)
        S_dI += width * (m_hi * _exp(G_lo) * SJp + m_lo * _exp(G_hi) * SJm) * cond
        if series:
            allow_dI += t1 + t2
    r = _rd(dI / I)
    S = float(S_dI / I) + float(r) * float(S_I / I)
    allowance = float(SERIES_TRUNCATION * (allow_dI / I + r * allow_I / I))
    return Exact(r, S, 4 * npieces + 8), allowance


# ---- the statistics the moves read ------------------------------------------------------------------------------------------
class NodeStats:
    """c_k (run.cpp:1695-1702, ints) and W_k = sum_i d log N(t_i) / d gamma_k (Fractions), both exact, of the inner nodes' times.
    W_S[k]: the S of W_k -- every node in knot k's support adds a term formed from 1 and a ratio of time differences, so it counts 3
    whatever the term's own size; W_n[k]: how many nodes that is."""

    def __init__(self, pop: X.Pop, inner_t):
        M = len(pop.x) - 1
        self.num_inner = len(inner_t)
        self.c = [0] * (M + 1); self.W = [F(0)] * (M + 1); self.W_n = [0] * (M + 1)
        for t in inner_t:
            t = _fl(t)
            kk = pop._sky_interval(t)
            self.c[min(kk, M)] += 1
            ks = (0,) if kk == 0 else (M,) if kk > M else (kk,) if not pop.log_linear else (kk - 1, kk)
            for k in ks:
                self.W[k] += d_log_N_d_gamma(pop, t, k)
                self.W_n[k] += 1
        self.W_S = [F(3 * n) for n in self.W_n]

    def W_exact(self, k) -> Exact:
        return Exact(self.W[k], self.W_S[k], self.W_n[k] + 2)


def sum_log_N_node_by_node(pop: X.Pop, inner_t) -> F:
    return sum((pop.log_N(_fl(t))[0] for t in inner_t), F(0))


class Grid:
    """The whole-tree lineage grid as the moves are given it: cell c = [t_ref + (first_cell + c) t_step, ... + t_step)."""

    def __init__(self, t_ref, t_step, first_cell, k_bar):
        self.t_ref, self.t_step, self.first_cell = _fl(t_ref), _fl(t_step), int(first_cell)
        self.k_bar = [_fl(v) for v in k_bar]

    def bounds(self, c):
        lo = self.t_ref + (self.first_cell + c) * self.t_step
        return lo, lo + self.t_step

    def bound_mag(self, c):
        return abs(self.t_ref) + abs((self.first_cell + c + 1) * self.t_step)

    def popsize_bar(self, pop: X.Pop, c):
        """(the cell's average N as a Fraction, its S): pop_integral / t_step with the cell bounds' own rounding (exact_model.scalable_log_prior's rule)."""
        cache = pop.__dict__.setdefault("_popsize_bar_cache", {})
        key = (self.t_ref, self.t_step, self.first_cell, c)
        if key not in cache:
            lo, hi = self.bounds(c)
            I = pop.pop_integral(lo, hi)
            Nmax = max(pop.pop_at_time(lo).value, pop.pop_at_time(hi).value)
            cache[key] = (_rd(I.value / self.t_step), _rd((I.S + Nmax * 2 * self.bound_mag(c)) / self.t_step), I.n)
        return cache[key]


def log_coalescent_prior(pop: X.Pop, grid: Grid, ns: NodeStats) -> Exact:
    """calc_log_prior (scalable_coalescent.cpp:163-187): -sum_c t_step k (k - 1) / (2 Nbar_c) - sum_k W_k gamma_k.  W_k is itself a sum of up to
    num_inner positive terms, so it adds num_inner to n and nothing but its own size to S."""
    v, S, nmax = F(0), F(0), 0
    for c, k in enumerate(grid.k_bar):
        if k == 0 or k == 1:
            continue
        N, NS, n = grid.popsize_bar(pop, c)
        term = _rd(grid.t_step * k * (k - 1) / (2 * N))
        v -= term
        S += float(abs(term)) * (3 + float(NS / N))
        nmax = max(nmax, n)
    for Wk, WS, g in zip(ns.W, ns.W_S, pop.gamma):
        v -= Wk * g
        S += abs(g) * (WS + Wk)
    return Exact(v, S, 4 * len(grid.k_bar) + 2 * len(ns.W) + nmax + max(ns.W_n))


def zero_mode_B(pop: X.Pop, grid: Grid) -> Exact:
    """run.cpp:2100-2112: sum_c (1/2) t_step k (k - 1) / Nbar_c, divided by I_bar = exp(-gamma_bar)."""
    M1 = len(pop.gamma)
    gamma_bar = sum(pop.gamma, F(0)) / M1
    gS = sum((abs(g) for g in pop.gamma), F(0)) / M1
    v, S, nmax = F(0), F(0), 0
    for c, k in enumerate(grid.k_bar):
        if k == 0 or k == 1:
            continue
        N, NS, n = grid.popsize_bar(pop, c)
        term = _rd(grid.t_step * k * (k - 1) / (2 * N))
        v += term
        S += float(abs(term)) * (3 + float(NS / N))
        nmax = max(nmax, n)
    e = _exp(gamma_bar)
    return Exact(v * e, (S + abs(v) * (2 + gS * (M1 + 2))) * e, 4 * len(grid.k_bar) + M1 + nmax + 16)


def tau_posterior(gamma, alpha, beta):
    """run.cpp:1337-1344: (post_alpha, post_beta) as Exacts."""
    g = [_fr(v) for v in gamma]; M = len(g) - 1
    ssq = sum(((g[k] - g[k - 1]) ** 2 for k in range(1, M + 1)), F(0))
    pa = _fl(alpha) + F(M, 2); pb = _fl(beta) + ssq / 2
    return Exact(pa, abs(_fl(alpha)) + F(M, 2), 2), Exact(pb, abs(_fl(beta)) + 2 * ssq, 3 * M + 4)


def tau_delta_log_prior(post_alpha, post_beta, new_tau, old_tau) -> Exact:
    """run.cpp:1355-1357 from the float64 post_alpha, post_beta and taus the caller holds."""
    pa, pb, nt, ot = (_fl(v) for v in (post_alpha, post_beta, new_tau, old_tau))
    lg = _log(nt / ot)
    v = (pa - 1) * lg - pb * (nt - ot)
    return Exact(v, (abs(pa) + 1) * (abs(lg) + 1) * 2 + abs(pb) * (abs(nt) + abs(ot)) * 2, 8)


def _barrier(g, spec) -> tuple:
    """(sum over knots below the barrier of ((loc - gamma) / scale)^2, its S, its term count)."""
    if not spec.low_gamma_barrier_enabled:
        return F(0), F(0), 0
    loc, sc = _fl(spec.low_gamma_barrier_loc), _fl(spec.low_gamma_barrier_scale)
    v, S, n = F(0), F(0), 0
    for gk in g:
        if gk < loc:
            e = (loc - gk) / sc
            v += e * e; n += 1
            S += 2 * e * (abs(loc) + abs(gk)) / sc + 3 * e * e
    return v, S, n


def U_prior(gamma, tau, spec) -> Exact:
    """calc_U_prior_from_gamma_k_s (run.cpp:1723-1753)."""
    g = [_fr(v) for v in gamma]; M1 = len(g); tau = _fr(tau)
    ssq = sum(((g[k] - g[k - 1]) ** 2 for k in range(1, M1)), F(0))
    S_ssq = sum((2 * abs(g[k] - g[k - 1]) * (abs(g[k]) + abs(g[k - 1])) + 2 * (g[k] - g[k - 1]) ** 2 for k in range(1, M1)), F(0))
    bv, bS, bn = _barrier(g, spec)
    a, b = _fl(spec.inv_nbar_prior_alpha), _fl(spec.inv_nbar_prior_beta)
    gamma_bar = sum(g, F(0)) / M1
    gS = sum((abs(v) for v in g), F(0)) / M1
    e = _exp(-gamma_bar)
    v = tau * ssq / 2 + bv + a * gamma_bar + b * e
    S = tau * (S_ssq + 2 * ssq) / 2 + bS + abs(a) * gS * 2 + abs(b) * e * (2 + gS * (M1 + 2))
    return Exact(v, S, 5 * M1 + bn + 16)


def log_prior_bound(gamma, spec) -> Exact:
    """run.cpp:2132-2143: minus the barrier's sum."""
    v, S, n = _barrier([_fr(x) for x in gamma], spec)
    return Exact(-v, S, n + 2)


def kinetic(p, m) -> Exact:
    """calc_K (run.cpp:1716-1722) with inv_m = 1 / m rounded first."""
    v = sum((_fl(pk) ** 2 / (2 * _fl(mk)) for pk, mk in zip(p, m)), F(0))
    return Exact(v, 4 * v, len(p) + 4)


def masses(c, tau):
    """run.cpp:1708, as Exacts."""
    M = len(c) - 1; tau = _fl(tau)
    return [Exact((tau if k > 0 else 0) + (tau if k < M else 0) + c[k], 2 * tau + c[k], 3) for k in range(M + 1)]


def force(pop: X.Pop, grid: Grid, ns: NodeStats, tau, spec, knots=None):
    """calc_f_k_s_from_gamma_k_s (run.cpp:1775-1843) at pop's gammas: [(Exact f_k, allowance)] for `knots` (all when None) -- the exact derivative -dU/dgamma_k.
    The cells of a knot are those that meet its support, as the reference picks them (:1785-1789)."""
    g, M = pop.gamma, len(pop.gamma) - 1
    tau = _fl(tau)
    C = len(grid.k_bar)
    t_min_coal, t_max_coal = grid.bounds(0)[0], grid.bounds(C - 1)[1]
    cell_of = lambda t: min(max(X._floor((_fl(t) - grid.t_ref) / grid.t_step) - grid.first_cell, 0), C - 1)
    a, b = _fl(spec.inv_nbar_prior_alpha), _fl(spec.inv_nbar_prior_beta)
    gamma_bar = sum(g, F(0)) / (M + 1)
    gS = sum((abs(v) for v in g), F(0)) / (M + 1)
    e = _exp(-gamma_bar)
    f_inv = (-a + b * e) / (M + 1)
    S_inv = (abs(a) + abs(b) * e * (2 + gS * (M + 3))) / (M + 1)
    cache = {}
    out = []
    for k in (range(M + 1) if knots is None else knots):
        lo, hi = support_of_d_log_N_d_gamma(pop, k)
        c_min = 0 if lo < t_min_coal else cell_of(lo)
        c_max = C - 1 if hi > t_max_coal else cell_of(hi)
        v, S, allow, n = F(0), F(0), 0.0, 0
        for c in range(c_min, c_max + 1):
            kc = grid.k_bar[c]
            if kc == 0 or kc == 1:
                continue
            if c not in cache:
                cache[c] = grid.popsize_bar(pop, c)
            N, NS, nN = cache[c]
            ca, cb = grid.bounds(c)
            d, al = d_log_int_N_d_gamma(pop, ca, cb, k)
            coef = _rd(grid.t_step * kc * (kc - 1) / (2 * N))
            # the gradient is taken at the cell's computed bounds: their rounding moves it by at most its own size times the bounds' relative
            # error over the cell's width, which the cell average's S already carries (NS / N)
            v += _rd(coef * d.value)
            S += float(abs(coef)) * (float(d.S) + float(d.value) * (4 + float(NS / N)))
            allow += float(abs(coef)) * al
            n = max(n, d.n + nN)
        v -= ns.W[k]; S += ns.W_S[k]
        if k > 0:
            v -= tau * (g[k] - g[k - 1]); S += tau * (abs(g[k]) + abs(g[k - 1])) * 2
        if k < M:
            v -= tau * (g[k] - g[k + 1]); S += tau * (abs(g[k]) + abs(g[k + 1])) * 2
        if spec.low_gamma_barrier_enabled and g[k] < _fl(spec.low_gamma_barrier_loc):
            loc, sc = _fl(spec.low_gamma_barrier_loc), _fl(spec.low_gamma_barrier_scale)
            v += 2 * (loc - g[k]) / (sc * sc); S += 2 * (abs(loc) + abs(g[k])) * 3 / (sc * sc)
        v += f_inv; S += S_inv
        out.append((Exact(v, S, (c_max - c_min + 1) + n + (M + 1) + ns.W_n[k] + 16), allow))
    return out


def U_total(pop: X.Pop, grid: Grid, ns: NodeStats, tau, spec) -> F:
    """U_coal + U_prior exactly (for the model's own central-difference check of `force`)."""
    return -log_coalescent_prior(pop, grid, ns).value + U_prior(pop.gamma, tau, spec).value


def half_step(gamma_k, dt, p_k, m_k) -> Exact:
    """gamma_k + 0.5 dt p_k inv_m_k (run.cpp:1893-1895, :1950-1952), from float64 inputs."""
    g, dt, p, m = (_fl(v) for v in (gamma_k, dt, p_k, m_k))
    d = dt * p / (2 * m)
    return Exact(g + d, abs(g) + 5 * abs(d), 2)


def momentum_step(p_k, dt, f_k) -> Exact:
    """p_k + dt f_k (run.cpp:1931-1933), from float64 inputs."""
    p, dt, f = (_fl(v) for v in (p_k, dt, f_k))
    return Exact(p + dt * f, abs(p) + 2 * abs(dt * f), 2)


def with_gamma(pm, gamma):
    """A PopModel like pm with other gammas."""
    from delphy_amd.engine import PopModel
    return PopModel.skygrid(pm.skygrid_x, gamma, pm.skygrid_type == 2)


# ---- inputs shared by the model's own checks and the device's ------------------------------------------------------------------
def pop_with_gammas(pop: X.Pop, gamma) -> X.Pop:
    """A copy of `pop` with other gammas (Fractions or floats)."""
    import copy
    q = copy.copy(pop)
    q.gamma = [g if isinstance(g, F) else _fl(g) for g in gamma]
    q.popsize_bar_cache = {}
    q.__dict__.pop("_pieces_cache", None); q.__dict__.pop("_popsize_bar_cache", None)
    return q


def adversarial_gammas(n: int, barrier_loc: float):
    """n gammas around 2 with, where there is room, adjacent pairs equal, 1e-12 apart, 0.9e-5 and 1.1e-5 apart (either side of the series
    branch) and one value below the barrier."""
    import numpy as np
    g = 2.0 + 0.8 * np.sin(0.7 * np.arange(n)) + 0.05 * np.cos(3.1 * np.arange(n))
    if n >= 3:
        g[2] = g[1] + 0.9e-5
    if n >= 12:
        g[4] = g[3]; g[6] = g[5] + 1e-12; g[8] = g[7] + 1.1e-5; g[10] = g[9] - 1.1e-5
        g[11] = barrier_loc - 0.37
    elif n >= 2:
        g[0] = barrier_loc - 0.37
    return g


def make_case(name, num_knots, num_cells, num_inner, log_linear, layout="finer", seed=1, **spec_kw):
    """One input of emat_skygrid_moves: (name, PopModel, SkygridSpec, t_ref, t_step, first_cell, k_bar, inner_t).  The grid is
    [-num_cells t_step, 0) with t_step = 1/4 (cell bounds are exact doubles).  layout: where the knots lie --
    'finer' / 'coarser': evenly over the middle 90 % of the grid (which it is follows from the counts); 'before': the whole grid before
    x_0; 'after': the whole grid after x_M; 'on': knots exactly on cell bounds and inner times exactly on knots and on cell bounds."""
    import numpy as np
    from delphy_amd.engine import PopModel, SkygridSpec
    rng = np.random.default_rng(seed)
    t_step, t_ref, first_cell = 0.25, 0.0, -num_cells
    span = num_cells * t_step
    if layout == "before":
        x = 1.0 + np.arange(num_knots) * 0.5
    elif layout == "after":
        x = -span - 3.0 - np.arange(num_knots)[::-1] * 0.5
    elif layout == "on":
        x = -span + t_step * np.round(np.linspace(0, num_cells, num_knots + 2)[1:-1])
        assert np.all(np.diff(x) > 0)
    else:
        x = np.linspace(-0.95 * span, -0.05 * span, num_knots)
    inner_t = -rng.uniform(0.0, span, num_inner) * (1 - 1e-9) - 1e-12
    if layout == "on":
        m = min(num_inner, num_knots)
        inner_t[:m] = x[:m]
        inner_t[m:] = -t_step * rng.integers(1, num_cells + 1, num_inner - m)
    k_bar = 1.0 + 6.0 * rng.uniform(size=num_cells) * np.linspace(0.2, 1.0, num_cells)
    if num_cells >= 8:
        k_bar[-1] = 0.0; k_bar[0] = 1.0; k_bar[num_cells // 2] = 0.0
    spec_kw.setdefault("low_gamma_barrier_enabled", True)
    spec_kw.setdefault("low_gamma_barrier_loc", 1.5)
    spec_kw.setdefault("low_gamma_barrier_scale", 0.35)
    spec_kw.setdefault("tau", 2.5)
    spec_kw.setdefault("tau_prior_alpha", 0.7); spec_kw.setdefault("tau_prior_beta", 0.3)
    spec_kw.setdefault("inv_nbar_prior_alpha", 0.4); spec_kw.setdefault("inv_nbar_prior_beta", 1.7)
    spec = SkygridSpec(**spec_kw)
    gam = adversarial_gammas(num_knots, spec.low_gamma_barrier_loc)
    return name, PopModel.skygrid(x, gam, log_linear), spec, t_ref, t_step, first_cell, k_bar, inner_t
