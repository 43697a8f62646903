"""The Exponential population moves restated on exact_model's arithmetic: the whole-tree coalescent prior under an Exp_pop_model{t0, n0, g,
min_pop} and every number a step of pop_size_move / pop_growth_rate_move reports (reference core/run.cpp:1237-1319;
core/scalable_coalescent.cpp:140-187; core/pop_model.cpp:22-91).  A third party for the HIP kernels (csrc/emat_exp_pop_kernels.hpp): Fractions,
mpmath at 60 digits, and every quantity an `Exact` with its condition magnitude S and term count n (exact_model's docstring), so that a float64
evaluation of the reference's formula in any order lies within (n + 8) u S.

Nothing here draws random numbers or runs a chain: the device's draws (the two uniforms of a step, which the CPU restates bit for bit from the key)
and its state before each step (n0, g and the prior it holds, from its trace) are INPUTS, and each function restates one line of the reference from them.

S of the steps' own lines, by exact_model's rules:
- scale = 0.75 + (1 / 0.75 - 0.75) u0 counts 0.75 + (4/3 + 0.75) u0: the constant 1 / 0.75 rounds, the difference rounds, the product and the sum round;
- new_n0 = scale old_n0 counts S(scale) old_n0;
- log(scale) counts |log scale| + 1 plus S(scale) / scale, the relative error its argument carries; log(old_n0 / new_n0) is -log(scale) with one more
  rounding in new_n0 and one in the quotient, and counts the same plus 2;
- 1 / new_n0 counts (1 + S(scale) / scale) / new_n0, 1 / old_n0 counts itself;
- new_g = old_g + (-w + 2 w u0) counts |old_g| + w + 2 w u0 (w = 1 / 365 rounds, the product and both sums round);
- |g - mu| counts |g| + |mu|, and S(new_g) + |mu| for the proposed g;
- log_metropolis, a sum of the two priors' difference, the prior ratio and the Hastings term, counts every term's own S (the issue's rule for a
  difference of two priors: the sum of their bounds) plus every term's magnitude, for the roundings of the sum itself.
"""
from __future__ import annotations

import math
from fractions import Fraction as F

import exact_model as X
from exact_model import Exact, _fl, _log
from skygrid_moves_model import Grid

W = F(1, 365)                    # the growth-rate window (run.cpp:1289)
SCALE_LO, SCALE_HI = F(3, 4), F(4, 3)   # run.cpp:1249-1251
STOPGAP = F(1e-100)              # scalable_coalescent.cpp:152-154
SMALLEST = F(1, 2 ** 1075)       # below this a float64 evaluation is 0


def exp_pop(t0, n0, g, min_pop) -> X.Pop:
    from delphy_amd.engine import PopModel
    return X.Pop(PopModel.exp(float(t0), float(n0), float(g), float(min_pop)))


def _rr(v: F) -> F:
    """v rounded to 300 significant bits (far below anything a check here resolves): a quotient's denominator would otherwise grow with every
    term a sum takes in.  Relative, not to a fixed 2^-260 as skygrid_moves_model rounds: a cell's N may lie at 1e-90 here."""
    if v == 0:
        return v
    shift = 300 - (abs(v.numerator).bit_length() - v.denominator.bit_length())
    if shift >= 0:
        return F((v.numerator << shift) // v.denominator, 1 << shift)
    return F(v.numerator // (v.denominator << -shift)) * (1 << -shift)


def popsize_bar(pop: X.Pop, grid: Grid, c):
    """(the cell's average N, its S, its n): pop_integral / t_step with the cell bounds' own rounding (exact_model.scalable_log_prior's rule)."""
    lo, hi = grid.bounds(c)
    I = pop.pop_integral(lo, hi)
    Nmax = max(pop.pop_at_time(lo).value, pop.pop_at_time(hi).value)
    return I.value / grid.t_step, (I.S + Nmax * 2 * grid.bound_mag(c)) / grid.t_step, I.n


def log_coalescent_prior(pop: X.Pop, grid: Grid, inner_t) -> Exact:
    """calc_log_prior (scalable_coalescent.cpp:163-187) node by node: -sum_c t_step k (k - 1) / (2 Nbar_c) - sum_i log N(t_i), with the
    reference's stopgap Nbar_c = 1e-100 where a float64 evaluation of the cell's integral is 0."""
    v, S, nmax = F(0), F(0), 0
    for c, k in enumerate(grid.k_bar):
        if k == 0 or k == 1:
            continue
        N, NS, n = popsize_bar(pop, grid, c)
        if N < SMALLEST:
            N, NS = STOPGAP, F(0)
        term = _rr(grid.t_step * k * (k - 1) / (2 * N))
        v -= term
        S += float(abs(term)) * (3 + float(NS / N))
        nmax = max(nmax, n)
    for t in inner_t:
        a, b = pop.neg_log_pop(_fl(t))
        v += a; S += b
    return Exact(v, S, 4 * len(grid.k_bar) + len(inner_t) + nmax)


def _scale(u0) -> Exact:
    u0 = _fl(u0)
    return Exact(SCALE_LO + (SCALE_HI - SCALE_LO) * u0, SCALE_LO + (SCALE_HI + SCALE_LO) * u0, 4)


def n0_step(old_n0, u0, alpha, beta):
    """pop_size_move's proposal (run.cpp:1249-1257) from the n0 held and the proposal uniform: (new_n0, log_prior_ratio, log(old_n0 / new_n0))."""
    old, alpha, beta = _fl(old_n0), _fl(alpha), _fl(beta)
    sc = _scale(u0)
    rel = sc.S / sc.value
    new = sc.value * old
    lg = _log(sc.value)
    S_log = abs(lg) + 1 + rel
    ratio = -(alpha + 1) * lg - beta * (1 / new - 1 / old)
    S_ratio = (abs(alpha) + 1) * S_log * 2 + abs(beta) * ((1 + rel) / new + 1 / old) * 2
    return Exact(new, sc.S * old, sc.n + 1), Exact(ratio, S_ratio, 12), Exact(-lg, S_log + 2, 6)


def g_step(old_g, u0, mu, scale):
    """pop_growth_rate_move's proposal (run.cpp:1289-1301): (new_g, log_prior_ratio)."""
    old, u0, mu, scale = _fl(old_g), _fl(u0), _fl(mu), _fl(scale)
    new = old + (-W + 2 * W * u0)
    S_new = abs(old) + W + 2 * W * u0
    ratio = (abs(old - mu) - abs(new - mu)) / scale
    return Exact(new, S_new, 5), Exact(ratio, (abs(old) + abs(mu) + S_new + abs(mu)) * 2 / scale, 10)


def log_metropolis(new_prior: Exact, old_prior: Exact, log_prior_ratio: Exact, log_hastings: Exact = None) -> Exact:
    """run.cpp:1265-1266, :1309 from the model's own priors of the two models."""
    terms = [new_prior, old_prior, log_prior_ratio] + ([log_hastings] if log_hastings is not None else [])
    v = new_prior.value - old_prior.value + log_prior_ratio.value + (log_hastings.value if log_hastings is not None else 0)
    S = sum((F(t.S) + abs(t.value) for t in terms), F(0))
    return Exact(v, S, max(t.n for t in terms) + 4)


def make_case(name, num_cells, num_inner, g, min_pop=0.0, n0=3.0, t_c=None, inner_span=None, seed=1, **spec_kw):
    """One input of emat_exp_pop_moves: (name, PopModel, ExpPopSpec, t_ref, t_step, first_cell, k_bar, inner_t).  The grid is
    [t_ref - num_cells t_step, t_ref) with t_ref = 1000 and t_step = 1/4 (cell bounds are exact doubles) and t0 = t_ref.  `t_c`: where the
    barrier is to start (min_pop is then chosen for it, so that t0 + log(min_pop / n0) / g rounds to it: the sum rounds at 1000's spacing, far
    coarser than the quotient's own error).  `inner_span`: the inner times lie in the last `inner_span` of the grid (all of it by default).
    The grid holds a cell with k_bar 0 and one with k_bar 1 where it has room."""
    import numpy as np
    from delphy_amd.engine import ExpPopSpec, PopModel
    rng = np.random.default_rng(seed)
    t_step, t_ref, first_cell = 0.25, 1000.0, -num_cells
    t0 = t_ref
    span = num_cells * t_step
    if t_c is not None:
        assert g != 0.0
        want = n0 * math.exp(g * (t_c - t0))
        min_pop = next(m for m in (want * (1.0 + k * 2.0 ** -52) for k in (0, 1, -1, 2, -2, 3, -3, 4, -4)) if t0 + math.log(m / n0) / g == t_c)
    inner_t = t_ref - rng.uniform(0.0, span if inner_span is None else inner_span, num_inner) * (1 - 1e-9) - 1e-9
    k_bar = 1.0 + 6.0 * rng.uniform(size=num_cells) * np.linspace(0.2, 1.0, num_cells)
    if num_cells >= 8:
        k_bar[-1] = 0.0; k_bar[1] = 1.0; k_bar[num_cells // 2] = 0.0
    spec_kw.setdefault("inv_n0_prior_alpha", 0.7); spec_kw.setdefault("inv_n0_prior_beta", 1.3)
    spec_kw.setdefault("g_prior_mu", 0.02); spec_kw.setdefault("g_prior_scale", 0.4)
    spec_kw.setdefault("rounds", 3)
    return name, PopModel.exp(t0, n0, g, min_pop), ExpPopSpec(**spec_kw), t_ref, t_step, first_cell, k_bar, inner_t
