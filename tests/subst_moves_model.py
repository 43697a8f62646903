"""The substitution-model moves restated on exact_model's arithmetic: the q of an HKY model (reference core/evo_hky.cpp:7-50), the posterior
mu_move draws from (core/run.cpp:781-821) and every number a step of hky_frequencies_move (:953-1034) / hky_kappa_move (:1036-1103) reports.
A third party for the HIP kernel (csrc/emat_subst_kernels.hpp): Fractions, mpmath at 60 digits, and every quantity an `Exact` with its
condition magnitude S and term count n (exact_model's docstring), so that a float64 evaluation of the reference's formula in any order lies
within (n + 8) u S.

Nothing here draws random numbers or runs a chain: the device's draws (the four words of a step, which the CPU restates bit for bit from the
key) and its state before each step (kappa and pi, from its trace; mu, from its result) are INPUTS, and each function restates one line of
the reference from them.

S and n, by exact_model's rules:
- an entry of q is r_ab pi_b / R, R = sum_ab pi_a r_ab pi_b, every term positive: a float64 evaluation carries a relative error of at most
  N_Q = 16 u (three products and three sums into a row, a product and four sums into R, a quotient and a product, two more sums into the
  diagonal: 14, and two for the second order).  A PROPOSED model's entries carry N_PROPOSAL = 6 more: pi + d rounds where d = 0.01 u0 has
  rounded, and kappa scale holds the four roundings of scale = 0.75 + (1 / 0.75 - 0.75) u0 and its own; q is no more sensitive to kappa
  or to one pi than proportionally (d is at most 0.01 of a pi that stays inside (0, 1) ... times the 1 / pi the ratio pi' / pi can carry,
  which the root term's own log counts).  These go into n, since they multiply every term alike;
- the branch term mu (q'_a - q_a) T counts mu (q'_a + q_a) T: the two escape rates round before they cancel;
- a count times log(y' / y) counts count (|log| + 1): the quotient's relative error is an absolute error of the log;
- the kappa prior ratio log(exp(x) old / new), x = ((log old - 1)^2 - (log new - 1)^2) / (2 1.25^2), counts each square's error 2 |d| (|log| + 1 + 6)
  + d^2 over 3.125, |x| + 1 for the exp, |log(old / new)| and 8 for the product, the quotient, the proposal's own roundings and the log;
- log(old / new) counts |log| + 1 + 6;
- log_metropolis, a sum, counts every term's own S plus every term's magnitude.
"""
from __future__ import annotations

from fractions import Fraction as F

from exact_model import Exact, _fl, _log

FREQ_DELTA = F(0.01)             # run.cpp:964, the double
SCALE_LO = F(0.75)               # run.cpp:1049
SCALE_HI = F(1.0 / 0.75)         # ... and the double 1 / 0.75
MEAN_LOG_KAPPA, SIGMA_LOG_KAPPA = F(1), F(5, 4)   # run.cpp:1061-1062
N_Q, N_PROPOSAL = 16, 6


def hky_q(kappa, pi):
    """q[a][b] of Hky_model::derive_site_evo_model as Fractions: exact for the float64 (or Fraction) kappa and pi given.  A, C, G, T = 0 .. 3;
    transitions are A <-> G and C <-> T."""
    k = kappa if isinstance(kappa, F) else _fl(kappa)
    p = [x if isinstance(x, F) else _fl(x) for x in pi]
    r = [[F(0) if a == b else (k if (a ^ b) == 2 else F(1)) for b in range(4)] for a in range(4)]
    R = sum(p[a] * r[a][b] * p[b] for a in range(4) for b in range(4))
    q = [[r[a][b] / R * p[b] for b in range(4)] for a in range(4)]
    for a in range(4):
        q[a][a] = -sum(q[a][b] for b in range(4) if b != a)
    return q


def _stats(T, M, C=None):
    """(Ttwiddle_beta_a as Fractions [P][4], num_muts_ab summed over the partitions [4][4], num_muts, root counts [4])."""
    T = [[v if isinstance(v, F) else _fl(v) for v in row] for row in T]      # (a test may hand in the exact statistics)
    P = len(T)
    Mab = [[sum(int(M[p][a][b]) for p in range(P)) for b in range(4)] for a in range(4)]
    nm = sum(Mab[a][b] for a in range(4) for b in range(4) if a != b)
    return T, Mab, nm, ([int(c) for c in C] if C is not None else [0] * 4)


def _q_of(q):
    """A q matrix handed in as float64 (what an engine was given), as Fractions."""
    return [[_fl(q[a][b]) for b in range(4)] for a in range(4)]


def mu_posterior(kappa, pi, T, M, alpha, beta, q=None):
    """(shape, rate, Ttwiddle, num_muts) of the Gamma mu_move draws from (run.cpp:797-810) under the model (kappa, pi) -- or under the float64 `q`."""
    T, _, nm, _ = _stats(T, M)
    q = hky_q(kappa, pi) if q is None else _q_of(q)
    Tt = sum(-q[a][a] * row[a] for row in T for a in range(4))
    n = N_Q + 4 * len(T) + 2
    return Exact(nm + _fl(alpha), nm + abs(_fl(alpha)), 2), Exact(Tt + _fl(beta), Tt + abs(_fl(beta)), n), Exact(Tt, Tt, n), nm


def mu_deltas(old_mu, new_mu, kappa, pi, T, M, alpha, beta, q=None):
    """(delta log G, delta log other priors) of mu_move (run.cpp:818-820) from the draw."""
    old, new, alpha, beta = _fl(old_mu), _fl(new_mu), _fl(alpha), _fl(beta)
    _, _, Tt, nm = mu_posterior(kappa, pi, T, M, alpha, beta, q)
    lg = _log(new / old)
    dG = Exact(-(new - old) * Tt.value + nm * lg, (new + old) * Tt.value + nm * (abs(lg) + 1), Tt.n + 6)
    dP = Exact((alpha - 1) * lg - beta * (new - old), (abs(alpha) + 1) * (abs(lg) + 1) + abs(beta) * (new + old), 8)
    return dG, dP


def pi_proposal(pi, u0, u1, u2):
    """(d, ia, ib, the proposed pi as Fractions or None when it leaves (0, 1)) of hky_frequencies_move (run.cpp:964-979), from the step's words."""
    d = FREQ_DELTA * _fl(u0)
    ia = int(4.0 * float(u1)); ib = (ia + 1 + int(3.0 * float(u2))) % 4
    p = [_fl(x) for x in pi]
    p[ia] += d; p[ib] -= d
    inside = 0 < p[ia] < 1 and 0 < p[ib] < 1
    return Exact(d, d, 1), ia, ib, (p if inside else None)


def kappa_proposal(kappa, u0):
    """(scale, the proposed kappa as a Fraction) of hky_kappa_move (run.cpp:1049-1054)."""
    u0 = _fl(u0)
    scale = SCALE_LO + (SCALE_HI - SCALE_LO) * u0
    return Exact(scale, SCALE_LO + (SCALE_HI + SCALE_LO) * u0, 4), _fl(kappa) * scale


def delta_log_G(mu, kappa, pi, new_kappa, new_pi, T, M, C, root_term, n_new=N_Q + N_PROPOSAL, q_old=None, q_new=None):
    """The reference's sums (run.cpp:985-1020, :1070-1088) for the move from (kappa, pi) to (new_kappa, new_pi) under mu: branch lengths, root
    counts where `root_term`, mutations.  None where the reference forces a rejection (a count above 0 against a q or pi of 0).  `q_old`,
    `q_new`: the two models' float64 matrices instead of the exact ones (what a whole-tree log G was evaluated with)."""
    T, Mab, _, C = _stats(T, M, C)
    mu = _fl(mu)
    qo = hky_q(kappa, pi) if q_old is None else _q_of(q_old)
    qn = hky_q(new_kappa, new_pi) if q_new is None else _q_of(q_new)
    po = [x if isinstance(x, F) else _fl(x) for x in pi]; pn = [x if isinstance(x, F) else _fl(x) for x in new_pi]
    v, S, terms = F(0), F(0), 0
    for row in T:
        for a in range(4):
            v -= mu * (-qn[a][a] - -qo[a][a]) * row[a]
            S += mu * (-qn[a][a] + -qo[a][a]) * row[a]
            terms += 1
    if root_term:
        for a in range(4):
            if C[a] > 0:
                if pn[a] == 0:
                    return None
                lg = _log(pn[a] / po[a])
                v += C[a] * lg; S += C[a] * (abs(lg) + 1); terms += 1
    for a in range(4):
        for b in range(4):
            if a != b and Mab[a][b] > 0:
                if qn[a][b] == 0:
                    return None
                lg = _log(qn[a][b] / qo[a][b])
                v += Mab[a][b] * lg; S += Mab[a][b] * (abs(lg) + 1); terms += 1
    return Exact(v, S, N_Q + n_new + 2 + terms)


def kappa_prior_and_hastings(kappa, new_kappa):
    """(log of prior_new_over_prior_old, run.cpp:1064-1067; log of alpha_kappa_n_to_o_over_o_to_n, :1063, :1091)."""
    old = _fl(kappa); new = new_kappa if isinstance(new_kappa, F) else _fl(new_kappa)
    lo, ln = _log(old), _log(new)
    do, dn = lo - MEAN_LOG_KAPPA, ln - MEAN_LOG_KAPPA
    two_s2 = 2 * SIGMA_LOG_KAPPA * SIGMA_LOG_KAPPA
    x = (-(dn * dn) + do * do) / two_s2
    lr = lo - ln
    S_prior = (2 * abs(dn) * (abs(ln) + 7) + 2 * abs(do) * (abs(lo) + 7) + 2 * dn * dn + 2 * do * do) / two_s2 + abs(x) + 1 + abs(lr) + 8
    return Exact(x + lr, S_prior, 12), Exact(lr, abs(lr) + 7, 4)


def log_metropolis(dG: Exact, log_prior_ratio: Exact = None, log_hastings: Exact = None) -> Exact:
    """run.cpp:1022, :1091."""
    terms = [t for t in (dG, log_prior_ratio, log_hastings) if t is not None]
    v = sum((t.value for t in terms), F(0))
    S = sum((F(t.S) + abs(t.value) for t in terms), F(0))
    return Exact(v, S, max(t.n for t in terms) + 4)
