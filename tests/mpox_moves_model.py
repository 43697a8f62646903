"""The APOBEC (mpox) model's moves restated on exact_model's arithmetic: the two q of Run::derive_evo (reference core/run.cpp:400-435), the sums
Run::mpox_hack_moves starts from (:854-905) and every number a round of it reports (:908-947, with safe_sample_truncated_gamma,
core/safe_gamma_math.h:110-139).  A third party for the HIP kernel (csrc/emat_mpox_kernels.hpp): Fractions, mpmath at 50 digits for the regularised
upper incomplete gamma function Q(a, x) and its inverse, and every sum an `Exact` with its condition magnitude S and term count n (exact_model's
docstring), so that a float64 evaluation of the reference's formula in any order lies within (n + 8) u S.

Nothing here runs a chain: the state before a round (mu, mu*), the device's own draws (mu_draw, and the Q_hi, rand_Q and y of its rho draw) and the
round's stream words (which the CPU restates bit for bit from the key) are INPUTS, and `check_round` restates one line of the reference from them
at a time.  A chain is never compared end to end.

S and n, by exact_model's rules:
- rho = mu* / mu is one quotient: S = rho, n = 1;
- Ttwiddle is 8 stored numbers; Ttwiddle_eff = Ttwiddle + 2 rho Ttwiddle* adds a sum of two, a quotient, two products and a sum: n = 8 + 6, all terms
  of one sign, so S is the value;
- the shape M + alpha - 1 counts M + |alpha| + 1, the rate Ttwiddle_eff + beta counts Ttwiddle_eff + |beta|;
- -(new - old) Ttwiddle_eff counts (new + old) Ttwiddle_eff; a count times log(y' / y) counts count (|log| + 1): the quotient's relative error is an
  absolute error of the log;
- beta = mu Ttwiddle* / 3: a sum of two, a product, a quotient: S the value, n = 4;
- -2 mu (rho' - rho) Ttwiddle* counts 2 mu (rho' + rho) Ttwiddle*; M* log((1 + 6 rho') / (1 + 6 rho)) counts M* (|log| + 1 + 6): each 1 + 6 rho rounds
  twice and the quotient once.
What is NOT a sum is held as the issue of this feature states it: the gamma draw to 1e-9 relative of the restated sampler (log, sqrt and cos are each
side's own), Q_hi to 1e-12 + 1e-10 Q, y to 1e-9 max(1, y), rand_Q to 2 ulp, and k, new_rho and mu* as the float64 functions of y they are.
"""
from __future__ import annotations

import math
from fractions import Fraction as F

import mpmath
import numpy as np

import skygrid_streams as RS
from exact_model import Exact, _fl, _log

ID_MU, ID_RHO = 0xFFFFFFF6, 0xFFFFFFF5     # include/emat_backend.h
MU_WORDS = 256                             # round i's mu draw starts at word 256 i
_DPS = 50
A, C, G, T_ = 0, 1, 2, 3


def derive_q(rho):
    """(q0, q1) of Run::derive_evo (run.cpp:407-432) as Fractions: Jukes-Cantor, and on the sites with APOBEC context C -> T and G -> A faster by 2 rho.
    The off-diagonal rate is the third itself (the engines hold the double 1. / 3., one rounding away)."""
    rho = rho if isinstance(rho, F) else _fl(rho)
    third = F(1, 3)
    q0 = [[F(-1) if a == b else third for b in range(4)] for a in range(4)]
    q1 = [row[:] for row in q0]
    q1[C][T_] += 2 * rho; q1[C][C] -= 2 * rho
    q1[G][A] += 2 * rho; q1[G][G] -= 2 * rho
    return q0, q1


def sums(T, M):
    """(M, M*, Ttwiddle, Ttwiddle*) of run.cpp:854-866, :897-905: the counts as ints, the lengths as Exacts."""
    Tf = [[v if isinstance(v, F) else _fl(v) for v in row] for row in T]
    assert len(Tf) == 2 and len(M) == 2
    nm = sum(int(M[p][a][b]) for p in range(2) for a in range(4) for b in range(4) if a != b)
    m_star = int(M[1][C][T_]) + int(M[1][G][A])
    tt = sum((v for row in Tf for v in row), F(0))
    ts = Tf[1][C] + Tf[1][G]
    return nm, m_star, Exact(tt, tt, 8), Exact(ts, ts, 2)


def round_top(mu, mu_star, T, M):
    """(rho, Ttwiddle_eff) at the top of a round (run.cpp:911-912)."""
    _, _, tt, ts = sums(T, M)
    rho = _fl(mu_star) / _fl(mu)
    te = tt.value + 2 * rho * ts.value
    return Exact(rho, rho, 1), Exact(te, te, 14)


def mu_posterior(mu, mu_star, T, M, alpha, beta):
    """(shape, rate) of the Gamma the round's mu is drawn from (run.cpp:916-918)."""
    nm, _, _, _ = sums(T, M)
    _, te = round_top(mu, mu_star, T, M)
    alpha, beta = _fl(alpha), _fl(beta)
    return Exact(nm + alpha - 1, nm + abs(alpha) + 1, 3), Exact(te.value + beta, te.value + abs(beta), te.n + 1)


def mu_deltas(old_mu, new_mu, mu_star, T, M, alpha, beta):
    """(delta log G, delta log other priors) of the mu draw (run.cpp:924-926); mu* / old_mu is the rho of the round's top."""
    nm, _, _, _ = sums(T, M)
    _, te = round_top(old_mu, mu_star, T, M)
    old, new, alpha, beta = _fl(old_mu), _fl(new_mu), _fl(alpha), _fl(beta)
    lg = _log(new / old)
    dG = Exact(-(new - old) * te.value + nm * lg, (new + old) * te.value + nm * (abs(lg) + 1), te.n + 6)
    dP = Exact((alpha - 1) * lg - beta * (new - old), (abs(alpha) + 1) * (abs(lg) + 1) + abs(beta) * (new + old), 8)
    return dG, dP


def rho_gamma(mu, T, M):
    """(alpha, beta) of the truncated Gamma k = 1 + 6 rho is drawn from (run.cpp:935-936), mu the value AFTER the round's mu draw."""
    _, m_star, _, ts = sums(T, M)
    b = _fl(mu) * ts.value / 3
    return m_star + 1, Exact(b, b, 4)


def rho_delta(mu, old_rho, new_rho, T, M):
    """delta log G of the rho draw (run.cpp:943-944): mu after the round's mu draw, old_rho from the round's top."""
    _, m_star, _, ts = sums(T, M)
    mu = _fl(mu); o = old_rho if isinstance(old_rho, F) else _fl(old_rho); n = _fl(new_rho)
    lg = _log((1 + 6 * n) / (1 + 6 * o))
    return Exact(-2 * mu * (n - o) * ts.value + m_star * lg, 2 * mu * (n + o) * ts.value + m_star * (abs(lg) + 7), 12)


def log_likelihood(mu, rho, T, M):
    """log G up to what no parameter touches, from the sufficient statistics and the two q: every branch's -mu q_a T and every mutation's log(mu q_ab),
    exact_model's branch and mutation terms summed over the tree (a Fraction)."""
    q = derive_q(rho)
    mu = mu if isinstance(mu, F) else _fl(mu)
    v = F(0)
    for p in range(2):
        for a in range(4):
            v -= mu * -q[p][a][a] * (T[p][a] if isinstance(T[p][a], F) else _fl(T[p][a]))
            for b in range(4):
                if a != b and int(M[p][a][b]) > 0:
                    v += int(M[p][a][b]) * _log(mu * q[p][a][b])
    return v


# ---- Q(a, x) and its inverse -------------------------------------------------------------------------------------------------------
def gamma_q(a, x):
    """The regularised upper incomplete gamma function Q(a, x) = Gamma(a, x) / Gamma(a), an mpmath number at 50 digits."""
    with mpmath.workdps(_DPS):
        if x == math.inf:
            return mpmath.mpf(0)
        return +mpmath.gammainc(mpmath.mpf(a), mpmath.mpf(x), mpmath.inf, regularized=True)


def gamma_q_inv(a, q):
    """The y with Q(a, y) = q for a >= 1 and 0 < q < 1: Newton on log Q(a, y) - log q, which is concave and decreasing in y (a Gamma of shape >= 1
    has a log-concave survival function), from the mode's side; d/dy log Q = -density / Q."""
    with mpmath.workdps(_DPS):
        a, q = mpmath.mpf(a), mpmath.mpf(q)
        if q >= 1:
            return mpmath.mpf(0)
        lq, lg = mpmath.log(q), mpmath.loggamma(a)
        y = a                                                   # left of the root or right of it: Newton on a concave function lands left, then climbs
        for _ in range(400):
            Q = mpmath.gammainc(a, y, mpmath.inf, regularized=True)
            dens = mpmath.exp(-y + (a - 1) * mpmath.log(y) - lg)
            y_new = y + (mpmath.log(Q) - lq) * Q / dens
            if y_new <= 0:
                y_new = y / 2
            if abs(y_new - y) <= mpmath.mpf(10) ** -40 * y_new:
                return +y_new
            y = y_new
        raise ArithmeticError("gamma_q_inv(%s, %s) did not converge" % (a, q))


# ---- the streams -------------------------------------------------------------------------------------------------------------------
def rho_uniform(key, i):
    """Round i's uniform in (0, 1]: word i of the rho stream through to_oc, the device's bit for bit."""
    return float(RS.to_oc(RS.word(np.uint64(key), ID_RHO, i)))


def gamma_draw_at(key, stream_id, shape, rate, first_word):
    """gamma_draw of csrc/emat_gamma_pure.hpp on the stream (key, stream_id) from word `first_word` on, in float64: Marsaglia-Tsang, a shape below 1
    drawn at shape + 1 and multiplied by u^(1 / shape).  Returns (the draw, the words taken)."""
    key = np.uint64(key); at = int(first_word)

    def next64():
        nonlocal at
        w = RS.word(key, stream_id, at); at += 1
        return w
    boost = shape < 1.0
    a = shape + 1.0 if boost else shape
    d = a - 1.0 / 3.0; c = 1.0 / math.sqrt(9.0 * d)
    g = d
    for _ in range(64):
        u1, u2 = float(RS.to_oc(next64())), float(RS.to_co(next64()))
        x = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586476925 * u2)
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        u = float(RS.to_oo(next64()))
        x2 = x * x
        if u < 1.0 - 0.0331 * (x2 * x2) or math.log(u) < 0.5 * x2 + d * (1.0 - v + math.log(v)):
            g = d * v
            break
    if boost:
        u = float(RS.to_oo(next64()))
        g *= math.exp(math.log(u) / shape)
    return g / rate, at - int(first_word)


# ---- a round, number by number -----------------------------------------------------------------------------------------------------
RHO_FIELDS = ("alpha", "beta", "Q_lo", "Q_hi", "u", "rand_Q", "y", "k", "new_rho", "rho_delta_log_G")


def _ulps(a, b):
    return abs(a - b) / math.ulp(max(abs(a), abs(b))) if a != b else 0.0


def check_round(tally, rec, i, mu, mu_star, spec, T, M, key, where=""):
    """Round i's record `rec` (the fields of emat_mpox_round) against the model, from the state (mu, mu*) before it.  Sums go through tally.check; what is
    no sum is held to the tolerance the module's docstring states, a miss appended to tally.fail.  Returns (mu, mu* after the round, the sum of the
    bounds of what it added to log G, whether its rho step ran / was skipped / was degenerate as "done" / "skipped" / "degenerate")."""
    w = "%s round %d" % (where, i)

    def hold(cond, what):
        if not cond:
            tally.fail.append("%s %s: %s" % (tally.who, w, what))
    mu, mu_star = float(mu), float(mu_star)
    nm, m_star, tt, ts = sums(T, M)
    rho, te = round_top(mu, mu_star, T, M)
    hold(float(rec["mu"]) == mu, "mu before the round is %r, the state holds %r" % (float(rec["mu"]), mu))
    tally.check("rho", rho, rec["rho"], w)
    tally.check("Ttwiddle_eff", te, rec["Ttwiddle_eff"], w)
    shape, rate = mu_posterior(mu, mu_star, T, M, spec.mu_prior_alpha, spec.mu_prior_beta)
    tally.check("mu_shape", shape, rec["mu_shape"], w)
    tally.check("mu_rate", rate, rec["mu_rate"], w)
    bounds = 0.0
    if float(rec["mu_shape"]) > 0.0 and float(rec["mu_rate"]) > 0.0:      # drawn whether needed or not; log, sqrt and cos are each side's own
        cpu, taken = gamma_draw_at(key, ID_MU, float(rec["mu_shape"]), float(rec["mu_rate"]), MU_WORDS * i)
        hold(taken <= 193, "the restated draw took %d words" % taken)
        hold(abs(float(rec["mu_draw"]) - cpu) <= 1e-9 * abs(cpu), "mu_draw %r, the restated sampler %r" % (float(rec["mu_draw"]), cpu))
    else:
        hold(math.isnan(float(rec["mu_draw"])) and not spec.do_mu, "a draw from a posterior that is none")
    if spec.do_mu:
        dG, dP = mu_deltas(mu, rec["mu_draw"], mu_star, T, M, spec.mu_prior_alpha, spec.mu_prior_beta)
        tally.check("mu_delta_log_G", dG, rec["mu_delta_log_G"], w)
        tally.check("mu_delta_log_other_priors", dP, rec["mu_delta_log_other_priors"], w)
        hold(int(rec["mu_done"]) == 1, "mu_done")
        mu = float(rec["mu_draw"]); bounds += dG.bound()
    else:
        hold((float(rec["mu_delta_log_G"]), float(rec["mu_delta_log_other_priors"]), int(rec["mu_done"])) == (0.0, 0.0, 0), "the mu draw is off and left a trace")
    if ts.value == 0:                                                         # run.cpp:930
        hold(all(float(rec[f]) == 0.0 for f in RHO_FIELDS) and (int(rec["rho_done"]), int(rec["rho_degenerate"])) == (0, 0), "a skipped rho step left a trace")
        return mu, mu_star, bounds, "skipped"
    alpha, beta = rho_gamma(mu, T, M)                                         # ... with the NEW mu
    hold(float(rec["alpha"]) == float(alpha), "alpha %r, M* + 1 = %d" % (float(rec["alpha"]), alpha))
    tally.check("beta", beta, rec["beta"], w)
    hold(float(rec["u"]) == rho_uniform(key, i), "u is not word %d of the rho stream" % i)
    hold(float(rec["Q_lo"]) == 0.0, "Q_lo")
    b, Q_hi = float(rec["beta"]), float(rec["Q_hi"])
    Q = float(gamma_q(alpha, b))                                              # at the device's own beta
    hold(abs(Q_hi - Q) <= 1e-12 + 1e-10 * Q, "Q_hi %r, Q(%d, %r) = %r" % (Q_hi, alpha, b, Q))
    if not (b > 0.0 and 0.0 < Q_hi):                                          # the reference's CHECK_GT / CHECK_LT: the step ends, rho stays
        hold((int(rec["rho_done"]), int(rec["rho_degenerate"])) == (0, 1) and all(float(rec[f]) == 0.0 for f in RHO_FIELDS[5:]), "a degenerate rho step must end with rho unchanged")
        return mu, mu_star, bounds, "degenerate"
    hold((int(rec["rho_done"]), int(rec["rho_degenerate"])) == (1, 0), "rho_done")
    u, rand_Q, y, k, new_rho = (float(rec[f]) for f in ("u", "rand_Q", "y", "k", "new_rho"))
    hold(_ulps(rand_Q, 0.0 + (Q_hi - 0.0) * u) <= 2.0, "rand_Q %r, Q_lo + (Q_hi - Q_lo) u = %r" % (rand_Q, Q_hi * u))
    y_ex = float(gamma_q_inv(alpha, rand_Q))                                  # at the device's own rand_Q
    hold(abs(y - y_ex) <= 1e-9 * max(1.0, y_ex), "y %r, the inverse of Q(%d, .) at %r is %r" % (y, alpha, rand_Q, y_ex))
    hold(k == max(1.0, y / b), "k %r is not max(1, y / beta) = %r" % (k, max(1.0, y / b)))
    hold(new_rho == (k - 1.0) / 6.0, "new_rho %r is not (k - 1) / 6" % new_rho)
    dR = rho_delta(mu, rho.value, new_rho, T, M)
    tally.check("rho_delta_log_G", dR, rec["rho_delta_log_G"], w)
    return mu, mu * new_rho, bounds + dR.bound(), "done"


def check_call(tally, r, spec, T, M, key, where=""):
    """A whole result `r` (the fields of emat_mpox_result with its trace): its sums, every round from the state the rounds before it left, its totals and
    its counters.  Returns the sum of the bounds of what the call added to log G."""
    def hold(cond, what):
        if not cond:
            tally.fail.append("%s %s: %s" % (tally.who, where, what))
    nm, m_star, tt, ts = sums(T, M)
    hold((r.M, r.M_star) == (float(nm), float(m_star)), "M, M*")
    tally.check("Ttwiddle", tt, r.Ttwiddle, where)
    tally.check("Ttwiddle_star", ts, r.Ttwiddle_star, where)
    mu, mu_star = float(spec.mu), float(spec.mu_star)
    hold(len(r.trace) == spec.rounds, "the trace has %d rounds" % len(r.trace))
    acc_G, acc_P, bounds, ends = [], [], 0.0, {"done": 0, "skipped": 0, "degenerate": 0}
    for i, rec in enumerate(r.trace):
        mu, mu_star, bd, end = check_round(tally, rec, i, mu, mu_star, spec, T, M, key, where)
        acc_G += [float(rec["mu_delta_log_G"]), float(rec["rho_delta_log_G"])]; acc_P.append(float(rec["mu_delta_log_other_priors"]))
        bounds += bd; ends[end] += 1
    hold((r.mu, r.mu_star) == (mu, mu_star), "mu, mu* after the call are %r, %r; the rounds leave %r, %r" % (r.mu, r.mu_star, mu, mu_star))
    hold((r.rho_skipped, r.rho_degenerate) == (ends["skipped"], ends["degenerate"]), "rho_skipped, rho_degenerate")
    fs = lambda vs: Exact(sum((F(v) for v in vs), F(0)), sum((abs(F(v)) for v in vs), F(0)), len(vs))
    tally.check("delta_log_G (total)", fs(acc_G), r.delta_log_G, where)
    tally.check("delta_log_other_priors", fs(acc_P), r.delta_log_other_priors, where)
    return bounds


# ---- the rounds in float64 on the CPU (what the tests of the model itself check `check_round` against) ------------------------------
def float_round(i, mu, mu_star, spec, T, M, key, old_rho_after_mu=False, rho_draw_with_old_mu=False):
    """Round i as run.cpp:908-947 states it, in float64 with scipy's Q and inverse; the two switches doctor it the two ways a restatement goes wrong most
    easily.  Returns (the record as a dict, mu, mu* after it)."""
    import scipy.special as sp
    T = np.asarray(T, np.float64)
    nm = sum(int(M[p][a][b]) for p in range(2) for a in range(4) for b in range(4) if a != b)
    m_star = int(M[1][C][T_]) + int(M[1][G][A])
    tt = 0.0
    for p in range(2):
        for a in range(4):
            tt += float(T[p][a])
    ts = float(T[1][C]) + float(T[1][G])
    rec = dict.fromkeys(RHO_FIELDS, 0.0); rec.update(mu_done=0, rho_done=0, rho_degenerate=0, mu_delta_log_G=0.0, mu_delta_log_other_priors=0.0)
    rho = mu_star / mu
    te = tt + 2 * rho * ts
    shape, rate = nm + spec.mu_prior_alpha - 1.0, te + spec.mu_prior_beta
    draw = gamma_draw_at(key, ID_MU, shape, rate, MU_WORDS * i)[0] if shape > 0.0 and rate > 0.0 else math.nan
    rec.update(mu=mu, rho=rho, Ttwiddle_eff=te, mu_shape=shape, mu_rate=rate, mu_draw=draw)
    old_mu = mu
    if spec.do_mu:
        mu = draw
        rec.update(mu_delta_log_G=-(mu - old_mu) * te + nm * math.log(mu / old_mu),
                   mu_delta_log_other_priors=(spec.mu_prior_alpha - 1) * math.log(mu / old_mu) - spec.mu_prior_beta * (mu - old_mu), mu_done=1)
    if ts > 0.0:
        alpha, beta = m_star + 1.0, (old_mu if rho_draw_with_old_mu else mu) * ts / 3
        u = rho_uniform(key, i)
        Q_hi = float(sp.gammaincc(alpha, beta))
        rec.update(alpha=alpha, beta=beta, Q_lo=0.0, Q_hi=Q_hi, u=u)
        if not (beta > 0.0 and 0.0 < Q_hi):
            rec["rho_degenerate"] = 1
        else:
            rand_Q = 0.0 + (Q_hi - 0.0) * u
            y = float(sp.gammainccinv(alpha, rand_Q))
            k = max(1.0, y / beta)
            new_rho = (k - 1.0) / 6.0
            old_rho = mu_star / mu if old_rho_after_mu else rho
            rec.update(rand_Q=rand_Q, y=y, k=k, new_rho=new_rho, rho_done=1,
                       rho_delta_log_G=-2 * mu * (new_rho - old_rho) * ts + m_star * math.log((1 + 6 * new_rho) / (1 + 6 * old_rho)))
            mu_star = mu * new_rho
    return rec, mu, mu_star
