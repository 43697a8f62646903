"""The APOBEC (mpox) model's moves on the device (emat_mpox_moves) against tests/mpox_moves_model.py.

Every number of every traced round is held against the exact model evaluated FROM THE DEVICE'S OWN STATE BEFORE IT: the mu and mu* the rounds so far
left, the mu it drew, and the beta, Q_hi and rand_Q of its own rho draw; the round's stream words are restated bit for bit from the key.  A chain is
never compared end to end.  Sums and increments lie within (n + 8) u S (Tally); the gamma draw within 1e-9 relative of the restated sampler; Q_hi within
1e-12 + 1e-10 Q and y within 1e-9 max(1, y) of mpmath at 50 digits -- the tolerances tests/test_parity_gpu.py holds the same routines to, over the range
they are pinned over (M* + 1 <= 1000, beta <= 1e5), and in one case beyond it (M* + 1 = 5001); rand_Q within 2 ulp; k, new_rho and mu* as the float64
functions of y they are.  Then the draws' distributions (KS over fixed keys), the sampler as a whole against a numpy quadrature of its target, the same
bits from every call and handle, and the handle's model after a call.

The statistics are hand-made 2 x 4 + 2 x 16 numbers: no tree is needed."""
import dataclasses
import math

import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as sst

import delphy_amd as d
import mpox_moves_model as MM
import skygrid_streams as RS
from delphy_amd.engine import mpox_q_matrices
from test_exact_model import Tally

pytestmark = pytest.mark.gpu

KS_P = 1e-6                      # the project's convention
L = 12


def _handle():
    b = d.EmatBackend(L)
    b.set_ref_sequence(np.arange(L) % 4)
    b.set_evo([1e-3] * 2, [[0.25] * 4] * 2, list(mpox_q_matrices(0.5)), np.ones(L), np.arange(L) % 2)
    return b


@pytest.fixture(scope="module")
def backend():
    b = _handle()
    yield b
    b.close()


# Statistics of a tree of a few hundred days under mu = 1e-3, a tenth of it on sites with APOBEC context: M = 44, M* = 15
TA = np.array([[41000.0, 52000.0, 38000.5, 47000.25], [4000.0, 5200.5, 3800.25, 4700.0]])
MA = np.array([[[0, 2, 5, 1], [2, 0, 1, 4], [4, 1, 0, 2], [1, 3, 1, 0]], [[0, 0, 1, 0], [0, 0, 0, 9], [6, 0, 0, 0], [0, 1, 0, 0]]], np.int64)
SPEC = d.MpoxSpec(mu=1e-3, mu_star=5e-4, mu_prior_alpha=1.0, mu_prior_beta=0.0, rounds=10)


def _with(a, entries):
    a = np.array(a)
    for idx, v in entries.items():
        a[idx] = v
    return a


T_NO_STAR = _with(TA, {(1, 1): 0.0, (1, 2): 0.0})                            # Ttwiddle* = 0
M_NO_STAR = _with(MA, {(1, 1, 3): 0, (1, 2, 0): 0})                          # M* = 0
T_800 = _with(TA, {(1, 1): 1.2e6, (1, 2): 1.2e6})                            # mu Ttwiddle* / 3 = 800 at mu = 1e-3
M_5000 = _with(MA, {(1, 1, 3): 3000, (1, 2, 0): 2000})                       # M* + 1 = 5001


def check(b, tally, spec, T, M, key, name=""):
    r = b.mpox_moves(spec, T, M, key=key, trace=True)
    MM.check_call(tally, r, spec, T, M, key, "%s key %d" % (name, key))
    assert all(math.isfinite(v) for v in (r.mu, r.mu_star, r.delta_log_G, r.delta_log_other_priors)) and r.mu > 0.0 and r.mu_star >= 0.0, name
    return r


CASES = [
    ("the references defaults", SPEC, TA, MA),
    ("one round", dataclasses.replace(SPEC, rounds=1), TA, MA),
    ("mu* starts at 0", dataclasses.replace(SPEC, mu_star=0.0), TA, MA),
    ("the mu draw off", dataclasses.replace(SPEC, do_mu=False), TA, MA),
    ("the mu draw off, mu* starts at 0", dataclasses.replace(SPEC, do_mu=False, mu_star=0.0, rounds=1), TA, MA),
    ("no APOBEC mutation", SPEC, TA, M_NO_STAR),
    ("a proper mu prior", dataclasses.replace(SPEC, mu_prior_alpha=1.5, mu_prior_beta=2e3), TA, MA),
    ("a shape below 1", dataclasses.replace(SPEC, mu_prior_alpha=1.5, mu_prior_beta=2e3), TA, np.zeros((2, 4, 4), np.int64)),
    ("thousands of mutations", SPEC, 50.0 * TA, 50 * MA),                 # M* + 1 = 751
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_every_traced_number(backend, case, record_property):
    name, spec, T, M = case
    tally = Tally("device")
    for key in (11, 12):
        r = check(backend, tally, spec, T, M, key, name)
        assert len(r.trace) == spec.rounds and r.rho_skipped == 0 and r.rho_degenerate == 0
        assert np.all(r.trace["rho_done"] == 1) and np.all(r.trace["mu_done"] == int(spec.do_mu))
        assert (r.mu == spec.mu) == (not spec.do_mu) and r.mu_star != spec.mu_star
        if name == "a shape below 1":
            assert np.all(r.trace["mu_shape"] == 0.5)                     # gamma_draw's boosted branch
        if name == "no APOBEC mutation":
            assert np.all(r.trace["alpha"] == 1.0) and r.M_star == 0.0
    tally.finish(record_property)


def test_rounds_0_does_nothing_and_a_call_without_a_trace_is_the_same_call(backend, record_property):
    tally = Tally("device")
    r0 = check(backend, tally, dataclasses.replace(SPEC, rounds=0), TA, MA, 41, "rounds 0")
    assert len(r0.trace) == 0 and (r0.mu, r0.mu_star, r0.delta_log_G, r0.delta_log_other_priors) == (1e-3, 5e-4, 0.0, 0.0)
    assert (r0.M, r0.M_star) == (44.0, 15.0)
    r3 = check(backend, tally, dataclasses.replace(SPEC, rounds=3), TA, MA, 41, "rounds 3")
    no_trace = backend.mpox_moves(dataclasses.replace(SPEC, rounds=3), TA, MA, key=41)
    assert no_trace.trace is None and (no_trace.mu, no_trace.mu_star, no_trace.delta_log_G) == (r3.mu, r3.mu_star, r3.delta_log_G)
    r10 = check(backend, tally, SPEC, TA, MA, 41, "rounds 10")
    assert np.array_equal(r10.trace[:3], r3.trace)                        # a round's draws depend on (key, i) alone
    off = check(backend, tally, dataclasses.replace(SPEC, do_mu=False), TA, MA, 41, "mu off")
    assert off.trace["mu_draw"][0] == r10.trace["mu_draw"][0] and np.array_equal(off.trace["u"], r10.trace["u"])     # drawn whether needed or not
    tally.finish(record_property)


def test_without_apobec_branch_length_every_rho_step_is_skipped(backend, record_property):
    tally = Tally("device")
    r = check(backend, tally, SPEC, T_NO_STAR, MA, 21, "Ttwiddle* = 0")
    assert r.Ttwiddle_star == 0.0 and r.rho_skipped == SPEC.rounds and r.rho_degenerate == 0 and np.all(r.trace["rho_done"] == 0)
    assert r.mu_star == SPEC.mu_star and r.mu != SPEC.mu and len(set(r.trace["mu_draw"].tolist())) == SPEC.rounds       # mu* stays while mu moves
    tally.finish(record_property)


def test_a_degenerate_q_range_ends_the_step_and_is_counted(backend, record_property):
    """M* = 0 and mu Ttwiddle* / 3 = 800: Q(1, 800) = exp(-800) underflows, Q_lo >= Q_hi, where the reference aborts (safe_gamma_math.h:124).  The step is
    skipped and counted, rho stays, and the call returns EMAT_OK."""
    tally = Tally("device")
    spec = dataclasses.replace(SPEC, do_mu=False, rounds=3)
    r = check(backend, tally, spec, T_800, M_NO_STAR, 31, "degenerate")
    assert np.all(np.abs(r.trace["beta"] - 800.0) < 1e-9) and np.all(r.trace["Q_hi"] == 0.0)
    assert r.rho_degenerate == 3 and r.rho_skipped == 0 and np.all(r.trace["rho_degenerate"] == 1) and np.all(r.trace["rho_done"] == 0)
    assert (r.mu, r.mu_star, r.delta_log_G) == (spec.mu, spec.mu_star, 0.0) and np.all(r.trace["rho"] == 0.5)
    moving = check(backend, tally, dataclasses.replace(spec, do_mu=True), T_800, M_NO_STAR, 31, "degenerate, mu moving")     # mu moves on; whatever its rho steps do is held to the model
    assert moving.mu != spec.mu
    tally.finish(record_property)


def test_beyond_the_pinned_range_5001(backend, record_property):
    """M* + 1 = 5001, five times the shape the incomplete-gamma routines are pinned up to, under the same two tolerances.  The inputs the device met are
    first put to the CPU oracle's routines (Boost's, which the reference calls), which must meet the tolerances there themselves."""
    from oracle_ffi import lib as oracle
    tally = Tally("device")
    spec = dataclasses.replace(SPEC, rounds=2)
    O = oracle()
    for key in (51, 52):
        r = backend.mpox_moves(spec, 100.0 * TA, M_5000, key=key, trace=True)
        for rec in r.trace:
            assert rec["alpha"] == 5001.0 and 0.0 < rec["beta"] <= 1e5 and rec["rho_done"] == 1
            q, y = float(MM.gamma_q(5001, float(rec["beta"]))), float(MM.gamma_q_inv(5001, float(rec["rand_Q"])))
            assert abs(O.orc_gamma_q(5001.0, float(rec["beta"])) - q) <= 1e-12 + 1e-10 * q
            assert abs(O.orc_gamma_q_inv(5001.0, float(rec["rand_Q"])) - y) <= 1e-9 * max(1.0, y)
            record_property("y_error_over_1e-9_max_1_y_key_%d" % key, float("%.3g" % (abs(float(rec["y"]) - y) / (1e-9 * max(1.0, y)))))
        MM.check_call(tally, r, spec, 100.0 * TA, M_5000, key, "M* + 1 = 5001 key %d" % key)
    tally.finish(record_property)


# ---- the same bits, and the handle's model ----------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a.trace, b.trace) and all(getattr(a, f) == getattr(b, f) for f in (
        "mu", "mu_star", "M", "M_star", "Ttwiddle", "Ttwiddle_star", "delta_log_G", "delta_log_other_priors", "rho_skipped", "rho_degenerate"))


def test_same_arguments_same_bits_in_every_call_and_on_every_handle(backend):
    spec = dataclasses.replace(SPEC, rounds=200)
    r1 = backend.mpox_moves(spec, TA, MA, key=77, trace=True)
    r2 = backend.mpox_moves(spec, TA, MA, key=77, trace=True)
    other = _handle()
    try:
        r3 = other.mpox_moves(spec, TA, MA, key=77, trace=True)
    finally:
        other.close()
    assert _same(r1, r2) and _same(r1, r3)
    assert np.all(r1.trace["rho_done"] == 1) and np.all(np.isfinite(r1.trace["rho_delta_log_G"])) and len(set(r1.trace["mu_draw"].tolist())) == 200
    r4 = backend.mpox_moves(spec, TA, MA, key=78, trace=True)
    assert not np.array_equal(r1.trace["u"], r4.trace["u"]) and r4.trace["mu_draw"][0] != r1.trace["mu_draw"][0]


def test_the_handles_model_after_a_call_and_after_a_refusal():
    b = _handle()
    try:
        r = b.mpox_moves(SPEC, TA, MA, key=61)
        mu, pi, q = b.get_evo()
        q0, q1 = mpox_q_matrices(r.mu_star / r.mu)                        # mpox_derive_q, mirrored in Python: the same float64 operations
        assert mu.tolist() == [r.mu, r.mu] and pi.tolist() == [[0.25] * 4] * 2
        assert np.array_equal(q[0], q0) and np.array_equal(q[1], q1) and q[1][1][3] > q[0][1][3] and q[1][2][0] == q[1][1][3]
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*mu_star"):
            b.mpox_moves(dataclasses.replace(SPEC, mu_star=-1.0), TA, MA, key=61)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*positive rate"):
            b.mpox_moves(SPEC, np.zeros((2, 4)), MA, key=61)
        again = b.get_evo()
        assert all(np.array_equal(x, y) for x, y in zip(again, (mu, pi, q)))
        assert np.array_equal(b.nu_l(), np.ones(L))                           # the site rates stay
    finally:
        b.close()


# ---- the draws' distributions ------------------------------------------------------------------------------------------------------
N_KEYS = 2000
KEYS = np.arange(7000, 7000 + N_KEYS, dtype=np.uint64)


@pytest.mark.parametrize("name,M,alpha", [("shape 0.5", np.zeros((2, 4, 4), np.int64), 1.5), ("shape 44", MA, 1.0)], ids=lambda v: v if isinstance(v, str) else "")
def test_the_mu_draws_follow_their_gamma(backend, name, M, alpha):
    """2 000 fixed keys, one round each: KS against Gamma(shape, rate), first shown on the CPU restatement of the stream at these keys."""
    spec = dataclasses.replace(SPEC, mu_prior_alpha=alpha, mu_prior_beta=0.25, rounds=1)
    first = backend.mpox_moves(spec, TA, M, key=int(KEYS[0]), trace=True).trace[0]
    shape, rate = float(first["mu_shape"]), float(first["mu_rate"])
    assert shape == {"shape 0.5": 0.5, "shape 44": 44.0}[name]
    draws = np.array([backend.mpox_moves(spec, TA, M, key=int(k)).mu for k in KEYS])
    dist = sst.gamma(shape, scale=1.0 / rate)
    cpu = RS.gamma_draw(KEYS, MM.ID_MU, shape, rate)                          # (round 0 starts at the stream's start)
    assert sst.kstest(cpu, dist.cdf).pvalue > KS_P                            # the keys' own
    assert np.allclose(draws, cpu, rtol=1e-9, atol=0)
    assert sst.kstest(draws, dist.cdf).pvalue > KS_P


@pytest.mark.parametrize("m_star,T", [(0, TA), (15, TA), (400, _with(TA, {(1, 1): 1.5e5, (1, 2): 1.5e5}))], ids=["M* 0", "M* 15", "M* 400"])
def test_the_k_draws_follow_their_truncated_gamma(backend, m_star, T):
    """2 000 fixed keys, one round each with the mu draw off: k = 1 + 6 rho against the CDF of Gamma(M* + 1, rate beta) truncated to [1, inf),
    F(k) = 1 - Q(alpha, beta k) / Q(alpha, beta), first shown on scipy's inverse at the keys' own uniforms."""
    M = _with(MA, {(1, 1, 3): m_star - m_star // 3, (1, 2, 0): m_star // 3})
    spec = dataclasses.replace(SPEC, do_mu=False, rounds=1)
    recs = [backend.mpox_moves(spec, T, M, key=int(k), trace=True).trace[0] for k in KEYS]
    alpha, beta = float(recs[0]["alpha"]), float(recs[0]["beta"])
    assert alpha == m_star + 1 and (beta == pytest.approx(100.0, rel=1e-3) if m_star == 400 else beta == pytest.approx(3.0, rel=1e-3))
    cdf = lambda k: 1.0 - sp.gammaincc(alpha, beta * np.asarray(k)) / sp.gammaincc(alpha, beta)
    u = RS.to_oc(RS.word(KEYS, MM.ID_RHO, 0))
    cpu = np.maximum(1.0, sp.gammainccinv(alpha, sp.gammaincc(alpha, beta) * u) / beta)
    assert sst.kstest(cpu, cdf).pvalue > KS_P                                 # the keys' own
    k = np.array([float(r["k"]) for r in recs])
    assert np.array_equal(np.array([float(r["u"]) for r in recs]), u) and np.all(k >= 1.0)
    assert np.allclose(k, cpu, rtol=1e-8, atol=0)
    assert sst.kstest(k, cdf).pvalue > KS_P


# ---- the sampler as a whole --------------------------------------------------------------------------------------------------------
def test_the_chain_samples_its_target(backend, record_property):
    """2 000 successive calls of 2 rounds, each from the last result's (mu, mu*): E[mu] and E[rho] against a numpy quadrature of the two marginals of
    P(mu, rho) ~ exp(-(beta + T + 2 rho T*) mu) mu^(M + alpha - 2) (1 + 6 rho)^M*  (run.cpp:843-844), by the rule the substitution-model moves' chains are
    held to: every mean within 4 batch-means standard errors (40 batches) of the quadrature, and an effective sample size of at least 200."""
    from test_subst_moves_gpu import BURN_IN, _chain_check
    n_calls = 2000
    spec = dataclasses.replace(SPEC, rounds=2)
    chain = np.zeros((n_calls, 2)); degenerate = 0
    mu, mu_star = spec.mu, spec.mu_star
    for i in range(-BURN_IN, n_calls):                                    # (the start is no draw from the target)
        r = backend.mpox_moves(dataclasses.replace(spec, mu=mu, mu_star=mu_star), TA, MA, key=0x5EED4000 + BURN_IN + i)
        mu, mu_star = r.mu, r.mu_star
        degenerate += r.rho_degenerate + r.rho_skipped
        if i >= 0:
            chain[i] = (mu, mu_star / mu)
    assert degenerate == 0                                                # no round may be degenerate
    Tt, Ts, M, Ms = float(TA.sum()), float(TA[1, 1] + TA[1, 2]), 44, 15
    span = chain.max(axis=0) - chain.min(axis=0)
    lo = np.maximum(chain.min(axis=0) - span, [chain.min(axis=0)[0] / 50.0, 0.0]); hi = chain.max(axis=0) + 2.0 * span

    def quad(n):
        m = np.linspace(lo[0], hi[0], n)[:, None]; rho = np.linspace(lo[1], hi[1], n)[None, :]
        logp = -(spec.mu_prior_beta + Tt + 2.0 * rho * Ts) * m + (M + spec.mu_prior_alpha - 2.0) * np.log(m) + Ms * np.log1p(6.0 * rho)
        w = np.exp(logp - logp.max()); w /= w.sum()
        edge = w[0].sum() + w[-1].sum() + w[:, -1].sum() + (w[:, 0].sum() if lo[1] > 0.0 else 0.0)
        return np.array([(w * m).sum(), (w * rho).sum()]), edge
    fine, edge = quad(1601); coarse, _ = quad(801)
    se = _chain_check(chain, fine, record_property, "mu_rho")
    assert np.all(np.abs(fine - coarse) < 0.1 * se) and edge < 1e-9, (fine, coarse, se, edge)
    assert chain[:, 0].std() > 0.1 * chain[:, 0].mean() and chain[:, 1].std() > 0.1 * chain[:, 1].mean()      # a wide posterior
