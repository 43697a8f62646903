"""tests/mpox_moves_model.py against closed forms and the model's own definitions: the two q are rate matrices, with no APOBEC mutation counted the
truncated Gamma is a shifted exponential, a round's two increments of log G are the difference of the full log-likelihood in (mu, rho) -- the
statistics ARE sufficient -- and `check_round` passes the reference's round restated in float64 and refuses the two doctored ones.  No GPU."""
import math
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

import delphy_amd as d
import mpox_moves_model as MM
from test_exact_model import Tally

# Hand-made statistics of two site partitions: a tree of a few hundred days under mu = 1e-3, a tenth of the sites with APOBEC context
T = np.array([[9000.0, 11000.5, 8000.25, 10000.0], [1000.0, 1200.5, 900.25, 1100.0]])
M = np.array([[[0, 2, 5, 1], [2, 0, 1, 6], [4, 1, 0, 2], [1, 5, 1, 0]], [[0, 0, 1, 0], [0, 0, 0, 9], [6, 0, 0, 0], [0, 1, 0, 0]]], np.int64)
SPEC = d.MpoxSpec(mu=1e-3, mu_star=2e-3, mu_prior_alpha=1.0, mu_prior_beta=0.0, rounds=10)


@pytest.mark.parametrize("rho", [0.0, 0.5, 7.25, 1e-300, 1e6])
def test_the_two_q_are_rate_matrices_and_differ_where_apobec_acts(rho):
    q0, q1 = MM.derive_q(rho)
    for q in (q0, q1):
        for a in range(4):
            assert sum(q[a]) == 0                                         # every row sums to 0
            assert all(q[a][b] >= 0 for b in range(4) if b != a)
    diff = {(a, b): q1[a][b] - q0[a][b] for a in range(4) for b in range(4) if q1[a][b] != q0[a][b]}
    want = {(1, 3): 2 * F(rho), (1, 1): -2 * F(rho), (2, 0): 2 * F(rho), (2, 2): -2 * F(rho)} if rho else {}
    assert diff == want
    f0, f1 = d.engine.mpox_q_matrices(rho)                                # the Python mirror of mpox_derive_q
    for q, f in ((q0, f0), (q1, f1)):
        for a in range(4):
            for b in range(4):
                assert abs(F(float(f[a][b])) - q[a][b]) <= 2 * 2.0 ** -53 * abs(q[a][b])


@pytest.mark.parametrize("beta", [1e-3, 0.7, 30.0, 800.0])
def test_with_no_apobec_mutation_k_minus_1_is_exponential(beta):
    """M* = 0: alpha = 1, Q(1, x) = exp(-x), so Q_hi = exp(-beta), y = -log(rand_Q) and k - 1 = y / beta - 1 = -log(u) / beta ~ Exp(beta) exactly."""
    with mpmath.workdps(50):
        assert abs(MM.gamma_q(1, beta) / mpmath.exp(-mpmath.mpf(beta)) - 1) < mpmath.mpf(10) ** -45
        for u in (1.0, 0.75, 2.0 ** -53, 1e-9):
            rand_Q = MM.gamma_q(1, beta) * u
            y = MM.gamma_q_inv(1, rand_Q)
            assert abs(y / -mpmath.log(rand_Q) - 1) < mpmath.mpf(10) ** -38
            assert abs((y / beta - 1) - -mpmath.log(mpmath.mpf(u)) / beta) < mpmath.mpf(10) ** -35 * max(1, y / beta)


@pytest.mark.parametrize("a,q", [(1, 0.3), (16, 1e-5), (16, 0.999), (401, 1e-200), (1000, 0.5), (5001, 1e-3)])
def test_the_inverse_inverts(a, q):
    with mpmath.workdps(50):
        y = MM.gamma_q_inv(a, q)
        assert abs(MM.gamma_q(a, y) / mpmath.mpf(q) - 1) < mpmath.mpf(10) ** -30
    import scipy.special as sp
    assert float(y) == pytest.approx(float(sp.gammainccinv(a, q)), rel=1e-9)


def test_a_rounds_two_increments_are_the_difference_of_the_full_log_likelihood():
    """mu from 1e-3 to 1.3e-3 at the old rho, then rho from 2 to 3.5 at the new mu: the sum of the two increments is log L(new mu, new rho) - log L(old
    mu, old rho), built from T, M, q0 and q1 alone."""
    mu0, mu1, rho0, rho1 = 1e-3, 1.3e-3, 2.0, 3.5
    mu_star0 = mu0 * rho0
    assert mu_star0 / mu0 == rho0
    dG_mu, _ = MM.mu_deltas(mu0, mu1, mu_star0, T, M, 1.0, 0.0)
    dG_rho = MM.rho_delta(mu1, rho0, rho1, T, M)
    whole = MM.log_likelihood(mu1, rho1, T, M) - MM.log_likelihood(mu0, rho0, T, M)
    # both sides are exact rationals of the same float64 inputs up to mpmath's 60 digits in a few dozen logs
    assert abs((dG_mu.value + dG_rho.value) - whole) < F(1, 10 ** 40), (float(dG_mu.value + dG_rho.value), float(whole))
    assert abs(float(whole)) > 1.0                                       # (the change is no fixed point)
    # each alone: mu at the old rho, rho at the new mu
    assert abs(dG_mu.value - (MM.log_likelihood(mu1, rho0, T, M) - MM.log_likelihood(mu0, rho0, T, M))) < F(1, 10 ** 40)
    assert abs(dG_rho.value - (MM.log_likelihood(mu1, rho1, T, M) - MM.log_likelihood(mu1, rho0, T, M))) < F(1, 10 ** 40)


def _chain(spec, key, **doctor):
    """The rounds in float64; the doctoring acts on round 1, the first whose rho at the top is not the spec's own quotient."""
    mu, mu_star, out = spec.mu, spec.mu_star, []
    for i in range(spec.rounds):
        before = (mu, mu_star)
        rec, mu, mu_star = MM.float_round(i, mu, mu_star, spec, T, M, key, **(doctor if i == 1 else {}))
        out.append((before, rec))
    return out


@pytest.mark.parametrize("key", [3, 4])
def test_the_model_passes_the_references_round_and_refuses_the_doctored_ones(key):
    tally = Tally("float64")
    for i, ((mu, mu_star), rec) in enumerate(_chain(SPEC, key)):
        _, _, _, end = MM.check_round(tally, rec, i, mu, mu_star, SPEC, T, M, key)
        assert end == "done"
    assert not tally.fail, tally.fail
    for doctor, what in ((dict(old_rho_after_mu=True), "rho_delta_log_G"), (dict(rho_draw_with_old_mu=True), "beta")):
        tally = Tally("doctored")
        (mu, mu_star), rec = _chain(SPEC, key, **doctor)[1]
        MM.check_round(tally, rec, 1, mu, mu_star, SPEC, T, M, key)
        assert tally.fail and any(what in f for f in tally.fail), (doctor, tally.fail)


def test_the_model_follows_the_switches_and_the_skipped_and_degenerate_steps():
    tally = Tally("float64")
    off = d.MpoxSpec(mu=1e-3, mu_star=0.0, do_mu=False, rounds=1)
    rec, mu, mu_star = MM.float_round(0, 1e-3, 0.0, off, T, M, 5)
    assert mu == 1e-3 and rec["mu_done"] == 0 and rec["rho_done"] == 1 and mu_star > 0.0
    assert MM.check_round(tally, rec, 0, 1e-3, 0.0, off, T, M, 5)[:2] == (mu, mu_star)
    T0 = T.copy(); T0[1, 1] = T0[1, 2] = 0.0                             # Ttwiddle* = 0: the rho step does not run
    rec, mu, mu_star = MM.float_round(0, 1e-3, 2e-3, SPEC, T0, M, 5)
    assert mu_star == 2e-3 and mu != 1e-3 and MM.check_round(tally, rec, 0, 1e-3, 2e-3, SPEC, T0, M, 5)[3] == "skipped"
    Tbig = T.copy(); Tbig[1, 1] = Tbig[1, 2] = 1.2e6                     # mu Ttwiddle* / 3 = 800 with M* = 0: Q(1, 800) = exp(-800) underflows
    M0 = M.copy(); M0[1, 1, 3] = M0[1, 2, 0] = 0
    rec, mu, mu_star = MM.float_round(0, 1e-3, 2e-3, off, Tbig, M0, 5)
    assert rec["beta"] == 800.0 and rec["Q_hi"] == 0.0 and rec["rho_degenerate"] == 1 and mu_star == 2e-3
    assert MM.check_round(tally, rec, 0, 1e-3, 2e-3, off, Tbig, M0, 5)[3] == "degenerate"
    assert not tally.fail, tally.fail


def test_the_restated_sampler_starts_where_it_is_told_and_takes_at_most_193_words():
    import skygrid_streams as RS
    for shape in (0.5, 1.0, 40.0, 1e5):
        a, n = MM.gamma_draw_at(9, MM.ID_MU, shape, 3.0, 0)
        assert a == pytest.approx(float(RS.gamma_draw(np.uint64(9), MM.ID_MU, shape, 3.0)[0]), rel=1e-14) and 3 <= n <= 193
        b, _ = MM.gamma_draw_at(9, MM.ID_MU, shape, 3.0, 256)
        assert b != a and b > 0.0
