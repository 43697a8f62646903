"""tests/subst_moves_model.py against the model's own definitions: the q it derives is a rate matrix of the HKY family, and the delta log G
it forms from the exact sufficient statistics is the difference of exact_model's whole-tree log G under the two models -- the statistics ARE
sufficient.  No GPU."""
from fractions import Fraction as F

import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import subst_moves_model as SM
from delphy_amd.scenarios import KAPPA, PI

MODELS = [(1.0, (0.25, 0.25, 0.25, 0.25)), (2.5, (0.1, 0.2, 0.3, 0.4)), (0.3, (0.7, 0.1, 0.15, 0.05)), (5e-324, (0.4, 0.3, 0.2, 0.1)), (1e6, (0.01, 0.01, 0.97, 0.01))]


@pytest.mark.parametrize("kappa,pi", MODELS)
def test_q_is_a_normalised_reversible_rate_matrix(kappa, pi):
    q = SM.hky_q(kappa, pi)
    p = [F(x) for x in pi]
    for a in range(4):
        assert sum(q[a]) == 0                                             # every row sums to 0
        for b in range(4):
            assert p[a] * q[a][b] == p[b] * q[b][a]                       # detailed balance
            if a != b:
                assert q[a][b] >= 0
    assert sum(p[a] * -q[a][a] for a in range(4)) == 1                    # one substitution per unit of mu t
    # transitions over transversions: kappa
    assert q[0][2] * p[1] == F(kappa) * q[0][1] * p[2] and q[1][3] * p[0] == F(kappa) * q[1][0] * p[3]


@pytest.mark.parametrize("kappa,pi", MODELS[:3])
def test_q_is_what_the_engines_are_handed(kappa, pi):
    """hky_q_matrix (the Python mirror of the run driver's arithmetic) within N_Q roundings of the exact entries."""
    q = SM.hky_q(kappa, pi)
    got = d.hky_q_matrix(kappa, pi)
    for a in range(4):
        for b in range(4):
            assert abs(F(float(got[a][b])) - q[a][b]) <= SM.N_Q * X.U * abs(q[a][b]), (a, b)


def _scenario(P):
    """A 16-tip tree with missing data and about a hundred mutations; P = 2: interleaved site partitions; every site its own nu_l."""
    from types import SimpleNamespace
    par = d.SynthParams(num_tips=16, num_sites=240, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=3e-2 / 365.0, gaps_per_tip=2, mean_gap_len=6.0, seed=77)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, _ = d.make_synthetic_emat(par)
    sc = SimpleNamespace(tree=tree, ref=ref, num_sites=240)
    L = sc.num_sites
    rng = np.random.default_rng(5)
    nu = rng.gamma(2.0, 0.5, L)
    pfs = (np.arange(L) * 7 // 3) % P
    return sc, nu, pfs


def _evo(sc, nu, pfs, P, mu, kappa, pi):
    q = d.hky_q_matrix(kappa, pi)
    return X.Evo([mu] * P, [pi] * P, [q] * P, nu, pfs), q


def _whole_tree_log_G(sc, evo):
    return X.Derived(sc.tree, sc.ref, evo).part_log_G(True)


CHANGES = [("mu", (1e-3, 2.0, (0.1, 0.2, 0.3, 0.4)), (1.7e-3, 2.0, (0.1, 0.2, 0.3, 0.4))),
           ("kappa", (1e-3, 2.0, (0.1, 0.2, 0.3, 0.4)), (1e-3, 2.0 * 0.83, (0.1, 0.2, 0.3, 0.4))),
           ("pi", (1e-3, 2.0, (0.1, 0.2, 0.3, 0.4)), (1e-3, 2.0, (0.1 + 0.0075, 0.2, 0.3 - 0.0075, 0.4)))]


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("change", CHANGES, ids=lambda c: c[0])
def test_delta_log_G_from_the_statistics_is_the_difference_of_the_whole_trees_log_G(P, change):
    what, (mu0, k0, pi0), (mu1, k1, pi1) = change
    sc, nu, pfs = _scenario(P)
    e0, q0 = _evo(sc, nu, pfs, P, mu0, k0, pi0)
    e1, q1 = _evo(sc, nu, pfs, P, mu1, k1, pi1)
    st = X.stats(sc.tree, sc.ref, e0)
    assert st["num_muts"] > 20
    T = [[st["Ttwiddle_beta_a"][p][a].value for a in range(4)] for p in range(P)]      # the EXACT statistics (Fractions)
    M = st["num_muts_beta_ab"]
    Cn = np.sum(np.asarray(X.Derived(sc.tree, sc.ref, e0).root_state_counts()), axis=0)
    whole = _whole_tree_log_G(sc, e1).value - _whole_tree_log_G(sc, e0).value
    if what == "mu":
        got, _ = SM.mu_deltas(mu0, mu1, k0, pi0, T, M, 1.0, 0.0, q=q0)
    else:
        got = SM.delta_log_G(mu0, k0, pi0, k1, pi1, T, M, Cn, root_term=what == "pi", q_old=q0, q_new=q1)
    # both sides are exact rationals of the same float64 inputs up to mpmath's 60 digits in a few dozen logs
    assert abs(got.value - whole) < F(1, 10 ** 45) * max(1, abs(whole)), (what, P, float(got.value), float(whole))
    assert abs(float(whole)) > 1e-3                                       # (the change is no fixed point)


def test_a_count_against_a_zero_rate_forces_the_rejection_and_a_zero_count_does_not():
    T = [[1.0, 2.0, 3.0, 4.0]]
    M = np.zeros((1, 4, 4), np.int64); M[0, 0, 1] = 3                     # a transversion only
    zero_kappa = SM.delta_log_G(1e-3, 2.0, (0.1, 0.2, 0.3, 0.4), F(0), (0.1, 0.2, 0.3, 0.4), T, M, [1, 1, 1, 1], root_term=False)
    assert zero_kappa is not None and zero_kappa.value != 0               # no transition was counted: q_ts = 0 multiplies a count of 0
    M[0, 0, 2] = 1
    assert SM.delta_log_G(1e-3, 2.0, (0.1, 0.2, 0.3, 0.4), F(0), (0.1, 0.2, 0.3, 0.4), T, M, [1, 1, 1, 1], root_term=False) is None


# ---- the keys the device tests use: the model alone, on the CPU -----------------------------------------------------------------
def _float_q(kappa, pi):
    r = [[0.0 if a == b else (kappa if (a ^ b) == 2 else 1.0) for b in range(4)] for a in range(4)]
    R = sum(pi[a] * r[a][b] * pi[b] for a in range(4) for b in range(4))
    q = [[r[a][b] / R * pi[b] for b in range(4)] for a in range(4)]
    for a in range(4):
        q[a][a] = -sum(q[a][b] for b in range(4) if b != a)
    return q


def _float_chain(spec, T, M, C, key):
    """The whole call in float64 on the CPU -- the mu draw from the restated stream, then every step from the state the steps before it left -- as
    (decisions made, decisions whose u lies within 1e-12 relative of exp(log_metropolis))."""
    import math
    import skygrid_streams as RS
    from test_subst_moves_gpu import ID_MU, _words
    P = len(T)
    Ta = [sum(float(T[p][a]) for p in range(P)) for a in range(4)]
    Mab = [[sum(int(M[p][a][b]) for p in range(P)) for b in range(4)] for a in range(4)]
    kappa, pi, mu = float(spec.kappa), [float(v) for v in spec.pi], float(spec.mu)
    q = _float_q(kappa, pi)
    if spec.do_mu:
        nm = sum(Mab[a][b] for a in range(4) for b in range(4) if a != b)
        mu = float(RS.gamma_draw(np.uint64(key), ID_MU, nm + spec.mu_prior_alpha, sum(-q[a][a] * Ta[a] for a in range(4)) + spec.mu_prior_beta)[0])
    made = close = 0
    for s in range(2 * spec.rounds):
        u = _words(key, s)
        if s % 2 == 0:
            if not spec.do_pi:
                continue
            d_ = 0.01 * u[0]; ia = int(4.0 * u[1]); ib = (ia + 1 + int(3.0 * u[2])) % 4
            pn = list(pi); pn[ia] += d_; pn[ib] -= d_
            if not (0.0 < pn[ia] < 1.0 and 0.0 < pn[ib] < 1.0):
                continue
            kn, uu, extra = kappa, u[3], 0.0
        else:
            if not spec.do_kappa:
                continue
            kn, pn, uu = kappa * (0.75 + (1 / 0.75 - 0.75) * u[0]), pi, u[1]
            extra = (-(math.log(kn) - 1.0) ** 2 + (math.log(kappa) - 1.0) ** 2) / (2 * 1.25 ** 2) + 2.0 * math.log(kappa / kn)
        qn = _float_q(kn, pn)
        if any(a != b and Mab[a][b] > 0 and qn[a][b] == 0 for a in range(4) for b in range(4)):
            continue
        lm = extra - sum(mu * (-qn[a][a] + q[a][a]) * Ta[a] for a in range(4))
        if s % 2 == 0:
            lm += sum(int(C[a]) * math.log(pn[a] / pi[a]) for a in range(4) if C[a] > 0)
        lm += sum(Mab[a][b] * math.log(qn[a][b] / q[a][b]) for a in range(4) for b in range(4) if a != b and Mab[a][b] > 0)
        e = math.exp(min(lm, 700.0))
        made += 1
        close += abs(uu - e) <= 1e-12 * e
        if lm > 0 or uu < e:
            kappa, pi, q = kn, pn, qn
    return made, close


def test_the_keys_of_the_device_tests_leave_no_decision_too_close_to_call():
    """Every call the device tests hold to the model step by step, run whole on the CPU in float64: at most 1 decision in 100 may lie within 1e-12
    relative of its threshold (the device tests set such a step aside and count it); at these keys none does."""
    import test_subst_moves_gpu as G
    made = close = 0
    for _, spec, T, M, C in G.CASES:
        for key in G.CASE_KEYS + G.LAST_KEYS:
            a, b = _float_chain(spec, T, M, C, key); made += a; close += b
    for key in G.P2_KEYS:
        a, b = _float_chain(G.SPEC, G.T2, G.M2, G.C1, key); made += a; close += b
    assert made >= 200 and close * 100 <= made, (made, close)
    assert close == 0
