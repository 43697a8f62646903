"""The Skygrid population moves on the device (emat_skygrid_moves, emat_debug_pop_gradient) against tests/skygrid_moves_model.py.

Every number a round reports is held to (n + 8) u S of the exact model evaluated FROM THE DEVICE'S OWN STATE BEFORE IT (its draws, and
the gammas and momenta of its trace): a trajectory is never compared end to end, because 25 steps amplify a last-bit difference.  The
force also gets the truncation of the reference's series branch, 3e-11 of each piece with |Delta| < 1e-5 (skygrid_moves_model's
docstring).  The two update lines of a leapfrog step are checked for every step and every knot; in the larger cases the exact FORCE is evaluated for a handful
of knots (both ends, the adversarial gammas, a spread) at the first and last step: Fractions at 60 digits cost milliseconds per knot interval.
Then the draws (KS over 2 000 fixed keys, each first shown on the CPU to pass at those keys) and the sampler as a whole against a
numpy quadrature of the posterior."""
import dataclasses
import math
from fractions import Fraction as F

import numpy as np
import pytest
import scipy.special as ssp
import scipy.stats as sst

import delphy_amd as d
import exact_model as X
import skygrid_moves_model as SM
import skygrid_streams as RS
from exact_model import Exact
from test_exact_model import Tally

pytestmark = pytest.mark.gpu

KS_P = 1e-6          # the project's convention


@pytest.fixture(scope="module")
def backend():
    b = d.EmatBackend(10)
    yield b
    b.close()


def _moves(b, case, key, trace=True, **spec_kw):
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    spec = dataclasses.replace(spec, **spec_kw)
    return b.skygrid_moves(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, key=key, trace=trace), spec


def _fsum(values) -> Exact:
    """A sum of float64 numbers the device added: exact value, S = the sum of the magnitudes."""
    fr = [F(float(v)) for v in values]
    return Exact(sum(fr, F(0)), sum((abs(v) for v in fr), F(0)), len(fr))


def _knots_to_check(n, limit):
    if n <= limit:
        return list(range(n))
    return sorted(set([0, 1, 2, 3, 4, 6, 8, 10, 11, n - 2, n - 1] + list(np.linspace(12, n - 3, max(1, limit - 11)).astype(int))))


def check_round(b, tally: Tally, case, key, knots_limit=16, steps="all", **spec_kw):
    """One call, every reported number against the model from the device's own state before it."""
    name, pm, _, t_ref, t_step, first_cell, k_bar, inner_t = case
    r, spec = _moves(b, case, key, **spec_kw)
    n, ni = pm.skygrid_x.shape[0], len(inner_t)
    where = "%s key %d" % (name, key)
    grid = SM.Grid(t_ref, t_step, first_cell, k_bar)
    pop0 = X.Pop(pm)
    ns = SM.NodeStats(pop0, inner_t); c = ns.c
    tally.equal("c_k", r.c_k, np.array(c, float), where)
    for k in range(n):
        tally.check("W_k", ns.W_exact(k), r.W_k[k], "%s knot %d" % (where, k))
    tally.check("log_coalescent_prior_start", SM.log_coalescent_prior(pop0, grid, ns), r.log_coalescent_prior_start, where)
    # tau
    pa, pb = SM.tau_posterior(pm.skygrid_gamma, spec.tau_prior_alpha, spec.tau_prior_beta)
    tally.check("tau_post_alpha", pa, r.tau_post_alpha, where); tally.check("tau_post_beta", pb, r.tau_post_beta, where)
    ran_tau = bool(spec.do_tau and spec.tau_move_enabled)
    assert r.tau == (r.tau_draw if ran_tau else spec.tau) and r.tau_draw > 0
    d_tau = SM.tau_delta_log_prior(r.tau_post_alpha, r.tau_post_beta, r.tau_draw, spec.tau) if ran_tau else Exact(F(0), F(0), 0)
    tally.check("tau_delta_log_prior", d_tau, r.tau_delta_log_prior, where)
    # zero mode
    g0 = pm.skygrid_gamma
    B = SM.zero_mode_B(pop0, grid)
    tally.check("zero_B", B, r.zero_B, where)
    assert r.zero_shape == ni + spec.inv_nbar_prior_alpha
    tally.check("zero_rate", _fsum([r.zero_B, spec.inv_nbar_prior_beta]), r.zero_rate, where)
    gbar = sum((F(float(v)) for v in g0), F(0)) / n
    lgI = X._log(F(r.zero_I_bar))
    tally.check("zero_delta_gamma_bar", Exact(-gbar - lgI, sum((abs(F(float(v))) for v in g0), F(0)) / n * (n + 2) + abs(lgI) + 2, n + 4), r.zero_delta_gamma_bar, where)
    g_new = g0 + r.zero_delta_gamma_bar                   # the device's own line (run.cpp:2125), one rounding per knot
    ob, nb = SM.log_prior_bound(g0, spec), SM.log_prior_bound(g_new, spec)
    tally.check("zero_log_metropolis", Exact(nb.value - ob.value, nb.S + ob.S, nb.n + ob.n), r.zero_log_metropolis, where)
    assert 0.0 <= r.zero_u < 1.0 and r.zero_u == float(RS.to_co(RS.word(np.uint64(key), RS.ID_ZERO_U, 0)))
    want_zero = bool(spec.do_zero_mode) and (r.zero_log_metropolis >= 0 or r.zero_u < math.exp(r.zero_log_metropolis))
    assert r.zero_accepted == int(want_zero), where
    g1 = g_new if r.zero_accepted else g0
    tally.equal("gamma after the zero mode", r.gamma_hmc_start, g1, where)
    pop1 = X.Pop(SM.with_gamma(pm, g1))
    d_zero = Exact(F(0), F(0), 0)
    if r.zero_accepted:
        a_, b_ = F(spec.inv_nbar_prior_alpha), F(spec.inv_nbar_prior_beta)
        gb1 = sum((F(float(v)) for v in g1), F(0)) / n
        e0, e1 = X._exp(-gbar), X._exp(-gb1)
        v = (-a_ * gb1 - b_ * e1) - (-a_ * gbar - b_ * e0) + (nb.value - ob.value)
        S = abs(a_) * (abs(gb1) + abs(gbar)) * (n + 2) + abs(b_) * (e0 * (2 + abs(gbar) * (n + 2)) + e1 * (2 + abs(gb1) * (n + 2))) + nb.S + ob.S
        d_zero = Exact(v, S, 2 * n + nb.n + ob.n + 8)
    # HMC: masses, energies at the start
    tau = r.tau
    for k, mk in enumerate(SM.masses(c, tau)):
        tally.check("m_k", mk, r.m_k[k], "%s knot %d" % (where, k))
    assert r.hmc_dt >= 0 and r.hmc_dt == pytest.approx(float(-spec.hmc_mean_dt * np.log(RS.to_oc(RS.word(np.uint64(key), RS.ID_DT, 0)))), rel=1e-14)
    assert r.hmc_u == float(RS.to_co(RS.word(np.uint64(key), RS.ID_HMC_U, 0)))
    prior1 = SM.log_coalescent_prior(pop1, grid, ns)
    tally.check("hmc_K_old", SM.kinetic(r.p_initial, r.m_k), r.hmc_K_old, where)
    tally.check("hmc_U_prior_old", SM.U_prior(g1, tau, spec), r.hmc_U_prior_old, where)
    tally.check("hmc_U_coal_old", Exact(-prior1.value, prior1.S, prior1.n), r.hmc_U_coal_old, where)
    K_limit = 100.0 * n
    made = r.hmc_steps_done
    ks = _knots_to_check(n, knots_limit)
    which = set(range(made)) if steps == "all" else {0, made - 1} & set(range(made))
    for s in range(made):                                     # the two update lines: every step, every knot; the exact force: `which` x `ks`
        g_before = r.gamma_hmc_start if s == 0 else r.gamma_after[s - 1]
        p_before = r.p_initial if s == 0 else r.p[s - 1]
        ended_here = r.hmc_K_exit_step == s + 1
        for k in range(n):
            w = "%s step %d knot %d" % (where, s, k)
            tally.check("gamma half step", SM.half_step(g_before[k], r.hmc_dt, p_before[k], r.m_k[k]), r.gamma_half[s][k], w)
            tally.check("p_k", SM.momentum_step(p_before[k], r.hmc_dt, r.f[s][k]), r.p[s][k], w)
            if not ended_here:
                tally.check("gamma after the step", SM.half_step(r.gamma_half[s][k], r.hmc_dt, r.p[s][k], r.m_k[k]), r.gamma_after[s][k], w)
        if s in which:
            pop_half = X.Pop(SM.with_gamma(pm, r.gamma_half[s]))
            for k, (fk, allow) in zip(ks, SM.force(pop_half, grid, ns, tau, spec, knots=ks)):
                tally.check("f_k", fk, r.f[s][k], "%s step %d knot %d" % (where, s, k), allowance=allow)
        K_s = float(SM.kinetic(r.p[s], r.m_k).value)
        if abs(K_s - K_limit) > 1e-9 * K_limit:           # away from the threshold the exit is decided
            assert (r.hmc_K_exit_step == s + 1) == (K_s > K_limit), where
    d_hmc = Exact(F(0), F(0), 0)
    if not spec.do_hmc:
        assert made == 0 and r.hmc_accepted == 0 and r.hmc_K_exit_step == -1
    elif r.hmc_K_exit_step >= 0:
        assert r.hmc_accepted == 0 and made == r.hmc_K_exit_step and not r.hmc_nan
    else:
        assert made == spec.hmc_steps
        g_end = r.gamma_after[-1] if made else r.gamma_hmc_start
        p_end = r.p[-1] if made else r.p_initial
        prior2 = SM.log_coalescent_prior(X.Pop(SM.with_gamma(pm, g_end)), grid, ns)
        tally.check("hmc_K_new", SM.kinetic(p_end, r.m_k), r.hmc_K_new, where)
        tally.check("hmc_U_prior_new", SM.U_prior(g_end, tau, spec), r.hmc_U_prior_new, where)
        tally.check("hmc_U_coal_new", Exact(-prior2.value, prior2.S, prior2.n), r.hmc_U_coal_new, where)
        H = _fsum([r.hmc_K_old, r.hmc_U_prior_old, r.hmc_U_coal_old, -r.hmc_K_new, -r.hmc_U_prior_new, -r.hmc_U_coal_new])
        tally.check("hmc_log_metropolis", H, r.hmc_log_metropolis, where)
        assert not r.hmc_nan
        assert r.hmc_accepted == int(r.hmc_log_metropolis > 0 or r.hmc_u < math.exp(r.hmc_log_metropolis)), where
        if r.hmc_accepted:
            d_hmc = _fsum([-r.hmc_U_prior_new, r.hmc_U_prior_old])
    g_out = r.gamma_after[-1] if r.hmc_accepted and made else r.gamma_hmc_start
    tally.equal("gamma returned", r.gamma, g_out, where)
    assert r.log_coalescent_prior_end == (-r.hmc_U_coal_new if r.hmc_accepted else -r.hmc_U_coal_old), where
    total = Exact(d_tau.value + d_zero.value + d_hmc.value, d_tau.S + d_zero.S + d_hmc.S + abs(d_tau.value) + abs(d_zero.value) + abs(d_hmc.value), d_tau.n + d_zero.n + d_hmc.n + 3)
    tally.check("delta_log_other_priors", total, r.delta_log_other_priors, where)
    return r


SMALL = [("2 knots, 1 cell, 1 node", 2, 1, 1, "finer"), ("3 knots, 63 cells, 63 nodes", 3, 63, 63, "coarser"), ("12 knots, 9 cells", 12, 9, 7, "finer"),
         ("grid before x_0", 3, 8, 4, "before"), ("grid after x_M", 3, 8, 4, "after"), ("times on knots and cell bounds", 5, 16, 9, "on"),
         ("dozens of knots a cell", 40, 1, 3, "finer")]


@pytest.mark.parametrize("log_linear", [False, True], ids=["staircase", "log-linear"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: s[0])
def test_small_rounds_every_step_and_every_knot(backend, shape, log_linear, record_property):
    name, nk, nc, ni, layout = shape
    tally = Tally("device")
    case = SM.make_case(name, nk, nc, ni, log_linear, layout=layout)
    check_round(backend, tally, case, key=11, knots_limit=64, hmc_steps=6)
    check_round(backend, tally, case, key=12, knots_limit=64, hmc_steps=2, low_gamma_barrier_enabled=False, tau_move_enabled=False, inv_nbar_prior_alpha=0.0, inv_nbar_prior_beta=0.0)
    tally.finish(record_property)


LARGE = [("64 knots, 65 cells, 1025 nodes", 64, 65, 1025, "finer"), ("65 knots, 1025 cells, 5000 nodes", 65, 1025, 5000, "coarser"),
         ("300 knots, 63 cells, 63 nodes", 300, 63, 63, "finer"), ("1024 knots, 65 cells, 1025 nodes", 1024, 65, 1025, "finer"),
         ("1024 knots, 1 cell", 1024, 1, 63, "finer"), ("2 knots, 1025 cells", 2, 1025, 63, "coarser")]


@pytest.mark.parametrize("log_linear", [False, True], ids=["staircase", "log-linear"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: s[0])
def test_large_rounds_first_and_last_step_on_a_handful_of_knots(backend, shape, log_linear, record_property):
    name, nk, nc, ni, layout = shape
    tally = Tally("device")
    case = SM.make_case(name, nk, nc, ni, log_linear, layout=layout)
    check_round(backend, tally, case, key=21, knots_limit=14, steps="ends", hmc_steps=25)
    tally.finish(record_property)


def test_1025_knots_are_refused(backend):
    with pytest.raises(d.EmatError, match="CAPACITY.*1025 knots"):
        _moves(backend, SM.make_case("", 1025, 8, 5, True), key=1)


def test_same_arguments_same_bits_in_every_call_and_on_every_handle(backend):
    case = SM.make_case("", 64, 65, 1025, True)
    r1, _ = _moves(backend, case, key=77)
    r2, _ = _moves(backend, case, key=77)
    other = d.EmatBackend(20)
    try:
        r3, _ = _moves(other, case, key=77)
    finally:
        other.close()
    for r in (r2, r3):
        assert np.array_equal(r1.gamma, r.gamma) and np.array_equal(r1.trace, r.trace, equal_nan=True)
        for f in ("tau", "log_coalescent_prior_start", "log_coalescent_prior_end", "delta_log_other_priors", "zero_B", "zero_I_bar", "hmc_log_metropolis", "hmc_K_new", "hmc_accepted"):
            assert getattr(r1, f) == getattr(r, f), f
    r4, _ = _moves(backend, case, key=78)
    assert not np.array_equal(r1.p_initial, r4.p_initial) and r1.tau_draw != r4.tau_draw


def test_the_gradient_hook_meets_the_references_expectations(backend):
    import json, os
    G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skygrid_gradient_expectations.json")))
    for name, m in G["models"].items():
        pm = d.PopModel.skygrid(G["knots_x"], G["knots_gamma"], name == "log_linear")
        for k in range(4):
            es = [e for e in m["d_log_N_d_gamma"] if e["k"] == k]
            got = backend.debug_pop_gradient(pm, 4, k, [e["t"] for e in es], [e["t"] for e in es])
            assert all(abs(g - e["expected"]) <= e["tol"] for g, e in zip(got, es)), (name, k, got)
            es = [e for e in m["d_log_int_N_d_gamma"] if e["k"] == k]
            got = backend.debug_pop_gradient(pm, 3, k, [e["a"] for e in es], [e["b"] for e in es])
            assert all(abs(g - e["expected"]) <= e["tol"] for g, e in zip(got, es)), (name, k, got)


def test_the_gradient_hook_against_the_model_on_adversarial_grids(backend, record_property):
    """Op 3 and op 4 over adversarial_pop_cases()'s Skygrid grids, every knot, plus gammas either side of the series branch."""
    tally = Tally("device")
    cases = [(nm, pm, a, bb) for nm, pm, a, bb in X.adversarial_pop_cases() if pm.kind == 2]
    assert len(cases) == 2
    nm, pm, a, bb = cases[1]
    g = pm.skygrid_gamma.copy(); g[1] = g[0] + 0.9e-5; g[3] = g[2] - 1.1e-5; g[5] = g[4] + 1.1e-5
    cases.append((nm + " at the series branch", d.PopModel.skygrid(pm.skygrid_x, g, True), a, bb))
    for nm, pm, a, bb in cases:
        keep = a < bb                                      # (a == b is 0 / 0 in the reference too)
        a, bb = a[keep][::3], bb[keep][::3]
        pop = X.Pop(pm)
        for k in range(pm.skygrid_x.shape[0]):
            got = backend.debug_pop_gradient(pm, 3, k, a, bb)
            at = backend.debug_pop_gradient(pm, 4, k, a, a)
            for i in range(a.shape[0]):
                ex, allow = SM.d_log_int_N_d_gamma(pop, float(a[i]), float(bb[i]), k)
                tally.check("d_log_int_N_d_gamma", ex, got[i], "%s knot %d [%r, %r]" % (nm, k, a[i], bb[i]), allowance=allow)
                v = SM.d_log_N_d_gamma(pop, float(a[i]), k)
                tally.check("d_log_N_d_gamma", Exact(v, 3 * abs(v) + (1 if 0 < v < 1 else 0), 3), at[i], "%s knot %d t=%r" % (nm, k, a[i]))
    tally.finish(record_property)


# ---- forced branches ---------------------------------------------------------------------------------------------------------
def test_exploding_momenta_take_the_references_exit_and_leave_gamma_and_tau_alone(backend):
    """A huge hmc_mean_dt (100: dt = 22 at this key, against 0.06 in the reference) puts K above 100 (M + 1) at the first momentum
    step (run.cpp:1940-1947) while every exponential stays finite.  The initial check (:1868) cannot be reached through dt -- K_old is a
    sum of (M + 1) squared normals over 2, whatever the masses -- so the rule is shown where it can act, and K_old is asserted below it."""
    case = SM.make_case("", 12, 9, 7, True)
    pm = case[1]
    r, spec = _moves(backend, case, key=5, hmc_mean_dt=100.0, do_tau=False, do_zero_mode=False)
    print("dt", r.hmc_dt, "K_old", r.hmc_K_old, "exit", r.hmc_K_exit_step, "steps", r.hmc_steps_done, "nan", r.hmc_nan, "p", r.p[:1], "f", r.f[:1])
    assert 20.0 < r.hmc_dt < 25.0 and np.all(np.isfinite(r.p[0])) and np.all(np.isfinite(r.f[0]))
    assert r.hmc_K_exit_step == 1 and r.hmc_steps_done == 1 and r.hmc_accepted == 0 and not r.hmc_nan
    assert float(SM.kinetic(r.p[0], r.m_k).value) > 100.0 * 12 >= r.hmc_K_old
    assert np.array_equal(r.gamma, pm.skygrid_gamma) and r.tau == spec.tau and r.delta_log_other_priors == 0.0
    assert r.log_coalescent_prior_end == r.log_coalescent_prior_start == -r.hmc_U_coal_old
    # ... and with the other two moves on, what THEY did stays
    r, spec = _moves(backend, case, key=5, hmc_mean_dt=100.0)
    assert r.hmc_K_exit_step == 1 and r.hmc_accepted == 0 and np.array_equal(r.gamma, r.gamma_hmc_start) and r.tau == r.tau_draw
    assert r.log_coalescent_prior_end == -r.hmc_U_coal_old
    # the NaN exit (run.cpp:1981-1989): a dt of 2e5 overflows the exponentials at the first half step, the forces become inf - inf, K is NaN and so
    # never above the bound; the trajectory runs all its steps and the NaN check rejects it, with nothing touched
    r, spec = _moves(backend, case, key=5, hmc_mean_dt=1e6, do_tau=False, do_zero_mode=False)
    print("dt", r.hmc_dt, "exit", r.hmc_K_exit_step, "steps", r.hmc_steps_done, "nan", r.hmc_nan)
    assert r.hmc_nan == 1 and r.hmc_K_exit_step == -1 and r.hmc_steps_done == spec.hmc_steps and r.hmc_accepted == 0
    assert np.isnan(r.hmc_log_metropolis) or np.any(np.isnan(r.gamma_after[-1]))
    assert np.array_equal(r.gamma, pm.skygrid_gamma) and r.tau == spec.tau and r.delta_log_other_priors == 0.0
    assert r.log_coalescent_prior_end == r.log_coalescent_prior_start


def test_a_key_whose_uniform_rejects(backend):
    """Keys found on the CPU (skygrid_streams: the same Philox streams) whose HMC uniform is above 0.999: whenever the trajectory's log
    Metropolis ratio is negative and not tiny the move must be rejected and gamma left as the zero mode left it."""
    keys = np.arange(1, 200001, dtype=np.uint64)
    u = RS.to_co(RS.word(keys, RS.ID_HMC_U, 0))
    picked = [int(k) for k in keys[u > 0.999][:8]]
    assert len(picked) == 8
    case = SM.make_case("", 64, 65, 1025, True)
    rejected = 0
    for key in picked:
        r, _ = _moves(backend, case, key=key, hmc_mean_dt=0.15)
        assert r.hmc_u == float(u[key - 1]) > 0.999
        assert r.hmc_accepted == int(r.hmc_K_exit_step < 0 and (r.hmc_log_metropolis > 0 or r.hmc_u < math.exp(r.hmc_log_metropolis)))
        if r.hmc_K_exit_step < 0 and -50.0 < r.hmc_log_metropolis < math.log(0.999):
            rejected += 1
            assert r.hmc_accepted == 0 and np.array_equal(r.gamma, r.gamma_hmc_start) and r.log_coalescent_prior_end == -r.hmc_U_coal_old
    assert rejected >= 1


# ---- the draws ---------------------------------------------------------------------------------------------------------------
KEYS = np.arange(1000, 3000, dtype=np.uint64)


def _ks(x, cdf):
    return sst.kstest(np.asarray(x, float), cdf).pvalue


def test_the_scalar_streams_pass_on_the_cpu_at_the_fixed_keys():
    """The reference distributions themselves at KEYS, from the CPU restatement of the streams: a failure here is the keys', not the device's."""
    assert _ks(RS.to_co(RS.word(KEYS, RS.ID_ZERO_U, 0)), "uniform") > KS_P and _ks(RS.to_co(RS.word(KEYS, RS.ID_HMC_U, 0)), "uniform") > KS_P
    assert _ks(-np.log(RS.to_oc(RS.word(KEYS, RS.ID_DT, 0))), "expon") > KS_P
    for k in (0, 1, 11):
        assert _ks(RS.normal(KEYS, k), "norm") > KS_P
    for shape, rate in ((0.501, 0.7), (6.2, 3.3), (1.0 + 0.4, 2.0), (63.4, 17.0), (100000.4, 5.0e4)):
        for sid in (RS.ID_TAU, RS.ID_I_BAR):
            assert _ks(RS.gamma_draw(KEYS, sid, shape, rate), sst.gamma(shape, scale=1.0 / rate).cdf) > KS_P, (shape, sid)


@pytest.mark.parametrize("num_inner", [1, 63, 100000])
def test_the_devices_draws_follow_their_distributions(backend, num_inner):
    """tau ~ Gamma(post_alpha, rate post_beta), I_bar ~ Gamma(N_inner + alpha, rate B + beta), dt exponential, p_k / sqrt(m_k) normal,
    both uniforms uniform: over KEYS, no leapfrog steps (the draws are made whether needed or not)."""
    case = SM.make_case("", 12, 9, num_inner, True, inv_nbar_prior_alpha=0.4, inv_nbar_prior_beta=1.7)
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    spec = dataclasses.replace(spec, hmc_steps=0, do_tau=False, do_zero_mode=False)
    tau, I_bar, dt, zu, hu, z = [], [], [], [], [], []
    for key in KEYS:
        r = backend.skygrid_moves(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, key=int(key), trace=True)
        tau.append(r.tau_draw); I_bar.append(r.zero_I_bar); dt.append(r.hmc_dt); zu.append(r.zero_u); hu.append(r.hmc_u); z.append(r.p_initial / np.sqrt(r.m_k))
    assert r.zero_shape == num_inner + 0.4
    assert _ks(tau, sst.gamma(r.tau_post_alpha, scale=1.0 / r.tau_post_beta).cdf) > KS_P
    assert _ks(I_bar, sst.gamma(r.zero_shape, scale=1.0 / r.zero_rate).cdf) > KS_P
    assert _ks(np.array(dt) / spec.hmc_mean_dt, "expon") > KS_P
    assert _ks(zu, "uniform") > KS_P and _ks(hu, "uniform") > KS_P
    z = np.array(z)
    for k in (0, 1, 11):
        assert _ks(z[:, k], "norm") > KS_P
    assert _ks(z.reshape(-1), "norm") > KS_P
    # the uniforms are the CPU streams' bit for bit; the device's own log / sqrt / cos may differ from the CPU's in the last bits
    assert np.array_equal(zu, RS.to_co(RS.word(KEYS, RS.ID_ZERO_U, 0))) and np.array_equal(hu, RS.to_co(RS.word(KEYS, RS.ID_HMC_U, 0)))
    assert np.allclose(z[:, 11], RS.normal(KEYS, 11), rtol=0, atol=1e-12)
    assert np.allclose(tau, RS.gamma_draw(KEYS, RS.ID_TAU, r.tau_post_alpha, r.tau_post_beta), rtol=1e-9)


def test_the_tau_draw_below_shape_one(backend):
    """Two knots and the reference's default tau prior (0.001, 0.001): the posterior shape is 0.501, the sampler's boost path."""
    case = SM.make_case("", 2, 8, 5, True, tau_prior_alpha=0.001, tau_prior_beta=0.001)
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    spec = dataclasses.replace(spec, hmc_steps=0)
    tau = []
    for key in KEYS:
        r = backend.skygrid_moves(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, key=int(key))
        tau.append(r.tau_draw)
    assert r.tau_post_alpha == 0.501
    assert _ks(tau, sst.gamma(r.tau_post_alpha, scale=1.0 / r.tau_post_beta).cdf) > KS_P
    assert np.allclose(tau, RS.gamma_draw(KEYS, RS.ID_TAU, r.tau_post_alpha, r.tau_post_beta), rtol=1e-9)


# ---- the sampler as a whole ----------------------------------------------------------------------------------------------------
def _posterior_means(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, npts):
    """E[gamma_0], E[gamma_1], E[log tau] under the posterior the three moves leave invariant, two log-linear knots: float64 numpy quadrature
    over (gamma_0, gamma_1) on an npts x npts grid, tau integrated in closed form (it is Gamma(A, b + ssq / 2) given the gammas)."""
    x0, x1 = pm.skygrid_x
    g = np.linspace(-3.0, 9.0, npts)
    G0, G1 = np.meshgrid(g, g, indexing="ij")
    U = np.zeros_like(G0)
    for c, kc in enumerate(k_bar):
        lo = t_ref + (first_cell + c) * t_step; hi = lo + t_step
        I = np.zeros_like(G0)
        if lo < x0:
            I += np.exp(G0) * (min(hi, x0) - lo)
        if hi > x1:
            I += np.exp(G1) * (hi - max(lo, x1))
        a, b = max(lo, x0), min(hi, x1)
        if b > a:
            Ga = G0 + (G1 - G0) * (a - x0) / (x1 - x0); D = (G1 - G0) * (b - a) / (x1 - x0)
            ratio = np.where(np.abs(D) < 1e-8, 1.0 + 0.5 * D, np.expm1(D) / np.where(D == 0, 1.0, D))
            I += np.exp(Ga) * (b - a) * ratio
        U += t_step * kc * (kc - 1.0) / (2.0 * (I / t_step))
    for t in inner_t:
        cc = min(max((t - x0) / (x1 - x0), 0.0), 1.0)
        U += (1 - cc) * G0 + cc * G1
    for Gk in (G0, G1):
        U += np.where(Gk < spec.low_gamma_barrier_loc, ((spec.low_gamma_barrier_loc - Gk) / spec.low_gamma_barrier_scale) ** 2, 0.0)
    gbar = 0.5 * (G0 + G1)
    U += spec.inv_nbar_prior_alpha * gbar + spec.inv_nbar_prior_beta * np.exp(-gbar)
    A = spec.tau_prior_alpha + 0.5                       # M / 2 with M = 1
    rate = spec.tau_prior_beta + 0.5 * (G1 - G0) ** 2
    logw = -U - A * np.log(rate)
    w = np.exp(logw - logw.max()); w /= w.sum()
    return np.array([(w * G0).sum(), (w * G1).sum(), (w * (ssp.digamma(A) - np.log(rate))).sum()]), w


def test_the_chain_of_4000_rounds_samples_the_posterior(backend, record_property):
    """Two knots, 8 cells, 5 coalescence times, log-linear, barrier and tau move on: 4 000 successive calls, each fed the previous gamma and
    tau; the chain means of gamma_0, gamma_1 and log tau within 4 batch-means standard errors of the quadrature."""
    x = np.array([-1.7, -0.3]); t_ref, t_step, first_cell = 0.0, 0.25, -8
    k_bar = np.array([1.0, 1.6, 2.0, 2.7, 3.4, 4.1, 3.0, 0.9]); inner_t = np.array([-1.9, -1.4, -1.1, -0.7, -0.2])
    spec = d.SkygridSpec(tau=1.0, tau_move_enabled=True, low_gamma_barrier_enabled=True, low_gamma_barrier_loc=0.0, low_gamma_barrier_scale=0.35,
                         tau_prior_alpha=2.0, tau_prior_beta=1.0, inv_nbar_prior_alpha=0.5, inv_nbar_prior_beta=0.5)
    gam = np.array([1.0, 1.0]); n_rounds, n_batches = 4000, 40
    chain = np.zeros((n_rounds, 3)); acc = 0
    for i in range(n_rounds):
        r = backend.skygrid_moves(d.PopModel.skygrid(x, gam, True), spec, t_ref, t_step, first_cell, k_bar, inner_t, key=0x5EED0000 + i)
        gam = r.gamma.copy(); spec = dataclasses.replace(spec, tau=r.tau); acc += r.hmc_accepted
        chain[i] = gam[0], gam[1], math.log(r.tau)
    mean = chain.mean(axis=0)
    se = chain.reshape(n_batches, -1, 3).mean(axis=1).std(axis=0, ddof=1) / math.sqrt(n_batches)
    pm = d.PopModel.skygrid(x, gam, True)
    fine, w = _posterior_means(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, 1201)
    coarse, _ = _posterior_means(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, 601)
    assert np.all(np.abs(fine - coarse) < 0.1 * se), (fine, coarse, se)          # the grid is fine enough ...
    assert w[0].sum() + w[-1].sum() + w[:, 0].sum() + w[:, -1].sum() < 1e-9      # ... and wide enough
    dist = (mean - fine) / se
    record_property("chain_distance_in_standard_errors", [float("%.3g" % v) for v in dist])
    record_property("hmc_acceptance", acc / n_rounds)
    print("chain means", mean, "quadrature", fine, "se", se, "distance / se", dist, "HMC acceptance", acc / n_rounds)
    assert np.all(np.abs(dist) < 4.0), (mean, fine, se, dist)
