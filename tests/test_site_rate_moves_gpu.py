"""The site-rate moves on the device (emat_site_rate_moves, emat_get_nu_l, emat_debug_sample_gamma and the run driver's calls) against
tests/site_rate_model.py and the known conditional distributions: every deterministic number within the model's (n + 8) u S, every
random one against its distribution with a KS threshold of p > 1e-6 at keys fixed here (a correct sampler fails one of the fifteen or so
such tests with probability about 1e-5; with fixed keys a pass stays a pass)."""
import math
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest
from scipy import stats as sst

import delphy_amd as d
import exact_model as X
import site_rate_model as SR
from delphy_amd.engine import hky_q_matrix
from delphy_amd.scenarios import make_scenario, random_scenario

pytestmark = pytest.mark.gpu

KS_P = 1e-6
PI = [0.3, 0.2, 0.2, 0.3]


def _handle(L, nu, mu=(1e-3,), pfs=None, pi=None, q=None, seed=1):
    b = d.EmatBackend(L)
    b.set_ref_sequence(np.random.default_rng(seed).integers(0, 4, L).astype(np.uint8))
    P = len(mu)
    pi = np.asarray([PI] * P if pi is None else pi); q = np.stack([hky_q_matrix(2.0 + p, pi[p]) for p in range(P)]) if q is None else q
    b.set_evo(np.asarray(mu), pi, q, nu, np.zeros(L, np.int32) if pfs is None else pfs)
    return b


def _synthetic(L, seed, mu=1e-3, mean_muts=2.0, all_zero=False):
    """Statistics made here (the engine call takes them as arguments, so no tree is needed): Ttwiddle_l around mean_muts / mu, M_l Poisson
    of a site's own gamma-distributed rate; the old rates are arbitrary positive numbers."""
    rng = np.random.default_rng(seed)
    T = mean_muts / mu * rng.uniform(0.7, 1.3, L)
    true_nu = rng.gamma(0.5, 2.0, L)
    M = np.zeros(L, np.int32) if all_zero else rng.poisson(mu * T * true_nu).astype(np.int32)
    nu_old = 0.2 + 1.8 * rng.random(L)
    return T, M, nu_old


def _chain(res, alpha0):
    """The alpha before every step of the trace and the current log p there, from the trace's own numbers; and the last alpha."""
    tr = res.trace
    last_acc = np.maximum.accumulate(np.where(tr["accepted"] != 0, np.arange(len(tr)), -1))       # the last accepted step up to and including each
    after = np.where(last_acc >= 0, tr["proposed_alpha"][last_acc], alpha0)
    lp_after = np.where(last_acc >= 0, tr["log_p_proposed"][last_acc], res.log_p_alpha_start)
    prev = np.concatenate(([alpha0], after[:-1])); cur = np.concatenate(([res.log_p_alpha_start], lp_after[:-1]))
    return prev, cur, float(after[-1]) if len(tr) else alpha0


def _check_call(res, alpha0, mu_l, T, M, nu_old, nu_new, what):
    """1-3 of the module's list for one call: log p(alpha), the steps, the increments."""
    ex = SR.log_p_alpha(alpha0, mu_l, T, M)
    assert ex.ok(res.log_p_alpha_start), "%s: log_p_alpha_start %r, exact %r, %.1f units of %d" % (what, res.log_p_alpha_start, ex.f, ex.units(res.log_p_alpha_start), ex.n + 8)
    prev, cur, last = _chain(res, alpha0)
    for k, s in enumerate(res.trace):
        prop, lp, lm, u = float(s["proposed_alpha"]), float(s["log_p_proposed"]), float(s["log_metropolis"]), float(s["u"])
        ex = SR.log_p_alpha(prop, mu_l, T, M)
        assert ex.ok(lp), "%s step %d: log_p_proposed %r, exact %r, %.1f units of %d" % (what, k, lp, ex.f, ex.units(lp), ex.n + 8)
        # scale in [0.9, 1/0.9): proposed = fl(scale * previous) is that product within one rounding
        ratio = F(prop) / F(float(prev[k]))
        assert F(SR.SCALE_LO) * (1 - F(1, 2 ** 52)) <= ratio <= F(SR.SCALE_HI) * (1 + F(1, 2 ** 52)), "%s step %d: scale %r" % (what, k, float(ratio))
        ex = SR.log_metropolis(float(prev[k]), prop, float(cur[k]), lp)
        assert ex.ok(lm), "%s step %d: log_metropolis %r, exact %r" % (what, k, lm, ex.f)
        assert 0.0 <= u < 1.0 and bool(s["accepted"]) == SR.accepts(lm, u), "%s step %d: accepted %d with log_metropolis %r, u %r" % (what, k, s["accepted"], lm, u)
    assert res.alpha == last and res.num_accepted == int(res.trace["accepted"].sum()) if res.trace is not None else res.alpha == alpha0
    assert np.all(nu_new >= SR.NU_FLOOR) and np.all(np.isfinite(nu_new))
    assert res.num_floored == int(np.count_nonzero(nu_new == SR.NU_FLOOR))
    for name, ex, got in (("delta_log_G", SR.delta_log_G(mu_l, T, M, nu_old, nu_new), res.delta_log_G),
                          ("delta_log_prior_alpha", SR.delta_log_prior_alpha(alpha0, res.alpha, nu_old), res.delta_log_prior_alpha),
                          ("delta_log_prior_nu", SR.delta_log_prior_nu(res.alpha, nu_old, nu_new), res.delta_log_prior_nu),
                          ("sum_nu_old", X.Exact(sum(map(F, nu_old.tolist())), sum(map(F, nu_old.tolist())), len(nu_old)), res.sum_nu_old),
                          ("sum_nu_new", X.Exact(sum(map(F, nu_new.tolist())), sum(map(F, nu_new.tolist())), len(nu_new)), res.sum_nu_new)):
        assert ex.ok(got), "%s: %s %r, exact %r, %.1f units of %d" % (what, name, got, ex.f, ex.units(got), ex.n + 8)


# L below a wave, across a wave, across the reducer's 1 024 threads; alpha small, middling, large; a case without any mutation (n_plus = 0)
CASES = [(1, 0.5, False), (63, 0.02, False), (65, 50.0, False), (1025, 0.5, False), (2000, 0.02, False), (2000, 50.0, False), (65, 0.5, True), (1025, 0.02, True)]


@pytest.mark.parametrize("L,alpha,all_zero", CASES)
def test_log_p_alpha_steps_and_increments_against_the_model(L, alpha, all_zero):
    T, M, nu_old = _synthetic(L, 100 + L, all_zero=all_zero)
    b = _handle(L, nu_old)
    try:
        assert np.array_equal(b.nu_l(), nu_old)                       # before any move: what emat_set_evo was given
        res = b.site_rate_moves(T, M, alpha, 10, key=0xA11CE + L)
        nu_new = b.nu_l()
        assert len(res.trace) == 10
        _check_call(res, alpha, [1e-3] * L, T, M, nu_old, nu_new, "L=%d alpha=%g" % (L, alpha))
        if all_zero:
            assert not M.any()
    finally:
        b.close()


def test_two_site_partitions_with_different_mu():
    rng = np.random.default_rng(7323)                                  # 33 tips, 2 000 sites, 74 mutations
    sc, _, evo, what = random_scenario(rng, 5, max_tips=60)
    assert evo is not None and evo[0][0] != evo[0][1], what
    mu, pi, q, pfs = evo
    L = sc.num_sites
    ev = X.Evo(mu, pi, q, np.ones(L), pfs)
    st = X.stats(sc.tree, sc.ref, ev)                                  # the tree's own statistics, from the exact model
    T = np.array([e.f for e in st["Ttwiddle_l"]]); M = st["num_muts_l"].astype(np.int32)
    nu_old = 0.5 + np.random.default_rng(5).random(L)
    b = _handle(L, nu_old, mu=tuple(mu), pfs=pfs, pi=pi, q=q)
    try:
        res = b.site_rate_moves(T, M, 0.5, 10, key=77)
        _check_call(res, 0.5, [float(mu[p]) for p in pfs], T, M, nu_old, b.nu_l(), what)
    finally:
        b.close()


def test_scales_of_20000_steps_are_uniform():
    L = 300
    T, M, nu_old = _synthetic(L, 9)
    b = _handle(L, nu_old)
    try:
        res = b.site_rate_moves(T, M, 0.5, 20000, key=2024)
    finally:
        b.close()
    prev, _, last = _chain(res, 0.5)
    scales = res.trace["proposed_alpha"] / prev
    p = sst.kstest(scales, sst.uniform(SR.SCALE_LO, SR.SCALE_HI - SR.SCALE_LO).cdf).pvalue
    assert p > KS_P, p
    assert res.alpha == last and res.num_accepted == int(res.trace["accepted"].sum())
    p = sst.kstest(res.trace["u"], "uniform").pvalue                    # the acceptance uniforms, drawn at every step
    assert p > KS_P, p


def test_totals_after_recalc_move_by_delta_log_G(record_property):
    """The reference's check_derived_quantities after alpha_moves: log G recomputed under the new rates minus log G before is the move's
    delta_log_G, within the bounds of the two totals and of the increment."""
    sc = make_scenario("C1", num_tips=60, num_sites=2000)
    nu_old = 0.25 + 1.5 * np.random.default_rng(3).random(sc.num_sites)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    try:
        run.set_num_parts(6); run.set_hky(sc.mu, sc.kappa, sc.pi, nu_old); run.set_pop_model(sc.pop)
        _, ref = run.tree()
        run.repartition()
        n, root_part = run.num_parts()
        T, M = run.Ttwiddle_l(), b.num_muts_l()
        b.recalc_derived()
        G0, A0 = b.totals()
        res = b.site_rate_moves(T, M, 1.0, 10, key=31337)
        nu_new = b.nu_l()
        b.recalc_derived()
        G1, A1 = b.totals()
        b.check_derived()
        trees = [b.part_download(p) for p in range(n)]
        bound = 0.0
        for nu in (nu_old, nu_new):
            ev = X.Evo.of(sc, nu)
            for p, t in enumerate(trees):
                bound += X.Derived(t, ref, ev).part_log_G(p == root_part).bound()
        ex = SR.delta_log_G([sc.mu] * sc.num_sites, T, M, nu_old, nu_new)
        bound += ex.bound()
        record_property("delta_log_G", res.delta_log_G); record_property("bound", bound)
        assert A1 == A0                                                 # the coalescent prior does not read the rates
        assert abs((F(G1) - F(G0)) - ex.value) <= bound, (G1 - G0, ex.f, res.delta_log_G, bound)
        assert ex.ok(res.delta_log_G)
    finally:
        run.close(); b.close()


def test_every_site_is_drawn_from_its_own_gamma():
    L, alpha = 4000, 0.5
    T, M, nu_old = _synthetic(L, 12, mean_muts=3.0)
    b = _handle(L, nu_old)
    try:
        res = b.site_rate_moves(T, M, alpha, 0, key=555, trace=False)
        nu_new = b.nu_l()
    finally:
        b.close()
    assert res.alpha == alpha and res.num_accepted == 0 and res.num_floored == 0 and res.trace is None and res.delta_log_prior_alpha == 0.0
    u = sst.gamma.cdf(nu_new, M + alpha, scale=1.0 / (1e-3 * T + alpha))
    p = sst.kstest(u, "uniform").pvalue
    assert p > KS_P, p
    assert SR.delta_log_G([1e-3] * L, T, M, nu_old, nu_new).ok(res.delta_log_G)


@pytest.fixture(scope="module")
def sampler():
    b = d.EmatBackend(16)
    yield b
    b.close()


@pytest.mark.parametrize("shape", [0.2, 0.5, 1.0, 1.7, 30.0, 5000.3])
def test_sampler_distribution_and_moments(sampler, shape):
    n, rate = 200000, 3.0
    x = sampler.debug_sample_gamma(1000 + int(shape * 10), n, shape, rate)
    assert np.all(np.isfinite(x)) and np.all(x > 0.0)
    p = sst.kstest(x, sst.gamma(shape, scale=1.0 / rate).cdf).pvalue
    assert p > KS_P, p
    mean, var = shape / rate, shape / rate ** 2
    se_mean = math.sqrt(var / n)
    se_var = math.sqrt((6.0 / shape + 2.0) * var * var / n)               # Var[(x - mean)^2] = mu4 - var^2, mu4 = (3 + 6 / shape) var^2
    assert abs(x.mean() - mean) <= 5 * se_mean, (x.mean(), mean, se_mean)
    assert abs(np.mean((x - mean) ** 2) - var) <= 5 * se_var, (np.mean((x - mean) ** 2), var, se_var)


def test_sampler_mass_below_the_floor_at_a_small_shape(sampler):
    n = 200000
    x = sampler.debug_sample_gamma(4242, n, 0.02, 1.0)
    assert np.all(np.isfinite(x)) and np.all(x > 0.0)
    want = float(sst.gamma.cdf(1e-50, 0.02))
    assert abs(want - 0.10113) < 1e-5
    share = np.count_nonzero(x < 1e-50) / n
    assert abs(share - want) <= 5 * math.sqrt(want * (1 - want) / n), (share, want)
    assert np.array_equal(x, sampler.debug_sample_gamma(4242, n, 0.02, 1.0))       # draw i is stream (key, i): the same bits again
    assert np.array_equal(x[:1000], sampler.debug_sample_gamma(4242, 1000, 0.02, 1.0))


def test_floored_draws_in_the_move_are_counted():
    L = 2000
    T, M, nu_old = _synthetic(L, 21, mean_muts=0.3)
    b = _handle(L, nu_old)
    try:
        res = b.site_rate_moves(T, M, 0.02, 0, key=99, trace=False)
        nu_new = b.nu_l()
    finally:
        b.close()
    floored = int(np.count_nonzero(nu_new == SR.NU_FLOOR))
    assert res.num_floored == floored and floored > 0 and np.all(nu_new >= SR.NU_FLOOR)
    # sites without mutations are below the floor with probability gamma.cdf(1e-50; 0.02, rate): about a tenth of them
    zero = M == 0
    want = sst.gamma.cdf(1e-50, 0.02, scale=1.0 / (1e-3 * T[zero] + 0.02))
    assert abs(floored - want.sum()) <= 5 * math.sqrt(np.sum(want * (1 - want))), (floored, want.sum())


def test_the_alpha_chain_samples_its_target(record_property):
    L = 300
    T, M, nu_old = _synthetic(L, 33, mean_muts=2.0)
    T = 2.0 / 1e-3 * np.random.default_rng(34).choice([0.8, 0.95, 1.05, 1.2], L)      # few distinct values: the quadrature's integrand groups the sites by (M_l, mu_l Ttwiddle_l)
    b = _handle(L, nu_old)
    try:
        res = b.site_rate_moves(T, M, 1.0, 100000, key=8080)
    finally:
        b.close()
    prev, _, _ = _chain(res, 1.0)
    after = np.append(prev[1:], res.alpha)                                 # alpha after every step
    kept = after[len(after) // 10:]
    batches = kept[: len(kept) // 30 * 30].reshape(30, -1).mean(axis=1)
    se = batches.std(ddof=1) / math.sqrt(30)
    _, want = SR.alpha_posterior_quadrature([1e-3] * L, T, M, [0, 0.1, 0.3, 0.6, 1, 2, 5, 20, mpmath.inf])
    record_property("acceptance_rate", res.num_accepted / 100000.0)
    record_property("posterior_mean", float(want)); record_property("chain_mean", float(batches.mean())); record_property("batch_means_se", float(se))
    assert abs(batches.mean() - float(want)) <= 5 * se, (batches.mean(), float(want), se)


def test_same_arguments_same_bits_and_refusals_leave_the_rates_alone():
    L = 1025
    T, M, nu_old = _synthetic(L, 44)
    a, b2 = _handle(L, nu_old), _handle(L, nu_old)
    try:
        r1 = a.site_rate_moves(T, M, 0.5, 10, key=7); n1 = a.nu_l()
        a.set_evo([1e-3], [PI], [hky_q_matrix(2.0, PI)], nu_old, np.zeros(L, np.int32))
        r2 = a.site_rate_moves(T, M, 0.5, 10, key=7); n2 = a.nu_l()
        r3 = b2.site_rate_moves(T, M, 0.5, 10, key=7); n3 = b2.nu_l()        # another backend in the same process
        for r, n in ((r2, n2), (r3, n3)):
            assert np.array_equal(n1, n) and r1.trace.tobytes() == r.trace.tobytes()
            assert (r1.alpha, r1.log_p_alpha_start, r1.num_accepted, r1.num_floored, r1.delta_log_G, r1.delta_log_prior_alpha, r1.delta_log_prior_nu, r1.sum_nu_old, r1.sum_nu_new) == \
                   (r.alpha, r.log_p_alpha_start, r.num_accepted, r.num_floored, r.delta_log_G, r.delta_log_prior_alpha, r.delta_log_prior_nu, r.sum_nu_old, r.sum_nu_new)
        a.set_evo([1e-3], [PI], [hky_q_matrix(2.0, PI)], nu_old, np.zeros(L, np.int32))
        r4 = a.site_rate_moves(T, M, 0.5, 10, key=8); n4 = a.nu_l()
        assert not np.array_equal(n1, n4) and r4.trace.tobytes() != r1.trace.tobytes() and r4.log_p_alpha_start == r1.log_p_alpha_start
        # refusals: the rates stay, and the next call works
        bad = T.copy(); bad[5] = -1.0
        with pytest.raises(d.EmatError, match="site 5 "):
            a.site_rate_moves(bad, M, 0.5, 10, key=9)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
            a.site_rate_moves(T, M, float("nan"), 10, key=9)
        assert np.array_equal(a.nu_l(), n4)
        r5 = a.site_rate_moves(T, M, 0.5, 10, key=9)
        assert not np.array_equal(a.nu_l(), n4) and len(r5.trace) == 10
    finally:
        a.close(); b2.close()


def test_before_set_evo_is_a_state_error():
    b = d.EmatBackend(8)
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            b.site_rate_moves(np.ones(8), np.zeros(8, np.int32), 1.0, 10, key=1)
        with pytest.raises(d.EmatError, match="STATE"):
            b.nu_l()
    finally:
        b.close()


def _driver_run(sc, seed, device_tree, on, cycles=3):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    out = []
    try:
        run.set_num_parts(24); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop)
        run.set_device_tree(device_tree); run.set_paranoid(True)
        if on:
            run.set_site_rate_moves(True, 1.0)
        with pytest.raises(d.EmatError, match="STATE"):
            run.site_rate_moves()                                      # the parts are not out yet
        out.append(run.site_rates())
        per_cycle = 20 * sc.tree.num_nodes
        for _ in range(cycles):
            run.do_mcmc_steps(per_cycle, per_cycle)                    # paranoid: emat_check_derived after the pass, inside
            out.append(run.site_rates())
        # one more cycle by hand: the move between repartition and the local moves, and the derived quantities checked here
        run.repartition()
        if on:
            res = run.site_rate_moves(trace=True)
            assert len(res.trace) == 10 and res.alpha == run.site_rates()[0] and np.array_equal(b.nu_l(), run.site_rates()[1])
            if not device_tree:
                run.push_params()                                      # the driver pushes the rates it kept: the same values
                assert np.array_equal(b.nu_l(), run.site_rates()[1])
        run.run_moves(per_cycle); b.check_derived()
        run.reassemble()
        out.append(run.site_rates())
    finally:
        run.close(); b.close()
    return out


@pytest.fixture(scope="module")
def driver_scenario():
    return make_scenario("C3", num_tips=700, num_sites=3000, uncertain_tips=0.2)


@pytest.mark.parametrize("device_tree", [False, True])
def test_the_run_driver_samples_the_site_rates_every_cycle(driver_scenario, device_tree):
    sc = driver_scenario
    first = _driver_run(sc, 71, device_tree, True)
    assert first[0][0] == 1.0 and np.array_equal(first[0][1], np.ones(sc.num_sites))
    for (a0, n0), (a1, n1) in zip(first, first[1:]):
        assert a0 != a1 and not np.array_equal(n0, n1)                  # site_rates() changes every cycle
    again = _driver_run(sc, 71, device_tree, True)
    for (a0, n0), (a1, n1) in zip(first, again):
        assert a0 == a1 and np.array_equal(n0, n1)                      # the same seed: the same alpha and nu_l, bit for bit


def test_the_run_driver_leaves_the_rates_alone_when_the_moves_are_off(driver_scenario):
    sc = driver_scenario
    for a, n in _driver_run(sc, 71, False, False, cycles=1):
        assert a == 1.0 and np.array_equal(n, np.ones(sc.num_sites))
