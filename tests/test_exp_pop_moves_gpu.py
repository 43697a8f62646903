"""The Exponential population moves on the device (emat_exp_pop_moves, emat_tree_exp_pop_moves) against tests/exp_pop_moves_model.py.

Every number a call reports is held to (n + 8) u S of the exact model evaluated FROM THE DEVICE'S OWN STATE BEFORE IT: the n0, g and prior it held
before a step (from its trace) and the step's two uniforms, which skygrid_streams restates bit for bit from the key.  A chain is never compared
end to end.  Every decision must agree with the device's own log_metropolis and u; a step whose u lies within 1e-12 relative of
exp(log_metropolis) is excluded, and at most 1 step in 100 may be.  Then the draws (KS over fixed keys) and the sampler as a whole against a
numpy quadrature of its target."""
import dataclasses
import math
from fractions import Fraction as F

import numpy as np
import pytest
import scipy.stats as sst

import delphy_amd as d
import exp_pop_moves_model as EM
import skygrid_streams as RS
from delphy_amd.scenarios import make_scenario
from exact_model import Exact
from skygrid_moves_model import Grid
from test_exact_model import Tally

pytestmark = pytest.mark.gpu

KS_P = 1e-6                      # the project's convention
ID_EXP_POP = 0xFFFFFFF9          # include/emat_backend.h
EXCLUDED = {"steps": 0, "excluded": 0}   # over the whole module: decisions too close to call


@pytest.fixture(scope="module")
def backend():
    b = d.EmatBackend(10)
    yield b
    b.close()


def _uniforms(key, s):
    """(u0, u1) of step s: block s of the stream."""
    return float(RS.to_co(RS.word(np.uint64(key), ID_EXP_POP, 2 * s))), float(RS.to_co(RS.word(np.uint64(key), ID_EXP_POP, 2 * s + 1)))


def _moves(b, case, key, trace=True, **spec_kw):
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    spec = dataclasses.replace(spec, **spec_kw)
    return b.exp_pop_moves(pm, spec, t_ref, t_step, first_cell, k_bar, inner_t, key=key, trace=trace), spec


def _fsum(values) -> Exact:
    fr = [F(float(v)) for v in values]
    return Exact(sum(fr, F(0)), sum((abs(v) for v in fr), F(0)), len(fr))


def check_call(b, tally: Tally, case, key, **spec_kw):
    """One call, every reported number against the model from the device's own state before it.  Returns the result."""
    name, pm, _, t_ref, t_step, first_cell, k_bar, inner_t = case
    r, spec = _moves(b, case, key, **spec_kw)
    where = "%s key %d" % (name, key)
    grid = Grid(t_ref, t_step, first_cell, k_bar)
    t0, n0, g, min_pop = (float(v) for v in pm.p)
    priors = {}

    def prior(n0_, g_):
        if (n0_, g_) not in priors:
            priors[(n0_, g_)] = EM.log_coalescent_prior(EM.exp_pop(t0, n0_, g_, min_pop), grid, inner_t)
        return priors[(n0_, g_)]

    tally.check("log_coalescent_prior_start", prior(n0, g), r.log_coalescent_prior_start, where)
    held = r.log_coalescent_prior_start
    assert len(r.trace) == 2 * spec.rounds
    accepted_ratios, n0_acc, g_acc, oob = [], 0, 0, 0
    for s, rec in enumerate(r.trace):
        w = "%s step %d" % (where, s)
        u0, u1 = _uniforms(key, s)
        assert rec["u"] == u1 and 0.0 <= u1 < 1.0, w                      # drawn whether needed or not
        hastings = None
        if s % 2 == 0:
            if not spec.n0_move_enabled:
                assert (rec["evaluated"], rec["accepted"], rec["proposed"], rec["log_prior_ratio"], rec["log_metropolis"]) == (0, 0, n0, 0.0, 0.0), w
                continue
            new, ratio, hastings = EM.n0_step(n0, u0, spec.inv_n0_prior_alpha, spec.inv_n0_prior_beta)
            tally.check("proposed n0", new, rec["proposed"], w)
            assert rec["evaluated"] == 1, w
            proposal = (float(rec["proposed"]), g)
        else:
            if not spec.g_move_enabled:
                assert (rec["evaluated"], rec["accepted"], rec["proposed"], rec["log_prior_ratio"], rec["log_metropolis"]) == (0, 0, g, 0.0, 0.0), w
                continue
            new, ratio = EM.g_step(g, u0, spec.g_prior_mu, spec.g_prior_scale)
            tally.check("proposed g", new, rec["proposed"], w)
            outside = rec["proposed"] < spec.g_min or rec["proposed"] > spec.g_max
            assert rec["evaluated"] == int(not outside), w
            if outside:                                                   # run.cpp:1298: nothing evaluated, nothing changes
                oob += 1
                assert (rec["accepted"], rec["log_prior_ratio"], rec["log_metropolis"]) == (0, 0.0, 0.0), w
                continue
            proposal = (n0, float(rec["proposed"]))
        tally.check("log_prior_ratio", ratio, rec["log_prior_ratio"], w)
        p_new = prior(*proposal)
        tally.check("log_coalescent_prior_proposed", p_new, rec["log_coalescent_prior_proposed"], w)
        tally.check("log_metropolis", EM.log_metropolis(p_new, prior(n0, g), ratio, hastings), rec["log_metropolis"], w)
        lm = float(rec["log_metropolis"])
        with np.errstate(over="ignore"):
            e = float(np.exp(lm))                                         # (inf above 709, NaN for a NaN)
        EXCLUDED["steps"] += 1
        if e == e and abs(u1 - e) <= 1e-12 * e:
            EXCLUDED["excluded"] += 1
        else:
            assert rec["accepted"] == int(lm > 0 or u1 < e), w
        if rec["accepted"]:
            n0, g = proposal
            held = float(rec["log_coalescent_prior_proposed"])
            accepted_ratios.append(float(rec["log_prior_ratio"]))
            n0_acc += 1 - s % 2; g_acc += s % 2
    assert (r.n0, r.g, r.log_coalescent_prior_end) == (n0, g, held), where
    assert (r.n0_accepted, r.g_accepted, r.g_out_of_bounds) == (n0_acc, g_acc, oob), where
    tally.check("log_coalescent_prior_end", prior(n0, g), r.log_coalescent_prior_end, where)
    tally.check("delta_log_other_priors", _fsum(accepted_ratios), r.delta_log_other_priors, where)
    assert all(math.isfinite(v) for v in (r.n0, r.g, r.log_coalescent_prior_start, r.log_coalescent_prior_end, r.delta_log_other_priors)), where
    return r


# 40 cells of 1/4 before t_ref = t0 = 1000: the grid is [990, 1000)
SMALL = [
    ("1 cell, 1 node, g > 0", (1, 1, 0.3), {}),
    ("2 cells, 63 nodes, g < 0", (2, 63, -0.4), {}),
    ("40 cells, 65 nodes, g = 0", (40, 65, 0.0), {}),
    ("g = 0 under a barrier above n0", (40, 65, 0.0), dict(min_pop=5.0)),
    ("g = 0 under a barrier below n0", (40, 65, 0.0), dict(min_pop=1.0)),
    ("the references default priors", (40, 65, 0.1), dict(inv_n0_prior_alpha=0.0, inv_n0_prior_beta=0.0, g_prior_mu=0.001 / 365.0, g_prior_scale=30.701135 / 365.0)),
    ("t_c before the grid, g > 0", (40, 65, 0.4), dict(t_c=985.0)),
    ("t_c before the grid, g < 0", (40, 65, -0.4), dict(t_c=985.0)),
    ("t_c after the grid, g > 0", (40, 65, 0.4), dict(t_c=1003.0)),
    ("t_c after the grid, g < 0", (40, 65, -0.4), dict(t_c=1003.0)),
    ("t_c on a cell bound, g > 0", (40, 65, 0.4), dict(t_c=998.5)),
    ("t_c on a cell bound, g < 0", (40, 65, -0.4), dict(t_c=998.5)),
    ("t_c inside a cell, g > 0", (40, 65, 0.4), dict(t_c=998.6)),
    ("t_c inside a cell, g < 0", (40, 65, -0.4), dict(t_c=995.3)),
]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: s[0])
def test_small_calls_every_step(backend, shape, record_property):
    name, (nc, ni, g), kw = shape
    tally = Tally("device")
    case = EM.make_case(name, nc, ni, g, **kw)
    r = check_call(backend, tally, case, key=11)
    check_call(backend, tally, case, key=12, rounds=1)
    assert r.n0_accepted + r.g_accepted >= 1
    tally.finish(record_property)


LARGE = [("1025 cells, 1025 nodes, t_c inside", (1025, 1025, 4.0), dict(t_c=900.1)), ("2049 cells, 2049 nodes", (2049, 2049, -4.0), {}),
         ("1 cell, 2048 nodes", (1, 2048, 0.5), {}), ("2 cells, 1024 nodes", (2, 1024, 0.5), {}), ("2049 cells, 1 node", (2049, 1, 4.0), dict(min_pop=0.5)),
         ("1025 cells, 63 nodes", (1025, 63, -4.0), {}), ("2 cells, 2049 nodes, barrier", (2, 2049, 0.5), dict(t_c=999.8))]


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: s[0])
def test_large_calls_either_side_of_the_thread_and_workgroup_counts(backend, shape, record_property):
    """g is given as the growth over the whole grid, so that N stays in range over 512 time units."""
    name, (nc, ni, g_span), kw = shape
    tally = Tally("device")
    case = EM.make_case(name, nc, ni, g_span / (0.25 * nc), rounds=1, **kw)
    check_call(backend, tally, case, key=21)
    tally.finish(record_property)


def _crossing_key():
    """The first key whose first g step proposes a g below -0.001 from +0.001 (found on the CPU: the streams are restated there)."""
    for key in range(1, 200):
        if 0.001 + (-1.0 / 365.0 + 2.0 / 365.0 * _uniforms(key, 1)[0]) < -0.001:
            return key


@pytest.mark.parametrize("min_pop", [0.0, 2.0, 4.0], ids=["no barrier", "barrier below n0", "barrier above n0"])
def test_g_crossing_zero_flips_t_c(backend, min_pop, record_property):
    tally = Tally("device")
    key = _crossing_key()
    case = EM.make_case("g crossing 0", 40, 65, 0.001, min_pop=min_pop, rounds=6)
    r = check_call(backend, tally, case, key=key)
    g_steps = r.trace[1::2]
    assert g_steps["proposed"][0] < -0.001 and g_steps["evaluated"][0] == 1
    assert case[1].p[2] > 0.0                                                 # ... from a start on the other side
    tally.finish(record_property)


def test_an_underflowing_early_cell_takes_the_stopgap(backend, record_property):
    """min_pop = 0, g = 50 and a cell 20 before t0 holding 2.5 lineages: its integral is 0 in float64 and the reference's 1e-100 stands in.  The cells
    between it and the last four time units hold 0 or 1 lineages (no term), the inner nodes lie in the last two: all numbers stay finite."""
    name, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = EM.make_case("stopgap", 80, 65, 50.0, inner_span=2.0)
    k_bar = k_bar.copy(); k_bar[0] = 2.5; k_bar[1:64] = np.arange(63) % 2
    tally = Tally("device")
    r = check_call(backend, tally, (name, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t), key=31)
    assert r.log_coalescent_prior_start < -1e99 and math.isfinite(r.log_coalescent_prior_start)
    tally.finish(record_property)


def _tight_key():
    """The first key whose first g step stays within 0.3 +- 0.0005 and whose second leaves 0.3 +- 0.0035, wherever the first left g (found on the CPU)."""
    for key in range(1, 2000):
        d1, d2 = (-1.0 / 365.0 + 2.0 / 365.0 * _uniforms(key, s)[0] for s in (1, 3))
        if abs(d1) < 0.0004 and abs(d2) > 0.0015:
            return key


def test_tight_bounds_on_g_leave_the_state_alone(backend, record_property):
    tally = Tally("device")
    case = EM.make_case("tight bounds", 40, 65, 0.3, min_pop=1.0, g_min=0.2995, g_max=0.3005, rounds=10)
    r = check_call(backend, tally, case, key=_tight_key())
    g_steps = r.trace[1::2]
    assert 1 <= r.g_out_of_bounds == int((g_steps["evaluated"] == 0).sum()) < 10           # some outside, some evaluated
    assert 0.2995 <= r.g <= 0.3005
    tally.finish(record_property)


def test_each_move_disabled_alone_and_both(backend, record_property):
    tally = Tally("device")
    case = EM.make_case("switches", 40, 65, 0.2, min_pop=1.0, rounds=4)
    pm = case[1]
    both = check_call(backend, tally, case, key=51)
    no_g = check_call(backend, tally, case, key=51, g_move_enabled=False)
    no_n0 = check_call(backend, tally, case, key=51, n0_move_enabled=False)
    none = check_call(backend, tally, case, key=51, n0_move_enabled=False, g_move_enabled=False)
    assert no_g.g == pm.p[2] and no_g.g_accepted == 0 and no_n0.n0 == pm.p[1] and no_n0.n0_accepted == 0
    assert (none.n0, none.g, none.delta_log_other_priors, none.n0_accepted, none.g_accepted) == (pm.p[1], pm.p[2], 0.0, 0, 0)
    assert none.log_coalescent_prior_end == none.log_coalescent_prior_start == both.log_coalescent_prior_start
    # a disabled move does not shift the other's draws: every step's u is its own block's, and the first steps, which start from the same state, propose the same
    for r in (no_g, no_n0, none):
        assert np.array_equal(r.trace["u"], both.trace["u"])
    assert no_g.trace["proposed"][0] == both.trace["proposed"][0] and no_g.trace["log_metropolis"][0] == both.trace["log_metropolis"][0]
    scale_1 = 0.75 + (1 / 0.75 - 0.75) * _uniforms(51, 2)[0]
    for r in (both, no_g):                                                # step 2's scale is block 2's whatever step 1 did
        before = r.trace["proposed"][0] if r.trace["accepted"][0] else pm.p[1]
        assert r.trace["proposed"][2] == pytest.approx(scale_1 * before, rel=1e-14)
    delta_1 = -1.0 / 365.0 + 2.0 / 365.0 * _uniforms(51, 1)[0]
    assert no_n0.trace["proposed"][1] == pytest.approx(pm.p[2] + delta_1, rel=1e-14) and both.trace["proposed"][1] == pytest.approx(pm.p[2] + delta_1, rel=1e-14)
    tally.finish(record_property)


def test_rounds_0_and_1(backend, record_property):
    tally = Tally("device")
    case = EM.make_case("rounds", 40, 65, 0.2, min_pop=1.0)
    pm = case[1]
    r0 = check_call(backend, tally, case, key=61, rounds=0)
    assert (r0.n0, r0.g, r0.delta_log_other_priors) == (pm.p[1], pm.p[2], 0.0) and r0.log_coalescent_prior_end == r0.log_coalescent_prior_start and len(r0.trace) == 0
    r1 = check_call(backend, tally, case, key=61, rounds=1)
    assert len(r1.trace) == 2 and r1.log_coalescent_prior_start == r0.log_coalescent_prior_start
    no_trace, _ = _moves(backend, case, 61, trace=False, rounds=1)
    assert no_trace.trace is None and (no_trace.n0, no_trace.g, no_trace.log_coalescent_prior_end) == (r1.n0, r1.g, r1.log_coalescent_prior_end)
    tally.finish(record_property)


def _same(a, b):
    return np.array_equal(a.trace, b.trace) and all(getattr(a, f) == getattr(b, f) for f in (
        "n0", "g", "log_coalescent_prior_start", "log_coalescent_prior_end", "delta_log_other_priors", "n0_accepted", "g_accepted", "g_out_of_bounds"))


def test_same_arguments_same_bits_in_every_call_and_on_every_handle(backend):
    case = EM.make_case("", 2049, 2049, 4.0 / 512.0, t_c=900.1, rounds=20)
    r1, _ = _moves(backend, case, key=77)
    r2, _ = _moves(backend, case, key=77)
    other = d.EmatBackend(20)
    try:
        r3, _ = _moves(other, case, key=77)
    finally:
        other.close()
    assert _same(r1, r2) and _same(r1, r3)
    assert np.all(np.isfinite(r1.trace["log_metropolis"])) and r1.n0_accepted + r1.g_accepted >= 1
    r4, _ = _moves(backend, case, key=78)
    assert not np.array_equal(r1.trace["u"], r4.trace["u"])


# ---- the draws ---------------------------------------------------------------------------------------------------------------
KEYS = (1001, 1002)
KS_ROUNDS = 1000


def _ks(x, lo, hi):
    return sst.kstest(np.asarray(x, float), sst.uniform(lo, hi - lo).cdf).pvalue


def test_the_scales_and_deltas_follow_their_distributions(backend):
    """Two calls of 1 000 rounds on one cell and one node: scale = new_n0 / old_n0 ~ U[0.75, 1 / 0.75), delta = new_g - old_g ~ U[-1/365, 1/365), and the
    acceptance uniforms U[0, 1); each first shown on the CPU restatement of the stream at these keys."""
    case = EM.make_case("", 1, 1, 0.1, rounds=KS_ROUNDS)
    pm = case[1]
    scales, deltas, us = [], [], []
    for key in KEYS:
        u0 = np.array([_uniforms(key, s)[0] for s in range(2 * KS_ROUNDS)])
        cpu_scale, cpu_delta = 0.75 + (1 / 0.75 - 0.75) * u0[0::2], -1.0 / 365.0 + 2.0 / 365.0 * u0[1::2]
        assert _ks(cpu_scale, 0.75, 1 / 0.75) > KS_P and _ks(cpu_delta, -1.0 / 365.0, 1.0 / 365.0) > KS_P       # the keys' own
        r, _ = _moves(backend, case, key=key)
        tr = r.trace
        n0_before = np.concatenate([[pm.p[1]], np.where(tr["accepted"][0::2] == 1, tr["proposed"][0::2], np.nan)])
        g_before = np.concatenate([[pm.p[2]], np.where(tr["accepted"][1::2] == 1, tr["proposed"][1::2], np.nan)])
        for a in (n0_before, g_before):                                   # carry the last accepted value forward
            for i in range(1, len(a)):
                if a[i] != a[i]:
                    a[i] = a[i - 1]
        sc = tr["proposed"][0::2] / n0_before[:-1]; de = tr["proposed"][1::2] - g_before[:-1]
        assert np.allclose(sc, cpu_scale, rtol=1e-14, atol=0) and np.allclose(de, cpu_delta, rtol=0, atol=1e-15)
        assert np.all(tr["evaluated"] == 1) and 0 < r.n0_accepted < KS_ROUNDS and 0 < r.g_accepted <= KS_ROUNDS     # (one node: a step of 1/365 in g is nearly always taken)
        scales.append(sc); deltas.append(de); us.append(tr["u"])
    scales, deltas, us = (np.concatenate(v) for v in (scales, deltas, us))
    assert _ks(scales, 0.75, 1 / 0.75) > KS_P and _ks(deltas, -1.0 / 365.0, 1.0 / 365.0) > KS_P and _ks(us, 0.0, 1.0) > KS_P
    assert scales.min() >= 0.75 and scales.max() < 1 / 0.75 * (1 + 1e-15) and np.abs(deltas).max() <= 1.0 / 365.0 + 1e-15


# ---- the sampler as a whole ----------------------------------------------------------------------------------------------------
def _target_means(t0, spec, t_ref, t_step, first_cell, k_bar, inner_t, x, g):
    """E[log n0], E[g] under exp(log prior of the tree) n0^-(alpha + 1) exp(-beta / n0) exp(-|g - mu| / scale) on [g_min, g_max], min_pop = 0: float64
    numpy quadrature over (x = log n0, g) on the grids given (the measure dn0 = n0 dx), each cell's integral of N by 8-point Gauss-Legendre."""
    X_, G_ = np.meshgrid(x, g, indexing="ij")
    logp = np.zeros_like(X_)
    nodes, weights = np.polynomial.legendre.leggauss(8)
    for c, kc in enumerate(k_bar):
        lo = t_ref + (first_cell + c) * t_step
        I = np.zeros_like(X_)
        for z, w in zip(nodes, weights):
            I += 0.5 * t_step * w * np.exp(X_ + G_ * (lo + 0.5 * t_step * (z + 1.0) - t0))
        logp -= t_step * kc * (kc - 1.0) / (2.0 * (I / t_step))
    for t in inner_t:
        logp -= X_ + G_ * (t - t0)
    logp += -(spec.inv_n0_prior_alpha + 1.0) * X_ - spec.inv_n0_prior_beta * np.exp(-X_) - np.abs(G_ - spec.g_prior_mu) / spec.g_prior_scale + X_
    wgt = np.exp(logp - logp.max()); wgt /= wgt.sum()
    return np.array([(wgt * X_).sum(), (wgt * G_).sum()]), wgt


def test_the_chain_of_2000_calls_samples_its_target(backend, record_property):
    """40 cells, 65 coalescence times, a proper prior (alpha 2, beta 1.5, g in [-0.6, 0.9]): 2 000 successive calls of 50 rounds, each from the last
    result; the chain means of log n0 and g within 4 batch-means standard errors (40 batches) of the quadrature."""
    _, pm, _, t_ref, t_step, first_cell, k_bar, inner_t = EM.make_case("", 40, 65, 0.1)
    spec = d.ExpPopSpec(inv_n0_prior_alpha=2.0, inv_n0_prior_beta=1.5, g_prior_mu=0.05, g_prior_scale=0.3, g_min=-0.6, g_max=0.9, rounds=50)
    t0 = pm.p[0]; n0, g = 3.0, 0.1
    n_calls, n_batches = 2000, 40
    chain = np.zeros((n_calls, 2)); acc = np.zeros(3)
    for i in range(n_calls):
        r = backend.exp_pop_moves(d.PopModel.exp(t0, n0, g, 0.0), spec, t_ref, t_step, first_cell, k_bar, inner_t, key=0x5EED0000 + i)
        n0, g = r.n0, r.g
        chain[i] = math.log(n0), g
        acc += r.n0_accepted, r.g_accepted, r.g_out_of_bounds
    mean = chain.mean(axis=0)
    se = chain.reshape(n_batches, -1, 2).mean(axis=1).std(axis=0, ddof=1) / math.sqrt(n_batches)
    lo, hi = chain[:, 0].min() - 3.0, chain[:, 0].max() + 3.0
    fine, w = _target_means(t0, spec, t_ref, t_step, first_cell, k_bar, inner_t, np.linspace(lo, hi, 401), np.linspace(spec.g_min, spec.g_max, 401))
    coarse, _ = _target_means(t0, spec, t_ref, t_step, first_cell, k_bar, inner_t, np.linspace(lo, hi, 201), np.linspace(spec.g_min, spec.g_max, 201))
    assert np.all(np.abs(fine - coarse) < 0.1 * se), (fine, coarse, se)          # the grid is fine enough ...
    assert w[0].sum() + w[-1].sum() < 1e-9                                       # ... and wide enough in log n0 (g is bounded by the prior itself)
    dist = (mean - fine) / se
    rates = acc / (n_calls * spec.rounds)
    record_property("chain_distance_in_standard_errors", [float("%.3g" % v) for v in dist])
    record_property("acceptance_n0_g_and_g_out_of_bounds", [float("%.3g" % v) for v in rates])
    print("chain means", mean, "quadrature", fine, "se", se, "distance / se", dist, "acceptance n0, g, g out of bounds", rates)
    assert np.all(np.abs(dist) < 4.0), (mean, fine, se, dist)


# ---- the tree variant ----------------------------------------------------------------------------------------------------------
def test_the_moves_on_the_trees_statistics_are_the_moves_on_their_download_and_the_state_rule():
    sc = make_scenario("C3", num_tips=60, num_sites=600, uncertain_tips=0.2)
    t = np.asarray(sc.tree.t)
    t_ref = float(t.max()); span = t_ref - float(t.min()); t_step = span / 37.0
    spec = d.ExpPopSpec(inv_n0_prior_alpha=0.5, inv_n0_prior_beta=0.5, rounds=10)
    b, other, rb = d.EmatBackend(sc.num_sites), d.EmatBackend(sc.num_sites), d.EmatBackend(sc.num_sites)
    run = None
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            b.tree_exp_pop_moves(d.PopModel.exp(t_ref, 3.0, 0.0), spec, t_ref, t_step)      # no tree uploaded
        b.tree_upload(sc.tree); other.tree_upload(sc.tree)
        for g, min_pop in ((2.0 / span, 0.0), (-2.0 / span, 1.5)):
            pm = d.PopModel.exp(t_ref, 3.0, g, min_pop)
            first, k_bar, inner_t = b.tree_coalescent_stats(t_ref, t_step)
            want = b.exp_pop_moves(pm, spec, t_ref, t_step, first, k_bar, inner_t, key=9, trace=True)
            for got in (b.tree_exp_pop_moves(pm, spec, t_ref, t_step, key=9, trace=True), b.tree_exp_pop_moves(pm, spec, t_ref, t_step, key=9, trace=True),
                        other.tree_exp_pop_moves(pm, spec, t_ref, t_step, key=9, trace=True)):
                assert _same(got, want)
            assert want.n0_accepted + want.g_accepted >= 1 and len(inner_t) == 59
        run = d.EmatRun(rb, sc.tree, sc.ref, 3)
        run.set_num_parts(4); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
        run.repartition()
        with pytest.raises(d.EmatError, match="STATE.*parts are out"):
            rb.tree_exp_pop_moves(d.PopModel.exp(t_ref, 3.0, 0.0), spec, t_ref, t_step)
        run.reassemble()
        assert rb.tree_exp_pop_moves(d.PopModel.exp(t_ref, 3.0, 0.0), spec, t_ref, t_step).log_coalescent_prior_start < 0.0
    finally:
        if run is not None:
            run.close()
        other.close(); b.close(); rb.close()


def test_at_most_one_decision_in_100_was_too_close_to_call():
    """Over every step the tests above checked (this one runs last)."""
    assert EXCLUDED["steps"] >= 100 and EXCLUDED["excluded"] * 100 <= EXCLUDED["steps"], EXCLUDED
