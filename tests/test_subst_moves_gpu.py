"""The substitution-model moves on the device (emat_subst_moves, emat_parts_subst_stats, emat_parts_subst_moves, emat_get_evo) against
tests/subst_moves_model.py.

Every number a call reports is held to (n + 8) u S of the exact model evaluated FROM THE DEVICE'S OWN STATE BEFORE IT: the kappa and pi it held
before a step (from its trace), the mu it drew (from its result) and the step's four words, which skygrid_streams restates bit for bit from the
key.  A chain is never compared end to end.  Every decision must agree with the device's own log_metropolis and u; a step whose u lies within
1e-12 relative of exp(log_metropolis) is excluded, and at most 1 step in 100 may be.  Then the mu draws (KS over fixed keys), the sampler as a
whole against numpy quadratures of its targets, the statistics of the parts on the handle against exact_model's, and the handle's model after a call.

The statistics are hand-made 4 P + 16 P + 4 numbers wherever no tree is needed."""
import dataclasses
import math
from fractions import Fraction as F

import numpy as np
import pytest
import scipy.stats as sst

import delphy_amd as d
import exact_model as X
import skygrid_streams as RS
import subst_moves_model as SM
from delphy_amd.scenarios import KAPPA, PI, Scenario
from exact_model import Exact
from helpers import configure, split_parts
from test_exact_model import Tally

pytestmark = pytest.mark.gpu

KS_P = 1e-6                      # the project's convention
ID_MU, ID_STEPS = 0xFFFFFFF8, 0xFFFFFFF7     # include/emat_backend.h
REDUCE_THREADS = 256             # csrc/emat_subst_kernels.hpp: k_sb_reduce_threads
EXCLUDED = {"steps": 0, "excluded": 0}       # over the whole module: decisions too close to call
L = 12
PI0 = (0.1, 0.2, 0.3, 0.4)


def _handle(P):
    b = d.EmatBackend(L)
    b.set_ref_sequence(np.arange(L) % 4)
    b.set_evo([1e-3] * P, [PI0] * P, [d.hky_q_matrix(2.0, PI0)] * P, np.ones(L), np.arange(L) % P)
    return b


@pytest.fixture(scope="module")
def backend():
    b = _handle(1)
    yield b
    b.close()


@pytest.fixture(scope="module")
def backend2():
    b = _handle(2)
    yield b
    b.close()


def _words(key, s):
    """The four uniforms of step s: words 4 s .. 4 s + 3 of the steps' stream."""
    return tuple(float(RS.to_co(RS.word(np.uint64(key), ID_STEPS, 4 * s + k))) for k in range(4))


# Statistics of a tree of a few hundred days under mu = 1e-3: mu q_a T of the order of the mutation counts.
T1 = np.array([[41000.0, 52000.0, 38000.5, 47000.25]])
M1 = np.array([[[0, 3, 11, 2], [4, 0, 1, 13], [9, 2, 0, 3], [1, 12, 2, 0]]], np.int64)
C1 = np.array([70, 80, 60, 90], np.int64)
T2 = np.array([[21000.0, 30000.0, 18000.5, 27000.25], [20000.0, 22000.0, 20000.0, 20000.0]])
M2 = np.array([M1[0] // 2, M1[0] - M1[0] // 2], np.int64)
SPEC = d.SubstSpec(mu=1e-3, kappa=2.0, pi=PI0, mu_prior_alpha=1.0, mu_prior_beta=0.0, rounds=6)


def _fsum(values) -> Exact:
    fr = [F(float(v)) for v in values]
    return Exact(sum(fr, F(0)), sum((abs(v) for v in fr), F(0)), len(fr))


def check_call(b, tally: Tally, spec, T, M, C, key, name=""):
    """One call, every reported number against the model from the device's own state before it.  Returns (the result, the sum of the bounds of
    what the call added to log G)."""
    r = b.subst_moves(spec, T, M, C, key=key, trace=True)
    where = "%s key %d" % (name, key)
    shape, rate, _, _ = SM.mu_posterior(spec.kappa, spec.pi, T, M, spec.mu_prior_alpha, spec.mu_prior_beta)
    tally.check("mu_post_shape", shape, r.mu_post_shape, where)
    tally.check("mu_post_rate", rate, r.mu_post_rate, where)
    cpu_draw = float(RS.gamma_draw(np.uint64(key), ID_MU, r.mu_post_shape, r.mu_post_rate)[0])
    assert r.mu_draw == pytest.approx(cpu_draw, rel=1e-9), where            # drawn whether needed or not; log, sqrt and cos are each side's own
    mu, bounds = float(spec.mu), 0.0
    if spec.do_mu:
        dG, dP = SM.mu_deltas(spec.mu, r.mu_draw, spec.kappa, spec.pi, T, M, spec.mu_prior_alpha, spec.mu_prior_beta)
        tally.check("mu_delta_log_G", dG, r.mu_delta_log_G, where)
        tally.check("mu_delta_log_other_priors", dP, r.mu_delta_log_other_priors, where)
        mu = r.mu_draw; bounds += dG.bound()
    else:
        assert (r.mu_delta_log_G, r.mu_delta_log_other_priors) == (0.0, 0.0), where
    assert r.mu == mu, where
    kappa, pi = float(spec.kappa), [float(v) for v in spec.pi]
    acc_G, acc_P = [r.mu_delta_log_G], [r.mu_delta_log_other_priors]
    n_pi = n_kappa = n_left = n_forced = 0
    assert len(r.trace) == 2 * spec.rounds
    for s, rec in enumerate(r.trace):
        w = "%s step %d" % (where, s)
        u = _words(key, s)
        assert rec["kappa"] == kappa and rec["pi"].tolist() == pi, w         # the state before the step is the state the steps so far left
        lpr = lh = None
        if s % 2 == 0:
            d_ex, ia, ib, new_pi = SM.pi_proposal(pi, u[0], u[1], u[2])
            assert rec["u"] == u[3] and (rec["ia"], rec["ib"]) == (ia, ib) and ia != ib, w
            tally.check("d", d_ex, rec["proposal"], w)
            if not spec.do_pi or new_pi is None:
                left = int(spec.do_pi)
                assert (rec["evaluated"], rec["accepted"], rec["left_unit"], rec["force_rejected"], rec["delta_log_G"], rec["log_metropolis"]) == (0, 0, left, 0, 0.0, 0.0), w
                n_left += left
                continue
            ex = SM.delta_log_G(mu, kappa, pi, kappa, new_pi, T, M, C, root_term=True)
            proposal = (kappa, [pi[k] + float(rec["proposal"]) if k == ia else (pi[k] - float(rec["proposal"]) if k == ib else pi[k]) for k in range(4)])
        else:
            sc_ex, new_kappa = SM.kappa_proposal(kappa, u[0])
            assert rec["u"] == u[1] and (rec["ia"], rec["ib"]) == (-1, -1), w
            tally.check("scale", sc_ex, rec["proposal"], w)
            if not spec.do_kappa:
                assert (rec["evaluated"], rec["accepted"], rec["force_rejected"], rec["delta_log_G"], rec["log_prior_ratio"], rec["log_metropolis"]) == (0, 0, 0, 0.0, 0.0, 0.0), w
                continue
            ex = SM.delta_log_G(mu, kappa, pi, new_kappa, pi, T, M, C, root_term=False)
            lpr, lh = SM.kappa_prior_and_hastings(kappa, new_kappa)
            proposal = (kappa * float(rec["proposal"]), pi)
        assert rec["evaluated"] == 1 and rec["left_unit"] == 0, w
        if ex is None:                                                      # run.cpp:1007, :1016, :1084
            assert (rec["force_rejected"], rec["accepted"], rec["delta_log_G"], rec["log_prior_ratio"], rec["log_metropolis"]) == (1, 0, 0.0, 0.0, 0.0), w
            n_forced += 1
            continue
        assert rec["force_rejected"] == 0, w
        tally.check("delta_log_G", ex, rec["delta_log_G"], w)
        if lpr is not None:
            tally.check("log_prior_ratio", lpr, rec["log_prior_ratio"], w)
        else:
            assert rec["log_prior_ratio"] == 0.0, w
        tally.check("log_metropolis", SM.log_metropolis(ex, lpr, lh), rec["log_metropolis"], w)
        lm = float(rec["log_metropolis"])
        with np.errstate(over="ignore"):
            e = float(np.exp(lm))                                           # (inf above 709, NaN for a NaN)
        EXCLUDED["steps"] += 1
        if e == e and abs(rec["u"] - e) <= 1e-12 * e:
            EXCLUDED["excluded"] += 1
        else:
            assert rec["accepted"] == int(lm > 0 or rec["u"] < e), w
        if rec["accepted"]:
            kappa, pi = proposal
            acc_G.append(float(rec["delta_log_G"])); acc_P.append(float(rec["log_prior_ratio"])); bounds += ex.bound()
            n_pi += 1 - s % 2; n_kappa += s % 2
    assert (r.kappa, r.pi.tolist()) == (kappa, pi), where
    assert (r.pi_accepted, r.kappa_accepted, r.pi_left_unit, r.forced_rejections) == (n_pi, n_kappa, n_left, n_forced), where
    tally.check("delta_log_G (total)", _fsum(acc_G), r.delta_log_G, where)
    tally.check("delta_log_other_priors", _fsum(acc_P), r.delta_log_other_priors, where)
    assert all(math.isfinite(v) for v in (r.mu, r.kappa, r.delta_log_G, r.delta_log_other_priors, *r.pi)) and abs(sum(r.pi) - 1.0) < 1e-9, where
    return r, bounds


CASE_KEYS, P2_KEYS, LAST_KEYS = (11, 12), (21, 22, 23), (13, 14)      # the keys of the calls held to the model step by step (shown callable on the CPU: test_subst_moves_model.py)
CASES = [
    ("the references defaults", SPEC, T1, M1, C1),
    ("a proper mu prior", dataclasses.replace(SPEC, mu_prior_alpha=2.5, mu_prior_beta=700.0), T1, M1, C1),
    ("kappa below 1, skewed pi", dataclasses.replace(SPEC, kappa=0.4, pi=(0.55, 0.05, 0.3, 0.1)), T1, M1, C1),
    ("no mutations, no root", SPEC, T1, np.zeros((1, 4, 4), np.int64), np.zeros(4, np.int64)),
    ("no branch lengths", dataclasses.replace(SPEC, mu_prior_beta=3.0), np.zeros((1, 4)), M1, C1),
    ("thousands of mutations", SPEC, 100.0 * T1, 100 * M1, 50 * C1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_every_traced_number_one_partition(backend, case, record_property):
    name, spec, T, M, C = case
    tally = Tally("device")
    r, _ = check_call(backend, tally, spec, T, M, C, key=CASE_KEYS[0], name=name)
    check_call(backend, tally, spec, T, M, C, key=CASE_KEYS[1], name=name)
    assert len(r.trace) == 12
    tally.finish(record_property)


def test_every_traced_number_two_partitions(backend2, record_property):
    tally = Tally("device")
    accepted = 0
    for key in P2_KEYS:
        r, _ = check_call(backend2, tally, SPEC, T2, M2, C1, key=key, name="P = 2")
        accepted += r.pi_accepted + r.kappa_accepted
    assert accepted >= 1
    tally.finish(record_property)


# ---- edges -------------------------------------------------------------------------------------------------------------------
def _leaving_key():
    """The first key whose step 0 picks ia = 0 with d > 0.005 (0.995 + d leaves at 1) and whose step 2 picks ib = 1, ia != 0 with d > 0.004
    (0.004 - d leaves at 0): with the kappa move off, both see the start state (found on the CPU: the streams are restated there)."""
    for key in range(1, 100000):
        a, b = _words(key, 0), _words(key, 2)
        ia2 = int(4.0 * b[1])
        if int(4.0 * a[1]) == 0 and 0.01 * a[0] > 0.0051 and ia2 != 0 and (ia2 + 1 + int(3.0 * b[2])) % 4 == 1 and 0.01 * b[0] > 0.0041:
            return key


def test_pi_leaving_the_unit_interval_on_either_side(backend, record_property):
    tally = Tally("device")
    spec = dataclasses.replace(SPEC, pi=(0.995, 0.004, 0.0005, 0.0005), do_kappa=False, rounds=8)
    key = _leaving_key()
    r, _ = check_call(backend, tally, spec, T1, M1, C1, key=key, name="pi at the edges")
    top, bottom = r.trace[0], r.trace[2]
    assert top["left_unit"] == 1 and top["ia"] == 0 and top["pi"][0] + top["proposal"] >= 1.0
    assert bottom["left_unit"] == 1 and bottom["ib"] == 1 and bottom["pi"][1] - bottom["proposal"] <= 0.0
    assert r.pi_left_unit >= 2 and np.all(np.isfinite(r.trace["log_metropolis"])) and np.all(r.pi > 0.0) and np.all(r.pi < 1.0)
    tally.finish(record_property)


def _scale_below_1_key():
    for key in range(1, 1000):
        if 0.75 + (1 / 0.75 - 0.75) * _words(key, 1)[0] < 0.9:
            return key


def test_the_smallest_kappa_with_transitions_counted_is_force_rejected(backend):
    """kappa = 5e-324 and a key whose first scale is below 1.  (kappa x scale rounds to 5e-324 again or to 0; either way) the transition rates
    kappa pi_b / R of the proposal underflow to 0 for the small pi_b while transitions were counted: every evaluated step is force-rejected
    (run.cpp:1016, :1084), nothing is accepted and the state stays what it was, finite."""
    pi = (0.05, 0.05, 0.45, 0.45)
    spec = dataclasses.replace(SPEC, kappa=5e-324, pi=pi, do_mu=False, rounds=4)
    r = backend.subst_moves(spec, T1, M1, C1, key=_scale_below_1_key(), trace=True)
    assert r.trace["proposal"][1] < 1.0
    ev = r.trace[r.trace["evaluated"] == 1]
    assert len(ev) >= 4 and np.all(ev["force_rejected"] == 1) and np.all(ev["accepted"] == 0) and r.forced_rejections == len(ev)
    assert (r.kappa, r.pi.tolist(), r.mu, r.delta_log_G, r.delta_log_other_priors) == (5e-324, list(pi), 1e-3, 0.0, 0.0)
    assert np.all(np.isfinite(r.trace["log_metropolis"])) and np.all(np.isfinite(r.trace["delta_log_G"]))
    mu, pi_h, q = backend.get_evo()
    assert np.all(np.isfinite(q)) and q[0][2][0] == 0.0 and q[0][3][1] == 0.0 and q[0][0][1] > 0.0     # G -> A and T -> C at rate kappa pi_b / R = 0, both counted; transversions as ever
    assert M1[0][2][0] > 0 and M1[0][3][1] > 0


def test_a_zero_count_paired_with_a_zero_rate(backend, record_property):
    """The same underflowing transition rates with no transition counted: the reference skips the term (:1015, :1083), nothing is forced and no
    0 x log(0) is formed.  The pi steps are held to the model; the kappa steps (whose proposal, 5e-324 x scale, rounds by up to half its value, far
    beyond what the model's bound for a proposal assumes) are held to being finite and unforced."""
    tally = Tally("device")
    M = M1.copy(); M[0, 0, 2] = M[0, 2, 0] = M[0, 1, 3] = M[0, 3, 1] = 0
    spec = dataclasses.replace(SPEC, kappa=5e-324, pi=(0.05, 0.05, 0.45, 0.45), rounds=4)
    r, _ = check_call(backend, tally, dataclasses.replace(spec, do_kappa=False), T1, M, C1, key=31, name="zero count, zero rate")
    assert r.forced_rejections == 0 and np.all(r.trace["evaluated"][0::2] == 1) and np.all(np.isfinite(r.trace["log_metropolis"]))
    raw = backend.subst_moves(spec, T1, M, C1, key=31, trace=True)
    assert raw.forced_rejections == 0 and np.all(raw.trace["evaluated"] == 1) and np.all(np.isfinite(raw.trace["log_metropolis"])) and np.all(np.isfinite(raw.trace["delta_log_G"]))
    assert math.isfinite(raw.delta_log_G) and raw.kappa in (0.0, 5e-324)
    tally.finish(record_property)


def test_rounds_0_is_the_mu_draw_alone(backend, record_property):
    tally = Tally("device")
    r0, _ = check_call(backend, tally, dataclasses.replace(SPEC, rounds=0), T1, M1, C1, key=41, name="rounds 0")
    assert len(r0.trace) == 0 and (r0.kappa, r0.pi.tolist()) == (2.0, list(PI0)) and r0.mu == r0.mu_draw != 1e-3
    assert (r0.delta_log_G, r0.delta_log_other_priors) == (r0.mu_delta_log_G, r0.mu_delta_log_other_priors)
    no_trace = backend.subst_moves(dataclasses.replace(SPEC, rounds=3), T1, M1, C1, key=41)
    r3, _ = check_call(backend, tally, dataclasses.replace(SPEC, rounds=3), T1, M1, C1, key=41, name="rounds 3")
    assert no_trace.trace is None and (no_trace.mu, no_trace.kappa, no_trace.pi.tolist(), no_trace.delta_log_G) == (r3.mu, r3.kappa, r3.pi.tolist(), r3.delta_log_G)
    assert r3.mu_draw == r0.mu_draw
    tally.finish(record_property)


def test_each_switch_off_leaves_the_other_moves_draws_unchanged(backend, record_property):
    tally = Tally("device")
    spec = dataclasses.replace(SPEC, rounds=5)
    every, _ = check_call(backend, tally, spec, T1, M1, C1, key=51, name="switches")
    no_mu, _ = check_call(backend, tally, dataclasses.replace(spec, do_mu=False), T1, M1, C1, key=51, name="switches")
    no_pi, _ = check_call(backend, tally, dataclasses.replace(spec, do_pi=False), T1, M1, C1, key=51, name="switches")
    no_kappa, _ = check_call(backend, tally, dataclasses.replace(spec, do_kappa=False), T1, M1, C1, key=51, name="switches")
    none, _ = check_call(backend, tally, dataclasses.replace(spec, do_mu=False, do_pi=False, do_kappa=False), T1, M1, C1, key=51, name="switches")
    assert (none.mu, none.kappa, none.pi.tolist(), none.delta_log_G, none.delta_log_other_priors) == (1e-3, 2.0, list(PI0), 0.0, 0.0)
    assert no_mu.mu == 1e-3 and no_mu.mu_draw == every.mu_draw and no_pi.pi.tolist() == list(PI0) and no_pi.pi_accepted == 0 and no_kappa.kappa == 2.0 and no_kappa.kappa_accepted == 0
    for r in (no_mu, no_pi, no_kappa, none):                                # every step's words are its own block's, whatever ran before it
        for f in ("u", "proposal", "ia", "ib"):
            assert np.array_equal(r.trace[f], every.trace[f]), f
    assert none.mu_draw == every.mu_draw
    tally.finish(record_property)


def _same(a, b):
    return np.array_equal(a.trace, b.trace) and a.pi.tolist() == b.pi.tolist() and all(getattr(a, f) == getattr(b, f) for f in (
        "mu", "kappa", "mu_post_shape", "mu_post_rate", "mu_draw", "delta_log_G", "delta_log_other_priors", "mu_delta_log_G", "mu_delta_log_other_priors",
        "pi_accepted", "kappa_accepted", "pi_left_unit", "forced_rejections"))


def test_same_arguments_same_bits_in_every_call_and_on_every_handle(backend):
    spec = dataclasses.replace(SPEC, rounds=200)
    r1 = backend.subst_moves(spec, 100.0 * T1, 100 * M1, 50 * C1, key=77, trace=True)
    r2 = backend.subst_moves(spec, 100.0 * T1, 100 * M1, 50 * C1, key=77, trace=True)
    other = _handle(1)
    try:
        r3 = other.subst_moves(spec, 100.0 * T1, 100 * M1, 50 * C1, key=77, trace=True)
    finally:
        other.close()
    assert _same(r1, r2) and _same(r1, r3)
    assert r1.pi_accepted >= 1 and r1.kappa_accepted >= 1 and np.all(np.isfinite(r1.trace["log_metropolis"]))
    r4 = backend.subst_moves(spec, 100.0 * T1, 100 * M1, 50 * C1, key=78, trace=True)
    assert not np.array_equal(r1.trace["u"], r4.trace["u"]) and r4.mu_draw != r1.mu_draw


def test_the_handles_model_after_a_call_and_after_a_refusal(backend2):
    r = backend2.subst_moves(SPEC, T2, M2, C1, key=61)
    mu, pi, q = backend2.get_evo()
    assert mu.tolist() == [r.mu, r.mu] and pi.tolist() == [r.pi.tolist()] * 2                # the new model on every partition
    want = d.hky_q_matrix(r.kappa, r.pi)                                                       # (the run driver's arithmetic, mirrored in Python)
    assert np.array_equal(q[0], q[1]) and np.allclose(q[0], want, rtol=4e-16, atol=0)
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*kappa"):
        backend2.subst_moves(dataclasses.replace(SPEC, kappa=-1.0), T2, M2, C1, key=61)
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*positive rate"):
        backend2.subst_moves(SPEC, np.zeros((2, 4)), M2, C1, key=61)
    again = backend2.get_evo()
    assert all(np.array_equal(x, y) for x, y in zip(again, (mu, pi, q)))
    assert np.array_equal(backend2.nu_l(), np.ones(L))                                     # the site rates stay


# ---- the mu draw -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,alpha", [("shape 0.5", np.zeros((1, 4, 4), np.int64), 0.5), ("shape 1", np.zeros((1, 4, 4), np.int64), 1.0),
                                           ("shape 1e5", 1590 * M1, 1.0)], ids=lambda v: v if isinstance(v, str) else "")
def test_the_mu_draws_follow_their_gamma(backend, name, M, alpha):
    """500 fixed keys, one draw each (rounds = 0): KS against Gamma(shape, rate), first shown on the CPU restatement of the stream at these keys."""
    keys = np.arange(7000, 7500, dtype=np.uint64)
    spec = dataclasses.replace(SPEC, mu_prior_alpha=alpha, mu_prior_beta=0.25, rounds=0)
    draws, shape, rate = [], None, None
    for key in keys:
        r = backend.subst_moves(spec, T1, M, C1, key=int(key))
        draws.append(r.mu_draw); shape, rate = r.mu_post_shape, r.mu_post_rate
        assert r.mu == r.mu_draw
    off = sum(int(M[0][a][b]) for a in range(4) for b in range(4) if a != b)
    assert shape == off + alpha and (name != "shape 1e5" or 9e4 < shape < 1.2e5)
    dist = sst.gamma(shape, scale=1.0 / rate)
    cpu = RS.gamma_draw(keys, ID_MU, shape, rate)
    assert sst.kstest(cpu, dist.cdf).pvalue > KS_P                                            # the keys' own
    assert np.allclose(draws, cpu, rtol=1e-9, atol=0)
    assert sst.kstest(np.asarray(draws), dist.cdf).pvalue > KS_P


# ---- the sampler as a whole ------------------------------------------------------------------------------------------------------
BURN_IN = 100                    # calls before the chain is recorded
T_BIG, M_BIG, C_BIG = 100.0 * T1, 60 * M1, 20 * C1          # a few thousand mutations: posterior widths near the 0.01 step


def _q_arrays(kappa, p):
    """q[a][b] of the HKY model for arrays of kappa and pi (p: four arrays), float64."""
    r = lambda a, b: 0.0 if a == b else (kappa if (a ^ b) == 2 else 1.0)
    R = sum(p[a] * r(a, b) * p[b] for a in range(4) for b in range(4))
    return [[r(a, b) / R * p[b] for b in range(4)] for a in range(4)]


def _log_G(mu, kappa, p, T, M, C=None):
    """log G up to a constant, as a function of the model: -mu sum q_a T_a + sum M_ab log q_ab (+ sum C_a log pi_a)."""
    q = _q_arrays(kappa, p)
    Mab = M.sum(axis=0); Ta = T.sum(axis=0)
    v = 0.0
    for a in range(4):
        v = v - mu * sum(q[a][b] for b in range(4) if b != a) * Ta[a]
        for b in range(4):
            if a != b and Mab[a, b] > 0:
                v = v + Mab[a, b] * np.log(q[a][b])
        if C is not None:
            v = v + C[a] * np.log(p[a])
    return v


def _chain_check(chain, target, record_property, what):
    """The exp-pop chain test's rule: every mean within 4 batch-means standard errors (40 batches) of the quadrature; and an effective sample size of at least 200."""
    n_batches = 40
    mean = chain.mean(axis=0)
    se = chain.reshape(n_batches, -1, chain.shape[1]).mean(axis=1).std(axis=0, ddof=1) / math.sqrt(n_batches)
    ess = chain.var(axis=0, ddof=1) / se ** 2
    dist = (mean - target) / se
    record_property(what + "_distance_in_standard_errors", [float("%.3g" % v) for v in dist])
    record_property(what + "_effective_sample_size", [float("%.4g" % v) for v in ess])
    print(what, "chain means", mean, "quadrature", target, "se", se, "distance / se", dist, "ESS", ess)
    assert np.all(ess >= 200.0), ess
    assert np.all(np.abs(dist) < 4.0), (mean, target, se, dist)
    return se


def test_the_kappa_chain_samples_its_target(backend, record_property):
    """kappa alone, 2 000 successive calls of 20 rounds, each from the last result: E[log kappa] against a 1-D quadrature of exp(log G(kappa)) x the
    log-normal prior (mean 1, sigma 1.25; the scaling move's Hastings term makes the target a density in kappa, so in x = log kappa it carries kappa)."""
    n_calls = 2000
    spec = dataclasses.replace(SPEC, do_mu=False, do_pi=False, rounds=20)
    chain = np.zeros((n_calls, 1)); acc = 0
    kappa = 2.0
    for i in range(-BURN_IN, n_calls):                                    # (the start is no draw from the target)
        r = backend.subst_moves(dataclasses.replace(spec, kappa=kappa), T_BIG, M_BIG, C_BIG, key=0x5EED0000 + BURN_IN + i)
        kappa = r.kappa
        if i >= 0:
            chain[i, 0] = math.log(kappa); acc += r.kappa_accepted
    lo, hi = chain.min() - 1.0, chain.max() + 1.0

    def quad(n):
        x = np.linspace(lo, hi, n); k = np.exp(x)
        logp = _log_G(1e-3, k, [np.full_like(k, v) for v in PI0], T_BIG, M_BIG) - (x - 1.0) ** 2 / (2 * 1.25 ** 2) - x + x
        w = np.exp(logp - logp.max()); w /= w.sum()
        return np.array([(w * x).sum()]), w
    fine, w = quad(20001); coarse, _ = quad(10001)
    se = _chain_check(chain, fine, record_property, "kappa")
    assert abs(fine - coarse) < 0.1 * se and w[0] + w[-1] < 1e-9
    assert 0.02 < acc / (n_calls * spec.rounds) < 0.9


def test_the_pi_chain_samples_its_target(backend, record_property):
    """pi alone, 2 000 successive calls of 20 rounds: E[pi_A], E[pi_C], E[pi_G] against a quadrature of exp(log G(pi)) on the simplex (uniform prior,
    symmetric delta exchange), a box of +- 7 posterior widths around the chain's mean."""
    n_calls = 2000
    spec = dataclasses.replace(SPEC, do_mu=False, do_kappa=False, rounds=20)
    chain = np.zeros((n_calls, 3)); acc = 0
    pi = PI0
    for i in range(-BURN_IN, n_calls):
        r = backend.subst_moves(dataclasses.replace(spec, pi=tuple(pi)), T_BIG, M_BIG, C_BIG, key=0x5EED8000 + BURN_IN + i)
        pi = r.pi
        if i >= 0:
            chain[i] = pi[:3]; acc += r.pi_accepted
    mid, sd = chain.mean(axis=0), chain.std(axis=0)

    def quad(n):
        ax = [np.linspace(mid[k] - 7 * sd[k], mid[k] + 7 * sd[k], n) for k in range(3)]
        p0, p1, p2 = np.meshgrid(*ax, indexing="ij"); p3 = 1.0 - p0 - p1 - p2
        logp = _log_G(1e-3, 2.0, [p0, p1, p2, p3], T_BIG, M_BIG, C_BIG)
        w = np.exp(logp - logp.max()); w /= w.sum()
        edge = w[0].sum() + w[-1].sum() + w[:, 0].sum() + w[:, -1].sum() + w[:, :, 0].sum() + w[:, :, -1].sum()
        return np.array([(w * p0).sum(), (w * p1).sum(), (w * p2).sum()]), edge
    assert np.all(mid - 7 * sd > 0.0) and mid.sum() + 7 * sd.sum() < 1.0                          # the box lies inside the simplex
    fine, edge = quad(81); coarse, _ = quad(41)
    se = _chain_check(chain, fine, record_property, "pi")
    assert np.all(np.abs(fine - coarse) < 0.1 * se) and edge < 1e-6
    assert 0.002 < sd.min() and sd.max() < 0.03                                                   # widths near the 0.01 step
    assert 0.05 < acc / (n_calls * spec.rounds) < 0.95


# ---- the statistics of the parts on the handle -------------------------------------------------------------------------------------
def _dense_scenario():
    """60 tips, 300 sites, about two hundred mutations, gaps."""
    par = d.SynthParams(num_tips=60, num_sites=300, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=4e-2 / 365.0, gaps_per_tip=2, mean_gap_len=10.0, seed=4242)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, tmax = d.make_synthetic_emat(par)
    return Scenario("dense", tree, ref, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, par.pop_n0, 0.0, 0.0), 300)


def _with_root_missations(part, num_sites):
    """`part` with two missation intervals more at its root, one of several sites and one of a single site, over sites nothing in the part touches (no
    mutation, no delta of the root, no missation of any node): the part as it would be were those sites missing in every tip below."""
    free = np.ones(num_sites, bool)
    free[part.mut_site[: part.mut_offset[part.num_nodes]]] = False
    for s, e in zip(part.miss_start[: part.miss_offset[part.num_nodes]], part.miss_end[: part.miss_offset[part.num_nodes]]):
        free[s:e] = False
    runs, l = [], 0
    while l < num_sites:
        if free[l]:
            e = l
            while e < num_sites and free[e]:
                e += 1
            runs.append((l, e)); l = e
        else:
            l += 1
    long_run = max(runs, key=lambda r: r[1] - r[0])
    single = next(r for r in runs if r != long_run)
    assert long_run[1] - long_run[0] >= 2
    new = sorted([long_run, (single[0], single[0] + 1)])
    r = part.root
    at = int(part.miss_offset[r + 1])
    n_iv = int(part.miss_offset[part.num_nodes])
    own = list(zip(part.miss_start[int(part.miss_offset[r]): at].tolist(), part.miss_end[int(part.miss_offset[r]): at].tolist()))
    merged = sorted(own + new)
    start = np.concatenate([part.miss_start[: int(part.miss_offset[r])], [s for s, _ in merged], part.miss_start[at: n_iv]]).astype(np.int32)
    end = np.concatenate([part.miss_end[: int(part.miss_offset[r])], [e for _, e in merged], part.miss_end[at: n_iv]]).astype(np.int32)
    off = part.miss_offset.copy(); off[r + 1:] += len(new)
    return dataclasses.replace(part, miss_offset=off, miss_start=start, miss_end=end)


@pytest.fixture(scope="module")
def dense():
    sc = _dense_scenario()
    parts, incl, seeds, root_part, ref = split_parts(sc, 3, 9)
    assert len(parts) == 3 and sc.tree.mut_site.shape[0] > 100
    below = max((k for k in range(3) if k != root_part), key=lambda k: parts[k].mut_offset[parts[k].root + 1] - parts[k].mut_offset[parts[k].root])
    parts = parts + [_with_root_missations(parts[below], sc.num_sites)]     # [3]: a part cut from below the root, its root with deltas AND missations
    seeds = list(seeds) + [seeds[below]]
    rng = np.random.default_rng(3)
    nu = 0.3 + 1.5 * rng.random(sc.num_sites)
    models = {1: (None, None), 2: (nu, (np.array([sc.mu, sc.mu]), np.stack([np.asarray(PI, np.float64)] * 2), np.stack([d.hky_q_matrix(KAPPA, PI)] * 2), (np.arange(sc.num_sites) // 7) % 2))}
    exact = {}
    for P, (nu_l, evo) in models.items():
        ev = X.Evo.of(sc, nu_l, evo)
        exact[P] = (ev, [X.stats(p, ref, ev) for p in parts], [np.sum(np.asarray(X.Derived(p, ref, ev).root_state_counts()), axis=0) for p in parts])
    return dict(sc=sc, parts=parts, incl=incl, seeds=seeds, root_part=root_part, ref=ref, models=models, exact=exact)


def _part_list(dn, count):
    """`count` parts for one handle: 1 -- a part cut from below the root, whose root carries deltas and missations against the reference
    sequence, uploaded as the run's root; 3 -- the tree's own three; more -- the root part, then the other two again and again (a handle adds up
    whatever parts it is given: the statistics are sums over parts)."""
    rp = dn["root_part"]; others = [k for k in range(3) if k != rp]
    if count == 1:
        return [3], 0
    if count == 3:
        return list(range(3)), rp
    return [rp] + [others[i % 2] for i in range(count - 1)], 0


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("count", [1, 3, REDUCE_THREADS - 1, REDUCE_THREADS, REDUCE_THREADS + 1])
def test_the_parts_statistics_and_the_moves_on_them(dense, count, P, record_property):
    sc, ref = dense["sc"], dense["ref"]
    nu_l, evo = dense["models"][P]
    ev, sts, roots = dense["exact"][P]
    ids, root_at = _part_list(dense, count)
    tally = Tally("device")
    b = d.EmatBackend(sc.num_sites)
    try:
        configure(b, sc, ref, [dense["parts"][k] for k in ids], [i == root_at for i in range(count)], [int(dense["seeds"][k]) ^ i for i, k in enumerate(ids)], root_at, nu_l=nu_l, evo=evo)
        T, M, Cn = b.parts_subst_stats(P)
        tot = sts[ids[0]]
        for k in ids[1:]:
            tot = X.add_stats(tot, sts[k])
        assert np.array_equal(M, tot["num_muts_beta_ab"]) and np.array_equal(Cn, roots[ids[root_at]])
        if count == 1:
            p = dense["parts"][ids[0]]; r = p.root
            assert p.mut_offset[r + 1] > p.mut_offset[r] and p.miss_offset[r + 1] > p.miss_offset[r]       # deltas and missations at the root
            assert not np.array_equal(Cn, np.bincount(np.asarray(ref), minlength=4))
        Tg, Mg, nm = b.global_stats(P)
        assert np.array_equal(Mg, M) and nm == tot["num_muts"]
        for p in range(P):
            for a in range(4):
                tally.check("Ttwiddle_beta_a", tot["Ttwiddle_beta_a"][p][a], T[p, a], "%d parts partition %d state %d" % (count, p, a))
                tally.check("Ttwiddle_beta_a (emat_get_global_stats)", tot["Ttwiddle_beta_a"][p][a], Tg[p, a], "%d parts partition %d state %d" % (count, p, a))
        T_again, M_again, C_again = b.parts_subst_stats(P)
        assert np.array_equal(T, T_again) and np.array_equal(M, M_again) and np.array_equal(Cn, C_again)                 # the same bits in every call
        spec = d.SubstSpec(mu=sc.mu, kappa=KAPPA, pi=PI, rounds=4)
        from_parts = b.parts_subst_moves(spec, key=91, trace=True)
        from_arrays = b.subst_moves(spec, T, M, Cn, key=91, trace=True)
        assert _same(from_parts, from_arrays)
        assert math.isfinite(from_parts.delta_log_G) and from_parts.mu != sc.mu
    finally:
        b.close()
    tally.finish(record_property)


def test_the_totals_move_by_the_reported_delta_log_G(dense, record_property):
    """recalc_derived and get_totals before and after a call on the tree's own three parts: log G after - log G before = delta_log_G within the sum of
    the exact bounds -- of the two totals, of what the call added step by step, and of the statistics the steps were made from."""
    sc, ref, parts, incl = dense["sc"], dense["ref"], dense["parts"], dense["incl"]
    tally = Tally("device")
    b = d.EmatBackend(sc.num_sites)
    try:
        parts, incl = parts[:3], incl[:3]
        configure(b, sc, ref, parts, incl, dense["seeds"][:3], dense["root_part"])
        ev0 = X.Evo.of(sc)
        b.recalc_derived()
        G0, _ = b.totals()
        T, M, Cn = b.parts_subst_stats(1)
        spec = d.SubstSpec(mu=sc.mu, kappa=KAPPA, pi=PI, rounds=10)
        r = b.parts_subst_moves(spec, key=93, trace=True)
        mirror = _handle(1)
        try:
            r_checked, step_bounds = check_call(mirror, tally, spec, T, M, Cn, key=93, name="totals")       # the same call on the arrays, every number checked
        finally:
            mirror.close()
        assert _same(r, r_checked) and r.pi_accepted + r.kappa_accepted >= 1
        b.recalc_derived()
        G1, _ = b.totals()
        mu, pi, q = b.get_evo()
        assert mu.tolist() == [r.mu] and pi[0].tolist() == r.pi.tolist()
        ev1 = X.Evo(mu, pi, q, np.ones(sc.num_sites), np.zeros(sc.num_sites, np.int32))
        ex0 = [X.Derived(p, ref, ev0).part_log_G(i) for p, i in zip(parts, incl)]
        ex1 = [X.Derived(p, ref, ev1).part_log_G(i) for p, i in zip(parts, incl)]
        exact_delta = sum((e.value for e in ex1), F(0)) - sum((e.value for e in ex0), F(0))
        # the statistics the device's steps read carry their own rounding: an error e_T of a Ttwiddle is an error mu q_a e_T of a step's branch term
        sts = [X.stats(p, ref, ev0) for p in parts]
        T_bound = sum(s["Ttwiddle_beta_a"][0][a].bound() for s in sts for a in range(4))
        q_max = max(float(np.abs(q).max()), float(np.abs(d.hky_q_matrix(KAPPA, PI)).max()))
        stats_bound = (1 + r.pi_accepted + r.kappa_accepted) * 2.0 * max(sc.mu, r.mu) * q_max * T_bound
        # the handle's q is the driver's float64 derivation from (kappa, pi), the steps' deltas are the exact model's: N_Q roundings of every rate
        q_bound = SM.N_Q * X.U * sum(float(e.S) for e in ex0 + ex1)
        allowed = sum(e.bound() for e in ex0) + sum(e.bound() for e in ex1) + step_bounds + stats_bound + q_bound + 4 * X.U * (abs(G0) + abs(G1))
        record_property("totals_error_over_allowed", float("%.3g" % (abs((G1 - G0) - r.delta_log_G) / allowed)))
        assert abs(float(exact_delta) - r.delta_log_G) <= allowed, (float(exact_delta), r.delta_log_G, allowed)
        assert abs((G1 - G0) - r.delta_log_G) <= allowed, (G1 - G0, r.delta_log_G, allowed)
        assert abs(r.delta_log_G) > 1e3 * allowed                           # (the check resolves the change)
    finally:
        b.close()
    tally.finish(record_property)


def test_at_most_one_decision_in_100_was_too_close_to_call(backend, record_property):
    """Over every step this module checked, and over the calls made here (two more keys of every case, so that the test stands when run alone): the
    keys' decisions were first shown callable on the model alone, on the CPU (test_subst_moves_model.py)."""
    tally = Tally("device")
    for name, spec, T, M, C in CASES:
        for key in LAST_KEYS:
            check_call(backend, tally, spec, T, M, C, key=key, name=name)
    tally.finish(record_property)
    assert EXCLUDED["steps"] >= 100 and EXCLUDED["excluded"] * 100 <= EXCLUDED["steps"], EXCLUDED
