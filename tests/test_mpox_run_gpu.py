"""The APOBEC (mpox) model through the parts and the run driver, on a C1-sized tree (60 tips, 2 000 sites, 3 parts): the moves on the statistics of the
parts are the moves on the arrays, the parts' log G moves by the reported delta, whole cycles with the model on keep every derived quantity and the
driver's and the backend's model equal, and a run that turns the model off at the start is the run that never heard of it."""
from fractions import Fraction as F

import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import mpox_moves_model as MM
import skygrid_streams as RS
from delphy_amd.engine import mpox_q_matrices
from delphy_amd.scenarios import make_scenario
from helpers import configure, replay_device_parts_in_the_oracle, split_parts
from test_exact_model import Tally
from test_mpox_run_host import apobec_partition, tip0_sequence

pytestmark = pytest.mark.gpu

SPEC = d.MpoxSpec(mu_star=0.0, mu_prior_alpha=1.0, mu_prior_beta=0.0, rounds=10)
KEY_TAG = 0x4D504F584D4F5631     # csrc/emat_run.cpp: "MPOXMOV1"
SEED = 73


@pytest.fixture(scope="module")
def scenario():
    return make_scenario("C1", num_tips=60, num_sites=2000, uncertain_tips=0.2)


def _same(a, b):
    return np.array_equal(a.trace, b.trace) and all(getattr(a, f) == getattr(b, f) for f in (
        "mu", "mu_star", "M", "M_star", "Ttwiddle", "Ttwiddle_star", "delta_log_G", "delta_log_other_priors", "rho_skipped", "rho_degenerate"))


def test_the_moves_on_the_parts_are_the_moves_on_their_statistics_and_log_G_moves_by_the_delta(scenario, record_property):
    sc = scenario
    parts, incl, seeds, root_part, ref = split_parts(sc, 3, 9)
    assert len(parts) == 3
    pfs = apobec_partition(tip0_sequence(sc.tree, sc.ref)[0])
    rho0 = 0.5
    q0, q1 = mpox_q_matrices(rho0)
    evo = (np.array([sc.mu, sc.mu]), np.full((2, 4), 0.25), np.stack([q0, q1]), pfs)
    tally = Tally("device")
    b = d.EmatBackend(sc.num_sites)
    mirror = d.EmatBackend(sc.num_sites)
    try:
        configure(b, sc, ref, parts, incl, seeds, root_part, evo=evo)
        b.recalc_derived()
        G0, _ = b.totals()
        T, M, _ = b.parts_subst_stats(2)
        assert M[1, 1, 3] + M[1, 2, 0] >= 1 and T[1, 1] + T[1, 2] > 0.0 and 0 < pfs.sum() < sc.num_sites
        spec = d.MpoxSpec(mu=sc.mu, mu_star=rho0 * sc.mu, rounds=10)
        assert spec.mu_star / spec.mu == rho0
        r = b.parts_mpox_moves(spec, key=93, trace=True)
        mirror.set_ref_sequence(ref); mirror.set_evo(*evo[:3], np.ones(sc.num_sites), pfs)
        from_arrays = mirror.mpox_moves(spec, T, M, key=93, trace=True)
        assert _same(r, from_arrays)                                      # bit for bit
        step_bounds = MM.check_call(tally, from_arrays, spec, T, M, 93, "totals")       # ... and every number of it checked
        assert r.rho_degenerate == 0 and r.rho_skipped == 0 and r.mu != sc.mu
        b.recalc_derived()
        G1, _ = b.totals()
        mu, pi, q = b.get_evo()
        assert mu.tolist() == [r.mu, r.mu] and np.array_equal(q[1], mpox_q_matrices(r.mu_star / r.mu)[1])
        ones = np.ones(sc.num_sites)
        ev0 = X.Evo(evo[0], evo[1], evo[2], ones, pfs); ev1 = X.Evo(mu, pi, q, ones, pfs)
        ex0 = [X.Derived(p, ref, ev0).part_log_G(i) for p, i in zip(parts, incl)]
        ex1 = [X.Derived(p, ref, ev1).part_log_G(i) for p, i in zip(parts, incl)]
        exact_delta = sum((e.value for e in ex1), F(0)) - sum((e.value for e in ex0), F(0))
        # the bound the substitution-model moves' totals test uses for the same statement: the two totals', what the call added round by round, the
        # statistics' own rounding (an error e_T of a Ttwiddle is an error mu q_a e_T of a round's branch term, two draws a round), and the handle's q,
        # a float64 derivation from rho (2 roundings of a rate)
        sts = [X.stats(p, ref, ev0) for p in parts]
        T_bound = sum(s["Ttwiddle_beta_a"][p][a].bound() for s in sts for p in range(2) for a in range(4))
        q_max = max(float(np.abs(q).max()), float(np.abs(evo[2]).max()))
        stats_bound = (1 + 2 * spec.rounds) * 2.0 * max(sc.mu, float(r.trace["mu_draw"].max())) * q_max * T_bound
        q_bound = 2 * X.U * sum(float(e.S) for e in ex0 + ex1)
        allowed = sum(e.bound() for e in ex0) + sum(e.bound() for e in ex1) + step_bounds + stats_bound + q_bound + 4 * X.U * (abs(G0) + abs(G1))
        record_property("totals_error_over_allowed", float("%.3g" % (abs((G1 - G0) - r.delta_log_G) / allowed)))
        assert abs(float(exact_delta) - r.delta_log_G) <= allowed, (float(exact_delta), r.delta_log_G, allowed)
        assert abs((G1 - G0) - r.delta_log_G) <= allowed, (G1 - G0, r.delta_log_G, allowed)
        assert abs(r.delta_log_G) > 1e3 * allowed                         # (the check resolves the change)
    finally:
        b.close(); mirror.close()
    tally.finish(record_property)


def _run(sc, device_tree, seed=SEED):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(3); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(device_tree)
    return b, run


def _round_key(k, seed=SEED):
    """keyed_round: the first 64-bit word of Philox4x32-10(counter = rounds so far, key = run seed ^ the group's tag)."""
    w = RS.philox4x32_10(np.uint64(k), np.uint64(seed ^ KEY_TAG))
    return int(w[0]) | (int(w[1]) << 32)


def _same_tree(a, b):
    (ta, ra), (tb, rb) = a, b
    return np.array_equal(ra, rb) and all(np.array_equal(getattr(ta, f), getattr(tb, f)) for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t"))


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_five_whole_cycles_with_the_model_on(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b, run = _run(sc, device_tree)
    try:
        run.set_mpox(True, SPEC)
        run.set_paranoid(True)                                             # check_derived on every part after every pass (raises when one is off)
        pfs, count = run.mpox_partition()
        assert np.array_equal(pfs, apobec_partition(tip0_sequence(sc.tree, sc.ref)[0])) and 0 < count < sc.num_sites
        assert run.mpox() == (sc.mu, 0.0)
        seen = [run.mpox()]
        for k in range(5):
            run.do_mcmc_steps(per_cycle, per_cycle)
            mu, mu_star = run.mpox()
            run.repartition()                                              # (the parts out again, and the model as the driver holds it beside the backend's)
            hm, hp, hq = b.get_evo()
            q0, q1 = mpox_q_matrices(mu_star / mu)
            assert hm.tolist() == [mu, mu] and hp.tolist() == [[0.25] * 4] * 2 and np.array_equal(hq[0], q0) and np.array_equal(hq[1], q1), k
            run.reassemble()
            assert np.array_equal(run.mpox_partition()[0], pfs), k         # the partition drawn at enabling stays
            seen.append((mu, mu_star))
        assert len(set(seen)) == 6 and all(np.isfinite(m) and m > 0.0 and s >= 0.0 for m, s in seen) and seen[-1][1] > 0.0
        kappa, pi = run.hky()[1:]
        assert (kappa, pi.tolist()) == (sc.kappa, list(sc.pi))            # the HKY model rests
        run.set_mpox(False)
        assert run.hky()[0] == seen[-1][0]                                 # mu goes back to the HKY model (run.cpp:395)
        run.repartition()
        assert b.get_evo()[0].tolist() == [seen[-1][0]] and np.allclose(b.get_evo()[2][0], d.hky_q_matrix(sc.kappa, sc.pi), rtol=4e-16, atol=0)      # one partition again
        run.reassemble()
        run.do_mcmc_steps(per_cycle, per_cycle)                            # ... and a cycle on it passes its checks
        assert run.hky()[0] == seen[-1][0]
    finally:
        run.close(); b.close()


def test_three_cycles_move_for_move_against_the_oracle_under_the_models_the_device_drew(scenario):
    """repartition(); mpox_moves(); then a pass of 3 x 600 + 7 local moves replayed in the oracle under the model the backend holds (get_evo) over the driver's
    site partition; reassemble().  From the second cycle on mu* > 0: the matrices are those the device's own Gibbs rounds made."""
    sc = scenario
    b = d.EmatBackend(sc.num_sites, trace_moves=700)
    run = d.EmatRun(b, sc.tree, sc.ref, SEED)
    run.set_num_parts(3); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    try:
        run.set_mpox(True, SPEC)
        ref, models = sc.ref, []
        for k in range(3):
            run.repartition()
            run.mpox_moves()
            mu, pi, q = b.get_evo()
            pfs, count = run.mpox_partition()
            m, m_star = run.mpox()
            assert mu.tolist() == [m, m] and np.array_equal(q[1], mpox_q_matrices(m_star / m)[1]) and 0 < count < sc.num_sites
            if k >= 1:
                assert m_star > 0.0
            models.append((m, m_star))
            n = replay_device_parts_in_the_oracle(sc, b, run, ref, 3 * 600 + 7, 700, evo=(mu, pi, q, pfs))
            assert n == 3
            run.reassemble()
            _, ref = run.tree()
        assert len(set(models)) == 3
    finally:
        run.close(); b.close()


def test_every_rounds_key_is_keyed_rounds_and_the_refusals(scenario):
    sc = scenario
    b, run = _run(sc, True)
    b2, byhand = _run(sc, True)
    try:
        run.set_mpox(True, SPEC); byhand.set_mpox(True, SPEC)
        with pytest.raises(d.EmatError, match="STATE.*repartition first"):
            run.mpox_moves()                                               # nothing cut yet
        for k in range(2):
            run.repartition(); byhand.repartition()
            mu, mu_star = run.mpox()
            res = run.mpox_moves(trace=True)
            want = b2.parts_mpox_moves(d.MpoxSpec(mu=mu, mu_star=mu_star, rounds=SPEC.rounds), key=_round_key(k), trace=True)
            assert _same(res, want) and len(res.trace) == SPEC.rounds, k
            assert run.mpox() == (res.mu, res.mu_star)
            assert all(np.array_equal(x, y) for x, y in zip(b.get_evo(), b2.get_evo()))
            held = [x.copy() for x in b.get_evo()]
            run.push_params()                                              # the whole model again, from the driver's copy
            assert all(np.array_equal(x, y) for x, y in zip(held, b.get_evo()))
            run.reassemble(); byhand.reassemble()
            with pytest.raises(d.EmatError, match="STATE.*repartition first"):
                run.mpox_moves()                                           # assembled again; a refusal draws no key
        run.repartition()
        run.set_mpox(False)                                                # off at any time ...
        with pytest.raises(d.EmatError, match="STATE.*emat_run_set_mpox.*reassemble first"):
            run.set_mpox(True, SPEC)                                       # ... on only with the tree assembled: the sequence at node 0 is read from it
        run.reassemble()
        run.set_mpox(True, SPEC)
    finally:
        run.close(); byhand.close(); b.close(); b2.close()


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_turned_off_at_the_start_the_run_is_the_run_that_never_heard_of_the_model(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, off = _run(sc, device_tree)
    b2, never = _run(sc, device_tree)
    try:
        off.set_mpox(False, SPEC)
        for _ in range(3):
            off.do_mcmc_steps(per_cycle, per_cycle); never.do_mcmc_steps(per_cycle, per_cycle)
            assert _same_tree(off.tree(), never.tree())
        assert off.hky()[0] == sc.mu
        off.repartition(); never.repartition()
        b1.recalc_derived(); b2.recalc_derived()
        assert b1.totals() == b2.totals() and all(np.isfinite(v) for v in b1.totals())
        assert all(np.array_equal(x, y) for x, y in zip(b1.get_evo(), b2.get_evo())) and b1.get_evo()[0].shape == (1,)
        off.reassemble(); never.reassemble()
    finally:
        off.close(); never.close(); b1.close(); b2.close()


def test_a_sharded_run_is_refused(scenario):
    sc = scenario
    b, run = _run(sc, False)
    try:
        run.set_mpox(True, SPEC)
        run.set_shard(0, 2)
        run.repartition()
        with pytest.raises(d.EmatError, match="STATE.*sharded run"):
            run.mpox_moves()
    finally:
        run.close(); b.close()
