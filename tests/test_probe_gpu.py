"""The tree probers on the tree resident in HBM (emat_tree_probe_ancestors, _probe_site_states, _branch_counts) against the
reference's own fixtures and against tests/prober_model.py, the Python restatement that test_prober_model.py pins to them.

Error bounds (derived, not tuned).  Branch counts: the device adds every fractional term in fixed point with quantum
q = 2^-f (f = min(52, 61 - ceil(log2(n + 1))), n nodes), each term rounded once: its cell sum is within B q / 2 of the exact
sum of the terms, B = fractional terms the cell received; it is then rounded to double once (u = 2^-53 relative).  The model
adds doubles one at a time: A additions into a cell (whole and fractional) leave it within A u (cell total) of the exact sum,
to first order.  So |device - model| <= B q / 2 + (A + 1) u total, asserted with SAFETY = 2; a cell that received no
fractional term must be the same integer on both sides exactly.  Probabilities: against the model run on the DEVICE's counts
(Tree_prober alone) 1e-12 absolute, what DESIGN.md records for device exp / log against glibc; end to end the counts' relative
error eps (the bound above over the cell total) moves a cell's coalescence probability by at most eps / e and a member's share
by 2 eps, and the recurrence is a convex combination, so the errors of the cells add up: 1e-12 + 3 eps cells.

Measured maxima are printed (pytest -s, or the captured output of a failure) for DESIGN.md section 9."""
import math
import time

import numpy as np
import pytest

import delphy_amd as d
import prober_model as M
from delphy_amd.scenarios import _skygrid, make_scenario
from prober_golden import G, check_prober_case, flat_tree, pop_model

pytestmark = pytest.mark.gpu

SAFETY = 2.0
U = 2.0 ** -53
P_TOL = 1e-12


def _quantum(num_nodes):
    return 2.0 ** -min(52, 61 - math.ceil(math.log2(num_nodes + 1)))


def _backend(sc_or_sites, tree=None, ref=None):
    if tree is None:
        tree, ref, sites = sc_or_sites.tree, sc_or_sites.ref, sc_or_sites.num_sites
    else:
        sites = sc_or_sites
    b = d.EmatBackend(sites)
    b.set_ref_sequence(ref)
    b.tree_upload(tree)
    return b


# ---- 1. the reference's fixtures on the device ----------------------------------------------------------------------
@pytest.mark.parametrize("case", G["ancestral_tree_prober"]["cases"], ids=lambda c: c["test"])
def test_reference_ancestral_fixtures_on_the_device(case):
    A = G["ancestral_tree_prober"]
    tree, ref = flat_tree(A["tree"])
    b = _backend(len(ref), tree, ref)
    try:
        for name in case["pops"]:
            p = b.tree_probe_ancestors(pop_model(A["pops"][name]), case["marked"], case["t_start"], case["t_end"], case["num_t_cells"])
            assert p.shape[0] == len(case["marked"]) + 1
            check_prober_case(case, p, "%s / %s" % (case["test"], name))
            want = M.probe_ancestors_on_tree(tree, M.OraclePop(pop_model(A["pops"][name])), case["marked"], case["t_start"], case["t_end"], case["num_t_cells"])
            assert np.max(np.abs(p - want)) <= P_TOL
    finally:
        b.close()


@pytest.mark.parametrize("case", G["site_states_tree_prober"], ids=lambda c: c["test"])
def test_reference_site_state_fixtures_on_the_device(case):
    tree, ref = flat_tree(case["tree"])
    b = _backend(len(ref), tree, ref)
    try:
        p = b.tree_probe_site_states(pop_model(case["pop"]), case["site"], case["t_start"], case["t_end"], case["num_t_cells"])
        check_prober_case(case, p, case["test"])
        want = M.probe_site_states_on_tree(tree, ref, M.OraclePop(pop_model(case["pop"])), case["site"], case["t_start"], case["t_end"], case["num_t_cells"])
        assert np.max(np.abs(p - want)) <= P_TOL
    finally:
        b.close()


def test_device_intensity_integral_against_the_oracle():
    """dev::pop_intensity_integral (emat_debug_pop op 2) point by point against orc_intensity_integral, on the inputs where population
    code goes wrong (exact_model.adversarial_pop_cases): the two differ by their exp / expm1 / log only, 1e-12 relative."""
    import exact_model as X
    b = d.EmatBackend(100)
    worst = 0.0
    try:
        for name, pm, a, bb in X.adversarial_pop_cases():
            got = b.debug_pop(pm, 2, a, bb)
            orc = M.OraclePop(pm)
            for i in range(a.shape[0]):
                want = orc.intensity_integral(float(a[i]), float(bb[i]))
                err = abs(got[i] - want) / max(abs(want), 1e-300) if want != got[i] else 0.0
                worst = max(worst, err)
                assert err <= 1e-12, (name, a[i], bb[i], got[i], want)
    finally:
        b.close()
    print("intensity_integral: largest relative difference device / oracle %.3g" % worst)


# ---- 2. + 3. branch counts and probabilities against the model --------------------------------------------------------
def _selections(sc, rng):
    """[(label, marked or None, site or None)]: k = 1, 7, 64 marked nodes plus a -1 and a duplicate; a site without mutations, the
    site with the most, and a site mutated on a branch that hangs off the root if there is one."""
    tree = sc.tree
    n = tree.num_nodes
    out = []
    for k in (1, 7, 64):
        mk = [int(v) for v in rng.choice(n, size=k, replace=False)]
        out.append(("k=%d" % k, mk + [-1, mk[0]], None))
    per_site = np.bincount(tree.mut_site[:int(tree.mut_offset[n])], minlength=sc.num_sites)
    out.append(("site without mutations", None, int(rng.choice(np.flatnonzero(per_site == 0)))))
    out.append(("site with most mutations", None, int(rng.choice(np.flatnonzero(per_site == per_site.max())))))
    below_root = [int(tree.mut_site[j]) for c in (tree.child0[tree.root], tree.child1[tree.root]) for j in range(int(tree.mut_offset[c]), int(tree.mut_offset[c + 1]))]
    if below_root:
        out.append(("site mutated next to the root", None, int(rng.choice(sorted(set(below_root))))))
    return out


def _pops(sc):
    n0 = 0.5 * (sc.t_max_tip - float(sc.tree.t[sc.tree.root]))
    return [("constant", d.PopModel.const(n0)), ("exponential", d.PopModel.exp(sc.t_max_tip, n0, 3.0 / max(n0, 1.0), 0.01 * n0)),
            ("skygrid", _skygrid(sc.t_max_tip, 2.4 * n0, n0, knots=20, log_linear=True))]


def _check_counts(got, fam, quantum, what):
    want, B, A = fam.array(), fam.touched(), fam.adds()
    whole = B == 0
    assert np.array_equal(got[whole], want[whole]) and np.array_equal(got[whole], np.round(got[whole])), what + ": whole cells"
    bound = B * quantum / 2 + (A + 1) * U * np.abs(want)
    err = np.abs(got - want)
    ratio = float(np.max(err[~whole] / bound[~whole])) if np.any(~whole) else 0.0
    assert ratio <= SAFETY, "%s: count error %.3g of its bound" % (what, ratio)
    tot = want.sum(axis=0)
    eps = float(np.max(SAFETY * bound.sum(axis=0)[tot > 0] / tot[tot > 0])) if np.any(tot > 0) else 0.0
    return ratio, eps


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_branch_counts_and_probabilities_against_the_model(name):
    sc = make_scenario(name)
    tree, n = sc.tree, sc.tree.num_nodes
    rng = np.random.default_rng(20261016)
    t_root, span = float(tree.t[tree.root]), sc.t_max_tip - float(tree.t[tree.root])
    quantum = _quantum(n)
    worst_ratio = worst_chain = worst_e2e = 0.0
    b = _backend(sc)
    try:
        for label, marked, site in _selections(sc, rng):
            for cells in (50, 1000):
                for t_start in (t_root - 0.1 * span, t_root + 0.3 * span):
                    t_end = sc.t_max_tip + 0.01 * span
                    what = "%s %s cells=%d t_start=%.6g" % (name, label, cells, t_start)
                    if marked is not None:
                        fam, skip = M.ancestors_branch_counts(tree, marked, t_start, t_end, cells)
                        got, got_skip, x0 = b.tree_branch_counts(t_start, t_end, cells, marked_nodes=marked)
                        p_initial = [0.0] * len(marked) + [1.0]
                    else:
                        fam, skip, root_state = M.site_states_branch_counts(tree, sc.ref, site, t_start, t_end, cells)
                        got, got_skip, x0 = b.tree_branch_counts(t_start, t_end, cells, site=site)
                        p_initial = [float(s == root_state) for s in range(4)]
                    assert (t_start > t_root) == (skip > 0)
                    assert got_skip == skip and x0 == fam.x_start and got.shape == (len(fam), fam.num_cells), what      # the same doubles, not nearly the same
                    ratio, eps = _check_counts(got, fam, quantum, what)
                    worst_ratio = max(worst_ratio, ratio)
                    dev_fam = M.StaircaseFamily.from_array(got, fam.x_start, fam.cell_size)
                    for pop_name, pop in _pops(sc):
                        p = b.tree_probe_ancestors(pop, marked, t_start, t_end, cells) if marked is not None else b.tree_probe_site_states(pop, site, t_start, t_end, cells)
                        orc = M.OraclePop(pop)
                        chain = float(np.max(np.abs(p - M.tree_prober(dev_fam, skip, orc, p_initial))))
                        e2e = float(np.max(np.abs(p - M.tree_prober(fam, skip, orc, p_initial))))
                        worst_chain, worst_e2e = max(worst_chain, chain), max(worst_e2e, e2e)
                        assert chain <= P_TOL, "%s %s: Tree_prober on the device's counts off by %.3g" % (what, pop_name, chain)
                        assert e2e <= P_TOL + 3.0 * eps * fam.num_cells, "%s %s: end to end off by %.3g (eps %.3g)" % (what, pop_name, e2e, eps)
    finally:
        b.close()
    print("%s (%d nodes, quantum 2^%d): largest count error / bound %.3g; probabilities: %.3g on the device's counts, %.3g end to end"
          % (name, n, round(math.log2(quantum)), worst_ratio, worst_chain, worst_e2e))


# ---- 4. properties ------------------------------------------------------------------------------------------------------
def _check_properties(p, what):
    assert np.all(p >= 0.0) and np.all(p <= 1.0), what
    tot = np.zeros(p.shape[1])
    for r in p:
        tot = tot + r
    assert np.all(np.abs(tot - 1.0) <= 1e-12), (what, float(np.max(np.abs(tot - 1.0))))


def test_properties_that_need_no_model():
    sc = make_scenario("C2")
    tree = sc.tree
    rng = np.random.default_rng(7)
    t_root = float(tree.t[tree.root])
    marked = [int(v) for v in rng.choice(tree.num_nodes, size=16, replace=False)]
    b = _backend(sc)
    try:
        for t_start in (t_root - 20.0, t_root + 100.0):
            args = (t_start, sc.t_max_tip + 1.0, 200)
            p = b.tree_probe_ancestors(sc.pop, marked, *args)
            _check_properties(p, "ancestors")
            assert np.array_equal(p, b.tree_probe_ancestors(sc.pop, marked, *args))           # identical bits from call to call
            s = b.tree_probe_site_states(sc.pop, int(tree.mut_site[0]), *args)
            _check_properties(s, "site states")
            assert np.array_equal(s, b.tree_probe_site_states(sc.pop, int(tree.mut_site[0]), *args))
            c1, _, _ = b.tree_branch_counts(*args, marked_nodes=marked)
            c2, _, _ = b.tree_branch_counts(*args, marked_nodes=marked)
            assert np.array_equal(c1, c2)
            none = b.tree_probe_ancestors(sc.pop, [], *args)
            root = b.tree_probe_ancestors(sc.pop, [tree.root], *args)
            assert none.shape == (1, 200)
            _check_properties(none, "nothing marked")                       # "none" holds everything there is
            # marking the root: every branch hangs below it, so member 0 coalesces where "none" did, and "none" keeps only what has not coalesced
            c_none, _, _ = b.tree_branch_counts(*args, marked_nodes=[])
            c_root, _, _ = b.tree_branch_counts(*args, marked_nodes=[tree.root])
            assert np.array_equal(c_root[0], c_none[0]) and not c_root[1].any()
            _check_properties(root, "root marked")
    finally:
        b.close()


# ---- 5. after real cycles -------------------------------------------------------------------------------------------------
def test_probe_after_cycles_of_the_run_driver_and_while_the_parts_are_out():
    sc = make_scenario("C3")
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    run.set_num_parts(128); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    rng = np.random.default_rng(11)
    marked = [int(v) for v in rng.choice(sc.tree.num_nodes, size=7, replace=False)]
    try:
        for cycle in range(3):
            run.repartition()
            if cycle == 1:
                for call in (lambda: b.tree_probe_ancestors(sc.pop, marked, -100.0, sc.t_max_tip, 50), lambda: b.tree_probe_site_states(sc.pop, 0, -100.0, sc.t_max_tip, 50),
                             lambda: b.tree_branch_counts(-100.0, sc.t_max_tip, 50, site=0)):
                    with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_reassemble first"):
                        call()
            run.run_moves(128 * 400); b.synchronize()
            run.reassemble()
        t_root_dev = b.tree_kids()[2]
        args = (t_root_dev + 30.0, sc.t_max_tip + 1.0, 200)
        counts, skip, x0 = b.tree_branch_counts(*args, marked_nodes=marked)
        p = b.tree_probe_ancestors(sc.pop, marked, *args)
        tree, ref = b.tree_download()
        site = int(np.argmax(np.bincount(tree.mut_site, minlength=sc.num_sites)))
        s_counts, s_skip, _ = b.tree_branch_counts(*args, site=site)
        s = b.tree_probe_site_states(sc.pop, site, *args)
    finally:
        run.close(); b.close()
    assert not np.array_equal(tree.t, sc.tree.t)                               # the moves did move the tree
    quantum = _quantum(tree.num_nodes)
    orc = M.OraclePop(sc.pop)
    fam, want_skip = M.ancestors_branch_counts(tree, marked, *args)
    assert skip == want_skip and x0 == fam.x_start
    ratio, eps = _check_counts(counts, fam, quantum, "ancestors after cycles")
    assert np.max(np.abs(p - M.tree_prober(fam, skip, orc, [0.0] * 7 + [1.0]))) <= P_TOL + 3.0 * eps * fam.num_cells
    fam, want_skip, root_state = M.site_states_branch_counts(tree, ref, site, *args)
    assert s_skip == want_skip
    ratio2, eps = _check_counts(s_counts, fam, quantum, "site states after cycles")
    assert np.max(np.abs(s - M.tree_prober(fam, s_skip, orc, [float(k == root_state) for k in range(4)]))) <= P_TOL + 3.0 * eps * fam.num_cells
    print("after three cycles: count error / bound %.3g (ancestors), %.3g (site %d)" % (ratio, ratio2, site))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_text_and_the_next_call_works():
    sc = make_scenario("C1")
    n = sc.tree.num_nodes
    b = _backend(sc)
    good = (sc.pop, [3, -1], -400.0, sc.t_max_tip, 20)
    bad_pop = d.PopModel.const(-1.0)
    no_such_pop = d.PopModel(7, (1.0, 0.0, 0.0, 0.0))
    try:
        for call, text in ((lambda: b.tree_probe_site_states(sc.pop, -1, 0.0, 1.0, 10), "site -1 is outside the valid range"),
                           (lambda: b.tree_probe_site_states(sc.pop, sc.num_sites, 0.0, 1.0, 10), "outside the valid range"),
                           (lambda: b.tree_probe_ancestors(sc.pop, [n + 10], 0.0, 1.0, 10), "neither `none` .-1. nor inside the valid range"),
                           (lambda: b.tree_probe_ancestors(sc.pop, [-2], 0.0, 1.0, 10), "neither `none`"),
                           (lambda: b.tree_probe_ancestors(sc.pop, [0], -3.5, -4.5, 10), "need t_start < t_end"),
                           (lambda: b.tree_probe_ancestors(sc.pop, [0], 1.0, 1.0, 10), "need t_start < t_end"),
                           (lambda: b.tree_probe_site_states(sc.pop, 0, 0.0, 1.0, 0), "number of cells should be positive"),
                           (lambda: b.tree_branch_counts(0.0, 1.0, -3, site=0), "number of cells should be positive"),
                           (lambda: b.tree_probe_ancestors(bad_pop, [0], 0.0, 1.0, 10), "Population size should be positive"),
                           (lambda: b.tree_probe_site_states(no_such_pop, 0, 0.0, 1.0, 10), "unknown population model kind")):
            with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*" + text):
                call()
            p = b.tree_probe_ancestors(*good)                                  # a good call still works
            assert p.shape == (3, 20) and np.all(np.abs(p.sum(axis=0) - 1.0) <= 1e-12)
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY"):            # a root a hundred million cells before t_start
            b.tree_probe_ancestors(sc.pop, [0], sc.t_max_tip, sc.t_max_tip + 1e-6, 1)
        assert b.tree_probe_ancestors(*good).shape == (3, 20)
    finally:
        b.close()
    b = d.EmatBackend(sc.num_sites)
    try:
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_upload first"):
            b.tree_probe_ancestors(*good)
    finally:
        b.close()


# ---- 7. full size ---------------------------------------------------------------------------------------------------------
def test_full_size_properties_and_the_cost_next_to_a_download():
    sc = make_scenario("C4")
    tree = sc.tree
    rng = np.random.default_rng(3)
    marked = [int(v) for v in rng.choice(tree.num_nodes, size=16, replace=False)]
    site = int(np.argmax(np.bincount(tree.mut_site, minlength=sc.num_sites)))
    t_root = float(tree.t[tree.root])
    args = (t_root - 1.0, sc.t_max_tip + 1.0, 200)
    b = _backend(sc)

    def median_ms(fn, reps=7):
        fn()                                                                    # warm-up: scratch allocations, code objects
        times = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); times.append(time.perf_counter() - t0)   # every call ends in a device synchronise and a copy
        return 1e3 * float(np.median(times))
    try:
        p = b.tree_probe_ancestors(sc.pop, marked, *args)
        _check_properties(p, "C4 ancestors")
        assert np.array_equal(p, b.tree_probe_ancestors(sc.pop, marked, *args))
        s = b.tree_probe_site_states(sc.pop, site, *args)
        _check_properties(s, "C4 site states")
        assert np.array_equal(s, b.tree_probe_site_states(sc.pop, site, *args))
        ms_anc = median_ms(lambda: b.tree_probe_ancestors(sc.pop, marked, *args))
        ms_site = median_ms(lambda: b.tree_probe_site_states(sc.pop, site, *args))
        ms_down = median_ms(lambda: b.tree_download(), reps=5)
    finally:
        b.close()
    print("C4 (%d nodes, 200 cells), median wall time of a call: probe_ancestors (k = 16) %.3f ms, probe_site_states %.3f ms, tree_download %.3f ms"
          % (tree.num_nodes, ms_anc, ms_site, ms_down))
