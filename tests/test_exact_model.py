"""The CPU oracle against the exact values of tests/exact_model.py, and exact_model against the reference project's own
expectations.  The parity tests compare the HIP engine with the oracle, which evaluates every sum as the engine does: a
mistake made in both is invisible there.  Here each quantity is held to the rounding bound (n + 8) u S of its exact value,
which holds for any order of summation (exact_model's docstring).  A maintained total after M moves gets that bound plus
min(4 M u, 1e-9) of the largest magnitude it held: each accepted move adds a delta whose terms are at most that magnitude
(one rounding of the running sum and a few in the delta).  That magnitude is read where it can be observed: the larger of the
exact values before and after the pass, and the largest value the engine reported at nine points inside it (the pass is run in
ten slices of M / 10 moves).  A peak between two of those points is not seen; the cap at 1e-9 keeps the allowance no looser
than the parity tests' 1e-9 of the same magnitude."""
import json
import math
import os

import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
from delphy_amd.scenarios import make_scenario, random_scenario
from graft_golden import fixture_tree
from helpers import configure, split_parts
from oracle_ffi import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_expectations.json")))


class Tally:
    """Every comparison of one test: worst |err| / (u S) per quantity, the quantities whose rounding bound is looser than
    1e-9 max(1, |x|) (only cancellation does that), and the failures."""

    def __init__(self, who):
        self.who, self.worst, self.worst_abs, self.loose, self.fail = who, {}, {}, set(), []

    def check(self, what, ex: X.Exact, got, where="", allowance=0.0):
        e = ex.err(got)
        if ex.S:
            self.worst[what] = max(self.worst.get(what, 0.0), ex.units(got))
        else:       # S = 0 (a cell no lineage reaches): no scale to count in, so the absolute error is reported
            self.worst_abs[what] = max(self.worst_abs.get(what, 0.0), e)
        u = ex.units(got)
        if ex.bound() + allowance > 1e-9 * max(1.0, abs(float(ex.value))):
            self.loose.add(what)
        if not e <= ex.bound() + allowance:
            self.fail.append("%s %s %s: %r, exact %r: %.3g u S off (S %.3g, bound %d u S%s)" % (
                self.who, what, where, float(got), float(ex.value), u, float(ex.S), ex.n + 8, " + %.3g" % allowance if allowance else ""))

    def equal(self, what, a, b, where=""):
        if not np.array_equal(np.asarray(a), np.asarray(b)):
            self.fail.append("%s %s %s differs" % (self.who, what, where))

    def summary(self):
        return "worst |err|/(u S): " + ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items())) + \
            ("; worst |err| where S = 0: " + ", ".join("%s %.3g" % kv for kv in sorted(self.worst_abs.items())) if self.worst_abs else "") + \
            ("; bound looser than 1e-9 for: " + ", ".join(sorted(self.loose)) if self.loose else "")

    def finish(self, record_property):
        for k, v in sorted(self.worst.items()):
            record_property("%s_worst_units_%s" % (self.who, k), float("%.4g" % v))
        for k, v in sorted(self.worst_abs.items()):
            record_property("%s_worst_abs_where_S_is_0_%s" % (self.who, k), float("%.4g" % v))
        record_property("%s_bound_looser_than_1e-9" % self.who, sorted(self.loose))
        assert not self.fail, "\n".join(self.fail[:25]) + "\n" + self.summary()


# ---- exact_model against the reference project's expectations -----------------------------------------------------------
def _more_digits_than_tol(expected, tol):
    """The fixture states the number to more digits than its tolerance needs."""
    if tol <= 0:
        return True
    places = max(0, int(math.ceil(-math.log10(tol))))
    return round(expected, places) != expected


def _golden_pop(m):
    if m["kind"] == "const":
        return d.PopModel.const(m["pop"])
    if m["kind"] == "exp":
        return d.PopModel.exp(m["t0"], m["n0"], m["g"], m["min_pop"])
    return d.PopModel.skygrid(np.array(m["x"], np.float64), np.array(m["gamma"], np.float64), m["type"] == "log_linear")


def test_exact_population_models_against_the_reference_expectations():
    checked = tight = 0
    for c in G["pop_model"]:
        if c["op"] not in ("pop_at_time", "pop_integral", "log_N"):
            continue
        pop = X.Pop(_golden_pop(c["model"]))
        a = c["args"]
        if c["op"] == "pop_at_time":
            got = pop.pop_at_time(a[0]).f
        elif c["op"] == "log_N":
            got = float(pop.log_N(a[0])[0])
        else:
            got = pop.pop_integral(a[0], a[1]).f
        exp = c["expected"]
        assert abs(got - exp) <= c["tol"] or got == exp, (c, got)
        if _more_digits_than_tol(exp, c["tol"]):
            assert abs(got - exp) <= 1e-13 * max(1.0, abs(exp)), ("the fixture's digits", c, got)
            tight += 1
        checked += 1
    assert checked >= 80 and tight >= 20, (checked, tight)


def _calc_fixture(pi=None):
    fx = dict(G["phylo_tree_calc"]["fixture"])
    ev = fx["evo"]
    evo = X.Evo(ev["mu"], pi if pi is not None else ev["pi"], ev["q"], ev["nu_l"], ev["partition_for_site"])
    return fixture_tree(fx), np.asarray(fx["ref_sequence"], np.uint8), evo


def test_exact_derived_quantities_against_the_reference_expectations():
    PC = G["phylo_tree_calc"]
    tree, ref, evo = _calc_fixture()
    dv = X.Derived(tree, ref, evo)
    brute = X.Derived(tree, ref, evo, brute=True)
    assert dv.lam == brute.lam
    for x, want in enumerate(PC["lambda_i"]["expected"]):
        assert abs(float(dv.lam[x]) - want) <= 1e-14 * abs(want), (x, float(dv.lam[x]), want)   # the fixture's 17 digits, not only its tol
    assert dv.nsm == PC["num_sites_missing"]["expected"]
    below = dv.log_G_below_root()
    want = PC["log_G_below_root"]["expected"]
    assert abs(below.f - want) <= 1e-13 * abs(want), (below, want)
    for case in PC["log_root_prior"]:
        _, _, evo2 = _calc_fixture(case["pi"])
        rp = X.Derived(tree, ref, evo2).log_root_prior()
        if case["expected"] == "-inf":
            assert rp.value == -math.inf
        else:
            assert abs(rp.f - case["expected"]) <= 1e-13 * abs(case["expected"]), (rp, case)
    st = X.stats(tree, ref, evo)
    assert st["num_muts"] == PC["num_muts"] and st["num_muts_beta_ab"].tolist() == PC["num_muts_beta_ab"]
    assert st["num_muts_l"].tolist() == PC["num_muts_l"] and st["T"].f == PC["T"]
    for p, row in enumerate(PC["Ttwiddle_beta_a"]["expected"]):
        for a, want in enumerate(row):
            assert abs(st["Ttwiddle_beta_a"][p][a].f - want) <= 1e-14 * max(1.0, abs(want)), (p, a, st["Ttwiddle_beta_a"][p][a], want)


def test_exact_grid_prior_against_the_reference_expectations():
    from test_golden_reference_expectations import _tree_with_node_times
    sc = G["scalable_coalescent"]
    for stage in sc["stages"]:
        tree = _tree_with_node_times(stage, sc["num_tips"])
        got = X.scalable_log_prior(tree, X.Pop(d.PopModel.const(sc["pop"])), sc["t_ref"], sc["t_step"])
        assert abs(got.f - stage["expected_log_prior"]) <= 1e-13 * abs(stage["expected_log_prior"]), (stage, got)


# ---- the fast path of exact_model against its brute-force path ------------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_exact_lambda_fast_path_equals_the_brute_force_path(case):
    """Every node's whole sequence, site by site, against the root's lambda plus exact branch changes: equal as Fractions,
    on whole trees and on parts cut from them (whose roots carry the deltas from the ref)."""
    rng = np.random.default_rng(900 + case)
    sc, nu_l, evo, what = random_scenario(rng, case, max_tips=40)
    if sc.num_sites > 2000:
        sc, nu_l, evo = make_scenario("C1", num_tips=30, num_sites=600, uncertain_tips=0.3, seed=901 + case), None, None
    ev = X.Evo.of(sc, nu_l, evo)
    fast, brute = X.Derived(sc.tree, sc.ref, ev), X.Derived(sc.tree, sc.ref, ev, brute=True)
    assert fast.lam == brute.lam, what
    parts, incl, seeds, root_part, ref = split_parts(sc, 3, 5 + case)
    for p in parts:
        assert X.Derived(p, ref, ev).lam == X.Derived(p, ref, ev, brute=True).lam, what


# ---- the oracle against the exact values ----------------------------------------------------------------------------
def check_part(tally, eng, p, ref, ev, pop, includes_root, tag, maintained_scale=None, moves=0):
    """Everything one part's from-scratch (or, with `maintained_scale`, maintained) derived quantities and coalescent table
    hold, against the exact values of the tree the engine holds now."""
    tree = eng.part_download(p)
    n = tree.num_nodes
    dv = X.Derived(tree, ref, ev)
    lam, nsm, Gv, Av = eng.part_derived(p, n)
    tally.equal("num_sites_missing", nsm, dv.nsm, "%s part %d" % (tag, p))
    tab = eng.part_coalescent(p)
    exG = dv.part_log_G(includes_root)
    exA = X.partial_log_prior(tree, pop, includes_root, tab)
    if maintained_scale is None:
        for x in range(n):
            tally.check("lambda_i", dv.lambda_i(x), lam[x], "%s part %d node %d" % (tag, p, x))
        tally.check("log_G", exG, Gv, "%s part %d" % (tag, p))
        tally.check("partial_prior", exA, Av, "%s part %d" % (tag, p))
    else:
        per_move = min(4 * moves * X.U, 1e-9)
        sG, sA = maintained_scale
        tally.check("maintained_log_G", exG, Gv, "%s part %d" % (tag, p), per_move * max(sG, abs(exG.f)))
        tally.check("maintained_partial_prior", exA, Av, "%s part %d" % (tag, p), per_move * max(sA, abs(exA.f)))
    kb, kS, kn = X.k_bar_p(tree, includes_root, tab["t_ref"], tab["t_step"], len(tab["k_bar_p"]))
    # k_bar_p is maintained by the moves (recalc_derived leaves it): each move that touches a cell adds a share computed from
    # a cell bound, one rounding of the cell's count and a few of its bound, capped at 1e-9 of the largest count
    kmax = max([1.0] + [abs(float(k)) for k in kb])
    bmax = (abs(tab["t_ref"]) + len(kb) * tab["t_step"]) / tab["t_step"]
    k_allow = min(4 * moves * X.U * (kmax + bmax), 1e-9 * kmax)
    for i in range(len(kb)):
        tally.check("k_bar_p" if not moves else "maintained_k_bar_p", X.Exact(kb[i], kS[i], kn[i]), tab["k_bar_p"][i], "%s part %d cell %d" % (tag, p, i), k_allow)
    return exG, exA, tree


def check_popsize_bar(tally, eng, p, pop, tag):
    """popsize_bar of every cell the part is active in."""
    tab = eng.part_coalescent(p)
    for i in range(len(tab["popsize_bar"])):
        if tab["num_active_parts"][i] > 0:
            tally.check("popsize_bar", X.popsize_bar_vsc(pop, tab["t_ref"], tab["t_step"], i), tab["popsize_bar"][i], "%s part %d cell %d" % (tag, p, i))


def check_stats(tally, eng, trees, ref, ev, tag, per_part_Ttwiddle=True):
    """global_stats and num_muts_l over the parts, Ttwiddle_l of each part, against the exact statistics below each part's root."""
    sts = [X.stats(t, ref, ev) for t in trees]
    tot = sts[0]
    for s in sts[1:]:
        tot = X.add_stats(tot, s)
    T, M, nm = eng.global_stats(ev.num_partitions)
    tally.equal("num_muts", nm, tot["num_muts"], tag)
    tally.equal("num_muts_beta_ab", M, tot["num_muts_beta_ab"], tag)
    for p in range(ev.num_partitions):
        for a in range(4):
            tally.check("Ttwiddle_beta_a", tot["Ttwiddle_beta_a"][p][a], T[p, a], "%s partition %d state %d" % (tag, p, a))
    tally.equal("num_muts_l", eng.num_muts_l(), tot["num_muts_l"], tag)
    if per_part_Ttwiddle and hasattr(eng, "Ttwiddle_l"):
        for k, s in enumerate(sts):
            got = eng.Ttwiddle_l(k)
            for l in range(len(got)):
                tally.check("Ttwiddle_l", s["Ttwiddle_l"][l], got[l], "%s part %d site %d" % (tag, k, l))
    return tot


def oracle_against_exact(tally, sc, num_parts, moves, seed, nu_l=None, evo=None, t_step=None, grid_prior=False, engine=None,
                         max_part_nodes=0, after_pass=None):
    """`engine`: an EmatBackend to check instead of the oracle (tests/test_exact_model_gpu.py), closed here whatever happens;
    `after_pass(engine, num_parts)` is called once the moves are done."""
    orc = engine if engine is not None else OracleEngine(sc.num_sites, trace_moves=0)
    try:
        parts, incl, seeds, root_part, ref = split_parts(sc, num_parts, seed, max_part_nodes)
        ev = X.Evo.of(sc, nu_l, evo)
        pop = X.Pop(sc.pop)
        configure(orc, sc, ref, parts, incl, seeds, root_part, t_step, nu_l=nu_l, evo=evo)
        scales = []
        for p in range(len(parts)):
            exG, exA, _ = check_part(tally, orc, p, ref, ev, pop, incl[p], "from scratch")
            scales.append((abs(exG.f), abs(exA.f)))
            check_popsize_bar(tally, orc, p, pop, "from scratch")
        check_stats(tally, orc, parts, ref, ev, "before moves")
        if grid_prior:
            assert len(parts) == 1
            tr, ts = sc.t_max_tip, t_step if t_step is not None else sc.default_t_step()
            got = orc.scalable_log_prior(0, tr, ts) if engine is None else orc.scalable_coalescent_log_prior(tr, ts)
            tally.check("scalable_prior", X.scalable_log_prior(parts[0], pop, tr, ts), got, "before moves")
        if moves:
            peaks = [list(s) for s in scales]
            for k in range(10):                 # ten slices: the totals' magnitudes are read between them
                m = moves // 10 + (1 if k < moves % 10 else 0)
                if engine is None:
                    orc.run_moves_per_part(m, threads=4)
                else:
                    orc.run_moves_per_part(m); orc.synchronize()
                for p in range(len(parts)):
                    _, _, Gv, Av = orc.part_derived(p, orc.part_stats(p)["num_nodes"])
                    peaks[p] = [max(peaks[p][0], abs(Gv)), max(peaks[p][1], abs(Av))]
            if after_pass is not None:
                after_pass(orc, len(parts))
            for p in range(len(parts)):
                assert orc.part_stats(p)["status"] == 0
                check_part(tally, orc, p, ref, ev, pop, incl[p], "maintained", peaks[p], moves)
            orc.recalc_derived()
            trees = []
            for p in range(len(parts)):
                trees.append(check_part(tally, orc, p, ref, ev, pop, incl[p], "after moves", moves=moves)[2])
            check_stats(tally, orc, trees, ref, ev, "after moves")
            if grid_prior:
                tr, ts = sc.t_max_tip, t_step if t_step is not None else sc.default_t_step()
                got = orc.scalable_log_prior(0, tr, ts) if engine is None else orc.scalable_coalescent_log_prior(tr, ts)
                tally.check("scalable_prior", X.scalable_log_prior(trees[0], pop, tr, ts), got, "after moves")
        return len(parts)
    finally:
        orc.close()


CONFIGS = {
    "C1": lambda: make_scenario("C1", num_tips=100, num_sites=3000, uncertain_tips=0.3),
    "C2": lambda: make_scenario("C2", num_tips=400, num_sites=3000, uncertain_tips=0.2),
    "C3": lambda: make_scenario("C3", num_tips=700, num_sites=3000),
    "C3-log-linear": lambda: make_scenario("C3", num_tips=700, num_sites=3000, skygrid_log_linear=True),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_whole_tree_against_exact(name, record_property):
    """One part holding the whole tree: derived quantities, the part's grid, the whole-tree grid prior and the global
    statistics, before and after 1 500 moves."""
    tally = Tally("oracle")
    oracle_against_exact(tally, CONFIGS[name](), 1, 1500, 3, grid_prior=True)
    tally.finish(record_property)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_parts_against_exact(name, record_property):
    """Parts cut by split_parts: each part's derived quantities and grid, the statistics summed over the parts, before and
    after 1 500 moves per part."""
    tally = Tally("oracle")
    oracle_against_exact(tally, CONFIGS[name](), 6, 1500, 5)
    tally.finish(record_property)


@pytest.mark.parametrize("block", range(4))
def test_oracle_random_scenarios_against_exact(block, record_property):
    """random_scenario's cases 0-23 (every population kind, site rates in every third, two partitions in every sixth, tip-date
    uncertainty in half), cut into 1-5 parts, before and after moves."""
    tally = Tally("oracle")
    for case in range(6 * block, 6 * block + 6):
        rng = np.random.default_rng(7100 + case)
        sc, nu_l, evo, what = random_scenario(rng, case, max_tips=160)
        nparts = int(rng.integers(1, 6))
        t_step = sc.default_t_step() * float(rng.choice([0.5, 1.0, 3.0]))
        tally.who = "oracle"
        before = len(tally.fail)
        oracle_against_exact(tally, sc, nparts, 600, 11 + case, nu_l=nu_l, evo=evo, t_step=t_step, grid_prior=(nparts == 1))
        if len(tally.fail) > before:
            tally.fail.insert(before, "-- " + what)
    tally.finish(record_property)


def test_oracle_population_models_on_adversarial_inputs(record_property):
    """The oracle's pop_at_time / pop_integral on the inputs test_exact_model_gpu.py gives the device: g dt from 1e-12 to 50 with
    both signs, intervals straddling, starting and ending on the minimum-population crossover, zero-length intervals, uneven
    skygrid knots with points on, beside and beyond them, adjacent gammas equal and 1e-12 apart, stepwise and log-linear."""
    import ctypes as C
    import oracle_ffi
    L = oracle_ffi.lib()
    tally = Tally("oracle")
    for name, pm, a, b in X.adversarial_pop_cases():
        pop, m = X.Pop(pm), pm.c_struct()
        for i in range(a.shape[0]):
            tally.check("pop_integral", pop.pop_integral(float(a[i]), float(b[i])), L.orc_pop_integral(C.byref(m), float(a[i]), float(b[i])), "%s [%r, %r]" % (name, a[i], b[i]))
            tally.check("pop_at_time", pop.pop_at_time(float(a[i])), L.orc_pop_at_time(C.byref(m), float(a[i])), "%s t=%r" % (name, a[i]))
    tally.finish(record_property)
