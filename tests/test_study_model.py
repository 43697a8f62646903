"""tests/study_model.py checked against itself without an engine, and the CPU oracle's accepted SPR1 moves of the rare kinds held to
the identity of move_steps.check_accepted_spr1 (test_study_model_gpu.py points the same chains at the device).

The model alone, on 200 seeded small trees (4-60 tips, gapped) and every analysable X: min_muts at the old nexus is the graft's closed
d_i summed (the two EMAT_CHECKs of emat_device_moves.hpp:555-556); the region probabilities sum to 1; a literal depth-first walk written
here finds the region set of limit 1 that the path-count definition names; the densities integrate to the region's probability, by 1 000
midpoints below the root and mpmath's quad above it, in both of the root's regimes.

The lean stepper.  SPR1 is one move in 32 and an unlimited scan one in 100 of those, so test_move_steps.py's cases hold perhaps one
unlimited scan.  `run_lean` advances every part by one move per pass and reads, per pass and part, part_stats, the trace's last row,
part_rng and part_download, nothing else; only for an accepted SPR1 move that may still add to a class of LEAN[case]["want"] does it
read the coalescent tables and build the exact side (Derived, GraftModel, both studies).  A case ends when its wants are met or after
its passes (never more than 4 000).  Classes: move_steps.Coverage.SPR1_CLASSES; test_lean_cases_cover_what_they_must asserts the counts
of the issue over all cases.

The block of a limited scan (emat_device_moves.hpp: EMAT_HOT_BYTES = 1536 by default, 36 bytes per scan item) holds 1536 // 36 = 42
items; a part that leaves more of its staging area free sets aside up to 32 768 bytes = 910 items.  A level of the breadth-first scan
wider than the wave's 64 lanes takes a second chunk: studies of more than 64 regions; one of more than 640 regions outgrows the default
block fifteen times over.  Whether that scan leaves LDS depends on what the part's staging leaves free, which nothing read here says:
the class is the issue's count, not an observation of the migration."""
import time
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

import delphy_amd as d
import delphy_amd.engine as E
import exact_model as X
import graft_model as GM
import move_steps as M
import study_model as SM
from delphy_amd.scenarios import KAPPA, PI, Scenario, make_scenario
from helpers import configure, split_parts
from oracle_ffi import OracleEngine
from test_exact_model import Tally
from test_move_steps import high_mutation_scenario

HOT_BYTES, ITEM_BYTES = 1536, 36          # emat_device_moves.hpp's default block and emat_device_spr.hpp's scan item
ITEMS_IN_DEFAULT_BLOCK = HOT_BYTES // ITEM_BYTES
assert ITEMS_IN_DEFAULT_BLOCK == 42


def synthetic(tips, sites, span, mu, gaps, gap_len, seed, uncertain=0.0, n0=365.0, prior_n0=None):
    """`prior_n0`: the population the chain's prior holds, when that is not the one the tree was drawn from."""
    par = E.SynthParams(num_tips=tips, num_sites=sites, tip_span=span, pop_n0=n0, mu=mu, gaps_per_tip=gaps, mean_gap_len=gap_len, seed=seed)
    par.pi, par.kappa = PI, KAPPA
    if uncertain:
        par.frac_uncertain_tips, par.tip_date_uncertainty = uncertain, 5.0
    tree, ref, tmax = E.make_synthetic_emat(par)
    return Scenario("S%d" % seed, tree, ref, tmax, mu, KAPPA, PI, d.PopModel.exp(tmax, prior_n0 or n0, 0.0, 0.0), sites)


# ---- the model alone ---------------------------------------------------------------------------------------------------------------
def small_tree(k):
    """Seeded: 4-60 tips, 40-240 sites, up to three gaps per tip; every fourth nearly free of mutations (the power law above the root)."""
    rng = np.random.default_rng(9100 + k)
    tips, sites = int(rng.integers(4, 61)), int(rng.choice([40, 120, 240]))
    span = float(rng.choice([30.0, 365.0]))
    mu = (3e-4 if k % 4 == 3 else float(10 ** rng.uniform(-1.5, 0.3))) / (sites * span)
    return synthetic(tips, sites, span, mu, int(rng.integers(0, 4)), float(rng.uniform(2.0, sites / 4)), int(rng.integers(1, 2 ** 31)))


def literal_walk(pr, limit):
    """spr_study.cpp:26-128 on the pruned tree: a stack of (region, where it came from, mutations counted so far); a region out of scope is
    neither kept nor left through.  -> {(branch, idx)}."""
    nm = {v: len(pr.muts[v]) for v in pr.nodes}
    seen = set()
    stack = [((pr.start_branch, pr.start_idx), None, 0)]
    while stack:
        (b, i), came, c = stack.pop()
        if c > limit:
            continue
        seen.add((b, i))
        nbrs = []
        if b != pr.root:
            if i > 0:
                nbrs.append(((b, i - 1), pr.muts[b][i - 1][0]))
            else:
                nbrs.append(((pr.parent[b], nm[pr.parent[b]]), None))
        if i < nm[b]:
            nbrs.append(((b, i + 1), pr.muts[b][i][0]))
        else:
            nbrs += [((k, 0), None) for k in pr.kids[b]]
        for q, site in nbrs:
            if q != came:
                stack.append((q, (b, i), c + int(site is not None and not pr.missing_at_X[site])))
    return seen


def test_the_model_alone_on_small_trees(record_property):
    counts = dict(trees=0, grafts=0, studies=0, walks=0, rooty=0, power=0, gamma=0, uncounted=0, quadratures=0, root_quadratures={"power": 0, "gamma": 0})
    for k in range(200):
        sc = small_tree(k)
        ev = X.Evo.of(sc, None, None)
        gm = GM.GraftModel(sc.tree, sc.ref, ev, True)
        dv = gm.dv
        counts["trees"] += 1
        xs = [x for x in range(gm.T.n) if gm.can_analyse(x)]
        rng = np.random.default_rng(k)
        studied = set(rng.choice(xs, size=min(2, len(xs)), replace=False).tolist())
        for x in xs:
            g = gm.graft(x)
            pr = SM.Pruned(gm, x)
            regs = SM.all_regions(pr, True)
            old = [r for r in regs if r.crossed == 0 and r.uncounted == 0 and r.branch == pr.start_branch and r.idx == pr.start_idx]
            assert len(old) == 1
            assert old[0].m == sum(b.d for b in g.infos if not b.is_open), (k, x, old[0], [b.d for b in g.infos])
            assert (old[0].t_min is None or old[0].t_min < F(g.t_P)) and (g.rooty or F(g.t_P) <= old[0].t_max), (k, x, old[0], g.t_P)
            counts["grafts"] += 1; counts["rooty"] += int(g.rooty)
            assert {(r.branch, r.idx) for r in regs if r.crossed <= 1} == literal_walk(pr, 1), (k, x)
            counts["walks"] += 1
            counts["uncounted"] += int(any(r.uncounted for r in regs if r.crossed <= 1))
            if x not in studied or dv.lam[x] == 0:
                continue
            for limit in (1, None):
                st = SM.Study(pr, True, limit, dv.lambda_i(x), sc.t_max_tip)
                p = st.probabilities()
                assert abs(sum(p) - 1.0) <= 1e-12, (k, x, limit, sum(p))
                counts["studies"] += 1
                if st.root_kind:                                # (None: the region above the root is out of the limit's reach)
                    counts[st.root_kind] += 1
                # the densities integrate to the regions' probabilities
                for i, r in enumerate(st.regions):
                    if st.log_p[i] is None:
                        continue
                    if r.above_root and counts["root_quadratures"][st.root_kind] < 4:
                        t_S, s_min, s_max, _, _, _ = st._root_params(r)
                        lo = (pr.t_X + t_S - s_max) / 2
                        with mpmath.workdps(20):
                            got = mpmath.quad(lambda t: mpmath.exp(X._mp(st.log_alpha(i, float(t)).exact.value)), mpmath.linspace(X._mp(lo), X._mp(r.t_max), 9))
                        # (the time goes through a float64: the end points move by a rounding of |t|)
                        assert abs(float(got) - p[i]) <= 1e-9 * max(p[i], 1e-30) + 1e-12, (k, x, limit, r, float(got), p[i])
                        counts["root_quadratures"][st.root_kind] += 1
                    elif not r.above_root and counts["quadratures"] < 20 and len(st.regions) <= 24:
                        h = (r.t_max - r.t_min) / 1000
                        got = sum(mpmath.exp(X._mp(st.log_alpha(i, float(r.t_min + (j + F(1, 2)) * h)).exact.value)) for j in range(1000)) * X._mp(h) if h > F(1, 10 ** 6) else None
                        if got is not None:
                            assert abs(float(got) - p[i]) <= 1e-12 * max(p[i], 1e-30) + 1e-300, (k, x, limit, r, float(got), p[i])
                            counts["quadratures"] += 1
    record_property("counts", counts)
    print(counts)
    assert counts["rooty"] >= 200 and counts["power"] >= 20 and counts["gamma"] >= 100 and counts["uncounted"] >= 50, counts
    assert counts["quadratures"] >= 20 and min(counts["root_quadratures"].values()) >= 4, counts


# ---- the lean stepper ----------------------------------------------------------------------------------------------------------------
C = M.Coverage.SPR1_CLASSES
UNLIMITED, ROOT_GAMMA, ROOT_POWER, OLD_ROOT, NO_ROOT, MIN_MUTS, UNCOUNTED, OVER_64, OVER_640 = range(len(C))
# The issue's conditions over this file's cases (and, with the same chains, over test_study_model_gpu.py's)
REQUIRED = {UNLIMITED: 2, ROOT_GAMMA: 3, ROOT_POWER: 3, OLD_ROOT: 3, NO_ROOT: 10, MIN_MUTS: 10, UNCOUNTED: 5, OVER_64: 3, OVER_640: 1}


def _c1_40():
    return make_scenario("C1", num_tips=40, num_sites=1000, uncertain_tips=0.3), None


def _gapped():
    # a third of every tip's sites missing, a mutation every few branches: paths that cross mutations at sites missing at X
    return synthetic(24, 240, 200.0, 1.5e-4, 3, 30.0, 515, uncertain=0.3), None


def _bare(tips, seed, mls=1e-4, prior_n0=400.0):
    # mu L tip_span = mls: next to no mutations, lambda_X f s_max < 0.01 (the power law above the root), every region within limit 1;
    # (the region above the root then outweighs the tree's, and a coarser grid -- LEAN's t_step factor -- holds the roots proposed);
    # a prior population far above the one the tree was drawn from, so that where X goes is decided by the study alone and moves are accepted
    return lambda: (synthetic(tips, 120, 100.0, mls / (120 * 100.0), 1, 6.0, seed, n0=60.0, prior_n0=prior_n0), None)


LEAN = {
    "C1-40/6": dict(make=_c1_40, parts=6, seed=5, passes=4000, want={UNLIMITED: 2, ROOT_GAMMA: 3, OLD_ROOT: 3, NO_ROOT: 10, MIN_MUTS: 10}),
    "high-mutation/1": dict(make=high_mutation_scenario, parts=1, seed=11, passes=4000, want={UNLIMITED: 2, OVER_64: 2}),
    "gapped/1": dict(make=_gapped, parts=1, seed=7, passes=4000, want={UNCOUNTED: 5}),
    "bare-5/1": dict(make=_bare(5, 30, 2e-5), parts=1, seed=2, passes=4000, t_step=16.0, want={ROOT_POWER: 3}),
    "bare-60/1": dict(make=_bare(60, 31), parts=1, seed=3, passes=2500, want={OVER_64: 3}),
    "bare-450/1": dict(make=_bare(450, 32), parts=1, seed=4, passes=2500, want={OVER_640: 1}),
}
_done = {}


class LeanWatch:
    """What check_accepted_spr1 asks of a PartWatch, built for one move from the tree before it."""

    def __init__(self, p, tree, ref, ev, includes_root, t_max_tip, tag):
        self.p, self.ref, self.ev, self.includes_root, self.t_max_tip, self.tag = p, np.asarray(ref), ev, bool(includes_root), t_max_tip, tag
        self.dv = X.Derived(tree, ref, ev)


def k_allowance(tab, moves):
    """check_part's allowance for a k_bar_p maintained over `moves` moves (move_steps.PartWatch.k_allowance, from the engine's table)."""
    kmax = max(1.0, float(np.abs(tab["k_bar_p"]).max()))
    bmax = (abs(tab["t_ref"]) + len(tab["k_bar_p"]) * tab["t_step"]) / tab["t_step"]
    return min(4 * moves * X.U * (kmax + bmax), 1e-9 * kmax)


def run_lean(name, make_engine, who):
    """-> (Tally, Coverage, dict(passes, proposed, accepted, checked, seconds of the engine's side))."""
    case = LEAN[name]
    sc, nu_l = case["make"]()
    parts, incl, seeds, root_part, ref = split_parts(sc, case["parts"], case["seed"])
    ev, pop = X.Evo.of(sc, nu_l, None), X.Pop(sc.pop)
    tally, cov = Tally(who), M.Coverage()
    want = dict(case["want"])
    eng = make_engine(sc.num_sites, case["passes"] + 8)
    info = dict(passes=0, proposed=0, accepted=0, checked=0, most_regions=0, engine_s=0.0, exact_s=0.0)
    try:
        configure(eng, sc, ref, parts, incl, seeds, root_part, sc.default_t_step() * case.get("t_step", 1.0), nu_l=nu_l)
        if hasattr(eng, "synchronize"):
            eng.synchronize()
        n = len(parts)
        trees = [eng.part_download(p) for p in range(n)]
        rngs = [M.stream_position(eng, p) for p in range(n)]
        for s in range(case["passes"]):
            t0 = time.perf_counter()
            M.advance_one_move(eng)
            info["engine_s"] += time.perf_counter() - t0
            info["passes"] += 1
            for p in range(n):
                st = eng.part_stats(p)
                assert st["status"] == 0 and st["moves_done"] == s + 1, (name, p, st)
                row = eng.part_trace(p, s + 1)[-1]
                before, rng_before = trees[p], rngs[p]
                trees[p], rngs[p] = eng.part_download(p), M.stream_position(eng, p, st)
                if int(row[0]) != 4:
                    continue
                info["proposed"] += 1
                if row[2] != 1.0:
                    continue
                info["accepted"] += 1
                # may this move still add to a class the case wants?  What can be said before the exact side is built: the scan's limit,
                # the part, whether the root changed
                limit = M.scan_limit_from_stream(rng_before)
                may = {UNLIMITED: limit is None, NO_ROOT: not incl[p], ROOT_GAMMA: int(trees[p].root) != int(before.root), ROOT_POWER: int(trees[p].root) != int(before.root),
                       OLD_ROOT: int(before.parent[int(row[1])]) == int(before.root), OVER_640: before.num_nodes + before.mut_site.shape[0] > 640 and (limit is None or name.startswith("bare"))}
                if not any(want.get(c, 0) > 0 and may.get(c, True) for c in want):
                    continue
                t0 = time.perf_counter()
                where = "%s part %d pass %d (spr1 of node %d, log_mh %r)" % (name, p, s, int(row[1]), float(row[3]))
                w = LeanWatch(p, before, ref, ev, incl[p], sc.t_max_tip, name)
                try:
                    M.assert_valid_part(trees[p], ref)
                    dvA = X.Derived(trees[p], ref, ev)
                    tab = eng.part_coalescent(p)
                    dP = X.partial_log_prior_delta(w.dv.T, dvA.T, pop, incl[p], tab)
                    k_term = float(dP.k_sensitivity) * k_allowance(tab, s + 1)
                    one = M.Coverage()
                    ident = M.check_accepted_spr1(tally, one, w, int(row[1]), dvA, dP, k_term, float(row[3]), rng_before, where)
                    info["most_regions"] = max(info["most_regions"], len(ident["pre"].regions), len(ident["post"].regions))
                    cov.add(one)
                    got = one.accepted_spr1_classes
                except AssertionError as e:
                    tally.fail.append("%s: %s" % (where, e)); cov.unchecked += 1
                    got = [0] * len(C)
                info["checked"] += 1
                info["exact_s"] += time.perf_counter() - t0
                for c in want:
                    want[c] -= got[c]
            if all(v <= 0 for v in want.values()):
                break
    finally:
        eng.close()
    info["unmet"] = {C[c]: v for c, v in want.items() if v > 0}
    return tally, cov, info


def _oracle(num_sites, trace):
    return OracleEngine(num_sites, trace_moves=trace)


@pytest.mark.parametrize("name", list(LEAN))
def test_oracle_accepted_spr1_of_the_rare_kinds(name, record_property):
    tally, cov, info = _done[name] = run_lean(name, _oracle, "oracle")
    record_property("classes", dict(zip(C, cov.accepted_spr1_classes)))
    record_property("run", info)
    print(name, info, dict(zip(C, cov.accepted_spr1_classes)))
    tally.finish(record_property)
    assert cov.unchecked == 0 and not info["unmet"], info


def assert_lean_conditions(done, record_property):
    total = M.Coverage()
    for name in LEAN:
        total.add(done[name][1])
    got = dict(zip(C, total.accepted_spr1_classes))
    record_property("classes", got)
    record_property("held", total.accepted_spr1_log_mh_exact)
    print("accepted SPR1 moves held to the identity:", total.accepted_spr1_log_mh_exact, got)
    assert total.unchecked == 0
    # the time every one of them drew in its new region was held to the region's inverse CDF (tests/draws_model.py), the rare regions too
    times = dict(zip(M.DM.SPR1_TIMES, total.draws_spr1_times))
    record_property("spr1_times_held", times)
    assert total.borderline == 0 and total.position_half_known == 0 and sum(total.draws_spr1_times) == total.accepted_spr1_log_mh_exact and min(total.draws_spr1_times) >= 1, times
    for c, need in REQUIRED.items():
        assert total.accepted_spr1_classes[c] >= need, (C[c], need, got)


def test_lean_cases_cover_what_they_must(record_property):
    for name in LEAN:
        if name not in _done:
            _done[name] = run_lean(name, _oracle, "oracle")
    assert_lean_conditions(_done, record_property)
