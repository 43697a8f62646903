"""The CPU oracle's graft analysis and forced re-attachments against the exact model of one graft (tests/graft_model.py has the
definitions and the bounds).  The oracle is the engine under test here; test_graft_model_gpu.py points the same cases, targets
and assertions at the device's own code through EmatBackend.debug_graft.

Cases.  "paths/1" and "paths/8": the graft-paths scenario of test_graft_analysis_paths_gpu.py (100 tips, 300 sites, gaps at a
third of the tips) as one part and cut into eight.  "sites/1" and "sites/4": 40 tips and 120 sites from the same generator with
the same gap rule, site rates nu_l = 0.25 + 1.5 U(0,1) and two site partitions with different HKY parameters, so that lambdas
and log rates depend on the site.  "gapped/1": 8 tips and 300 sites from the same generator with its gaps kept at EVERY tip.
A rooty graft has hot sites in all three of its infos only where each child of the run's root misses sites the other has data
for.  In the paths scenario two thirds of the tips miss nothing, so one child of the root always has data everywhere -- in the
tree as built, after any forced re-attachment (one side is then the whole old tree or holds a tip without gaps), and in the
eight-part cut's root part, whose tips are cut points above such tips -- and the count cannot be met there by any seed; gapped/1
(seed 10: the first of 1..12 at 8, 10 and 12 tips whose root's children each miss sites the other has) is where it is required.

Mode 0 (analyze_graft) on every X the move code can analyse, at mu_proposal 1e-9, 1e-3 and 1e-1: with T of days to years that
puts 4/3 mu T in the range where expm1 cancels, the ordinary range and the saturating range.

Mode 3 (a whole forced re-attachment: analyse, peel, move, propose, apply) on a seeded list of 60 targets per cut of the paths
scenario and on gapped/1, ten of each kind of KINDS.  The hook does not validate (new_sibling, new_t_P): `targets` builds only valid ones and asserts their validity in
plain Python before any engine sees them.  The model's graft of X on the tree before is compared with the first graft
returned, the model's graft of X on the tree downloaded AFTER with the second -- the proposed history is read back from the tree,
so log_alpha_mut(new) is the density of the history actually written and the deltas are its net change.

The counts of HONEST are taken from the oracle's results alone, never the device's; TARGET_SEED = 1, the first tried, meets them
on every cut.  A seed that does not is replaced on the CPU, as the header of test_graft_analysis_paths_gpu.py describes for its
seed; a count is never lowered to fit one."""
import functools
import hashlib
import time
from fractions import Fraction as F

import numpy as np
import pytest

import exact_model as X
import graft_model as GM
import move_steps as M
from delphy_amd.engine import hky_q_matrix
from helpers import configure, split_parts
from oracle_ffi import OracleEngine
from test_exact_model import Tally
from test_graft_analysis_paths_gpu import MU_PROPOSAL, REQUIRED, REQUIRED_CUT, REQUIRED_ROOT_PART, coverage, reference, scenario

MUS = (1e-9, 1e-3, 1e-1)
CASES = ("paths/1", "paths/8", "sites/1", "sites/4", "gapped/1")
FORCED = ("paths/1", "paths/8", "gapped/1")
TARGETS_PER_CUT = 60
TARGET_SEED = 1
# Minimum counts over the grafts of ONE cut of the paths scenario (mode 0 and both grafts of every forced move), from the oracle's results
HONEST = {"infos with d > 0": 10, "infos with M > d": 5, "level-0 infos where X misses sites": 5}
# ... and over the grafts of gapped/1 (see the docstring: no cut of the paths scenario can hold one)
HONEST_ROOTY = {"rooty grafts with hot sites in all three infos": 2, "open infos with hot mutations": 2}
KINDS = ("same branch", "further up", "further down", "across", "into the rooty position", "out of the rooty position")


# ---- the cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(sc, parts, incl, seeds, root_part, ref, nu_l, evo)."""
    which, nparts = name.split("/")
    nparts = int(nparts)
    if which == "paths":
        sc = scenario()
        (parts, incl, seeds, root_part, ref), _ = reference(nparts)
        nu_l = evo = None
    elif which == "gapped":
        sc = scenario(8, 300, 10, 0, True)
        parts, incl, seeds, root_part, ref = split_parts(sc, nparts, 11)
        nu_l = evo = None
    else:
        sc = scenario(40, 120, 117, 9)
        parts, incl, seeds, root_part, ref = split_parts(sc, nparts, 11)
        rng = np.random.default_rng(40120)
        nu_l = 0.25 + 1.5 * rng.random(sc.num_sites)
        pis = [(0.31, 0.19, 0.21, 0.29), (0.22, 0.33, 0.27, 0.18)]
        evo = ([sc.mu, 1.7 * sc.mu], pis, [hky_q_matrix(5.0, pis[0]), hky_q_matrix(1.5, pis[1])], (rng.random(sc.num_sites) < 0.4).astype(np.int32))
    assert len(parts) == nparts, (name, len(parts))
    return dict(sc=sc, parts=parts, incl=incl, seeds=seeds, root_part=root_part, ref=ref, nu_l=nu_l, evo=evo, ev=X.Evo.of(sc, nu_l, evo))


def setup(engine, name):
    c = case(name)
    configure(engine, c["sc"], c["ref"], c["parts"], c["incl"], c["seeds"], c["root_part"], nu_l=c["nu_l"], evo=c["evo"])
    return engine


@functools.lru_cache(maxsize=None)
def models(name):
    c = case(name)
    return [GM.GraftModel(t, c["ref"], c["ev"], r) for t, r in zip(c["parts"], c["incl"])]


@functools.lru_cache(maxsize=None)
def analysable(name):
    """[(part, X)] of every X the move code can analyse."""
    return [(p, Xn) for p, m in enumerate(models(name)) for Xn in range(m.T.n) if m.can_analyse(Xn)]


def _digest(tree):
    h = hashlib.sha1()
    for f in M._TOPO[1:] + M._MUT + ("t", "mut_t"):
        h.update(np.ascontiguousarray(getattr(tree, f)).tobytes())
    h.update(str(int(tree.root)).encode())
    return h.hexdigest()


_after = {}


def model_after(name, p, tree):
    """The GraftModel of a tree an engine left behind, kept by the tree's content: the oracle's and the device's trees after the
    same forced move are the same tree, and its model is built once."""
    key = (name, p, _digest(tree))
    if key not in _after:
        c = case(name)
        _after[key] = GM.GraftModel(tree, c["ref"], c["ev"], c["incl"][p])
    return _after[key]


# ---- mode 0 ------------------------------------------------------------------------------------------------------------
def check_analyses(tally, name, engine, mu):
    """Mode 0 of `engine` on every analysable X of the case, against the model."""
    c = case(name)
    n = 0
    for p, Xn in analysable(name):
        g = engine.debug_graft(p, Xn, mu)["grafts"][0]
        GM.compare(tally, g, models(name)[p].graft(Xn), mu, c["sc"].num_sites, "%s part %d X %d mu %g" % (name, p, Xn, mu))
        n += 1
    return n


# ---- mode 3: the targets -------------------------------------------------------------------------------------------------
def _subtree(T, Xn):
    out, st = set(), [Xn]
    while st:
        v = st.pop(); out.add(v); st += T.kids[v]
    return out


def assert_valid_target(T, incl, Xn, SS, t):
    """The conditions under which Spr_move::move may be called (the hook checks none of them)."""
    root = T.root
    assert Xn != root and 0 <= SS < T.n
    P = T.parent[Xn]
    assert SS != Xn and SS not in _subtree(T, Xn), "the new sibling lies in X's subtree"
    assert SS != P, "the new sibling is X's parent"
    if not incl:
        assert SS != root and P != root, "a part without the run's root keeps its root"
    S = [k for k in T.kids[P] if k != Xn][0]
    above = T.parent[P] if SS == S else T.parent[SS]          # the new sibling's parent-to-be, once P is gone
    if above == P:
        above = T.parent[P]
    t = F(t)
    assert t < min(T.t[Xn], T.t[SS]) and (above < 0 or T.t[above] < t), "new_t_P outside the branch above the new sibling"
    assert all(t != x for x in T.t), "new_t_P is a node's time"


def kind_of(T, Xn, SS):
    P = T.parent[Xn]
    S = [k for k in T.kids[P] if k != Xn][0]
    if SS == T.root:
        return "into the rooty position"
    if P == T.root and SS != S:
        return "out of the rooty position"
    if SS == S:
        return "same branch"
    anc = set()
    v = P
    while v >= 0:
        anc.add(v); v = T.parent[v]
    if SS in anc:
        return "further up"
    if SS in _subtree(T, S):
        return "further down"
    return "across"


@functools.lru_cache(maxsize=None)
def targets(name):
    """[(part, X, new_sibling, new_t_P, kind)]: TARGETS_PER_CUT seeded valid targets, ten of each kind while the parts offer them
    (the rooty kinds in the root part only), every one asserted valid."""
    c = case(name)
    rng = np.random.default_rng(TARGET_SEED)
    ms = models(name)
    per_kind = {k: [] for k in KINDS}
    for p, m in enumerate(ms):
        T = m.T
        for Xn in range(T.n):
            if not m.can_analyse(Xn):
                continue
            sub, P = _subtree(T, Xn), T.parent[Xn]
            for SS in range(T.n):
                if SS in sub or SS == P or (SS == T.root and not c["incl"][p]):
                    continue
                S = [k for k in T.kids[P] if k != Xn][0]
                above = T.parent[P] if SS == S else T.parent[SS]
                hi = min(T.t[Xn], T.t[SS])
                lo = T.t[above] if above >= 0 else hi - 200
                if lo < hi:
                    per_kind[kind_of(T, Xn, SS)].append((p, Xn, SS, float(lo), float(hi)))
    out = []
    want = TARGETS_PER_CUT // len(KINDS)
    for k in KINDS:
        cand = per_kind[k]
        assert cand, "%s: no valid target of kind '%s'" % (name, k)
        for i in rng.choice(len(cand), size=min(want, len(cand)), replace=False).tolist():
            p, Xn, SS, lo, hi = cand[i]
            t = lo + (hi - lo) * float(rng.uniform(0.05, 0.95))
            out.append((p, Xn, SS, t, k))
    while len(out) < TARGETS_PER_CUT:           # a kind the parts offer fewer than ten of: fill up with moves across the tree
        p, Xn, SS, lo, hi = per_kind["across"][int(rng.integers(len(per_kind["across"])))]
        out.append((p, Xn, SS, lo + (hi - lo) * float(rng.uniform(0.05, 0.95)), "across"))
    for p, Xn, SS, t, k in out:
        assert_valid_target(ms[p].T, c["incl"][p], Xn, SS, t)
    assert {k for *_, k in out} == set(KINDS)
    return out


def forced_moves(name, make_engine):
    """Every target on a freshly configured engine (targets in different parts share one): [(result of mode 3, log_G before, log_G
    after, tree after)] in the order of targets(name)."""
    c = case(name)
    tg = targets(name)
    out = [None] * len(tg)
    todo = list(range(len(tg)))
    while todo:
        batch, used, rest = [], set(), []
        for i in todo:
            (rest if tg[i][0] in used else batch).append(i); used.add(tg[i][0])
        todo = rest
        eng = setup(make_engine(c["sc"].num_sites), name)
        try:
            for i in batch:
                p, Xn, SS, t, _ = tg[i]
                if hasattr(eng, "synchronize"):
                    eng.synchronize()
                n = c["parts"][p].num_nodes
                Gb = float(eng.part_derived(p, n)[2])
                try:
                    r = eng.debug_graft(p, Xn, MU_PROPOSAL, 3, SS, t)
                except Exception as e:
                    raise AssertionError("%s target %d (part %d of %d nodes, X %d above %d at %r): %s" % (name, i, p, n, Xn, SS, t, e)) from e
                if hasattr(eng, "synchronize"):
                    eng.synchronize()
                out[i] = (r, Gb, float(eng.part_derived(p, n)[2]), eng.part_download(p))
        finally:
            eng.close()
    return out


def assert_outside_the_paths_unchanged(B, A, Xn, where, fails):
    """Everything but the nodes on X's path to the root before and after, and their children (whose missing intervals the hops
    factor anew), is what it was, bit for bit."""
    touched = set()
    for T in (B, A):
        v = Xn
        while v >= 0:
            touched.add(v); touched.update(T.kids[v]); v = T.parent[v]
    for v in range(B.n):
        if v in touched:
            continue
        if (B.parent[v], sorted(B.kids[v]), B.t[v], B.muts[v], B.miss[v], B.mfs[v]) != (A.parent[v], sorted(A.kids[v]), A.t[v], A.muts[v], A.miss[v], A.mfs[v]):
            fails.append("%s: node %d, off both paths, changed" % (where, v))
    return B.n - len(touched)


def check_forced_moves(tally, name, results):
    """The assertions of one cut's forced moves; returns the number of nodes found untouched."""
    c = case(name)
    L = c["sc"].num_sites
    untouched = 0
    for (p, Xn, SS, t, kind), (r, Gb, Ga, after) in zip(targets(name), results):
        where = "%s part %d X %d -> above %d at %r (%s)" % (name, p, Xn, SS, t, kind)
        if r["status"] != 0 or len(r["grafts"]) != 2:
            tally.fail.append("%s: status %d, %d grafts" % (where, r["status"], len(r["grafts"]))); continue
        mb = models(name)[p]
        GM.compare(tally, r["grafts"][0], mb.graft(Xn), MU_PROPOSAL, L, where + " old graft")
        try:
            M.assert_valid_part(after, c["ref"])
            ma = model_after(name, p, after)
        except AssertionError as e:
            tally.fail.append("%s: the tree after: %s" % (where, e)); continue
        P = ma.T.parent[Xn]
        if not (float(ma.T.t[P]) == t and SS in ma.T.kids[P]):
            tally.fail.append("%s: X hangs below %d at %r with %s" % (where, P, float(ma.T.t[P]), ma.T.kids[P]))
        GM.compare(tally, r["grafts"][1], ma.graft(Xn), MU_PROPOSAL, L, where + " new graft")
        dG = X.part_log_G_delta(mb.dv, ma.dv, c["ref"], c["ev"], c["incl"][p])
        # the maintained total moves by -old.delta_log_G + new.delta_log_G: both grafts' own bounds, and the additions at the total's magnitude
        allowance = mb.graft(Xn).delta_log_G.bound() + ma.graft(Xn).delta_log_G.bound() + 4 * X.U * max(abs(Gb), abs(Ga))
        tally.check("increment_log_G", dG, F(Ga) - F(Gb), where, allowance)
        untouched += assert_outside_the_paths_unchanged(mb.T, ma.T, Xn, where, tally.fail)
    return untouched


# ---- what keeps the file honest --------------------------------------------------------------------------------------------
def _sites_missing(tree):
    """Per node, the number of sites in the missing intervals on its path from the root (the tree's lists alone)."""
    o = tree.miss_offset
    own = [int((tree.miss_end[o[v]:o[v + 1]] - tree.miss_start[o[v]:o[v + 1]]).sum()) for v in range(tree.num_nodes)]
    out = np.zeros(tree.num_nodes, np.int64)
    for v in range(tree.num_nodes):
        u = v
        while u >= 0:
            out[v] += own[u]; u = int(tree.parent[u])
    return out


def _count_graft(cnt, g, tree, nsm):
    bis = g["branch_infos"]
    rooty = int(tree.parent[g["X"]]) == int(tree.root)
    if rooty:
        cnt["rooty grafts with hot sites in all three infos"] += len(bis) == 3 and all(b["hot_sites"] for b in bis)
    elif nsm[g["X"]] > 0:         # info 0's hot sites hold every site X misses (the sites that slide on have data below X)
        cnt["level-0 infos where X misses sites"] += 1
    for b in bis:
        cnt["open infos with hot mutations"] += b["is_open"] and len(b["hot_muts_to_X"]) > 0
        cnt["infos with d > 0"] += len(b["hot_deltas_to_X"]) > 0
        cnt["infos with M > d"] += (not b["is_open"]) and len(b["hot_muts_to_X"]) > len(b["hot_deltas_to_X"])


@functools.lru_cache(maxsize=None)
def oracle_forced(name):
    return forced_moves(name, lambda L: OracleEngine(L))


@functools.lru_cache(maxsize=None)
def honest_counts(name):
    """From the oracle's results alone."""
    c = case(name)
    nparts = len(c["parts"])
    if name.startswith("paths"):
        _, want = reference(nparts)
    else:
        eng = setup(OracleEngine(c["sc"].num_sites), name)
        try:
            want = {(p, Xn): eng.debug_graft(p, Xn, MU_PROPOSAL)["grafts"][0] for p, Xn in analysable(name)}
        finally:
            eng.close()
    cnt = dict.fromkeys(list(HONEST) + list(HONEST_ROOTY), 0)
    for (p, Xn), g in want.items():
        _count_graft(cnt, g, c["parts"][p], _sites_missing(c["parts"][p]))
    for (p, Xn, SS, t, k), (r, _, _, after) in zip(targets(name), oracle_forced(name)):
        assert r["status"] == 0 and len(r["grafts"]) == 2, (name, p, Xn, SS, t)
        _count_graft(cnt, r["grafts"][0], c["parts"][p], _sites_missing(c["parts"][p]))
        _count_graft(cnt, r["grafts"][1], after, _sites_missing(after))
    return cnt


# ---- the tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORCED)
def test_the_cases_hold_what_they_must(name, record_property):
    nparts = int(name.split("/")[1])
    if name.startswith("paths"):
        have = dict(coverage(nparts), **honest_counts(name))
        need = dict(REQUIRED, **(REQUIRED_ROOT_PART if nparts == 1 else REQUIRED_CUT), **HONEST)
        # why HONEST_ROOTY is not asked of this scenario (the docstring): in the part that holds the run's root, one child of the root
        # has data at every site the root has, so no rooty graft here can have hot sites on both open infos
        c = case(name)
        m = models(name)[c["root_part"]]
        assert c["incl"][c["root_part"]] and any(np.array_equal(m.data(k), m.data(m.T.root)) for k in m.T.kids[m.T.root]), name
        assert have["rooty grafts with hot sites in all three infos"] == 0, have
    else:
        have, need = honest_counts(name), HONEST_ROOTY
    for k, v in have.items():
        record_property("have_" + k, int(v))
    for what, n in need.items():
        assert have[what] >= n, "%s must hold %d of '%s' (has %d): %s" % (name, n, what, have[what], have)
    kinds = [k for *_, k in targets(name)]
    assert len(kinds) == TARGETS_PER_CUT and all(kinds.count(k) >= 1 for k in KINDS), kinds


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("name", CASES)
def test_oracle_analyses_against_the_model(name, mu, record_property):
    tally = Tally("oracle")
    eng = setup(OracleEngine(case(name)["sc"].num_sites), name)
    try:
        n = check_analyses(tally, name, eng, mu)
    finally:
        eng.close()
    record_property("grafts", n)
    # (paths: the 196 and 182 inner grafts of the graft-paths scenario's two cuts and two rooty grafts each)
    assert n == len(analysable(name)) and n >= {"paths/1": 198, "paths/8": 184, "gapped/1": 14}.get(name, 60), n
    tally.finish(record_property)


def test_the_second_scenario_depends_on_the_site():
    c = case("sites/1")
    mu, pi, q, pfs = c["evo"]
    assert mu[0] != mu[1] and 20 <= int(np.sum(pfs)) <= 100 and np.ptp(c["nu_l"]) > 1.0
    hot = [m for g in (models("sites/1")[0].graft(Xn) for _, Xn in analysable("sites/1")) for b in g.infos for m in b.muts]
    assert {int(pfs[l]) for (_, l, _, _) in hot} == {0, 1}, "hot mutations in both site partitions"


@pytest.mark.parametrize("name", FORCED)
def test_oracle_forced_moves_against_the_model(name, record_property):
    tally = Tally("oracle")
    t0 = time.perf_counter()
    untouched = check_forced_moves(tally, name, oracle_forced(name))
    record_property("model_and_checks_s", round(time.perf_counter() - t0, 2))
    assert untouched > 0
    tally.finish(record_property)
