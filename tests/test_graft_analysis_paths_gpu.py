"""The inner graft analysis (start_inner_graft_analysis, emat_device_spr.hpp) builds each level of the hot path in one pass over its lists:
one walk splits the sliding set into the level's hot sites and what slides on (iv_split), the sliding from-states are filtered by a merged walk,
the hot mutations are dealt to their owners in one pass, and nothing is sized by the path to the part's root.  Here every list it leaves behind is
held to the oracle's restatement of the reference's analyze_graft, entry for entry and bit for bit, on a tree made for it: short and many missing
intervals at a third of the tips, several mutations on every branch, hot paths that climb past the first four branch infos, end in the open
branch above the run's root and end at the root of a part that is not the run's.  Then the full move mix runs through the same code on parts
staged whole, by their prefix and not at all, move for move against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import KAPPA, PI, Scenario
from helpers import configure, run_parity, split_parts
from oracle_ffi import OracleBuild, OracleEngine

pytestmark = pytest.mark.gpu

# Chosen on the CPU with the oracle alone (coverage() below needs no device): the first seeds whose single-part AND eight-part cuts each
# meet every count of REQUIRED by themselves were 16, 74 and 117 of 1..119; 117 is the one that cuts into exactly eight parts.
SEED = 117
TIPS, SITES = 100, 300
MU_SCALE = 60.0          # x C1's rate: 4-6 mutations on the average branch of the rebuilt tree, 3-10 on most of a hot path
SPINE_TIPS = 24
MU_PROPOSAL = 1e-3
# Minimum counts over the analysed grafts of ONE cut, from the oracle's results (never the device's)
REQUIRED = {"levels_above_PX >= 2": 20, "branch_infos > 4": 5, "hot mutations": 20, "hot mutations of two levels": 5, "S misses nothing": 10}
REQUIRED_ROOT_PART = {"ends in the open branch": 3, "rooty grafts": 2}
REQUIRED_CUT = {"ends at a non-root part's root": 5}


def _gapped_third(tree, td, sites, spine_tips=SPINE_TIPS, every_tip=False):
    """Tip descriptors with missing stretches at a third of the tips and none at the others.  The third: the tips of the small clades that hang
    off the spine from the root towards the larger clade -- they also share one stretch, so that the analysis of a spine node still slides
    missing sites when it reaches the root -- and then runs of neighbours in leaf order, each with a tip or two that miss nothing in between,
    so that a graft's sibling and the siblings above it miss overlapping sites.  A tip's deltas inside its missing sites are dropped.
    `every_tip`: the generator's gaps kept at every tip instead (no spine, no shared stretch): both children of the root then miss sites."""
    n = td.num_tips
    size = np.ones(tree.num_nodes, np.int64)
    order, pre, stack = [], [], [int(tree.root)]
    while stack:
        v = stack.pop(); pre.append(v)
        if tree.child0[v] < 0:
            order.append(v)
        else:
            stack += [int(tree.child1[v]), int(tree.child0[v])]
    for v in reversed(pre):
        if tree.child0[v] >= 0:
            size[v] = size[tree.child0[v]] + size[tree.child1[v]]

    def leaves(v):
        out, st = [], [v]
        while st:
            u = st.pop()
            if tree.child0[u] < 0:
                out.append(u)
            else:
                st += [int(tree.child0[u]), int(tree.child1[u])]
        return out

    spine, v = [], int(tree.root)
    while tree.child0[v] >= 0:
        a, b = int(tree.child0[v]), int(tree.child1[v])
        small, big = (a, b) if size[a] <= size[b] else (b, a)
        if len(spine) + size[small] > spine_tips:
            break
        spine += leaves(small); v = big
    if every_tip:
        spine = []
    keep = np.full(n, bool(every_tip)); keep[spine] = True
    for pos, t in enumerate(order):
        if keep.sum() >= n // 3:
            break
        if pos % 12 in (0, 1, 3, 4):
            keep[t] = True
    shared = [sites // 3, sites // 3 + 20]
    moff, ms, me, doff, ds, dt = [0], [], [], [0], [], []
    for i in range(n):
        iv = []
        if keep[i]:
            iv = [[int(td.miss_start[k]), int(td.miss_end[k])] for k in range(td.miss_offset[i], td.miss_offset[i + 1])]
            if i in spine:
                merged = []
                for s, e in sorted(iv + [shared]):
                    if merged and s <= merged[-1][1]:
                        merged[-1][1] = max(merged[-1][1], e)
                    else:
                        merged.append([s, e])
                iv = merged
        for s, e in iv:
            ms.append(s); me.append(e)
        moff.append(len(ms))
        for k in range(td.delta_offset[i], td.delta_offset[i + 1]):
            l = int(td.delta_site[k])
            if not any(s <= l < e for s, e in iv):
                ds.append(l); dt.append(int(td.delta_to[k]))
        doff.append(len(ds))
    return d.TipDescs(td.t_min, td.t_max, np.asarray(doff, np.int32), np.asarray(ds, np.int32), np.asarray(dt, np.uint8),
                      np.asarray(moff, np.int32), np.asarray(ms, np.int32), np.asarray(me, np.int32)), int(keep.sum())


@functools.lru_cache(maxsize=None)
def scenario(tips_n=TIPS, sites=SITES, seed=SEED, spine_tips=SPINE_TIPS, every_tip=False):
    """C1-sized, 300 sites, six short gaps per gapped tip: the synthetic tips, gaps kept at a third of them, and the product's default builder's
    tree for those tips (host code) -- so every list of the tree is what the product itself makes of such data.  (Other sizes from the same
    generator with the same gap rule, and `every_tip` gapped: tests/test_graft_model.py's further scenarios.)"""
    p = d.SynthParams(num_tips=tips_n, num_sites=sites, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=MU_SCALE * 1e-3 / 365.0, gaps_per_tip=6, mean_gap_len=25.0, seed=seed)
    p.pi, p.kappa = PI, KAPPA
    tree, ref, tmax = d.make_synthetic_emat(p)
    ob = OracleBuild(ref)
    try:
        tips, gapped = _gapped_third(tree, ob.tip_descs_of(tree), sites, spine_tips, every_tip)
    finally:
        ob.close()
    assert gapped == (tips_n if every_tip else tips_n // 3)
    b = d.EmatBackend(sites, device=-1)
    try:
        b.set_ref_sequence(ref)
        built, built_ref, _ = b.build_default(tips, seed)
    finally:
        b.close()
    return Scenario("graft-paths", built, built_ref, tmax, p.mu, KAPPA, PI, d.PopModel.exp(tmax, 365.0, 0.0, 0.0), sites)


@functools.lru_cache(maxsize=None)
def reference(num_parts):
    """(the cut, {(part, X): the oracle's analysis}) of every X the move code can analyse: every node but the part's root and, in a part that
    does not hold the run's root, the root's children (spr_move_core returns before the analysis there); the children of the run's root in the
    root part are the rooty grafts.  Computed once, never changed."""
    sc = scenario()
    cut = split_parts(sc, num_parts, 11)
    parts, incl, seeds, root_part, ref = cut
    orc = OracleEngine(sc.num_sites)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part)
        want = {}
        for p, t in enumerate(parts):
            for X in range(t.num_nodes):
                if X != t.root and (incl[p] or int(t.parent[X]) != t.root):
                    want[(p, X)] = orc.debug_graft(p, X, MU_PROPOSAL)["grafts"][0]
    finally:
        orc.close()
    return cut, want


def coverage(num_parts):
    (parts, incl, _, _, _), want = reference(num_parts)
    c = dict.fromkeys(list(REQUIRED) + list(REQUIRED_ROOT_PART) + list(REQUIRED_CUT), 0)
    for (p, X), g in want.items():
        bis, t = g["branch_infos"], parts[p]
        if int(t.parent[X]) == t.root:          # a rooty graft: P -> X and P -> S open, S -> P -> X closed; the counts below are the inner grafts'
            c["rooty grafts"] += len(bis) == 3 and [b["is_open"] for b in bis] == [True, True, False]
            continue
        c["levels_above_PX >= 2"] += sum(1 for b in bis[1:] if not b["is_open"]) >= 2
        c["branch_infos > 4"] += len(bis) > 4
        c["ends in the open branch"] += bis[-1]["is_open"]
        c["ends at a non-root part's root"] += (not incl[p]) and len(bis) > 1 and bis[-1]["A"] == t.root
        owners = sum(1 for b in bis if b["hot_muts_to_X"])
        c["hot mutations"] += owners >= 1
        c["hot mutations of two levels"] += owners >= 2
        c["S misses nothing"] += int(t.miss_offset[g["S"] + 1] - t.miss_offset[g["S"]]) == 0
    return c


@pytest.mark.parametrize("num_parts", [1, 8])
def test_every_list_of_the_analysis_equals_the_oracles(num_parts):
    sc = scenario()
    (parts, incl, seeds, root_part, ref), want = reference(num_parts)
    assert len(parts) == num_parts
    gaps = np.diff(sc.tree.miss_offset)[: TIPS]
    muts = np.diff(sc.tree.mut_offset)
    assert np.count_nonzero(gaps) <= TIPS // 3 and 3.0 <= muts.mean() <= 10.0, (np.count_nonzero(gaps), muts.mean())
    have = coverage(num_parts)
    need = dict(REQUIRED, **(REQUIRED_ROOT_PART if num_parts == 1 else REQUIRED_CUT))
    for what, n in need.items():
        assert have[what] >= n, "the scenario must hold %d analyses with '%s' (has %d): %s" % (n, what, have[what], have)
    b = d.EmatBackend(sc.num_sites)
    try:
        configure(b, sc, ref, parts, incl, seeds, root_part)
        for (p, X), w in want.items():
            g = b.debug_graft(p, X, MU_PROPOSAL)["grafts"][0]
            what = "part %d X %d" % (p, X)
            assert (g["X"], g["S"], g["t_P"]) == (w["X"], w["S"], w["t_P"]) and len(g["branch_infos"]) == len(w["branch_infos"]), (what, g, w)
            for i, (gb, wb) in enumerate(zip(g["branch_infos"], w["branch_infos"])):
                for f in ("A", "B", "is_open", "T_to_X", "warm_sites", "hot_sites", "hot_muts_to_X", "hot_deltas_to_X"):     # entry for entry, in order
                    assert gb[f] == wb[f], (what, i, f, gb[f], wb[f])
                for f in ("partial_lambda_at_A", "partial_lambda_at_X"):                                                 # bit for bit
                    assert np.float64(gb[f]).tobytes() == np.float64(wb[f]).tobytes(), (what, i, f, gb[f], wb[f], gb[f] - wb[f])
            assert abs(g["delta_log_G"] - w["delta_log_G"]) <= 1e-9 * max(1.0, abs(w["delta_log_G"])), what
            assert abs(g["log_alpha_mut"] - w["log_alpha_mut"]) <= 1e-9 * max(1.0, abs(w["log_alpha_mut"])), what
    finally:
        b.close()


def test_the_one_walk_split_equals_two_subtractions():
    """iv_split on its own: its difference is the subtraction's, what it leaves is the second subtraction's -- pieces of b that touch come out
    joined, intervals of a that touch stay apart -- on seeded random pairs of sets and on the edges."""
    rng = np.random.default_rng(5)

    def rand_set(maxn, touching):
        out, p = [], int(rng.integers(0, 3))
        for _ in range(int(rng.integers(0, maxn + 1))):
            p += int(rng.integers(0 if touching else 1, 3))
            n = int(rng.integers(1, 5))
            out.append([p, p + n]); p += n
        return out

    cases = [([], []), ([], [[1, 4]]), ([[0, 10]], []), ([[0, 10]], [[2, 4], [4, 6]]), ([[0, 5], [5, 9]], [[3, 7]]), ([[0, 10]], [[2, 4], [3, 12]]),
             ([[2, 6]], [[0, 8]]), ([[2, 6]], [[2, 6]]), ([[0, 300]], [[0, 7], [20, 21], [299, 300]])]
    cases += [(rand_set(5, k % 2 == 1), rand_set(6, k % 3 == 2)) for k in range(60)]
    b = d.EmatBackend(16)
    try:
        for A, B in cases:
            diff = b.debug_interval_op(3, A, B)
            assert b.debug_interval_op(7, A, B) == diff, (A, B)
            assert b.debug_interval_op(8, A, B) == b.debug_interval_op(3, A, diff), (A, B)
    finally:
        b.close()


TRACE = 2000


def _staging_cap(sc, num_parts, variant, monkeypatch):
    """A staging cap (option lds_max through EMAT_LDS_MAX; None = the default) at which a part of the cut runs staged whole / by its prefix.
    The 2 000-move trace lies in front of a part's list heap, so the single part's prefix is 116 KiB, above the default cap: the caps are worked
    out from the parts' slab layouts (host code) and then confirmed by the host's evaluation of the kernel's own per-part decision."""
    lib = d.load_library()
    lib.emat_debug_variant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    (parts, incl, seeds, root_part, ref), _ = reference(num_parts)
    monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
    h = d.EmatBackend(sc.num_sites, device=-1, trace_moves=TRACE)
    try:
        configure(h, sc, ref, parts, incl, seeds, root_part)
        lay = [h.debug_slab_layout(p) for p in range(len(parts))]
    finally:
        h.close()
    begin = [x["header"] + x["nodes"] + x["cells"] + x["trace"] for x in lay]                  # where the list heap begins = the prefix
    top = [b + x["heap_used"] for b, x in zip(begin, lay)]
    up = lambda v: (v + 511) // 512 * 512
    if variant == "whole":
        caps = [None, up(min(top) + 1024) + 512]                                                # (the kernel keeps 1 KiB for the heap to grow into)
    else:
        caps = [up(b) + 512 for b, t in sorted(zip(begin, top)) if up(b) + 512 < t + 1024]
    for cap in caps:
        if cap is None:
            monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
        else:
            monkeypatch.setenv("EMAT_LDS_MAX", str(cap))
        b = d.EmatBackend(sc.num_sites, trace_moves=TRACE)
        try:
            configure(b, sc, ref, parts, incl, seeds, root_part)
            out = (C.c_int32 * 3)()
            assert lib.emat_debug_variant_counts(b.handle, out) == 0
        finally:
            b.close()
        if out[0 if variant == "whole" else 1] > 0:
            return cap
    raise AssertionError("no staging cap of %s runs a part of the %d-part cut %s-staged (layouts %s)" % (caps, num_parts, variant, lay))


@pytest.mark.parametrize("num_parts", [1, 8])
@pytest.mark.parametrize("variant", ["whole", "prefix", "hbm"])
def test_moves_through_the_analysis(num_parts, variant, monkeypatch):
    """2 000 moves of the full mix per part on the same tree and cuts, traced against the oracle move for move."""
    sc = scenario()
    monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
    if variant != "hbm":
        cap = _staging_cap(sc, num_parts, variant, monkeypatch)
        if cap is None:
            monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
        else:
            monkeypatch.setenv("EMAT_LDS_MAX", str(cap))
    st = run_parity(sc, num_parts, 2000, trace=TRACE, use_lds=variant != "hbm")
    assert st["num_parts"] == num_parts and st["moves_done"] == 2000
