"""SURVEY 8(f).4, the graft step of k_build_usher_graft (delphy_amd/csrc/emat_build.hpp) at every size class it selects code by, on the
shipped library: each case is hand-built (tests/builder_cases.py), states the kernel condition it selects as an assertion on the oracle's
account of the graft (graft_facts: a precondition on the input, not on the code under test), and then compares the device's tree with
oracle/orc_build.hpp's exactly as test_initial_tree.py does -- root and every field bit for bit, then the reference's closing checks -- on
1 and on 3 workgroups (EMAT_BUILD_BLOCKS), so that both stretch-boundary arithmetics run.  The tip a case is about is always the LAST one:
its facts are then those of the very build that is compared (see graft_facts on the order of the draws).

Classes that NO input reaches, by reading the kernel against the reference:
  dxn = 0 or T = 0 in the composition (the table's `T = 0`, `dxn = 0`, `T = 1024 with dxn = 0`).  A tip without deltas has distance 0 at the
    root, nothing is smaller, and the reference picks above the root whenever that ties: no composition.  A graft point with no mutation above
    it has the root's distance, dxn: above the root again.  So below the root dxn >= 1 and T >= 1 always; the LDS composition (dxn + T <=
    k_g_sd = 1024) therefore has T <= 1023 and dxn <= 1023, its parallel form's `T <= 1024 && dxn < 1024 && T < k_g_path && dxn < k_g_path`
    always hold, and its serial form in LDS runs for L >= 2^22 only (case j).
  T <= k_g_pm as a limit of its own: dxn + T <= k_g_sd = 1024 already excludes T > 1024 (d2 tests the limit that binds, and T = 1536 / 1537
    for the record: both in HBM).
Overflow exits (emat_build_host.hpp: pool_cap = 4 sum(deltas) + 4096, sd_cap = 2 max_deltas + 4096, tie_cap = N + pool_cap):
  3, tie list: a branch with m mutations has m + 1 regions, so the regions are at most (nodes - 1) + pool_top <= N + pool_cap: unreachable.
  2, delta buffer: the list holds one entry per site, so never more than L: unreachable for L <= 4096 + 2 max_deltas.  Beyond that it
    needs a path point that differs from the reference sequence at more than max_deltas + 4096 sites while no tip differs at more than
    max_deltas, i.e. thousands of mutations gathered on one path that parsimony still prefers to the region above the root (cost dxn <=
    max_deltas): not with an input of a few thousand sites; no case, and no hook to force one.  (In LDS: dxn + T <= k_g_sd by selection.)
  1, mutation pool: REACHABLE.  A graft adds nsd mutations, and nsd is not bounded by dxn: the distance counts only sites the tip has, the
    composition also turns back every path mutation at a site the tip MISSES (fix_up_missations drops those later, on the host).  Tips of
    two deltas that miss a block of m path sites add up to m + 1 mutations each: test_mutation_pool_overflows_and_the_host_retries.
Case j (L = 2^22 - 1 and 2^22) is in: handle, oracle and one build take 0.3 s at that length.
On one MI355X the module runs in 30 s, its slowest case (the pool overflow, which builds twice) in 3.3 s; the mutation check of these
cases is in DESIGN.md, (f).4."""
import numpy as np
import pytest

import builder_cases as bc
from oracle_ffi import OracleBuild

L0 = 30011            # room for gap(0) .. gap(256) and some 9 000 private sites
_CACHE = {}


def _prepared(key, make):
    """(ref, descriptors, seed, facts of the last graft) of a case, built once; facts.tree is the oracle's tree of the whole input."""
    if key not in _CACHE:
        ref, tips, seed = make()
        td = bc.write_descs(ref, tips)
        ob = OracleBuild(ref)
        try:
            f = bc.graft_facts(ob, td, seed, td.num_tips - 1)
        finally:
            ob.close()
        print("%s: np %d T %d (%d sites) dxn %d mxn %d nsd %d%s" % (key, f.np, f.T, f.T_sites, f.dxn, f.mxn, f.nsd, " above the root" if f.above_root else ""))
        _CACHE[key] = (ref, td, seed, f)
    return _CACHE[key]


def _compare(case, blocks, monkeypatch):
    ref, td, seed, f = case
    monkeypatch.setenv("EMAT_BUILD_BLOCKS", blocks)
    bc.compare_builds(ref, td, seed, want=f.tree)


BLOCKS = ["1", "3"]


# ---- recipes ----------------------------------------------------------------------------------------------------------------

def _ladder(sizes, private=0, seed=11, L=L0, descending=False):
    """A ladder with sizes[i] sites on rung i; the last tip has `private` more deltas (part of its rung, as far as the builder can tell).
    descending: rung i's sites lie below rung i - 1's.  The composition in HBM edits a sorted list one path mutation at a time, root first,
    by ONE lane, and a cancelled entry closes the gap behind it: with the rungs in descending site order that entry is the list's last, and
    a thousand tips of a thousand deltas each cost a binary search per mutation instead of half a list (minutes on the device)."""
    def make():
        ref = bc.make_ref(L); sites = bc.Sites(L)
        sizes2 = list(sizes); sizes2[-1] += private
        rungs = [sites.take(c) for c in sizes2]
        if descending:
            pool = sorted((s for r in rungs for s in r), reverse=True); rungs = []
            for c in sizes2:
                rungs.append(sorted(pool[:c])); pool = pool[c:]
        return ref, bc.ladder(ref, rungs), seed
    return make


def _stem(m, seed=12):
    """Tip 0 carries z; m tips equal to the reference sequence follow, the first its sibling under the first root, every later one above the
    root: tip 0 ends up m nodes below the root with one mutation on the way.  The last tip carries z and y and belongs on tip 0's branch
    below z: np = m + 1, T = 1, dxn = 2."""
    def make():
        ref = bc.make_ref(L0); z, y = 501, 20002
        tips = [bc.tip(1000.0, bc.alt(ref, [z]))] + bc.stem(m, t0=1010.0) + [bc.tip(1010.0 + 10.0 * m, bc.alt(ref, [z, y]))]
        return ref, tips, seed
    return make


def _three(ref, sites, veiled_extra=False):
    """The 3-tip tree: a ladder of three rungs of five.  veiled_extra: rung 1 has a site inside gap(50), and tip 2 carries eight more deltas
    at sites inside gaps, which a tip with those missing intervals must not count."""
    rungs = [sites.take(5), sites.take(5), sites.take(5)]
    if veiled_extra:
        rungs[1] = sorted(rungs[1] + [bc.Sites.gap(50)[0]])
        rungs[2] = sorted(rungs[2] + [bc.Sites.gap(j)[0] for j in (3, 17, 60, 99, 120, 180, 200, 255)])
    return bc.ladder(ref, rungs)


def _fat_on_three(num_deltas=None, private=0, num_miss=0, seed=13):
    """A fat tip on the 3-tip tree: tip 2's sequence (one site of rung 0 at ANOTHER state: a tree mutation on one of its deltas that is no
    match), private deltas, missing intervals.  It belongs on tip 2's branch below its mutations."""
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0)
        three = _three(ref, sites, veiled_extra=num_miss > 0)
        base = dict(three[2]["deltas"]); s0 = min(three[0]["deltas"]); base[s0] = (base[s0] + 1) % 4
        if base[s0] == ref[s0]: base[s0] = (base[s0] + 1) % 4
        return ref, three + [bc.fat_tip(ref, sites, base, 2000.0, num_deltas=num_deltas, private=private, num_miss=num_miss)], seed
    return make


def _unrelated_on_three(num_deltas, seed=14):
    """A tip that shares nothing with the 3-tip tree: its distance is dxn everywhere, and above the root wins the tie."""
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0)
        return ref, _three(ref, sites) + [bc.tip(2000.0, bc.alt(ref, sites.take(num_deltas), 2))], seed
    return make


def _veiled(nQ, nY=1, nF=0, nQs=0, nQd=0, seed=15):
    """Tip 1 carries Q, tip 2 carries Q and Y: the inner node made for tip 2 gets all of Q, tip 2's branch Y.  The last tip carries Y, F
    (private), Qs (sites of Q at the same state), Qd (sites of Q at another state) and MISSES the rest of Q, one interval: distance |F| +
    |Qd| below Y on tip 2's branch, at least |Y| more anywhere else.  T = |Q| + |Y|, dxn = |Y| + |F| + |Qs| + |Qd|.  (Q empty: tip 2 goes
    above the root instead; the last tip still belongs below Y.)"""
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0 - 3000)
        a = L0 - 2500; Qm = list(range(a, a + nQ - nQs - nQd))
        Qs, Qd, Y, F, z0 = sites.take(nQs), sites.take(nQd), sites.take(nY), sites.take(nF), sites.take(1)
        Q = bc.alt(ref, Qm + Qs + Qd)
        last = dict(bc.alt(ref, Y + Qs)); last.update(bc.alt(ref, Qd, 2)); last.update(bc.alt(ref, F, 3))
        tips = [bc.tip(1000.0, bc.alt(ref, z0)), bc.tip(1010.0, Q), bc.tip(1020.0, {**Q, **bc.alt(ref, Y)}),
                bc.tip(1030.0, last, [(a, a + len(Qm))] if Qm else [])]
        return ref, tips, seed
    return make


def _reverted(seed=16):
    """Tips 1 .. 3: Q; Q + Y; Q - R + Y + Z (|R| = 2 < |Y| = 3: it belongs below Y on tip 2's branch and turns R back on its own).  The last
    tip is tip 3's sequence plus W: its path mutates R on the way down and reverts it further down."""
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0)
        Q, Y, Z, W, z0 = sites.take(20), sites.take(3), sites.take(2), sites.take(1), sites.take(1)
        R = Q[3:5]
        q, y, z, w = bc.alt(ref, Q), bc.alt(ref, Y), bc.alt(ref, Z), bc.alt(ref, W)
        t3 = {s: v for s, v in {**q, **y, **z}.items() if s not in R}
        return ref, [bc.tip(1000.0, bc.alt(ref, z0)), bc.tip(1010.0, q), bc.tip(1020.0, {**q, **y}), bc.tip(1030.0, t3), bc.tip(1040.0, {**t3, **w})], seed
    return make


def _bush(count, odd, seed):
    def make():
        ref = bc.make_ref(L0)
        return ref, bc.bush(ref, 7001, count, q=12345 if odd else None), seed
    return make


# ---- a, b, f2, f3: the path ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("depth", [1023, 1024, 1025])
def test_path_found_or_walked_on_a_ladder(depth, blocks, monkeypatch):
    """Row a (and f, f3): `np <= k_g_path` (1024): the path is found by the workgroup and sorted in LDS, else walked into b.path.  One delta
    per rung: T = np and dxn = np + 1, so the composition runs in HBM on either path buffer -- np = 1023 / 1024 is round 4's combination
    (row f: the path fits, dxn + T does not), np = 1025 is row f3 (both over)."""
    case = _prepared(("deep ladder", depth), _ladder([1] * (depth + 1), descending=True))
    f = case[3]
    assert not f.above_root and f.np == depth and f.T == depth and f.dxn == depth + 1
    assert (f.np <= 1024) == (depth <= 1024) and f.dxn + f.T > 1024
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("depth", [1023, 1024, 1025])
def test_path_found_or_walked_with_everything_else_small(depth, blocks, monkeypatch):
    """Rows a and f2: np = 1023 / 1024 (found; composition in LDS, parallel, T = 1) / 1025 (walked: `np > k_g_path` sends the composition
    to HBM although dxn + T = 3) on a stem: a path without mutations but one."""
    case = _prepared(("stem", depth), _stem(depth - 1))
    f = case[3]
    assert not f.above_root and f.np == depth and f.T == 1 and f.dxn == 2 and f.nsd == 1
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_path_walked_under_a_fat_last_tip(blocks, monkeypatch):
    """Row f3 with room to spare: np = 1030 > k_g_path, dxn + T = 2361 > k_g_sd, nsd = 301."""
    case = _prepared("f3", _ladder([1] * 1031, private=300, descending=True))
    f = case[3]
    assert not f.above_root and f.np == 1030 and f.np > 1024 and f.dxn + f.T == 2361 and f.nsd == 301
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("depth", [64, 65])
def test_path_sorted_by_one_wave_or_in_lds(depth, blocks, monkeypatch):
    """Row b: the found path is padded to P2 >= np, a power of two: `P2 <= 64` sorts in one wave's registers, else bitonic in LDS."""
    case = _prepared(("ladder", depth), _ladder([1] * (depth + 1)))
    f = case[3]
    assert not f.above_root and f.np == depth and f.dxn + f.T == 2 * depth + 1 <= 1024
    _compare(case, blocks, monkeypatch)


# ---- c: staging of the new tip -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("dxn,mxn", [(2048, 0), (2049, 0), (40, 256), (40, 257), (2049, 257), (2048, 257), (2049, 256)])
def test_new_tip_staged_in_lds_or_scanned_in_hbm(dxn, mxn, blocks, monkeypatch):
    """Rows c, c2, c3: `dxn <= k_x_deltas && mxn <= k_x_miss` (2048, 256) stages the new tip's descriptor in LDS, else b_step searches it
    in HBM.  With missing intervals the tree has eight mutations on tip 2's branch and one above it at sites the tip misses, and one on a
    site where the tip has another state: counted as differences they would make tip 1's branch the cheaper place."""
    case = _prepared(("fat", dxn, mxn), _fat_on_three(num_deltas=dxn, num_miss=mxn))
    f = case[3]
    assert f.dxn == dxn and f.mxn == mxn and not f.above_root
    assert f.S == 2 and f.np == 3 and f.T == (24 if mxn else 15)          # on tip 2's branch, below all its mutations
    _compare(case, blocks, monkeypatch)


# ---- d, e, f: where the deltas are composed ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("total", [1024, 1025])
def test_composition_in_lds_or_hbm_by_deltas_plus_path_mutations(total, blocks, monkeypatch):
    """Row d: `dxn + T <= k_g_sd` (1024) with np = 3: a ladder of four tips, a hundred sites per rung, T = 300."""
    case = _prepared(("d", total), _ladder([100, 100, 100, 100], private=total - 700))
    f = case[3]
    assert not f.above_root and f.np == 3 and f.T == 300 and f.dxn + f.T == total
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("T", [1023, 1024])
def test_composition_limit_that_binds_at_the_most_path_mutations(T, blocks, monkeypatch):
    """Row d2, the limit that can bind: T <= k_g_pm (1536) never decides, because dxn >= 1 below the root and dxn + T <= k_g_sd (1024)
    is asked as well.  The most path mutations LDS ever holds: T = 1023 with dxn = 1; T = 1024 with dxn = 1 goes to HBM.  (A tip that
    misses the 1 022 / 1 023 sites its path mutates: nsd = T - 1.)"""
    case = _prepared(("veiled", T), _veiled(T - 1))
    f = case[3]
    assert not f.above_root and f.T == T and f.dxn == 1 and f.mxn == 1 and f.nsd == T - 1 and (f.dxn + f.T <= 1024) == (T == 1023)
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("T", [1536, 1537])
def test_composition_in_hbm_around_the_path_mutation_area(T, blocks, monkeypatch):
    """Row d2 as the table states it: T = k_g_pm and k_g_pm + 1.  Both run in HBM (dxn + T > 1024 whatever dxn)."""
    case = _prepared(("d2", T), _ladder([512, 512, T - 1024, 1]))
    f = case[3]
    assert not f.above_root and f.np == 3 and f.T == T and f.dxn == T + 1 and f.nsd == 1
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1023])
def test_parallel_composition_sorts_its_keys_by_one_wave_or_in_lds(T, blocks, monkeypatch):
    """Row e with dxn = 1 (the least below the root): T = 1, 63, 64 (`P2 <= 64`: one wave), 65 (bitonic in LDS), 1023 (the most).  The tip's
    one delta is at a path site and cancels; every other path mutation is turned back at a site the tip misses."""
    case = _prepared(("veiled", T), _veiled(T - 1))
    f = case[3]
    assert not f.above_root and f.T == T and f.dxn == 1 and f.nsd == T - 1 and f.dxn + f.T <= 1024
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_parallel_composition_with_the_most_own_deltas(blocks, monkeypatch):
    """Row e: dxn = 1023 (`tid == dxn` is the last thread that writes a rank), T = 1."""
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0); z = sites.take(1)
        return ref, [bc.tip(1000.0, bc.alt(ref, z)), bc.tip(1010.0), bc.tip(1020.0, {**bc.alt(ref, z), **bc.alt(ref, sites.take(1022), 2)})], 17
    case = _prepared("e-dxn1023", make)
    f = case[3]
    assert not f.above_root and f.T == 1 and f.dxn == 1023 and f.nsd == 1022
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_parallel_composition_merges_runs_with_the_tips_own_deltas(blocks, monkeypatch):
    """Row e, the per-site run and the rank merge: 40 path sites of which the tip shares 12 (the entry cancels: `has` goes false), has 9 at
    ANOTHER state (the entry stays, from the path's state), misses 19 (a run with no entry to start from) -- between 30 private deltas."""
    case = _prepared("e-merge", _veiled(37, nY=3, nF=30, nQs=9, nQd=9))
    f = case[3]
    assert not f.above_root and f.T == 40 and f.dxn == 3 + 30 + 9 + 9 and f.nsd == 30 + 9 + 19 and f.T_sites == f.T
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_parallel_composition_of_a_site_reverted_down_the_path(blocks, monkeypatch):
    """Row e: two sites mutate on the way down and are reverted further down (runs of two calls at one site, which leave nothing)."""
    case = _prepared("e-reverted", _reverted())
    f = case[3]
    assert not f.above_root and f.S == 3 and f.T == 27 and f.T_sites == 25 and f.dxn == 24 and f.nsd == 1
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_parallel_composition_on_a_ladder(blocks, monkeypatch):
    """Row e: every path site is one of the tip's own deltas (65 runs that cancel an entry, 13 entries left alone)."""
    case = _prepared("e-ladder", _ladder([13] * 6))
    f = case[3]
    assert not f.above_root and f.np == 5 and f.T == 65 and f.dxn == 78 and f.nsd == 13
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_found_path_read_by_the_composition_in_hbm(blocks, monkeypatch):
    """Row f, round 4's combination: `np <= k_g_path` (the path is in s_path) while `dxn + T > k_g_sd` (the composition runs in HBM)."""
    case = _prepared("f", _fat_on_three(num_deltas=1100))
    f = case[3]
    assert not f.above_root and f.np == 3 and f.np <= 1024 and f.T == 15 and f.dxn + f.T == 1115 > 1024
    _compare(case, blocks, monkeypatch)


# ---- g: the tying regions ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("count,odd,seed,chunk", [(514, False, 3, 0), (514, True, 1, 0), (514, True, 70, 1), (514, True, 282, 1), (1052, False, 1, 0), (1052, False, 2, 1), (1052, False, 22, 2)])
def test_tying_regions_summed_a_chunk_at_a_time(count, odd, seed, chunk, blocks, monkeypatch):
    """Row g: the two loops over the tying regions, 1 024 at a time: n_tie = 1024 (one full chunk), 1025 (one region in the second), 2100
    (three), and the draw landing in chunk `chunk`.  n_tie and the drawn region's index come from bush_account (see there): 2 X - 2 regions
    for the X-th tip of a bush, one more with the q mutation."""
    case = _prepared(("bush", count, odd, seed), _bush(count, odd, seed))
    ref, td, _, f = case
    n_tie, drawn = bc.bush_account(f.tree, td, 7001)
    print("bush of %d tips%s, seed %d: n_tie %d, region drawn %d" % (count, " with q" if odd else "", seed, n_tie, drawn))
    X = count - 1
    assert n_tie == 2 * X - 2 + (1 if odd else 0) and n_tie in (1024, 1025, 2100) and not f.above_root and f.dxn == 1
    assert drawn // 1024 == chunk
    _compare(case, blocks, monkeypatch)


# ---- h, i: above the root, and the sort of the new mutations ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("dxn", [1024, 1025, 1536, 1537, 2049])
def test_above_the_root(dxn, blocks, monkeypatch):
    """Rows h and i: a tip unrelated to the 3-tip tree goes above the root with nsd = dxn: `dxn <= k_g_sd` (1024) keeps its deltas in LDS,
    `nsd <= k_g_pm` (1536) sorts its new mutations in LDS, else in the pool; 2049 is also past the staging of the tip itself."""
    case = _prepared(("h", dxn), _unrelated_on_three(dxn))
    f = case[3]
    assert f.above_root and f.dxn == dxn and f.nsd == dxn
    _compare(case, blocks, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("nsd", [1536, 1537])
def test_new_mutations_sorted_in_lds_or_in_the_pool_below_the_root(nsd, blocks, monkeypatch):
    """Row i below the root: nsd = 1536 / 1537 after a composition in HBM (15 path mutations, 14 of which cancel a delta of the tip)."""
    case = _prepared(("i", nsd), _fat_on_three(num_deltas=nsd + 14))
    f = case[3]
    assert not f.above_root and f.nsd == nsd and f.T == 15
    _compare(case, blocks, monkeypatch)


# ---- j: the key of the parallel composition ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("L", [(1 << 22) - 1, 1 << 22])
def test_sites_up_to_the_key_limit(L, blocks, monkeypatch):
    """Row j: the parallel composition sorts `site << 10 | index` in 32 bits: `b.L < 2^22`.  At L = 2^22 - 1 with the path's mutations at the
    last sites the top key bits are in use; at L = 2^22 the composition is the serial one in LDS (the only way into it, see above)."""
    def make():
        ref = bc.make_ref(L)
        return ref, bc.ladder(ref, [[L - 1 - 3 * i] for i in range(12)]), 19
    case = _prepared(("j", L), make)
    f = case[3]
    assert not f.above_root and f.np == 11 and f.T == 11 and f.dxn == 12 and f.dxn + f.T <= 1024 and f.max_path_site == L - 1
    _compare(case, blocks, monkeypatch)


# ---- the overflow exits ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
def test_mutation_pool_overflows_and_the_host_retries(blocks, monkeypatch):
    """Status 1.  Tip 1 carries a block Q of 900 sites, tip 2 Q and y, so Q sits on the inner branch above tip 2 and y on the lineage of
    tip 2 (the trunk).  Eighty tips then carry y, a private delta and a hundred sites of Q each (C_i, drawn by a seeded generator) and MISS
    the rest of Q: distance 1 anywhere on the trunk below y, where such a tip turns the 800 sites it misses back (in LDS: dxn + T = 1003): 801 new mutations for 102
    deltas.  (C_i keeps them apart: the branch of an earlier such tip turns C_i back too, some ninety mutations the later tip DOES see; and they
    are dated right after tip 2, so that those branches are no longer than the trunk.)
    Where each lands still depends on the draws, so the precondition counts on the oracle's tree those that landed on the trunk (the inner
    node made for the tip is an ancestor of tip 2) and asks that they alone outgrow the first pool: the kernel must stop at status 1 and
    the host start over with a larger pool, to the same tree."""
    m, K, c = 900, 80, 100
    def make():
        ref = bc.make_ref(L0); sites = bc.Sites(L0 - 3000); rng = np.random.default_rng(29)
        a = L0 - 2500; Q = bc.alt(ref, range(a, a + m)); y = bc.alt(ref, sites.take(1))
        tips = [bc.tip(1000.0, bc.alt(ref, sites.take(1))), bc.tip(1010.0, Q), bc.tip(1020.0, {**Q, **y})]
        for i in range(K):
            C = set(int(x) for x in a + rng.choice(m, size=c, replace=False))
            miss, s = [], a
            while s < a + m:                                           # the maximal runs of Q - C_i
                if s in C: s += 1; continue
                e = s
                while e < a + m and e not in C: e += 1
                miss.append((s, e)); s = e
            tips.append(bc.tip(1020.0 + (i + 1) / 64.0, {**y, **bc.alt(ref, sites.take(1)), **{x: Q[x] for x in C}}, miss))
        return ref, tips, 23
    case = _prepared("pool", make)
    ref, td, seed, f = case
    n = td.num_tips; tr = f.tree
    assert int(np.max(np.diff(td.miss_offset))) <= 256
    trunk = set()
    v = int(tr.parent[2])
    while v != -1:
        trunk.add(v); v = int(tr.parent[v])
    landed = sum(1 for V in range(3, n) if V + n - 1 in trunk)
    pool_cap = 4 * int(td.delta_offset[n]) + 4096
    print("pool: %d of %d veiled tips on the trunk, at least %d mutations against a first pool of %d" % (landed, K, 2 + m + landed * (m - c + 1), pool_cap))
    assert 2 + m + landed * (m - c + 1) > pool_cap
    _compare(case, blocks, monkeypatch)
