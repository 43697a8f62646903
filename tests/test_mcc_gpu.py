"""The store of sampled trees in HBM (emat_tree_sample_*) and the MCC tree derived from it on the device (emat_mcc_derive) against
tests/mcc_model.py: (b), the definitions on sets of tips, EXACTLY -- clade counts, support, topology, corresponding nodes and exact flags
of every sample, and t / t_mrca bit for bit, because the device sums over the samples in sample order as the reference does -- and (a),
derive_mcc_tree to the letter, for log clade credibility and the master.

log_cc bound (derived, not tuned).  The device sums hist[c] (log c - log M) over c ascending, model (a) the same terms node by node.  To
first order a floating-point sum of N terms errs by at most (N - 1) u sum|terms| in any order, u = 2^-53, and the histogram form adds one
rounding per product, u sum|terms| in all; the errors of two orders of the same terms largely cancel, and the bound held to is
mcc_model.log_cc_bound = (n_inner + 2) u sum|terms|, the first-order bound of two summation orders of the same terms, which the model test
holds (a) to against the correctly rounded sum as well.  It is not widened here; the worst observed ratio is printed (0.28 in the sweep).
log c - log M are the same doubles on both sides (the C library's log on both).
The master: mcc_model.expected_master; tests/test_mcc_model.py asserts that no case of this file's sweep is decided by rounding.

Every test needs the new exports and so fails on a library without them.  Measured values are printed (pytest -s) for DESIGN.md section 9."""
import os
import random
import time

import numpy as np
import pytest

import delphy_amd as d
import mcc_model as M
from delphy_amd.scenarios import make_scenario
from test_mcc_model import GPU_SWEEP_CASES, GPU_SWEEP_SEED, check_four_tips, four_tip_samples, sweep_case, tree_from_newick_like

pytestmark = pytest.mark.gpu


def _backend(num_tips, capacity=None):
    sc = make_scenario("C1", num_tips=num_tips, num_sites=60)
    b = d.EmatBackend(sc.num_sites)
    b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree)
    if capacity: b.tree_samples_reserve(capacity)
    return b, sc


def _push(b, s: M.Sample):
    return b.tree_sample_push_flat(s.parent, s.child0, s.child1, s.t, s.root)


def _as_model(r: d.MccTree, b, count) -> M.Mcc:
    corr = np.zeros((count, r.parent.shape[0]), np.int64); exact = np.zeros((count, r.parent.shape[0]), bool)
    for k in range(count): corr[k], exact[k] = b.mcc_correspondence(k)
    return M.Mcc(r.master, list(r.log_cc), [], r.num_exact.astype(np.int64), r.support, r.t, r.t_mrca, corr, exact)


def check_against_models(b, chosen, r: d.MccTree, seed, what):
    """Items 2 and 3 of the module text for one derivation over the samples `chosen`; returns (worst log_cc error / bound, master decided by the bound)."""
    Mn = len(chosen); n_inner = len(chosen[0].inner_nodes())
    a = M.derive_letter(chosen, seed)
    want_master, by_bound = M.expected_master(a, n_inner)
    got = _as_model(r, b, Mn)
    worst = 0.0
    for k in range(Mn):
        bound = M.log_cc_bound(n_inner, a.log_cc_terms_abs[k])
        err = abs(got.log_cc[k] - a.log_cc[k])
        assert err <= bound, (what, k, err, bound)
        if bound > 0: worst = max(worst, err / bound)
    assert got.master == want_master, (what, got.master, want_master, by_bound)
    m = chosen[got.master]
    assert np.array_equal(r.parent, m.parent) and np.array_equal(r.child0, m.child0) and np.array_equal(r.child1, m.child1) and r.root == m.root, what
    s = M.derive_sets(chosen, master=got.master)
    assert np.array_equal(got.num_exact, s.num_exact), what                      # clade counts
    assert np.array_equal(r.support, s.num_exact / float(Mn)) and np.array_equal(r.support, s.support), what
    assert np.array_equal(got.corr, s.corr) and np.array_equal(got.exact, s.exact), what
    assert np.array_equal(r.t, s.t) and np.array_equal(r.t_mrca, s.t_mrca), what   # bit for bit: the sums run in sample order
    for k in range(Mn):                                                          # log_cc's histogram is (b)'s counts of the inner nodes
        terms = sorted(s.inner_counts[k].values())
        assert got.log_cc[k] == sum_in_histogram_order(terms, Mn), (what, k)
    return worst, by_bound


def sum_in_histogram_order(sorted_counts, Mn):
    """What the header says log_cc is: the sum over c ascending of hist[c] (log c - log M)."""
    import math
    out, i = 0.0, 0
    while i < len(sorted_counts):
        j = i
        while j < len(sorted_counts) and sorted_counts[j] == sorted_counts[i]: j += 1
        out += float(j - i) * (math.log(sorted_counts[i]) - math.log(Mn)); i = j
    return out


# ---- 1. the cases worked by hand ----------------------------------------------------------------------------------------------
def test_the_hand_worked_cases_on_the_device():
    b, _ = _backend(4, 8)
    try:
        ss = four_tip_samples()
        assert [_push(b, s) for s in ss] == [0, 1, 2] and b.tree_samples_count() == 3
        r = b.mcc_derive(seed=7)
        check_four_tips(_as_model(r, b, 3))
        assert r.master_index == 0 and r.root == 6 and list(r.parent) == list(ss[0].parent)
        check_against_models(b, ss, r, 7, "four tips")
        # M = 1
        r = b.mcc_derive(first=2, count=1)
        assert r.master == 0 and r.master_index == 2 and list(r.log_cc) == [0.0] and list(r.support) == [1.0] * 7 and np.array_equal(r.t, ss[2].t) and np.array_equal(r.t_mrca, ss[2].t)
        assert list(r.child0) == list(ss[2].child0)
        # all samples identical
        b.tree_samples_clear()
        for s in (ss[0], ss[1], ss[0], ss[1]): _push(b, s)
        r = b.mcc_derive()
        assert r.master == 0 and list(r.log_cc) == [0.0] * 4 and list(r.support) == [1.0] * 7 and r.t[4] == -2.0 and np.array_equal(r.t, r.t_mrca)
    finally:
        b.close()
    b, _ = _backend(2, 2)
    try:
        x = tree_from_newick_like((0, 1), {0: 0.5, 1: 0.25, 2: -1.0}); y = tree_from_newick_like((1, 0), {0: 0.5, 1: 0.25, 2: -2.0})
        _push(b, x); _push(b, y)
        r = b.mcc_derive()
        assert r.master == 0 and list(r.log_cc) == [0.0, 0.0] and list(r.support) == [1.0] * 3 and list(r.t) == [0.5, 0.25, -1.5] and list(r.t_mrca) == [0.5, 0.25, -1.5] and list(r.num_exact) == [2, 2, 2]
    finally:
        b.close()


# ---- 2, 3, 5, 6. the sweep ------------------------------------------------------------------------------------------------------
def test_random_sample_sets_against_both_models_exactly():
    """~200 seeded sets of 2-400 tips and 1-64 samples (EMAT_FUZZ_SEED / EMAT_FUZZ_CASES for other hunts), first / stride varied, every one
    through ONE handle: the resident tree changes size between sets, which makes every push fail until the store is cleared (checked each
    time), and the clear re-binds the store.  Every few sets the derivation is repeated (identical bytes), repeated with another seed
    (identical results), and repeated with the table of clade counts forced down to 4 slots (it grows; identical results)."""
    base = int(os.environ.get("EMAT_FUZZ_SEED", str(GPU_SWEEP_SEED)))
    cases = int(os.environ.get("EMAT_FUZZ_CASES", str(GPU_SWEEP_CASES)))
    b, _ = _backend(2, 64)
    worst = 0.0; by_bound = 0; regrown = 0; t_dev = 0.0
    try:
        for case in range(cases):
            ss = sweep_case(base * 1000 + case, 400, 64)
            num_tips = (ss[0].n + 1) // 2
            sc = make_scenario("C1", num_tips=num_tips, num_sites=60)
            n_before = b.tree_samples_info()[2]
            b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree)
            if n_before != ss[0].n:
                with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_clear first"):
                    _push(b, ss[0])
            b.tree_samples_clear()
            assert b.tree_samples_info() == (0, 64, ss[0].n)
            for s in ss: _push(b, s)
            rng = random.Random(case)
            first = rng.randrange(len(ss)) if rng.random() < 0.5 else 0
            stride = rng.choice((1, 1, 2, 3))
            chosen = ss[first::stride]
            if rng.random() < 0.3: chosen = chosen[:rng.randint(1, len(chosen))]
            t0 = time.perf_counter()
            r = b.mcc_derive(first, len(chosen), stride, seed=case)
            t_dev += time.perf_counter() - t0
            w, bb = check_against_models(b, chosen, r, case, "case %d (%d tips, %d of %d samples, first %d stride %d)" % (case, num_tips, len(chosen), len(ss), first, stride))
            worst = max(worst, w); by_bound += bb
            if case % 4 == 0:
                got = _as_model(r, b, len(chosen))
                r2 = b.mcc_derive(first, len(chosen), stride, seed=case); got2 = _as_model(r2, b, len(chosen))
                assert _bytes(r, got) == _bytes(r2, got2), case
                r3 = b.mcc_derive(first, len(chosen), stride, seed=case + 12345); got3 = _as_model(r3, b, len(chosen))
                assert _bytes(r, got) == _bytes(r3, got3), case
                b.set_option("mcc_table_log2", 2)
                r4 = b.mcc_derive(first, len(chosen), stride, seed=case); got4 = _as_model(r4, b, len(chosen))
                b.set_option("mcc_table_log2", 0)
                assert r4.table_regrows > 0 and r4.table_slots >= 2 * r4.num_distinct_clades and r4.num_distinct_clades == r.num_distinct_clades
                assert _bytes(r, got) == _bytes(r4, got4), case
                regrown += 1
    finally:
        b.close()
    print("sweep: %d cases, worst log_cc error / bound %.3g, master decided within the bound in %d (all exact ties: test_mcc_model), table grown in %d, device time %.2f s" % (cases, worst, by_bound, regrown, t_dev))
    assert regrown > 0


def _bytes(r: d.MccTree, got: M.Mcc):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (r.log_cc, r.parent, r.child0, r.child1, r.support, r.t, r.t_mrca, r.num_exact, got.corr, got.exact)) + bytes([r.master, r.master_index % 256])


# ---- 4. samples pushed from the resident tree over cycles of the run driver --------------------------------------------------------
def test_samples_pushed_after_every_cycle_of_a_run_and_the_mcc_tree_of_them():
    sc = make_scenario("C3")
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    run.set_num_parts(128); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    kept = []
    try:
        for cycle in range(24):
            run.repartition()
            if cycle == 0:
                b.tree_samples_reserve(24)
            if cycle == 1:
                with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_reassemble first"):
                    b.tree_sample_push()
                assert b.tree_samples_count() == 1
            run.run_moves(128 * 400); b.synchronize()
            run.reassemble()
            assert b.tree_sample_push() == cycle
            kept.append(M.Sample(*b.tree_topology()))
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*full"):
            b.tree_sample_push()
        for i, s in enumerate(kept):
            parent, c0, c1, t, root = b.tree_sample_get(i)
            assert np.array_equal(parent, s.parent) and np.array_equal(c0, s.child0) and np.array_equal(c1, s.child1) and np.array_equal(t, s.t) and root == s.root, i
        r = b.mcc_derive(seed=3)
        w1, _ = check_against_models(b, kept, r, 3, "24 cycles")
        assert (r.support[kept[0].inner_nodes()] < 1).any()       # the moves did change the topology
        r2 = b.mcc_derive(first=8, stride=2, seed=4)
        assert len(r2.log_cc) == 8
        w2, _ = check_against_models(b, kept[8::2], r2, 4, "24 cycles, first 8 stride 2")
    finally:
        run.close(); b.close()
    inner = kept[0].inner_nodes()
    print("C3, 24 cycles: %d of %d inner nodes with support < 1, least %.3f; master %d; log_cc error / bound %.3g, %.3g" % (int((r.support[inner] < 1).sum()), len(inner), r.support[inner].min(), r.master, w1, w2))


# ---- 7. states and arguments ----------------------------------------------------------------------------------------------------------
def test_states_and_arguments_are_refused_with_a_text_and_the_next_call_works():
    b, sc = _backend(4)
    ss = four_tip_samples()
    try:
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_reserve first"):
            b.tree_sample_push()
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*capacity must be positive"):
            b.tree_samples_reserve(0)
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*needs .* MB, the device has .* MB free"):
            b.tree_samples_reserve(2 ** 31 - 1)                   # 7 nodes x 41 bytes x 2^31: more than any HBM
        b.tree_samples_reserve(3)
        assert b.tree_sample_push() == 0                          # the resident tree itself: sample 0 says which nodes are tips
        s = ss[0]
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*a tree of 5 nodes"):
            b.tree_sample_push_flat(s.parent[:5], s.child0[:5], s.child1[:5], s.t[:5], 4)
        two_roots = s.copy(); two_roots.parent[4] = -1
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*one root"):
            _push(b, two_roots)
        cyc = s.copy()                                            # 4 and 5 each other's parent and child, beside the tree
        cyc.parent[4], cyc.parent[5] = 5, 4; cyc.child0[4], cyc.child1[4] = 5, 0; cyc.child0[5], cyc.child1[5] = 4, 2
        cyc.child0[6], cyc.child1[6] = 1, 3; cyc.parent[1] = cyc.parent[3] = 6
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*cycle"):
            _push(b, cyc)
        tip_inner = tree_from_newick_like(((0, 1), (2, 3)), {v: 0.0 for v in range(7)})
        m = np.array([4, 1, 2, 3, 0, 5, 6])                       # node 0 and node 4 change places: 0 is an inner node now
        moved = M.Sample(np.full(7, -1, np.int32), np.full(7, -1, np.int32), np.full(7, -1, np.int32), np.zeros(7), 6)
        mm = lambda a: np.where(a == -1, -1, m[np.maximum(a, 0)]).astype(np.int32)
        moved.parent[m] = mm(tip_inner.parent); moved.child0[m] = mm(tip_inner.child0); moved.child1[m] = mm(tip_inner.child1)
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*sample 0"):
            _push(b, moved)
        unary = s.copy(); unary.child1[4] = -1
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT"):
            _push(b, unary)
        assert b.tree_samples_count() == 1
        assert _push(b, ss[1]) == 1 and _push(b, ss[2]) == 2       # the next valid call works
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*full"):
            _push(b, ss[0])
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*full"):
            b.tree_sample_push()
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_clear first"):
            b.tree_samples_reserve(10)                            # nothing is dropped silently
        for args in ((0, 0, 1), (0, 2, 0), (2, 2, 1), (-1, 1, 1), (0, 3, 2), (3, 1, 1)):
            with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT"):
                b.mcc_derive(*args)
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_mcc_derive first"):
            b.mcc_correspondence(0)
        r = b.mcc_derive(1, 2, 1)
        assert r.master == 0 and r.master_index == 1 and list(r.num_exact) == [2, 2, 2, 2, 1, 1, 2]
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT"):
            b.mcc_correspondence(2)
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT"):
            b.tree_sample_get(3)
        # a tree of another size: no push until the store is cleared
        sc6 = make_scenario("C1", num_tips=6, num_sites=60)
        b.tree_upload(sc6.tree)
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_clear first"):
            b.tree_sample_push()
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_clear first"):
            _push(b, ss[0])
        b.tree_samples_clear()
        assert b.tree_samples_info() == (0, 3, 11) and b.tree_sample_push() == 0
        got = b.tree_sample_get(0)
        assert np.array_equal(got[0], sc6.tree.parent) and np.array_equal(got[3], sc6.tree.t) and got[4] == sc6.tree.root
    finally:
        b.close()
    h = d.EmatBackend(60, device=-1)
    try:
        for call in (lambda: h.tree_samples_reserve(2), h.tree_sample_push, lambda: h.mcc_derive(0, 1, 1), h.tree_samples_clear):
            with pytest.raises(d.EmatError, match="EMAT_ERR_NO_DEVICE"):
                call()
    finally:
        h.close()


# ---- 8. full size ---------------------------------------------------------------------------------------------------------------------
def _median_ms(f, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def test_c4_thirty_two_samples_over_thirty_two_cycles_and_what_a_push_costs():
    """Config C4 (199 999 nodes): a sample after each of 32 cycles of the run driver, then the MCC tree of them, checked through properties that
    need no model, and the correspondence of 2 000 MCC nodes against find_MRCA_of by node times folded over the node's tips (model (a)'s walk).
    Times, medians, synchronise included: a push against the two calls it replaces, emat_tree_get_topology and emat_tree_download, each
    measured right after a reassemble (the way a sampler meets them: 32 calls) and as repeated calls (21) on the same tree.  Asserted: a push
    is faster than emat_tree_get_topology, both ways, with no margin.  Nothing else is asserted as a time."""
    sc = make_scenario("C4")
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    P = 8192
    run.set_num_parts(P); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    n = sc.tree.num_nodes
    t_push, t_topo, kept = [], [], {}
    try:
        for cycle in range(32):
            run.repartition()
            if cycle == 0: b.tree_samples_reserve(32 + 21)            # (21 slots for the repeated pushes below)
            run.run_moves(P * 200); b.synchronize()
            run.reassemble(); b.synchronize()
            t0 = time.perf_counter(); b.tree_sample_push(); b.synchronize(); t1 = time.perf_counter()
            topo = b.tree_topology(); t2 = time.perf_counter()
            t_push.append((t1 - t0) * 1e3); t_topo.append((t2 - t1) * 1e3)
            if cycle in (0, 13, 31): kept[cycle] = M.Sample(*topo)
        push_rep = _median_ms(lambda: (b.tree_sample_push(), b.synchronize()), 21)
        topo_rep = _median_ms(b.tree_topology, 21)
        download = _median_ms(b.tree_download, 21)
        t0 = time.perf_counter(); r = b.mcc_derive(0, 32, 1, seed=1); derive_first = (time.perf_counter() - t0) * 1e3
        derive = _median_ms(lambda: b.mcc_derive(0, 32, 1, seed=1), 20)
        corr = {k: b.mcc_correspondence(k) for k in kept}
        master = M.Sample(*b.tree_sample_get(r.master_index))
    finally:
        run.close(); b.close()
    push_cycle, topo_cycle = float(np.median(t_push)), float(np.median(t_topo))
    print("C4 times, ms (medians): push after a reassemble %.3f, emat_tree_get_topology after a reassemble %.3f; repeated: push %.3f, get_topology %.3f, emat_tree_download %.3f; "
          "mcc_derive M = 32: first call %.1f, then %.1f; %d distinct clades, table of %d slots, grown %d times"
          % (push_cycle, topo_cycle, push_rep, topo_rep, download, derive_first, derive, r.num_distinct_clades, r.table_slots, r.table_regrows))
    # properties that need no model
    assert np.array_equal(r.parent, master.parent) and np.array_equal(r.child0, master.child0) and r.root == master.root
    tips = r.child0 < 0; inner = ~tips
    assert r.num_exact[r.root] == 32 and r.support[r.root] == 1.0 and (r.num_exact[tips] == 32).all() and (r.support[tips] == 1.0).all()
    assert (r.num_exact >= 1).all() and (r.num_exact <= 32).all() and np.array_equal(r.support, r.num_exact / 32.0)
    assert r.log_cc[r.master] == r.log_cc.max() and r.master == int(np.argmax(r.log_cc))
    # the master's own log_cc from the counts of ITS nodes, which num_exact are (the MCC tree has the master's nodes)
    assert r.log_cc[r.master] == sum_in_histogram_order(sorted(int(c) for c in r.num_exact[inner]), 32)
    # A node is never later than its children.  For t_mrca that holds always: in every sample the MRCA of more tips is an ancestor of the MRCA of
    # fewer, and sums of termwise smaller doubles in the same order are smaller.  For t it holds where parent and child are both in every sample
    # (the same argument); where their supports differ, t averages over DIFFERENT samples and can come out later than a child's (the reference's
    # does too): counted and printed, not asserted.
    for c in (r.child0, r.child1):
        assert (r.t_mrca[inner] <= r.t_mrca[c[inner]]).all()
        both = inner & (r.num_exact == 32); both[inner] &= r.num_exact[c[inner]] == 32
        assert (r.t[both] <= r.t[c[both]]).all()
    later = int(((r.t[inner] > r.t[r.child0[inner]]) | (r.t[inner] > r.t[r.child1[inner]])).sum())
    print("C4: %d of %d inner nodes with support < 1 (least %.3f); %d have a mean time t later than a child's" % (int((r.support[inner] < 1).sum()), int(inner.sum()), r.support[inner].min(), later))
    assert (r.support[inner] < 1).any()
    # 2 000 MCC nodes: find_MRCA_of by node times folded over the tips below the node, in three of the samples
    rng = random.Random(5)
    sizes = np.zeros(n, np.int64); tip_lists = {}
    order = master.post_order()
    for v in order: sizes[v] = 1 if tips[v] else sizes[master.child0[v]] + sizes[master.child1[v]]
    cand = [v for v in range(n) if inner[v] and sizes[v] <= 300]
    picked = rng.sample(cand, 2000)
    for k, s in kept.items():
        node, ex = corr[k]
        assert np.array_equal(node[tips], np.flatnonzero(tips)) and ex[tips].all()
        ssize = np.zeros(n, np.int64)
        for v in s.post_order(): ssize[v] = 1 if s.child0[v] < 0 else ssize[s.child0[v]] + ssize[s.child1[v]]
        for v in picked:
            below = [u for u in M._below(master, v) if tips[u]]
            want = below[0]
            for u in below[1:]: want = M.find_mrca_by_times(s, want, u)
            assert node[v] == want, (k, v)
            assert bool(ex[v]) == (ssize[want] == len(below)), (k, v)
    assert push_cycle < topo_cycle and push_rep < topo_rep, (push_cycle, topo_cycle, push_rep, topo_rep)
