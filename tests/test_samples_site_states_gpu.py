"""Samples that keep their mutations (emat_tree_samples_reserve_mutations, the pushes, emat_tree_sample_get_mutations) and the site-state
prober over all kept samples in one call (emat_tree_samples_probe_site_states, emat_mcc_probe_site_states): against the reference's
fixtures, against the single-tree device call (emat_tree_probe_site_states) bit for bit, against tests/samples_site_states_model.py per
sample and site, and against numpy for the summaries.

Bounds (derived, not tuned).  Per (sample, site) the end-to-end bound of test_probe_gpu.py, computed by samples_site_states_model.model_one:
1e-12 + 3 eps cells.  Against the single-tree call, between chunk sizes and between the MCC form and the direct one: identical bytes.
Mean and order statistics: the doubles numpy gives for the same order of additions, and for a sort, exactly.

Every test needs the new exports and so fails on a library without them.  Measured maxima are printed (pytest -s) for DESIGN.md section 9."""
import random

import numpy as np
import pytest

import delphy_amd as d
import prober_model as M
import samples_probe_model as SP
import samples_site_states_model as SS
from delphy_amd.scenarios import make_scenario
from prober_golden import G, check_prober_case, flat_tree, pop_model

pytestmark = pytest.mark.gpu


def _backend(num_tips, capacity, records):
    """A handle with SS.NUM_SITES sites whose store is bound to trees of `num_tips` tips, with mutation room when `records` > 0."""
    sc = make_scenario("C1", num_tips=num_tips, num_sites=SS.NUM_SITES)
    b = d.EmatBackend(sc.num_sites)
    b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree)
    b.tree_samples_reserve(capacity)
    if records: b.tree_samples_reserve_mutations(records)
    return b


def _rebind(b, num_tips, capacity, records):
    """The store follows the resident tree's node count; the mutation room is made for the new slots."""
    sc = make_scenario("C1", num_tips=num_tips, num_sites=SS.NUM_SITES)
    b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree); b.tree_samples_clear()
    b.tree_samples_reserve(capacity)
    b.tree_samples_reserve_mutations(records)


def _push(b, s):
    return b.tree_sample_push_flat_mutations(*s.push_args())


def _lists(off, site, frm, to, t):
    """Per node the records of its list, in order."""
    return [list(zip(site[off[v]:off[v + 1]].tolist(), frm[off[v]:off[v + 1]].tolist(), to[off[v]:off[v + 1]].tolist(), t[off[v]:off[v + 1]].tolist())) for v in range(len(off) - 1)]


def _same(r, q):
    return r.p.tobytes() == q.p.tobytes() and r.mean.tobytes() == q.mean.tobytes() and np.array_equal(r.cells_to_skip, q.cells_to_skip)


# ---- 1. the reference's own fixtures through the batched path -------------------------------------------------------------------
@pytest.mark.parametrize("case", G["site_states_tree_prober"], ids=lambda c: c["test"])
def test_the_reference_fixtures_through_the_batched_path(case):
    tree, ref = flat_tree(case["tree"])
    b = d.EmatBackend(len(ref))
    try:
        b.set_ref_sequence(ref); b.tree_upload(tree); b.tree_samples_reserve(3); b.tree_samples_reserve_mutations(64)
        for k in range(3):
            assert b.tree_sample_push() == k
        pop = pop_model(case["pop"])
        args = (case["t_start"], case["t_end"], case["num_t_cells"])
        r = b.tree_samples_probe_site_states(pop, [case["site"]], *args)
        assert r.p.shape == (3, 1, 4, case["num_t_cells"]) and r.mean.shape == (1, 4, case["num_t_cells"])
        want = M.probe_site_states_on_tree(tree, ref, M.OraclePop(pop), case["site"], *args)
        for k in range(3):
            check_prober_case(case, r.p[k, 0], "%s, sample %d" % (case["test"], k))
            assert np.max(np.abs(r.p[k, 0] - want)) <= SP.P_TOL
            assert r.p[k].tobytes() == r.p[0].tobytes()
        assert r.p[0, 0].tobytes() == b.tree_probe_site_states(pop, case["site"], *args).tobytes()
    finally:
        b.close()


# ---- 2. bit for bit against the single-tree call ---------------------------------------------------------------------------------
def test_bit_for_bit_what_the_single_tree_call_gave_for_each_sample_and_site():
    sc = make_scenario("C1", num_tips=150, num_sites=60)
    L = sc.num_sites
    b = d.EmatBackend(L)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    run.set_num_parts(4); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    t_root, span = float(sc.tree.t[sc.tree.root]), sc.t_max_tip - float(sc.tree.t[sc.tree.root])
    windows = [(t_root - 0.5 * span, sc.t_max_tip + 1.0, 50), (t_root + 0.45 * span, sc.t_max_tip + 1.0, 37)]
    family = SP.pops_for(sc.t_max_tip, t_root)
    pops, recorded, roots, downloads = [], [[], []], [], []
    try:
        for cycle in range(6):
            run.repartition()
            if cycle == 0:
                b.tree_samples_reserve(6); b.tree_samples_reserve_mutations(6 * (4 * int(sc.tree.mut_offset[sc.tree.num_nodes]) + 256))
            run.run_moves(4 * 300); b.synchronize()
            run.reassemble()
            assert b.tree_sample_push() == cycle
            roots.append(b.tree_kids()[2])
            downloads.append(b.tree_download())
            pop = family[cycle % 3]                                                  # constant, exponential, Skygrid in turn
            pops.append(pop)
            for i, w in enumerate(windows):                                          # every site: which three are compared is known only once all samples are in
                recorded[i].append(np.stack([b.tree_probe_site_states(pop, s, *w) for s in range(L)]))
        assert all(r < windows[1][0] for r in roots) and all(r > windows[0][0] for r in roots)     # the windows start before and after every root
        per_site = np.zeros(L, np.int64)
        for tree, _ in downloads: per_site += np.bincount(tree.mut_site[:int(tree.mut_offset[tree.num_nodes])], minlength=L)
        first_site = int(sc.tree.mut_site[0])
        never = int(np.flatnonzero(per_site == 0)[0])
        rest = [s for s in np.argsort(-per_site, kind="stable").tolist() if s not in (first_site, never)]
        sites = [first_site, never, rest[0]]
        first = []
        for i, w in enumerate(windows):
            r = b.tree_samples_probe_site_states(pops, sites, *w)
            want = np.stack([recorded[i][k][sites] for k in range(6)])
            assert r.p.shape == want.shape == (6, 3, 4, w[2])
            assert r.p.tobytes() == want.tobytes(), "window %d: largest difference %.3g" % (i, float(np.max(np.abs(r.p - want))))
            assert (r.cells_to_skip > 0).all() if i == 1 else not r.cells_to_skip.any()
            first.append(r)
        for chunk in (0, 1, 4):
            b.set_option("samples_probe_chunk", chunk)
            for i, w in enumerate(windows):
                assert _same(first[i], b.tree_samples_probe_site_states(pops, sites, *w)), (chunk, i)
        b.set_option("samples_probe_chunk", 0)
        used, cap, sites_bound = b.tree_samples_mutation_info()
        assert sites_bound == L and sum(int(t.mut_offset[t.num_nodes]) for t, _ in downloads) <= used <= cap
        for k, (tree, ref) in enumerate(downloads):                                   # every slot holds that cycle's lists and reference sequence
            off, site, frm, to, t, got_ref = b.tree_sample_get_mutations(k)
            nm = int(tree.mut_offset[tree.num_nodes])
            assert np.array_equal(off, tree.mut_offset[:tree.num_nodes + 1]) and np.array_equal(got_ref, ref), k
            assert _lists(off, site, frm, to, t) == _lists(tree.mut_offset, tree.mut_site[:nm], tree.mut_from[:nm], tree.mut_to[:nm], tree.mut_t[:nm]), k
        run.repartition()                                                            # the parts are out: the store is still there to be probed
        for i, w in enumerate(windows):
            assert _same(first[i], b.tree_samples_probe_site_states(pops, sites, *w)), i
        run.run_moves(4 * 10); b.synchronize(); run.reassemble()
    finally:
        run.close(); b.close()
    print("six cycles: sites %s, mutations per sample %s" % (sites, [int(t.mut_offset[t.num_nodes]) for t, _ in downloads]))


def test_bit_for_bit_at_every_mutated_site_of_a_run():
    """The 299-node scenario above has one mutation; this one has twenty, so that the branches that fade from one state into another are
    held to the single-tree call's bits too, at every site any kept sample mutates, in one call."""
    sc = make_scenario("C1", num_tips=60, num_sites=2000)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 3)
    run.set_num_parts(3); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    t_root, span = float(sc.tree.t[sc.tree.root]), sc.t_max_tip - float(sc.tree.t[sc.tree.root])
    w = (t_root + 0.2 * span, sc.t_max_tip + 1.0, 41)
    family = SP.pops_for(sc.t_max_tip, t_root)
    trees = []
    try:
        for cycle in range(3):
            run.repartition()
            if cycle == 0:
                b.tree_samples_reserve(3); b.tree_samples_reserve_mutations(3 * (4 * int(sc.tree.mut_offset[sc.tree.num_nodes]) + 256))
            run.run_moves(3 * 500); b.synchronize()
            run.reassemble()
            assert b.tree_sample_push() == cycle
            trees.append(b.tree_download()[0])
        sites = sorted({int(s) for t in trees for s in t.mut_site[:int(t.mut_offset[t.num_nodes])]})
        assert len(sites) >= 10
        r = b.tree_samples_probe_site_states(family, sites, *w)                        # the samples are in the store; the last is also the resident tree
        last = np.stack([b.tree_probe_site_states(family[2], s, *w) for s in sites])
        assert r.p[2].tobytes() == last.tobytes(), float(np.max(np.abs(r.p[2] - last)))
        for k in range(2):                                                          # the earlier ones: uploaded again as the resident tree
            off, site, frm, to, t, ref = b.tree_sample_get_mutations(k)
            tree = trees[k]
            assert np.array_equal(off, tree.mut_offset[:tree.num_nodes + 1]) and np.array_equal(site, tree.mut_site[:off[-1]]) and np.array_equal(to, tree.mut_to[:off[-1]])
            b2 = d.EmatBackend(sc.num_sites)
            try:
                b2.set_ref_sequence(ref); b2.tree_upload(tree)
                single = np.stack([b2.tree_probe_site_states(family[k], s, *w) for s in sites])
            finally:
                b2.close()
            assert r.p[k].tobytes() == single.tobytes(), (k, float(np.max(np.abs(r.p[k] - single))))
        fading = sum(int(np.any((r.p[k, i] > 1e-9).sum(axis=0) > 1)) for k in range(3) for i in range(len(sites)))
        assert fading > 0                                                           # some (sample, site) does hold two states at once
    finally:
        run.close(); b.close()
    print("three cycles: %d sites mutated in some sample, two states at once in %d (sample, site) pairs" % (len(sites), fading))


# ---- 3. against the model on seeded sample sets, per sample and site ----------------------------------------------------------------
def test_seeded_sample_sets_against_the_model():
    b = _backend(2, 1, 1)
    worst = 0.0; differing = 0; seen = set()
    try:
        for case, (tips, pushed, first, stride, cells, spec, split) in enumerate(SS.gpu_cases()):
            ss, special = SS.sample_set(case + 1, tips, pushed)
            _rebind(b, tips, pushed, sum(int(s.mut_offset[s.n]) for s in ss) + 1)
            for k, s in enumerate(ss): assert _push(b, s) == k
            chosen = ss[first::stride]
            rng = random.Random(1000 + case)
            sites = SS.sites_of(spec, special)
            t_start, t_end = SS.window(chosen, rng, split)
            family = SP.pops_for(t_end, min(float(s.t[s.root]) for s in chosen))
            pops = [family[(case + k) % 3] for k in range(len(chosen))] if case % 2 else [family[case % 3]]
            what = "case %d (%d tips, %d of %d samples, first %d stride %d, %d cells, sites %s)" % (case, tips, len(chosen), pushed, first, stride, cells, sites)
            b.set_option("samples_probe_chunk", (0, 1, 3)[case % 3])
            r = b.tree_samples_probe_site_states(pops, sites, t_start, t_end, cells, first=first, count=len(chosen), stride=stride)
            assert r.p.shape == (len(chosen), len(sites), 4, cells), what
            want, _, _, skip, tol = SS.model_batched(chosen, pops, sites, t_start, t_end, cells)
            assert np.array_equal(r.cells_to_skip, skip), what
            err = np.max(np.abs(r.p - want), axis=(2, 3))
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), "%s: off by up to %.3g of the bound" % (what, float(np.max(err / tol)))
            for i, a in enumerate(sites):                                                # a site given twice gets the same answer twice
                for j in range(i): assert sites[j] != a or r.p[:, i].tobytes() == r.p[:, j].tobytes(), what
            if split and len({float(s.t[s.root]) for s in chosen}) > 1:
                assert len(set(r.cells_to_skip.tolist())) > 1 and (r.cells_to_skip == 0).any(), what          # grids extended per sample, not per call
                differing += 1
            seen.add((ss[0].n, len(chosen), cells, len(sites)))
    finally:
        b.close()
    assert {3, 255, 257, 511, 513} <= {c[0] for c in seen} and {1, 2, 3, 65, 100} <= {c[1] for c in seen}
    assert {1, 63, 64, 65, 1000} <= {c[2] for c in seen} and {1, 2, 3, 5} <= {c[3] for c in seen} and differing >= 10
    print("seeded sets: %d cases, cells_to_skip differs within the call in %d; largest error / bound %.3g" % (len(seen), differing, worst))


# ---- 4. summaries, exactly -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 65])
def test_mean_and_order_statistics_are_numpys(count):
    tips = 4
    ss, special = SS.sample_set(500 + count, tips, count)
    rng = random.Random(count)
    b = _backend(tips, count, sum(int(s.mut_offset[s.n]) for s in ss) + 1)
    try:
        for s in ss: _push(b, s)
        sites = [special["root"], special["never"], special["tip"]]
        t_start, t_end = SS.window(ss, rng, True)
        pop = SP.pops_for(t_end, t_start)[1]
        ranks = [0, count - 1, count // 2, count - 1, 0]                                             # ends, repeated, unsorted
        r = b.tree_samples_probe_site_states(pop, sites, t_start, t_end, 9, ranks=ranks)
        assert r.p.shape == (count, 3, 4, 9) and r.mean.shape == (3, 4, 9) and r.order_stats.shape == (5, 3, 4, 9)
        total = np.zeros(r.p.shape[1:])
        for k in range(count): total = total + r.p[k]                                              # sample order; np.mean sums in another
        assert r.mean.tobytes() == (total / count).tobytes()
        srt = np.sort(r.p, axis=0)
        for j, q in enumerate(ranks):
            assert r.order_stats[j].tobytes() == srt[q].tobytes(), (j, q)
        for arr in (r.p, r.mean[None]):                                                            # the four states of a site sum to 1
            states = np.zeros(arr[:, :, 0, :].shape)
            for m in range(4): states = states + arr[:, :, m, :]
            assert np.all(np.abs(states - 1.0) <= 1e-12)
        q = b.tree_samples_probe_site_states(pop, sites, t_start, t_end, 9, ranks=ranks, per_sample=False)
        assert q.p is None and q.mean.tobytes() == r.mean.tobytes() and q.order_stats.tobytes() == r.order_stats.tobytes()
        assert np.array_equal(q.cells_to_skip, r.cells_to_skip)
    finally:
        b.close()


# ---- 5. the MCC form ---------------------------------------------------------------------------------------------------------------
def test_the_mcc_form_probes_the_samples_of_the_last_derivation():
    tips, pushed = 9, 9
    ss, special = SS.sample_set(40, tips, pushed)
    b = _backend(tips, pushed, sum(int(s.mut_offset[s.n]) for s in ss) + 1)
    try:
        for s in ss: _push(b, s)
        b.mcc_derive(first=2, stride=2)
        chosen = ss[2::2]
        t_start, t_end = SS.window(chosen, random.Random(5), True)
        pops = SP.pops_for(t_end, t_start)
        sites = [special["tip"], special["root"], 0, special["never"]]
        for pop_arg in (pops[2], [pops[k % 3] for k in range(len(chosen))]):
            got = b.mcc_probe_site_states(pop_arg, sites, t_start, t_end, 12, ranks=[0, len(chosen) - 1])
            direct = b.tree_samples_probe_site_states(pop_arg, sites, t_start, t_end, 12, first=2, count=len(chosen), stride=2, ranks=[0, len(chosen) - 1])
            assert got.p.shape == (len(chosen), 4, 4, 12)
            assert _same(got, direct) and got.order_stats.tobytes() == direct.order_stats.tobytes()
    finally:
        b.close()


# ---- 6. opt-in means opt-in --------------------------------------------------------------------------------------------------------
def test_a_store_with_mutation_room_derives_and_probes_ancestors_as_one_without():
    tips, pushed = 12, 8
    ss, _ = SS.sample_set(41, tips, pushed)
    b = _backend(tips, pushed, 0)
    results = []
    try:
        t_start, t_end = SS.window(ss, random.Random(6), True)
        pop = SP.pops_for(t_end, t_start)[0]
        for with_room in (False, True):
            if with_room:
                b.tree_samples_clear(); b.tree_samples_reserve_mutations(sum(int(s.mut_offset[s.n]) for s in ss) + 1)
            assert (b.tree_samples_mutation_info()[1] > 0) == with_room
            for s in ss:
                if with_room: _push(b, s)
                else: b.tree_sample_push_flat(s.parent, s.child0, s.child1, s.t, s.root)
            t = b.mcc_derive(first=1, stride=2, seed=3)
            corr = [b.mcc_correspondence(k) for k in range(4)]
            probe = b.mcc_probe_ancestors(pop, [int(t.root), 0, 3], t_start, t_end, 16, ranks=[0, 3])
            results.append(b"".join([np.int32([t.master, t.master_index, t.root]).tobytes(), t.log_cc.tobytes(), t.parent.tobytes(), t.child0.tobytes(), t.child1.tobytes(), t.support.tobytes(),
                                     t.t.tobytes(), t.t_mrca.tobytes(), t.num_exact.tobytes()] + [c[0].tobytes() + c[1].tobytes() for c in corr] +
                                    [probe.p.tobytes(), probe.mean.tobytes(), probe.order_stats.tobytes(), probe.cells_to_skip.tobytes()]))
            for k, s in enumerate(ss):
                got = b.tree_sample_get(k)
                assert all(np.array_equal(a, w) for a, w in zip(got[:4], (s.parent, s.child0, s.child1, s.t))) and got[4] == s.root
        assert results[0] == results[1]
    finally:
        b.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_text_and_the_next_call_works():
    tips = 4
    ss, special = SS.sample_set(900, tips, 3)
    n, L = ss[0].n, SS.NUM_SITES
    records = [int(s.mut_offset[s.n]) for s in ss]
    pop = d.PopModel.const(2.0)
    t_end = max(float(s.t.max()) for s in ss) + 1.0
    w = (min(float(s.t[s.root]) for s in ss) - 1.0, t_end, 10)
    b = _backend(tips, 5, 0)
    refused = 0
    try:
        # no mutation room yet
        for call, text in ((lambda: b.tree_samples_probe_site_states(pop, [0], *w, count=1), "emat_tree_samples_reserve_mutations first"),
                           (lambda: _push(b, ss[0]), "emat_tree_samples_reserve_mutations first"),
                           (lambda: b.tree_sample_get_mutations(0), "emat_tree_samples_reserve_mutations first")):
            b.tree_sample_push_flat(ss[0].parent, ss[0].child0, ss[0].child1, ss[0].t, ss[0].root)
            with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*" + text):
                call()
            assert b.tree_samples_count() == 1
            b.tree_samples_clear()
        b.tree_sample_push_flat(ss[0].parent, ss[0].child0, ss[0].child1, ss[0].t, ss[0].root)
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*holds 1 samples: emat_tree_samples_clear first"):
            b.tree_samples_reserve_mutations(100)
        b.tree_samples_clear()
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*must not be negative"):
            b.tree_samples_reserve_mutations(-1)
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*MB of list headers.*MB of reference sequences of %d sites.*records.*the device has .* MB free" % L):
            b.tree_samples_reserve_mutations(1 << 39)
        # an arena that holds the first two samples and not the third: nothing is pushed, the count is unchanged, and after clear it works
        b.tree_samples_reserve_mutations(records[0] + records[1] + records[2] - 1)
        assert b.tree_samples_mutation_info() == (0, sum(records) - 1, L)
        assert _push(b, ss[0]) == 0 and _push(b, ss[1]) == 1
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*this sample has %d mutation records and the arena has %d free of %d" % (records[2], records[2] - 1, sum(records) - 1)):
            _push(b, ss[2])
        assert b.tree_samples_count() == 2 and b.tree_samples_mutation_info()[0] == records[0] + records[1]
        b.tree_samples_clear()
        assert b.tree_samples_mutation_info() == (0, sum(records) - 1, L)
        assert _push(b, ss[2]) == 0
        b.tree_samples_clear(); b.tree_samples_reserve_mutations(0)
        assert b.tree_samples_mutation_info()[1] == 0
        b.tree_samples_reserve_mutations(2 * sum(records) + 8)
        # what emat_tree_sample_push_flat_mutations checks of the lists
        s = ss[0]
        arg = lambda **kw: [kw.get(k, v) for k, v in zip(("parent", "child0", "child1", "t", "root", "off", "site", "frm", "to", "mt", "ref"), s.push_args())]
        bad_off = s.mut_offset.copy(); bad_off[2] = bad_off[1] - 1 if bad_off[1] > 0 else -1
        off1 = s.mut_offset.copy(); off1[0] = 1
        site_hi = s.mut_site.copy(); site_hi[0] = L
        to4 = s.mut_to.copy(); to4[0] = 4
        ref4 = s.ref.copy(); ref4[3] = 4
        for kw, text in (({"off": off1}, "mut_offset must start at 0"), ({"off": bad_off}, "mut_offset must not decrease: node 1"),
                         ({"site": site_hi}, "mutation 0: site %d is outside the valid range .0, %d." % (L, L)), ({"to": to4}, "mutation 0: states must be 0..3"),
                         ({"ref": ref4}, "reference sequence states must be 0..3, and site 3 has 4"), ({"root": n}, "root %d is outside the valid range" % n)):
            with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*" + text):
                b.tree_sample_push_flat_mutations(*arg(**kw))
            assert b.tree_samples_count() == 0 and b.tree_samples_mutation_info()[0] == 0
            refused += 1
        # samples 0 and 2 with mutations, 1 without
        assert _push(b, ss[0]) == 0
        assert b.tree_sample_push_flat(ss[1].parent, ss[1].child0, ss[1].child1, ss[1].t, ss[1].root) == 1
        assert _push(b, ss[2]) == 2
        sites = [special["root"], special["never"]]
        good = lambda: b.tree_samples_probe_site_states(pop, sites, *w, count=2, stride=2)
        first_good = good()
        assert first_good.p.shape == (2, 2, 4, 10)
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_mcc_derive first"):
            b.mcc_probe_site_states(pop, sites, *w)
        for call, status, text in (
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w), "STATE", "sample 1 .slot 1. was pushed without mutations"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, first=1, count=1), "STATE", "sample 0 .slot 1. was pushed without mutations"),
                (lambda: b.tree_sample_get_mutations(1), "STATE", "sample 1 was pushed without mutations"),
                (lambda: b.tree_sample_get_mutations(3), "INVALID_ARGUMENT", "sample 3 is outside the valid range .0, 3."),
                (lambda: b.tree_samples_probe_site_states(pop, [], *w, count=1), "INVALID_ARGUMENT", "num_sites must be positive"),
                (lambda: b.tree_samples_probe_site_states(pop, [0, L], *w, count=1), "INVALID_ARGUMENT", "entry 1: site %d is outside the valid range .0, %d." % (L, L)),
                (lambda: b.tree_samples_probe_site_states(pop, [-1], *w, count=1), "INVALID_ARGUMENT", "entry 0: site -1 is outside the valid range"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, count=0), "INVALID_ARGUMENT", "must be positive"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, count=1, stride=0), "INVALID_ARGUMENT", "stride must be positive"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, first=2, count=2), "INVALID_ARGUMENT", "outside the valid range .0, 3."),
                (lambda: b.tree_samples_probe_site_states([pop, pop, pop], sites, *w, count=2, stride=2), "INVALID_ARGUMENT", "one for all samples or one per chosen sample .2., not 3"),
                (lambda: b.tree_samples_probe_site_states([pop, d.PopModel.const(-1.0)], sites, *w, count=2, stride=2), "INVALID_ARGUMENT", "population model 1: Population size should be positive"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, 1.0, 1.0, 10, count=1), "INVALID_ARGUMENT", "need t_start < t_end"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, w[0], w[1], 0, count=1), "INVALID_ARGUMENT", "number of cells should be positive"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, count=2, stride=2, ranks=[0, 2]), "INVALID_ARGUMENT", "rank 2 is outside the valid range .0, 2."),
                (lambda: b.tree_samples_probe_site_states(pop, sites, *w, count=1, per_sample=False, mean=False), "INVALID_ARGUMENT", "nothing is asked for"),
                (lambda: b.tree_samples_probe_site_states(pop, sites, t_end, t_end + 1e-6, 1, count=1), "CAPACITY", "sample 0 .slot 0.*more than the prober holds")):
            with pytest.raises(d.EmatError, match="EMAT_ERR_" + status + ".*" + text):
                call()
            refused += 1
            assert good().p.tobytes() == first_good.p.tobytes()
        b.mcc_derive(first=0, stride=2)
        assert _same(b.mcc_probe_site_states(pop, sites, *w), first_good)
        b.mcc_derive()                                                                  # all three: the one without mutations among them
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*sample 1 .slot 1. was pushed without mutations"):
            b.mcc_probe_site_states(pop, sites, *w)
        # a sample whose inner node is later than its child: the pushes do not look at times
        late = ss[2]
        v = next(u for u in late.topology().inner_nodes() if u != late.root)
        t_late = late.t.copy(); t_late[v] = float(late.t[[late.child0[v], late.child1[v]]].max()) + 0.5
        args = list(late.push_args()); args[3] = t_late
        assert b.tree_sample_push_flat_mutations(*args) == 3
        with pytest.raises(d.EmatError, match="EMAT_ERR_INTERNAL.*sample 1 .slot 3. is earlier than its parent"):
            b.tree_samples_probe_site_states(pop, sites, *w, first=2, count=2)
        assert good().p.tobytes() == first_good.p.tobytes()                             # the other samples are unharmed
        # a reserve that re-binds the store drops the mutation room
        b.tree_samples_clear(); b.tree_samples_reserve(7)
        assert b.tree_samples_mutation_info()[1] == 0
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_reserve_mutations first"):
            _push(b, ss[0])
    finally:
        b.close()
    assert refused == 23
    # more samples than the sort holds: refused on the host's arithmetic
    s = SS.sample_set(901, 2, 1)[0][0]
    b = _backend(2, 4097, 4097 * int(s.mut_offset[s.n]))
    try:
        for _ in range(4097): _push(b, s)
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*order statistics over 4097 samples, and the sort holds 4096"):
            b.tree_samples_probe_site_states(pop, [0], -5.0, 4.0, 3, ranks=[0], per_sample=False)
        r = b.tree_samples_probe_site_states(pop, [0, 1], -5.0, 4.0, 3, ranks=[0, 4095], count=4096, per_sample=False)
        assert r.order_stats[0].tobytes() == r.order_stats[1].tobytes()                                            # 4 096 copies of one tree
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*4097 samples x 8 sites x 4 members x 1048576 cells need .* MB and the working room of one sample with all its sites .* MB; the device has .* MB free"):
            b.tree_samples_probe_site_states(pop, [0] * 8, -5.0, 4.0, 1 << 20, per_sample=False)                   # 4097 x 2^25 doubles
        assert b.tree_samples_probe_site_states(pop, [0], -5.0, 4.0, 3, count=2).p.shape == (2, 1, 4, 3)
    finally:
        b.close()
    h = d.EmatBackend(60, device=-1)
    try:
        for call in (lambda: h.tree_samples_probe_site_states(pop, [0], 0.0, 1.0, 2, count=1), lambda: h.mcc_probe_site_states(pop, [0], 0.0, 1.0, 2),
                     lambda: h.tree_samples_reserve_mutations(1), lambda: h.tree_samples_mutation_info()):
            with pytest.raises(d.EmatError, match="EMAT_ERR_NO_DEVICE"):
                call()
    finally:
        h.close()
