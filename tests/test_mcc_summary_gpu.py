"""emat_mcc_node_times and emat_mcc_mutation_support on the device against tests/mcc_summary_model.py, with the table emat_mcc_get_correspondence
serves: every comparison is np.array_equal -- each output is one of the store's doubles, an integer, or one sum in sample order divided once.

Every test needs the new exports and so fails on a library without them."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import delphy_amd as d
import mcc_model as M
import mcc_summary_model as S
import samples_site_states_model as SS
from delphy_amd import engine
from delphy_amd.scenarios import make_scenario
from test_mcc_model import GPU_SWEEP_SEED, four_tip_samples, sweep_case, tree_from_newick_like
from test_mcc_summary_model import HAND_MASS, HAND_QUANTILES, HAND_SITES, check_four_tip_mutations, check_four_tip_node_times, four_tip_mut_samples

pytestmark = pytest.mark.gpu

QUANTILES = (0.0, 0.025, 0.5, 0.975, 1.0)
MASSES = (0.95, 0.5, 1.0, 1e-9)


def _backend(num_tips, capacity, num_sites=60, records=0):
    sc = make_scenario("C1", num_tips=num_tips, num_sites=num_sites)
    b = d.EmatBackend(sc.num_sites)
    b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree)
    b.tree_samples_reserve(capacity)
    if records: b.tree_samples_reserve_mutations(records)
    return b


def _push(b, s):
    return b.tree_sample_push_flat(s.parent, s.child0, s.child1, s.t, s.root)


def _table(b, count):
    n = b.tree_samples_info()[2]
    corr = np.zeros((count, n), np.int64); exact = np.zeros((count, n), bool)
    for k in range(count): corr[k], exact[k] = b.mcc_correspondence(k)
    return corr, exact


def _same_node_times(r: d.MccNodeTimes, w: S.NodeTimes, what, per_sample=False):
    assert np.array_equal(r.num_exact, w.num_exact), what
    if w.q_mrca.shape[0]: assert np.array_equal(r.q_mrca, w.q_mrca) and np.array_equal(r.q_exact, w.q_exact), what
    if w.hpd_mrca is not None: assert np.array_equal(r.hpd_mrca, w.hpd_mrca) and np.array_equal(r.hpd_exact, w.hpd_exact), what
    if per_sample: assert np.array_equal(r.times, w.times) and np.array_equal(r.is_exact, w.is_exact), what


def _check_all(b, chosen, what, nodes=None, masses=MASSES, table=None):
    """Every quantile and every mass for `nodes` of the current derivation over `chosen`, against the model on the device's table."""
    corr, exact = table if table is not None else _table(b, len(chosen))
    for mass in masses:
        _same_node_times(b.mcc_node_times(nodes, QUANTILES, mass), S.node_times(chosen, corr, exact, nodes, QUANTILES, mass), (what, mass))
    return corr, exact


def _bytes(r: d.MccNodeTimes):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (r.num_exact, r.q_exact, r.q_mrca, r.hpd_exact, r.hpd_mrca, r.times, r.is_exact) if x is not None)


def _derive_bytes(r: d.MccTree):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (r.log_cc, r.parent, r.child0, r.child1, r.support, r.t, r.t_mrca, r.num_exact)) + bytes([r.master % 256, r.master_index % 256, r.root % 256])


def fixed_set(seed, num_tips, count, integer_times=False):
    """`count` samples of `num_tips` tips, perturbed from one another by SPRs and re-timings (mcc_model's moves), tips 0 .. num_tips - 1."""
    rng = random.Random(seed)
    cur = M.random_tree(rng, num_tips, list(range(num_tips)), list(range(num_tips, 2 * num_tips - 1)), integer_times)
    out = []
    for _ in range(count):
        if rng.random() < 0.5: M.random_spr(rng, cur, integer_times)
        for v in cur.post_order():
            if cur.is_tip(v):
                if rng.random() < 0.3: cur.t[v] = rng.randint(1, 3) if integer_times else rng.uniform(1.0, 3.0)    # tip-date moves: tips are nodes like any other
                continue
            lo = min(cur.t[cur.child0[v]], cur.t[cur.child1[v]])
            cur.t[v] = lo - (rng.randint(0, 2) if integer_times else rng.uniform(0.01, 1.0))
        out.append(cur.copy())
    return out


# ---- the cases worked by hand ---------------------------------------------------------------------------------------------------------
def test_the_hand_worked_four_tip_case_on_the_device():
    b = _backend(4, 8)
    try:
        ss = four_tip_samples()
        for s in ss: _push(b, s)
        assert b.mcc_derive(seed=7).master == 0
        r = b.mcc_node_times(None, HAND_QUANTILES, HAND_MASS, per_sample=True)
        check_four_tip_node_times(r)
        corr, exact = _table(b, 3)
        _same_node_times(r, S.node_times(ss, corr, exact, None, HAND_QUANTILES, HAND_MASS), "four tips", per_sample=True)
        assert r.nodes.tolist() == list(range(7)) and r.quantiles.tolist() == list(HAND_QUANTILES) and r.hpd_mass == HAND_MASS
    finally:
        b.close()
    b = _backend(4, 8, HAND_SITES, 64)
    try:
        ms = four_tip_mut_samples()
        for s in ms: b.tree_sample_push_flat_mutations(*s.push_args())
        assert b.mcc_derive(seed=7).master == 0
        r = b.mcc_mutation_support()
        check_four_tip_mutations(r)       # a branch with one site twice, a root list, a matching clade without the mutation, the mutation without the clade
        corr, exact = _table(b, 3)
        w = S.mutation_support(ms, corr, exact, 0)
        assert np.array_equal(r.num_with, w.num_with) and np.array_equal(r.mean_t, w.mean_t) and np.array_equal(r.t_min, w.t_min) and np.array_equal(r.t_max, w.t_max)
        # the master carrying one record twice: two records of the answer, both with the first one's time
        b.tree_samples_clear()
        for s in (ms[1], ms[0], ms[2]): b.tree_sample_push_flat_mutations(*s.push_args())
        assert b.mcc_derive(seed=1).master == 0
        r = b.mcc_mutation_support()
        assert list(r.num_with[:3]) == [3, 1, 3] and list(r.t_min[:3]) == [-0.75, -0.5, -0.75] and r.mean_t[0] == r.mean_t[2] == (-0.75 + -0.5 + -0.3) / 3
    finally:
        b.close()


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(6))
def test_the_first_sixty_cases_of_the_device_sweep(block):
    """sweep_case(GPU_SWEEP_SEED * 1000 + k, 400, 64), k < 60, ten to a test: all nodes, QUANTILES, every mass of MASSES.  A quarter have integer times."""
    b = _backend(2, 64)
    try:
        for case in range(10 * block, 10 * block + 10):
            ss = sweep_case(GPU_SWEEP_SEED * 1000 + case, 400, 64)
            sc = make_scenario("C1", num_tips=(ss[0].n + 1) // 2, num_sites=60)
            b.set_ref_sequence(sc.ref); b.tree_upload(sc.tree); b.tree_samples_clear()
            for s in ss: _push(b, s)
            b.mcc_derive(seed=case)
            _check_all(b, ss, "case %d (%d nodes, %d samples)" % (case, ss[0].n, len(ss)))
    finally:
        b.close()


# ---- sample counts at the sort's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 255, 256, 257, 513])
def test_sample_counts_at_the_edges_of_the_sort_on_five_tips(count):
    b = _backend(5, count)
    try:
        ss = fixed_set(900 + count, 5, count, integer_times=count % 2 == 1)
        for s in ss: _push(b, s)
        b.mcc_derive(seed=count)
        corr, exact = _check_all(b, ss, "%d samples" % count)
        r = b.mcc_node_times([8, 0, 5], QUANTILES, 0.95, per_sample=True)
        _same_node_times(r, S.node_times(ss, corr, exact, [8, 0, 5], QUANTILES, 0.95), "%d samples, picked" % count, per_sample=True)
    finally:
        b.close()


def test_as_many_samples_as_the_sort_holds_and_one_more_is_refused():
    b = _backend(2, 4097)
    try:
        rng = random.Random(4096)
        for k in range(4097):
            root_t = float(rng.randint(-40, -1)) if k % 3 == 0 else rng.uniform(-40.0, -1.0)
            _push(b, tree_from_newick_like((0, 1), {0: 0.0, 1: rng.choice((0.0, 0.25, 0.5)), 2: root_t}))
        ss = [M.Sample(*b.tree_sample_get(k)) for k in range(4096)]
        b.mcc_derive(count=4096)
        table = (np.tile(np.arange(3), (4096, 1)), np.ones((4096, 3), bool))     # two tips: every sample is the same clades
        assert all(np.array_equal(b.mcc_correspondence(k)[0], table[0][k]) and b.mcc_correspondence(k)[1].all() for k in (0, 1, 2047, 4095))
        _check_all(b, ss, "4096 samples", table=table)
        b.mcc_derive(count=4097)
        with pytest.raises(d.EmatError, match="EMAT_ERR_CAPACITY.*4097 samples, and the sort holds 4096"):
            b.mcc_node_times(None, QUANTILES, 0.95)
        b.mcc_derive(count=4096)
        assert b.mcc_node_times(None, (0.5,)).q_mrca.shape == (1, 3)
        # per-sample arrays of more than 2^26 values (16 385 entries x 4 096 samples) are refused on the host's arithmetic, before anything is written
        st, text = _raw_node_times(b, 16385, [0] * 16385, outputs=("times",))
        assert engine.STATUS_NAMES[st] == "EMAT_ERR_CAPACITY" and "16385 nodes x 4096 samples are more than 67108864 values" in text
        st, text = _raw_node_times(b, 16385, [0] * 16385, outputs=("num_exact",), out_count=16385)
        assert st == 0, text
        assert b.mcc_node_times([2, 0], (1.0,), per_sample=True).times.shape == (2, 4096)
    finally:
        b.close()


# ---- degenerate spreads ------------------------------------------------------------------------------------------------------------------
def test_identical_times_give_windows_of_width_zero_that_start_at_the_first_value():
    b = _backend(5, 40)
    try:
        base = fixed_set(31, 5, 1)[0]
        ss = [base.copy() for _ in range(40)]
        for s in ss: _push(b, s)
        b.mcc_derive()
        corr, exact = _table(b, 40)
        for mass in MASSES:
            r = b.mcc_node_times(None, QUANTILES, mass); w = S.node_times(ss, corr, exact, None, QUANTILES, mass)
            _same_node_times(r, w, mass)
            assert w.i_star_mrca == [0] * 9 and w.i_star_exact == [0] * 9
            assert np.array_equal(r.hpd_mrca[0], r.hpd_mrca[1]) and np.array_equal(r.hpd_mrca[0], base.t) and np.array_equal(r.hpd_exact, r.hpd_mrca)
            assert all(np.array_equal(row, base.t) for row in r.q_mrca) and list(r.num_exact) == [40] * 9
    finally:
        b.close()


# ---- derivations, node lists, per-sample arrays, chunks ----------------------------------------------------------------------------------
def test_a_strided_derivation_a_shuffled_node_list_the_per_sample_arrays_and_every_chunk_size():
    b = _backend(30, 64)
    try:
        ss = fixed_set(5, 30, 40); n = ss[0].n
        for s in ss: _push(b, s)
        b.mcc_derive(first=3, stride=2, seed=9)
        chosen = ss[3::2]
        corr, exact = _check_all(b, chosen, "first 3, stride 2")
        nodes = [n - 1, 0, 31, 31, 7, n - 1, 2]                                      # out of order, with repeats
        _check_all(b, chosen, "picked", nodes=nodes, table=(corr, exact))
        r = b.mcc_node_times([40, 3, 58], per_sample=True)                           # the per-sample arrays are the table's columns
        assert r.q_exact is None and r.hpd_mrca is None and r.times.shape == (3, len(chosen))
        for i, v in enumerate((40, 3, 58)):
            assert np.array_equal(r.times[i], [chosen[k].t[corr[k, v]] for k in range(len(chosen))]) and np.array_equal(r.is_exact[i], exact[:, v])
        assert np.array_equal(r.num_exact, exact[:, [40, 3, 58]].sum(axis=0))
        want = [_bytes(b.mcc_node_times(nd, QUANTILES, 0.95, per_sample=True)) for nd in (None, nodes)]
        for chunk in (1, 7, n):
            b.set_option("mcc_summary_chunk", chunk)
            assert [_bytes(b.mcc_node_times(nd, QUANTILES, 0.95, per_sample=True)) for nd in (None, nodes)] == want, chunk
        b.set_option("mcc_summary_chunk", 0)
        assert [_bytes(b.mcc_node_times(nd, QUANTILES, 0.95, per_sample=True)) for nd in (None, nodes)] == want      # and from call to call
    finally:
        b.close()


# ---- mutation support ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tips,count", [(2, 1), (5, 3), (40, 33)])
def test_mutation_support_on_generated_sample_sets(tips, count):
    ss, _ = SS.sample_set(100 + tips, tips, count)
    b = _backend(tips, count, SS.NUM_SITES, sum(int(s.mut_offset[s.n]) for s in ss) + 1)
    try:
        for s in ss: b.tree_sample_push_flat_mutations(*s.push_args())
        r0 = b.mcc_derive(seed=tips)
        corr, exact = _table(b, count)
        w = S.mutation_support(ss, corr, exact, r0.master)
        r = b.mcc_mutation_support()
        assert len(w.records) == int(ss[r0.master].mut_offset[ss[r0.master].n]) == r.num_with.shape[0]
        assert np.array_equal(r.num_with, w.num_with) and np.array_equal(r.mean_t, w.mean_t) and np.array_equal(r.t_min, w.t_min) and np.array_equal(r.t_max, w.t_max)
        assert (r.num_with >= 1).all() and (count == 1 or (r.num_with < count).any() or tips == 2)
        assert _derive_bytes(b.mcc_derive(seed=tips)) == _derive_bytes(r0)
    finally:
        b.close()


# ---- a whole run ------------------------------------------------------------------------------------------------------------------------------
def test_six_cycles_of_a_run_pushed_with_their_mutations_and_both_calls_on_their_mcc_tree():
    sc = make_scenario("C1", num_tips=150, num_sites=2000)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    run.set_num_parts(4); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    try:
        for cycle in range(6):
            run.repartition()
            if cycle == 0:
                b.tree_samples_reserve(6); b.tree_samples_reserve_mutations(6 * (4 * int(sc.tree.mut_offset[sc.tree.num_nodes]) + 256))
            run.run_moves(4 * 300); b.synchronize()
            run.reassemble()
            assert b.tree_sample_push() == cycle
        before = b.mcc_derive(seed=2)
        kept = []
        for k in range(6):
            off, site, frm, to, t, ref = b.tree_sample_get_mutations(k)
            kept.append(SS.MutSample(M.Sample(*b.tree_sample_get(k)), off, site, frm, to, t, ref))
        corr, exact = _check_all(b, kept, "six cycles")
        w = S.mutation_support(kept, corr, exact, before.master)
        r = b.mcc_mutation_support()
        assert len(w.records) > 0 and np.array_equal(r.num_with, w.num_with) and np.array_equal(r.mean_t, w.mean_t) and np.array_equal(r.t_min, w.t_min) and np.array_equal(r.t_max, w.t_max)
        print("six cycles: %d mutations on the master, %d of them in fewer than all six samples" % (len(w.records), int((r.num_with < 6).sum())))
        assert _derive_bytes(b.mcc_derive(seed=2)) == _derive_bytes(before)          # the derivation's own outputs, before and after the new calls
        run.repartition()                                                            # the parts are out: both calls touch only the store
        assert np.array_equal(b.mcc_mutation_support().mean_t, r.mean_t)
        _check_all(b, kept, "parts out", masses=(0.95,), table=(corr, exact))
        run.run_moves(4 * 10); b.synchronize(); run.reassemble()
    finally:
        run.close(); b.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def _raw_node_times(b, num_nodes, nodes, quantiles=None, num_quantiles=0, hpd_mass=0.0, outputs=(), out_count=1 << 12):
    """The call with exactly the arguments given; `outputs`: which of the result's arrays are not NULL (each of `out_count` elements)."""
    keep = []
    def arr(ct):
        a = (ct * out_count)(); keep.append(a); return a
    res = engine._MccNodeTimesResultC()
    res.num_quantiles = num_quantiles; res.hpd_mass = hpd_mass
    if quantiles is not None: res.quantiles = (C.c_double * max(len(quantiles), 1))(*quantiles)
    for name in outputs:
        ct = {"num_exact": C.c_int32, "is_exact": C.c_uint8}.get(name, C.c_double)
        setattr(res, name, arr(ct))
    nd = None if nodes is None else (C.c_int32 * max(len(nodes), 1))(*nodes)
    return b._lib.emat_mcc_node_times(b._h, num_nodes, nd, C.byref(res)), b.last_error()


def test_every_refusal_and_the_next_call_works():
    INVALID = 1
    b = _backend(5, 8, SS.NUM_SITES)
    try:
        ss = fixed_set(77, 5, 4)
        works = lambda: _check_all(b, ss, "after a refusal", masses=(0.95,))
        # no valid derivation: none yet, cleared since (a derivation that fails on the device leaves the same state, derived_M = 0, and cannot be provoked from here)
        for s in ss: _push(b, s)
        for call in (lambda: b.mcc_node_times(None, QUANTILES, 0.95), lambda: b.mcc_mutation_support()):
            with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_mcc_derive first"):
                call()
        b.mcc_derive(); works()
        b.tree_samples_clear()
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_mcc_derive first"):
            b.mcc_node_times(None, QUANTILES, 0.95)
        for s in ss: _push(b, s)
        b.mcc_derive(); works()
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT"):          # a derive refused for its arguments leaves the one before it in place
            b.mcc_derive(first=2, count=9)
        works()
        # arguments
        n = ss[0].n
        for kw, text in ((dict(num_nodes=0, nodes=[0], outputs=("num_exact",)), "num_nodes must be positive"),
                         (dict(num_nodes=-3, nodes=[0], outputs=("num_exact",)), "num_nodes must be positive"),
                         (dict(num_nodes=3, nodes=[0, n, 1], outputs=("num_exact",)), "entry 1: node %d is outside the valid range \\[0, %d\\)" % (n, n)),
                         (dict(num_nodes=2, nodes=[0, -1], outputs=("num_exact",)), "entry 1: node -1 is outside"),
                         (dict(num_nodes=0, nodes=None, quantiles=[0.5, 1.5], num_quantiles=2, outputs=("q_mrca",)), "quantile 1 is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, quantiles=[-0.1], num_quantiles=1, outputs=("q_mrca",)), "quantile 0 is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, quantiles=[float("nan")], num_quantiles=1, outputs=("q_exact",)), "quantile 0 is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, hpd_mass=1.5, outputs=("hpd_mrca",)), "hpd_mass is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, hpd_mass=-0.5, outputs=("hpd_mrca",)), "hpd_mass is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, hpd_mass=float("nan"), outputs=("hpd_exact",)), "hpd_mass is .*outside \\[0, 1\\]"),
                         (dict(num_nodes=0, nodes=None, num_quantiles=2, outputs=("q_mrca",)), "with num_quantiles > 0 quantiles must be given"),
                         (dict(num_nodes=0, nodes=None, num_quantiles=-1, outputs=("num_exact",)), "num_quantiles must not be negative"),
                         (dict(num_nodes=0, nodes=None, quantiles=[0.5], num_quantiles=1, hpd_mass=0.9), "nothing is asked for"),
                         (dict(num_nodes=0, nodes=None, outputs=("q_exact",)), "q_exact / q_mrca are asked for without quantiles"),
                         (dict(num_nodes=0, nodes=None, quantiles=[0.5], num_quantiles=1, outputs=("q_mrca", "hpd_exact")), "hpd_exact / hpd_mrca are asked for without hpd_mass")):
            st, text_got = _raw_node_times(b, **kw)
            assert st == INVALID, (kw, st, text_got)
            assert re.search("emat_mcc_node_times: .*" + text, text_got), (kw, text_got)
            works()
        with pytest.raises(d.EmatError, match="EMAT_ERR_INVALID_ARGUMENT.*num_nodes must be positive"):
            b.mcc_node_times([], QUANTILES)
        assert b.mcc_node_times([2, 2], (1.0,)).q_mrca.shape == (1, 2)                # a node given twice is answered twice
        # a time that is not finite in a chosen sample: +inf is the sort's padding
        b.tree_samples_clear()
        for k, s in enumerate(ss):
            x = s.copy()
            if k == 2: x.t[x.root] = -np.inf
            _push(b, x)
        b.mcc_derive()
        with pytest.raises(d.EmatError, match="EMAT_ERR_INTERNAL.*sample 2 \\(slot 2\\) holds a node time that is not finite"):
            b.mcc_node_times(None, QUANTILES, 0.95)
        b.mcc_derive(count=2); _check_all(b, ss[:2], "without the sample that is not finite", masses=(0.5,))
        # mutation support: a store without mutation room, a sample pushed without mutations, too little room
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*emat_tree_samples_reserve_mutations first"):
            b.mcc_mutation_support()
        ms, _ = SS.sample_set(3, 5, 3)
        b.tree_samples_clear(); b.tree_samples_reserve_mutations(sum(int(s.mut_offset[s.n]) for s in ms) + 1)
        b.tree_sample_push_flat_mutations(*ms[0].push_args()); _push(b, ms[1].topology()); b.tree_sample_push_flat_mutations(*ms[2].push_args())
        b.mcc_derive()
        with pytest.raises(d.EmatError, match="EMAT_ERR_STATE.*sample 1 \\(slot 1\\) was pushed without mutations"):
            b.mcc_mutation_support()
        master = b.mcc_derive(first=0, count=2, stride=2).master                     # samples 0 and 2: both with mutations
        records = int(ms[2 * master].mut_offset[ms[0].n])
        nm = C.c_int64(-1); few = np.zeros(max(records, 1), np.int32)
        st = b._lib.emat_mcc_mutation_support(b._h, records - 1, C.byref(nm), few.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None)
        assert records > 1 and engine.STATUS_NAMES[st] == "EMAT_ERR_CAPACITY" and nm.value == records and "room for %d" % (records - 1) in b.last_error()
        corr, exact = _table(b, 2)
        w = S.mutation_support([ms[0], ms[2]], corr, exact, master)
        r = b.mcc_mutation_support()
        assert np.array_equal(r.num_with, w.num_with) and np.array_equal(r.mean_t, w.mean_t) and np.array_equal(r.t_min, w.t_min) and np.array_equal(r.t_max, w.t_max)
    finally:
        b.close()
