"""The host layer of the HBM-resident tree (delphy_amd/csrc/emat_gtree_host.hpp) across changes of path: every way into
emat_tree_repartition on ONE handle, a block of the parts on each of two handles, the emat_tree_* entry points that begin with the
resident tree's preconditions in every state, and the smallest tree there is.  The C-ABI is driven directly: the run driver picks one way in by the size
of the tree, and never changes the table path of a handle.  The checker of whole cycles is the host cycle of the same
draws (emat_run_* on a host-owned tree, as in test_device_tree_gpu.py)."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from test_device_tree_gpu import _partition_in_python, _same_tree

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_preconditions.json")
TIPS, SITES, PARTS, MOVES, CYCLES = 65, 60, 4, 20, 6
WAYS = [(made_here, host_tables) for host_tables in (0, 1) for made_here in (True, False)]   # (partition made by emat_tree_partition, tree_host_coalescent)


def _backend(sc, **options):
    b = d.EmatBackend(sc.num_sites)
    for k, v in options.items():
        b.set_option(k, v)
    b.set_ref_sequence(sc.ref); b.set_hky(sc.mu, sc.kappa, sc.pi); b.set_flags(sc.t_max_tip)
    return b


def _repartition(b, sc, partition, seeds, t_step, made_here, lo=0, hi=None):
    """emat_tree_repartition_range with the four arrays, or after emat_tree_partition with none; returns the status."""
    n, root_part, off, orig, k0, k1 = partition
    hi = n if hi is None else hi
    sd = np.ascontiguousarray(seeds, np.uint64); m = sc.pop.c_struct()
    I = C.POINTER(C.c_int32)
    arrays = [None] * 4 if made_here else [a.ctypes.data_as(I) for a in (off, orig, k0, k1)]
    return b._lib.emat_tree_repartition_range(b._h, n, *arrays, root_part, sd.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m), t_step, lo, hi)


def _set_table_path(b, host_tables):
    """`tree_host_coalescent` of a handle whose slabs are on the device: options are set before the first launch, and
    emat_begin_upload is what takes a handle back there (its parts are forgotten; the resident tree is not)."""
    b._ck(b._lib.emat_begin_upload(b._h, 1), "emat_begin_upload")
    b.set_option("tree_host_coalescent", host_tables)


def _host_cycle(rh, tree):
    """One repartition of the host cycle; its draws in the whole tree's numbering: cut nodes in the order of the parts, and
    the parts' seeds.  A part's root is its cut node, found by its time among the cut nodes of the draw."""
    rh.repartition()
    n, root_part = rh.num_parts()
    drawn = [int(v) for v in rh.debug_redraw_partition()]
    cuts, seeds = [], []
    for p in range(n):
        sub, incl, seed = rh.part(p)
        seeds.append(seed)
        if incl:
            cuts.append(int(tree.root)); assert p == root_part
            continue
        match = [v for v in drawn if tree.t[v] == sub.t[sub.root] and v != tree.root]
        assert len(match) == 1, (p, match, drawn)
        cuts.append(match[0])
    if cuts[-1] == tree.root:
        cuts = cuts[:-1]                  # (a part of its own at the end: partition_tree's rule when the stencil does not name the root)
    return cuts, seeds


def _walk(sc, parts, moves, cycles, ways, t_step, seed=31, **options):
    """`cycles` cycles on one resident-tree handle, cycle c entering the repartition by ways[c % len(ways)], each compared
    bit for bit with the host cycle of the same draws."""
    bh = d.EmatBackend(sc.num_sites)
    rh = d.EmatRun(bh, sc.tree, sc.ref, seed)
    rh.set_num_parts(parts); rh.set_hky(sc.mu, sc.kappa, sc.pi); rh.set_pop_model(sc.pop); rh.set_coalescent_t_step(t_step)
    bd = _backend(sc, **options)
    try:
        bd.tree_upload(sc.tree)
        tree = sc.tree
        host_tables = 0
        for cycle in range(cycles):
            made_here, want_tables = ways[cycle % len(ways)]
            what = "cycle %d (%s, tree_host_coalescent %d)" % (cycle, "emat_tree_partition" if made_here else "arrays handed in", want_tables)
            cuts, seeds = _host_cycle(rh, tree)
            if want_tables != host_tables:
                _set_table_path(bd, want_tables); host_tables = want_tables
            parent, c0, c1, t, root = bd.tree_topology()
            want = _partition_in_python(parent, c0, c1, root, cuts)
            assert want[0] == len(seeds), what
            if made_here:
                got = bd.tree_partition(cuts)
                assert got[:2] == want[:2] and all(np.array_equal(g, w) for g, w in zip(got[2:], want[2:])), what
            bd._ck(_repartition(bd, sc, want, seeds, t_step, made_here), what)
            rh.run_moves(want[0] * moves); bd.run_moves_per_part(moves); bd.synchronize()
            rh.reassemble(); bd.tree_reassemble()
            (th, refh), (tree, refd) = rh.tree(), bd.tree_download()
            _same_tree(th, tree, what)
            assert np.array_equal(refh, refd), what
    finally:
        rh.close(); bh.close(); bd.close()


@pytest.mark.parametrize("tight", [0, 1])
def test_every_way_into_the_repartition_in_turn_on_one_handle(tight):
    """Partition made by emat_tree_partition or handed in as arrays, tables built by kernels or by the host's builder: the
    four in turn over six cycles of one handle, so that each works on the flags and the buffers the one before it left; once
    with `tree_tight`, where the pools and the heaps start without room (whether one of them then has to grow depends on the
    tree and is not asserted here: the growth itself is test_pools_and_heaps_grow_when_they_run_out's)."""
    sc = make_scenario("C1", num_tips=TIPS, num_sites=SITES)
    _walk(sc, PARTS, MOVES, CYCLES, WAYS, sc.default_t_step(), tree_tight=tight)


def test_a_two_tip_tree_as_one_part_passes_every_stage():
    """The smallest tree there is, without a single list record, as one part, through both table paths and both ways in: empty
    heaps, one cell range."""
    sc = make_scenario("C1", num_tips=2, num_sites=SITES)
    n = sc.tree.num_nodes
    sc.tree = dataclasses.replace(sc.tree, miss_offset=np.zeros(n + 1, sc.tree.miss_offset.dtype), miss_start=sc.tree.miss_start[:0], miss_end=sc.tree.miss_end[:0])
    assert sc.tree.mut_offset[n] == 0 and sc.tree.mfs_offset[n] == 0
    _walk(sc, 1, 10, 4, WAYS, 0.5 * float(np.max(sc.tree.t) - np.min(sc.tree.t)))


def test_two_handles_each_with_a_block_of_the_parts():
    """Parts [0, 2) on one handle and [2, 4) on another, both on one device: root changes, gather, export, apply and the end
    of the reassemble through host buffers, over three cycles.  Both handles' trees equal the single handle's of the same cycle."""
    sc = make_scenario("C1", num_tips=TIPS, num_sites=SITES)
    t_step = sc.default_t_step()
    one, blocks = _backend(sc), [_backend(sc), _backend(sc)]
    rng = np.random.default_rng(5)
    try:
        for b in [one] + blocks:
            b.tree_upload(sc.tree)
        for cycle in range(3):
            parent, c0, c1, t, root = one.tree_topology()
            inner = np.flatnonzero(c0 >= 0)
            cuts = [int(v) for v in rng.choice(inner[inner != root], size=PARTS - 1, replace=False)]
            part = _partition_in_python(parent, c0, c1, root, cuts)
            seeds = rng.integers(1, 2**62, PARTS).astype(np.uint64)
            one._ck(_repartition(one, sc, part, seeds, t_step, False), "cycle %d" % cycle)
            one.run_moves_per_part(MOVES); one.synchronize()
            one.tree_reassemble()
            want, want_ref = one.tree_download()
            for k, b in enumerate(blocks):
                b._ck(_repartition(b, sc, part, seeds, t_step, False, 2 * k, 2 * k + 2), "cycle %d block %d" % (cycle, k))
                b.run_moves_per_part(MOVES); b.synchronize()
            deltas = [b.tree_root_deltas() for b in blocks]
            assert [x is not None for x in deltas] == [2 * k <= part[1] < 2 * k + 2 for k in range(2)]     # the block with the root part reads them
            site, frm, to = next(x for x in deltas if x is not None)
            for b in blocks:
                b.tree_gather_local(site, frm, to)
            sent = [b.tree_export_nodes() for b in blocks]
            blocks[0].tree_apply_nodes(sent[1]); blocks[1].tree_apply_nodes(sent[0])
            for k, b in enumerate(blocks):
                b.tree_reassemble_end()
                got, got_ref = b.tree_download()
                _same_tree(got, want, "cycle %d block %d" % (cycle, k))
                assert np.array_equal(got_ref, want_ref), (cycle, k)
    finally:
        for b in [one] + blocks:
            b.close()


# ---- the entry points in every state: status code and text -------------------------------------------------------------
STATES = ("no tree uploaded", "parts home", "parts out", "after a failed deferred gather")


class _Refused(Exception):
    pass


def _status(b, call):
    """The status of the first C call that a method of the Python wrapper makes and that fails, 0 if none does."""
    def ck(st, what):
        if st != 0:
            raise _Refused(st)
    b._ck = ck                                    # (on the instance, for this call only)
    try:
        call()
        return 0
    except _Refused as r:
        return r.args[0]
    finally:
        del b._ck


def _entries(b, sc, part, seeds):
    """name -> a call of the entry point with arguments that are valid in SOME state; returns the status.  The entry points of
    emat_gtree_host.hpp first, then the ones elsewhere that begin with the same preconditions (the probers, the sample store,
    the Skygrid moves), through the Python wrapper."""
    L, I, U8 = b._lib, C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    n = sc.tree.num_nodes
    i32 = lambda k=1: np.zeros(max(k, 1), np.int32)                     # noqa: E731
    u8 = lambda k=1: np.zeros(max(k, 1), np.uint8)                      # noqa: E731
    p = lambda a: a.ctypes.data_as(I if a.dtype == np.int32 else U8)    # noqa: E731
    out = d.FlatTree.empty(n, 4096, 4096, 4096); view = out.c_view()
    kids = I(); need = C.c_uint64()
    stale = np.zeros(32, np.uint8)                                      # (a header that is not an export's: read only after the state was accepted)
    cuts = np.ascontiguousarray(_cuts(sc), np.int32)
    t = np.asarray(sc.tree.t)
    win = (float(t.min()), float(t.max()) + 0.25, 8)
    curve = d.PopModel.skygrid(np.linspace(t.min() - 1.0, t.max(), 9), 4.0 + 0.5 * np.sin(np.arange(9.0)), True)
    return {
        "emat_tree_get_sizes": lambda: L.emat_tree_get_sizes(b._h, p(i32()), p(i32()), p(i32()), p(i32())),
        "emat_tree_download": lambda: (out, L.emat_tree_download(b._h, C.byref(view), p(u8(sc.num_sites))))[1],   # (`out` owns what `view` points to)
        "emat_tree_get_topology": lambda: L.emat_tree_get_topology(b._h, p(i32(n)), p(i32(n)), p(i32(n)), np.zeros(n).ctypes.data_as(C.POINTER(C.c_double)), p(i32())),
        "emat_tree_get_kids": lambda: L.emat_tree_get_kids(b._h, C.byref(kids), p(i32()), p(i32()), C.byref(C.c_double())),
        "emat_tree_partition": lambda: L.emat_tree_partition(b._h, cuts.shape[0], p(cuts), p(i32()), p(i32()), p(i32(PARTS))),
        "emat_tree_get_partition": lambda: L.emat_tree_get_partition(b._h, p(i32(PARTS + 1)), None, None, None),
        "emat_tree_repartition": lambda: _repartition(b, sc, part, seeds, sc.default_t_step(), False),
        "emat_tree_repartition (no arrays)": lambda: _repartition(b, sc, part, seeds, sc.default_t_step(), True),
        "emat_tree_reassemble": lambda: L.emat_tree_reassemble(b._h, p(i32()), p(i32(SITES)), p(u8(SITES)), p(u8(SITES)), SITES),
        "emat_tree_get_root_deltas": lambda: L.emat_tree_get_root_deltas(b._h, p(i32()), p(i32(SITES)), p(u8(SITES)), p(u8(SITES)), SITES),
        "emat_tree_gather_local": lambda: L.emat_tree_gather_local(b._h, 0, None, None, None),
        "emat_tree_export_nodes": lambda: L.emat_tree_export_nodes(b._h, None, 0, C.byref(need)),
        "emat_tree_apply_nodes": lambda: L.emat_tree_apply_nodes(b._h, p(stale), 32),
        "emat_tree_reassemble_end": lambda: L.emat_tree_reassemble_end(b._h),
        "emat_tree_probe_ancestors": lambda: _status(b, lambda: b.tree_probe_ancestors(sc.pop, [int(sc.tree.root)], *win)),
        "emat_tree_probe_site_states": lambda: _status(b, lambda: b.tree_probe_site_states(sc.pop, 0, *win)),
        "emat_tree_branch_counts": lambda: _status(b, lambda: b.tree_branch_counts(*win, marked_nodes=[int(sc.tree.root)])),
        "emat_tree_samples_reserve": lambda: _status(b, lambda: b.tree_samples_reserve(2)),
        "emat_tree_sample_push": lambda: _status(b, lambda: b.tree_sample_push()),
        "emat_tree_sample_push_flat": lambda: _status(b, lambda: b.tree_sample_push_flat(sc.tree.parent, sc.tree.child0, sc.tree.child1, sc.tree.t, int(sc.tree.root))),
        "emat_tree_samples_clear": lambda: _status(b, lambda: b.tree_samples_clear()),
        "emat_tree_coalescent_stats": lambda: _status(b, lambda: b.tree_coalescent_stats(win[1], 5.0)),
        "emat_tree_skygrid_moves": lambda: _status(b, lambda: b.tree_skygrid_moves(curve, d.SkygridSpec(), win[1], 5.0)),
    }


def _cuts(sc):
    inner = np.flatnonzero(sc.tree.child0 >= 0)
    return [int(v) for v in inner[inner != sc.tree.root][:: max(1, (len(inner) - 1) // (PARTS - 1))][:PARTS - 1]]


def record_preconditions():
    """{state: {entry point: [status, last_error or ""]}}: every entry point called in every state, the state made afresh for each call."""
    sc = make_scenario("C1", num_tips=TIPS, num_sites=SITES)
    part = _partition_in_python(sc.tree.parent, sc.tree.child0, sc.tree.child1, sc.tree.root, _cuts(sc))
    seeds = np.arange(1, PARTS + 1, dtype=np.uint64)
    table = {}
    for state in STATES:
        b = _backend(sc)
        try:
            names = list(_entries(b, sc, part, seeds))
            for name in names:
                if state != STATES[0]:
                    b.tree_upload(sc.tree)
                if state in STATES[2:]:
                    b._ck(_repartition(b, sc, part, seeds, sc.default_t_step(), False), state)
                if state == STATES[3]:
                    b.set_option("debug_fail_gather", 1)
                    b.tree_reassemble()                               # returns: no move was run, so the root did not change and the gather is deferred
                    first = b._lib.emat_tree_get_sizes(b._h, None, None, None, None)
                    table.setdefault(state, {})["(whoever touches the tree first)"] = [int(first), b.last_error()]
                st = int(_entries(b, sc, part, seeds)[name]())
                table.setdefault(state, {})[name] = [st, b.last_error() if st != 0 else ""]
        finally:
            b.close()
    return table


def test_every_entry_point_in_every_state_answers_as_recorded():
    """Status code and `last_error` of the emat_tree_* entry points listed in _entries where no tree was uploaded, where the parts are home, where they are
    out, and after a deferred gather failed (`debug_fail_gather`): the table recorded from the library before its preconditions got
    one owner each (tests/golden/make_tree_preconditions.py)."""
    want = json.load(open(GOLDEN))["table"]
    got = record_preconditions()
    assert sorted(got) == sorted(want)
    for state in want:
        assert sorted(got[state]) == sorted(want[state]), state
        for name in want[state]:
            assert got[state][name] == want[state][name], (state, name)
    wrong = sum(1 for s in want.values() for st, _ in s.values() if st != 0)
    assert wrong >= 60, "the table holds %d refusals: it no longer covers the wrong states" % wrong
