"""The frame around every move (emat_device_moves.hpp: run_chain, mcmc_sub_iteration, begin_move, note_move, the heap mark a move may
start under, the root part's remembered stream position, the one byte count per move) against the oracle, on a 100-tip tree cut into five
parts of which one holds the run's root.

What the frame keeps per move is only looked at in a few places, and each test here looks through one of them:
  * the trace row, formed from the context's integers only where a row is stored: a trace that fills up in mid-pass, and the rows of moves
    that returned before they were noted (kind, node or -1, 0, NaN);
  * the three code variants (part staged whole, its prefix staged, all in HBM) and the side launch, which fill the context on their own;
  * the heap mark, fixed per leg: a pass whose parts run out of list heap, stop before a move and are given room;
  * the stream position of the move's first draw, kept by the root part alone: a pass interrupted to regrow the root part's grid.
The oracle runs once per scenario (module cache); every device run is compared with that."""
import ctypes as C
import functools

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from helpers import assert_traces_match, assert_trees_match, configure, split_parts
from oracle_ffi import OracleEngine

pytestmark = pytest.mark.gpu

NPARTS, MOVES, SEED, SHORT = 5, 200, 11, 37
TREE_FIELDS = ("parent", "child0", "child1", "t", "t_min", "t_max", "mut_offset", "mut_site", "mut_from", "mut_to", "mut_t", "miss_offset", "miss_start", "miss_end",
               "mfs_offset", "mfs_site", "mfs_state")


@functools.lru_cache(maxsize=None)
def _scenario():
    sc = make_scenario("C1", num_tips=100, num_sites=2000, uncertain_tips=0.2)
    return sc, split_parts(sc, NPARTS, SEED)


@functools.lru_cache(maxsize=None)
def _oracle():
    """The oracle's pass, traced in full: per part (trace, stats, tree, largest |partial prior| seen, cells before, cells after)."""
    sc, (parts, incl, seeds, root_part, ref) = _scenario()
    orc = OracleEngine(sc.num_sites, trace_moves=MOVES)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part)
        before = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[3])), orc.part_coalescent(p)["k_bar_p"].shape[0]) for p in range(len(parts))]
        orc.run_moves_per_part(MOVES, threads=4)
        out = []
        for p in range(len(parts)):
            scale = max(before[p][0], abs(float(orc.part_derived(p, parts[p].num_nodes)[3])))
            out.append(dict(trace=orc.part_trace(p, MOVES).copy(), stats=orc.part_stats(p), tree=orc.part_download(p), prior_scale=scale,
                            cells=(before[p][1], orc.part_coalescent(p)["k_bar_p"].shape[0])))
        return out
    finally:
        orc.close()


def _variant_counts(b):
    lib = d.load_library()
    lib.emat_debug_variant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)()
    assert lib.emat_debug_variant_counts(b.handle, out) == 0
    return list(out)   # parts staged whole, by prefix, not at all


def _device_pass(trace, options=(), use_lds=True, want_variant=None):
    """One pass of the scenario on the device.  Per part (trace, stats, tree), and how the parts ran: (variant counts, main-launch mask).
    None when `want_variant` is asked for and these options put no part in it."""
    sc, (parts, incl, seeds, root_part, ref) = _scenario()
    b = d.EmatBackend(sc.num_sites, trace_moves=trace, use_lds=use_lds)
    try:
        for k, v in options:
            b.set_option(k, v)
        configure(b, sc, ref, parts, incl, seeds, root_part)
        counts = _variant_counts(b)
        if want_variant is not None and counts[want_variant] == 0:
            return None
        b.run_moves_per_part(MOVES); b.synchronize()
        out = []
        for p in range(len(parts)):
            st = b.part_stats(p)
            assert st["status"] == 0, "part %d: device status %d: %s" % (p, st["status"], b.last_error())
            out.append(dict(trace=b.part_trace(p, trace).copy(), stats=st, tree=b.part_download(p)))
        return out, (counts, b.main_class_mask(len(parts)))
    finally:
        b.close()


def _assert_pass_is_the_oracles(dev, rows, what):
    """The first `rows` trace rows of every part, its counters, its random draws and its tree, against the oracle's pass; log MH ratios to
    run_parity's tolerance (1e-9 relative, with compare_part's floor for a part whose grid grew or whose prior is huge)."""
    orc = _oracle()
    for p, (g, o) in enumerate(zip(dev, orc)):
        floored = o["prior_scale"] > 1e6 or o["cells"][1] > o["cells"][0]
        assert g["trace"].shape[0] == rows, "%s: part %d holds %d trace rows, not %d" % (what, p, g["trace"].shape[0], rows)
        assert_traces_match(g["trace"], o["trace"][:rows], 1e-9, "%s, part %d" % (what, p), abs_floor=16 * np.finfo(np.float64).eps * o["prior_scale"] if floored else 0.0)
        for k in ("moves_done", "rng_draws", "proposed", "accepted"):
            assert g["stats"][k] == o["stats"][k], "%s, part %d: %s %s, the oracle's %s" % (what, p, k, g["stats"][k], o["stats"][k])
        assert g["stats"]["moves_done"] == MOVES
        assert_trees_match(g["tree"], o["tree"], 1e-9, "%s, part %d" % (what, p))


def _assert_same_chain(a, b, what, bytes_too=True):
    """Two device passes left the same bits behind: trees, counters, draws -- and, between passes that ran the parts the same way, the
    algorithmic byte counts."""
    for p, (x, y) in enumerate(zip(a, b)):
        assert x["tree"].root == y["tree"].root
        for f in TREE_FIELDS:
            assert np.array_equal(getattr(x["tree"], f), getattr(y["tree"], f), equal_nan=True), "%s: part %d: %s differs" % (what, p, f)
        for k in ("moves_done", "rng_draws", "proposed", "accepted") + (("algorithmic_bytes", "algorithmic_write_bytes") if bytes_too else ()):
            assert x["stats"][k] == y["stats"][k], "%s: part %d: %s %s vs %s" % (what, p, k, x["stats"][k], y["stats"][k])


@functools.lru_cache(maxsize=None)
def _default_passes():
    return {t: _device_pass(t) for t in (SHORT, MOVES, 0)}


def test_a_trace_that_fills_up_in_mid_pass_holds_the_first_rows_and_does_not_steer_the_chain():
    """37 rows of room, 200 moves per part, the full move mix: the 37 rows are the oracle's first 37, and trees, counters and draws after the
    200 moves are those of the same pass traced in full and not traced at all."""
    runs = _default_passes()
    (counts, _) = runs[SHORT][1]
    print("variants (whole, prefix, HBM):", counts)
    assert counts[0] > 0, "no part was staged whole: %s" % counts
    _assert_pass_is_the_oracles(runs[SHORT][0], SHORT, "37 rows")
    _assert_pass_is_the_oracles(runs[MOVES][0], MOVES, "200 rows")
    _assert_pass_is_the_oracles(runs[0][0], 0, "no trace")
    _assert_same_chain(runs[SHORT][0], runs[MOVES][0], "37 rows vs 200 rows")
    _assert_same_chain(runs[SHORT][0], runs[0][0], "37 rows vs no trace")


def _early(trace):
    return (trace[:, 2] == 0) & np.isnan(trace[:, 3])


def test_rows_of_moves_that_return_before_they_are_noted():
    """A move that returns early leaves (kind, the node it picked or -1, 0, NaN).  The oracle's pass has at least 20 such rows of at least
    three kinds (asserted from its trace); the device's are the same rows with the same kind and node."""
    orc = _oracle()
    per_kind = {}
    for o in orc:
        for k in o["trace"][_early(o["trace"]), 0]:
            per_kind[int(k)] = per_kind.get(int(k), 0) + 1
    print("early-return rows per move kind (oracle):", per_kind)
    assert sum(per_kind.values()) >= 20 and len(per_kind) >= 3, "the scenario no longer produces enough early returns: %s" % per_kind
    dev = _default_passes()[MOVES][0]
    got = {}
    for p, (g, o) in enumerate(zip(dev, orc)):
        eg, eo = _early(g["trace"]), _early(o["trace"])
        assert np.array_equal(eg, eo), "part %d: early-return rows at %s, the oracle's at %s" % (p, np.nonzero(eg)[0], np.nonzero(eo)[0])
        assert np.array_equal(g["trace"][eg, :2], o["trace"][eo, :2]), "part %d: (kind, node) of the early-return rows differ" % p
        for k in g["trace"][eg, 0]:
            got[int(k)] = got.get(int(k), 0) + 1
    assert got == per_kind


@pytest.mark.parametrize("variant", ["prefix", "hbm"])
def test_the_filling_trace_in_parts_staged_by_prefix_and_resident_in_hbm(variant):
    """The staging area capped until the kernel's own decision (mirrored by emat_debug_variant_counts) puts parts in the variant."""
    v = {"prefix": 1, "hbm": 2}[variant]
    for cap in (32768, 16384, 12288, 10240, 8192, 6144, 4096, 2048, 512):
        r = _device_pass(SHORT, options=(("lds_max", cap),), want_variant=v)
        if r is not None:
            print("lds_max %d: variants (whole, prefix, HBM) %s" % (cap, r[1][0]))
            _assert_pass_is_the_oracles(r[0], SHORT, "%s, lds_max %d" % (variant, cap))
            _assert_same_chain(r[0], _default_passes()[SHORT][0], "%s vs staged whole" % variant, bytes_too=False)
            return
    pytest.fail("no staging cap tried puts a part in the %s variant" % variant)


def test_the_filling_trace_with_staging_off_and_in_a_side_launch():
    """Staging off: every part in HBM.  And the default classes put the part that holds the run's root -- its grid has room for 512 more
    cells than it uses -- in a side launch (k_run_moves_side)."""
    off = _device_pass(SHORT, use_lds=False)
    _assert_pass_is_the_oracles(off[0], SHORT, "staging off")
    (counts, main) = _default_passes()[SHORT][1]
    print("main-launch mask:", main, "variants:", counts)
    assert not np.all(main), "no part ran in a side launch"


def test_parts_that_run_out_of_list_heap_stop_before_a_move_and_finish_with_more_room():
    """No slack and no heap per node: the lists a pass grows do not fit, the check before a move (heap mark above the leg's limit) squeezes
    the heap and then stops the part with k_part_need_space, finish_pass gives it twice the room and the rest of its moves.  That the pass
    was interrupted is read from the slabs: a part that stopped has a larger heap afterwards.  (Whether a part compacted its heap without
    stopping leaves no mark in the part statistics; the stop is reached through the compaction, which is what this case exercises.)"""
    import delphy_amd.engine as e
    sc = make_scenario("C1", num_tips=80, num_sites=400, seed=77)
    sc.mu = 3e-4
    tree, ref0, tmax = e.make_synthetic_emat(e.SynthParams(num_tips=80, num_sites=400, mu=3e-4, gaps_per_tip=3, mean_gap_len=25, seed=77))
    sc.tree, sc.ref, sc.t_max_tip = tree, ref0, tmax
    sc.pop = d.PopModel.exp(tmax, 365.0, 0.0, 0.0)
    moves, T = 1500, 1500
    parts, incl, seeds, root_part, ref = split_parts(sc, 4, 11)
    assert any(incl)
    gpu = d.EmatBackend(sc.num_sites, trace_moves=T); orc = OracleEngine(sc.num_sites, trace_moves=T)
    try:
        gpu.set_option("slack", "1.0"); gpu.set_option("heap_per_node", "0")
        configure(gpu, sc, ref, parts, incl, seeds, root_part)
        configure(orc, sc, ref, parts, incl, seeds, root_part)
        cap0 = [gpu.debug_slab_layout(p)["heap_cap"] for p in range(len(parts))]
        gpu.run_moves_per_part(moves); gpu.synchronize(); orc.run_moves_per_part(moves, threads=4)
        cap1 = [gpu.debug_slab_layout(p)["heap_cap"] for p in range(len(parts))]
        print("heap capacity before %s after %s" % (cap0, cap1))
        assert any(b > a for a, b in zip(cap0, cap1)), "no part stopped for space: the case no longer interrupts a pass"
        for p in range(len(parts)):
            sg, so = gpu.part_stats(p), orc.part_stats(p)
            assert sg["status"] == 0, gpu.last_error()
            assert_traces_match(gpu.part_trace(p, T), orc.part_trace(p, T), 1e-9, "part %d" % p)
            for k in ("moves_done", "rng_draws", "proposed", "accepted"):
                assert sg[k] == so[k], "part %d: %s %s, the oracle's %s" % (p, k, sg[k], so[k])
            assert sg["moves_done"] == moves
            assert_trees_match(gpu.part_download(p), orc.part_download(p), 1e-9, "part %d" % p)
    finally:
        gpu.close(); orc.close()


def test_the_root_part_resumes_from_the_same_stream_position_after_its_grid_is_regrown():
    """The root part outgrows its coalescent grid in mid-pass (stop_for_cells: the move undone, the stream rewound to the move's first
    draw), the parts are re-materialised and the move runs again -- the settings of
    test_parity_gpu.py::test_a_re_materialisation_in_mid_pass_keeps_what_the_moves_maintain.  Every part's trace is the oracle's across
    the interruption, and every part has consumed as many random numbers."""
    from helpers import random_scenario
    rng = np.random.default_rng(6202)
    for case in range(54):
        sc, nu_l, evo, what = random_scenario(rng, case)
        nparts = int(min(max(1, sc.tree.num_nodes // 24), rng.integers(1, 14)))
        split_seed = int(rng.integers(1, 10**6))
    parts, incl, seeds, root_part, ref = split_parts(sc, nparts, split_seed)
    T = 1600
    gpu = d.EmatBackend(sc.num_sites, trace_moves=T); orc = OracleEngine(sc.num_sites, trace_moves=T)
    try:
        configure(gpu, sc, ref, parts, incl, seeds, root_part, None, nu_l=nu_l, evo=evo)
        configure(orc, sc, ref, parts, incl, seeds, root_part, None, nu_l=nu_l, evo=evo)
        cells_before = len(gpu.part_coalescent(root_part)["k_bar_p"])
        scale = [abs(float(orc.part_derived(p, parts[p].num_nodes)[3])) for p in range(len(parts))]
        for _ in range(2):
            gpu.run_moves_per_part(800); gpu.synchronize(); orc.run_moves_per_part(800, threads=4)
            scale = [max(s, abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p, s in enumerate(scale)]
        assert len(gpu.part_coalescent(root_part)["k_bar_p"]) > cells_before + max(512, cells_before), "the root part's grid did not outgrow its slab: the case no longer interrupts a pass"
        for p in range(len(parts)):
            sg, so = gpu.part_stats(p), orc.part_stats(p)
            assert sg["status"] == 0, gpu.last_error()
            tg, to = gpu.part_trace(p, T), orc.part_trace(p, T)
            assert tg.shape == to.shape == (T, 4)
            # (the grid grew, and the population integrals of its new cells come from the device's exp on one side and glibc's on the
            # other: compare_part's floor, 16 units in the last place of the largest partial prior the part has held)
            assert_traces_match(tg, to, 1e-9, "part %d" % p, abs_floor=16 * np.finfo(np.float64).eps * scale[p])
            assert sg["rng_draws"] == so["rng_draws"], "part %d: %d draws, the oracle's %d" % (p, sg["rng_draws"], so["rng_draws"])
            assert sg["moves_done"] == so["moves_done"] == T and sg["proposed"] == so["proposed"] and sg["accepted"] == so["accepted"]
    finally:
        gpu.close(); orc.close()
