"""The chain's frame with scalar loop control: run_chain and the frame part of mcmc_sub_iteration (emat_device_moves.hpp) branch on values
said to be uniform where they are loaded or returned (emat_device_core.hpp: uniform_flag / uniform_u32).  No draw, counter, trace row or
slab byte may change, whichever way the loop is left and entered again.

  1. One pass of C1 under three launch shapes -- one ticket, four tickets, one move per launch -- in each of the ways a part can run:
     staged whole, staged by its prefix, resident in HBM, and in the side launch.  Every exit of the loop is walked: moves used up, the
     park for the next stretch of the random stream, both parks of an SPR1 move, and resumption in a later launch.
  2. The smallest parts the cutter makes (three nodes: a cut node and its two children), where every pick is over n = 3 and the topology
     moves and the branch reform return early most of the time.  Parts of one or two nodes do not exist: every part is a full binary
     subtree, and the displacement moves' pick loops rely on an inner node and a tip being there; uniform_int at
     n = 1 and 2 is held to the 128-bit product on the host (scripts/micro/draw_arith_host.cpp).
  3. The two stops: the root part outgrowing its grid (k_part_need_cells: the move undone, the stream rewound, the pass resumed), and a
     part without heap slack (make_heap_room -> k_part_need_space).  Same traces as the oracle, and moves_done / proposed exact.
  4. The site-rate kernels draw through the conversions the moves use (emat_gamma_pure.hpp): the smallest cases of
     test_site_rate_moves_gpu.py against tests/site_rate_model.py, and gamma draws, whose uniforms go through to_oo, against the streams
     restated in numpy -- the guard of any shorter spelling of the conversions (one was tried with this frame and not kept).
The oracle runs once per scenario (module cache)."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import delphy_amd as d
import delphy_amd.engine as e
from delphy_amd.scenarios import KAPPA, PI, Scenario, make_scenario
from helpers import assert_traces_match, assert_trees_match, compare_part, configure, split_parts
from oracle_ffi import OracleEngine

pytestmark = pytest.mark.gpu

TREE_FIELDS = ("parent", "child0", "child1", "t", "t_min", "t_max", "mut_offset", "mut_site", "mut_from", "mut_to", "mut_t", "miss_offset", "miss_start", "miss_end",
               "mfs_offset", "mfs_site", "mfs_state")
COUNTERS = ("moves_done", "rng_draws", "proposed", "accepted")


def _variant_counts(b):
    lib = d.load_library()
    lib.emat_debug_variant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)()
    assert lib.emat_debug_variant_counts(b.handle, out) == 0
    return list(out)   # parts staged whole, by prefix, not at all


def _digest(tree, stats, rng):
    """Everything a part's chain leaves in its slab that the host can read back, as one hash."""
    h = hashlib.sha256()
    h.update(np.int64(tree.root).tobytes())
    for f in TREE_FIELDS:
        h.update(np.ascontiguousarray(getattr(tree, f)).tobytes())
    h.update(repr([stats[k] for k in COUNTERS]).encode())
    h.update(repr((rng["key"], rng["counter"], rng["has_spare"], rng["spare"] if rng["has_spare"] else 0)).encode())
    return h.hexdigest()


# ---- 1. one pass, three launch shapes, four ways to run a part -------------------------------------------------------------
C1_PARTS, C1_MOVES, C1_SEED = 4, 300, 11


@functools.lru_cache(maxsize=None)
def _c1():
    sc = make_scenario("C1", num_tips=100, num_sites=30000, uncertain_tips=0.2)
    return sc, split_parts(sc, C1_PARTS, C1_SEED)


@functools.lru_cache(maxsize=None)
def _c1_oracle():
    sc, (parts, incl, seeds, root_part, ref) = _c1()
    orc = OracleEngine(sc.num_sites, trace_moves=C1_MOVES)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part)
        orc.run_moves_per_part(C1_MOVES, threads=4)
        out = [dict(trace=orc.part_trace(p, C1_MOVES).copy(), stats=orc.part_stats(p), tree=orc.part_download(p)) for p in range(len(parts))]
        assert all(o["stats"]["status"] == 0 and o["trace"].shape == (C1_MOVES, 4) for o in out)
        kinds = np.concatenate([o["trace"][:, 0] for o in out])
        assert all(np.count_nonzero(kinds == k) > 0 for k in range(5)), "the pass does not hold every kind of move"
        return out
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def _c1_pass(shape, use_lds=True, lds_max=None):
    """shape: 'one' ticket, 'four' tickets, 'stepped' (one move per launch).  Per part (trace, stats, tree, rng, digest), the variant
    counts and the main-launch mask."""
    sc, (parts, incl, seeds, root_part, ref) = _c1()
    b = d.EmatBackend(sc.num_sites, trace_moves=C1_MOVES, use_lds=use_lds)
    try:
        if lds_max is not None:
            b.set_option("lds_max", lds_max)
        if shape != "stepped":
            b.set_option("chunks", {"one": 1, "four": 4}[shape])
        configure(b, sc, ref, parts, incl, seeds, root_part)
        counts = _variant_counts(b)
        if shape == "stepped":
            for _ in range(C1_MOVES):
                b.run_moves_per_part(1); b.synchronize()
        else:
            b.run_moves_per_part(C1_MOVES); b.synchronize()
        out = []
        for p in range(len(parts)):
            st = b.part_stats(p)
            assert st["status"] == 0 and st["moves_done"] == C1_MOVES, "part %d: %s: %s" % (p, st, b.last_error())
            tree, rng = b.part_download(p), b.part_rng(p)
            out.append(dict(trace=b.part_trace(p, C1_MOVES).copy(), stats=st, tree=tree, rng=rng, digest=_digest(tree, st, rng)))
        return out, counts, b.main_class_mask(len(parts))
    finally:
        b.close()


def _assert_the_oracles_pass(dev, what):
    for p, (g, o) in enumerate(zip(dev, _c1_oracle())):
        assert_traces_match(g["trace"], o["trace"], 1e-9, "%s, part %d" % (what, p))
        for k in COUNTERS:
            assert g["stats"][k] == o["stats"][k], "%s, part %d: %s %s, the oracle's %s" % (what, p, k, g["stats"][k], o["stats"][k])
        assert_trees_match(g["tree"], o["tree"], 1e-9, "%s, part %d" % (what, p))


def _assert_identical(a, b, what):
    for p, (x, y) in enumerate(zip(a, b)):
        assert x["trace"].tobytes() == y["trace"].tobytes(), "%s: part %d: traces differ" % (what, p)
        assert x["stats"]["rng_draws"] == y["stats"]["rng_draws"], "%s: part %d: rng_draws %d vs %d" % (what, p, x["stats"]["rng_draws"], y["stats"]["rng_draws"])
        assert x["digest"] == y["digest"], "%s: part %d: part digests differ (%s vs %s)" % (what, p, x["stats"], y["stats"])


def _prefix_cap():
    """The largest staging cap, of those tried, under which the kernel's own decision puts a part in the prefix variant."""
    sc, (parts, incl, seeds, root_part, ref) = _c1()
    for cap in (32768, 16384, 12288, 10240, 8192, 6144, 4096, 2048, 512):
        b = d.EmatBackend(sc.num_sites, trace_moves=C1_MOVES)      # (the trace is part of the slab: the same handle as the passes')
        try:
            b.set_option("lds_max", cap)
            configure(b, sc, ref, parts, incl, seeds, root_part)
            if _variant_counts(b)[1] > 0:
                return cap
        finally:
            b.close()
    pytest.fail("no staging cap tried puts a part in the prefix variant")


@pytest.mark.parametrize("mode", ["whole", "prefix", "no_lds", "side"])
def test_c1_is_the_same_chain_under_every_launch_shape(mode):
    """One ticket, four tickets and one move per launch: identical traces, rng_draws and part digests, and the oracle's pass move for move."""
    kw = {}
    if mode == "prefix":
        kw = dict(lds_max=_prefix_cap())
    elif mode == "no_lds":
        kw = dict(use_lds=False)
    one, counts, main = _c1_pass("one", **kw)
    print("%s: variants (whole, prefix, HBM) %s, main-launch mask %s" % (mode, counts, list(main)))
    if mode == "whole":
        assert counts[0] > 0, "no part was staged whole: %s" % counts
    elif mode == "prefix":
        assert counts[1] > 0
    elif mode == "no_lds":
        assert counts[2] == C1_PARTS, "staging off, but not every part is resident in HBM: %s" % counts
    else:
        assert not np.all(main), "no part ran in a side launch"
    _assert_the_oracles_pass(one, "%s, one ticket" % mode)
    for shape in ("four", "stepped"):
        other = _c1_pass(shape, **kw)[0]
        _assert_the_oracles_pass(other, "%s, %s" % (mode, shape))
        _assert_identical(one, other, "%s: %s against one ticket" % (mode, shape))


# ---- 2. the smallest parts ---------------------------------------------------------------------------------------------
TINY_MOVES = 200


def test_parts_of_three_nodes_are_the_oracles():
    """60 tips cut with at most three nodes asked per part: 19 parts, eight of them a cut node and its two children, the root part of five
    nodes.  In a three-node part every pick is over n = 3, and most topology moves and branch reforms return before they are noted."""
    sc = make_scenario("C1", num_tips=60, num_sites=500, uncertain_tips=0.2)
    parts, incl, seeds, root_part, ref = split_parts(sc, 4, 2, 3)
    small = [p for p in range(len(parts)) if parts[p].num_nodes == 3]
    assert len(small) >= 5 and min(t.num_nodes for t in parts) == 3, sorted(t.num_nodes for t in parts)
    for use_lds in (True, False):
        gpu = d.EmatBackend(sc.num_sites, trace_moves=TINY_MOVES, use_lds=use_lds); orc = OracleEngine(sc.num_sites, trace_moves=TINY_MOVES)
        try:
            configure(gpu, sc, ref, parts, incl, seeds, root_part)
            configure(orc, sc, ref, parts, incl, seeds, root_part)
            scales = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[2])), abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p in range(len(parts))]
            cells = [orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(len(parts))]
            gpu.run_moves_per_part(TINY_MOVES); gpu.synchronize(); orc.run_moves_per_part(TINY_MOVES, threads=4)
            early = 0
            for p in range(len(parts)):
                compare_part(gpu, orc, p, parts[p].num_nodes, TINY_MOVES, 1e-9, TINY_MOVES, scales[p], cells[p])
                if p in small:
                    early += int(np.isnan(gpu.part_trace(p, TINY_MOVES)[:, 3]).sum())
            assert early >= 100, "the three-node parts returned early from only %d moves" % early
        finally:
            gpu.close(); orc.close()


# ---- 3. the stops ------------------------------------------------------------------------------------------------------
def _stopped_pass(sc, parts, incl, seeds, root_part, ref, moves, t_step=None, options=()):
    """One pass on the device and in the oracle; everything compared, moves_done exact.  Returns (root grid cells, heap capacities) before
    and after, from the device."""
    gpu = d.EmatBackend(sc.num_sites, trace_moves=moves); orc = OracleEngine(sc.num_sites, trace_moves=moves)
    try:
        for k, v in options:
            gpu.set_option(k, v)
        configure(gpu, sc, ref, parts, incl, seeds, root_part, t_step)
        configure(orc, sc, ref, parts, incl, seeds, root_part, t_step)
        n = len(parts)
        scales = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[2])), abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p in range(n)]
        cells = [orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(n)]
        before = (gpu.part_coalescent(root_part)["k_bar_p"].shape[0], [gpu.debug_slab_layout(p)["heap_cap"] for p in range(n)])
        gpu.run_moves_per_part(moves); gpu.synchronize(); orc.run_moves_per_part(moves, threads=4)
        after = (gpu.part_coalescent(root_part)["k_bar_p"].shape[0], [gpu.debug_slab_layout(p)["heap_cap"] for p in range(n)])
        for p in range(n):
            compare_part(gpu, orc, p, parts[p].num_nodes, moves, 1e-9, moves, scales[p], cells[p])   # (moves_done, proposed, accepted, rng_draws: the oracle's)
        return before, after
    finally:
        gpu.close(); orc.close()


def test_a_pass_stopped_to_regrow_the_root_grid_is_the_oracles():
    """tests/test_miss_dl_memo_gpu.py's interrupted pass: the root part outgrows the cells its slab has room for, the move that wanted them
    is undone before it changed anything (neither proposed nor moves_done counts it), the grid is regrown and the move runs again."""
    par = e.SynthParams(num_tips=120, num_sites=60, tip_span=30.0, pop_n0=400.0, pop_growth=0.0, mu=2e-5, gaps_per_tip=1, mean_gap_len=4.0, seed=3)
    par.pi, par.kappa = PI, KAPPA
    tree, ref0, tmax = e.make_synthetic_emat(par)
    sc = Scenario("deep-root", tree, ref0, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, 400.0, 0.0, 0.0), 60)
    parts, incl, seeds, root_part, ref = split_parts(sc, 5, 7)
    (cells0, _), (cells1, _) = _stopped_pass(sc, parts, incl, seeds, root_part, ref, 4000, t_step=sc.default_t_step() * 0.25)
    assert cells1 > cells0 + max(512, cells0), "the root part's grid did not outgrow its slab (%d -> %d cells): the case no longer interrupts a pass" % (cells0, cells1)


def test_a_part_without_heap_slack_is_stopped_for_space_and_finishes_as_the_oracle():
    """No slack and no heap per node: the check before a move squeezes the heap, then stops the part with k_part_need_space; the host gives
    it room and the rest of its moves (the settings of tests/test_move_frame_gpu.py's case)."""
    sc = make_scenario("C1", num_tips=80, num_sites=400, seed=77)
    sc.mu = 3e-4
    tree, ref0, tmax = e.make_synthetic_emat(e.SynthParams(num_tips=80, num_sites=400, mu=3e-4, gaps_per_tip=3, mean_gap_len=25, seed=77))
    sc.tree, sc.ref, sc.t_max_tip = tree, ref0, tmax
    sc.pop = d.PopModel.exp(tmax, 365.0, 0.0, 0.0)
    parts, incl, seeds, root_part, ref = split_parts(sc, 4, 11)
    (_, cap0), (_, cap1) = _stopped_pass(sc, parts, incl, seeds, root_part, ref, 1500, options=(("slack", "1.0"), ("heap_per_node", "0")))
    print("heap capacity before %s after %s" % (cap0, cap1))
    assert any(b > a for a, b in zip(cap0, cap1)), "no part stopped for space: the case no longer interrupts a pass"


# ---- 4. the site-rate kernels' draws -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,alpha", [(1, 0.5), (63, 0.02)])
def test_site_rate_moves_against_the_model(L, alpha):
    import test_site_rate_moves_gpu as T
    t, m, nu_old = T._synthetic(L, 100 + L)
    b = T._handle(L, nu_old)
    try:
        res = b.site_rate_moves(t, m, alpha, 10, key=0xA11CE + L)
        nu_new = b.nu_l()
        assert len(res.trace) == 10
        T._check_call(res, alpha, [1e-3] * L, t, m, nu_old, nu_new, "L=%d alpha=%g" % (L, alpha))
    finally:
        b.close()


def test_gamma_draws_are_the_restated_streams():
    """Draw i of emat_debug_sample_gamma is stream (key, i).  A shape below 1 ends in u^(1 / shape) with u = to_oo of the stream's next
    word, and every round's squeeze test takes one: the draws restated with tests/skygrid_streams.py (the integer part exact, log / exp /
    cos the CPU's, hence 1e-9) would differ in their leading digits if to_oo gave another double."""
    import skygrid_streams as SS
    b = d.EmatBackend(4)
    try:
        for key, shape, rate in ((4242, 0.3, 1.0), (77, 0.5, 3.0), (5, 2.5, 0.25)):
            n = 64
            x = b.debug_sample_gamma(key, n, shape, rate)
            want = np.array([SS.gamma_draw(np.array([key], np.uint64), i, shape, rate)[0] for i in range(n)])
            assert np.allclose(x, want, rtol=1e-9, atol=0.0), (key, shape, np.max(np.abs(x / want - 1.0)))
    finally:
        b.close()
