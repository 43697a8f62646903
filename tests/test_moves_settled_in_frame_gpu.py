"""Moves that end at once, settled in the chain's frame (settle_moves, emat_device_moves.hpp): in a part without the run's root the frame
draws the move and its node itself; a tip displacement of an exactly dated tip, a branch reform that picks the part's root and a branch
reform of a branch without mutations are finished there, in runs, with their counters held in registers until the run ends, and every
other tip displacement and reform is called with the node already picked.  No draw, counter, trace row or slab byte may change, wherever
a run is cut.

  1. C1-sized passes (100 tips, 4 parts, 300 traced moves -- several refills of the random words), with every tip exactly dated
     (_date_tips_exactly: each tip displacement ends at once, long runs) and with 30 % of the tips uncertain (settled and real tip
     displacements interleave: the picked-node entries run right after settled moves), as one ticket, four tickets and one move per launch, with the parts staged
     whole, by prefix, resident in HBM and with a part in the side launch: everything compare_part compares is the oracle's, move for
     move, and the three launch shapes leave identical traces, rng_draws and part digests.
  2. The same passes untraced (trace_cap = 0, the benchmark's setting): the registers' counts are then the only record.  Counters, stream
     position, trees and totals against the oracle, and the digests of the traced passes.
  3. The smallest parts (60 tips in 19 parts, eight of three nodes), 200 traced moves each: a reform there often picks the part's root.
  4. The interrupted passes of tests/test_chain_frame_gpu.py (the root grid regrown in mid-pass; parts stopped for heap space between
     two moves, where a run has to have stored what it held), through compare_part.
The oracle runs once per scenario (module cache)."""
import functools

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from helpers import assert_trees_match, compare_part, configure, rel_close, split_parts
from oracle_ffi import OracleEngine
from test_chain_frame_gpu import COUNTERS, _digest, _variant_counts
import test_chain_frame_gpu as CF

pytestmark = pytest.mark.gpu

PARTS, MOVES, SEED = 4, 300, 11
UNCERTAIN = (0.0, 0.3)
SHAPES = ("one", "four", "stepped")


def _date_tips_exactly(sc):
    """The synthetic generator keeps a tip's date, a double, inside [t_min, t_max], two floats: a tip it calls certain still has an interval
    of one float step, and its displacement is a real move.  Here every such tip gets a date a float holds and t_min == t_max == that date,
    as a tip of a data set with exact dates has; tips drawn uncertain keep their interval."""
    t = sc.tree
    tips = np.flatnonzero(t.child0 < 0)
    tips = tips[t.t_max[tips] - t.t_min[tips] < 1.0]
    t32 = t.t[tips].astype(np.float32)
    t.t[tips] = t32.astype(np.float64); t.t_min[tips] = t32; t.t_max[tips] = t32
    assert np.all(t.t[t.parent[tips]] < t.t[tips]) and np.all(t.mut_t[np.isfinite(t.mut_t)] <= sc.t_max_tip)
    for i in tips:   # (mutations of a tip's branch stay above it)
        assert np.all(t.mut_t[t.mut_offset[i]:t.mut_offset[i + 1]] <= t.t[i])
    return sc


@functools.lru_cache(maxsize=None)
def _c1(uncertain):
    sc = _date_tips_exactly(make_scenario("C1", num_tips=100, num_sites=30000, uncertain_tips=uncertain))
    return sc, split_parts(sc, PARTS, SEED)


_oracles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_oracles():
    yield
    for orc, _, _ in _oracles.values():
        orc.close()
    _oracles.clear()


def _oracle(uncertain):
    """The oracle after its pass (kept open: compare_part reads it), with the totals' scales and grid lengths from before the pass."""
    if uncertain not in _oracles:
        sc, (parts, incl, seeds, root_part, ref) = _c1(uncertain)
        orc = OracleEngine(sc.num_sites, trace_moves=MOVES)
        configure(orc, sc, ref, parts, incl, seeds, root_part)
        scales = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[2])), abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p in range(len(parts))]
        cells = [orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(len(parts))]
        orc.run_moves_per_part(MOVES, threads=4)
        _oracles[uncertain] = (orc, scales, cells)
        # what the scenario is for: settled moves of all three kinds, and tip displacements that are real moves only where tips are uncertain
        rows = np.concatenate([orc.part_trace(p, MOVES) for p in range(len(parts)) if p != root_part])
        tips_settled = np.count_nonzero((rows[:, 0] == 1) & np.isnan(rows[:, 3])); tips_real = np.count_nonzero((rows[:, 0] == 1) & ~np.isnan(rows[:, 3]))
        empty_reforms = np.count_nonzero((rows[:, 0] == 2) & (rows[:, 2] == 1) & (rows[:, 3] == 0.0))
        print("uncertain %.1f: of %d rows %d settled tip displacements, %d noted ones, %d reforms with log MH 0" % (uncertain, rows.shape[0], tips_settled, tips_real, empty_reforms))
        assert tips_settled > 100 and empty_reforms > 100
        assert (tips_real == 0) if uncertain == 0.0 else (tips_real > 20)
    return _oracles[uncertain]


@functools.lru_cache(maxsize=None)
def _prefix_cap(uncertain, traced):
    """The largest staging cap, of those tried, under which the kernel's own decision puts a part in the prefix variant (the trace is part
    of the slab: a handle like the pass's)."""
    sc, (parts, incl, seeds, root_part, ref) = _c1(uncertain)
    for cap in (32768, 16384, 12288, 10240, 8192, 6144, 4096, 2048, 512):
        b = d.EmatBackend(sc.num_sites, trace_moves=MOVES if traced else 0)
        try:
            b.set_option("lds_max", cap)
            configure(b, sc, ref, parts, incl, seeds, root_part)
            if _variant_counts(b)[1] > 0:
                return cap
        finally:
            b.close()
    pytest.fail("no staging cap tried puts a part in the prefix variant")


def _mode_kw(mode, uncertain, traced):
    if mode == "prefix":
        return dict(lds_max=_prefix_cap(uncertain, traced))
    if mode == "no_lds":
        return dict(use_lds=False)
    return {}


def _run(b, shape):
    if shape == "stepped":
        for _ in range(MOVES):
            b.run_moves_per_part(1); b.synchronize()
    else:
        b.run_moves_per_part(MOVES); b.synchronize()


def _pass(uncertain, mode, shape, traced):
    """One pass on the device, compared with the oracle's while the handle is open.  Per part (trace bytes, rng_draws, digest)."""
    sc, (parts, incl, seeds, root_part, ref) = _c1(uncertain)
    orc, scales, cells = _oracle(uncertain)
    kw = _mode_kw(mode, uncertain, traced)
    b = d.EmatBackend(sc.num_sites, trace_moves=MOVES if traced else 0, use_lds=kw.get("use_lds", True))
    try:
        if "lds_max" in kw:
            b.set_option("lds_max", kw["lds_max"])
        if shape != "stepped":
            b.set_option("chunks", {"one": 1, "four": 4}[shape])
        configure(b, sc, ref, parts, incl, seeds, root_part)
        counts, main = _variant_counts(b), b.main_class_mask(len(parts))
        if mode == "whole":
            assert counts[0] > 0, "no part was staged whole: %s" % counts
        elif mode == "prefix":
            assert counts[1] > 0
        elif mode == "no_lds":
            assert counts[2] == PARTS, "staging off, but not every part is resident in HBM: %s" % counts
        else:
            assert not np.all(main), "no part ran in a side launch"
        _run(b, shape)
        out = []
        for p in range(len(parts)):
            n = parts[p].num_nodes
            if traced:
                compare_part(b, orc, p, n, MOVES, 1e-9, MOVES, scales[p], cells[p])
            st, so = b.part_stats(p), orc.part_stats(p)
            assert st["status"] == 0, "part %d: %s: %s" % (p, st, b.last_error())
            for k in COUNTERS:   # (with no trace, the only record of what a run of settled moves held in registers)
                assert st[k] == so[k], "%s %s, part %d: %s %s, the oracle's %s" % (mode, shape, p, k, st[k], so[k])
            tree, rng = b.part_download(p), b.part_rng(p)
            assert_trees_match(tree, orc.part_download(p), 1e-9, "%s %s, part %d" % (mode, shape, p))
            (_, _, Gg, Ag), (_, _, Go, Ao) = b.part_derived(p, n), orc.part_derived(p, n)
            assert abs(Gg - Go) <= 1e-9 * max(1.0, abs(Go), scales[p][0]) and abs(Ag - Ao) <= 1e-9 * max(1.0, abs(Ao), scales[p][1]), "part %d totals: %r/%r %r/%r" % (p, Gg, Go, Ag, Ao)
            out.append(dict(trace=b.part_trace(p, MOVES).tobytes() if traced else b"", rng_draws=st["rng_draws"], digest=_digest(tree, st, rng)))
        return out
    finally:
        b.close()


def _assert_identical(a, b, what, traces=True):
    for p, (x, y) in enumerate(zip(a, b)):
        assert not traces or x["trace"] == y["trace"], "%s: part %d: traces differ" % (what, p)
        assert x["rng_draws"] == y["rng_draws"], "%s: part %d: rng_draws %d vs %d" % (what, p, x["rng_draws"], y["rng_draws"])
        assert x["digest"] == y["digest"], "%s: part %d: part digests differ" % (what, p)


@functools.lru_cache(maxsize=None)
def _traced_one_ticket(uncertain, mode):
    return _pass(uncertain, mode, "one", True)


@pytest.mark.parametrize("mode", ["whole", "prefix", "no_lds", "side"])
@pytest.mark.parametrize("uncertain", UNCERTAIN)
def test_traced_passes_are_the_oracles_under_every_launch_shape(uncertain, mode):
    """One ticket, four tickets, one move per launch: the oracle's pass move for move (compare_part), and identical to one another."""
    one = _traced_one_ticket(uncertain, mode)
    for shape in ("four", "stepped"):
        _assert_identical(one, _pass(uncertain, mode, shape, True), "%s: %s against one ticket" % (mode, shape))


@pytest.mark.parametrize("mode", ["whole", "prefix", "no_lds", "side"])
@pytest.mark.parametrize("uncertain", UNCERTAIN)
def test_untraced_passes_leave_the_same_parts(uncertain, mode):
    """trace_cap = 0: counters, stream position, trees and totals are the oracle's (asserted in _pass), and the part digests -- tree,
    counters, stream position -- are those of the traced pass."""
    one = _traced_one_ticket(uncertain, mode)
    for shape in SHAPES:
        _assert_identical(one, _pass(uncertain, mode, shape, False), "%s, untraced, %s against the traced ticket" % (mode, shape), traces=False)


# ---- 3. the smallest parts -----------------------------------------------------------------------------------------------
TINY_MOVES = 200


def test_parts_of_three_nodes_are_the_oracles():
    """60 tips, four in five dated exactly, cut with at most three nodes asked per part: 19 parts, eight of three nodes.  In a three-node
    part a reform picks the root one time in three, and most tip displacements end at once."""
    sc = _date_tips_exactly(make_scenario("C1", num_tips=60, num_sites=500, uncertain_tips=0.2))   # (the tree of tests/test_chain_frame_gpu.py's case)
    parts, incl, seeds, root_part, ref = split_parts(sc, 4, 2, 3)
    small = [p for p in range(len(parts)) if parts[p].num_nodes == 3 and p != root_part]
    assert len(small) >= 5 and min(t.num_nodes for t in parts) == 3, sorted(t.num_nodes for t in parts)
    for use_lds in (True, False):
        gpu = d.EmatBackend(sc.num_sites, trace_moves=TINY_MOVES, use_lds=use_lds); orc = OracleEngine(sc.num_sites, trace_moves=TINY_MOVES)
        try:
            configure(gpu, sc, ref, parts, incl, seeds, root_part)
            configure(orc, sc, ref, parts, incl, seeds, root_part)
            scales = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[2])), abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p in range(len(parts))]
            cells = [orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(len(parts))]
            gpu.run_moves_per_part(TINY_MOVES); gpu.synchronize(); orc.run_moves_per_part(TINY_MOVES, threads=4)
            root_picks = 0
            for p in range(len(parts)):
                compare_part(gpu, orc, p, parts[p].num_nodes, TINY_MOVES, 1e-9, TINY_MOVES, scales[p], cells[p])
                if p in small:
                    tr = gpu.part_trace(p, TINY_MOVES)
                    root_picks += int(np.count_nonzero((tr[:, 0] == 2) & (tr[:, 1] == parts[p].root) & np.isnan(tr[:, 3])))
            assert root_picks >= 50, "the reforms of the three-node parts picked the root only %d times" % root_picks
        finally:
            gpu.close(); orc.close()


# ---- 4. the stops --------------------------------------------------------------------------------------------------------
def test_interrupted_passes_are_the_oracles():
    """The two interrupted passes of tests/test_chain_frame_gpu.py, which compare every part through compare_part: the root part's grid
    regrown in mid-pass while the other parts run on, and parts stopped for heap space between two moves and finished later."""
    CF.test_a_pass_stopped_to_regrow_the_root_grid_is_the_oracles()
    CF.test_a_part_without_heap_slack_is_stopped_for_space_and_finishes_as_the_oracle()
