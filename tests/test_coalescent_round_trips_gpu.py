"""The coalescent delta of a displaced coalescence or tip, with its scalar loads in batches (emat_device_core.hpp): the Skygrid ratio
takes the model table's head as one load and, for both times at once, the two knots and two gammas around a GUESSED knot interval; the
guess stands when the two knots bracket the time, and goes through the old loops when they do not.  The table rows of an interval's two
end cells are asked for together.  No draw, counter, trace row or slab byte may change, so every case is the oracle's pass move for
move (compare_part), with the parts staged whole, staged by prefix and resident in HBM.

  1. Skygrid, 100 tips, 4 parts, 300 traced moves: 2, 3 and 50 knots, staircase and log-linear, knots evenly spaced and unevenly -- bunched
     at the early end of twice the tree's span ("up": the guess falls short and the second loop steps up) and at the late end ("down": the
     first loop steps down).  For the uneven grids the guess is wrong for at least half of the times of the displaced inner nodes, counted
     on the CPU from the nodes the traces name and their times before and after the pass.  (Two knots are always evenly spaced.)
  2. Edge times, 2 parts: inner nodes and tips moved exactly onto cell bounds, knots laid exactly on node and tip times, the first knot
     later than the earliest nodes and the last knot earlier than the latest tips.
  3. Parts whose window is a single cell (a part's window reaches from its earliest node to the latest tip of the run: a grid step as long
     as the tree puts every part but the root's in one cell; both end cells are then the same cell).
  4. Long branches: two parts under a fine grid, displacements that cross ten cells and more (the middle cells' loop).
  5. The exponential and the constant model through the same passes, and one move per launch.
Tolerances are compare_part's (1e-9 relative on log MH ratios, totals and times; integers exact).  The oracle runs once per case."""
import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from helpers import compare_part, configure, split_parts
from oracle_ffi import OracleEngine
from test_chain_frame_gpu import _variant_counts

pytestmark = pytest.mark.gpu

MOVES, SEED = 300, 11
MODES = ("whole", "prefix", "no_lds")
K_INNER = 0   # trace row kind of an inner-node displacement


def _base(num_tips=100, uncertain=0.3):
    return make_scenario("C1", num_tips=num_tips, num_sites=2000, uncertain_tips=uncertain)


def _span(sc):
    t_root = float(sc.tree.t[sc.tree.root])
    return t_root, sc.t_max_tip - t_root


def _knots(sc, n, layout):
    """`n` knots from a little before the root: over the tree's span ("even"), or over twice the span and bunched at one end."""
    t_root, span = _span(sc)
    lo = t_root - 0.05 * span
    u = np.linspace(0.0, 1.0, n)
    if layout == "even":
        return lo + (sc.t_max_tip - lo) * u
    width = 2.0 * (sc.t_max_tip - lo)
    if layout == "up":       # all but the last knot among the early times: lower_bound lies above the guess
        return lo + width * u ** 4
    hi = sc.t_max_tip + 0.05 * span   # "down": all but the first knot among the late times, the grid ending just after the tips
    return hi - width * (1.0 - u) ** 4


def _gamma(n, n0=365.0):
    return np.array([np.log(n0) + 0.4 * np.sin(0.37 * k) + 0.05 * k / n for k in range(n)])


def _guess_is_wrong(x, t):
    """The batch's guess (int)g + 1 against lower_bound, in the device's arithmetic (doubles, the same operations)."""
    n = x.shape[0]
    inv_dx = (n - 1) / (x[-1] - x[0])
    g = (np.asarray(t, np.float64) - x[0]) * inv_dx
    guess = np.where(g > 0.0, np.where(g < n, np.minimum(g, n).astype(np.int64) + 1, n), 0)
    return guess != np.searchsorted(x, t, side="left")


def _prefix_cap(sc, split, t_step, trace):
    """A staging cap under which the kernel's own decision puts a part in the prefix variant: one that holds some part's fixed-size prefix
    (header, nodes, cells, trace) and not its list heap -- tried from the parts' own layouts first, then a sweep."""
    parts, incl, seeds, root_part, ref = split
    b = d.EmatBackend(sc.num_sites, trace_moves=trace)
    try:
        configure(b, sc, ref, parts, incl, seeds, root_part, t_step)
        lay = [b.debug_slab_layout(p) for p in range(len(parts))]
    finally:
        b.close()
    own = sorted({(l["header"] + l["nodes"] + l["cells"] + l["trace"] + 15) // 16 * 16 + 16 * k for l in lay for k in (1, 4, 16)}, reverse=True)
    for cap in own + list(range(32768, 256, -256)):
        b = d.EmatBackend(sc.num_sites, trace_moves=trace)
        try:
            b.set_option("lds_max", cap)
            configure(b, sc, ref, parts, incl, seeds, root_part, t_step)
            if _variant_counts(b)[1] > 0:
                return cap
        finally:
            b.close()
    pytest.fail("no staging cap tried puts a part in the prefix variant")


def _check(sc, num_parts, moves=MOVES, t_step=None, max_part_nodes=0, seed=SEED, modes=MODES, stepped=False, inspect=None):
    """One pass of `moves` traced moves per part in the oracle and, per mode, on the device: compare_part on every part.
    `inspect(parts, root_part, orc, cells)` looks at the oracle's finished pass (what the case is for)."""
    split = split_parts(sc, num_parts, seed, max_part_nodes)
    parts, incl, seeds, root_part, ref = split
    orc = OracleEngine(sc.num_sites, trace_moves=moves)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part, t_step)
        scales = [(abs(float(orc.part_derived(p, parts[p].num_nodes)[2])), abs(float(orc.part_derived(p, parts[p].num_nodes)[3]))) for p in range(len(parts))]
        cells = [orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(len(parts))]
        orc.run_moves_per_part(moves, threads=4)
        if inspect is not None:
            inspect(parts, root_part, orc, cells)
        for mode in modes:
            b = d.EmatBackend(sc.num_sites, trace_moves=moves, use_lds=mode != "no_lds")
            try:
                if mode == "prefix":
                    b.set_option("lds_max", _prefix_cap(sc, split, t_step, moves))
                configure(b, sc, ref, parts, incl, seeds, root_part, t_step)
                counts = _variant_counts(b)
                assert {"whole": counts[0] > 0, "prefix": counts[1] > 0, "no_lds": counts[2] == len(parts)}[mode], "%s: parts staged whole, by prefix, not at all: %s" % (mode, counts)
                if stepped:
                    for _ in range(moves):
                        b.run_moves_per_part(1); b.synchronize()
                else:
                    b.run_moves_per_part(moves); b.synchronize()
                for p in range(len(parts)):
                    compare_part(b, orc, p, parts[p].num_nodes, moves, 1e-9, moves, scales[p], cells[p])
            finally:
                b.close()
    finally:
        orc.close()


def _displaced_times(parts, orc, moves):
    """Times of the inner nodes that the traces' noted inner-node displacements name: before the pass, and after it."""
    before, after = [], []
    for p in range(len(parts)):
        tr = orc.part_trace(p, moves)
        nodes = np.unique(tr[(tr[:, 0] == K_INNER) & ~np.isnan(tr[:, 3]), 1].astype(np.int64))
        before.append(np.asarray(parts[p].t)[nodes]); after.append(np.asarray(orc.part_download(p).t)[nodes])
    return np.concatenate(before), np.concatenate(after)


# ---- 1. Skygrid grids ----------------------------------------------------------------------------------------------------
GRIDS = [(2, "even"), (3, "even"), (3, "up"), (3, "down"), (50, "even"), (50, "up"), (50, "down")]


@pytest.mark.parametrize("log_linear", [False, True], ids=["staircase", "log_linear"])
@pytest.mark.parametrize("knots,layout", GRIDS)
def test_skygrid_ratio_is_the_oracles(knots, layout, log_linear):
    sc = _base()
    x = _knots(sc, knots, layout)
    sc.pop = d.PopModel.skygrid(x, _gamma(knots), log_linear)

    def inspect(parts, root_part, orc, cells):
        t = np.concatenate(_displaced_times(parts, orc, MOVES))
        wrong = int(np.count_nonzero(_guess_is_wrong(x, t)))
        print("%d knots, %s: the guess is wrong for %d of %d displaced times" % (knots, layout, wrong, t.shape[0]))
        assert t.shape[0] >= 100
        if layout == "even":
            assert wrong <= t.shape[0] // 20, "an even grid's guess should stand: wrong for %d of %d times" % (wrong, t.shape[0])
        else:
            assert 2 * wrong >= t.shape[0], "the guess is wrong for only %d of %d displaced times" % (wrong, t.shape[0])

    _check(sc, 4, inspect=inspect)


# ---- 2. edge times -------------------------------------------------------------------------------------------------------
def _grid_origin(sc, num_parts, t_step):
    parts, incl, seeds, root_part, ref = split_parts(sc, num_parts, SEED)
    orc = OracleEngine(sc.num_sites, trace_moves=0)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part, t_step)
        return orc.part_coalescent(root_part)["t_ref"]
    finally:
        orc.close()


def _snap_to_cell_bounds(sc, t_ref, t_step, every=3):
    """Every `every`-th node whose neighbours allow it gets the time of the nearest cell bound (a double of the form t_ref - t_step * cell,
    as cell_ubound forms it).  Returns the snapped inner nodes and tips."""
    t = sc.tree
    snapped_inner, snapped_tips = [], []
    for i in range(0, t.num_nodes, every):
        if i == t.root:
            continue
        cell = int(np.round((t_ref - t.t[i]) / t_step))
        new_t = t_ref - t_step * cell
        lo = max(float(t.t[t.parent[i]]), float(np.max(t.mut_t[t.mut_offset[i]:t.mut_offset[i + 1]], initial=-np.inf)))
        hi = np.inf
        if t.child0[i] >= 0:
            for ch in (t.child0[i], t.child1[i]):
                hi = min(hi, float(t.t[ch]), float(np.min(t.mut_t[t.mut_offset[ch]:t.mut_offset[ch + 1]], initial=np.inf)))
        else:
            lo, hi = max(lo, float(t.t_min[i])), min(hi, float(t.t_max[i]))
            if t.t_min[i] == t.t_max[i] or t.t[i] == sc.t_max_tip:
                continue
        if lo < new_t < hi:
            t.t[i] = new_t
            (snapped_inner if t.child0[i] >= 0 else snapped_tips).append(i)
    return snapped_inner, snapped_tips


@pytest.mark.parametrize("log_linear", [False, True], ids=["staircase", "log_linear"])
def test_times_on_knots_on_cell_bounds_and_beyond_the_grid(log_linear):
    sc = _base()
    t_step = sc.default_t_step()
    t_ref = _grid_origin(sc, 2, t_step)
    inner, tips = _snap_to_cell_bounds(sc, t_ref, t_step)
    assert len(inner) >= 10 and len(tips) >= 3, "snapped %d inner nodes and %d tips" % (len(inner), len(tips))
    assert _grid_origin(sc, 2, t_step) == t_ref
    t = sc.tree
    is_inner = np.asarray(t.child0) >= 0
    t_inner, t_tips = np.sort(np.asarray(t.t)[is_inner]), np.sort(np.asarray(t.t)[~is_inner])
    # knots ON node and tip times (snapped ones among them), the first later than a fifth of the inner nodes, the last earlier than a fifth of the tips
    first, last = t_inner[len(t_inner) // 5], t_tips[(4 * len(t_tips)) // 5]
    on = np.concatenate([np.asarray(t.t)[inner], np.asarray(t.t)[tips], t_inner[::4], t_tips[::6]])
    x = np.unique(np.concatenate([[first, last], on[(on > first) & (on < last)]]))
    assert x.shape[0] >= 20 and x[0] == first and x[-1] == last
    sc.pop = d.PopModel.skygrid(x, _gamma(x.shape[0]), log_linear)

    def inspect(parts, root_part, orc, cells):
        before, _ = _displaced_times(parts, orc, MOVES)
        on_knots = int(np.count_nonzero(np.isin(before, x)))
        on_bounds = int(np.count_nonzero(t_ref - t_step * np.round((t_ref - before) / t_step) == before))
        print("displaced times: %d on knots, %d on cell bounds, %d before the first knot, %d after the last" % (on_knots, on_bounds, np.count_nonzero(before < x[0]), np.count_nonzero(before > x[-1])))
        assert on_knots >= 5 and on_bounds >= 5 and np.count_nonzero(before < x[0]) >= 5
        for p in range(len(parts)):   # tip displacements of tips beyond the last knot, and of tips on cell bounds
            tr = orc.part_trace(p, MOVES)
            assert p == root_part or np.count_nonzero((tr[:, 0] == 1) & ~np.isnan(tr[:, 3])) >= 5

    _check(sc, 2, t_step=t_step, inspect=inspect)


# ---- 3. one cell ---------------------------------------------------------------------------------------------------------
def test_a_part_whose_window_is_one_cell():
    sc = make_scenario("C3", num_tips=60, num_sites=500, uncertain_tips=0.2)   # (a Skygrid model of 50 knots)
    _, span = _span(sc)

    def inspect(parts, root_part, orc, cells):
        one = [p for p in range(len(parts)) if p != root_part and cells[p] == 1]
        print("%d parts, %d of them with a window of one cell" % (len(parts), len(one)))
        assert len(one) >= 3
        noted = sum(int(np.count_nonzero(~np.isnan(orc.part_trace(p, 200)[:, 3]) & (orc.part_trace(p, 200)[:, 0] <= 1))) for p in one)
        assert noted >= 50, "only %d displacements were evaluated in the one-cell parts" % noted

    _check(sc, 4, moves=200, t_step=span, max_part_nodes=3, seed=2, inspect=inspect)


# ---- 4. long branches ----------------------------------------------------------------------------------------------------
def test_displacements_across_ten_cells_and_more():
    sc = make_scenario("C3", num_tips=100, num_sites=2000, uncertain_tips=0.3)
    _, span = _span(sc)
    t_step = span / 4000.0

    def inspect(parts, root_part, orc, cells):
        crossed = 0
        for p in range(len(parts)):
            if p == root_part:
                continue
            tr = orc.part_trace(p, MOVES)
            nodes = np.unique(tr[(tr[:, 0] <= 1) & (tr[:, 2] == 1), 1].astype(np.int64))
            crossed += int(np.count_nonzero(np.abs(np.asarray(orc.part_download(p).t)[nodes] - np.asarray(parts[p].t)[nodes]) >= 10 * t_step))
        print("%d displaced nodes ended ten cells or more from where they began" % crossed)
        assert crossed >= 10

    _check(sc, 2, t_step=t_step, inspect=inspect)


# ---- 5. the other models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepped", [False, True], ids=["one_launch", "one_move_per_launch"])
@pytest.mark.parametrize("model", ["exponential", "constant"])
def test_exponential_and_constant_models_are_unchanged(model, stepped):
    sc = _base()
    sc.pop = d.PopModel.exp(sc.t_max_tip, 3 * 365.0, 2.0 / 365.0, 1.0) if model == "exponential" else d.PopModel.const(365.0)
    _check(sc, 4, stepped=stepped, modes=("whole",) if stepped else MODES)
