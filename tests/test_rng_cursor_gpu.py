"""The chain's place in its random stream is one cursor into the words the wave computes ahead (emat_rng_pos.hpp; Ctx::rng_base,
Ctx::rng_pos): every way a leg can begin and end, draws across the end of the buffer, the rewind of a stopped move and the hooks
that draw on a context nobody fills -- each against the CPU oracle, move for move.

What the oracle knows of a stream's position is the number of Philox blocks opened (part_stats()["rng_draws"]); whether the second
half of the last block is still to come (has_spare) it keeps to itself.  Where a test needs a WORD position it therefore takes the
block count from the oracle, stepped one move at a time, and the parity from the device stepped the same way (part_rng()["has_spare"]):
the device's counter is held to the oracle's after every single move and its trace to the oracle's trace, and a chain whose parity
were off would draw other words than the oracle's from the next move on.
"""
import numpy as np
import pytest

import delphy_amd as d
import delphy_amd.engine as e
from delphy_amd.scenarios import KAPPA, PI, Scenario, make_scenario
from helpers import assert_traces_match, configure, run_parity, split_parts
from oracle_ffi import OracleEngine

pytestmark = pytest.mark.gpu

RNG_BLOCKS, RNG_MARGIN = 32, 8      # emat_device_core.hpp: EMAT_RNG_BLOCKS, EMAT_RNG_MARGIN


# ---- the cursor, restated (emat_rng_pos.hpp) ---------------------------------------------------------------------------
def cursor_of_a_single_leg(words):
    """`words[m]` = the stream's word position before move m of a pass that is ONE leg (words[-1]: after the last move).  Returns, per
    move, (pos at its first draw, pos after its last draw), with the fill rule applied between moves as run_chain applies it."""
    pos = 2 * RNG_BLOCKS + 2 + (words[0] & 1)        # rng_pos_enter: nothing counts as computed ahead
    out = []
    for m in range(len(words) - 1):
        if ((pos + 1) >> 1) + RNG_MARGIN > RNG_BLOCKS:       # rng_pos_wants_fill
            pos &= 1                                         # rng_pos_after_fill
        out.append((pos, pos + int(words[m + 1] - words[m])))
        pos = out[-1][1]
    return out


# ---- passes ------------------------------------------------------------------------------------------------------------
def _setup(sc, nparts, seed, t_step=None):
    return (sc,) + split_parts(sc, nparts, seed) + (t_step,)


def _configured(engine, case):
    sc, parts, incl, seeds, root_part, ref, t_step = case
    configure(engine, sc, ref, parts, incl, seeds, root_part, t_step)
    return engine


_oracle_cache = {}


def oracle_stepped(key, case, moves):
    """The oracle, one move at a time: (trace per part, blocks opened per part after 0 .. moves moves).  Computed once per case."""
    if key not in _oracle_cache:
        n = len(case[1])
        orc = _configured(OracleEngine(case[0].num_sites, trace_moves=moves), case)
        try:
            blocks = [[orc.part_stats(p)["rng_draws"]] for p in range(n)]
            for _ in range(moves):
                orc.run_moves_per_part(1, threads=1)
                for p in range(n):
                    blocks[p].append(orc.part_stats(p)["rng_draws"])
            traces = [orc.part_trace(p, moves) for p in range(n)]
            assert all(orc.part_stats(p)["status"] == 0 and traces[p].shape == (moves, 4) for p in range(n))
        finally:
            orc.close()
        _oracle_cache[key] = (traces, np.array(blocks, np.int64))
    return _oracle_cache[key]


def device_pass(case, moves, chunks=None, stepped=False, use_lds=True):
    """One pass of `moves` moves per part.  Returns the traces, the counters and the streams' positions it left (per part), and for a
    stepped pass (one move per launch) the position after every move."""
    n = len(case[1])
    b = d.EmatBackend(case[0].num_sites, trace_moves=moves, use_lds=use_lds)
    try:
        if chunks is not None:
            b.set_option("chunks", chunks)
        _configured(b, case)
        after = []
        if stepped:
            for _ in range(moves):
                b.run_moves_per_part(1); b.synchronize()
                after.append([b.part_rng(p) for p in range(n)])
        else:
            b.run_moves_per_part(moves); b.synchronize()
        st = [b.part_stats(p) for p in range(n)]
        assert all(s["status"] == 0 and s["moves_done"] == moves for s in st), (st, b.last_error())
        return dict(trace=[b.part_trace(p, moves) for p in range(n)], draws=[s["rng_draws"] for s in st], rng=[b.part_rng(p) for p in range(n)], after=after)
    finally:
        b.close()


def assert_same_pass(a, b, what):
    for p in range(len(a["trace"])):
        assert a["trace"][p].tobytes() == b["trace"][p].tobytes(), "%s: part %d: traces differ" % (what, p)
        assert a["draws"][p] == b["draws"][p], "%s: part %d: rng_draws %d vs %d" % (what, p, a["draws"][p], b["draws"][p])
        ra, rb = a["rng"][p], b["rng"][p]
        assert (ra["key"], ra["counter"], ra["has_spare"]) == (rb["key"], rb["counter"], rb["has_spare"]), "%s: part %d: %s vs %s" % (what, p, ra, rb)
        if ra["has_spare"]:
            assert ra["spare"] == rb["spare"], "%s: part %d: the pending word differs: %s vs %s" % (what, p, ra, rb)


def assert_the_oracles_chain(run, traces, blocks, what):
    for p in range(len(traces)):
        assert_traces_match(run["trace"][p], traces[p], 1e-9, "%s part %d" % (what, p))
        assert run["draws"][p] == blocks[p][-1], "%s: part %d: rng_draws %d, the oracle's %d" % (what, p, run["draws"][p], blocks[p][-1])
        for m, after in enumerate(run["after"]):
            assert after[p]["counter"] == blocks[p][m + 1], "%s: part %d move %d: %d blocks opened, the oracle's %d" % (what, p, m, after[p]["counter"], blocks[p][m + 1])


def word_positions(stepped, blocks, p):
    """Word position of part p's stream before move 0 .. after the last move: the oracle's blocks, the stepped device run's parity."""
    return np.array([2 * int(blocks[p][0])] + [2 * int(blocks[p][m + 1]) - int(bool(a[p]["has_spare"])) for m, a in enumerate(stepped["after"])], np.int64)


# ---- 1. every way a leg can begin --------------------------------------------------------------------------------------
C1_MOVES = 300


def _c1_case():
    return _setup(make_scenario("C1", num_tips=100, num_sites=3000, uncertain_tips=0.2), 4, 11)


def test_a_pass_is_the_same_chain_however_its_legs_begin():
    """One ticket, four tickets, six tickets, and one move per launch: identical traces, rng_draws and stream positions, and the oracle's
    trace.  A leg of the stepped pass begins where the move before it ended, and those positions are odd and even, in every part."""
    case = _c1_case()
    traces, blocks = oracle_stepped("C1", case, C1_MOVES)
    one = device_pass(case, C1_MOVES, chunks=1)
    assert_the_oracles_chain(one, traces, blocks, "one ticket")
    for chunks in (4, 6):
        assert_same_pass(one, device_pass(case, C1_MOVES, chunks=chunks), "%d tickets against one" % chunks)
    stepped = device_pass(case, C1_MOVES, stepped=True)
    assert_the_oracles_chain(stepped, traces, blocks, "one move per launch")
    assert_same_pass(one, stepped, "one move per launch against one ticket")
    for p in range(len(traces)):
        begins = [int(bool(a[p]["has_spare"])) for a in stepped["after"][:-1]]     # where legs 1 .. moves - 1 began (leg 0: at word 0, even)
        odd = sum(begins)
        print("part %d: %d legs of the stepped pass began on an odd word, %d on an even one; %d blocks in %d moves" % (p, odd, len(begins) + 1 - odd, blocks[p][-1], C1_MOVES))
        assert odd >= 10 and len(begins) - odd >= 10, "part %d: legs began on %d odd and %d even positions" % (p, odd, len(begins) - odd)


# ---- 2. across the end of the buffer -----------------------------------------------------------------------------------
LONG_MOVES = 300
LONG_SEED = 1


def _long_branches_case():
    """Few tips and a high rate: branches of tens of mutations, so that a branch reform (one draw per mutation, the pick, the
    acceptance) draws more than the 16 numbers the margin keeps for a move."""
    par = e.SynthParams(num_tips=16, num_sites=4000, tip_span=30.0, pop_n0=300.0, pop_growth=0.0, mu=2.5e-2 / 365.0, gaps_per_tip=1, mean_gap_len=20.0, seed=LONG_SEED)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, tmax = e.make_synthetic_emat(par)
    sc = Scenario("long-branches", tree, ref, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, 300.0, 0.0, 0.0), par.num_sites)
    return _setup(sc, 1, 7)


def buffer_crossings(words):
    """(moves that drew beyond the buffer and began on an even word, ... on an odd word, moves that ended exactly on its last word)."""
    k2 = 2 * RNG_BLOCKS
    cur = cursor_of_a_single_leg(words)
    past = [(a, b) for a, b in cur if b > k2]
    return sum(1 for a, _ in past if a % 2 == 0), sum(1 for a, _ in past if a % 2 == 1), sum(1 for _, b in cur if b == k2)


@pytest.mark.parametrize("use_lds", [True, False])
def test_moves_that_draw_beyond_the_buffer_are_the_oracles(use_lds):
    """The cursor of the one-ticket pass, from the oracle's blocks per move, the stepped device run's parity and the fill rule: at least
    ten moves draw beyond the buffer, beginning on odd and on even words, and at least one move ends exactly on the buffer's last word.
    Then the pass, staged whole and resident in HBM, is the oracle's move for move."""
    case = _long_branches_case()
    muts = np.diff(case[1][0].mut_offset)
    assert np.sum((muts >= 20) & (muts <= 60)) >= 5, "branches of 20 to 60 mutations: %s" % sorted(muts.tolist())
    traces, blocks = oracle_stepped("long", case, LONG_MOVES)
    stepped = device_pass(case, LONG_MOVES, stepped=True, use_lds=use_lds)
    assert_the_oracles_chain(stepped, traces, blocks, "one move per launch")
    even, odd, on_last = buffer_crossings(word_positions(stepped, blocks, 0))
    print("moves that drew beyond the buffer: %d began on an even word, %d on an odd one; %d moves ended on its last word" % (even, odd, on_last))
    assert even + odd >= 10 and even >= 1 and odd >= 1 and on_last >= 1, (even, odd, on_last)
    one = device_pass(case, LONG_MOVES, chunks=1, use_lds=use_lds)
    assert_the_oracles_chain(one, traces, blocks, "one ticket")
    assert_same_pass(one, stepped, "one move per launch against one ticket")


# ---- 3. the rewind -----------------------------------------------------------------------------------------------------
def _deep_root_case(split_seed):
    """tests/test_miss_dl_memo_gpu.py's interrupted pass: almost no signal in the data, so the root wanders past the cells its slab has room for."""
    par = e.SynthParams(num_tips=120, num_sites=60, tip_span=30.0, pop_n0=400.0, pop_growth=0.0, mu=2e-5, gaps_per_tip=1, mean_gap_len=4.0, seed=3)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, tmax = e.make_synthetic_emat(par)
    sc = Scenario("deep-root", tree, ref, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, 400.0, 0.0, 0.0), 60)
    return sc, sc.default_t_step() * 0.25


REWIND_MOVES = 4000
REWIND_SEEDS = (7, 14)      # split seeds; chosen so that the first stopped move began on an even word with one and on an odd word with the other


def stopped_moves(case, moves):
    """The root part's pass on the device in launches of one move, up to the first launch that had to regrow the grid: (index of the
    stopped move, has_spare before it)."""
    sc, parts, incl, seeds, root_part, ref, t_step = case
    b = _configured(d.EmatBackend(sc.num_sites), case)
    try:
        cells = b.part_coalescent(root_part)["k_bar_p"].shape[0]
        cap = cells + max(512, cells)
        odd = False                                   # a fresh stream stands at word 0
        for m in range(moves):
            b.run_moves_per_part(1); b.synchronize()
            if b.part_coalescent(root_part)["k_bar_p"].shape[0] > cap:
                return m, odd
            odd = bool(b.part_rng(root_part)["has_spare"])
    finally:
        b.close()
    return None, None


@pytest.mark.parametrize("split_seed", REWIND_SEEDS)
def test_a_move_stopped_to_regrow_the_grid_starts_again_from_its_first_draw(split_seed):
    sc, t_step = _deep_root_case(split_seed)
    st = run_parity(sc, 5, REWIND_MOVES, seed=split_seed, trace=REWIND_MOVES, t_step=t_step)
    assert st["moves_done"] == REWIND_MOVES


def test_the_stopped_moves_began_on_an_odd_and_on_an_even_word():
    """The two cases above differ in where the first stopped move found the stream: stepped one move per launch up to the launch whose
    move outgrew the grid (a stop inside that launch: the root part's grid is past the room a freshly cut slab has)."""
    seen = {}
    for split_seed in REWIND_SEEDS:
        sc, t_step = _deep_root_case(split_seed)
        m, odd = stopped_moves(_setup(sc, 5, split_seed, t_step), 1500)
        print("split seed %d: move %s was stopped, the stream %s" % (split_seed, m, None if m is None else ("held a spare word" if odd else "stood at a block's first word")))
        assert m is not None, "split seed %d: no move outgrew the grid within 1500 moves" % split_seed
        seen[odd] = split_seed
    assert set(seen) == {True, False}, seen


# ---- 4. the hooks with a private context ---------------------------------------------------------------------------------
def test_the_hooks_draw_the_oracles_numbers_on_a_context_nobody_fills():
    """emat_debug_sample_history and emat_debug_graft mode 3 run dev:: code on a private context: every draw computes its block
    (rng_next64_computed).  The same fixture, seed and arguments through the oracle's counterparts: the same histories, the same graft."""
    import graft_golden as gg
    from test_golden_reference_expectations import SM
    h = SM["sample_mutational_history"]
    fx = SM["fixtures"][h["fixture"]]
    tree = gg.fixture_tree(fx)
    rng = np.random.default_rng(7)
    n = 200
    branch = rng.integers(0, tree.num_nodes - 1, n).astype(np.int32)
    branch = np.where(branch >= fx["root"], branch + 1, branch).astype(np.int32)
    lo, hi = tree.t[tree.parent[branch]], tree.t[branch]
    t_end = lo + (hi - lo) * rng.random(n)
    T = h["mu_T"] / SM["mu_JC"]
    start = np.asarray(h["target_start_seq"], np.uint8)
    got = {}
    for name, cls in (("device", d.EmatBackend), ("oracle", OracleEngine)):
        eng = cls(len(fx["ref_sequence"]))
        try:
            gg.configure_fixture(eng, fx, True, 12345)
            got[name] = (eng.debug_sample_history(0, branch, t_end, start, T, SM["mu_JC"]), eng.part_stats(0)["rng_draws"])
        finally:
            eng.close()
    assert got["device"][1] == got["oracle"][1] and got["device"][1] > n, got["device"][1]
    for i, (a, b) in enumerate(zip(got["device"][0], got["oracle"][0])):
        assert [m[:3] for m in a] == [m[:3] for m in b], (i, a, b)
        assert np.allclose([m[3] for m in a], [m[3] for m in b], rtol=1e-9, atol=0.0), (i, a, b)
    lst = SM["full_spr_move"][0]
    fx = SM["fixtures"][lst["fixture"]]
    X, SS, t = lst["cases"][0]
    res = {}
    for name, cls in (("device", d.EmatBackend), ("oracle", OracleEngine)):
        eng = cls(len(fx["ref_sequence"]))
        try:
            gg.configure_fixture(eng, fx, True, 12345)
            if name == "device":
                eng.recalc_derived()
            res[name] = (eng.debug_graft(0, X, SM["mu_JC"], 3, SS, t), eng.part_stats(0)["rng_draws"], eng.part_download(0))
        finally:
            eng.close()
    assert res["device"][1] == res["oracle"][1], (res["device"][1], res["oracle"][1])
    gg.same_grafts(res["device"][0]["grafts"][1], res["oracle"][0]["grafts"][1])
    ta, tb = res["device"][2], res["oracle"][2]
    assert np.array_equal(ta.mut_site, tb.mut_site) and np.array_equal(ta.mut_to, tb.mut_to) and np.allclose(ta.mut_t, tb.mut_t, rtol=1e-9, atol=0.0)
