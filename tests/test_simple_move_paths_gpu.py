"""The simple moves with one copy of each path and their cold paths out of line (emat_device_core.hpp, emat_device_moves.hpp): a
displacement selects the ordered pair of its two times and walks the coalescent cells once, whichever way it goes; the Skygrid ratio
carries the batch and calls the knot search; a node's remembered rate change carries the test and calls the miss; a branch reform
dispatches to the register paths or to the general path.  All of it is code motion, so every case is the oracle's pass move for move
(compare_part), with the parts staged whole, staged by prefix and resident in HBM, each as one ticket per pass and as four.

What a case is FOR is asserted from the oracle's side alone, before anything of the device's is looked at -- a case that no longer
reaches its paths fails.  The oracle's chain is advanced one move at a time where the proposals matter (a stepped chain is the chain:
test_move_steps.py), and each displacement's PROPOSED time is restated from the part's random stream (draws_model.Words; the words of a
move are the kind, the node picks, the bounded exponential's uniform) in double arithmetic: for an accepted move it must be the time
the oracle wrote, to 1e-9 of the window (asserted), and for a rejected one it is the only witness of where the move meant to go.

  even      100 tips, 4 parts, 300 traced moves, an even Skygrid of 50 knots whose curve rises towards the present (a flat one rejects no
            inner node that moves towards the present), a grid of cells about as long as a typical displacement: inner-node displacements
            towards the past and towards the present, each accepted and rejected; walks within one cell and across exactly two, in the
            root part as well; the batch's guess stands (the knot search does not run).
  sparse    tip displacements towards the past and towards the present, each accepted and rejected.  A tip that moves towards the past
            takes lineage time out of its cells, which the prior rewards unless the part holds less than half a lineage there: four
            tips in five uncertain, 12 parts asked for (9 made), a fine grid, a small population that falls towards the present.
  bunched   the same with the knots bunched at the early end of twice the tree's span: the guess is wrong for at least half of the
            displaced times, so the knot search runs, and both verdicts occur behind it.
  fine      2 parts under a grid of 4 000 cells: walks across ten cells and more, in the root part as well.
  memo      two passes without topology moves (which alone forget a remembered rate change): every entry is unknown when the first
            starts (a fresh upload; counted on the device), and every entry the second asks for is known (from the traces: each child
            of each inner node the second pass displaces was asked for in the first; on the device: every entry a displacement can
            ask for is known between the passes, and no other).
  reforms   the 100-tip tree with its 30 000 sites, 5 parts, topology moves off, one branch given a site twice: noted reforms of branches
            of 1, 2, 3 and 4 mutations (the register paths), of exactly 5 and exactly 9 (the general path: two and three rounds of its
            four-wide gather) and of the branch with a site twice (handed on by the register path).
Tolerances are compare_part's (1e-9 relative on log MH ratios, totals and times; integers exact).  The oracle runs once per case."""
import ctypes as C
import math

import numpy as np
import pytest

import delphy_amd as d
import draws_model as DM
from delphy_amd.scenarios import make_scenario
from helpers import compare_part, configure, split_parts
from oracle_ffi import OracleEngine
from test_branch_reform_small_gpu import _with_a_site_twice
from test_chain_frame_gpu import _variant_counts
from test_coalescent_round_trips_gpu import _gamma, _guess_is_wrong, _knots, _prefix_cap, _span

pytestmark = pytest.mark.gpu

SEED = 11
MODES = ("whole", "prefix", "no_lds")
TICKETS = (1, 4)
K_INNER, K_TIP, K_REFORM = 0, 1, 2
HANDFUL = 5


class Case:
    """A scenario, its split, how it is run, and the oracle's finished pass (engine kept open for compare_part)."""

    def __init__(self, sc, num_parts, launches, t_step=None, topology=True, seed=SEED):
        self.sc, self.launches, self.t_step, self.topology = sc, tuple(launches), t_step, topology
        self.moves = sum(self.launches)
        self.split = split_parts(sc, num_parts, seed)
        self.parts, self.incl, self.seeds, self.root_part, self.ref = self.split
        self.orc = OracleEngine(sc.num_sites, trace_moves=self.moves)
        configure(self.orc, sc, self.ref, self.parts, self.incl, self.seeds, self.root_part, t_step, topology=topology)
        n = [p.num_nodes for p in self.parts]
        self.scales = [(abs(float(self.orc.part_derived(p, n[p])[2])), abs(float(self.orc.part_derived(p, n[p])[3]))) for p in range(len(n))]
        self.cells = [self.orc.part_coalescent(p)["k_bar_p"].shape[0] for p in range(len(n))]

    def run_oracle(self):
        for m in self.launches:
            self.orc.run_moves_per_part(m, threads=4)

    def traces(self):
        return [self.orc.part_trace(p, self.moves) for p in range(len(self.parts))]


# ---- a displacement's proposal, restated ----------------------------------------------------------------------------------
def _bounded_exponential(v, lam, a, b):
    """distributions.h:38-69 in doubles."""
    ltr = lam * (b - a)
    if lam == 0.0:
        x = a + v * (b - a)
    elif lam > 0 and ltr > 100:
        x = b + math.log(v) / lam
    elif lam < 0 and ltr < -100:
        x = a + math.log(v) / lam
    else:
        x = a + math.log1p(v * math.expm1(ltr)) / lam
    return min(max(x, a), b)


def _proposal(sc, tree, lam, rng, kind, node):
    """(t_min, t_max, proposed time) of the displacement of `node` (not the run's root) that starts at stream position `rng` on `tree`."""
    W = DM.Words(rng)
    assert DM.kind_of(W[0]) == kind, "the stream's first word does not say kind %d" % kind
    at, n = 1, tree.num_nodes
    while True:
        x = DM.pick(W[at], n); at += 1
        if (tree.child0[x] >= 0) == (kind == K_INNER):
            break
        assert at < 4096
    assert x == node, "the first acceptable pick is node %d, the row says %d" % (x, node)
    v = float(DM.to_oo(W[at]))
    muts = lambda i: tree.mut_t[tree.mut_offset[i]:tree.mut_offset[i + 1]]
    lo = max(float(tree.t[tree.parent[node]]), float(np.max(muts(node), initial=-np.inf)))
    if kind == K_TIP:
        lo, hi, slope = max(lo, float(tree.t_min[node])), float(tree.t_max[node]), -float(lam[node])
    else:
        q_a = -np.diag(d.hky_q_matrix(sc.kappa, sc.pi))
        hi, slope = np.inf, -float(lam[node])
        for ch in (int(tree.child0[node]), int(tree.child1[node])):
            hi = min(hi, float(tree.t[ch]), float(np.min(muts(ch), initial=np.inf)))
            sl = slice(int(tree.mut_offset[ch]), int(tree.mut_offset[ch + 1]))
            # lambda just below the node on the way to this child: the child's, without what its branch's mutations change
            slope += float(lam[ch]) - float(np.sum(sc.mu * (q_a[tree.mut_to[sl]] - q_a[tree.mut_from[sl]])))
    return lo, hi, _bounded_exponential(v, slope, lo, hi)


def _stepped_displacements(case):
    """The oracle's pass one move at a time.  Every NOTED displacement of a node other than the run's root, as a dict: part, root_part
    (bool), kind, accepted, old and proposed time, cells walked."""
    orc, sc, out = case.orc, case.sc, []
    ids = range(len(case.parts))
    tab = [orc.part_coalescent(p) for p in ids]
    snap = lambda p: (orc.part_download(p), orc.part_derived(p, case.parts[p].num_nodes)[0], orc.part_rng(p))
    for m in case.launches[:-1]:      # (whole: only the last launch is looked at move by move)
        orc.run_moves_per_part(m, threads=4)
    before = case.moves - case.launches[-1]
    prev = [snap(p) for p in ids]
    checked = 0
    for step in range(case.launches[-1]):
        orc.run_moves_per_part(1, threads=1)
        for p in ids:
            row = orc.part_trace(p, before + step + 1)[-1]
            kind, node, acc = int(row[0]), int(row[1]), bool(row[2])
            cur = snap(p) if (acc or kind >= K_REFORM) else (prev[p][0], prev[p][1], orc.part_rng(p))   # a rejected simple move changed nothing but the stream
            tree, lam, rng = prev[p]
            prev[p] = cur
            if kind > K_TIP or np.isnan(row[3]) or (node == tree.root and case.incl[p]):
                continue
            lo, hi, t_new = _proposal(sc, tree, lam, rng, kind, node)
            t_old = float(tree.t[node])
            if acc:
                wrote = float(cur[0].t[node])
                assert abs(wrote - t_new) <= 1e-9 * max(hi - lo, abs(wrote) * 1e-3), "part %d move %d: the restated proposal %r, the oracle wrote %r" % (p, step, t_new, wrote)
                t_new = wrote; checked += 1
            cell = lambda t: int(math.floor((tab[p]["t_ref"] - t) / tab[p]["t_step"]))
            out.append(dict(part=p, root_part=p == case.root_part, kind=kind, acc=acc, t_old=t_old, t_new=t_new, cells=abs(cell(t_new) - cell(t_old)) + 1))
    assert checked >= 50, "only %d accepted displacements checked the restated proposals" % checked
    return out


def _count(moves, **want):
    return sum(all((m[k] >= -v if (k == "cells" and v < 0) else m[k] == v) for k, v in want.items()) for m in moves)


def _assert_directions_and_verdicts(moves, what, kinds):
    for kind in kinds:
        for past in (True, False):
            for acc in (True, False):
                n = sum(m["kind"] == kind and m["acc"] == acc and (m["t_new"] < m["t_old"]) == past and m["t_new"] != m["t_old"] for m in moves)
                print("%s: %s displacements towards the %s, %s: %d" % (what, ("inner-node", "tip")[kind], "past" if past else "present", "accepted" if acc else "rejected", n))
                assert n >= HANDFUL, "%s: only %d %s displacements towards the %s were %s" % (what, n, ("inner-node", "tip")[kind], "past" if past else "present", "accepted" if acc else "rejected")


def _assert_walks(moves, what, lengths):
    """`lengths`: cells walked, a negative number meaning "at least".  Asked of the root part and of the others apart."""
    for root in (False, True):
        for L in lengths:
            n = _count(moves, root_part=root, cells=L)
            print("%s: walks of %s%d cells in %s: %d" % (what, "at least " if L < 0 else "", abs(L), "the root part" if root else "the other parts", n))
            assert n >= HANDFUL, "%s: only %d walks of %s%d cells in %s" % (what, n, "at least " if L < 0 else "", abs(L), "the root part" if root else "the other parts")


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _base():
    return make_scenario("C1", num_tips=100, num_sites=2000, uncertain_tips=0.3)


def _case_even():
    sc = _base()
    x = _knots(sc, 50, "even")
    sc.pop = d.PopModel.skygrid(x, _gamma(50, EVEN_N0) + EVEN_RISE * np.arange(50) / 50.0, True)
    case = Case(sc, 4, (300,), t_step=_span(sc)[1] / EVEN_CELLS)
    moves = _stepped_displacements(case)
    _assert_directions_and_verdicts(moves, "even", (K_INNER,))
    _assert_walks(moves, "even", (1, 2))
    t = np.array([m["t_old"] for m in moves if m["kind"] == K_INNER] + [m["t_new"] for m in moves if m["kind"] == K_INNER])
    wrong = int(np.count_nonzero(_guess_is_wrong(x, t)))
    print("even: the guess is wrong for %d of %d times of displaced inner nodes" % (wrong, t.shape[0]))
    assert t.shape[0] >= 100 and wrong <= t.shape[0] // 20
    return case


def _case_sparse():
    sc = make_scenario("C1", num_tips=100, num_sites=2000, uncertain_tips=0.8)
    sc.pop = d.PopModel.skygrid(_knots(sc, 50, "even"), _gamma(50, 10.0) - 6.0 * np.arange(50) / 50.0, True)
    case = Case(sc, 12, (300,), t_step=_span(sc)[1] / 100.0)
    _assert_directions_and_verdicts(_stepped_displacements(case), "sparse", (K_TIP,))
    return case


def _case_bunched():
    sc = _base()
    x = _knots(sc, 50, "up")
    sc.pop = d.PopModel.skygrid(x, _gamma(50), True)
    case = Case(sc, 4, (300,), t_step=_span(sc)[1] / EVEN_CELLS)
    moves = [m for m in _stepped_displacements(case) if m["kind"] == K_INNER]
    searched = [m for m in moves if _guess_is_wrong(x, np.array([m["t_old"]]))[0] or _guess_is_wrong(x, np.array([m["t_new"]]))[0]]
    n_acc = sum(m["acc"] for m in searched)
    print("bunched: the knot search runs for %d of %d noted inner-node displacements (%d accepted, %d rejected)" % (len(searched), len(moves), n_acc, len(searched) - n_acc))
    assert len(moves) >= 100 and 2 * len(searched) >= len(moves)
    assert n_acc >= HANDFUL and len(searched) - n_acc >= HANDFUL
    return case


def _case_fine():
    sc = make_scenario("C3", num_tips=100, num_sites=2000, uncertain_tips=0.3)
    case = Case(sc, 2, (300,), t_step=_span(sc)[1] / 4000.0)
    moves = _stepped_displacements(case)
    _assert_walks(moves, "fine", (-10,))
    return case


def _asked_for(case, tr, part):
    """The nodes whose remembered rate change the rows `tr` of part `part` ask for, in order: both children of every displaced inner node
    (in a part without the run's root, a pick of the part's root ends before it asks)."""
    t = case.parts[part]
    out = []
    for row in tr[tr[:, 0] == K_INNER]:
        node = int(row[1])
        if node == t.root and not case.incl[part]:
            continue
        out += [int(t.child0[node]), int(t.child1[node])]
    return out


def _askable(case, part):
    """The nodes a pass without topology moves can ask for: every child of an inner node that a displacement can get as far as."""
    t = case.parts[part]
    inner = [x for x in range(t.num_nodes) if t.child0[x] >= 0 and (x != t.root or case.incl[part])]
    return {int(t.child0[x]) for x in inner} | {int(t.child1[x]) for x in inner}


def _case_memo():
    sc = _base()
    sc.pop = d.PopModel.skygrid(_knots(sc, 50, "even"), _gamma(50), True)
    case = Case(sc, 4, (MEMO_FIRST, 300), topology=False)
    case.run_oracle()
    for p, tr in enumerate(case.traces()):
        first, second = _asked_for(case, tr[:MEMO_FIRST], p), _asked_for(case, tr[MEMO_FIRST:], p)
        misses = len(set(first))
        print("memo: part %d: the first pass asks %d times for %d nodes (all unknown at the start), the second %d times" % (p, len(first), misses, len(second)))
        assert misses >= HANDFUL and len(first) - misses >= HANDFUL, "part %d: the first pass holds %d misses and %d hits" % (p, misses, len(first) - misses)
        assert len(second) >= HANDFUL and set(second) <= set(first), "part %d: the second pass asks for nodes the first did not: %s" % (p, sorted(set(second) - set(first)))
        assert set(first) == _askable(case, p), "part %d: the first pass leaves entries unknown: %s" % (p, sorted(_askable(case, p) - set(first)))
    return case


def _reform_scenario():
    sc = make_scenario("C1", num_tips=100)
    t = sc.tree
    free = np.ones(sc.num_sites, bool)
    free[t.mut_site[:int(t.mut_offset[-1])]] = False
    free[t.mfs_site[:int(t.mfs_offset[-1])]] = False
    for s, e in zip(t.miss_start[:int(t.miss_offset[-1])], t.miss_end[:int(t.miss_offset[-1])]):
        free[s:e] = False
    return _with_a_site_twice(sc, REFORM_TWICE_NODE, int(np.nonzero(free)[0][0]))


def _case_reforms():
    case = Case(_reform_scenario(), 5, (REFORM_MOVES,), topology=False, seed=REFORM_SEED)
    case.run_oracle()
    cls = {}
    for part, tr in zip(case.parts, case.traces()):
        for row in tr[(tr[:, 0] == K_REFORM) & ~np.isnan(tr[:, 3])]:
            s = part.mut_site[part.mut_offset[int(row[1])]:part.mut_offset[int(row[1]) + 1]]
            key = "twice" if len(set(s.tolist())) != len(s) else len(s)
            cls[key] = cls.get(key, 0) + 1
    print("reforms: noted reforms per number of mutations on the branch:", {k: cls[k] for k in sorted(cls, key=str)})
    for k in (1, 2, 3, 4, 5, 9, "twice"):
        assert cls.get(k, 0) >= HANDFUL, "only %d noted reforms of class %s" % (cls.get(k, 0), k)
    return case


EVEN_RISE = 4.0           # how much log N rises from the first knot to the last in `even`
EVEN_N0 = 365.0           # its level, as a population size
EVEN_CELLS = 40           # cells over the tree's span in `even` and `bunched`
MEMO_FIRST = 1500         # moves of the memo case's first pass
REFORM_TWICE_NODE, REFORM_SEED, REFORM_MOVES = 6, 11, 300
BUILDERS = {"even": _case_even, "sparse": _case_sparse, "bunched": _case_bunched, "fine": _case_fine, "memo": _case_memo, "reforms": _case_reforms}
_open = {}


def _case(name):
    if name not in _open:
        _open[name] = BUILDERS[name]()      # (a builder that fails its assertions leaves nothing behind: the next test builds, and fails, again)
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_oracles():
    yield
    for case in _open.values():
        case.orc.close()
    _open.clear()


def _known_entries(b, num_parts):
    lib = d.load_library()
    lib.emat_debug_miss_dl_check.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.emat_debug_miss_dl_check.restype = C.c_int
    out = np.zeros(2 * num_parts, np.int32)
    assert lib.emat_debug_miss_dl_check(b.handle, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0, b.last_error()
    assert np.all(out[0::2] == 0), "stale remembered values: %s" % out[0::2]
    return out[1::2]


@pytest.mark.parametrize("tickets", TICKETS, ids=["one_ticket", "four_tickets"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(BUILDERS))
def test_the_pass_is_the_oracles(name, mode, tickets):
    case = _case(name)
    sc, parts = case.sc, case.parts
    b = d.EmatBackend(sc.num_sites, trace_moves=case.moves, use_lds=mode != "no_lds")
    try:
        b.set_option("chunks", tickets)
        if mode == "prefix":
            b.set_option("lds_max", _prefix_cap(sc, case.split, case.t_step, case.moves))
        configure(b, sc, case.ref, parts, case.incl, case.seeds, case.root_part, case.t_step, topology=case.topology)
        counts = _variant_counts(b)
        assert {"whole": counts[0] > 0, "prefix": counts[1] > 0, "no_lds": counts[2] == len(parts)}[mode], "%s: parts staged whole, by prefix, not at all: %s" % (mode, counts)
        for k, m in enumerate(case.launches):
            b.run_moves_per_part(m); b.synchronize()
            if name == "memo":
                known = _known_entries(b, len(parts))
                print("memo, after pass %d: known entries per part %s of %s nodes" % (k, known.tolist(), [p.num_nodes for p in parts]))
                # (the part that holds the run's root also asks for the root's own entry: calc_lambda_at_node walks up to it when a reform next to the root re-hangs its branch)
                assert all(known[p] == len(_askable(case, p)) + (p == case.root_part) for p in range(len(parts))), "known entries %s" % known.tolist()
        for p in range(len(parts)):
            compare_part(b, case.orc, p, parts[p].num_nodes, case.moves, 1e-9, case.moves, case.scales[p], case.cells[p])
    finally:
        b.close()


def test_every_remembered_rate_change_is_unknown_after_an_upload():
    """What `memo`'s first pass starts from, counted on the device after ONE move per part (the parts lie on the device from the first
    launch on): a move asks for two entries at most, so no part may know more."""
    case = _case("memo")
    b = d.EmatBackend(case.sc.num_sites)
    try:
        configure(b, case.sc, case.ref, case.parts, case.incl, case.seeds, case.root_part, case.t_step, topology=False)
        b.run_moves_per_part(1); b.synchronize()
        known = _known_entries(b, len(case.parts))
        print("known entries per part after one move:", known.tolist())
        assert np.all(known <= 2)
    finally:
        b.close()
