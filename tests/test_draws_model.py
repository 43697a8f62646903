"""tests/draws_model.py on the CPU: its inverse CDFs against an independent quadrature of the densities, the cases that reach what
test_move_steps.py's do not (a slope steep enough for the bounded exponential's short spellings, a slope that is exactly zero, a window two doubles wide in which
every drawn time lands on a bound) on the oracle, and recorded oracle steps, doctored, each of which the model must refuse.
test_draws_model_gpu.py points the same cases at the device."""
import copy
from fractions import Fraction as F
from types import SimpleNamespace

import mpmath as mp
import numpy as np
import pytest

import draws_model as DM
import exact_model as X
import move_steps as M
from test_exact_model import Tally
from test_move_steps import DRAW_CASES, TOPOLOGY_OFF, _oracle, prepare, run_case

_done = {}
V_GRID = [F(1, 2 ** 53), F(1, 1000), F(3, 10), F(1, 2), F(9, 10), 1 - F(1, 2 ** 53)]


# ---- the model's inverse CDFs against quadrature ------------------------------------------------------------------------
@pytest.mark.parametrize("lam, a, b, cls", [(F(25), F(-3), F(7), 0), (F(-25), F(-3), F(7), 1), (F(1, 10 ** 8), F(-3), F(7), 2), (F(-1, 10 ** 8), F(5), F(6), 2),
                                              (F(3, 10), F(-3), F(7), 3), (F(-4), F(-3), F(7), 3), (F(0), F(-3), F(7), 4)])
def test_bounded_exponential_quantile_against_quadrature(lam, a, b, cls):
    """integral of the density lambda exp(lambda (y - a)) / expm1(lambda (b - a)) from a to F^-1(v) is v, for v down to 2^-53 and up to
    1 - 2^-53, in every class of ltr."""
    D = b - a
    assert DM.bexp_class(lam, D) == cls
    with mp.workdps(60):
        dens = (lambda y: mp.mpf(1)) if lam == 0 else (lambda y: mp.exp(X._mp(lam) * (y - X._mp(b))))       # (scaled by exp(-lambda (b - a)): the ratio is what counts)
        for v in V_GRID:
            x = X._mp(a) + DM.bexp_offset(v, lam, D)
            assert X._mp(a) <= x <= X._mp(b)
            cuts = lambda lo, hi: [lo + (hi - lo) * mp.mpf(k) / 16 for k in range(17)]
            part, whole = mp.quad(dens, cuts(X._mp(a), x)), mp.quad(dens, cuts(X._mp(a), x)) + mp.quad(dens, cuts(x, X._mp(b)))
            assert abs(part / whole - X._mp(v)) <= mp.mpf(10) ** -30 * max(X._mp(v), mp.mpf(10) ** -10), (float(lam), float(v), float(part / whole))


def test_gaussian_radius_power_law_and_gamma_against_quadrature():
    with mp.workdps(60):
        for w1 in (0, 1 << 11, 1 << 40, 1 << 63, (1 << 64) - 1):
            z, r = DM.gauss_z(w1, 0)                              # angle 0: z is the radius, P(R > r) = u1 for the Rayleigh radius
            tail = mp.quad(lambda y: y * mp.exp(-y * y / 2), [r, r + 1, r + 4, r + 16, mp.inf])
            assert z == r and abs(tail - X._mp(DM.to_oc(w1))) <= mp.mpf(10) ** -40
        z, r = DM.gauss_z(5 << 50, 1 << 62)                       # a quarter turn: the cosine of pi / 2
        assert abs(z) <= mp.mpf(10) ** -50 * r
        for a, s_min, s_max in ((F(1), F(0), F(3)), (F(0.8) * 3 + 1, F(1, 7), F(40)), (F(0.8) + 1, F(2), F(2) + F(1, 1000))):
            for v in V_GRID:
                s, _ = DM.power_quantile(v, a, s_min, s_max)
                dens = lambda y: X._mp(a) * mp.power(y, X._mp(a) - 1)
                part, whole = mp.quad(dens, [X._mp(s_min), s]), mp.quad(dens, [X._mp(s_min), X._mp(s_max)])
                assert abs(part / whole - X._mp(v)) <= mp.mpf(10) ** -30, (float(a), float(v))
        for a, x in ((F(1), F(1, 3)), (F(0.8) * 2 + 1, F(5)), (F(0.8) * 7 + 1, F(1, 50))):
            g = lambda y: mp.exp((X._mp(a) - 1) * mp.log(y) - y - mp.loggamma(X._mp(a)))
            assert abs(mp.quad(g, [X._mp(x), X._mp(x) + 10, X._mp(x) + 100, mp.inf]) - DM.gamma_Q(a, X._mp(x))) <= mp.mpf(10) ** -35


def test_the_uniforms_and_the_pick():
    top = (1 << 64) - 1
    assert DM.to_co(0) == 0 and DM.to_co(top) == 1 - F(1, 2 ** 53) and DM.to_oc(0) == F(1, 2 ** 53) and DM.to_oc(top) == 1
    assert DM.to_oo(0) == F(1, 2 ** 53) and DM.to_oo(top) == 1 - F(1, 2 ** 53) and 1 - DM.to_oo(12345 << 12) == DM.to_oo(top - (12345 << 12))
    assert [DM.pick(w, 7) for w in (0, top, 1 << 63)] == [0, 6, 3]
    at = lambda r, total: int(F(r) / F(total) * 2 ** 53) << 11             # the word whose draw is exactly r (r / total a dyadic fraction)
    assert [DM.kind_of(at(r, 32.0), 32.0) for r in DM.CUTS] == [1, 2, 3, 4]
    assert [DM.kind_of(at(r, 32.0) - (1 << 11), 32.0) for r in DM.CUTS] == [0, 1, 2, 3]
    assert [DM.kind_of(at(r, 30.0), 30.0, False) for r in DM.CUTS[:2]] == [1, 2] and [DM.kind_of(at(r, 30.0) - (1 << 11), 30.0, False) for r in DM.CUTS[:2]] == [0, 1]
    assert DM.kind_of(top, 30.0, False) == 2 and DM.kind_of(top, 32.0) == 4


# ---- the cases CASES do not reach, on the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("name", DRAW_CASES)
def test_oracle_draw_cases(name, record_property):
    tally, cov = _done[name] = run_case(name, _oracle, "oracle")
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    tally.finish(record_property)
    assert cov.unchecked == 0 and cov.borderline == 0, cov.as_dict()


def assert_draw_case_conditions(done, record_property=None):
    """What DRAW_CASES must reach (the minimums are the oracle's counts on the committed seeds; the device meets the same)."""
    cov = {name: done[name][1] for name in DRAW_CASES}
    for name, c in cov.items():
        if record_property:
            record_property("coverage_" + name, c.as_dict())
        assert c.unchecked == 0 and c.borderline == 0 and c.position_half_known == 0 and c.draws_held == c.steps, (name, c.as_dict())
        if name != "zero-slope":
            assert c.slope_sign_undetermined == 0, (name, c.as_dict())
    steep, zero, bound = cov["steep"], cov["zero-slope"], cov["on-a-bound"]
    assert steep.draws_bexp[0] >= 24 and steep.draws_bexp[1] >= 53 and steep.draws_bexp[3] >= 96, dict(zip(DM.BEXP_CLASSES, steep.draws_bexp))
    # the steep windows lie in the part WITHOUT the run's root: both short spellings ran in that copy of the simple moves
    assert steep.draws_bexp_outside_root_part[:2] == steep.draws_bexp[:2], dict(zip(DM.BEXP_CLASSES, steep.draws_bexp_outside_root_part))
    assert steep.draws_gaussian_root >= 7 and steep.draws_early_end[6] >= 1, steep.as_dict()
    assert zero.draws_bexp[4] >= 9, zero.as_dict()                      # steps of the zero-slope case that passed as the uniform draw
    # tip displacements whose drawn time landed on an end of the window: un-noted, the pick's words and one more, no acceptance word
    assert bound.draws_early_end[5] >= 18 and bound.draws_early_end[11] == 0, dict(zip(DM.EARLY, bound.draws_early_end))


def test_oracle_draw_cases_cover_what_they_must(record_property):
    for name in DRAW_CASES:
        if name not in _done:
            _done[name] = run_case(name, _oracle, "oracle")
    assert_draw_case_conditions(_done, record_property)


# ---- the checker must be able to fail -----------------------------------------------------------------------------------
def _record(name, parts_watched, steps, wanted):
    """Steps of the oracle's chain of case `name` as draws_model.Step, the first of each kind `wanted` names: {label: predicate(step)}."""
    sc, parts, incl, ref, ev, pop, _, setup = prepare(name)
    eng = setup(_oracle(sc.num_sites, steps + 8))
    tally, cov, watches, got = Tally("oracle"), M.Coverage(), {}, {}
    topo = name not in TOPOLOGY_OFF
    try:
        def on_step(p, s, b, a):
            if p not in watches:
                watches[p] = M.PartWatch(p, b, ref, ev, pop, incl[p], name)
                watches[p].t_max_tip, watches[p].topology = sc.t_max_tip, topo
            w = watches[p]
            before = copy.copy(w)
            M.check_step(tally, cov, w, s, b, a)
            row = a["row"]
            kind, node, acc, log_mh = int(row[0]), int(row[1]), row[2] == 1.0, float(row[3])
            st = DM.Step(before, b, a, kind, node, log_mh == log_mh, acc, log_mh, False, 32.0 if topo else 30.0, topo)
            for label, pred in wanted.items():
                if label not in got and pred(st):
                    got[label] = st
        M.step_chain(eng, parts_watched if parts_watched is not None else list(range(len(parts))), steps, on_step)
    finally:
        eng.close()
    assert not tally.fail and cov.unchecked == 0, tally.fail[:3]
    assert set(got) == set(wanted), sorted(set(wanted) - set(got))
    return got


def _holds(st):
    DM.check_reading(st, st.b["rng"], st.a["rng"], M.Coverage(), {})


def _refused(st, **changes):
    """The step with `changes` (attributes of the Step; `tree`: an edit of a copy of the tree after) must raise Mismatch."""
    st = copy.copy(st)
    edit = changes.pop("tree", None)
    for k, v in changes.items():
        setattr(st, k, v)
    if edit:
        st.a = dict(st.a, tree=copy.deepcopy(st.a["tree"]))
        edit(st.a["tree"])
    with pytest.raises(DM.Mismatch):
        _holds(st)


def _is_tip(st, x):
    return st.b["tree"].child0[x] < 0


def test_doctored_steps_are_refused():
    noted = lambda st: st.noted and st.acc

    def between(st):            # (in the cancellation regime the reference's own exp(ltr) - 1 hides a shift of 1e-9 of the window)
        T, n = st.w.dv.T, st.node
        a, b = DM.tip_window(T, st.b["tree"], n) if st.kind == 1 else DM.inner_window(T, n)
        return DM.bexp_class(-st.w.dv.lam[n] if st.kind == 1 else X.displacement_slope(st.w.dv, n), b - a) == 3
    got = _record("C1/6", None, 120, {
        "tip": lambda st: st.kind == 1 and noted(st) and between(st),
        "inner": lambda st: st.kind == 0 and noted(st) and st.node != st.w.dv.T.root and between(st),
        "drawn verdict": lambda st: st.kind <= 1 and st.noted and st.log_mh < -0.05,
        "reform": lambda st: st.kind == 2 and noted(st) and not (st.w.includes_root and st.w.dv.T.parent[st.node] == st.w.dv.T.root)
        and len({m[0] for m in st.w.dv.T.muts[st.node]}) >= 2,
        "spr1": lambda st: st.kind == 4 and noted(st),
        "exact tip": lambda st: st.kind == 1 and not st.noted,
    })
    for st in got.values():
        _holds(st)

    # the bounded exponential: moved by 1e-9 (b - a); drawn with a and b swapped; drawn from the neighbouring word
    for label in ("tip", "inner"):
        st = got[label]
        T, n = st.w.dv.T, st.node
        a, b = DM.tip_window(T, st.b["tree"], n) if label == "tip" else DM.inner_window(T, n)
        lam = -st.w.dv.lam[n] if label == "tip" else X.displacement_slope(st.w.dv, n)
        t_new = float(st.a["tree"].t[n])
        _refused(st, tree=lambda t: t.t.__setitem__(n, t_new + 1e-9 * float(b - a)))
        W = DM.Words(st.b["rng"])
        k = 1
        while _is_tip(st, DM.pick(W[k], T.n)) != (label == "tip"):
            k += 1
        assert DM.pick(W[k], T.n) == n
        with mp.workdps(60):
            v = DM.to_oo(W[k + 1])
            assert abs(X._mp(a) + DM.bexp_offset(v, lam, b - a) - t_new) < 1e-9 * float(b - a)            # (the word is the right one)
            swapped = float(X._mp(b) - DM.bexp_offset(v, -lam, b - a))                                    # the same draw on the window read from b down
            neighbour = float(X._mp(a) + DM.bexp_offset(DM.to_oo(W[k + 2]), lam, b - a))
        for other in (swapped, neighbour):
            assert abs(other - t_new) > 1e-6 * float(b - a)
            _refused(st, tree=lambda t, o=other: t.t.__setitem__(n, o))
        _refused(st, node=next(x for x in range(T.n) if x != n and _is_tip(st, x) == (label == "tip")))     # another node in the row
    # a pick off by one (whatever kind of node that is)
    _refused(got["tip"], node=got["tip"].node + (1 if got["tip"].node + 1 < got["tip"].w.dv.T.n else -1))
    # the verdict flipped
    st = got["drawn verdict"]
    _refused(st, acc=not st.acc)
    _refused(got["tip"], acc=False)
    # a row that is not noted says the drawn time landed on a bound: refused when the draw lies inside the window
    st = got["tip"]
    back = DM.index_of(st.a["rng"]) - int(st.log_mh < 0.0)
    _refused(st, noted=False, acc=False, log_mh=float("nan"), a=dict(st.a, rng=dict(st.a["rng"], counter=(back + 1) // 2, has_spare=bool(back & 1), spare=None)))
    # an exact-date tip must end un-noted, after its leading words
    _refused(got["exact tip"], noted=True, acc=True, log_mh=0.0)
    # two reform times exchanged between mutations of different sites
    st = got["reform"]
    lo = int(st.b["tree"].mut_offset[st.node])
    sites = st.a["tree"].mut_site[lo:int(st.b["tree"].mut_offset[st.node + 1])].tolist()
    j = next(i for i in range(1, len(sites)) if sites[i] != sites[0])

    def swap(t):
        t.mut_t[lo], t.mut_t[lo + j] = t.mut_t[lo + j], t.mut_t[lo]
    _refused(st, tree=swap)
    # the SPR1 time mirrored within its region
    st = got["spr1"]
    limit = M.scan_limit_from_stream(st.b["rng"])
    dvA = X.Derived(st.a["tree"], st.w.ref, st.w.ev)
    d = M.spr1_identity(st.w, st.node, dvA, limit)
    r = d["pre"].regions[d["new_region"]]
    assert not r.above_root
    for t_P, ok in ((d["ga"].t_P, True), (float(r.t_min + r.t_max - F(float(d["ga"].t_P))), False)):
        tally, cov = Tally("oracle"), M.Coverage()
        DM.check_spr1_time(tally, cov, st.w, st.node, dict(d, ga=SimpleNamespace(t_P=t_P)), limit, st.b["rng"], "doctored")
        assert (not tally.fail and cov.unchecked == 0) == ok, tally.fail
    tally, cov = Tally("oracle"), M.Coverage()
    DM.check_spr1_time(tally, cov, st.w, st.node, d, None if limit == 1 else 1, st.b["rng"], "doctored")       # the other scan limit
    assert tally.fail and cov.unchecked == 1


def test_doctored_slide_down_is_refused():
    """random8, part 3: the slide of its 19th move goes down past the sibling with four straddling branches to choose from."""
    got = _record("random8", [3], 19, {"down": lambda st: st.kind == 3 and st.noted and st.acc})
    st = got["down"]
    _holds(st)
    B = X._Tree(st.b["tree"])
    Xn, P = st.node, B.parent[st.node]
    new_S = [c for c in (int(st.a["tree"].child0[P]), int(st.a["tree"].child1[P])) if c != Xn][0]
    br = M.straddling_branches(B, P, F(float(st.a["tree"].t[P])), Xn)
    assert len(br) >= 2 and new_S in br
    other = next(v for v in br if v != new_S)

    def resibling(t):
        if t.child0[P] == new_S:
            t.child0[P] = other
        else:
            t.child1[P] = other
    _refused(st, tree=resibling)
    t_new = float(st.a["tree"].t[P])
    _refused(st, tree=lambda t: t.t.__setitem__(P, t_new + 1e-9))
    _refused(st, tree=lambda t: t.t.__setitem__(P, 2 * float(st.b["tree"].t[P]) - t_new))       # the step's sign flipped


def _moved_on(rng, words):
    """The stream position `words` words after `rng`."""
    at = DM.index_of(rng) + words
    return dict(rng, counter=(at + 1) // 2, has_spare=bool(at & 1), spare=None)


def test_doctored_root_displacement_is_refused():
    """The Gaussian step of an accepted displacement of the run's root (the steep case's first)."""
    st = _record("steep", None, 60, {"root": lambda st: st.kind == 0 and st.noted and st.acc and st.node == st.w.dv.T.root})["root"]
    _holds(st)
    T, n = st.w.dv.T, st.node
    old, t_new = float(st.b["tree"].t[n]), float(st.a["tree"].t[n])
    _refused(st, tree=lambda t: t.t.__setitem__(n, t_new + 1e-9))
    _refused(st, tree=lambda t: t.t.__setitem__(n, 2 * old - t_new))                            # the step's sign flipped
    W = DM.Words(st.b["rng"])
    k = 1
    while not T.kids[DM.pick(W[k], T.n)]:
        k += 1
    assert DM.pick(W[k], T.n) == n
    lo, hi = DM.inner_window(T, n)
    span = F(float(st.w.t_max_tip)) - hi
    own, _ = DM.gaussian_step(W[k + 1], W[k + 2], st.w.dv.lambda_i(n), span, 0)
    assert abs(float(own) - (t_new - old)) < 1e-9                                               # (the words are the right ones)
    for w1, w2 in ((W[k + 2], W[k + 3]), (W[k + 2], W[k + 1])):                                 # the neighbouring words; the two words exchanged
        other = old + float(DM.gaussian_step(w1, w2, st.w.dv.lambda_i(n), span, 0)[0])
        assert abs(other - t_new) > 1e-6
        _refused(st, tree=lambda t, o=other: t.t.__setitem__(n, o))
    _refused(st, acc=False)


def test_a_time_on_a_bound_ends_the_move_and_takes_no_acceptance_word():
    """The on-a-bound case's first tip displacement of the uncertain tip: un-noted after the pick's words and one more.  Refused: the same
    row after one word more (a clamp that ate the acceptance word) or one less, and the row noted."""
    st = _record("on-a-bound", None, 40, {"landed": lambda st: st.kind == 1 and not st.noted and st.b["tree"].t_min[st.node] != st.b["tree"].t_max[st.node]})["landed"]
    cov = M.Coverage()
    DM.check_reading(st, st.b["rng"], st.a["rng"], cov, {})
    assert cov.draws_early_end[5] == 1 and cov.draws_held == 1
    for extra in (1, -1):
        _refused(st, a=dict(st.a, rng=_moved_on(st.a["rng"], extra)))
    _refused(st, noted=True, acc=False, log_mh=-1.0)
