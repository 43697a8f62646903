"""tests/exp_pop_moves_model.py against what it restates: its whole-tree prior equals exact_model.scalable_log_prior on a small tree, the
Exponential model's integral pieces at the barrier against mpmath quadrature, the stopgap, and the steps' lines against a direct evaluation.  No GPU."""
import math
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import exp_pop_moves_model as EM
from delphy_amd.scenarios import make_scenario
from skygrid_moves_model import Grid


def _tree_grid(tree, t_ref, t_step):
    """exact_model's whole-tree grid as a Grid holding the EXACT k_bar (Fractions), and the inner nodes' times."""
    T = X._Tree(tree)
    tr, ts = X._fl(t_ref), X._fl(t_step)
    cell = lambda t: X._floor((t - tr) / ts)
    c0, c1 = cell(T.t[T.root]), cell(max(T.t))
    iv = X._lineage_intervals(T) + [(tr + c0 * ts, T.t[T.root])]
    kb, _, _ = X._grid(iv, cell, lambda c: tr + c * ts, lambda c: tr + (c + 1) * ts, c0, c1, ts, lambda c: abs(tr) + abs((c + 1) * ts))
    grid = Grid(t_ref, t_step, c0, [0.0] * len(kb))
    grid.k_bar = kb
    t = np.asarray(tree.t); inner = np.asarray(tree.child0) >= 0
    return grid, t[inner]


@pytest.fixture(scope="module")
def small_tree():
    return make_scenario("C3", num_tips=24, num_sites=200, uncertain_tips=0.2).tree


@pytest.mark.parametrize("g_span,min_pop", [(0.0, 0.0), (3.0, 0.0), (-2.0, 0.0), (3.0, 2.5), (-2.0, 2.5), (0.0, 5.0)])
def test_the_models_prior_is_exact_models_on_a_small_tree(small_tree, g_span, min_pop):
    """g_span: the growth over the tree's whole span, g (t_max - t_min); t0 lies inside the tree, so the barrier starts inside it too."""
    tree = small_tree
    t = np.asarray(tree.t)
    t_ref = float(t.max()); span = t_ref - float(t.min()); t_step = span / 9.0
    pm = d.PopModel.exp(t_ref - 0.4 * span, 3.0, g_span / span, min_pop)
    want = X.scalable_log_prior(tree, X.Pop(pm), t_ref, t_step)
    grid, inner_t = _tree_grid(tree, t_ref, t_step)
    got = EM.log_coalescent_prior(X.Pop(pm), grid, inner_t)
    assert abs(got.value - want.value) < F(1, 10 ** 55) * max(1, abs(want.value))      # (the model rounds its terms to 2^-260)
    assert got.S > 0 and math.isfinite(float(got.S)) and got.n >= len(inner_t)


@pytest.mark.parametrize("g", [0.37, -0.37, 2.5, -1e-3])
def test_pop_integral_pieces_at_the_clamp_against_quadrature(g):
    t0, n0, mp = 100.0, 50.0, 7.0
    pop = EM.exp_pop(t0, n0, g, mp)
    tc = float(pop.t_c)
    N = lambda t: max(mpmath.mpf(mp), mpmath.mpf(n0) * mpmath.exp(mpmath.mpf(g) * (t - mpmath.mpf(t0))))
    with mpmath.workdps(40):
        for a, b in ((tc - 1.0, tc + 1.0), (tc, tc + 0.5), (tc - 0.5, tc), (tc - 2.0, tc - 1.0), (tc + 1.0, tc + 2.0), (tc - 1e-9, tc + 1e-9), (tc - 3.0, tc + 1e-12)):
            I = pop.pop_integral(a, b)
            want = mpmath.quad(N, [mpmath.mpf(a), X._mp(pop.t_c), mpmath.mpf(b)] if a < tc < b else [mpmath.mpf(a), mpmath.mpf(b)])
            assert abs(X._mp(I.value) - want) <= mpmath.mpf(10) ** -25 * max(1, abs(want)), (g, a, b)
            assert I.S >= abs(I.value)


def test_the_stopgap_and_cells_without_a_term():
    """g = 50 and a cell 20 before t0: the cell's integral is far below the smallest double, the reference puts 1e-100 there."""
    grid = Grid(1000.0, 0.25, -80, [2.0] + [0.0] * 40 + [1.0] * 38 + [3.0])
    pop = EM.exp_pop(1000.0, 3.0, 50.0, 0.0)
    inner_t = [999.9]
    got = EM.log_coalescent_prior(pop, grid, inner_t)
    N_last, _, _ = grid.popsize_bar(pop, 79)
    want = -F(0.25) * 2 * 1 / (2 * F(1e-100)) - F(0.25) * 3 * 2 / (2 * N_last) + pop.neg_log_pop(X._fl(999.9))[0]
    assert abs(got.value - want) < abs(want) * F(1, 10 ** 50)
    assert math.isfinite(got.f) and got.f < -1e99


def test_the_steps_lines_against_a_direct_evaluation():
    with mpmath.workdps(50):
        u0, old = 0.3125, 2.75
        new, ratio, hastings = EM.n0_step(old, u0, 0.7, 1.3)
        s = mpmath.mpf(3) / 4 + (mpmath.mpf(4) / 3 - mpmath.mpf(3) / 4) * u0
        assert abs(X._mp(new.value) - s * old) < 1e-40 and 0.75 * old <= new.f < old / 0.75
        assert abs(X._mp(ratio.value) - (-(0.7 + 1) * mpmath.log(s) - mpmath.mpf(1.3) * (1 / (s * old) - 1 / mpmath.mpf(old)))) < 1e-40
        assert abs(X._mp(hastings.value) + mpmath.log(s)) < 1e-40
        new_g, ratio_g = EM.g_step(0.001, u0, 0.02, 0.4)
        dg = -mpmath.mpf(1) / 365 + 2 * mpmath.mpf(1) / 365 * u0
        assert abs(X._mp(new_g.value) - (mpmath.mpf(0.001) + dg)) < 1e-40
        assert abs(X._mp(ratio_g.value) - (abs(mpmath.mpf(0.001) - mpmath.mpf(0.02)) - abs(mpmath.mpf(0.001) + dg - mpmath.mpf(0.02))) / mpmath.mpf(0.4)) < 1e-40
    # a float64 evaluation in the reference's order lies within each line's bound
    scale = 0.75 + (1 / 0.75 - 0.75) * u0
    assert new.ok(scale * old) and hastings.ok(math.log(old / (scale * old)))
    assert ratio.ok(-(0.7 + 1) * math.log(scale) - 1.3 * (1.0 / (scale * old) - 1.0 / old))
    assert new_g.ok(0.001 + (-1.0 / 365.0 + 2 * (1.0 / 365.0) * u0))
    a, b = X.Exact(F(-10), 12, 30), X.Exact(F(-11), 13, 30)
    lm = EM.log_metropolis(a, b, ratio, hastings)
    assert lm.value == 1 + ratio.value + hastings.value and lm.bound() >= a.bound() + b.bound() + ratio.bound() + hastings.bound()


def test_make_case_puts_t_c_where_asked():
    for t_c in (998.5, 998.6, 1003.0, 900.0):
        for g in (0.4, -0.4):
            _, pm, _, t_ref, t_step, first_cell, k_bar, inner_t = EM.make_case("", 40, 65, g, t_c=t_c)
            assert pm.p[0] + math.log(pm.p[3] / pm.p[1]) / pm.p[2] == t_c and pm.p[3] > 0
            assert len(k_bar) == 40 and len(inner_t) == 65 and np.all(inner_t < t_ref) and np.all(inner_t >= t_ref + first_cell * t_step)
