"""tests/skygrid_moves_model.py checked against itself and against the reference's own expectations: the gradient of the Skygrid curve at the
tolerances the reference's tests state (as data, tests/golden/skygrid_gradient_expectations.json), the model's force against the central
difference of the model's own U at 60 digits, and sum_k W_k gamma_k against the node-by-node sum of log N(t_i), exactly.  No GPU."""
import json
import math
import os
from fractions import Fraction as F

import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import skygrid_moves_model as SM

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skygrid_gradient_expectations.json")))


@pytest.mark.parametrize("name", ["staircase", "log_linear"])
def test_the_model_meets_the_references_expectations_of_the_gradient(name):
    pm = d.PopModel.skygrid(GOLDEN["knots_x"], GOLDEN["knots_gamma"], name == "log_linear")
    pop = X.Pop(pm)
    m = GOLDEN["models"][name]
    assert len(m["d_log_N_d_gamma"]) == 44 and len(m["support_of_d_log_N_d_gamma"]) == 4 and len(m["d_log_int_N_d_gamma"]) == (36 if name == "staircase" else 32)
    for e in m["d_log_N_d_gamma"]:
        assert abs(float(SM.d_log_N_d_gamma(pop, e["t"], e["k"])) - e["expected"]) <= e["tol"], e
    for e in m["support_of_d_log_N_d_gamma"]:
        lo, hi = SM.support_of_d_log_N_d_gamma(pop, e["k"])
        assert (lo == float(e["lo"]) or abs(lo - float(e["lo"])) <= e["tol"]) and (hi == float(e["hi"]) or abs(hi - float(e["hi"])) <= e["tol"]), e
    for e in m["d_log_int_N_d_gamma"]:
        ex, allowance = SM.d_log_int_N_d_gamma(pop, e["a"], e["b"], e["k"])
        assert allowance == 0.0 and abs(ex.f - e["expected"]) <= e["tol"], (e, ex)


def _small_cases():
    return [SM.make_case("2 knots", 2, 8, 5, True), SM.make_case("12 knots stair", 12, 9, 7, False), SM.make_case("12 knots", 12, 9, 7, True),
            SM.make_case("before", 3, 8, 4, True, layout="before"), SM.make_case("after", 3, 8, 4, False, layout="after"),
            SM.make_case("on", 5, 16, 9, True, layout="on"), SM.make_case("dozens of knots a cell", 40, 1, 3, True)]


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: c[0])
def test_the_models_force_is_the_central_difference_of_its_own_U(case):
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    pop = X.Pop(pm)
    grid = SM.Grid(t_ref, t_step, first_cell, k_bar)
    ns = SM.NodeStats(pop, inner_t)
    tau = spec.tau
    # away from the barrier's kink and from equal gammas' removable point the derivative is smooth: h = 1e-20 leaves h^2 = 1e-40 relative
    f = SM.force(pop, grid, ns, tau, spec)
    h = F(1, 10 ** 20)
    for k in range(len(pop.gamma)):
        up = list(pop.gamma); up[k] += h
        dn = list(pop.gamma); dn[k] -= h
        cd = -(SM.U_total(SM.pop_with_gammas(pop, up), grid, ns, tau, spec) - SM.U_total(SM.pop_with_gammas(pop, dn), grid, ns, tau, spec)) / (2 * h)
        scale = max(abs(f[k][0].value), F(1))
        assert abs(cd - f[k][0].value) <= scale * F(1, 10 ** 30), (k, float(cd), f[k][0])


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: c[0])
def test_the_knot_sums_equal_the_node_by_node_sum_exactly(case):
    _, pm, spec, t_ref, t_step, first_cell, k_bar, inner_t = case
    pop = X.Pop(pm)
    ns = SM.NodeStats(pop, inner_t); c, W = ns.c, ns.W
    assert sum(c) == len(inner_t)
    assert sum((w * g for w, g in zip(W, pop.gamma)), F(0)) == SM.sum_log_N_node_by_node(pop, inner_t)
    assert sum(W, F(0)) == len(inner_t)          # every node's gradient sums to 1 over the knots
    assert SM.force(pop, grid := SM.Grid(t_ref, t_step, first_cell, k_bar), ns, spec.tau, spec, knots=[0])[0][0].value == SM.force(pop, grid, ns, spec.tau, spec)[0][0].value
