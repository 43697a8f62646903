"""tests/prober_model.py -- the Python restatement of the reference's tree probers that the device is measured against --
reproduces every expectation of the reference's own unit tests (tests/golden/prober_expectations.json: staircase_tests.cpp,
tree_prober_tests.cpp, ancestral_tree_prober_tests.cpp, site_states_tree_prober_tests.cpp), each at the tolerance the
reference's matcher states.  No GPU."""
import numpy as np
import pytest

import prober_model as M
from prober_golden import G, check_prober_case, check_tree_prober_case, flat_tree, pop_model


@pytest.mark.parametrize("case", G["staircase"], ids=lambda c: c["test"])
def test_staircase_cases_of_the_reference(case):
    s, checked = None, 0
    for st in case["steps"]:
        if st["op"] == "new":
            s = M.Staircase(st["x_start"], st["x_end"], st["num_cells"])
        elif st["op"] == "add_boxcar":
            M.add_boxcar(s, *st["args"])
        elif st["op"] == "add_trapezoid":
            M.add_trapezoid(s, *st["args"])
        else:
            assert abs(s.f[st["cell"]] - st["value"]) <= st["tol"], (st, s.f)
            checked += 1
    assert checked >= 3


def test_staircase_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError):
        M.Staircase(0.0, 0.0, 1)
    with pytest.raises(ValueError):
        M.Staircase(0.0, 1.0, 0)
    s = M.Staircase(0.0, 10.0, 10)
    with pytest.raises(ValueError):
        M.add_boxcar(s, 0.0, -4.0, 0.0)
    with pytest.raises(ValueError):
        M.add_trapezoid(s, 0.0, -4.0, 0.0, 0.0)
    M.add_boxcar(s, 0.0, 0.0, 0.0); M.add_trapezoid(s, 0.0, 0.0, 0.0, 0.0)      # empty: no complaint
    assert list(s.f) == [0.0] * 10


@pytest.mark.parametrize("case", G["tree_prober"], ids=lambda c: c["test"])
def test_tree_prober_cases_of_the_reference(case):
    fam = M.StaircaseFamily(case["num_cats"], case["t_start"], case["t_end"], case["num_cells"])
    for b in case["boxcars"]:
        M.add_boxcar(fam[b["member"]], *b["args"])
    p = M.tree_prober(fam, case["cells_to_skip"], M.OraclePop(pop_model(case["pop"])), case["p_initial"])
    check_tree_prober_case(case, p, case["test"])


def test_tree_prober_refuses_bad_starting_probabilities():
    fam = M.StaircaseFamily(2, 0.0, 10.0, 10)
    pop = M.OraclePop(pop_model({"kind": "const", "pop": 0.2}))
    with pytest.raises(ValueError):
        M.tree_prober(fam, 0, pop, [0.0, 0.0, 0.0])
    with pytest.raises(IndexError):
        M.tree_prober(fam, 0, pop, [-0.3, -0.2])
    with pytest.raises(IndexError):
        M.tree_prober(fam, 0, pop, [0.6, 0.7])


@pytest.mark.parametrize("case", G["ancestral_tree_prober"]["cases"], ids=lambda c: c["test"])
def test_ancestral_prober_cases_of_the_reference(case):
    A = G["ancestral_tree_prober"]
    tree, _ = flat_tree(A["tree"])
    for name in case["pops"]:
        p = M.probe_ancestors_on_tree(tree, M.OraclePop(pop_model(A["pops"][name])), case["marked"], case["t_start"], case["t_end"], case["num_t_cells"])
        assert p.shape[0] == len(case["marked"]) + 1
        check_prober_case(case, p, "%s / %s" % (case["test"], name))
        assert np.all(np.abs(p.sum(axis=0) - 1.0) <= 1e-12)       # with the "none" member the k + 1 probabilities are a partition
    with pytest.raises(IndexError):
        M.probe_ancestors_on_tree(tree, None, [tree.num_nodes + 10], -1.0, 3.0, 20)
    with pytest.raises(ValueError):
        M.probe_ancestors_on_tree(tree, None, [0], -3.5, -4.5, 10)


@pytest.mark.parametrize("case", G["site_states_tree_prober"], ids=lambda c: c["test"])
def test_site_state_prober_cases_of_the_reference(case):
    tree, ref = flat_tree(case["tree"])
    p = M.probe_site_states_on_tree(tree, ref, M.OraclePop(pop_model(case["pop"])), case["site"], case["t_start"], case["t_end"], case["num_t_cells"])
    check_prober_case(case, p, case["test"])
    for site in (-1, 5):
        with pytest.raises(IndexError):
            M.probe_site_states_on_tree(tree, ref, None, site, 0.0, 1.0, 10)
