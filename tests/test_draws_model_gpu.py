"""What the HIP engine's moves draw, held to tests/draws_model.py: the cases of test_draws_model.py (test_move_steps.DRAW_CASES: a slope
steep enough for the bounded exponential's short spellings, a slope that is exactly zero, a window in which every drawn time lands on a
bound) through EmatBackend with the parts staged in
LDS and resident in HBM, and the zero-slope case through the run driver with the tree resident in HBM.  Every other stepped case of the
device goes through the same identities in test_move_steps_gpu.py and test_study_model_gpu.py (move_steps.check_step calls the model).
The conditions are the oracle's, test_draws_model.assert_draw_case_conditions."""
import pytest

import delphy_amd as d
import exact_model as X
import move_steps as M
from test_draws_model import assert_draw_case_conditions
from test_exact_model import Tally
from test_move_steps import DRAW_CASES, run_case, zero_slope_scenario

pytestmark = pytest.mark.gpu

_done = {}


def _device(use_lds):
    return lambda num_sites, trace: d.EmatBackend(num_sites, trace_moves=trace, use_lds=use_lds)


def _run(name, use_lds):
    if (name, use_lds) not in _done:
        _done[(name, use_lds)] = run_case(name, _device(use_lds), "device")
    return _done[(name, use_lds)]


@pytest.mark.parametrize("use_lds", [True, False])
@pytest.mark.parametrize("name", DRAW_CASES)
def test_device_draw_cases(name, use_lds, record_property):
    tally, cov = _run(name, use_lds)
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    tally.finish(record_property)
    assert cov.unchecked == 0 and cov.borderline == 0, cov.as_dict()


@pytest.mark.parametrize("use_lds", [True, False])
def test_device_draw_cases_cover_what_they_must(use_lds, record_property):
    assert_draw_case_conditions({name: _run(name, use_lds) for name in DRAW_CASES}, record_property)


def test_device_tree_resident_in_hbm_zero_slope(record_property):
    """The zero-slope case through the run driver, the tree resident in HBM and its one part cut by kernels: 200 single-move passes."""
    sc = zero_slope_scenario()
    ev, pop = X.Evo.of(sc), X.Pop(sc.pop)
    b = d.EmatBackend(sc.num_sites, trace_moves=256)
    run = d.EmatRun(b, sc.tree, sc.ref, 3)
    run.set_num_parts(1); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_coalescent_t_step(1.0)
    run.set_device_tree(True)
    tally, cov = Tally("device"), M.Coverage()
    try:
        _, ref = run.tree()
        run.repartition()
        n, root_part = run.num_parts()

        def advance(e):
            run.run_moves(n); e.synchronize()
        M.run_stepped(tally, cov, b, sc, list(range(n)), [p == root_part for p in range(n)], ref, ev, pop, 200, tag="hbm tree, zero slope", advance=advance)
    finally:
        run.close(); b.close()
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    tally.finish(record_property)
    assert cov.unchecked == 0 and cov.borderline == 0 and cov.position_half_known == 0 and cov.draws_held == cov.steps, cov.as_dict()
    assert cov.draws_bexp[4] >= 1 and cov.draws_gaussian_root >= 1, cov.as_dict()
