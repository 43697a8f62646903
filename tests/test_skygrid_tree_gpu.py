"""The Skygrid moves' statistics from the tree resident in HBM (emat_tree_coalescent_stats) and the moves on them (emat_tree_skygrid_moves): the
lineage grid against exact_model's, the inner nodes' times bit for bit, the state rule of the tree probers, and the moves bit for bit those of
emat_skygrid_moves fed the downloaded statistics."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
from delphy_amd.scenarios import make_scenario
from exact_model import Exact
from test_exact_model import Tally

pytestmark = pytest.mark.gpu


def _exact_grid(tree, t_ref, t_step):
    """exact_model's whole-tree grid (scalable_log_prior's): (first cell, [Exact k_bar])."""
    T = X._Tree(tree)
    tr, ts = X._fl(t_ref), X._fl(t_step)
    cell = lambda t: X._floor((t - tr) / ts)
    c0, c1 = cell(T.t[T.root]), cell(max(T.t))
    iv = X._lineage_intervals(T) + [(tr + c0 * ts, T.t[T.root])]
    kb, kS, kn = X._grid(iv, cell, lambda c: tr + c * ts, lambda c: tr + (c + 1) * ts, c0, c1, ts, lambda c: abs(tr) + abs((c + 1) * ts))
    return c0, c1, [Exact(v, S, n) for v, S, n in zip(kb, kS, kn)]


def _scenario(tips):
    return make_scenario("C3", num_tips=tips, num_sites=600, uncertain_tips=0.2)


@pytest.mark.parametrize("tips", [2, 33, 600])
@pytest.mark.parametrize("cells", [1, 7, 400])
def test_the_trees_statistics_against_the_exact_grid(tips, cells, record_property):
    sc = _scenario(tips)
    t = np.asarray(sc.tree.t); inner = np.asarray(sc.tree.child0) >= 0
    t_ref = float(t.max()) + 0.125
    t_step = (t_ref - float(t[sc.tree.root])) / (cells - 0.5) if cells > 1 else 4.0 * (t_ref - float(t.min()))
    b = d.EmatBackend(sc.num_sites)
    tally = Tally("device")
    try:
        b.tree_upload(sc.tree)
        first, k_bar, inner_t = b.tree_coalescent_stats(t_ref, t_step)
        c0, c1, exact = _exact_grid(sc.tree, t_ref, t_step)
        assert first == c0 and len(k_bar) == c1 - c0 + 1 == len(exact)          # from the root's cell to the latest tip's
        assert first == int(np.floor((t[sc.tree.root] - t_ref) / t_step)) and first + len(k_bar) - 1 == int(np.floor((t[~inner].max() - t_ref) / t_step))
        for c, ex in enumerate(exact):
            tally.check("k_bar", ex, k_bar[c], "%d tips cell %d" % (tips, c))
        assert np.array_equal(inner_t, t[inner])                                 # node order, bit for bit
        again = b.tree_coalescent_stats(t_ref, t_step)
        assert again[0] == first and np.array_equal(again[1], k_bar) and np.array_equal(again[2], inner_t)
    finally:
        b.close()
    tally.finish(record_property)


def _curve(sc, log_linear):
    t = np.asarray(sc.tree.t)
    x = np.linspace(t.min() - 1.0, t.max(), 9)
    return d.PopModel.skygrid(x, 4.0 + 0.5 * np.sin(np.arange(9.0)), log_linear)


@pytest.mark.parametrize("tips", [2, 33, 600])
def test_the_moves_on_the_trees_statistics_are_the_moves_on_their_download(tips):
    sc = _scenario(tips)
    t = np.asarray(sc.tree.t)
    t_ref = float(t.max()); t_step = max((t_ref - float(t.min())) / 37.0, 1e-3)
    spec = d.SkygridSpec(tau=1.5, low_gamma_barrier_enabled=True)
    b, other = d.EmatBackend(sc.num_sites), d.EmatBackend(sc.num_sites)
    try:
        b.tree_upload(sc.tree); other.tree_upload(sc.tree)
        for log_linear in (False, True):
            pm = _curve(sc, log_linear)
            first, k_bar, inner_t = b.tree_coalescent_stats(t_ref, t_step)
            want = b.skygrid_moves(pm, spec, t_ref, t_step, first, k_bar, inner_t, key=9, trace=True)
            for got in (b.tree_skygrid_moves(pm, spec, t_ref, t_step, key=9, trace=True), b.tree_skygrid_moves(pm, spec, t_ref, t_step, key=9, trace=True),
                        other.tree_skygrid_moves(pm, spec, t_ref, t_step, key=9, trace=True)):
                assert np.array_equal(got.gamma, want.gamma) and np.array_equal(got.trace, want.trace, equal_nan=True)
                for f in ("tau", "log_coalescent_prior_start", "log_coalescent_prior_end", "delta_log_other_priors", "zero_B", "zero_I_bar", "hmc_K_new", "hmc_log_metropolis",
                          "hmc_accepted", "hmc_steps_done", "hmc_K_exit_step"):
                    assert getattr(got, f) == getattr(want, f), f
            assert want.hmc_steps_done >= 1 and not np.array_equal(want.gamma, pm.skygrid_gamma)
    finally:
        b.close(); other.close()


def test_the_state_rule_and_the_refusals():
    sc = _scenario(600)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 3)
    pm = _curve(sc, True); spec = d.SkygridSpec()
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            b.tree_coalescent_stats(0.0, 1.0)                                    # no tree uploaded
        run.set_num_parts(8); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
        run.repartition()
        with pytest.raises(d.EmatError, match="STATE.*parts are out"):
            b.tree_coalescent_stats(0.0, 1.0)
        with pytest.raises(d.EmatError, match="STATE.*parts are out"):
            b.tree_skygrid_moves(pm, spec, 0.0, 1.0)
        run.reassemble()
        first, k_bar, inner_t = b.tree_coalescent_stats(float(np.asarray(sc.tree.t).max()), 5.0)
        assert len(inner_t) == 599 and k_bar[0] >= 1.0
        for bad in ((float("nan"), 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, float("inf"))):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*t_step"):
                b.tree_coalescent_stats(*bad)
        with pytest.raises(d.EmatError, match="CAPACITY.*cells"):
            b.tree_coalescent_stats(0.0, 1e-9)
        import ctypes as C
        fc, nc, ni = C.c_int32(), C.c_int32(), C.c_int32(); kb = np.zeros(2)
        assert b._lib.emat_tree_coalescent_stats(b._h, 0.0, 5.0, C.byref(fc), C.byref(nc), kb.ctypes.data_as(C.POINTER(C.c_double)), 2, None, 0, C.byref(ni)) == 7   # EMAT_ERR_BUFFER_TOO_SMALL
        assert nc.value > 2 and ni.value == 599
    finally:
        run.close(); b.close()
