"""The remembered missation rate change of every node (emat_slab.hpp: one double beside each node record, "not known" until a move
asks for it, put back to "not known" by whatever writes the node's missation lists) against a fresh evaluation on the lists as they
stand after passes of the full move mix: emat_debug_miss_dl_check counts, per part, the entries that are known and differ in BITS from
what delta_lambda_across_missations gives now.  That count must be 0 everywhere -- a missing invalidation shows up here even where the
chain has not yet read the stale value -- and a good share of the entries must be known, or the check would hold for a memo nobody uses.

The share asked for: an inner-node displacement (about a fifth of the moves) asks for both children of an inner node drawn uniformly, so
after thousands of moves on parts of tens of nodes every node but the part's root has been asked for many times over, and the only
entries not known are the root's and those of the handful of nodes the last topology moves (one move in sixteen) touched since: half of
all nodes is far below that and far above nothing."""
import ctypes as C

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from helpers import configure, split_parts

pytestmark = pytest.mark.gpu

MIN_KNOWN_SHARE = 0.5


def _check(b, num_nodes, what):
    """emat_debug_miss_dl_check on a settled handle: no known entry differs, half of all entries are known.  Returns (bad, known) per part."""
    n = len(num_nodes)
    lib = d.load_library()
    lib.emat_debug_miss_dl_check.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.emat_debug_miss_dl_check.restype = C.c_int
    out = np.zeros(2 * n, np.int32)
    assert lib.emat_debug_miss_dl_check(b.handle, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0, b.last_error()
    bad, known = out[0::2], out[1::2]
    print("%s: known %d of %d nodes in %d parts, stale %d" % (what, int(known.sum()), int(np.sum(num_nodes)), n, int(bad.sum())))
    assert np.all(known <= np.asarray(num_nodes)), what
    assert np.all(bad == 0), "%s: parts with stale remembered values: %s" % (what, {int(p): int(bad[p]) for p in np.nonzero(bad)[0]})
    assert known.sum() >= MIN_KNOWN_SHARE * np.sum(num_nodes), "%s: only %d of %d entries known" % (what, int(known.sum()), int(np.sum(num_nodes)))
    return bad, known


def _variant_counts(b):
    lib = d.load_library()
    lib.emat_debug_variant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)()
    assert lib.emat_debug_variant_counts(b.handle, out) == 0
    return list(out)


def _passes(sc, num_parts, moves, seed, what, passes=2, use_lds=True, t_step=None, want_variant=None):
    parts, incl, seeds, root_part, ref = split_parts(sc, num_parts, seed)
    nodes = [p.num_nodes for p in parts]
    b = d.EmatBackend(sc.num_sites, use_lds=use_lds)
    try:
        configure(b, sc, ref, parts, incl, seeds, root_part, t_step)
        counts = _variant_counts(b)
        if want_variant is not None and counts[want_variant] == 0:
            return None
        for k in range(passes):
            b.run_moves_per_part(moves); b.synchronize()
            assert all(b.part_stats(p)["status"] == 0 and b.part_stats(p)["moves_done"] == (k + 1) * moves for p in range(len(parts))), b.last_error()
            bad, known = _check(b, nodes, "%s, pass %d, variants %s" % (what, k, counts))
            assert known[root_part] > 0, "%s: nothing remembered in the part that holds the run's root" % what
        st = [b.part_stats(p) for p in range(len(parts))]
        assert sum(s["accepted"][3] + s["accepted"][4] for s in st) > 0, "%s: no topology move was accepted" % what
        return b.main_class_mask(len(parts)), b.part_coalescent(root_part)["k_bar_p"].shape[0]
    finally:
        b.close()


@pytest.mark.parametrize("size", ["C1", "C2"])
def test_remembered_values_in_parts_staged_whole_by_prefix_and_hbm_resident(monkeypatch, size):
    """C1- and C2-sized scenarios, with the staging area capped until each code variant -- whole slab in LDS, fixed-size prefix in LDS,
    everything in HBM -- has run the parts (the decision is the kernel's own, mirrored by emat_debug_variant_counts), and with staging off."""
    if size == "C1":
        sc, nparts = make_scenario("C1", num_tips=120, num_sites=4000, uncertain_tips=0.3), 4
    else:
        sc, nparts = make_scenario("C2", num_tips=400, num_sites=4000, uncertain_tips=0.2), 12
    seen = set()
    for cap in (None, 32768, 16384, 12288, 10240, 8192, 6144, 4096, 2048, 512):
        if cap is None:
            monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
        else:
            monkeypatch.setenv("EMAT_LDS_MAX", str(cap))
        for v in range(3):
            if v not in seen and _passes(sc, nparts, 3000, 23, "%s cap %s variant %d" % (size, cap, v), want_variant=v) is not None:
                seen.add(v)
    assert seen == {0, 1, 2}, "staging caps tried do not exercise every variant: %s" % seen
    monkeypatch.delenv("EMAT_LDS_MAX", raising=False)
    _passes(sc, nparts, 3000, 23, size + " staging off", use_lds=False)


def test_remembered_values_in_the_side_launches():
    """Parts whose prefix does not fit the main class's staging area run in k_run_moves_side, on streams of their own."""
    sc = make_scenario("C3", num_tips=1500, num_sites=12000, uncertain_tips=0.1)
    main, _ = _passes(sc, 40, 2500, 9, "side classes")
    assert not np.all(main), "no part ran in a side launch"


def test_remembered_values_survive_a_pass_interrupted_to_regrow_the_root_grid():
    """The root part outgrows its coalescent grid in mid-pass, every part is re-encoded with what the moves maintain carried over
    (PartHost::kept_*), the remembered values among it, and the rest of the pass runs on them."""
    import delphy_amd.engine as e
    from delphy_amd.scenarios import Scenario, KAPPA, PI
    par = e.SynthParams(num_tips=120, num_sites=60, tip_span=30.0, pop_n0=400.0, pop_growth=0.0, mu=2e-5, gaps_per_tip=1, mean_gap_len=4.0, seed=3)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, tmax = e.make_synthetic_emat(par)
    sc = Scenario("deep-root", tree, ref, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, 400.0, 0.0, 0.0), 60)
    t_step = sc.default_t_step() * 0.25
    parts, incl, seeds, root_part, ref2 = split_parts(sc, 5, 7)
    b = d.EmatBackend(sc.num_sites)
    try:
        configure(b, sc, ref2, parts, incl, seeds, root_part, t_step)
        cells0 = b.part_coalescent(root_part)["k_bar_p"].shape[0]
    finally:
        b.close()
    _, cells1 = _passes(sc, 5, 4000, 7, "regrown grid", passes=1, t_step=t_step)
    assert cells1 > cells0 + max(512, cells0), "the root part's grid did not outgrow its slab (%d -> %d cells): the case no longer interrupts a pass" % (cells0, cells1)


def test_remembered_values_in_parts_cut_on_the_device():
    """The tree resident in HBM: the parts' slabs are written by the cutter kernel, which starts every entry as not known."""
    sc = make_scenario("C1", num_tips=300, num_sites=3000, uncertain_tips=0.2)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 3)
    run.set_num_parts(8); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop)
    run.set_device_tree(True)
    try:
        for cyc in range(2):
            run.repartition()
            n, _ = run.num_parts()
            nodes = [b.part_download(p).num_nodes for p in range(n)]
            run.run_moves(n * 2000); b.synchronize()
            _check(b, nodes, "device-cut parts, cycle %d" % cyc)
            run.reassemble()
    finally:
        run.close(); b.close()
