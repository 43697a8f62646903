"""The branch reform's register path (emat_device_moves.hpp: branch_reform_small<N>, N = 1..4 mutations at N different sites) and the
general path beside it (five mutations or more, or a site twice on the branch) against the oracle, on the 100-tip C1 tree with its 30 000
sites, cut into five parts.  Its branches carry 0 / 1 / 2 / 3 / 4 / 5 or more mutations on 62 / 38 / 33 / 12 / 14 / 40 of them and none
carries a site twice.

With the topology moves off no list changes its length, so the class of every reform in a trace is read from the tree the pass started
from.  What the scenario covers is asserted from the oracle's trace and that tree alone, before anything of the device's is looked at.
A reform of this tree is almost never rejected (its log MH ratio is of the order of -1e-5): the split seed is one of the few under which
the oracle's 200 moves per part hold a rejected short reform -- found by running the oracle over seeds, the device had no say in it.
The oracle runs once per setting (module cache); every device run is compared with that."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from helpers import assert_traces_match, assert_trees_match, configure, split_parts
from oracle_ffi import OracleEngine

pytestmark = pytest.mark.gpu

NPARTS, MOVES, SEED = 5, 200, 22447
K_REFORM = 2   # the move's kind in a trace row (kind, node, accepted, log MH ratio)
TREE_FIELDS = ("parent", "child0", "child1", "t", "t_min", "t_max", "mut_offset", "mut_site", "mut_from", "mut_to", "mut_t", "miss_offset", "miss_start", "miss_end",
               "mfs_offset", "mfs_site", "mfs_state")


@functools.lru_cache(maxsize=None)
def _scenario():
    sc = make_scenario("C1", num_tips=100)
    return sc, split_parts(sc, NPARTS, SEED)


@functools.lru_cache(maxsize=None)
def _site_rates():
    """Relative site rates that are not all one: every other site keeps exactly 1.0 (its log(mu q_ab) comes from the staged table), the
    rest lie in [0.2, 2) (theirs from the logarithm)."""
    sc, _ = _scenario()
    nu = 0.2 + 1.8 * np.random.default_rng(4711).random(sc.num_sites)
    nu[::2] = 1.0
    return nu


def _run_oracle(sc, split, topology, nu_l):
    parts, incl, seeds, root_part, ref = split
    orc = OracleEngine(sc.num_sites, trace_moves=MOVES)
    try:
        configure(orc, sc, ref, parts, incl, seeds, root_part, topology=topology, nu_l=nu_l)
        orc.run_moves_per_part(MOVES, threads=4)
        return [dict(trace=orc.part_trace(p, MOVES).copy(), stats=orc.part_stats(p), tree=orc.part_download(p)) for p in range(len(parts))]
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def _oracle(topology=False, site_rates=False):
    sc, split = _scenario()
    return _run_oracle(sc, split, topology, _site_rates() if site_rates else None)


def _variant_counts(b):
    lib = d.load_library()
    lib.emat_debug_variant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)()
    assert lib.emat_debug_variant_counts(b.handle, out) == 0
    return list(out)   # parts staged whole, by prefix, not at all


def _run_device(sc, split, topology, nu_l, options=(), use_lds=True, want_variant=None):
    """One pass on the device.  Per part (trace, stats, tree), and how the parts ran: (variant counts, main-launch mask).  None when
    `want_variant` is asked for and these options put no part in it."""
    parts, incl, seeds, root_part, ref = split
    b = d.EmatBackend(sc.num_sites, trace_moves=MOVES, use_lds=use_lds)
    try:
        for k, v in options:
            b.set_option(k, v)
        configure(b, sc, ref, parts, incl, seeds, root_part, topology=topology, nu_l=nu_l)
        counts = _variant_counts(b)
        if want_variant is not None and counts[want_variant] == 0:
            return None
        b.run_moves_per_part(MOVES); b.synchronize()
        out = []
        for p in range(len(parts)):
            st = b.part_stats(p)
            assert st["status"] == 0, "part %d: device status %d: %s" % (p, st["status"], b.last_error())
            out.append(dict(trace=b.part_trace(p, MOVES).copy(), stats=st, tree=b.part_download(p)))
        return out, (counts, b.main_class_mask(len(parts)))
    finally:
        b.close()


def _device_pass(topology=False, site_rates=False, **kw):
    sc, split = _scenario()
    return _run_device(sc, split, topology, _site_rates() if site_rates else None, **kw)


@functools.lru_cache(maxsize=None)
def _default_pass():
    return _device_pass()


def _assert_pass_is_the_oracles(dev, orc, what):
    """Move for move: kind, node and verdict equal, the log MH ratio within 1e-9; counters and random draws equal; the trees equal (times
    within 1e-9)."""
    worst = 0.0
    for p, (g, o) in enumerate(zip(dev, orc)):
        worst = max(worst, assert_traces_match(g["trace"], o["trace"], 1e-9, "%s, part %d" % (what, p)))
        for k in ("moves_done", "rng_draws", "proposed", "accepted"):
            assert g["stats"][k] == o["stats"][k], "%s, part %d: %s %s, the oracle's %s" % (what, p, k, g["stats"][k], o["stats"][k])
        assert g["stats"]["moves_done"] == MOVES
        assert_trees_match(g["tree"], o["tree"], 1e-9, "%s, part %d" % (what, p))
    print("%s: worst |log MH difference| / max(1, |log MH|) = %.3g" % (what, worst))


def _assert_same_bits(a, b, what):
    """Two device passes left the same bits behind: every tree array, counters, draws and algorithmic byte counts."""
    for p, (x, y) in enumerate(zip(a, b)):
        assert x["tree"].root == y["tree"].root
        for f in TREE_FIELDS:
            assert np.array_equal(getattr(x["tree"], f), getattr(y["tree"], f), equal_nan=True), "%s: part %d: %s differs" % (what, p, f)
        for k in ("moves_done", "rng_draws", "proposed", "accepted", "algorithmic_bytes", "algorithmic_write_bytes"):
            assert x["stats"][k] == y["stats"][k], "%s: part %d: %s %s vs %s" % (what, p, k, x["stats"][k], y["stats"][k])


def _noted_reforms_by_class(orc, parts):
    """{class: [rejected, accepted]} of the noted branch reforms of a pass without topology moves: class = mutations on the branch in the
    tree the pass started from, 5 standing for five or more."""
    cls = {}
    for o, part in zip(orc, parts):
        n = np.diff(part.mut_offset)
        tr = o["trace"]
        for row in tr[(tr[:, 0] == K_REFORM) & ~np.isnan(tr[:, 3])]:
            cls.setdefault(min(int(n[int(row[1])]), 5), [0, 0])[int(row[2])] += 1
    return cls


def test_short_and_long_reforms_with_the_topology_moves_off():
    """200 traced moves per part, list lengths fixed.  From the oracle's trace and the initial tree: each class n = 1, 2, 3, 4 and >= 5
    holds at least 10 noted reforms, and the reforms of n <= 4 hold both verdicts.  Then the device's pass is the oracle's."""
    sc, split = _scenario()
    orc = _oracle()
    for part in split[0]:
        for x in range(part.num_nodes):
            s = part.mut_site[part.mut_offset[x]:part.mut_offset[x + 1]]
            assert len(set(s.tolist())) == len(s), "a branch of the scenario carries a site twice"
    cls = _noted_reforms_by_class(orc, split[0])
    print("noted reforms per class [rejected, accepted] (oracle):", dict(sorted(cls.items())))
    for k in (1, 2, 3, 4, 5):
        assert sum(cls.get(k, [0, 0])) >= 10, "class %d holds %s noted reforms: the scenario no longer covers it" % (k, cls.get(k))
    short = [sum(cls.get(k, [0, 0])[v] for k in (1, 2, 3, 4)) for v in (0, 1)]
    assert short[0] >= 1 and short[1] >= 1, "the short reforms hold %d rejections and %d acceptances" % tuple(short)
    dev, (counts, main) = _default_pass()
    print("variants (whole, prefix, HBM):", counts, "main-launch mask:", main)
    _assert_pass_is_the_oracles(dev, orc, "topology moves off")


def _pass_in_variant(variant):
    """The pass of the first test with every part (or, for the side launch, at least one) run the named way, or None."""
    if variant == "whole":      # no side launches: every part in the main launch, staged whole
        r = _device_pass(options=(("giants", "0"),))
        return r if r[1][0][0] > 0 and np.all(r[1][1]) else None
    if variant == "prefix":
        for cap in (32768, 24576, 16384, 12288, 10240, 8192, 6144, 4096, 2048, 512):
            r = _device_pass(options=(("lds_max", cap),), want_variant=1)
            if r is not None:
                print("lds_max %d: variants (whole, prefix, HBM) %s" % (cap, r[1][0]))
                return r
        return None
    if variant == "hbm":
        r = _device_pass(use_lds=False)
        return r if r[1][0][2] > 0 else None
    if variant == "side":       # the default classes put the part that holds the run's root in a side launch
        r = _default_pass()
        return r if not np.all(r[1][1]) else None
    raise ValueError(variant)


@pytest.mark.parametrize("variant", ["whole", "prefix", "hbm", "side"])
def test_every_code_variant_leaves_the_same_bits(variant):
    """The same pass with the parts staged whole, staged by prefix, resident in HBM, and in a side launch: the oracle's pass, and the very
    bits of the default pass -- every tree array, counters, draws, algorithmic byte counts."""
    r = _pass_in_variant(variant)
    if r is None:
        pytest.skip("no part lands in the %s variant" % variant)
    print("%s: variants (whole, prefix, HBM) %s, main-launch mask %s" % (variant, r[1][0], r[1][1]))
    _assert_pass_is_the_oracles(r[0], _oracle(), variant)
    _assert_same_bits(r[0], _default_pass()[0], "%s vs the default pass" % variant)


def test_factors_from_the_per_site_arrays_and_from_the_logarithm():
    """`no_uniform_sites`: site partition and relative rate are loaded per site although all are 0 and 1.0 -- the same pass.  And relative
    rates that are not all one, so that B comes from the logarithm at every other site and from the staged table at the rest."""
    _assert_pass_is_the_oracles(_device_pass(options=(("no_uniform_sites", "1"),))[0], _oracle(), "no_uniform_sites")
    sc, split = _scenario()
    orc = _oracle(site_rates=True)
    cls = _noted_reforms_by_class(orc, split[0])
    print("site rates: noted reforms per class [rejected, accepted] (oracle):", dict(sorted(cls.items())))
    assert all(sum(cls.get(k, [0, 0])) >= 10 for k in (1, 2, 3, 4, 5))
    _assert_pass_is_the_oracles(_device_pass(site_rates=True)[0], orc, "site rates")


def _with_a_site_twice(sc, node, site):
    """The scenario with a pair a -> b, b -> a at `site` added to the branch above `node`, at a quarter and three quarters of its length."""
    t = sc.tree
    a = int(sc.ref[site]); b = (a + 1) % 4
    lo, hi = int(t.mut_offset[node]), int(t.mut_offset[node + 1])
    t_P, t_X = float(t.t[t.parent[node]]), float(t.t[node])
    recs = [(float(t.mut_t[i]), int(t.mut_site[i]), int(t.mut_from[i]), int(t.mut_to[i])) for i in range(lo, hi)]
    recs += [(t_P + 0.25 * (t_X - t_P), site, a, b), (t_P + 0.75 * (t_X - t_P), site, b, a)]
    recs.sort(key=lambda r: (r[0], r[1]))

    def splice(arr, col, dt):
        return np.concatenate([arr[:lo], np.array([r[col] for r in recs], dt), arr[hi:]])
    t2 = copy.copy(t)
    t2.mut_t, t2.mut_site, t2.mut_from, t2.mut_to = splice(t.mut_t, 0, np.float64), splice(t.mut_site, 1, np.int32), splice(t.mut_from, 2, np.uint8), splice(t.mut_to, 3, np.uint8)
    t2.mut_offset = t.mut_offset.copy(); t2.mut_offset[node + 1:] += 2
    sc2 = copy.copy(sc); sc2.tree = t2
    return sc2


def test_a_branch_that_carries_a_site_twice_takes_the_general_path():
    """Node 6's branch (one mutation) is given a -> b, b -> a at a site nothing else touches: three mutations, one site twice, which the
    register path must hand to the general one.  The oracle accepts the tree and, under split seed 11, notes 7 reforms of that branch in
    its 200 moves per part (asserted: at least 5); the device's pass is the oracle's."""
    node, seed = 6, 11
    sc, _ = _scenario()
    t = sc.tree
    free = np.ones(sc.num_sites, bool)
    free[t.mut_site[:int(t.mut_offset[-1])]] = False
    free[t.mfs_site[:int(t.mfs_offset[-1])]] = False
    for s, e in zip(t.miss_start[:int(t.miss_offset[-1])], t.miss_end[:int(t.miss_offset[-1])]):
        free[s:e] = False
    sc2 = _with_a_site_twice(sc, node, int(np.nonzero(free)[0][0]))
    split = split_parts(sc2, NPARTS, seed)
    orc = _run_oracle(sc2, split, False, None)
    reforms = 0
    for o, part in zip(orc, split[0]):
        for x in range(part.num_nodes):
            s = part.mut_site[part.mut_offset[x]:part.mut_offset[x + 1]]
            if len(set(s.tolist())) != len(s):
                assert len(s) == 3
                tr = o["trace"]
                reforms += int(np.sum((tr[:, 0] == K_REFORM) & (tr[:, 1] == x) & ~np.isnan(tr[:, 3])))
    print("noted reforms of the branch with a site twice (oracle):", reforms)
    assert reforms >= 5, "the oracle reforms the branch %d times: the case no longer reaches the guard" % reforms
    dev, _ = _run_device(sc2, split, False, None)
    _assert_pass_is_the_oracles(dev, orc, "a site twice")


def test_the_full_move_mix():
    """200 moves per part with the topology moves on: lists change their length under the moves, branches move between the two paths."""
    _assert_pass_is_the_oracles(_device_pass(topology=True)[0], _oracle(topology=True), "full move mix")
