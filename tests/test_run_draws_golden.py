"""The run driver's draws, pinned -- CPU only, no backend.

What a cycle's partition is drawn from -- the ten stencils (redrawn every 200 cycles), the pick, the part-size limit's refinement and
the per-part seeds -- is a function of (seed, cycle, topology) alone.  tests/golden/run_driver_draws.json holds what the library gave
when the fixture was recorded (tests/golden/make_run_driver_draws.py); any change of the driver must give the same, integer for integer.

The tree is made by integer arithmetic alone: 1 001 tips joined pairwise in the order a 64-bit linear congruential recurrence picks,
every node's time minus its depth below the root (labels that tell the nodes apart in a part's node order; no backend ever reads
them as dates), all lists empty.  Nothing here depends on a machine's libm.
"""
import json
import os

import numpy as np

import delphy_amd as d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_driver_draws.json")
NUM_TIPS, NUM_SITES, SEED, NUM_PARTS, CYCLES = 1001, 16, 20261017, 8, 202
RECORDED_CYCLES = (0, 1, 2, 199, 200, 201)   # the stencils are redrawn at cycle 200
LIMITS = (64, 0)   # parts of about 250 nodes refined, and their pieces refined again | the reference's rule alone


def build_tree():
    n = 2 * NUM_TIPS - 1
    parent, c0, c1 = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    active, x = list(range(NUM_TIPS)), 88172645463325252
    for inner in range(NUM_TIPS, n):
        kids = []
        for _ in range(2):
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            kids.append(active.pop((x >> 33) % len(active)))
        c0[inner], c1[inner] = kids
        parent[kids[0]] = parent[kids[1]] = inner
        active.append(inner)
    root = n - 1
    depth = np.zeros(n, np.int64)
    for v in range(n - 2, -1, -1):   # (a child's index is below its parent's)
        depth[v] = depth[parent[v]] + 1
    tips = c0 == -1
    fmax = np.finfo(np.float32).max
    t = -depth.astype(np.float64)
    zeros = np.zeros(n + 1, np.int32)
    e32, e8, e64 = np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.float64)
    return d.FlatTree(root, parent, c0, c1, t, np.where(tips, t, -fmax).astype(np.float32), np.where(tips, t, fmax).astype(np.float32),
                      zeros.copy(), e32.copy(), e8.copy(), e8.copy(), e64, zeros.copy(), e32.copy(), e32.copy(), zeros.copy(), e32.copy(), e8.copy())


def _exact_int(x):
    assert x == int(x)   # (the times are minus a depth: whole numbers, written as such)
    return int(x)


def record(max_part_nodes):
    """{cycle: what the driver drew} at RECORDED_CYCLES of CYCLES cycles of repartition(); reassemble()."""
    run = d.EmatRun(None, build_tree(), np.zeros(NUM_SITES, np.uint8), SEED)
    run.set_num_parts(NUM_PARTS)
    run.set_max_part_nodes(max_part_nodes)
    out = {}
    for cycle in range(CYCLES):
        run.repartition()
        if cycle in RECORDED_CYCLES:
            n, root_part = run.num_parts()
            parts = [run.part(i) for i in range(n)]
            out[str(cycle)] = {"cut_nodes": [int(c) for c in run.debug_redraw_partition()], "partition_stats": run.partition_stats(), "num_parts": [n, root_part],
                               "part_seeds": [int(s) for _, _, s in parts], "part_first_times": [[_exact_int(x) for x in t.t[:5]] for t, _, _ in parts]}
        run.reassemble()
    run.close()
    return out


def test_tree_is_the_one_the_fixture_was_recorded_on():
    t = build_tree()
    gold = json.load(open(GOLDEN))
    assert t.num_nodes == 2001 and int(np.sum(t.child0 == -1)) == NUM_TIPS
    assert gold["tree_checksum"] == tree_checksum(t)


def tree_checksum(t):
    return [int(np.sum(t.child0.astype(np.int64) * np.arange(t.num_nodes))), int(np.sum(t.child1.astype(np.int64) * np.arange(t.num_nodes))), int(-np.sum(t.t))]


def test_draws_equal_the_recorded_ones():
    gold = json.load(open(GOLDEN))
    for limit in LIMITS:
        got, want = record(limit), gold["max_part_nodes=%d" % limit]
        assert sorted(got) == sorted(want) == sorted(str(c) for c in RECORDED_CYCLES)
        for cycle in want:
            for key in ("cut_nodes", "partition_stats", "num_parts", "part_seeds", "part_first_times"):
                assert got[cycle][key] == want[cycle][key], (limit, cycle, key)
    # the limit is what the fixture says it exercises: cut nodes beyond the stencil's, every part within it; and off, none
    on, off = gold["max_part_nodes=64"], gold["max_part_nodes=0"]
    assert all(c["partition_stats"]["extra_cuts"] > 0 and c["partition_stats"]["largest_part_nodes"] <= 64 for c in on.values())
    assert all(c["partition_stats"]["extra_cuts"] == 0 and c["num_parts"][0] <= NUM_PARTS for c in off.values())
    assert on["199"]["cut_nodes"] != on["200"]["cut_nodes"]
