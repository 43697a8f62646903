"""The reference's prober fixtures (tests/golden/prober_expectations.json) as objects, and its expectations as checks that take
any implementation's results: shared by test_prober_model.py (the Python model) and test_probe_gpu.py (the device)."""
import json
import math
import os

import numpy as np

import delphy_amd as d

G = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prober_expectations.json")))


def pop_model(m):
    return d.PopModel.const(m["pop"]) if m["kind"] == "const" else d.PopModel.exp(m["t0"], m["n0"], m["g"], m["min_pop"])


def flat_tree(t):
    nodes = t["nodes"]
    n = len(nodes)
    muts = [m for nd in nodes for m in nd["mutations"]]
    ft = d.FlatTree.empty(n, len(muts), 0, 0)
    ft.root = t["root"]
    k = 0
    for i, nd in enumerate(nodes):
        ft.parent[i] = nd["parent"]
        if nd["children"]:
            ft.child0[i], ft.child1[i] = nd["children"]
        ft.t[i], ft.t_min[i], ft.t_max[i] = nd["t"], nd["t_min"], nd["t_max"]
        for frm, site, to, tm in nd["mutations"]:
            ft.mut_from[k], ft.mut_site[k], ft.mut_to[k], ft.mut_t[k] = frm, site, to, tm
            k += 1
        ft.mut_offset[i + 1] = k
    return ft, np.array(t["ref_sequence"], np.uint8)


def cell_of(x, t_start, t_end, num_cells):
    """Staircase::cell_for on the RESULT's grid (the cells the caller asked for)."""
    return int(math.floor((x - t_start) / ((t_end - t_start) / num_cells)))


def check_prober_case(case, p, what):
    """The expectations of an ancestral / site-state case on p [members][cells]."""
    p = np.asarray(p)
    ts, te, nc = case["t_start"], case["t_end"], case["num_t_cells"]
    assert p.shape[1] == nc, what
    if "num_members" in case:
        assert p.shape[0] == case["num_members"], what
    for e in case.get("each_ge", []):
        assert np.all(p[e["member"]] >= e["value"]), (what, e)
    for e in case.get("each_eq", []):
        assert np.all(p[e["member"]] == e["value"]), (what, e)
    for e in case.get("at", []):
        assert abs(p[e["member"], cell_of(e["x"], ts, te, nc)] - e["value"]) <= e["tol"], (what, e)
    if "cells" in case:
        c = case["cells"]
        rows = p[:len(case["marked"])] if c["members"] == "marked" else p
        assert np.all(rows >= c["each_ge"]) and np.all(rows <= c["each_le"]), what
        tot = np.zeros(nc)
        for r in rows:                       # (summed member by member, as the reference's loop does)
            tot = tot + r
        assert np.all(np.abs(tot - c["sum_near"][0]) <= c["sum_near"][1]), (what, tot)


def check_tree_prober_case(case, p, what):
    """The expectations of a Tree_prober case on p [categories][cells - cells_to_skip]."""
    cell_size = (case["t_end"] - case["t_start"]) / case["num_cells"]
    t0 = case["t_start"] + case["cells_to_skip"] * cell_size      # cell_lbound(counts, cells_to_skip)
    nc = case["num_cells"] - case["cells_to_skip"]
    at = lambda member, x: p[member][int(math.floor((x - t0) / cell_size))]   # noqa: E731
    assert np.asarray(p).shape == (case["num_cats"], nc), what
    for e in case["expect"]:
        v = at(e["member"], e["x"])
        if e["matcher"] == "eq":
            assert v == e["value"], (what, e, v)
        elif e["matcher"] == "near":
            assert abs(v - e["value"]) <= e["tol"], (what, e, v)
        elif e["matcher"] == "gt":
            assert v > e["value"], (what, e, v)
        else:
            assert v > at(e["other_member"], e["other_x"]), (what, e, v)
    if "expect_t_start" in case:
        assert abs(t0 - case["expect_t_start"]["value"]) <= case["expect_t_start"]["tol"], what
