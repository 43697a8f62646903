"""The bits the tree probers give, as SHA-256 digests: to compare two builds of the library on one device (the loaded one is the one
at EMAT_LIB_PATH, or the tree's own).  Only the public API of delphy_amd/engine.py is used, every tree is made on the host and no
move is run, so nothing but the probers is in play.

A group is (tips, cells, where the window starts, population model); it yields one digest per kind of call, over the bytes of
everything the calls of that kind return (p, mean, order_stats, cells_to_skip, the counts):

  resident_ancestors   tree_probe_ancestors with no marks, the root, a repeated node, a -1
  resident_sites       tree_probe_site_states for a site with a mutation and one without
  branch_counts        tree_branch_counts of both kinds
  samples_ancestors    M = 1 and 5 samples x marks shared and per sample x chunk 0 and 1; mean and three ranks
  mcc_ancestors        through the correspondence of an mcc_derive over the 5 samples, chunk 0 and 1
  samples_sites        3 sites over 5 samples that kept their mutations, chunk 0 and 1; mean and three ranks

Mutations are put on the scenario's tree by hand (with_mutations).  The 5 samples are that tree with its times stretched away from
the latest tip by 0, 7, 14, ... per cent, so every sample has a root time, and with it a grid, of its own.

    python scripts/prober_bits.py > digests.json        # {"emat_build_id": ..., "digests": {case: sha256}}
    python scripts/prober_bits.py --compare a.json b.json > profiles/prober_bits_latest.json   (exit status 1 when a digest differs)
"""
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import delphy_amd as d  # noqa: E402
import samples_probe_model as SP  # noqa: E402
from delphy_amd.scenarios import make_scenario  # noqa: E402

TIPS, CELLS, SAMPLES = (2, 129, 257), (1, 65, 200), 5


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None: h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def batched(r):
    return [r.p, r.mean, r.order_stats, r.cells_to_skip]


def with_mutations(tree, ref):
    """The tree with one mutation half way along the branch of every third node, each at a site of its own (so every `from` is the
    reference's state); the last site is never mutated.  (The scenario's own mutation rate leaves a tree this small without any.)"""
    nodes = [v for v in range(tree.num_nodes) if v != tree.root][::3][:len(ref) - 1]
    count = np.zeros(tree.num_nodes, np.int64); count[nodes] = 1
    site = np.arange(len(nodes))
    frm = np.asarray(ref)[site]
    return dataclasses.replace(tree, mut_offset=np.concatenate([[0], np.cumsum(count)]).astype(tree.mut_offset.dtype), mut_site=site.astype(tree.mut_site.dtype),
                               mut_from=frm.astype(tree.mut_from.dtype), mut_to=((frm + 1) % 4).astype(tree.mut_to.dtype),
                               mut_t=(0.5 * (tree.t[tree.parent[nodes]] + tree.t[nodes])).astype(tree.mut_t.dtype))


def stretched(tree, t_max, k):
    """(t, mut_t) of sample k: monotone in the tree's own times, so no branch turns round."""
    s = 1.0 + 0.07 * k
    return t_max - (t_max - tree.t) * s, t_max - (t_max - tree.mut_t) * s


def main():
    out = {}
    for tips in TIPS:
        sc = make_scenario("C1", num_tips=tips, num_sites=60)
        tree = with_mutations(sc.tree, sc.ref)
        n, root, nm = tree.num_nodes, int(tree.root), int(tree.mut_offset[tree.num_nodes])
        sites = [0, sc.num_sites - 1, 1]                   # mutated, never mutated, mutated
        times = [stretched(tree, sc.t_max_tip, k) for k in range(SAMPLES)]
        roots = [float(t[root]) for t, _ in times]
        span = sc.t_max_tip - roots[0]
        v, w = (root + 1) % n, (root + 2) % n
        mark_sets = ([], [root], [v, w, v], [v, -1])
        shared = [root, v, -1, v]
        per_sample = [[(v + k) % n, root, -1] for k in range(SAMPLES)]
        b = d.EmatBackend(sc.num_sites)
        try:
            b.set_ref_sequence(sc.ref); b.tree_upload(tree)
            b.tree_samples_reserve(SAMPLES)
            for t, _ in times: b.tree_sample_push_flat(tree.parent, tree.child0, tree.child1, t, root)
            mcc = b.mcc_derive()
            picks = [int(mcc.root), int(np.flatnonzero(mcc.child0 < 0)[0]), int(np.flatnonzero(mcc.child0 >= 0)[-1])]
            windows = {"before": min(roots) - 0.3 * span, "after": roots[0] + 0.37 * span}
            groups = [(cells, where, i) for cells in CELLS for where in windows for i in range(3)]
            res = {}

            def chunks(f):
                got = []
                for chunk in (0, 1):
                    b.set_option("samples_probe_chunk", chunk)
                    got += f()
                b.set_option("samples_probe_chunk", 0)
                return got

            for cells, where, i in groups:                 # the store without mutation room (tree_sample_push_flat)
                win = (windows[where], sc.t_max_tip + 0.25, cells)
                pop = SP.pops_for(win[1], min(roots))[i]
                g = res.setdefault((cells, where, i), {})
                g["resident_ancestors"] = digest(b.tree_probe_ancestors(pop, mk, *win) for mk in mark_sets)
                g["resident_sites"] = digest(b.tree_probe_site_states(pop, s, *win) for s in sites[:2])
                g["branch_counts"] = digest(x for r in (b.tree_branch_counts(*win, marked_nodes=shared), b.tree_branch_counts(*win, site=sites[0])) for x in (r[0], np.array([r[1]], np.int64), np.array([r[2]])))
                g["samples_ancestors"] = digest(x for x in chunks(lambda: [y for M in (1, SAMPLES) for marks in (shared, per_sample[:M])
                                                                          for y in batched(b.tree_samples_probe_ancestors(pop, marks, *win, count=M, ranks=[0, M // 2, M - 1]))]))
                g["mcc_ancestors"] = digest(x for x in chunks(lambda: batched(b.mcc_probe_ancestors(pop, picks, *win, ranks=[0, 2, 4]))))
            b.tree_samples_clear()
            b.tree_samples_reserve_mutations(SAMPLES * (nm + 16))
            for t, mut_t in times:
                b.tree_sample_push_flat_mutations(tree.parent, tree.child0, tree.child1, t, root, tree.mut_offset, tree.mut_site, tree.mut_from, tree.mut_to, mut_t, sc.ref)
            for cells, where, i in groups:                 # the same samples with their mutations (tree_sample_push_flat_mutations)
                win = (windows[where], sc.t_max_tip + 0.25, cells)
                pop = SP.pops_for(win[1], min(roots))[i]
                res[(cells, where, i)]["samples_sites"] = digest(x for x in chunks(lambda: batched(b.tree_samples_probe_site_states(pop, sites, *win, ranks=[0, 2, 4]))))
            for (cells, where, i), g in res.items():
                for kind, h in g.items():
                    out["tips %d, cells %d, %s the root, pop %d: %s" % (tips, cells, where, i, kind)] = h
        finally:
            b.close()
    print(json.dumps({"emat_build_id": d.library_build_id(), "digests": out}, indent=1))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    differing = sorted(k for k in set(A["digests"]) | set(B["digests"]) if A["digests"].get(k) != B["digests"].get(k))
    print(json.dumps({"cases": len(A["digests"]), "differing": differing, "parent": A, "new": B}, indent=1))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if len(sys.argv) > 1 and sys.argv[1] == "--compare" else main())
