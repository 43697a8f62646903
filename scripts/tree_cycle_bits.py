"""The bits whole cycles of the HBM-resident tree give through the C-ABI (emat_tree_*), as SHA-256 digests: to compare two builds of the
library on one device (the loaded one is the one at EMAT_LIB_PATH, or the tree's own).  No run driver: cut nodes and part seeds are
drawn here, so each way into emat_tree_repartition can be asked for by name.

A case is (input, tables built by kernels or by the host's builder, partition made by emat_tree_partition or handed in as arrays,
tree_tight); it yields one digest per cycle and kind, over the bytes of what the calls return in node order:

  partition    emat_tree_partition + emat_tree_get_partition: parts, root part, offsets, orig, kid0, kid1
  parts        after the repartition, for every part: part_download, part_coalescent, part_rng, debug_slab_layout
  moved        after the moves, for every part: part_download, part_rng; then totals
  tree         after the reassemble: the root changes returned, tree_download and the reference sequence

Every case yields all four kinds (the two-handle exchange: parts and moved per block, over its local parts).  Nothing else is digested:
the list heaps, the cut-state pools and the export buffers are filled through atomics in whatever order the workgroups arrive, and
their raw bytes differ from run to run of one library.

    python scripts/tree_cycle_bits.py > digests.json        # {"emat_build_id": ..., "digests": {case: sha256}}
    python scripts/tree_cycle_bits.py --compare parent.json new.json [parent_again.json] > profiles/tree_cycle_bits_latest.json
                                                            (exit status 1 when a digest differs, between the two parent runs too)
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import delphy_amd as d  # noqa: E402
import delphy_amd.engine as e  # noqa: E402
from delphy_amd.scenarios import KAPPA, PI, Scenario, make_scenario  # noqa: E402

FIELDS = ("parent", "child0", "child1", "t", "t_min", "t_max", "mut_offset", "mut_site", "mut_from", "mut_to", "mut_t",
          "miss_offset", "miss_start", "miss_end", "mfs_offset", "mfs_site", "mfs_state")
CYCLES = 3


class Digest:
    def __init__(self): self.h = hashlib.sha256()

    def add(self, *xs):
        for x in xs:
            self.h.update(np.ascontiguousarray(x).tobytes())
        return self

    def tree(self, t): return self.add(np.int64(t.root), *(getattr(t, f) for f in FIELDS))

    def dict(self, m): return self.add(*(np.asarray(m[k]) for k in sorted(m)))

    def hex(self): return self.h.hexdigest()


def backend(sc, **options):
    b = d.EmatBackend(sc.num_sites)
    for k, v in options.items():
        b.set_option(k, v)
    b.set_ref_sequence(sc.ref); b.set_hky(sc.mu, sc.kappa, sc.pi); b.set_flags(sc.t_max_tip)
    return b


def repartition(b, sc, partition, seeds, made_here, lo=0, hi=None):
    n, root_part, off, orig, k0, k1 = partition
    I = C.POINTER(C.c_int32)
    arrays = [None] * 4 if made_here else [np.ascontiguousarray(a, np.int32).ctypes.data_as(I) for a in (off, orig, k0, k1)]
    sd = np.ascontiguousarray(seeds, np.uint64); m = sc.pop.c_struct()
    b._ck(b._lib.emat_tree_repartition_range(b._h, n, *arrays, root_part, sd.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m), sc.default_t_step(), lo, n if hi is None else hi),
          "emat_tree_repartition_range")


def draw(b, rng, parts):
    """Cut nodes (distinct inner nodes other than the root, nested ones included) and seeds of one cycle; the partition they give."""
    parent, c0, c1, t, root = b.tree_topology()
    inner = np.flatnonzero(c0 >= 0); inner = inner[inner != root]
    cuts = [int(v) for v in rng.choice(inner, size=min(parts - 1, len(inner)), replace=False)]
    partition = b.tree_partition(cuts)
    return partition, rng.integers(1, 2**62, partition[0]).astype(np.uint64)


def parts_digest(b, n, built):
    g = Digest()
    for p in range(n):
        g.tree(b.part_download(p)).dict(b.part_rng(p))
        if built: g.dict(b.part_coalescent(p)).dict(b.debug_slab_layout(p))
    return g.add(*(() if built else b.totals())).hex()


def cycles(out, name, sc, parts, moves, host_tables=0, made_here=True, **options):
    b = backend(sc, tree_host_coalescent=host_tables, **options)
    rng = np.random.default_rng(parts)
    try:
        b.tree_upload(sc.tree)
        for c in range(CYCLES):
            partition, seeds = draw(b, rng, parts)
            out["%s, cycle %d: partition" % (name, c)] = Digest().add(*partition).hex()
            repartition(b, sc, partition, seeds, made_here)
            out["%s, cycle %d: parts" % (name, c)] = parts_digest(b, partition[0], True)
            b.run_moves_per_part(moves); b.synchronize()
            out["%s, cycle %d: moved" % (name, c)] = parts_digest(b, partition[0], False)
            changes = b.tree_reassemble()
            tree, ref = b.tree_download()
            out["%s, cycle %d: tree" % (name, c)] = Digest().add(*changes).tree(tree).add(ref).hex()
        return b.tree_counters()
    finally:
        b.close()


def injected_root_changes(out, num_changes=700):
    """The input of test_gather_rereferences_missing_data_for_any_number_of_root_changes: changes of the root sequence handed to
    emat_tree_gather_local, more than the gather caches in LDS."""
    par = e.SynthParams(num_tips=150, num_sites=4000, tip_span=200.0, pop_n0=300.0, pop_growth=0.0, mu=2e-3 / 365.0, gaps_per_tip=4, mean_gap_len=200.0, seed=12)
    par.pi, par.kappa = PI, KAPPA
    tree, ref, tmax = e.make_synthetic_emat(par)
    sc = Scenario("gaps", tree, ref, tmax, par.mu, KAPPA, PI, d.PopModel.exp(tmax, 300.0, 0.0, 0.0), 4000)
    b = backend(sc)
    try:
        b.tree_upload(sc.tree)
        partition = b.tree_partition([])
        name = "%d root changes handed to the gather" % num_changes
        out[name + ": partition"] = Digest().add(*partition).hex()
        repartition(b, sc, partition, [7], False)
        out[name + ": parts"] = parts_digest(b, 1, True)
        out[name + ": moved"] = parts_digest(b, 1, False)          # (no move is run: the totals of the part as built)
        rng = np.random.default_rng(num_changes)
        mutated = set(int(x) for x in sc.tree.mut_site)
        site = np.array(sorted(rng.choice([l for l in range(sc.num_sites) if l not in mutated], num_changes, replace=False)), np.int32)
        frm = sc.ref[site].astype(np.uint8); to = ((frm + rng.integers(1, 4, num_changes)) % 4).astype(np.uint8)
        before = b.tree_root_deltas()
        b.tree_gather_local(site, frm, to); b.tree_reassemble_end()
        tree, ref = b.tree_download()
        out[name + ": tree"] = Digest().add(*before).tree(tree).add(ref).hex()
    finally:
        b.close()


def two_blocks(out, sc, parts=4, moves=200):
    """Two handles on one device with the parts [0, 2) and [2, 4): the staged gather with the exchange through host buffers."""
    blocks = [backend(sc), backend(sc)]
    rng = np.random.default_rng(17)
    try:
        for b in blocks: b.tree_upload(sc.tree)
        for c in range(CYCLES):
            partition, seeds = draw(blocks[0], rng, parts)
            out["two blocks, cycle %d: partition" % c] = Digest().add(*partition).hex()
            for k, b in enumerate(blocks):   # (a block's parts are its local parts 0, 1)
                repartition(b, sc, partition, seeds, False, 2 * k, 2 * k + 2)
                out["two blocks, cycle %d, block %d: parts" % (c, k)] = parts_digest(b, 2, True)
                b.run_moves_per_part(moves); b.synchronize()
                out["two blocks, cycle %d, block %d: moved" % (c, k)] = parts_digest(b, 2, False)
            deltas = [b.tree_root_deltas() for b in blocks]
            site, frm, to = next(x for x in deltas if x is not None)
            for b in blocks: b.tree_gather_local(site, frm, to)
            sent = [b.tree_export_nodes() for b in blocks]
            blocks[0].tree_apply_nodes(sent[1]); blocks[1].tree_apply_nodes(sent[0])
            for k, b in enumerate(blocks):
                b.tree_reassemble_end()
                tree, ref = b.tree_download()
                out["two blocks, cycle %d, block %d: tree" % (c, k)] = Digest().add(site, frm, to).tree(tree).add(ref).hex()
    finally:
        for b in blocks: b.close()


def main():
    out, counters = {}, {}
    inputs = ((2, make_scenario("C1", num_tips=2, num_sites=60), 1, 50), (257, make_scenario("C1", num_tips=257, num_sites=300, uncertain_tips=0.2), 8, 300),
              (3000, make_scenario("C3", num_tips=3000, num_sites=29903, uncertain_tips=0.1), 128, 400))
    for tips, sc, parts, moves in inputs:
        for host_tables in (0, 1):
            for made_here in (True, False):
                for tight in (0, 1):
                    name = "%d tips, tables by the %s, partition %s, tree_tight %d" % (tips, "host" if host_tables else "kernels", "made on the device" if made_here else "handed in", tight)
                    counters[name] = cycles(out, name, sc, parts, moves, host_tables, made_here, tree_tight=tight)
    # test_cut_point_states_larger_than_the_small_kernel_holds: a fast-evolving genome
    p = e.SynthParams(num_tips=400, num_sites=12000, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=5e-3 / 365.0, gaps_per_tip=2, mean_gap_len=60.0, seed=20261099)
    p.pi = PI; p.kappa = KAPPA
    tree, ref, tmax = e.make_synthetic_emat(p)
    hot = Scenario("hot", tree, ref, tmax, p.mu, p.kappa, PI, d.PopModel.exp(tmax, 365.0, 0.0, 0.0), p.num_sites)
    for made_here in (True, False):
        name = "large cut-point states, partition %s" % ("made on the device" if made_here else "handed in")
        counters[name] = cycles(out, name, hot, 12, 600, 0, made_here)
    injected_root_changes(out)
    # test_out_of_space_recoveries_inside_cycles: list heaps with almost no slack, so that parts stop for lack of room and are given more
    counters["out of space"] = cycles(out, "out-of-space recoveries", inputs[2][1], 128, 1500, 0, True, slack=1.05, heap_per_node=8)
    two_blocks(out, make_scenario("C1", num_tips=65, num_sites=60))
    print(json.dumps({"emat_build_id": d.library_build_id(), "digests": out, "pool regrows, heap regrows, large measures": counters}, indent=1))


def compare(a, b, again=None):
    A, B = json.load(open(a)), json.load(open(b))
    def differing(X, Y): return sorted(k for k in set(X["digests"]) | set(Y["digests"]) if X["digests"].get(k) != Y["digests"].get(k))   # noqa: E704
    res = {"cases": len(A["digests"]), "differing": differing(A, B)}
    if again is not None:
        res["differing between two runs of the parent"] = differing(A, json.load(open(again)))
    res.update(parent=A, new=B)
    print(json.dumps(res, indent=1))
    return 1 if res["differing"] or res.get("differing between two runs of the parent") else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:5]) if len(sys.argv) > 1 and sys.argv[1] == "--compare" else main())
