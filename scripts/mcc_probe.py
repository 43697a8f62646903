"""What the store of sampled trees and the MCC derivation cost at full size (config C4, 199 999 nodes): one JSON line.

Medians of >= 20 calls in one process, synchronise included:
  * emat_tree_sample_push against the two calls it replaces, emat_tree_get_topology and emat_tree_download, on the same build, each both
    right after a reassemble (a push per cycle, as a sampler meets it) and as repeated calls on one tree;
  * emat_mcc_derive at M = 32, 256 and 1 000 samples (--samples), the samples pushed after as many cycles of the run driver;
  * with --host-model: tests/mcc_model.py (a), derive_mcc_tree to the letter in Python, on the first 32 samples on the host;
  * with --samples-probe: emat_mcc_probe_ancestors over the samples of each derivation (16 MCC nodes picked at random among the inner nodes
    with support < 1, 200 cells) in four modes -- the mean alone; the mean and three order statistics (2.5 %, 50 %, 97.5 %); everything copied
    back; the mean alone with the chunk forced to one sample -- and, beside them, the unchanged emat_tree_probe_ancestors on the resident tree
    with 16 marks, which a loop over the samples would call M times.  The store then also keeps every sample's mutations (the pushes of the
    cycles are pushes WITH mutation room; a push without it is measured at the end, on the store cleared and its room released), and
    emat_mcc_probe_site_states is timed for 1 and 8 sites (the sites the resident tree mutates most; 200 cells, the mean and three order
    statistics) beside the unchanged emat_tree_probe_site_states on the resident tree, which a loop would call M x sites times.
  * with --summaries: emat_mcc_node_times (all nodes with five quantiles and a 95 % HPD; 16 picked nodes with their per-sample times) and
    emat_mcc_mutation_support over the samples of each derivation, medians of >= 10 calls, and beside them in the same process what a front end
    does today: M x (emat_mcc_get_correspondence + emat_tree_sample_get of the times) with NumPy's sorts, and M x emat_tree_sample_get_mutations.

    python scripts/mcc_probe.py [--samples 32,256,1000] [--moves-per-part 50] [--host-model] [--samples-probe] [--summaries] > profiles/mcc_probe_latest.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import delphy_amd as d  # noqa: E402
from delphy_amd.scenarios import make_scenario  # noqa: E402


def median_ms(f, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def summaries(b, sc, sizes, calls):
    """--summaries: emat_mcc_node_times and emat_mcc_mutation_support over the samples of each derivation, and beside them what a front end
    does today: M x (emat_mcc_get_correspondence + emat_tree_sample_get of the times) and NumPy's sorts; for the mutations M x
    emat_tree_sample_get_mutations on top, the download alone (matching the records in Python is not timed: a lower bound of the host's path)."""
    import ctypes as C
    Q = (0.025, 0.25, 0.5, 0.75, 0.975); mass = 0.95
    n = int(sc.tree.num_nodes)
    rng = np.random.default_rng(17)
    res = {"quantiles": list(Q), "hpd_mass": mass, "layout": "one workgroup per node, column read from the sample-major chunk", "by_M": []}
    t_buf = np.zeros(n)

    def times_of(k):
        b._ck(b._lib.emat_tree_sample_get(b._h, k, None, None, None, t_buf.ctypes.data_as(C.POINTER(C.c_double)), None), "emat_tree_sample_get")
        return t_buf

    for M in sizes:
        r = b.mcc_derive(0, M, 1, seed=1)
        picks = [int(v) for v in rng.choice(n, size=16, replace=False)]
        dev_calls, host_calls = max(10, calls if M <= 256 else 10), (3 if M <= 256 else 1)      # (NumPy's two sorts of M x n doubles take a minute at M = 1 000)
        row = {"M": M, "device_calls_per_median": dev_calls, "host_calls_per_median": host_calls}
        # the calls as a front end makes them: into arrays it allocated once (fresh arrays of 23 MB cost more in page faults than the call)
        qa = np.array(Q); keep = []

        def request(nodes, per_sample):
            cols = n if nodes is None else len(nodes)
            arrs = [np.zeros((len(Q), cols)), np.zeros((len(Q), cols)), np.zeros((2, cols)), np.zeros((2, cols)), np.zeros(cols, np.int32)]
            if per_sample: arrs += [np.zeros((cols, M)), np.zeros((cols, M), np.uint8)]
            dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
            res = d.engine._MccNodeTimesResultC(len(Q), dp(qa), mass, dp(arrs[0]), dp(arrs[1]), dp(arrs[2]), dp(arrs[3]), arrs[4].ctypes.data_as(C.POINTER(C.c_int32)),
                                                dp(arrs[5]) if per_sample else None, arrs[6].ctypes.data_as(C.POINTER(C.c_uint8)) if per_sample else None)
            nd = None if nodes is None else np.ascontiguousarray(nodes, np.int32)
            keep.append((arrs, nd))
            return lambda: b._ck(b._lib.emat_mcc_node_times(b._h, 0 if nd is None else len(nodes), None if nd is None else nd.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res)), "emat_mcc_node_times")

        ms = b.mcc_mutation_support()
        nm = C.c_int64(0); k = int(ms.num_with.shape[0])
        sup = [np.zeros(k, np.int32), np.zeros(k), np.zeros(k), np.zeros(k)]
        support = lambda: b._ck(b._lib.emat_mcc_mutation_support(b._h, k, C.byref(nm), sup[0].ctypes.data_as(C.POINTER(C.c_int32)), *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in sup[1:]]), "emat_mcc_mutation_support")
        all_nodes, picked = request(None, False), request(picks, True)
        all_nodes(); picked(); support()                      # (first calls: allocations)
        row["master_mutations"] = k; row["master_mutations_in_every_sample"] = int((ms.num_with == M).sum())
        row["node_times_all_nodes_ms"] = median_ms(all_nodes, dev_calls)
        row["node_times_all_nodes_min_ms"] = min(median_ms(all_nodes, 1) for _ in range(dev_calls))
        row["node_times_16_nodes_with_times_ms"] = median_ms(picked, dev_calls)
        row["mutation_support_ms"] = median_ms(support, dev_calls)
        row["node_times_all_nodes_fresh_python_arrays_ms"] = median_ms(lambda: b.mcc_node_times(None, Q, mass), dev_calls)
        x = np.empty((M, n)); ex = np.empty((M, n), bool)

        def download():
            for k in range(M):
                corr, e = b.mcc_correspondence(k)
                x[k] = times_of(k)[corr]; ex[k] = e

        def numpy_sorts():                                   # the same numbers, but for the exact kind's HPD (a window per node): a lower bound
            s = np.sort(x, axis=0); se = np.sort(np.where(ex, x, np.inf), axis=0); m = ex.sum(axis=0)
            cols = np.arange(n)
            q = [(s[int(np.floor(p * (M - 1)))], se[np.floor(p * (m - 1)).astype(np.int64), cols]) for p in Q]
            w = min(M, max(1, int(np.ceil(mass * M))))
            i = np.argmin(s[w - 1:] - s[:M - w + 1], axis=0)
            return q, s[i, cols], s[i + w - 1, cols]

        def download_mutations():
            for k in range(M): b.tree_sample_get_mutations(k)

        row["host_download_table_and_times_ms"] = median_ms(download, host_calls)
        last = []
        row["host_numpy_sorts_ms"] = median_ms(lambda: last.append(numpy_sorts()), host_calls)
        row["host_download_mutations_ms"] = median_ms(download_mutations, host_calls)
        got = b.mcc_node_times(None, Q, mass); q, lo, hi = last[-1]
        row["equal_to_numpy"] = bool(all(np.array_equal(got.q_mrca[j], q[j][0]) and np.array_equal(got.q_exact[j], q[j][1]) for j in range(len(Q))) and np.array_equal(got.hpd_mrca[0], lo) and np.array_equal(got.hpd_mrca[1], hi))
        res["by_M"].append(row)
        print("summaries", row, file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--samples", default="32,256,1000")
    ap.add_argument("--parts", type=int, default=8192)
    ap.add_argument("--moves-per-part", type=int, default=50)
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--host-model", action="store_true")
    ap.add_argument("--samples-probe", action="store_true")
    ap.add_argument("--summaries", action="store_true")
    a = ap.parse_args()
    if a.host_model and a.samples_probe: ap.error("--host-model reads the samples --samples-probe has cleared by then: run them apart")
    sizes = sorted(int(x) for x in a.samples.split(","))
    sc = make_scenario(a.config)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 5)
    run.set_num_parts(a.parts); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    out = {"config": a.config, "num_nodes": int(sc.tree.num_nodes), "emat_build_id": d.library_build_id(), "date": time.strftime("%Y-%m-%d"), "calls_per_median": a.calls,
           "parts": a.parts, "moves_per_part_and_cycle": a.moves_per_part}
    t_push, t_topo = [], []
    try:
        for cycle in range(sizes[-1]):
            run.repartition()
            if cycle == 0:
                b.tree_samples_reserve(sizes[-1] + a.calls)
                if a.samples_probe or a.summaries: b.tree_samples_reserve_mutations((sizes[-1] + a.calls) * (2 * int(sc.tree.mut_offset[sc.tree.num_nodes]) + 4096))
            run.run_moves(a.parts * a.moves_per_part); b.synchronize()
            run.reassemble(); b.synchronize()
            t0 = time.perf_counter(); b.tree_sample_push(); b.synchronize(); t1 = time.perf_counter()
            t_push.append((t1 - t0) * 1e3)
            if cycle < 32:
                b.tree_topology(); t_topo.append((time.perf_counter() - t1) * 1e3)
            if cycle % 100 == 99: print("cycle", cycle + 1, file=sys.stderr, flush=True)
        out["push_after_reassemble_ms"] = float(np.median(t_push)); out["get_topology_after_reassemble_ms"] = float(np.median(t_topo))
        out["push_repeated_ms"] = median_ms(lambda: (b.tree_sample_push(), b.synchronize()), a.calls)
        out["get_topology_repeated_ms"] = median_ms(b.tree_topology, a.calls)
        out["tree_download_ms"] = median_ms(b.tree_download, a.calls)
        out["derive"] = []
        for M in sizes:
            t0 = time.perf_counter(); r = b.mcc_derive(0, M, 1, seed=1); first = (time.perf_counter() - t0) * 1e3
            ms = median_ms(lambda: b.mcc_derive(0, M, 1, seed=1), 20 if M <= 256 else 5)
            inner = r.child0 >= 0
            out["derive"].append({"M": M, "first_call_ms": first, "median_ms": ms, "distinct_clades": r.num_distinct_clades, "table_slots": r.table_slots, "table_regrows": r.table_regrows,
                                  "master": r.master, "inner_nodes_with_support_below_1": int((r.support[inner] < 1).sum()), "least_support": float(r.support[inner].min())})
            print("derive", M, ms, file=sys.stderr, flush=True)
        if a.summaries:
            out["summaries"] = summaries(b, sc, sizes, a.calls)
        if a.samples_probe:
            rng = np.random.default_rng(16)
            t_root = b.tree_kids()[2]
            window = (t_root - 1.0, sc.t_max_tip + 1.0, 200)
            marked = [int(v) for v in rng.choice(sc.tree.num_nodes, size=16, replace=False)]
            out["samples_probe"] = {"cells": 200, "mcc_nodes": 16, "single_tree_probe_ancestors_ms": median_ms(lambda: b.tree_probe_ancestors(sc.pop, marked, *window), a.calls), "by_M": []}
            for M in sizes:
                r = b.mcc_derive(0, M, 1, seed=1)
                shaky = np.flatnonzero((r.child0 >= 0) & (r.support < 1))
                picks = [int(v) for v in rng.choice(shaky, size=16, replace=False)]
                ranks = [int(round(q * (M - 1))) for q in (0.025, 0.5, 0.975)]
                calls = a.calls if M <= 256 else 5
                modes = {"mean_only_ms": dict(per_sample=False), "mean_and_three_ranks_ms": dict(per_sample=False, ranks=ranks), "everything_copied_back_ms": dict(ranks=ranks)}
                row = {"M": M, "ranks": ranks}
                for name, kw in modes.items():
                    b.mcc_probe_ancestors(sc.pop, picks, *window, **kw)                      # (first call: allocations)
                    row[name] = median_ms(lambda: b.mcc_probe_ancestors(sc.pop, picks, *window, **kw), calls)
                b.set_option("samples_probe_chunk", 1)
                b.mcc_probe_ancestors(sc.pop, picks, *window, per_sample=False)
                row["mean_only_chunk_of_one_ms"] = median_ms(lambda: b.mcc_probe_ancestors(sc.pop, picks, *window, per_sample=False), calls)
                b.set_option("samples_probe_chunk", 0)
                row["M_single_tree_calls_ms"] = M * out["samples_probe"]["single_tree_probe_ancestors_ms"]
                out["samples_probe"]["by_M"].append(row)
                print("samples probe", row, file=sys.stderr, flush=True)
            # the site-state form: samples that kept their mutations
            per_site = np.bincount(sc.tree.mut_site[:int(sc.tree.mut_offset[sc.tree.num_nodes])], minlength=sc.num_sites)
            busy = [int(v) for v in np.argsort(-per_site, kind="stable")[:8]]
            used, cap, _ = b.tree_samples_mutation_info()
            st = {"cells": 200, "sites": busy, "mutation_records_per_sample": used / b.tree_samples_count(), "arena_records": cap,
                  "push_with_mutation_room_after_reassemble_ms": out["push_after_reassemble_ms"], "push_with_mutation_room_repeated_ms": out["push_repeated_ms"],
                  "single_tree_probe_site_states_ms": median_ms(lambda: b.tree_probe_site_states(sc.pop, busy[0], *window), a.calls), "by_M": []}
            for M in sizes:
                b.mcc_derive(0, M, 1, seed=1)
                ranks = [int(round(q * (M - 1))) for q in (0.025, 0.5, 0.975)]
                calls = a.calls if M <= 256 else 5
                row = {"M": M, "ranks": ranks}
                for num_sites in (1, 8):
                    b.mcc_probe_site_states(sc.pop, busy[:num_sites], *window, per_sample=False, ranks=ranks)      # (first call: allocations)
                    row["mean_and_three_ranks_%d_sites_ms" % num_sites] = median_ms(lambda: b.mcc_probe_site_states(sc.pop, busy[:num_sites], *window, per_sample=False, ranks=ranks), calls)
                    row["M_x_%d_single_tree_calls_ms" % num_sites] = M * num_sites * st["single_tree_probe_site_states_ms"]
                st["by_M"].append(row)
                print("samples site states", row, file=sys.stderr, flush=True)
            b.tree_samples_clear(); b.tree_samples_reserve_mutations(0)
            st["push_without_mutation_room_repeated_ms"] = median_ms(lambda: (b.tree_sample_push(), b.synchronize()), a.calls)
            out["samples_site_states"] = st
        if a.host_model:
            import mcc_model as mm
            ss = [mm.Sample(*b.tree_sample_get(i)) for i in range(min(32, sizes[-1]))]
            t0 = time.perf_counter(); mm.derive_letter(ss, 1); out["host_model_a_M32_s"] = time.perf_counter() - t0
    finally:
        run.close(); b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
