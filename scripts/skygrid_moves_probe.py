"""What one round of the Skygrid population moves costs at C4 (100 000 tips), as one JSON line into profiles/skygrid_moves_probe_latest.json:
  rounds   per number of knots (2, 50, 400) and Skygrid type: milliseconds per emat_skygrid_moves call (wall time, measured WITHOUT spans), with what
           the moves did (accepted, the step the K rule ended at, log Metropolis ratio)
  phases   the same calls in a second child under EMAT_VERBOSE=spans, which waits for each kernel on its own: the call by phase (statistics to the
           device, k_skygrid_node_stats, k_skygrid_moves, copy-back), mean over ALL calls of all six cases -- the first call of each size allocates,
           which is most of phase 1's mean
  cycles   whole cycles per second over 60 cycles of the run driver, tree in HBM, with the group off and on
The statistics are the C4 scenario tree's own: its lineage grid (Scalable_coalescent_prior's, about 400 cells) and the times of its inner
nodes, made here on the host with numpy; the knots span the tree.
Usage:
  python scripts/skygrid_moves_probe.py          every step as a child process under its own time limit, one after the other, stopping at the first
                                                 that fails; then the JSON line
  python scripts/skygrid_moves_probe.py STEP     one step in this process: rounds | cycles_off | cycles_on   (prints its own JSON)"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT_S, ROUNDS, CELLS = 300, 20, 400
SEED, PARTS, CYCLES = 20261001, 8192, 60


def tree_statistics(tree, num_cells):
    """(t_ref, t_step, first_cell, k_bar, inner_t) of a FlatTree: scalable_coalescent.cpp:88-138, in float64 with difference arrays."""
    t = np.asarray(tree.t, np.float64); parent = np.asarray(tree.parent); inner = np.asarray(tree.child0) >= 0
    t_ref, t_root = float(t[~inner].max()), float(t[tree.root])
    t_step = (t_ref - t_root) / (num_cells - 1.5)
    cell = lambda x: np.floor((x - t_ref) / t_step).astype(np.int64)
    first = int(cell(np.array([t_root]))[0]); n = int(cell(np.array([t_ref]))[0]) - first + 1
    whole = np.zeros(n + 1); frac = np.zeros(n)
    v = np.flatnonzero(parent >= 0)
    lo = np.concatenate([t[parent[v]], [t_ref + first * t_step]]); hi = np.concatenate([t[v], [t_root]])   # (one lineage before the root inside its cell)
    cs, ce = cell(lo) - first, np.minimum(cell(hi) - first, n - 1)
    same = cs == ce
    np.add.at(frac, cs[same], (hi[same] - lo[same]) / t_step)
    d = ~same
    np.add.at(frac, cs[d], ((t_ref + (cs[d] + first + 1) * t_step) - lo[d]) / t_step)
    np.add.at(frac, ce[d], (hi[d] - (t_ref + (ce[d] + first) * t_step)) / t_step)
    np.add.at(whole, cs[d] + 1, 1.0); np.add.at(whole, ce[d], -1.0)
    return t_ref, t_step, first, np.maximum(frac + np.cumsum(whole)[:n], 0.0), t[inner]


def step_rounds():
    import delphy_amd as d
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
    t_ref, t_step, first, k_bar, inner_t = tree_statistics(sc.tree, CELLS)
    b = d.EmatBackend(sc.num_sites)
    out = {"num_cells": int(k_bar.shape[0]), "num_inner": int(inner_t.shape[0]), "rounds": ROUNDS, "cases": []}
    t_root = float(inner_t.min())
    for knots in (2, 50, 400):
        for log_linear in (False, True):
            x = np.linspace(t_root, t_ref, knots + 1)[1:] if knots > 2 else np.array([t_root + 0.25 * (t_ref - t_root), t_ref])
            gam = np.full(knots, np.log(max(1.0, 0.5 * (t_ref - t_root))))
            spec = d.SkygridSpec(tau=1.0, low_gamma_barrier_enabled=True)
            ms, acc, exits, lm = [], 0, [], []
            for k in range(ROUNDS + 1):
                t0 = time.perf_counter()
                r = b.skygrid_moves(d.PopModel.skygrid(x, gam, log_linear), spec, t_ref, t_step, first, k_bar, inner_t, key=1000 + k)
                if k:                                                   # the first round pays the allocations
                    ms.append((time.perf_counter() - t0) * 1e3)
                gam = r.gamma.copy(); spec.tau = r.tau; acc += r.hmc_accepted; exits.append(r.hmc_K_exit_step); lm.append(r.hmc_log_metropolis)
            out["cases"].append({"knots": knots, "log_linear": log_linear, "ms_per_call_mean": float(np.mean(ms)), "ms_per_call_min": float(np.min(ms)),
                                 "hmc_accepted": acc, "K_exits": int(sum(e >= 0 for e in exits)), "median_log_metropolis": float(np.median(lm)), "tau": r.tau})
    b.close()
    return out


def step_cycles(on):
    import delphy_amd as d
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
    b = d.EmatBackend(sc.num_sites)
    r = d.EmatRun(b, sc.tree, sc.ref, SEED)
    r.set_num_parts(PARTS); r.set_max_part_nodes(-1); r.set_hky(sc.mu, sc.kappa, sc.pi); r.set_pop_model(sc.pop); r.set_device_tree(True)
    if on:
        r.set_skygrid_moves(True, d.SkygridSpec(tau=1.0, low_gamma_barrier_enabled=True))
    per_cycle = 50 * sc.tree.num_nodes
    r.do_mcmc_steps(2 * per_cycle, per_cycle); b.synchronize()
    t0 = time.perf_counter()
    r.do_mcmc_steps(CYCLES * per_cycle, per_cycle); b.synchronize()
    dt = time.perf_counter() - t0
    out = {"cycles": CYCLES, "cycles_per_s": CYCLES / dt, "ms_per_cycle": dt / CYCLES * 1e3, "knots": int(sc.pop.skygrid_x.shape[0])}
    if on:
        g, tau = r.skygrid()
        out.update({"tau": tau, "gamma_min": float(g.min()), "gamma_max": float(g.max())})
    r.close(); b.close()
    return out


def main():
    if len(sys.argv) > 1:
        step = sys.argv[1]
        print("RESULT " + json.dumps(step_rounds() if step == "rounds" else step_cycles(step == "cycles_on")), flush=True)
        return 0
    import delphy_amd as d
    line = {"workload": os.environ.get("EMAT_WORKLOAD", "C4"), "build_id": d.source_build_id()}
    for name, step, spans in (("rounds", "rounds", False), ("phases", "rounds", True), ("cycles_off", "cycles_off", False), ("cycles_on", "cycles_on", False)):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), step], env=dict(os.environ, EMAT_VERBOSE="spans") if spans else dict(os.environ),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print("skygrid_moves_probe: step %s ended with status %d; nothing further is started" % (name, p.returncode), file=sys.stderr)
            return p.returncode
        if spans:   # the engine call's own stretches over ALL calls of all cases: mean milliseconds per call, from the spans table
            line["engine_call_by_phase_ms_over_all_calls"] = {m.group(1).strip(): float(m.group(2)) / 1e3
                                                              for m in re.finditer(r"\[emat\]\s+(skygrid_moves: .*?)\s+[\d.]+\s+\d+\s+([\d.]+)\s+[\d.]+\s*$", p.stderr, re.M)}
        else:
            line[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "skygrid_moves_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
