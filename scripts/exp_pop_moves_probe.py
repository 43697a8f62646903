"""What one call of the Exponential population moves (50 rounds: 100 Metropolis steps, 101 evaluations of the whole-tree coalescent prior) costs at
C4 (100 000 tips), as one JSON line into profiles/exp_pop_moves_probe_latest.json:
  rounds   with min_pop = 0 and min_pop > 0: milliseconds per emat_exp_pop_moves call (wall time, measured WITHOUT spans), with what the steps did
  phases   the same calls in a second child under EMAT_VERBOSE=spans: the call by phase (statistics to the device, queueing the launch chain, the
           chain itself, copy-back), mean over ALL calls of both cases -- the first call allocates, which is most of phase 1's mean
  cycles   whole cycles per second over 60 cycles of the run driver, tree in HBM, under an exponential model, with the group off and on
The statistics are the C4 scenario tree's own (skygrid_moves_probe.tree_statistics: about 400 cells, 99 999 inner nodes); the model is the
generating one's, N(t) = 1500 x 365 e^{(6 / 365) (t - t_max)}.
Usage:
  python scripts/exp_pop_moves_probe.py          every step as a child process under its own time limit, one after the other, stopping at the first
                                                 that fails; then the JSON line
  python scripts/exp_pop_moves_probe.py STEP     one step in this process: rounds | cycles_off | cycles_on   (prints its own JSON)"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from skygrid_moves_probe import tree_statistics  # noqa: E402

LIMIT_S, CALLS, CELLS, ROUNDS = 300, 20, 400, 50
SEED, PARTS, CYCLES = 20261001, 8192, 60
N0, G = 1500.0 * 365.0, 6.0 / 365.0


def step_rounds():
    import delphy_amd as d
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
    t_ref, t_step, first, k_bar, inner_t = tree_statistics(sc.tree, CELLS)
    b = d.EmatBackend(sc.num_sites)
    out = {"num_cells": int(k_bar.shape[0]), "num_inner": int(inner_t.shape[0]), "rounds": ROUNDS, "calls": CALLS, "cases": []}
    spec = d.ExpPopSpec(rounds=ROUNDS)
    for min_pop in (0.0, 1000.0):
        n0, g = N0, G
        ms, acc = [], np.zeros(3)
        for k in range(CALLS + 1):
            t0 = time.perf_counter()
            r = b.exp_pop_moves(d.PopModel.exp(t_ref, n0, g, min_pop), spec, t_ref, t_step, first, k_bar, inner_t, key=1000 + k)
            if k:                                                   # the first call pays the allocations
                ms.append((time.perf_counter() - t0) * 1e3)
            n0, g = r.n0, r.g; acc += r.n0_accepted, r.g_accepted, r.g_out_of_bounds
        out["cases"].append({"min_pop": min_pop, "ms_per_call_mean": float(np.mean(ms)), "ms_per_call_min": float(np.min(ms)), "n0_accepted": int(acc[0]), "g_accepted": int(acc[1]),
                             "g_out_of_bounds": int(acc[2]), "n0": n0, "g": g, "log_coalescent_prior_end": r.log_coalescent_prior_end})
    b.close()
    return out


def step_cycles(on):
    import delphy_amd as d
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
    b = d.EmatBackend(sc.num_sites)
    r = d.EmatRun(b, sc.tree, sc.ref, SEED)
    r.set_num_parts(PARTS); r.set_max_part_nodes(-1); r.set_hky(sc.mu, sc.kappa, sc.pi); r.set_pop_model(d.PopModel.exp(sc.t_max_tip, N0, G, 0.0)); r.set_device_tree(True)
    if on:
        r.set_exp_pop_moves(True, d.ExpPopSpec(rounds=ROUNDS))
    per_cycle = 50 * sc.tree.num_nodes
    r.do_mcmc_steps(2 * per_cycle, per_cycle); b.synchronize()
    t0 = time.perf_counter()
    r.do_mcmc_steps(CYCLES * per_cycle, per_cycle); b.synchronize()
    dt = time.perf_counter() - t0
    out = {"cycles": CYCLES, "cycles_per_s": CYCLES / dt, "ms_per_cycle": dt / CYCLES * 1e3}
    if on:
        n0, g = r.exp_pop()
        out.update({"n0": n0, "g": g})
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
            print("exp_pop_moves_probe: step %s ended with status %d; nothing further is started" % (name, p.returncode), file=sys.stderr)
            return p.returncode
        if spans:   # the engine call's own stretches over ALL calls of both cases: mean milliseconds per call, from the spans table
            line["engine_call_by_phase_ms_over_all_calls"] = {m.group(1).strip(): float(m.group(2)) / 1e3
                                                              for m in re.finditer(r"\[emat\]\s+(exp_pop_moves: .*?)\s+[\d.]+\s+\d+\s+([\d.]+)\s+[\d.]+\s*$", p.stderr, re.M)}
        else:
            line[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "exp_pop_moves_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
