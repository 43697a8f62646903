"""What the site-rate moves cost at C4 (100 000 tips, 29 903 sites), as one JSON line into profiles/site_rate_probe_latest.json:
  phases_ms      milliseconds per emat_run_site_rate_moves by phase: the statistics (Ttwiddle_l and the mutations per site), the alpha
                 kernel, the draw with its reductions, the copy-back with refresh_ref_derived, and the emat_recalc_derived the new rates force
  cycles         whole cycles per second over 60 cycles with the moves off and on
  pass           the pass's moves/s with all-one rates (the engine's uniform_sites short cut) and with drawn rates: the price of the model
Usage:
  python scripts/site_rate_probe.py             every step below as a child process under its own time limit, one after the other,
                                                stopping at the first that fails; then the JSON line
  python scripts/site_rate_probe.py STEP        one step in this process: phases | cycles_off | cycles_on | pass   (prints its own JSON)"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"phases": 300, "cycles_off": 300, "cycles_on": 300, "pass": 300}     # seconds each child may take
SEED, PARTS, CYCLES, ROUNDS = 20261001, 8192, 60, 20


def _run(sc, on):
    import delphy_amd as d
    b = d.EmatBackend(sc.num_sites)
    r = d.EmatRun(b, sc.tree, sc.ref, SEED)
    r.set_num_parts(PARTS); r.set_max_part_nodes(-1); r.set_hky(sc.mu, sc.kappa, sc.pi); r.set_pop_model(sc.pop); r.set_device_tree(True)
    if on:
        r.set_site_rate_moves(True, 1.0)
    return b, r


def step_phases(sc):
    """EMAT_VERBOSE=spans makes the engine call wait for each of its kernels and book the stretches (the parent reads the table from stderr)."""
    b, r = _run(sc, False)
    r.repartition()
    t = {"statistics": 0.0, "engine_call": 0.0, "recalc_derived": 0.0}
    for k in range(ROUNDS + 1):
        t0 = time.perf_counter(); r.Ttwiddle_l(); b.num_muts_l(); t1 = time.perf_counter()
        res = r.site_rate_moves(); t2 = time.perf_counter()             # (computes the statistics again: booked as a whole below)
        b.recalc_derived(); b.synchronize(); t3 = time.perf_counter()
        if k:                                                           # the first round pays the allocations
            t["statistics"] += (t1 - t0) * 1e3 / ROUNDS; t["engine_call"] += ((t2 - t1) - (t1 - t0)) * 1e3 / ROUNDS; t["recalc_derived"] += (t3 - t2) * 1e3 / ROUNDS
    out = {"ms": t, "alpha": res.alpha, "num_accepted_of_10": res.num_accepted, "num_floored": res.num_floored, "rounds": ROUNDS}
    r.close(); b.close()
    return out


def step_cycles(sc, on):
    b, r = _run(sc, on)
    per_cycle = 50 * sc.tree.num_nodes
    r.do_mcmc_steps(2 * per_cycle, per_cycle)
    b.synchronize()
    t0 = time.perf_counter()
    r.do_mcmc_steps(CYCLES * per_cycle, per_cycle)
    b.synchronize()
    dt = time.perf_counter() - t0
    alpha, nu = r.site_rates()
    out = {"cycles": CYCLES, "cycles_per_s": CYCLES / dt, "ms_per_cycle": dt / CYCLES * 1e3, "moves_per_s": CYCLES * per_cycle / dt, "alpha": alpha, "mean_nu": float(nu.mean())}
    r.close(); b.close()
    return out


def step_pass(sc):
    """One partition, the same moves per part, timed on the device: with nu_l == 1 and after one round of site-rate moves."""
    b, r = _run(sc, False)
    r.repartition()
    n, _ = r.num_parts()
    out = {}
    for name in ("all_one_rates", "drawn_rates"):
        if name == "drawn_rates":
            r.site_rate_moves()
        ms = []
        for _ in range(4):
            r.run_moves(n * 1000); b.synchronize(); ms.append(b.last_run_ms())
        out[name] = {"pass_ms": min(ms[1:]), "moves_per_s": n * 1000 / (min(ms[1:]) * 1e-3), "parts": n}
    r.close(); b.close()
    return out


def main():
    if len(sys.argv) > 1:
        from delphy_amd.scenarios import make_scenario
        sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
        step = sys.argv[1]
        out = step_phases(sc) if step == "phases" else step_cycles(sc, step == "cycles_on") if step in ("cycles_off", "cycles_on") else step_pass(sc)
        print("RESULT " + json.dumps(out), flush=True)
        return 0
    import delphy_amd as d
    line = {"workload": os.environ.get("EMAT_WORKLOAD", "C4"), "build_id": d.source_build_id()}
    for step, limit in STEPS.items():                                   # one after the other; a step that fails or runs out of time ends the probe
        env = dict(os.environ, EMAT_VERBOSE="spans") if step == "phases" else dict(os.environ)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print("site_rate_probe: step %s ended with status %d; nothing further is started" % (step, p.returncode), file=sys.stderr)
            return p.returncode
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        if step == "phases":                                            # the engine call's own stretches: mean microseconds per call, from the spans table
            spans = {m.group(1).strip(): float(m.group(2)) / 1e3 for m in re.finditer(r"\[emat\]\s+(site_rate_moves: .*?)\s+[\d.]+\s+\d+\s+([\d.]+)\s+[\d.]+\s*$", p.stderr, re.M)}
            res["engine_call_by_phase_ms"] = spans
        line[step] = res
    line["num_sites"] = 29903 if line["workload"] == "C4" else None
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "site_rate_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
