"""What one call of the APOBEC (mpox) model's moves (10 rounds of the Gibbs draws of mu and rho = mu* / mu) costs at C4 (100 000 tips, about 8 000 parts
out on the device, the sites split in two by the APOBEC context of the sequence at node 0), as one JSON line into profiles/mpox_moves_probe_latest.json:
  round    in ONE process, 30 repeats each, median and p10-p90 in milliseconds (wall time, measured WITHOUT spans):
             device   emat_parts_mpox_moves: the statistics of the parts reduced on the device, the rounds in one launch, one small copy back
             host     the same round from the calls there were before: emat_get_global_stats (one 81-double row per part to the host, summed
                      there), the draws on the host (this file's restatement: Python's gammavariate and scipy's incomplete gamma function, a few
                      dozen microseconds a round), emat_set_evo (the whole two-partition model, its L-long site arrays re-sent)
             the two are measured alternately, a device round then a host round, and both leave the handle with a model of the same kind
  phases   the device rounds in a second child under EMAT_VERBOSE=spans: the call by phase, mean over all calls
  cycles   whole cycles per second over 40 cycles of the run driver, tree in HBM, with the model off and on, three runs of each, alternating
Usage:
  python scripts/mpox_moves_probe.py          every step as a child process under its own time limit, one after the other, stopping at the first
                                              that fails; then the JSON line
  python scripts/mpox_moves_probe.py STEP     one step in this process: round | cycles_off | cycles_on   (prints its own JSON)"""
import json
import os
import random
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT_S, REPEATS, ROUNDS = 300, 30, 10
SEED, PARTS, CYCLES, CYCLE_RUNS = 20261001, 8192, 40, 3


def host_moves(mu, mu_star, T, M, rng, rounds=ROUNDS):
    """Run::mpox_hack_moves (reference run.cpp:823-951) in Python floats: what a host that makes these draws itself runs between emat_get_global_stats and
    emat_set_evo.  Returns (mu, mu*, q0, q1)."""
    import scipy.special as sp
    nm = sum(M[p][a][b] for p in range(2) for a in range(4) for b in range(4) if a != b)
    m_star = M[1][1][3] + M[1][2][0]
    tt = sum(T[p][a] for p in range(2) for a in range(4)); ts = T[1][1] + T[1][2]
    for _ in range(rounds):
        rho = mu_star / mu
        mu = rng.gammavariate(nm + 1.0 - 1.0, 1.0 / (tt + 2 * rho * ts))
        if ts > 0.0:
            alpha, beta = m_star + 1.0, mu * ts / 3
            q_hi = float(sp.gammaincc(alpha, beta))
            if q_hi > 0.0:
                k = max(1.0, float(sp.gammainccinv(alpha, q_hi * (1.0 - rng.random()))) / beta)
                mu_star = mu * (k - 1.0) / 6.0
    rho = mu_star / mu
    q0 = [[-1.0 if a == b else 1.0 / 3.0 for b in range(4)] for a in range(4)]
    q1 = [row[:] for row in q0]
    q1[1][3] += 2 * rho; q1[1][1] -= 2 * rho; q1[2][0] += 2 * rho; q1[2][2] -= 2 * rho
    return mu, mu_star, q0, q1


def _summary(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "repeats": len(ms)}


def _run_with_parts_out():
    import delphy_amd as d
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario(os.environ.get("EMAT_WORKLOAD", "C4"))
    b = d.EmatBackend(sc.num_sites)
    r = d.EmatRun(b, sc.tree, sc.ref, SEED)
    r.set_num_parts(PARTS); r.set_max_part_nodes(-1); r.set_hky(sc.mu, sc.kappa, sc.pi); r.set_pop_model(sc.pop); r.set_device_tree(True)
    return d, sc, b, r


def step_round():
    d, sc, b, r = _run_with_parts_out()
    r.set_mpox(True, d.MpoxSpec(rounds=ROUNDS))
    r.repartition()
    n_parts, _ = r.num_parts()
    L = sc.num_sites
    pfs, context_sites = r.mpox_partition()
    nu, pi = np.ones(L), [[0.25] * 4] * 2
    rng = random.Random(7)
    mu, mu_star = sc.mu, 0.0
    dev, host, host_parts = [], [], {"get_global_stats": [], "moves": [], "set_evo": []}
    for k in range(REPEATS + 1):
        t0 = time.perf_counter()
        res = b.parts_mpox_moves(d.MpoxSpec(mu=mu, mu_star=mu_star, rounds=ROUNDS), key=1000 + k)
        t1 = time.perf_counter()
        T, M, _ = b.global_stats(2)
        t2 = time.perf_counter()
        mu, mu_star, q0, q1 = host_moves(res.mu, res.mu_star, T.tolist(), M.tolist(), rng)
        t3 = time.perf_counter()
        b.set_evo([mu, mu], pi, [q0, q1], nu, pfs)
        t4 = time.perf_counter()
        if k:                                                       # the first round of each pays its allocations
            dev.append((t1 - t0) * 1e3); host.append((t4 - t1) * 1e3)
            for name, dt in (("get_global_stats", t2 - t1), ("moves", t3 - t2), ("set_evo", t4 - t3)):
                host_parts[name].append(dt * 1e3)
    out = {"num_parts": int(n_parts), "num_sites": int(L), "sites_with_apobec_context": int(context_sites), "rounds": ROUNDS, "device": _summary(dev), "host": _summary(host),
           "host_by_call": {k: _summary(v) for k, v in host_parts.items()}, "bytes_to_host": {"device": 13 * 8, "host": int(n_parts) * 81 * 8},
           "bytes_to_device_by_the_call": {"device": 0, "host": int(L) * (8 + 4) + 2 * 21 * 8}, "mu": mu, "mu_star": mu_star, "M": res.M, "M_star": res.M_star,
           "rho_degenerate": int(res.rho_degenerate), "rho_skipped": int(res.rho_skipped)}
    r.reassemble(); r.close(); b.close()
    return out


def step_cycles(on):
    d, sc, b, r = _run_with_parts_out()
    if on:
        r.set_mpox(True, d.MpoxSpec(rounds=ROUNDS))
    per_cycle = 50 * sc.tree.num_nodes
    r.do_mcmc_steps(2 * per_cycle, per_cycle); b.synchronize()
    t0 = time.perf_counter()
    r.do_mcmc_steps(CYCLES * per_cycle, per_cycle); b.synchronize()
    dt = time.perf_counter() - t0
    out = {"cycles": CYCLES, "cycles_per_s": CYCLES / dt, "ms_per_cycle": dt / CYCLES * 1e3}
    if on:
        mu, mu_star = r.mpox()
        out.update({"mu": mu, "mu_star": mu_star})
    r.close(); b.close()
    return out


def main():
    if len(sys.argv) > 1:
        step = sys.argv[1]
        print("RESULT " + json.dumps(step_round() if step == "round" else step_cycles(step == "cycles_on")), flush=True)
        return 0
    import delphy_amd as d
    line = {"workload": os.environ.get("EMAT_WORKLOAD", "C4"), "build_id": d.source_build_id(), "date": time.strftime("%Y-%m-%d"), "cycles_off": [], "cycles_on": []}
    steps = [("round", "round", False), ("phases", "round", True)] + [(s, s, False) for _ in range(CYCLE_RUNS) for s in ("cycles_off", "cycles_on")]
    for name, step, spans in steps:
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), step], env=dict(os.environ, EMAT_VERBOSE="spans") if spans else dict(os.environ),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print("mpox_moves_probe: step %s ended with status %d; nothing further is started" % (name, p.returncode), file=sys.stderr)
            return p.returncode
        if spans:   # the engine call's own stretches over all calls: mean milliseconds per call, from the spans table
            line["engine_call_by_phase_ms_over_all_calls"] = {m.group(1).strip(): float(m.group(2)) / 1e3
                                                              for m in re.finditer(r"\[emat\]\s+(mpox_moves: .*?)\s+[\d.]+\s+\d+\s+([\d.]+)\s+[\d.]+\s*$", p.stderr, re.M)}
            continue
        result = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        if name == "round":
            line[name] = result
        else:
            line[name].append(result)
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mpox_moves_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
