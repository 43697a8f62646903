"""What one round of the substitution-model moves (the mu draw and 10 rounds: 20 Metropolis steps) costs at C4 (100 000 tips, about 8 000 parts out
on the device), as one JSON line into profiles/subst_moves_probe_latest.json:
  round    in ONE process, 30 repeats each, median and p10-p90 in milliseconds (wall time, measured WITHOUT spans):
             device   emat_parts_subst_moves: the statistics of the parts reduced on the device, the chain in one launch, one small copy back
             host     the same round from the calls there were before: emat_get_global_stats (one 81-double row per part to the host, summed
                      there), the moves on the host (this file's restatement in plain Python floats: INTERPRETED, a compiled host would spend
                      microseconds on them -- read the host route without its "moves" share beside the device's), emat_set_evo (the whole model, its
                      L-long site arrays re-sent); the root's state counts, which those calls do not give, are taken once beforehand
                      (emat_parts_subst_stats) and not timed
             the two are measured alternately, a device round then a host round, and both leave the handle with a model of the same kind
  phases   the device rounds in a second child under EMAT_VERBOSE=spans: the call by phase, mean over all calls
  cycles   whole cycles per second over 40 cycles of the run driver, tree in HBM, with the group off and on, three runs of each, alternating
Usage:
  python scripts/subst_moves_probe.py          every step as a child process under its own time limit, one after the other, stopping at the first
                                               that fails; then the JSON line
  python scripts/subst_moves_probe.py STEP     one step in this process: round | cycles_off | cycles_on   (prints its own JSON)"""
import json
import math
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


def _q(kappa, pi):
    r = [[0.0 if a == b else (kappa if (a ^ b) == 2 else 1.0) for b in range(4)] for a in range(4)]
    R = sum(pi[a] * r[a][b] * pi[b] for a in range(4) for b in range(4))
    q = [[r[a][b] / R * pi[b] for b in range(4)] for a in range(4)]
    for a in range(4):
        q[a][a] = -sum(q[a][b] for b in range(4) if b != a)
    return q


def host_moves(mu, kappa, pi, T, M, C, rng, rounds=ROUNDS):
    """Run::mu_move, then `rounds` times hky_frequencies_move and hky_kappa_move (reference run.cpp:781-821, :953-1103) on one site partition, in plain
    Python floats: what a host that makes these moves itself runs between emat_get_global_stats and emat_set_evo."""
    pi = list(pi); q = _q(kappa, pi)
    nm = sum(M[a][b] for a in range(4) for b in range(4) if a != b)
    mu = rng.gammavariate(nm + 1.0, 1.0 / sum(-q[a][a] * T[a] for a in range(4)))

    def delta(qn, pn):
        v = -sum(mu * (-qn[a][a] + q[a][a]) * T[a] for a in range(4))
        if pn is not None:
            v += sum(C[a] * math.log(pn[a] / pi[a]) for a in range(4) if C[a] > 0)
        return v + sum(M[a][b] * math.log(qn[a][b] / q[a][b]) for a in range(4) for b in range(4) if a != b and M[a][b] > 0)
    for _ in range(rounds):
        d = rng.uniform(0.0, 0.01); ia = rng.randrange(4); ib = (ia + 1 + rng.randrange(3)) % 4
        pn = list(pi); pn[ia] += d; pn[ib] -= d
        if 0.0 < pn[ia] < 1.0 and 0.0 < pn[ib] < 1.0:
            qn = _q(kappa, pn); lp = delta(qn, pn)
            if lp > 0 or rng.random() < math.exp(lp):
                pi, q = pn, qn
        scale = rng.uniform(0.75, 1.0 / 0.75); kn = kappa * scale
        qn = _q(kn, pi)
        lp = delta(qn, None) + (-(math.log(kn) - 1.0) ** 2 + (math.log(kappa) - 1.0) ** 2) / (2 * 1.25 ** 2) + 2.0 * math.log(kappa / kn)
        if lp > 0 or rng.random() < math.exp(lp):
            kappa, q = kn, qn
    return mu, kappa, pi, q


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
    r.repartition()
    n_parts, _ = r.num_parts()
    L = sc.num_sites
    nu, pfs = np.ones(L), np.zeros(L, np.int32)
    _, _, C = b.parts_subst_stats()
    rng = random.Random(7)
    mu, kappa, pi = sc.mu, sc.kappa, list(sc.pi)
    dev, host, host_parts = [], [], {"get_global_stats": [], "moves": [], "set_evo": []}
    for k in range(REPEATS + 1):
        t0 = time.perf_counter()
        res = b.parts_subst_moves(d.SubstSpec(mu=mu, kappa=kappa, pi=tuple(pi), rounds=ROUNDS), key=1000 + k)
        t1 = time.perf_counter()
        T, M, _ = b.global_stats(1)
        t2 = time.perf_counter()
        mu, kappa, pi, q = host_moves(res.mu, res.kappa, res.pi, T[0].tolist(), M[0].tolist(), C.tolist(), rng)
        t3 = time.perf_counter()
        b.set_evo([mu], [pi], [q], nu, pfs)
        t4 = time.perf_counter()
        if k:                                                       # the first round of each pays its allocations
            dev.append((t1 - t0) * 1e3); host.append((t4 - t1) * 1e3)
            for name, dt in (("get_global_stats", t2 - t1), ("moves", t3 - t2), ("set_evo", t4 - t3)):
                host_parts[name].append(dt * 1e3)
    out = {"num_parts": int(n_parts), "num_sites": int(L), "rounds": ROUNDS, "device": _summary(dev), "host": _summary(host),
           "host_by_call": {k: _summary(v) for k, v in host_parts.items()}, "bytes_to_host": {"device": 21 * 8, "host": int(n_parts) * 81 * 8},
           "bytes_to_device_by_the_call": {"device": 0, "host": int(L) * (8 + 4) + 21 * 8}, "mu": mu, "kappa": kappa, "pi": list(pi)}
    r.reassemble(); r.close(); b.close()
    return out


def step_cycles(on):
    d, sc, b, r = _run_with_parts_out()
    if on:
        r.set_subst_moves(True, d.SubstSpec(rounds=ROUNDS))
    per_cycle = 50 * sc.tree.num_nodes
    r.do_mcmc_steps(2 * per_cycle, per_cycle); b.synchronize()
    t0 = time.perf_counter()
    r.do_mcmc_steps(CYCLES * per_cycle, per_cycle); b.synchronize()
    dt = time.perf_counter() - t0
    out = {"cycles": CYCLES, "cycles_per_s": CYCLES / dt, "ms_per_cycle": dt / CYCLES * 1e3}
    if on:
        mu, kappa, pi = r.hky()
        out.update({"mu": mu, "kappa": kappa, "pi": pi.tolist()})
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
            print("subst_moves_probe: step %s ended with status %d; nothing further is started" % (name, p.returncode), file=sys.stderr)
            return p.returncode
        if spans:   # the engine call's own stretches over all calls: mean milliseconds per call, from the spans table
            line["engine_call_by_phase_ms_over_all_calls"] = {m.group(1).strip(): float(m.group(2)) / 1e3
                                                              for m in re.finditer(r"\[emat\]\s+(subst_moves: .*?)\s+[\d.]+\s+\d+\s+([\d.]+)\s+[\d.]+\s*$", p.stderr, re.M)}
            continue
        result = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        if name == "round":
            line[name] = result
        else:
            line[name].append(result)
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "subst_moves_probe_latest.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
