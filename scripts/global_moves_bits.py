"""The bits the five groups of global moves give (site rates, Skygrid, Exponential population, substitution model, APOBEC model), as SHA-256 digests: to compare two builds of the
library on one device (the loaded one is the one at EMAT_LIB_PATH, or the tree's own).  Only the public API of delphy_amd/engine.py is used.

A digest is over the bytes of everything a call returns: every scalar, the curve, the trace, the rates; a refusal gives the digest of its text.

  tree / host      per (tips 2, 33, 600) x (cells 1, 7, 400): emat_tree_coalescent_stats, then both population groups on the resident tree and on
                   the statistics downloaded from it.  Skygrid: 1 (refused), 2 and 33 knots x both types x barrier on and off x 0, 1 and 25
                   leapfrog steps.  Exponential: 0, 1 and 50 rounds x g just above and just below 0 (the steps cross it) x min_pop 0 and above.
  synthetic        host statistics with max(num_inner, num_cells) at 1 024 and 1 025, either side of the second workgroup
  site rates       L = 255, 256, 257 and the scenario's own, with 0 and 10 alpha steps, two calls on one handle
  parts            per tips 33 and 600, 300 sites cut into parts: the substitution-model moves under 1, 2 and 4 site partitions and the APOBEC model's under 2, with 0, 1
                   and 50 rounds and with each switch off in turn, on the parts' own statistics and on those downloaded from them; the model before every call
                   is the one the parts went out under.  Each call's result, then emat_get_evo
  run              three cycles of do_mcmc_steps per group on 33 and 600 tips, tree in HBM: the group's parameters after each cycle and tree()

    python scripts/global_moves_bits.py > digests.json        # {"emat_build_id": ..., "digests": {case: sha256}}
    python scripts/global_moves_bits.py --compare parent_a.json parent_b.json new.json > profiles/global_moves_bits_latest.json
        (a case on which the parent's two runs differ is dropped and listed; exit status 1 when a remaining digest differs)
"""
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import delphy_amd as d  # noqa: E402
from delphy_amd.scenarios import make_scenario  # noqa: E402

TIPS, CELLS = (2, 33, 600), (1, 7, 400)


def digest(call):
    h = hashlib.sha256()
    try:
        res = call()
        parts = res if isinstance(res, tuple) else (dataclasses.asdict(res) if dataclasses.is_dataclass(res) else vars(res)).values()
        for a in parts:
            if a is not None: h.update(np.ascontiguousarray(a).tobytes())
    except d.EmatError as e:
        h.update(str(e).encode())
    return h.hexdigest()


def sky_cases(t_lo, t_hi):
    for knots in (1, 2, 33):
        for log_linear in (False, True):
            x = np.linspace(t_lo - 1.0, t_hi, knots) if knots > 1 else np.array([t_hi])
            pop = d.PopModel.skygrid(x, 1.0 + 0.4 * np.sin(np.arange(float(knots))), log_linear)
            for barrier in (False, True):
                for steps in (0, 1, 25):
                    yield "Skygrid %d knots, %s, barrier %s, %d steps" % (knots, "log-linear" if log_linear else "staircase", "on" if barrier else "off", steps), pop, \
                        d.SkygridSpec(tau=1.5, low_gamma_barrier_enabled=barrier, hmc_steps=steps)


def xp_cases(t_hi, span):
    for rounds in (0, 1, 50):
        for g in (0.02 / span, -0.02 / span):
            for min_pop in (0.0, 1.5):
                yield "Exponential %d rounds, g %+.0e / span, min_pop %g" % (rounds, g * span, min_pop), d.PopModel.exp(t_hi, 3.0, g, min_pop), \
                    d.ExpPopSpec(inv_n0_prior_alpha=0.5, inv_n0_prior_beta=0.5, rounds=rounds)


def population_groups(out):
    for tips in TIPS:
        sc = make_scenario("C1", num_tips=tips, num_sites=60)
        t = np.asarray(sc.tree.t); t_max, span = float(t.max()), float(t.max() - t.min())
        b = d.EmatBackend(sc.num_sites)
        try:
            b.tree_upload(sc.tree)
            for cells in CELLS:
                t_step = span / (cells - 0.75); t_ref = t_max + 0.25 * t_step       # the latest tip in cell -1, the root in cell -cells
                where = "tips %d, cells %d: " % (tips, cells)
                first, k_bar, inner_t = b.tree_coalescent_stats(t_ref, t_step)
                assert (first, len(k_bar), len(inner_t)) == (-cells, cells, tips - 1), (first, len(k_bar), len(inner_t))
                out[where + "tree_coalescent_stats"] = digest(lambda: b.tree_coalescent_stats(t_ref, t_step))
                for key, (name, pop, spec) in enumerate(sky_cases(t_max - span, t_ref)):
                    out[where + name + ", tree"] = digest(lambda: b.tree_skygrid_moves(pop, spec, t_ref, t_step, key=key, trace=True))
                    out[where + name + ", host"] = digest(lambda: b.skygrid_moves(pop, spec, t_ref, t_step, first, k_bar, inner_t, key=key, trace=True))
                for key, (name, pop, spec) in enumerate(xp_cases(t_ref, span)):
                    out[where + name + ", tree"] = digest(lambda: b.tree_exp_pop_moves(pop, spec, t_ref, t_step, key=key, trace=True))
                    out[where + name + ", host"] = digest(lambda: b.exp_pop_moves(pop, spec, t_ref, t_step, first, k_bar, inner_t, key=key, trace=True))
        finally:
            b.close()
    b = d.EmatBackend(60)
    try:
        for n_cells, n_inner in ((1024, 1024), (1025, 7), (7, 1025), (1025, 1025)):
            where = "synthetic %d cells, %d inner nodes: " % (n_cells, n_inner)
            t_step = 4.0 / n_cells
            k_bar = 1.0 + (np.arange(n_cells) % 5); inner_t = -np.linspace(0.25 * t_step, 4.0 - 0.25 * t_step, n_inner)
            for name, pop, spec in list(sky_cases(-4.0, 0.0))[-6:]:
                out[where + name] = digest(lambda: b.skygrid_moves(pop, spec, 0.0, t_step, -n_cells, k_bar, inner_t, key=21, trace=True))
            for name, pop, spec in list(xp_cases(0.0, 4.0))[-4:]:
                out[where + name] = digest(lambda: b.exp_pop_moves(pop, spec, 0.0, t_step, -n_cells, k_bar, inner_t, key=22, trace=True))
    finally:
        b.close()


def site_rates(out):
    sc = make_scenario("C1", num_tips=33, num_sites=300)
    for L in (255, 256, 257, sc.num_sites):
        rng = np.random.default_rng(L)
        T = rng.uniform(0.5, 40.0, L); M = rng.poisson(1.5, L).astype(np.int32)
        for steps in (0, 10):
            b = d.EmatBackend(L)
            try:
                b.set_ref_sequence(np.zeros(L, np.uint8)); b.set_hky(1e-3, 2.0, [0.3, 0.2, 0.2, 0.3], rng.gamma(2.0, 0.5, L))
                for call in (1, 2):
                    what = "site rates L %d, %d alpha steps, call %d" % (L, steps, call)
                    out[what] = digest(lambda: b.site_rate_moves(T, M, 0.8, steps, key=100 * call + steps, trace=steps > 0 and call == 1))
                    out[what + ": nu_l"] = digest(lambda: (b.nu_l(),))
            finally:
                b.close()


def parts_groups(out):
    for tips in (33, 600):
        sc = make_scenario("C1", num_tips=tips, num_sites=300)
        cutter = d.EmatRun(None, sc.tree, sc.ref, 9)                                 # the product's host driver cuts the tree (no device needed)
        try:
            cutter.set_num_parts(4 if tips > 100 else 3); cutter.repartition()
            n, root_part = cutter.num_parts()
            parts, incl, seeds = zip(*[cutter.part(i) for i in range(n)])
            ref = cutter.tree()[1]
        finally:
            cutter.close()
        L = sc.num_sites
        models = [("subst", P, ([sc.mu] * P, [sc.pi] * P, [d.hky_q_matrix(sc.kappa + p, sc.pi) for p in range(P)], np.ones(L), np.arange(L) % P)) for P in (1, 2, 4)]
        models.append(("mpox", 2, ([sc.mu] * 2, [[0.25] * 4] * 2, list(d.engine.mpox_q_matrices(0.5)), np.ones(L), np.arange(L) % 2)))
        for group, P, evo in models:
            b = d.EmatBackend(L)
            try:
                b.set_ref_sequence(ref); b.set_evo(*evo); b.set_flags(sc.t_max_tip, False, True)
                b.upload_parts(list(parts), list(incl), list(seeds)); b.build_coalescent_parts(sc.pop, root_part, sc.default_t_step())
                where = "parts %s, tips %d, %d site partitions: " % (group, tips, P)
                out[where + "parts_subst_stats"] = digest(lambda: b.parts_subst_stats(P))
                T, M, Cn = b.parts_subst_stats(P)
                if group == "subst":
                    base = d.SubstSpec(mu=sc.mu, kappa=sc.kappa, pi=tuple(sc.pi))
                    specs = [("%d rounds" % r, dataclasses.replace(base, rounds=r)) for r in (0, 1, 50)] + [(sw + " off", dataclasses.replace(base, **{sw: False})) for sw in ("do_mu", "do_pi", "do_kappa")]
                    calls = {"host": lambda sp, key: b.subst_moves(sp, T, M, Cn, key=key, trace=True), "parts": lambda sp, key: b.parts_subst_moves(sp, key=key, trace=True)}
                else:
                    base = d.MpoxSpec(mu=sc.mu, mu_star=0.5 * sc.mu)
                    specs = [("%d rounds" % r, dataclasses.replace(base, rounds=r)) for r in (0, 1, 50)] + [("do_mu off", dataclasses.replace(base, do_mu=False))]
                    calls = {"host": lambda sp, key: b.mpox_moves(sp, T, M, key=key, trace=True), "parts": lambda sp, key: b.parts_mpox_moves(sp, key=key, trace=True)}
                for key, (name, sp) in enumerate(specs):
                    for source, call in calls.items():
                        b.set_evo(*evo)
                        out[where + name + ", " + source] = digest(lambda: call(sp, 40 + key))
                        out[where + name + ", " + source + ": get_evo"] = digest(lambda: b.get_evo())
            finally:
                b.close()


def run_cycles(out):
    groups = {"site rates": ("C1", lambda r: r.set_site_rate_moves(True, 1.0), lambda r: (np.float64(r.site_rates()[0]), r.site_rates()[1])),
              "Skygrid": ("C3", lambda r: r.set_skygrid_moves(True, d.SkygridSpec(tau=2.0, low_gamma_barrier_enabled=True)), lambda r: (r.skygrid()[0], np.float64(r.skygrid()[1]))),
              "Exponential": ("C2", lambda r: r.set_exp_pop_moves(True, d.ExpPopSpec(inv_n0_prior_alpha=1.0, inv_n0_prior_beta=50.0)), lambda r: (np.asarray(r.exp_pop()),)),
              "substitution model": ("C1", lambda r: r.set_subst_moves(True, d.SubstSpec()), lambda r: (np.float64(r.hky()[:2]), r.hky()[2])),
              "APOBEC model": ("C1", lambda r: r.set_mpox(True, d.MpoxSpec()), lambda r: (np.float64(r.mpox()),))}
    for tips in (33, 600):
        for group, (kind, switch_on, params) in groups.items():
            sc = make_scenario(kind, num_tips=tips, num_sites=300, **(dict(skygrid_log_linear=True) if kind == "C3" else {}))
            b = d.EmatBackend(sc.num_sites)
            run = d.EmatRun(b, sc.tree, sc.ref, 17)
            try:
                run.set_num_parts(4 if tips > 100 else 2); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
                switch_on(run)
                for cycle in range(3):
                    run.do_mcmc_steps(10 * sc.tree.num_nodes, 10 * sc.tree.num_nodes)
                    out["run %s, %d tips, cycle %d: parameters" % (group, tips, cycle + 1)] = digest(lambda: params(run))
                tree, ref = run.tree()
                out["run %s, %d tips: tree()" % (group, tips)] = digest(lambda: tuple(getattr(tree, f) for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t")) + (ref,))
            finally:
                run.close(); b.close()


def main():
    out = {}
    population_groups(out); site_rates(out); parts_groups(out); run_cycles(out)
    print(json.dumps({"emat_build_id": d.library_build_id(), "digests": out}, indent=1))


def compare(a1, a2, b):
    A1, A2, B = (json.load(open(f)) for f in (a1, a2, b))
    unstable = sorted(k for k in A1["digests"] if A1["digests"][k] != A2["digests"].get(k))
    differing = sorted(k for k in set(A1["digests"]) | set(B["digests"]) if k not in unstable and A1["digests"].get(k) != B["digests"].get(k))
    print(json.dumps({"cases": len(A1["digests"]), "dropped_because_the_parents_two_runs_differ": unstable, "differing": differing,
                      "emat_build_id": {"parent": A1["emat_build_id"], "new": B["emat_build_id"]}, "digests": B["digests"]}, indent=1))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:5]) if len(sys.argv) > 1 and sys.argv[1] == "--compare" else main())
