"""What the global moves (site rates, Skygrid, Exponential population) refuse, and in which words: status and last-error text of the backend's
entry points on a handle without a device and of the run driver's calls on a run without a backend, against the table recorded from the library
BEFORE the three groups' rules got one owner each (tests/golden/make_global_moves_refusals.py).  The arguments are every case of
test_site_rate_abi.py, test_skygrid_moves_abi.py and test_exp_pop_moves_abi.py, and calls with two faults that pin which one is named.  No GPU."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_moves_refusals.json")
INF, NAN = float("inf"), float("nan")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
L_SITES = 40

# The one deliberate change of text: the run driver's setters used to restate the backend's spec checks in their own words, several tests to
# a message; they now refuse in the backend's words behind their own name.  Status as recorded; text: the setter's name + the backend's text.
SETTER_ROWS = {
    "run set_skygrid hmc_steps=-2": ("emat_run_set_skygrid_moves", "sky spec hmc_steps=-2"),
    "run set_skygrid hmc_mean_dt=-1.0": ("emat_run_set_skygrid_moves", "sky spec hmc_mean_dt=-1.0"),
    "run set_exp_pop g_prior_mu=nan": ("emat_run_set_exp_pop_moves", "xp spec g_prior_mu=nan"),
    "run set_exp_pop inv_n0_prior_alpha=inf": ("emat_run_set_exp_pop_moves", "xp spec inv_n0_prior_alpha=inf"),
    "run set_exp_pop inv_n0_prior_beta=nan": ("emat_run_set_exp_pop_moves", "xp spec inv_n0_prior_beta=nan"),
}


def _dbl(a):
    return None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(DP)


class _Recorder:
    def __init__(self):
        self.lib = d.load_library()
        self.table = {}
        self.keep = []                                   # arrays the C structs point into

    def backend(self, name, h, fn, *args):
        st = int(getattr(self.lib, fn)(h, *args))
        self.table[name] = [st, self.lib.emat_last_error(h).decode() if st != 0 and h is not None else ""]

    def run(self, name, r, fn, *args):
        st = int(getattr(self.lib, fn)(r, *args))
        self.table[name] = [st, self.lib.emat_run_last_error(r).decode() if st != 0 and r is not None else ""]


# ---- the Skygrid group --------------------------------------------------------------------------------------------------------------------
def _sky_good():
    return dict(pop=d.PopModel.skygrid([-3.0, -2.0, -1.0], [1.0, 2.0, 1.5], True), spec=d.SkygridSpec(low_gamma_barrier_enabled=True), t_ref=0.0, t_step=0.5, first_cell=-8,
                k_bar=np.linspace(1.0, 4.0, 8), inner_t=np.array([-3.9, -2.0, -0.01]), trace_capacity=None)


def _sky_spec(**kw):
    return dataclasses.replace(_sky_good()["spec"], **kw)


def _sky_result(rec, a, gamma=True):
    n = max(1, int(a["pop"].c_struct().skygrid_num_knots)) if a["pop"].kind == 2 else 1
    res = engine._SkygridResultC()
    if gamma:
        g = np.zeros(n); rec.keep.append(g); res.gamma = _dbl(g)
    if a["trace_capacity"] is not None:
        tr = np.zeros((5 + 4 * max(0, a["trace_capacity"]), n)); rec.keep.append(tr); res.trace = _dbl(tr); res.trace_capacity = a["trace_capacity"]
    return res


def _sky(rec, name, h, tree=False, null=(), gamma=True, **kw):
    a = _sky_good(); a.update(kw)
    m = a["pop"].c_struct(); sp = a["spec"].c_struct(); res = _sky_result(rec, a, gamma)
    kb = np.ascontiguousarray(a["k_bar"], np.float64); ts = np.ascontiguousarray(a["inner_t"], np.float64)
    ptr = lambda what, p: None if what in null else p                                    # noqa: E731
    head = [None if "h" in null else h, ptr("m", C.byref(m)), ptr("sp", C.byref(sp)), float(a["t_ref"]), float(a["t_step"])]
    stats = [] if tree else [int(a["first_cell"]), kb.shape[0], ptr("kb", _dbl(kb)), ts.shape[0], ptr("ts", _dbl(ts))]
    rec.backend(name, head[0], "emat_tree_skygrid_moves" if tree else "emat_skygrid_moves", *head[1:], *stats, 5, ptr("res", C.byref(res)))


SKY_REFUSALS = [
    ("pop=const", dict(pop=d.PopModel.const(3.0))), ("pop=exp", dict(pop=d.PopModel.exp(0.0, 3.0, 0.1))), ("pop=one knot", dict(pop=d.PopModel.skygrid([0.0], [1.0]))),
    ("pop=equal knots", dict(pop=d.PopModel.skygrid([0.0, 0.0], [1.0, 1.0]))), ("pop=nan gamma", dict(pop=d.PopModel.skygrid([0.0, 1.0, 2.0], [1.0, NAN, 1.0]))),
] + [("spec %s=%r" % (k, v), dict(spec=_sky_spec(**{k: v}))) for k, v in (("tau", 0.0), ("tau", -1.0), ("tau", NAN), ("tau", INF), ("low_gamma_barrier_scale", 0.0), ("low_gamma_barrier_scale", -0.3),
                                                                            ("hmc_steps", -1), ("hmc_steps", -2), ("hmc_mean_dt", 0.0), ("hmc_mean_dt", -0.1), ("hmc_mean_dt", -1.0))] + [
    ("t_step=0", dict(t_step=0.0)), ("t_ref=nan", dict(t_ref=NAN)), ("no cells", dict(k_bar=np.zeros(0))), ("no inner nodes", dict(inner_t=np.zeros(0))),
    ("k_bar negative", dict(k_bar=np.array([1.0, 2.0, -1e-300, 3.0, -1.0, 1.0, 1.0, 1.0]))), ("k_bar inf", dict(k_bar=np.array([1.0, 2.0, 2.0, 3.0, INF, NAN, 1.0, 1.0]))),
    ("inner_t nan", dict(inner_t=np.array([-3.9, NAN, INF]))), ("inner_t after the grid", dict(inner_t=np.array([-3.9, -2.0, 0.0]))), ("inner_t before the grid", dict(inner_t=np.array([-4.0000001, -2.0, -0.1]))),
]
BIG = (1 << 22) + 1
FAR = [("cells beyond +2^30", dict(first_cell=(1 << 30) - 4, inner_t=np.array([0.5 * ((1 << 30) - 2)]))), ("cells beyond -2^30", dict(first_cell=-(1 << 30) - 8, inner_t=np.array([0.5 * (-(1 << 30) - 4)])))]
BAD_ORIGINS = ((NAN, 1.0), (0.0, 0.0), (0.0, INF))


def _skygrid_rows(rec, h):
    knots = lambda n: d.PopModel.skygrid(np.arange(float(n)), np.ones(n))               # noqa: E731
    _sky(rec, "sky good", h); _sky(rec, "sky good, trace", h, trace_capacity=25)
    for name, kw in SKY_REFUSALS + FAR:
        _sky(rec, "sky " + name, h, **kw)
    _sky(rec, "sky barrier off, scale 0", h, spec=_sky_spec(low_gamma_barrier_enabled=False, low_gamma_barrier_scale=0.0))
    _sky(rec, "sky 1024 knots", h, pop=knots(1024)); _sky(rec, "sky 1025 knots", h, pop=knots(1025))
    _sky(rec, "sky 2^22+1 cells", h, first_cell=-BIG, k_bar=np.ones(BIG))
    for what in ("h", "m", "sp", "kb", "ts", "res"):
        _sky(rec, "sky null " + what, h, null=(what,))
    _sky(rec, "sky null gamma", h, gamma=False); _sky(rec, "sky trace_capacity 24", h, trace_capacity=24)
    # the tree's entry points
    n = C.c_int32()
    stats = lambda name, hh, t_ref, t_step, first=True: rec.backend(name, hh, "emat_tree_coalescent_stats", t_ref, t_step, C.byref(n) if first else None, C.byref(n), None, 0, None, 0, C.byref(n))   # noqa: E731
    stats("tree_stats good", h, 0.0, 1.0); stats("tree_stats null first_cell", h, 0.0, 1.0, False); stats("tree_stats null h", None, 0.0, 1.0)
    _sky(rec, "tree_sky good, trace", h, tree=True, t_step=1.0, trace_capacity=25)
    for t_ref, t_step in BAD_ORIGINS:
        stats("tree_stats origin %r %r" % (t_ref, t_step), h, t_ref, t_step)
        _sky(rec, "tree_sky origin %r %r" % (t_ref, t_step), h, tree=True, t_ref=t_ref, t_step=t_step)
    for name, kw in (("pop=const", dict(pop=d.PopModel.const(3.0))), ("tau=0", dict(spec=_sky_spec(tau=0.0))), ("hmc_steps=-1", dict(spec=_sky_spec(hmc_steps=-1))),
                     ("hmc_mean_dt=0", dict(spec=_sky_spec(hmc_mean_dt=0.0))), ("barrier scale 0", dict(spec=_sky_spec(low_gamma_barrier_scale=0.0))), ("1025 knots", dict(pop=knots(1025)))):
        _sky(rec, "tree_sky " + name, h, tree=True, t_step=1.0, **kw)
    _sky(rec, "tree_sky nulls", h, tree=True, null=("m", "sp", "res")); _sky(rec, "tree_sky null h", h, tree=True, null=("h",)); _sky(rec, "tree_sky null gamma", h, tree=True, gamma=False)
    # two faults, the one named first pinned
    _sky(rec, "sky 2: model + spec", h, pop=d.PopModel.const(3.0), spec=_sky_spec(tau=0.0))
    _sky(rec, "sky 2: knot + origin", h, pop=d.PopModel.skygrid([0.0, 1.0, 2.0], [1.0, NAN, 1.0]), t_step=0.0)
    _sky(rec, "sky 2: origin + spec", h, t_step=0.0, spec=_sky_spec(tau=0.0))
    _sky(rec, "sky 2: spec + spec", h, spec=_sky_spec(hmc_steps=-1, hmc_mean_dt=0.0))
    _sky(rec, "sky 2: origin + trace", h, t_step=0.0, trace_capacity=24)
    _sky(rec, "sky 2: spec + trace", h, spec=_sky_spec(hmc_mean_dt=0.0), trace_capacity=24)
    _sky(rec, "sky 2: origin + statistics", h, t_ref=NAN, k_bar=np.zeros(0))
    _sky(rec, "sky 2: trace + statistics", h, trace_capacity=24, inner_t=np.zeros(0))
    _sky(rec, "sky 2: statistics + knots", h, k_bar=np.array([1.0, 2.0, -1.0, 3.0, 1.0, 1.0, 1.0, 1.0]), pop=knots(1025))
    _sky(rec, "sky 2: knots + cells", h, pop=knots(1025), first_cell=-BIG, k_bar=np.ones(BIG))
    _sky(rec, "sky 2: cells + cell numbers", h, first_cell=(1 << 30) - 4, k_bar=np.ones(BIG), inner_t=np.array([0.5 * ((1 << 30) - 2)]))
    _sky(rec, "sky 2: null + model", h, null=("kb",), pop=d.PopModel.const(3.0))
    _sky(rec, "tree_sky 2: spec + knots", h, tree=True, t_step=1.0, spec=_sky_spec(tau=0.0), pop=knots(1025))
    _sky(rec, "tree_sky 2: trace + knots", h, tree=True, t_step=1.0, trace_capacity=3, pop=knots(1025))
    # the gradient's hook
    m = _sky_good()["pop"].c_struct(); a = np.zeros(2); c = d.PopModel.const(1.0).c_struct()
    ok = [C.byref(m), 3, 0, 2, _dbl(a), _dbl(a), _dbl(a)]
    rec.backend("gradient good", h, "emat_debug_pop_gradient", *ok)
    for i, v in ((0, None), (4, None), (5, None), (6, None), (1, 2), (1, 5), (2, -1), (2, 3), (3, -1)):
        bad = list(ok); bad[i] = v
        rec.backend("gradient arg %d = %r" % (i, v), h, "emat_debug_pop_gradient", *bad)
    rec.backend("gradient pop=const", h, "emat_debug_pop_gradient", C.byref(c), *ok[1:])


# ---- the Exponential group ----------------------------------------------------------------------------------------------------------------
def _xp_good():
    return dict(pop=d.PopModel.exp(0.0, 3.0, 0.1, 0.5), spec=d.ExpPopSpec(), t_ref=0.0, t_step=0.5, first_cell=-8, k_bar=np.linspace(1.0, 4.0, 8), inner_t=np.array([-3.9, -2.0, -0.01]),
                trace_capacity=None)


def _xp_spec(**kw):
    return dataclasses.replace(_xp_good()["spec"], **kw)


def _xp(rec, name, h, tree=False, null=(), **kw):
    a = _xp_good(); a.update(kw)
    m = a["pop"].c_struct(); sp = a["spec"].c_struct(); res = engine._ExpPopResultC()
    if a["trace_capacity"] is not None:
        tr = np.zeros(max(1, a["trace_capacity"]), engine.EXP_POP_STEP_DTYPE); rec.keep.append(tr)
        res.trace = tr.ctypes.data_as(C.POINTER(engine._ExpPopStepC)); res.trace_capacity = a["trace_capacity"]
    kb = np.ascontiguousarray(a["k_bar"], np.float64); ts = np.ascontiguousarray(a["inner_t"], np.float64)
    ptr = lambda what, p: None if what in null else p                                    # noqa: E731
    head = [None if "h" in null else h, ptr("m", C.byref(m)), ptr("sp", C.byref(sp)), float(a["t_ref"]), float(a["t_step"])]
    stats = [] if tree else [int(a["first_cell"]), kb.shape[0], ptr("kb", _dbl(kb)), ts.shape[0], ptr("ts", _dbl(ts))]
    rec.backend(name, head[0], "emat_tree_exp_pop_moves" if tree else "emat_exp_pop_moves", *head[1:], *stats, 5, ptr("res", C.byref(res)))


XP_GOOD = [("rounds=0", dict(spec=_xp_spec(rounds=0))), ("rounds=4096", dict(spec=_xp_spec(rounds=4096))), ("pop at its limits", dict(pop=d.PopModel.exp(-3.0, 1e-300, -2.0, 0.0))),
           ("g_min = g = g_max", dict(spec=_xp_spec(g_min=0.1, g_max=0.1))), ("both moves off", dict(spec=_xp_spec(n0_move_enabled=False, g_move_enabled=False)))]
XP_REFUSALS = [("pop=const", dict(pop=d.PopModel.const(3.0))), ("pop=skygrid", dict(pop=d.PopModel.skygrid([-3.0, -2.0], [1.0, 2.0])))] + [
    ("pop %r" % (p,), dict(pop=d.PopModel.exp(*p))) for p in ((0.0, 0.0, 0.1), (0.0, -1.0, 0.1), (0.0, INF, 0.1), (0.0, NAN, 0.1), (0.0, 3.0, INF), (0.0, 3.0, NAN), (NAN, 3.0, 0.1), (-INF, 3.0, 0.1),
                                                               (0.0, 3.0, 0.1, -1e-300), (0.0, 3.0, 0.1, INF), (0.0, 3.0, 0.1, NAN))] + [
    ("spec " + ", ".join("%s=%r" % kv for kv in kw.items()), dict(spec=_xp_spec(**kw))) for kw in (
        dict(g_min=0.2), dict(g_max=0.05), dict(g_max=0.0), dict(g_min=0.3, g_max=0.2), dict(g_min=1.0, g_max=0.0), dict(g_min=NAN), dict(g_max=NAN), dict(g_prior_scale=0.0), dict(g_prior_scale=-1.0),
        dict(g_prior_scale=INF), dict(g_prior_scale=NAN), dict(g_prior_mu=INF), dict(g_prior_mu=NAN), dict(inv_n0_prior_alpha=NAN), dict(inv_n0_prior_alpha=INF), dict(inv_n0_prior_beta=-INF),
        dict(inv_n0_prior_beta=NAN), dict(rounds=-1), dict(rounds=-2), dict(rounds=-3), dict(rounds=4097), dict(rounds=5000))] + [
    ("t_step=0", dict(t_step=0.0)), ("t_step=inf", dict(t_step=INF)), ("t_ref=nan", dict(t_ref=NAN))] + SKY_REFUSALS[-7:] + FAR


def _exp_pop_rows(rec, h):
    _xp(rec, "xp good", h); _xp(rec, "xp good, trace", h, trace_capacity=100)
    for name, kw in XP_GOOD + XP_REFUSALS:
        _xp(rec, "xp " + name, h, **kw)
    _xp(rec, "xp 2^22+1 cells", h, first_cell=-BIG, k_bar=np.ones(BIG))
    for what in ("h", "m", "sp", "kb", "ts", "res"):
        _xp(rec, "xp null " + what, h, null=(what,))
    _xp(rec, "xp trace_capacity 99", h, trace_capacity=99)
    _xp(rec, "tree_xp good, trace", h, tree=True, t_step=1.0, trace_capacity=100)
    _xp(rec, "tree_xp nulls", h, tree=True, null=("m", "sp", "res")); _xp(rec, "tree_xp null h", h, tree=True, null=("h",))
    for t_ref, t_step in BAD_ORIGINS:
        _xp(rec, "tree_xp origin %r %r" % (t_ref, t_step), h, tree=True, t_ref=t_ref, t_step=t_step)
    for name, kw in (("pop=const", dict(pop=d.PopModel.const(3.0))), ("n0=0", dict(pop=d.PopModel.exp(0.0, 0.0, 0.1))), ("g_prior_scale=0", dict(spec=_xp_spec(g_prior_scale=0.0))),
                     ("g_max=0", dict(spec=_xp_spec(g_max=0.0))), ("rounds=-3", dict(spec=_xp_spec(rounds=-3))), ("rounds=5000", dict(spec=_xp_spec(rounds=5000)))):
        _xp(rec, "tree_xp " + name, h, tree=True, t_step=1.0, **kw)
    # two faults
    _xp(rec, "xp 2: model + spec", h, pop=d.PopModel.exp(0.0, 0.0, 0.1), spec=_xp_spec(g_prior_scale=0.0))
    _xp(rec, "xp 2: bounds + g outside", h, pop=d.PopModel.exp(0.0, 3.0, 5.0), spec=_xp_spec(g_min=NAN))
    _xp(rec, "xp 2: g outside + spec", h, spec=_xp_spec(g_max=0.05, g_prior_scale=0.0))
    _xp(rec, "xp 2: spec + spec", h, spec=_xp_spec(g_prior_mu=NAN, inv_n0_prior_beta=NAN))
    _xp(rec, "xp 2: spec + origin", h, spec=_xp_spec(rounds=-1), t_step=0.0)
    _xp(rec, "xp 2: trace + origin", h, trace_capacity=99, t_step=0.0)
    _xp(rec, "xp 2: origin + statistics", h, t_ref=NAN, k_bar=np.zeros(0))
    _xp(rec, "xp 2: statistics + cells", h, first_cell=-BIG, k_bar=-np.ones(BIG))
    _xp(rec, "xp 2: statistics + rounds", h, inner_t=np.array([-3.9, -2.0, 0.0]), spec=_xp_spec(rounds=4097))
    _xp(rec, "xp 2: cells + rounds", h, first_cell=-BIG, k_bar=np.ones(BIG), spec=_xp_spec(rounds=4097))
    _xp(rec, "xp 2: cell numbers + rounds", h, spec=_xp_spec(rounds=4097), **FAR[0][1])
    _xp(rec, "xp 2: null + model", h, null=("ts",), pop=d.PopModel.const(3.0))
    _xp(rec, "tree_xp 2: origin + rounds", h, tree=True, t_step=0.0, spec=_xp_spec(rounds=5000))
    _xp(rec, "tree_xp 2: trace + rounds", h, tree=True, t_step=1.0, trace_capacity=7, spec=_xp_spec(rounds=5000))


# ---- the site-rate group ------------------------------------------------------------------------------------------------------------------
def _sr(rec, name, h, T=None, M=None, alpha=1.0, steps=10, trace_capacity=None, null=()):
    T = np.full(L_SITES, 3.0) if T is None else T; M = (np.arange(L_SITES, dtype=np.int32) % 3) if M is None else M
    res = engine._SiteRateResultC()
    if trace_capacity is not None:
        buf = (engine._SiteRateStepC * max(1, trace_capacity))(); rec.keep.append(buf); res.trace = buf; res.trace_capacity = trace_capacity
    ptr = lambda what, p: None if what in null else p                                    # noqa: E731
    rec.backend(name, None if "h" in null else h, "emat_site_rate_moves", ptr("T", T.ctypes.data_as(DP)), ptr("M", M.ctypes.data_as(IP)), float(alpha), int(steps), 1, ptr("res", C.byref(res)))


def _site_rate_rows(rec, h, h_no_evo):
    def edited(base, **at):
        a = base.copy()
        for i, v in at.items():
            a[int(i[1:])] = v
        return a
    T0, M0 = np.full(L_SITES, 3.0), np.arange(L_SITES, dtype=np.int32) % 3
    _sr(rec, "sr good, trace", h, trace_capacity=10); _sr(rec, "sr good, no steps", h, steps=0); _sr(rec, "sr good, no trace", h, steps=5)
    nu = np.zeros(L_SITES)
    rec.backend("nu_l good", h, "emat_get_nu_l", _dbl(nu)); rec.backend("nu_l null", h, "emat_get_nu_l", None); rec.backend("nu_l before set_evo", h_no_evo, "emat_get_nu_l", _dbl(nu))
    _sr(rec, "sr before set_evo", h_no_evo)
    for alpha in (0.0, -1.0, NAN, INF):
        _sr(rec, "sr alpha=%r" % alpha, h, alpha=alpha)
    _sr(rec, "sr steps=-1", h, steps=-1); _sr(rec, "sr trace_capacity 4 of 5", h, steps=5, trace_capacity=4)
    for what in ("T", "M", "res", "h"):
        _sr(rec, "sr null " + what, h, steps=5, null=(what,))
    for bad in (-1e-300, NAN, INF, -INF):
        _sr(rec, "sr T[17]=T[31]=%r" % bad, h, T=edited(T0, i17=bad, i31=bad))
    M1 = edited(M0, i9=-1, i12=-5)
    _sr(rec, "sr M[9]<0", h, M=M1); _sr(rec, "sr M[9]<0, T[11]<0", h, M=M1, T=edited(T0, i11=-1.0)); _sr(rec, "sr M[9]<0, T[3]<0", h, M=M1, T=edited(T0, i11=-1.0, i3=-1.0))
    for shape, rate, n in ((0.5, 3.0, 8), (0.0, 1.0, 8), (-1.0, 1.0, 8), (NAN, 1.0, 8), (1.0, 0.0, 8), (1.0, INF, 8), (1.0, 1.0, -1)):
        rec.backend("sampler %r %r %d" % (shape, rate, n), h, "emat_debug_sample_gamma", 1, n, shape, rate, _dbl(np.zeros(8)))
    rec.backend("sampler null out", h, "emat_debug_sample_gamma", 1, 4, 0.5, 3.0, None)
    # two faults
    _sr(rec, "sr 2: null + alpha", h, alpha=0.0, null=("M",)); _sr(rec, "sr 2: alpha + steps", h, alpha=NAN, steps=-1); _sr(rec, "sr 2: steps + trace", h, steps=-1, trace_capacity=0)
    _sr(rec, "sr 2: trace + statistics", h, steps=5, trace_capacity=4, T=edited(T0, i0=-1.0)); _sr(rec, "sr 2: statistics + set_evo", h_no_evo, M=M1)


# ---- the run driver -----------------------------------------------------------------------------------------------------------------------
def _run_rows(rec):
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario("C1", num_tips=20, num_sites=300)
    run = d.EmatRun(None, sc.tree, sc.ref, 1)
    r = run._h
    try:
        g3 = np.zeros(3); tau = C.c_double(); n0 = C.c_double()
        sky_spec = lambda **kw: C.byref(d.SkygridSpec(**kw).c_struct())                  # noqa: E731
        xp_spec = lambda **kw: C.byref(d.ExpPopSpec(**kw).c_struct())                    # noqa: E731
        rec.run("run get_skygrid, no model", r, "emat_run_get_skygrid", _dbl(g3), C.byref(tau)); rec.run("run get_exp_pop, no model", r, "emat_run_get_exp_pop", C.byref(n0), C.byref(tau))
        rec.run("run skygrid_moves, no model", r, "emat_run_skygrid_moves", None); rec.run("run exp_pop_moves, no model", r, "emat_run_exp_pop_moves", None)
        run.set_pop_model(d.PopModel.skygrid([-3.0, -1.0, 0.0], [1.0, 2.0, 3.0], True))
        rec.run("run get_skygrid", r, "emat_run_get_skygrid", _dbl(g3), C.byref(tau)); rec.run("run get_exp_pop, a Skygrid", r, "emat_run_get_exp_pop", C.byref(n0), C.byref(tau))
        for kw in (dict(tau=0.0), dict(tau=INF), dict(hmc_steps=-2), dict(hmc_mean_dt=-1.0), dict(low_gamma_barrier_enabled=True, low_gamma_barrier_scale=-1.0), dict(tau=0.7)):
            rec.run("run set_skygrid " + ", ".join("%s=%r" % kv for kv in kw.items()), r, "emat_run_set_skygrid_moves", 1, sky_spec(**kw))
        rec.run("run set_skygrid 2: tau + hmc_steps", r, "emat_run_set_skygrid_moves", 1, sky_spec(tau=0.0, hmc_steps=-1))
        rec.run("run set_skygrid 2: barrier + hmc_mean_dt", r, "emat_run_set_skygrid_moves", 1, sky_spec(low_gamma_barrier_enabled=True, low_gamma_barrier_scale=0.0, hmc_mean_dt=0.0))
        rec.run("run set_skygrid null spec", r, "emat_run_set_skygrid_moves", 1, None); rec.run("run set_skygrid null run", None, "emat_run_set_skygrid_moves", 1, sky_spec())
        rec.run("run skygrid_moves", r, "emat_run_skygrid_moves", None); rec.run("run skygrid_moves null run", None, "emat_run_skygrid_moves", None)
        rec.run("run get_skygrid null run", None, "emat_run_get_skygrid", None, None)
        run.set_pop_model(d.PopModel.exp(0.0, 3.0, 0.1, 0.5))
        rec.run("run get_exp_pop", r, "emat_run_get_exp_pop", C.byref(n0), C.byref(tau)); rec.run("run get_skygrid, an exponential", r, "emat_run_get_skygrid", _dbl(g3), C.byref(tau))
        for kw in (dict(g_prior_scale=0.0), dict(g_prior_scale=INF), dict(g_min=1.0, g_max=0.0), dict(g_min=NAN), dict(g_prior_mu=NAN), dict(inv_n0_prior_alpha=INF), dict(inv_n0_prior_beta=NAN),
                   dict(rounds=-2), dict(rounds=2)):
            rec.run("run set_exp_pop " + ", ".join("%s=%r" % kv for kv in kw.items()), r, "emat_run_set_exp_pop_moves", 1, xp_spec(**kw))
        rec.run("run set_exp_pop 2: bounds + g_prior_mu", r, "emat_run_set_exp_pop_moves", 1, xp_spec(g_min=1.0, g_max=0.0, g_prior_mu=NAN))
        rec.run("run set_exp_pop 2: g_prior_scale + rounds", r, "emat_run_set_exp_pop_moves", 1, xp_spec(g_prior_scale=0.0, rounds=-2))
        rec.run("run set_exp_pop null spec", r, "emat_run_set_exp_pop_moves", 1, None); rec.run("run set_exp_pop null run", None, "emat_run_set_exp_pop_moves", 1, xp_spec())
        rec.run("run exp_pop_moves", r, "emat_run_exp_pop_moves", None); rec.run("run exp_pop_moves null run", None, "emat_run_exp_pop_moves", None)
        rec.run("run get_exp_pop null run", None, "emat_run_get_exp_pop", None, None)
        a = C.c_double(); nu = np.zeros(sc.num_sites)
        rec.run("run get_site_rates", r, "emat_run_get_site_rates", C.byref(a), _dbl(nu)); rec.run("run get_site_rates null run", None, "emat_run_get_site_rates", None, None)
        for alpha in (0.0, -2.0, NAN, INF, 0.7):
            rec.run("run set_site_rate alpha=%r" % alpha, r, "emat_run_set_site_rate_moves", 1, alpha)
        rec.run("run site_rate_moves", r, "emat_run_site_rate_moves", None); rec.run("run site_rate_moves null run", None, "emat_run_site_rate_moves", None)
        rec.run("run get_Ttwiddle_l", r, "emat_run_get_Ttwiddle_l", _dbl(nu)); rec.run("run get_Ttwiddle_l null", r, "emat_run_get_Ttwiddle_l", None)
    finally:
        run.close()


def record_refusals():
    """{row: [status, last-error text or ""]} of the library in use (EMAT_LIB_PATH, else the built one)."""
    rec = _Recorder()
    h = d.EmatBackend(30, device=-1)
    hs = d.EmatBackend(L_SITES, device=-1); hs.set_ref_sequence(np.zeros(L_SITES, np.uint8)); hs.set_hky(1e-3, 2.0, [0.25, 0.25, 0.25, 0.25])
    h0 = d.EmatBackend(L_SITES, device=-1)
    try:
        _skygrid_rows(rec, h.handle); _exp_pop_rows(rec, h.handle); _site_rate_rows(rec, hs.handle, h0.handle); _run_rows(rec)
    finally:
        h.close(); hs.close(); h0.close()
    return rec.table


@pytest.fixture(scope="module")
def tables():
    return json.load(open(GOLDEN))["host_only"], record_refusals()


def test_the_table_covers_the_three_groups_and_the_order_of_their_checks(tables):
    want, got = tables
    assert sorted(got) == sorted(want)
    assert sum(1 for st, _ in want.values() if st not in (0, 2)) >= 200, "the table no longer holds the refusals"
    assert sum(1 for name in want if " 2: " in name) >= 8, "the table no longer pins which of two faults is named"
    assert all(name in want for name in SETTER_ROWS) and all(source in want for _, source in SETTER_ROWS.values())


def test_every_status_is_as_recorded(tables):
    want, got = tables
    assert {n: got[n][0] for n in want} == {n: want[n][0] for n in want}


def test_every_text_is_as_recorded_but_the_five_setter_texts(tables):
    want, got = tables
    for name in want:
        if name not in SETTER_ROWS:
            assert got[name][1] == want[name][1], name


def test_the_five_setter_texts_are_the_backends_behind_the_setters_name(tables):
    want, got = tables
    for name, (setter, source) in SETTER_ROWS.items():
        fn, fault = want[source][1].split(": ", 1)                       # "emat_skygrid_moves: hmc_steps must not be negative", as recorded
        assert fn in ("emat_skygrid_moves", "emat_exp_pop_moves") and got[source][1] == want[source][1]
        assert got[name] == [want[name][0], setter + ": " + fault], name
