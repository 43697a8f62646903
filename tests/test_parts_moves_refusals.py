"""What the two groups that read the parts' substitution statistics (the substitution-model moves, the APOBEC model's moves) refuse, and in which words: status and
last-error text of the backend's entry points on a handle without a device and of the run driver's calls on a run without a backend, against the table recorded from
the library BEFORE the two groups got one frame (tests/golden/make_global_moves_refusals.py parts_host_only).  The arguments are every case of test_subst_moves_abi.py and
test_mpox_moves_abi.py, a null for every pointer of every entry point, and calls with two faults that pin which one is named.  After every backend call that did not
return EMAT_OK the handle's model is byte for byte what it was.  No exception list: every row's status and text are the recorded ones.  No GPU."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine
from test_global_moves_refusals import GOLDEN, INF, NAN, _Recorder

DP, IP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
L = 30
PI = (0.1, 0.2, 0.3, 0.4)
Q0, Q1 = engine.mpox_q_matrices(0.5)


def _handle(P, apobec=False, evo=True):
    b = d.EmatBackend(L, device=-1)
    b.set_ref_sequence(np.arange(L) % 4)
    if evo and apobec:
        b.set_evo([1e-3] * P, [[0.25] * 4] * P, ([Q0, Q1] * P)[:P], np.ones(L), np.arange(L) % P)
    elif evo:
        b.set_evo([1e-3] * P, [PI] * P, [d.hky_q_matrix(2.0, PI)] * P, np.ones(L), np.arange(L) % P)
    return b


def _model_bytes(b):
    try:
        return b"".join(np.asarray(v).tobytes() for v in b.get_evo())
    except d.EmatError:
        return None                                      # no model yet


class _PartsRecorder(_Recorder):
    """... that also looks at the model of the handle (an EmatBackend, or None for a null handle) around every call."""
    def __init__(self):
        super().__init__()
        self.model_changed = []

    def call(self, name, b, fn, *args):
        before = None if b is None else _model_bytes(b)
        self.backend(name, None if b is None else b.handle, fn, *args)
        if b is not None and self.table[name][0] != 0 and _model_bytes(b) != before:
            self.model_changed.append(name)


def _arr(a, idx, v):
    a = np.array(a); a[idx] = v
    return a


def _ptr(null, what, p):
    return None if what in null else p


# ---- the substitution-model moves -----------------------------------------------------------------------------------------------------------
SB_SPEC = d.SubstSpec(mu=1e-3, kappa=2.0, pi=PI)


def _sb_spec(**kw):
    return dataclasses.replace(SB_SPEC, **kw)


def _sb(rec, name, b, P=1, parts=False, null=(), trace_capacity=None, spec=SB_SPEC, T=None, M=None, Cn=None):
    T = np.ascontiguousarray(np.full((P, 4), 50.0) if T is None else T, np.float64); M = np.ascontiguousarray(np.full((P, 4, 4), 3) if M is None else M, np.int64)
    Cn = np.ascontiguousarray([7, 8, 9, 6] if Cn is None else Cn, np.int64)
    sp = spec.c_struct(); res = engine._SubstResultC()
    if trace_capacity is not None:
        tr = np.zeros(max(1, trace_capacity), engine.SUBST_STEP_DTYPE); rec.keep.append(tr)
        res.trace = tr.ctypes.data_as(C.POINTER(engine._SubstStepC)); res.trace_capacity = trace_capacity
    stats = [] if parts else [P, _ptr(null, "T", T.ctypes.data_as(DP)), _ptr(null, "M", M.ctypes.data_as(IP)), _ptr(null, "C", Cn.ctypes.data_as(IP))]
    rec.call(name, None if "h" in null else b, "emat_parts_subst_moves" if parts else "emat_subst_moves", _ptr(null, "sp", C.byref(sp)), *stats, 5, _ptr(null, "res", C.byref(res)))


T1, M1 = np.full((1, 4), 50.0), np.full((1, 4, 4), 3, np.int64)
Z1 = np.zeros((1, 4, 4), np.int64)
SB_GOOD = [("", {}), (", trace", dict(trace_capacity=20)), (" rounds=0", dict(spec=_sb_spec(rounds=0))), (" rounds=4096", dict(spec=_sb_spec(rounds=4096))), (" kappa=5e-324", dict(spec=_sb_spec(kappa=5e-324))),
           (" every switch off", dict(spec=_sb_spec(do_mu=False, do_pi=False, do_kappa=False))), (" T=0, no mu draw", dict(T=np.zeros((1, 4)), spec=_sb_spec(do_mu=False))),
           (" M=0, C=0", dict(M=Z1, Cn=np.zeros(4))), (" pi off 1 by 2e-10", dict(spec=_sb_spec(pi=(0.25 + 2e-10, 0.25, 0.25, 0.25))))]
SB_REFUSALS = [("spec " + ", ".join("%s=%r" % kv for kv in kw.items()), dict(spec=_sb_spec(**kw))) for kw in (
    dict(mu=0.0), dict(mu=-1.0), dict(mu=INF), dict(mu=NAN), dict(kappa=0.0), dict(kappa=-2.0), dict(kappa=INF), dict(kappa=NAN), dict(pi=(0.0, 0.3, 0.3, 0.4)), dict(pi=(1.0, 0.3, 0.3, 0.4)),
    dict(pi=(0.1, 0.2, NAN, 0.4)), dict(pi=(-0.1, 0.4, 0.3, 0.4)), dict(pi=(0.1, 0.2, 0.3, 0.4 + 1e-8)), dict(pi=(0.1, 0.2, 0.3, 0.3)), dict(mu_prior_alpha=NAN), dict(mu_prior_beta=INF), dict(rounds=-1),
    dict(rounds=4097))] + [
    ("T[0][2]=-1e-300", dict(T=_arr(T1, (0, 2), -1e-300))), ("T[0][1]=inf", dict(T=_arr(T1, (0, 1), INF))), ("T[0][3]=nan", dict(T=_arr(T1, (0, 3), NAN))), ("M[0][2][1]=-1", dict(M=_arr(M1, (0, 2, 1), -1))),
    ("C[2]=-9", dict(Cn=[7, 8, -9, 6])), ("shape 0", dict(M=Z1, spec=_sb_spec(mu_prior_alpha=0.0))), ("shape -0.5", dict(M=Z1, spec=_sb_spec(mu_prior_alpha=-0.5))),
    ("rate 0", dict(T=np.zeros((1, 4)))), ("rate negative", dict(spec=_sb_spec(mu_prior_beta=-1e9))), ("5 partitions", dict(P=5)), ("2 partitions for a model of 1", dict(P=2)), ("trace_capacity 19 of 20", dict(trace_capacity=19))]


def _stats(rec, name, b, null=(), P=1):
    T = np.zeros((P, 4)); M = np.zeros((P, 4, 4), np.int64); Cn = np.zeros(4, np.int64); rec.keep += [T, M, Cn]
    rec.call(name, None if "h" in null else b, "emat_parts_subst_stats", _ptr(null, "T", T.ctypes.data_as(DP)), _ptr(null, "M", M.ctypes.data_as(IP)), _ptr(null, "C", Cn.ctypes.data_as(IP)))


def _get_evo(rec, name, b, room, null=(), only_P=False):
    n = C.c_int32(room); mu = np.zeros(8); pi = np.zeros((8, 4)); q = np.zeros((8, 4, 4)); rec.keep += [n, mu, pi, q]
    out = [None, None, None] if only_P else [mu.ctypes.data_as(DP), pi.ctypes.data_as(DP), q.ctypes.data_as(DP)]
    rec.call(name, None if "h" in null else b, "emat_get_evo", _ptr(null, "n", C.byref(n)), *out)


def _subst_rows(rec, one, two, five, bare):
    bad_T, bad_M = _arr(T1, (0, 0), -1.0), _arr(M1, (0, 0, 1), -1)
    for name, kw in SB_GOOD:
        _sb(rec, "sb good" + name, one, **kw)
    _sb(rec, "sb good, 2 partitions", two, P=2)
    for name, kw in SB_REFUSALS:
        _sb(rec, "sb " + name, one, **kw)
    for what in ("h", "sp", "T", "M", "C", "res"):
        _sb(rec, "sb null " + what, one, null=(what,))
    for what in ("h", "sp", "res"):
        _sb(rec, "parts_sb null " + what, one, parts=True, null=(what,))
    for what in ("h", "T", "M", "C"):
        _stats(rec, "parts_stats null " + what, one, null=(what,))
    _get_evo(rec, "get_evo good", two, 2); _get_evo(rec, "get_evo only P", two, 0, only_P=True); _get_evo(rec, "get_evo room for 1 of 2", two, 1); _get_evo(rec, "get_evo no model", bare, 4)
    _get_evo(rec, "get_evo null h", two, 2, null=("h",)); _get_evo(rec, "get_evo null num_partitions", two, 2, null=("n",)); _get_evo(rec, "get_evo 5 partitions", five, 5)
    # the parts calls by the handle's state (with parts on it: _parts_rows)
    for state, b in (("no model", bare), ("5 partitions", five), ("no parts", one)):
        _sb(rec, "parts_sb " + state, b, parts=True); _stats(rec, "parts_stats " + state, b)
    _sb(rec, "parts_sb kappa=0", one, parts=True, spec=_sb_spec(kappa=0.0)); _sb(rec, "parts_sb rounds=5000", one, parts=True, spec=_sb_spec(rounds=5000))
    _sb(rec, "parts_sb trace_capacity 19 of 20", one, parts=True, trace_capacity=19)
    # two faults, the one named first pinned
    _sb(rec, "sb 2: null + spec", one, null=("M",), spec=_sb_spec(mu=NAN))
    _sb(rec, "sb 2: spec + spec", one, spec=_sb_spec(kappa=0.0, mu_prior_beta=NAN))
    _sb(rec, "sb 2: spec + trace", one, spec=_sb_spec(mu_prior_alpha=NAN), trace_capacity=19)
    _sb(rec, "sb 2: trace + 4097 rounds", one, spec=_sb_spec(rounds=4097), trace_capacity=8)
    _sb(rec, "sb 2: 4097 rounds + no model", bare, spec=_sb_spec(rounds=4097))
    _sb(rec, "sb 2: 4097 rounds + 5 partitions", one, spec=_sb_spec(rounds=4097), P=5)
    _sb(rec, "sb 2: 5 partitions + no model", bare, P=5)
    _sb(rec, "sb 2: no model + T", bare, T=bad_T)
    _sb(rec, "sb 2: partition mismatch + T", one, P=2, T=_arr(np.full((2, 4), 50.0), (1, 3), NAN))
    _sb(rec, "sb 2: T + M", one, T=bad_T, M=bad_M)
    _sb(rec, "sb 2: T + T", one, T=_arr(bad_T, (0, 3), INF))
    _sb(rec, "sb 2: M + C", one, M=bad_M, Cn=[-1, 0, 0, 0])
    _sb(rec, "sb 2: C + posterior", one, M=Z1, Cn=[0, 0, 0, -2], spec=_sb_spec(mu_prior_alpha=0.0))
    _sb(rec, "sb 2: M + posterior", one, M=_arr(Z1, (0, 3, 3), -1), spec=_sb_spec(mu_prior_alpha=0.0))
    _sb(rec, "sb 2: shape + rate", one, M=Z1, T=np.zeros((1, 4)), spec=_sb_spec(mu_prior_alpha=0.0))
    _sb(rec, "parts_sb 2: spec + no model", bare, parts=True, spec=_sb_spec(rounds=-1))
    _sb(rec, "parts_sb 2: trace + 5000 rounds", one, parts=True, spec=_sb_spec(rounds=5000), trace_capacity=3)
    _sb(rec, "parts_sb 2: 5000 rounds + no parts", one, parts=True, spec=_sb_spec(rounds=5000))
    _sb(rec, "parts_sb 2: 5000 rounds + 5 partitions", five, parts=True, spec=_sb_spec(rounds=5000))


# ---- the APOBEC model's moves ---------------------------------------------------------------------------------------------------------------
MX_SPEC = d.MpoxSpec(mu=1e-3, mu_star=5e-4)


def _mx_spec(**kw):
    return dataclasses.replace(MX_SPEC, **kw)


def _mx(rec, name, b, parts=False, null=(), trace_capacity=None, spec=MX_SPEC, T=None, M=None):
    T = np.ascontiguousarray(np.full((2, 4), 50.0) if T is None else T, np.float64); M = np.ascontiguousarray(np.full((2, 4, 4), 3) if M is None else M, np.int64)
    sp = spec.c_struct(); res = engine._MpoxResultC()
    if trace_capacity is not None:
        tr = np.zeros(max(1, trace_capacity), engine.MPOX_ROUND_DTYPE); rec.keep.append(tr)
        res.trace = tr.ctypes.data_as(C.POINTER(engine._MpoxRoundC)); res.trace_capacity = trace_capacity
    stats = [] if parts else [_ptr(null, "T", T.ctypes.data_as(DP)), _ptr(null, "M", M.ctypes.data_as(IP))]
    rec.call(name, None if "h" in null else b, "emat_parts_mpox_moves" if parts else "emat_mpox_moves", _ptr(null, "sp", C.byref(sp)), *stats, 5, _ptr(null, "res", C.byref(res)))


T2, M2 = np.full((2, 4), 50.0), np.full((2, 4, 4), 3, np.int64)
Z2 = np.zeros((2, 4, 4), np.int64)
MX_GOOD = [("", {}), (", trace", dict(trace_capacity=10)), (" rounds=0", dict(spec=_mx_spec(rounds=0))), (" rounds=4096", dict(spec=_mx_spec(rounds=4096))), (" mu_star=0", dict(spec=_mx_spec(mu_star=0.0))),
           (" no mu draw", dict(spec=_mx_spec(do_mu=False))), (" T=0, no mu draw", dict(T=np.zeros((2, 4)), spec=_mx_spec(do_mu=False))), (" M=0, alpha 1.5", dict(M=Z2, spec=_mx_spec(mu_prior_alpha=1.5))),
           (" M=0, no round", dict(M=Z2, spec=_mx_spec(rounds=0))), (" T=0, M=0, no mu draw", dict(T=np.zeros((2, 4)), M=Z2, spec=_mx_spec(do_mu=False)))]
MX_REFUSALS = [("spec " + ", ".join("%s=%r" % kv for kv in kw.items()), dict(spec=_mx_spec(**kw))) for kw in (
    dict(mu=0.0), dict(mu=-1.0), dict(mu=INF), dict(mu=NAN), dict(mu_star=-1e-300), dict(mu_star=INF), dict(mu_star=NAN), dict(mu_prior_alpha=NAN), dict(mu_prior_beta=INF), dict(rounds=-1), dict(rounds=4097))] + [
    ("T[1][2]=-1e-300", dict(T=_arr(T2, (1, 2), -1e-300))), ("T[0][1]=inf", dict(T=_arr(T2, (0, 1), INF))), ("T[1][3]=nan", dict(T=_arr(T2, (1, 3), NAN))), ("M[1][2][0]=-1", dict(M=_arr(M2, (1, 2, 0), -1))),
    ("shape 0", dict(M=Z2)), ("shape -0.5", dict(M=Z2, spec=_mx_spec(mu_prior_alpha=0.5))), ("rate 0", dict(T=np.zeros((2, 4)))), ("rate negative", dict(spec=_mx_spec(mu_prior_beta=-1e9))),
    ("trace_capacity 9 of 10", dict(trace_capacity=9))]


def _mpox_rows(rec, one, two, three, bare):
    bad_T, bad_M = _arr(T2, (0, 0), -1.0), _arr(M2, (0, 0, 1), -1)
    for name, kw in MX_GOOD:
        _mx(rec, "mx good" + name, two, **kw)
    for name, kw in MX_REFUSALS:
        _mx(rec, "mx " + name, two, **kw)
    for what in ("h", "sp", "T", "M", "res"):
        _mx(rec, "mx null " + what, two, null=(what,))
    for what in ("h", "sp", "res"):
        _mx(rec, "parts_mx null " + what, two, parts=True, null=(what,))
    for state, b in (("no model", bare), ("1 partition", one), ("3 partitions", three), ("no parts", two)):
        _mx(rec, "parts_mx " + state, b, parts=True)
    _mx(rec, "mx 1 partition", one); _mx(rec, "mx 3 partitions", three); _mx(rec, "mx no model", bare)
    _mx(rec, "parts_mx mu_star=nan", two, parts=True, spec=_mx_spec(mu_star=NAN)); _mx(rec, "parts_mx rounds=5000", two, parts=True, spec=_mx_spec(rounds=5000))
    _mx(rec, "parts_mx trace_capacity 9 of 10", two, parts=True, trace_capacity=9)
    # the ladder of test_mpox_moves_abi.py: every call carries one offence of each later kind as well
    spec = dict(mu=NAN, mu_star=-1.0, mu_prior_alpha=INF, mu_prior_beta=NAN, rounds=-3)
    for k in list(spec):
        _mx(rec, "mx ladder from " + k, three, spec=_mx_spec(**spec), T=bad_T, M=bad_M, trace_capacity=0)
        spec.pop(k)
    # two faults
    _mx(rec, "mx 2: null + spec", two, null=("T",), spec=_mx_spec(mu=NAN))
    _mx(rec, "mx 2: spec + trace", two, spec=_mx_spec(mu_prior_beta=NAN), trace_capacity=9)
    _mx(rec, "mx 2: trace + 4097 rounds", three, spec=_mx_spec(rounds=4097), trace_capacity=8, T=bad_T, M=bad_M)
    _mx(rec, "mx 2: 4097 rounds + no model", bare, spec=_mx_spec(rounds=4097))
    _mx(rec, "mx 2: 4097 rounds + 3 partitions", three, spec=_mx_spec(rounds=4097), T=bad_T, M=bad_M)
    _mx(rec, "mx 2: no model + T", bare, T=bad_T)
    _mx(rec, "mx 2: partition mismatch + T", three, T=bad_T, M=bad_M)
    _mx(rec, "mx 2: T + M", two, T=bad_T, M=bad_M)
    _mx(rec, "mx 2: M + no model", bare, M=bad_M)
    _mx(rec, "mx 2: no model + posterior", bare, T=np.zeros((2, 4)), M=Z2)
    _mx(rec, "mx 2: M + posterior", two, M=_arr(Z2, (1, 3, 3), -1))
    _mx(rec, "mx 2: T + posterior", two, T=_arr(np.zeros((2, 4)), (1, 1), NAN), M=Z2)
    _mx(rec, "mx 2: shape + rate", two, T=np.zeros((2, 4)), M=Z2)
    _mx(rec, "parts_mx 2: spec + no model", bare, parts=True, spec=_mx_spec(rounds=-1))
    _mx(rec, "parts_mx 2: trace + 5000 rounds", two, parts=True, spec=_mx_spec(rounds=5000), trace_capacity=3)
    _mx(rec, "parts_mx 2: 5000 rounds + 3 partitions", three, parts=True, spec=_mx_spec(rounds=5000))
    _mx(rec, "parts_mx 2: 3 partitions + no parts", three, parts=True)
    _mx(rec, "parts_mx 2: no model + no parts", bare, parts=True)


# ---- parts on a handle without a device -----------------------------------------------------------------------------------------------------
def _parts_rows(rec):
    from delphy_amd.scenarios import make_scenario
    from helpers import split_parts
    sc = make_scenario("C1", num_tips=20, num_sites=L)
    parts, incl, seeds, root_part, ref = split_parts(sc, 2, 3)
    others = [k for k in range(len(parts)) if not incl[k]]
    for P, apobec in ((1, False), (2, True)):
        b = _handle(P, apobec)
        try:
            b.set_ref_sequence(ref)
            for state in ("without the root part", "with the root part"):
                if state == "without the root part":
                    b.upload_parts([parts[k] for k in others], [False] * len(others), [seeds[k] for k in others])
                else:
                    b.upload_parts(parts, incl, seeds)
                tag = " %s, %d partition%s" % (state, P, "s" * (P > 1))
                _sb(rec, "parts_sb" + tag, b, parts=True); _stats(rec, "parts_stats" + tag, b, P=P); _mx(rec, "parts_mx" + tag, b, parts=True)
        finally:
            b.close()


# ---- the run driver -------------------------------------------------------------------------------------------------------------------------
def _run_rows(rec):
    tree, ref, _ = d.make_synthetic_emat(d.SynthParams(num_tips=20, num_sites=300, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=0.15 / 365.0, gaps_per_tip=2, mean_gap_len=12.0, seed=1))
    run = d.EmatRun(None, tree, ref, 1)
    r = run._h
    sb = lambda **kw: C.byref(d.SubstSpec(**kw).c_struct())                               # noqa: E731
    mx = lambda **kw: C.byref(d.MpoxSpec(**kw).c_struct())                                # noqa: E731
    mu, ms, n = C.c_double(), C.c_double(), C.c_int32(); pfs = np.zeros(300, np.int32)
    SB_FAULTS = (dict(mu_prior_alpha=NAN), dict(mu_prior_alpha=INF), dict(mu_prior_beta=INF), dict(mu_prior_beta=NAN), dict(rounds=-1), dict(rounds=-2), dict(rounds=4097), dict(rounds=4097, mu_prior_alpha=NAN),
                 dict(mu_prior_alpha=NAN, mu_prior_beta=NAN), dict(mu_prior_beta=INF, rounds=-1), dict(mu=NAN, kappa=-1.0, pi=(9, 9, 9, 9), rounds=2), dict(rounds=4096))
    MX_FAULTS = (dict(mu_star=-1.0), dict(mu_star=NAN), dict(mu_star=INF), dict(mu_prior_alpha=NAN), dict(mu_prior_beta=INF), dict(rounds=-1), dict(rounds=4097), dict(rounds=4097, mu_prior_alpha=NAN),
                 dict(mu_star=-1.0, rounds=4097), dict(mu_prior_alpha=INF, mu_prior_beta=NAN), dict(mu=NAN, rounds=2), dict(rounds=4096))

    def getters(state):
        rec.run("run get_mpox, " + state, r, "emat_run_get_mpox", C.byref(mu), C.byref(ms)); rec.run("run get_mpox_partition, " + state, r, "emat_run_get_mpox_partition", pfs.ctypes.data_as(I32P), C.byref(n))
        rec.run("run get_mpox nulls, " + state, r, "emat_run_get_mpox", None, None); rec.run("run get_mpox_partition nulls, " + state, r, "emat_run_get_mpox_partition", None, None)
        rec.run("run subst_moves, " + state, r, "emat_run_subst_moves", None); rec.run("run mpox_moves, " + state, r, "emat_run_mpox_moves", None)

    def setters(state):
        for kw in SB_FAULTS:
            rec.run("run set_subst %s, %s" % (", ".join("%s=%r" % kv for kv in kw.items()), state), r, "emat_run_set_subst_moves", 1, sb(**kw))
        rec.run("run set_subst null spec, " + state, r, "emat_run_set_subst_moves", 1, None); rec.run("run set_subst off, null spec, " + state, r, "emat_run_set_subst_moves", 0, None)
        rec.run("run set_subst off, rounds=4097, " + state, r, "emat_run_set_subst_moves", 0, sb(rounds=4097)); rec.run("run set_subst off, " + state, r, "emat_run_set_subst_moves", 0, sb())
        for kw in MX_FAULTS:
            rec.run("run set_mpox %s, %s" % (", ".join("%s=%r" % kv for kv in kw.items()), state), r, "emat_run_set_mpox", 1, mx(**kw))
        rec.run("run set_mpox null spec, " + state, r, "emat_run_set_mpox", 1, None)
    try:
        for fn, args in (("emat_run_set_subst_moves", (1, sb())), ("emat_run_subst_moves", (None,)), ("emat_run_set_mpox", (1, mx())), ("emat_run_mpox_moves", (None,)), ("emat_run_get_mpox", (None, None)),
                         ("emat_run_get_mpox_partition", (None, None)), ("emat_run_get_hky", (None, None, None))):
            rec.run("run %s null run" % fn, None, fn, *args)
        getters("before set_hky"); setters("before set_hky")
        rec.run("run set_mpox off when off, null spec", r, "emat_run_set_mpox", 0, None); rec.run("run set_mpox off when off", r, "emat_run_set_mpox", 0, mx(rounds=-1))
        run.set_hky(1e-3, 2.0, list(PI))
        rec.run("run set_subst on", r, "emat_run_set_subst_moves", 1, sb(rounds=3))
        getters("subst on"); setters("subst on")                                            # (the last set_subst of setters turns the group off again)
        rec.run("run set_subst on again", r, "emat_run_set_subst_moves", 1, sb(rounds=3))
        rec.run("run set_mpox, subst on", r, "emat_run_set_mpox", 1, mx()); rec.run("run set_mpox off, subst on", r, "emat_run_set_mpox", 0, None)
        rec.run("run set_subst off again", r, "emat_run_set_subst_moves", 0, sb())
        rec.run("run set_mpox on", r, "emat_run_set_mpox", 1, mx(mu_star=5e-4, rounds=3))
        getters("mpox on"); setters("mpox on")
        rec.run("run set_mpox on when on", r, "emat_run_set_mpox", 1, mx(mu_star=0.25, rounds=5)); rec.run("run get_mpox, after on when on", r, "emat_run_get_mpox", C.byref(mu), C.byref(ms))
        rec.table["run mu and mu* after on when on"] = [0, "%r %r" % (mu.value, ms.value)]
        rec.run("run set_mpox off", r, "emat_run_set_mpox", 0, None); rec.run("run set_mpox off twice", r, "emat_run_set_mpox", 0, None)
        getters("mpox off again")
    finally:
        run.close()


def record_refusals():
    """{row: [status, last-error text or ""]} of the library in use (EMAT_LIB_PATH, else the built one), and the rows after which a refused call had changed the handle's model."""
    rec = _PartsRecorder()
    one, two, three, five, bare = _handle(1), _handle(2, apobec=True), _handle(3, apobec=True), _handle(5), _handle(1, evo=False)
    one_apobec = _handle(1, apobec=True)
    try:
        _subst_rows(rec, one, two, five, bare); _mpox_rows(rec, one_apobec, two, three, bare); _parts_rows(rec); _run_rows(rec)
    finally:
        for b in (one, two, three, five, bare, one_apobec):
            b.close()
    return rec.table, rec.model_changed


@pytest.fixture(scope="module")
def tables():
    got, model_changed = record_refusals()
    return json.load(open(GOLDEN))["parts_host_only"], got, model_changed


def test_the_table_covers_both_groups_and_the_order_of_their_checks(tables):
    want, got, _ = tables
    assert sorted(got) == sorted(want)
    assert sum(1 for st, _ in want.values() if st not in (0, 2)) >= 200, "the table no longer holds the refusals"
    for group in ("sb 2: ", "mx 2: ", "parts_sb 2: ", "parts_mx 2: "):
        assert sum(1 for name in want if name.startswith(group)) >= 3, "the table no longer pins which of two faults is named: " + group
    assert sum(1 for st, _ in want.values() if st == 2) >= 25, "good arguments no longer reach the device question"


def test_every_status_and_text_is_as_recorded(tables):
    want, got, _ = tables
    for name in want:
        assert got[name] == want[name], name


def test_a_refused_call_leaves_the_model_untouched(tables):
    assert tables[2] == []
