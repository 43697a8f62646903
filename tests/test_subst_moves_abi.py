"""The substitution-model moves' engine calls on a handle without a device: every bad argument is refused with a text naming the first
offender before the device is asked for, good arguments get EMAT_ERR_NO_DEVICE (there is no CPU path), and the Python mirror has the
header's signatures and struct layouts.  No GPU."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine
from test_skygrid_moves_abi import _declared, _struct_fields

NEW = ["emat_subst_moves", "emat_parts_subst_stats", "emat_parts_subst_moves", "emat_get_evo", "emat_run_set_subst_moves", "emat_run_subst_moves", "emat_run_get_hky"]
CTYPE = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double),
         "const int64_t*": C.POINTER(C.c_int64), "int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32),
         "emat_run*": C.c_void_p, "emat_backend*": C.c_void_p, "const emat_subst_spec*": C.POINTER(engine._SubstSpecC), "emat_subst_result*": C.POINTER(engine._SubstResultC)}
FIELD = {"double": C.c_double, "int32_t": C.c_int32, "emat_subst_step*": C.POINTER(engine._SubstStepC)}
INF = float("inf"); NAN = float("nan")


@pytest.mark.parametrize("name", NEW)
def test_exported_and_mirrored_with_the_headers_signature(name):
    assert hasattr(C.CDLL(d.library_path()), name), "missing export: " + name
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


def _field(name, ty):
    m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
    return (m.group(1), FIELD[ty] * int(m.group(2))) if m else (name, FIELD[ty])


@pytest.mark.parametrize("name,mirror,size", [("emat_subst_spec", engine._SubstSpecC, 80), ("emat_subst_step", engine._SubstStepC, 104), ("emat_subst_result", engine._SubstResultC, 136)])
def test_the_structs_mirror_the_header_field_for_field(name, mirror, size):
    want = [_field(n, t) for n, t in _struct_fields(name)]
    assert want == [(n, t) for n, t in mirror._fields_], name
    assert C.sizeof(mirror) == size


def test_the_step_records_dtype_is_the_struct():
    assert engine.SUBST_STEP_DTYPE.itemsize == C.sizeof(engine._SubstStepC) == 104
    for n, _ in engine._SubstStepC._fields_:
        assert engine.SUBST_STEP_DTYPE.fields[n][1] == getattr(engine._SubstStepC, n).offset


def test_the_specs_defaults_are_the_references():
    s = d.SubstSpec()
    assert (s.mu_prior_alpha, s.mu_prior_beta, s.do_mu, s.do_pi, s.do_kappa, s.rounds) == (1.0, 0.0, True, True, True, 10)


L = 30


def _handle(P=1, evo=True):
    b = d.EmatBackend(L, device=-1)
    b.set_ref_sequence(np.arange(L) % 4)
    if evo:
        pi = [0.1, 0.2, 0.3, 0.4]
        b.set_evo([1e-3] * P, [pi] * P, [d.hky_q_matrix(2.0, pi)] * P, np.ones(L), np.arange(L) % P)
    return b


@pytest.fixture()
def handle():
    b = _handle()
    yield b
    b.close()


def _good(P=1):
    return dict(spec=d.SubstSpec(mu=1e-3, kappa=2.0, pi=(0.1, 0.2, 0.3, 0.4)), T=np.full((P, 4), 50.0), M=np.full((P, 4, 4), 3, np.int64), C=np.array([7, 8, 9, 6], np.int64), key=5)


def _call(b, P=1, **kw):
    a = _good(P); a.update(kw)
    return b.subst_moves(a["spec"], a["T"], a["M"], a["C"], key=a["key"], trace=a.get("trace", False))


def _spec(**kw):
    return dataclasses.replace(_good()["spec"], **kw)


def _arr(a, idx, v):
    a = np.array(a); a[idx] = v
    return a


def test_good_arguments_reach_the_device_question_and_only_then(handle):
    for kw in (dict(), dict(trace=True), dict(spec=_spec(rounds=0)), dict(spec=_spec(rounds=4096)), dict(spec=_spec(kappa=5e-324)), dict(spec=_spec(do_mu=False, do_pi=False, do_kappa=False)),
               dict(T=np.zeros((1, 4)), spec=_spec(do_mu=False)), dict(M=np.zeros((1, 4, 4), np.int64), C=np.zeros(4, np.int64)), dict(spec=_spec(pi=(0.25 + 2e-10, 0.25, 0.25, 0.25)))):
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            _call(handle, **kw)
    two = _handle(2)
    try:
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            _call(two, P=2)
    finally:
        two.close()


@pytest.mark.parametrize("kw,text", [
    (dict(spec=_spec(mu=0.0)), "mu must be finite and positive"), (dict(spec=_spec(mu=-1.0)), "mu must"), (dict(spec=_spec(mu=INF)), "mu must"), (dict(spec=_spec(mu=NAN)), "mu must"),
    (dict(spec=_spec(kappa=0.0)), "kappa must be finite and positive"), (dict(spec=_spec(kappa=-2.0)), "kappa"), (dict(spec=_spec(kappa=INF)), "kappa"), (dict(spec=_spec(kappa=NAN)), "kappa"),
    (dict(spec=_spec(pi=(0.0, 0.3, 0.3, 0.4))), "pi[a] must lie inside (0, 1)"), (dict(spec=_spec(pi=(1.0, 0.3, 0.3, 0.4))), "inside (0, 1)"), (dict(spec=_spec(pi=(0.1, 0.2, NAN, 0.4))), "inside (0, 1)"),
    (dict(spec=_spec(pi=(-0.1, 0.4, 0.3, 0.4))), "inside (0, 1)"),
    (dict(spec=_spec(pi=(0.1, 0.2, 0.3, 0.4 + 1e-8))), "add up to 1"), (dict(spec=_spec(pi=(0.1, 0.2, 0.3, 0.3))), "add up to 1"),
    (dict(spec=_spec(mu_prior_alpha=NAN)), "mu_prior_alpha"), (dict(spec=_spec(mu_prior_beta=INF)), "mu_prior_beta"),
    (dict(spec=_spec(rounds=-1)), "rounds must not be negative"),
    (dict(T=_arr(np.full((1, 4), 50.0), (0, 2), -1e-300)), "Ttwiddle_beta_a[0][2] is negative or not finite"), (dict(T=_arr(np.full((1, 4), 50.0), (0, 1), INF)), "Ttwiddle_beta_a[0][1]"),
    (dict(T=_arr(np.full((1, 4), 50.0), (0, 3), NAN)), "Ttwiddle_beta_a[0][3]"),
    (dict(M=_arr(np.full((1, 4, 4), 3, np.int64), (0, 2, 1), -1)), "num_muts_beta_ab[0][2][1] is negative"),
    (dict(C=np.array([7, 8, -9, 6], np.int64)), "root_state_counts[2] is negative"),
    (dict(M=np.zeros((1, 4, 4), np.int64), spec=_spec(mu_prior_alpha=0.0)), "positive shape"),
    (dict(M=np.zeros((1, 4, 4), np.int64), spec=_spec(mu_prior_alpha=-0.5)), "positive shape"),
    (dict(T=np.zeros((1, 4))), "positive rate"), (dict(spec=_spec(mu_prior_beta=-1e9)), "positive rate"),
])
def test_every_refusal_names_its_offender(handle, kw, text):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_subst_moves.*" + re.escape(text)):
        _call(handle, **kw)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):      # the next call works as far as a handle without a device lets it
        _call(handle)
    mu, pi, q = handle.get_evo()                              # ... and the model is untouched
    assert mu.tolist() == [1e-3] and pi.tolist() == [[0.1, 0.2, 0.3, 0.4]] and np.array_equal(q[0], d.hky_q_matrix(2.0, [0.1, 0.2, 0.3, 0.4]))


def test_a_bad_mu_posterior_is_no_offence_while_the_mu_draw_is_off(handle):
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle, T=np.zeros((1, 4)), spec=_spec(do_mu=False))


def test_capacity_of_partitions_and_rounds(handle):
    with pytest.raises(d.EmatError, match="CAPACITY.*4097 rounds"):
        _call(handle, spec=_spec(rounds=4097))
    with pytest.raises(d.EmatError, match="CAPACITY.*4 site partitions"):
        _call(handle, P=5)
    five = _handle(5)
    try:
        for call in (lambda: five.parts_subst_moves(_spec()), lambda: five.parts_subst_stats(5)):
            with pytest.raises(d.EmatError, match="CAPACITY.*4 site partitions"):
                call()
    finally:
        five.close()


def test_the_number_of_partitions_must_be_the_models(handle):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*num_partitions does not match"):
        _call(handle, P=2)


def test_state_before_set_evo_and_without_parts(handle):
    bare = _handle(evo=False)
    try:
        for call in (lambda: _call(bare), lambda: bare.parts_subst_moves(_spec()), lambda: bare.parts_subst_stats(1), lambda: bare.get_evo()):
            with pytest.raises(d.EmatError, match="STATE.*emat_set_evo must precede"):
                call()
    finally:
        bare.close()
    for call in (lambda: handle.parts_subst_moves(_spec()), lambda: handle.parts_subst_stats(1)):
        with pytest.raises(d.EmatError, match="STATE.*no parts are out"):
            call()
    # the parts calls refuse a spec as emat_subst_moves does, before they look at the parts
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_parts_subst_moves.*kappa"):
        handle.parts_subst_moves(_spec(kappa=0.0))
    with pytest.raises(d.EmatError, match="CAPACITY.*rounds"):
        handle.parts_subst_moves(_spec(rounds=5000))


def test_parts_without_the_root_part_are_refused_and_with_it_reach_the_device_question(handle):
    from delphy_amd.scenarios import make_scenario
    from helpers import split_parts
    sc = make_scenario("C1", num_tips=20, num_sites=L)
    parts, incl, seeds, root_part, ref = split_parts(sc, 2, 3)
    handle.set_ref_sequence(ref)
    others = [k for k in range(len(parts)) if not incl[k]]
    handle.upload_parts([parts[k] for k in others], [False] * len(others), [seeds[k] for k in others])
    for call in (lambda: handle.parts_subst_moves(_spec()), lambda: handle.parts_subst_stats(1)):
        with pytest.raises(d.EmatError, match="STATE.*root part is not on this handle"):
            call()
    handle.upload_parts(parts, incl, seeds)
    for call in (lambda: handle.parts_subst_moves(_spec()), lambda: handle.parts_subst_stats(1)):
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            call()


def test_null_pointers_and_a_trace_without_room(handle):
    lib = d.load_library()
    g = _good()
    sp = g["spec"].c_struct(); dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int64)
    T = np.ascontiguousarray(g["T"]); M = np.ascontiguousarray(g["M"]); Cn = np.ascontiguousarray(g["C"])
    res = engine._SubstResultC()
    args = lambda **o: [o.get("h", handle.handle), o.get("sp", C.byref(sp)), 1, o.get("T", T.ctypes.data_as(dp)), o.get("M", M.ctypes.data_as(ip)), o.get("C", Cn.ctypes.data_as(ip)), 5, o.get("res", C.byref(res))]
    assert lib.emat_subst_moves(*args()) == 2                        # EMAT_ERR_NO_DEVICE: the arguments pass
    for o in (dict(h=None), dict(sp=None), dict(T=None), dict(M=None), dict(C=None), dict(res=None)):
        assert lib.emat_subst_moves(*args(**o)) == 1, o
    assert b"must not be null" in lib.emat_last_error(handle.handle)
    tr = np.zeros(19, engine.SUBST_STEP_DTYPE); res.trace = tr.ctypes.data_as(C.POINTER(engine._SubstStepC)); res.trace_capacity = 19   # 20 steps asked for
    assert lib.emat_subst_moves(*args()) == 1
    assert b"trace_capacity" in lib.emat_last_error(handle.handle)
    res.trace_capacity = 20
    assert lib.emat_subst_moves(*args()) == 2
    res.trace = None; res.trace_capacity = 0                         # no trace: its capacity does not matter
    assert lib.emat_subst_moves(*args()) == 2
    assert lib.emat_parts_subst_moves(handle.handle, None, 1, C.byref(res)) == 1 and lib.emat_parts_subst_moves(handle.handle, C.byref(sp), 1, None) == 1
    assert lib.emat_parts_subst_moves(None, C.byref(sp), 1, C.byref(res)) == 1
    assert lib.emat_parts_subst_stats(handle.handle, None, M.ctypes.data_as(ip), Cn.ctypes.data_as(ip)) == 1 and lib.emat_parts_subst_stats(None, None, None, None) == 1
    assert lib.emat_get_evo(handle.handle, None, None, None, None) == 1 and lib.emat_get_evo(None, None, None, None, None) == 1
    n = C.c_int32(0); mu = np.zeros(1)
    assert lib.emat_get_evo(handle.handle, C.byref(n), mu.ctypes.data_as(dp), None, None) == 7 and n.value == 1     # EMAT_ERR_BUFFER_TOO_SMALL, and the P to come back with


def test_get_evo_reads_back_what_set_evo_was_given():
    b = _handle(2)
    try:
        mu, pi, q = b.get_evo()
        assert mu.tolist() == [1e-3, 1e-3] and pi.shape == (2, 4) and q.shape == (2, 4, 4)
        assert np.array_equal(q[1], d.hky_q_matrix(2.0, [0.1, 0.2, 0.3, 0.4]))
    finally:
        b.close()


def test_the_run_driver_checks_its_arguments_and_defaults_to_off():
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario("C1", num_tips=20, num_sites=300)
    run = d.EmatRun(None, sc.tree, sc.ref, 1)
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            run.hky()                                       # no model yet
        run.set_hky(1e-3, 2.0, [0.1, 0.2, 0.3, 0.4])
        mu, kappa, pi = run.hky()
        assert (mu, kappa, pi.tolist()) == (1e-3, 2.0, [0.1, 0.2, 0.3, 0.4])
        for bad in (dict(mu_prior_alpha=NAN), dict(mu_prior_beta=INF), dict(rounds=-2), dict(rounds=4097)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_run_set_subst_moves"):
                run.set_subst_moves(True, d.SubstSpec(**bad))
        run.set_subst_moves(True, d.SubstSpec(mu=NAN, kappa=-1.0, pi=(9, 9, 9, 9), rounds=2))     # the spec's model is ignored
        assert run.hky()[:2] == (1e-3, 2.0)
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.subst_moves()                               # no backend attached: the driver never runs moves itself
        lib = d.load_library()
        assert lib.emat_run_set_subst_moves(run._h, 1, None) == 1 and lib.emat_run_subst_moves(None, None) == 1 and lib.emat_run_get_hky(None, None, None, None) == 1
    finally:
        run.close()
