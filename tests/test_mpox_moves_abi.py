"""The APOBEC (mpox) model's engine calls on a handle without a device: every bad argument is refused with a text naming the first offender before
the device is asked for, in the order the header states, good arguments get EMAT_ERR_NO_DEVICE (there is no CPU path), the model is untouched after
every refusal, and the Python mirror has the header's signatures and struct layouts.  No GPU."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine
from test_skygrid_moves_abi import _declared, _struct_fields

NEW = ["emat_mpox_moves", "emat_parts_mpox_moves", "emat_run_set_mpox", "emat_run_mpox_moves", "emat_run_get_mpox", "emat_run_get_mpox_partition"]
CTYPE = {"uint64_t": C.c_uint64, "int32_t": C.c_int32, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int64_t*": C.POINTER(C.c_int64),
         "int32_t*": C.POINTER(C.c_int32), "emat_run*": C.c_void_p, "emat_backend*": C.c_void_p, "const emat_mpox_spec*": C.POINTER(engine._MpoxSpecC),
         "emat_mpox_result*": C.POINTER(engine._MpoxResultC)}
FIELD = {"double": C.c_double, "int32_t": C.c_int32, "emat_mpox_round*": C.POINTER(engine._MpoxRoundC)}
INF = float("inf"); NAN = float("nan")
OK, INVALID, NO_DEVICE, STATE = 0, 1, 2, 4      # emat_status (include/emat_backend.h)


@pytest.mark.parametrize("name", NEW)
def test_exported_and_mirrored_with_the_headers_signature(name):
    assert hasattr(C.CDLL(d.library_path()), name), "missing export: " + name
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


@pytest.mark.parametrize("name,mirror,size", [("emat_mpox_spec", engine._MpoxSpecC, 40), ("emat_mpox_round", engine._MpoxRoundC, 160), ("emat_mpox_result", engine._MpoxResultC, 88)])
def test_the_structs_mirror_the_header_field_for_field(name, mirror, size):
    want = [(n, FIELD[t]) for n, t in _struct_fields(name)]
    assert want == [(n, t) for n, t in mirror._fields_], name
    assert C.sizeof(mirror) == size


def test_the_round_records_dtype_is_the_struct():
    assert engine.MPOX_ROUND_DTYPE.itemsize == C.sizeof(engine._MpoxRoundC) == 160
    for n, _ in engine._MpoxRoundC._fields_:
        assert engine.MPOX_ROUND_DTYPE.fields[n][1] == getattr(engine._MpoxRoundC, n).offset


def test_the_specs_defaults_are_the_references():
    s = d.MpoxSpec()
    assert (s.mu_star, s.mu_prior_alpha, s.mu_prior_beta, s.do_mu, s.rounds) == (0.0, 1.0, 0.0, True, 10)


L = 30
Q0, Q1 = engine.mpox_q_matrices(0.5)


def _handle(P=2, evo=True):
    b = d.EmatBackend(L, device=-1)
    b.set_ref_sequence(np.arange(L) % 4)
    if evo:
        b.set_evo([1e-3] * P, [[0.25] * 4] * P, ([Q0, Q1] * P)[:P], np.ones(L), np.arange(L) % P)
    return b


@pytest.fixture()
def handle():
    b = _handle()
    yield b
    b.close()


def _untouched(b, P=2):
    mu, pi, q = b.get_evo()
    return mu.tolist() == [1e-3] * P and pi.tolist() == [[0.25] * 4] * P and all(np.array_equal(q[p], (Q0, Q1)[p % 2]) for p in range(P))


def _good():
    return dict(spec=d.MpoxSpec(mu=1e-3, mu_star=5e-4), T=np.full((2, 4), 50.0), M=np.full((2, 4, 4), 3, np.int64), key=5)


def _call(b, **kw):
    a = _good(); a.update(kw)
    return b.mpox_moves(a["spec"], a["T"], a["M"], key=a["key"], trace=a.get("trace", False))


def _spec(**kw):
    return dataclasses.replace(_good()["spec"], **kw)


def _arr(a, idx, v):
    a = np.array(a); a[idx] = v
    return a


def test_good_arguments_reach_the_device_question_and_only_then(handle):
    for kw in (dict(), dict(trace=True), dict(spec=_spec(rounds=0)), dict(spec=_spec(rounds=4096)), dict(spec=_spec(mu_star=0.0)), dict(spec=_spec(do_mu=False)),
               dict(T=np.zeros((2, 4)), spec=_spec(do_mu=False)), dict(M=np.zeros((2, 4, 4), np.int64), spec=_spec(mu_prior_alpha=1.5)),
               dict(M=np.zeros((2, 4, 4), np.int64), spec=_spec(rounds=0))):          # (no round, no posterior to be bad)
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            _call(handle, **kw)
    assert _untouched(handle)


REFUSALS = [    # in the order in which they are answered
    (dict(spec=_spec(mu=0.0)), "mu must be finite and positive"), (dict(spec=_spec(mu=-1.0)), "mu must"), (dict(spec=_spec(mu=INF)), "mu must"), (dict(spec=_spec(mu=NAN)), "mu must"),
    (dict(spec=_spec(mu_star=-1e-300)), "mu_star must be finite and not negative"), (dict(spec=_spec(mu_star=INF)), "mu_star must"), (dict(spec=_spec(mu_star=NAN)), "mu_star must"),
    (dict(spec=_spec(mu_prior_alpha=NAN)), "mu_prior_alpha must be finite"), (dict(spec=_spec(mu_prior_beta=INF)), "mu_prior_beta must be finite"),
    (dict(spec=_spec(rounds=-1)), "rounds must not be negative"),
    (dict(T=_arr(np.full((2, 4), 50.0), (1, 2), -1e-300)), "Ttwiddle_beta_a[1][2] is negative or not finite"), (dict(T=_arr(np.full((2, 4), 50.0), (0, 1), INF)), "Ttwiddle_beta_a[0][1]"),
    (dict(T=_arr(np.full((2, 4), 50.0), (1, 3), NAN)), "Ttwiddle_beta_a[1][3]"),
    (dict(M=_arr(np.full((2, 4, 4), 3, np.int64), (1, 2, 0), -1)), "num_muts_beta_ab[1][2][0] is negative"),
    (dict(M=np.zeros((2, 4, 4), np.int64)), "positive shape"),                             # 0 + 1 - 1
    (dict(M=np.zeros((2, 4, 4), np.int64), spec=_spec(mu_prior_alpha=0.5)), "positive shape"),
    (dict(T=np.zeros((2, 4))), "positive rate"), (dict(spec=_spec(mu_prior_beta=-1e9)), "positive rate"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_every_refusal_names_its_offender(handle, kw, text):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_mpox_moves.*" + re.escape(text)):
        _call(handle, **kw)
    assert _untouched(handle)                                  # the model is untouched
    with pytest.raises(d.EmatError, match="NO_DEVICE"):        # ... and the next call works as far as a handle without a device lets it
        _call(handle)


def test_the_refusals_are_answered_in_the_stated_order():
    """Every call carries one offence of each later kind as well: the first in the header's order is the one named."""
    bad_T = _arr(np.full((2, 4), 50.0), (0, 0), -1.0); bad_M = _arr(np.full((2, 4, 4), 3, np.int64), (0, 0, 1), -1)
    three = _handle(3)
    bare = _handle(evo=False)
    lib = d.load_library()
    try:
        ladder = [(dict(mu=NAN), "mu must"), (dict(mu_star=-1.0), "mu_star must"), (dict(mu_prior_alpha=INF), "mu_prior_alpha"), (dict(mu_prior_beta=NAN), "mu_prior_beta"),
                  (dict(rounds=-3), "rounds must not be negative")]
        spec = dict(mu=NAN, mu_star=-1.0, mu_prior_alpha=INF, mu_prior_beta=NAN, rounds=-3)
        for fix, text in ladder:
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*" + text):
                three.mpox_moves(_spec(**spec), bad_T, bad_M, key=1)
            spec.pop(next(iter(fix)))
        # ... a trace too small (through the C interface: the mirror always makes room), then the rounds' capacity
        sp = _spec(rounds=4097).c_struct(); res = engine._MpoxResultC()
        tr = np.zeros(8, engine.MPOX_ROUND_DTYPE); res.trace = tr.ctypes.data_as(C.POINTER(engine._MpoxRoundC)); res.trace_capacity = 8
        args = (bad_T.ctypes.data_as(C.POINTER(C.c_double)), bad_M.ctypes.data_as(C.POINTER(C.c_int64)), 1, C.byref(res))
        assert lib.emat_mpox_moves(three.handle, C.byref(sp), *args) == INVALID and b"trace_capacity is smaller than rounds" in lib.emat_last_error(three.handle)
        with pytest.raises(d.EmatError, match="CAPACITY.*4097 rounds"):
            three.mpox_moves(_spec(rounds=4097), bad_T, bad_M, key=1)
        # ... the model's partitions, before the statistics are looked at
        for call in (lambda: three.mpox_moves(_spec(), bad_T, bad_M, key=1), lambda: three.parts_mpox_moves(_spec(), key=1)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*has 3 site partitions, the APOBEC model has 2"):
                call()
        assert _untouched(three, 3)
        # ... the statistics, Ttwiddle first, before the handle's state
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*Ttwiddle_beta_a\\[0\\]\\[0\\]"):
            bare.mpox_moves(_spec(), bad_T, bad_M, key=1)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*num_muts_beta_ab\\[0\\]\\[0\\]\\[1\\]"):
            bare.mpox_moves(_spec(), np.full((2, 4), 50.0), bad_M, key=1)
        # ... EMAT_ERR_STATE before emat_set_evo comes before the posterior is looked at, and before the device is asked for
        for call in (lambda: bare.mpox_moves(_spec(), np.zeros((2, 4)), np.zeros((2, 4, 4), np.int64), key=1), lambda: bare.parts_mpox_moves(_spec(), key=1)):
            with pytest.raises(d.EmatError, match="STATE.*emat_set_evo must precede emat_(parts_)?mpox_moves"):
                call()
    finally:
        three.close(); bare.close()


def test_one_partition_is_refused_as_three_are():
    one = _handle(1)
    try:
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*has 1 site partitions"):
            _call(one)
        assert _untouched(one, 1)
    finally:
        one.close()


def test_a_bad_mu_posterior_is_no_offence_while_the_mu_draw_is_off(handle):
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle, T=np.zeros((2, 4)), M=np.zeros((2, 4, 4), np.int64), spec=_spec(do_mu=False))


def test_state_without_parts_and_the_parts_calls_own_refusals(handle):
    with pytest.raises(d.EmatError, match="STATE.*no parts are out"):
        handle.parts_mpox_moves(_spec())
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_parts_mpox_moves.*mu_star"):      # a spec is refused as emat_mpox_moves refuses it, before the parts are looked at
        handle.parts_mpox_moves(_spec(mu_star=NAN))
    with pytest.raises(d.EmatError, match="CAPACITY.*rounds"):
        handle.parts_mpox_moves(_spec(rounds=5000))
    assert _untouched(handle)


def test_parts_without_the_root_part_are_refused_and_with_it_reach_the_device_question(handle):
    from delphy_amd.scenarios import make_scenario
    from helpers import split_parts
    sc = make_scenario("C1", num_tips=20, num_sites=L)
    parts, incl, seeds, root_part, ref = split_parts(sc, 2, 3)
    handle.set_ref_sequence(ref)
    others = [k for k in range(len(parts)) if not incl[k]]
    handle.upload_parts([parts[k] for k in others], [False] * len(others), [seeds[k] for k in others])
    with pytest.raises(d.EmatError, match="STATE.*root part is not on this handle"):
        handle.parts_mpox_moves(_spec())
    handle.upload_parts(parts, incl, seeds)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.parts_mpox_moves(_spec())
    assert _untouched(handle)


def test_null_pointers_and_a_trace_without_room(handle):
    lib = d.load_library()
    g = _good()
    sp = g["spec"].c_struct(); dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int64)
    T = np.ascontiguousarray(g["T"]); M = np.ascontiguousarray(g["M"])
    res = engine._MpoxResultC()
    args = lambda **o: [o.get("h", handle.handle), o.get("sp", C.byref(sp)), o.get("T", T.ctypes.data_as(dp)), o.get("M", M.ctypes.data_as(ip)), 5, o.get("res", C.byref(res))]
    assert lib.emat_mpox_moves(*args()) == NO_DEVICE                 # the arguments pass
    for o in (dict(h=None), dict(sp=None), dict(T=None), dict(M=None), dict(res=None)):
        assert lib.emat_mpox_moves(*args(**o)) == INVALID, o
    assert b"must not be null" in lib.emat_last_error(handle.handle)
    tr = np.zeros(9, engine.MPOX_ROUND_DTYPE); res.trace = tr.ctypes.data_as(C.POINTER(engine._MpoxRoundC)); res.trace_capacity = 9   # 10 rounds asked for
    assert lib.emat_mpox_moves(*args()) == INVALID
    assert b"trace_capacity" in lib.emat_last_error(handle.handle)
    res.trace_capacity = 10
    assert lib.emat_mpox_moves(*args()) == NO_DEVICE
    res.trace = None; res.trace_capacity = 0                         # no trace: its capacity does not matter
    assert lib.emat_mpox_moves(*args()) == NO_DEVICE
    assert lib.emat_parts_mpox_moves(handle.handle, None, 1, C.byref(res)) == INVALID and lib.emat_parts_mpox_moves(handle.handle, C.byref(sp), 1, None) == INVALID
    assert lib.emat_parts_mpox_moves(None, C.byref(sp), 1, C.byref(res)) == INVALID
    assert _untouched(handle)
