"""The Exponential population moves' engine calls on a handle without a device: every bad argument is refused with a text naming the first
offender before the device is asked for, good arguments get EMAT_ERR_NO_DEVICE (there is no CPU path), and the Python mirror has the
header's signatures.  No GPU."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine
from test_skygrid_moves_abi import _declared, _struct_fields

NEW = ["emat_exp_pop_moves", "emat_tree_exp_pop_moves", "emat_run_set_exp_pop_moves", "emat_run_exp_pop_moves", "emat_run_get_exp_pop"]
CTYPE = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double),
         "emat_run*": C.c_void_p, "emat_backend*": C.c_void_p, "const emat_pop_model*": C.POINTER(engine._PopModelC), "const emat_exp_pop_spec*": C.POINTER(engine._ExpPopSpecC),
         "emat_exp_pop_result*": C.POINTER(engine._ExpPopResultC)}
FIELD = {"double": C.c_double, "int32_t": C.c_int32, "emat_exp_pop_step*": C.POINTER(engine._ExpPopStepC)}
INF = float("inf"); NAN = float("nan")


@pytest.mark.parametrize("name", NEW)
def test_exported_and_mirrored_with_the_headers_signature(name):
    assert hasattr(C.CDLL(d.library_path()), name), "missing export: " + name
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


@pytest.mark.parametrize("name,mirror", [("emat_exp_pop_spec", engine._ExpPopSpecC), ("emat_exp_pop_step", engine._ExpPopStepC), ("emat_exp_pop_result", engine._ExpPopResultC)])
def test_the_structs_mirror_the_header_field_for_field(name, mirror):
    want = [(n, FIELD[t]) for n, t in _struct_fields(name)]
    assert want == [(n, t) for n, t in mirror._fields_], name


def test_the_step_records_dtype_is_the_struct():
    assert engine.EXP_POP_STEP_DTYPE.itemsize == C.sizeof(engine._ExpPopStepC) == 48
    for n, _ in engine._ExpPopStepC._fields_:
        assert engine.EXP_POP_STEP_DTYPE.fields[n][1] == getattr(engine._ExpPopStepC, n).offset


def test_the_specs_defaults_are_the_references():
    s = d.ExpPopSpec()
    assert (s.n0_move_enabled, s.g_move_enabled, s.inv_n0_prior_alpha, s.inv_n0_prior_beta, s.rounds) == (True, True, 0.0, 0.0, 50)
    assert (s.g_prior_mu, s.g_prior_scale, s.g_min, s.g_max) == (0.001 / 365.0, 30.701135 / 365.0, -INF, INF)


@pytest.fixture()
def handle():
    b = d.EmatBackend(30, device=-1)
    yield b
    b.close()


def _good():
    return dict(pop=d.PopModel.exp(0.0, 3.0, 0.1, 0.5), spec=d.ExpPopSpec(), t_ref=0.0, t_step=0.5, first_cell=-8, k_bar=np.linspace(1.0, 4.0, 8), inner_t=np.array([-3.9, -2.0, -0.01]), key=5)


def _call(b, **kw):
    a = _good(); a.update(kw)
    return b.exp_pop_moves(a["pop"], a["spec"], a["t_ref"], a["t_step"], a["first_cell"], a["k_bar"], a["inner_t"], key=a["key"], trace=a.get("trace", False))


def _spec(**kw):
    return dataclasses.replace(_good()["spec"], **kw)


def test_good_arguments_reach_the_device_question_and_only_then(handle):
    for kw in (dict(), dict(trace=True), dict(spec=_spec(rounds=0)), dict(spec=_spec(rounds=4096)), dict(pop=d.PopModel.exp(-3.0, 1e-300, -2.0, 0.0)),
               dict(spec=_spec(g_min=0.1, g_max=0.1)), dict(spec=_spec(n0_move_enabled=False, g_move_enabled=False))):
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            _call(handle, **kw)


@pytest.mark.parametrize("kw,text", [
    (dict(pop=d.PopModel.const(3.0)), "the population model is not an exponential one"),
    (dict(pop=d.PopModel.skygrid([-3.0, -2.0], [1.0, 2.0])), "the population model is not an exponential one"),
    (dict(pop=d.PopModel.exp(0.0, 0.0, 0.1)), "n0"), (dict(pop=d.PopModel.exp(0.0, -1.0, 0.1)), "n0"), (dict(pop=d.PopModel.exp(0.0, INF, 0.1)), "n0"), (dict(pop=d.PopModel.exp(0.0, NAN, 0.1)), "n0"),
    (dict(pop=d.PopModel.exp(0.0, 3.0, INF)), "g must be finite"), (dict(pop=d.PopModel.exp(0.0, 3.0, NAN)), "g must be finite"),
    (dict(pop=d.PopModel.exp(NAN, 3.0, 0.1)), "t0"), (dict(pop=d.PopModel.exp(-INF, 3.0, 0.1)), "t0"),
    (dict(pop=d.PopModel.exp(0.0, 3.0, 0.1, -1e-300)), "min_pop"), (dict(pop=d.PopModel.exp(0.0, 3.0, 0.1, INF)), "min_pop"), (dict(pop=d.PopModel.exp(0.0, 3.0, 0.1, NAN)), "min_pop"),
    (dict(spec=_spec(g_min=0.2)), "g lies outside [g_min, g_max]"), (dict(spec=_spec(g_max=0.05)), "g lies outside [g_min, g_max]"),
    (dict(spec=_spec(g_min=0.3, g_max=0.2)), "g_min must not exceed g_max"), (dict(spec=_spec(g_min=NAN)), "g_min"), (dict(spec=_spec(g_max=NAN)), "g_max"),
    (dict(spec=_spec(g_prior_scale=0.0)), "g_prior_scale"), (dict(spec=_spec(g_prior_scale=-1.0)), "g_prior_scale"), (dict(spec=_spec(g_prior_scale=INF)), "g_prior_scale"),
    (dict(spec=_spec(g_prior_scale=NAN)), "g_prior_scale"),
    (dict(spec=_spec(g_prior_mu=INF)), "g_prior_mu"), (dict(spec=_spec(g_prior_mu=NAN)), "g_prior_mu"),
    (dict(spec=_spec(inv_n0_prior_alpha=NAN)), "inv_n0_prior_alpha"), (dict(spec=_spec(inv_n0_prior_beta=-INF)), "inv_n0_prior_beta"),
    (dict(spec=_spec(rounds=-1)), "rounds"),
    (dict(t_step=0.0), "t_step"), (dict(t_step=INF), "t_step"), (dict(t_ref=NAN), "t_ref"),
    (dict(k_bar=np.zeros(0)), "num_cells"), (dict(inner_t=np.zeros(0)), "num_inner"),
    (dict(k_bar=np.array([1.0, 2.0, -1e-300, 3.0, -1.0, 1.0, 1.0, 1.0])), "k_bar of cell 2 "),
    (dict(k_bar=np.array([1.0, 2.0, 2.0, 3.0, INF, NAN, 1.0, 1.0])), "k_bar of cell 4 "),
    (dict(inner_t=np.array([-3.9, NAN, INF])), "inner_t of node 1 is not finite"),
    (dict(inner_t=np.array([-3.9, -2.0, 0.0])), "inner_t of node 2 lies outside the grid"),
    (dict(inner_t=np.array([-4.0000001, -2.0, -0.1])), "inner_t of node 0 lies outside the grid"),
])
def test_every_refusal_names_its_offender(handle, kw, text):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_exp_pop_moves.*" + re.escape(text)):
        _call(handle, **kw)


def test_capacity_of_cells_and_rounds(handle):
    with pytest.raises(d.EmatError, match="CAPACITY.*4097 rounds"):
        _call(handle, spec=_spec(rounds=4097))
    nc = (1 << 22) + 1
    with pytest.raises(d.EmatError, match="CAPACITY.*cells"):
        _call(handle, first_cell=-nc, k_bar=np.ones(nc))
    with pytest.raises(d.EmatError, match="CAPACITY.*cells' numbers"):
        _call(handle, first_cell=(1 << 30) - 4, inner_t=np.array([0.5 * ((1 << 30) - 2)]), t_ref=0.0)
    with pytest.raises(d.EmatError, match="CAPACITY.*cells' numbers"):
        _call(handle, first_cell=-(1 << 30) - 8, inner_t=np.array([0.5 * (-(1 << 30) - 4)]), t_ref=0.0)


def test_null_pointers_and_a_trace_without_room(handle):
    lib = d.load_library()
    g = _good()
    m = g["pop"].c_struct(); sp = g["spec"].c_struct(); dp = C.POINTER(C.c_double)
    kb = np.ascontiguousarray(g["k_bar"]); ts = np.ascontiguousarray(g["inner_t"])
    res = engine._ExpPopResultC()
    args = lambda **o: [o.get("h", handle.handle), o.get("m", C.byref(m)), o.get("sp", C.byref(sp)), 0.0, 0.5, -8, 8, o.get("kb", kb.ctypes.data_as(dp)), 3, o.get("ts", ts.ctypes.data_as(dp)), 5,
                        o.get("res", C.byref(res))]
    assert lib.emat_exp_pop_moves(*args()) == 2                      # EMAT_ERR_NO_DEVICE: the arguments pass
    for o in (dict(h=None), dict(m=None), dict(sp=None), dict(kb=None), dict(ts=None), dict(res=None)):
        assert lib.emat_exp_pop_moves(*args(**o)) == 1, o
    assert b"must not be null" in lib.emat_last_error(handle.handle)
    tr = np.zeros(99, engine.EXP_POP_STEP_DTYPE); res.trace = tr.ctypes.data_as(C.POINTER(engine._ExpPopStepC)); res.trace_capacity = 99   # 100 steps asked for
    assert lib.emat_exp_pop_moves(*args()) == 1
    assert b"trace_capacity" in lib.emat_last_error(handle.handle)
    res.trace_capacity = 100
    assert lib.emat_exp_pop_moves(*args()) == 2
    res.trace = None; res.trace_capacity = 0                         # no trace: its capacity does not matter
    assert lib.emat_exp_pop_moves(*args()) == 2
    assert lib.emat_tree_exp_pop_moves(handle.handle, None, None, 0.0, 1.0, 1, None) == 1 and lib.emat_tree_exp_pop_moves(None, C.byref(m), C.byref(sp), 0.0, 1.0, 1, C.byref(res)) == 1


def test_the_tree_call_checks_its_arguments_and_then_asks_for_the_device(handle):
    g = _good()
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.tree_exp_pop_moves(g["pop"], g["spec"], 0.0, 1.0, key=1, trace=True)
    for bad in ((NAN, 1.0), (0.0, 0.0), (0.0, INF)):
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_tree_exp_pop_moves.*t_step"):
            handle.tree_exp_pop_moves(g["pop"], g["spec"], *bad)
    for kw, text in ((dict(pop=d.PopModel.const(3.0)), "not an exponential one"), (dict(pop=d.PopModel.exp(0.0, 0.0, 0.1)), "n0"), (dict(spec=_spec(g_prior_scale=0.0)), "g_prior_scale"),
                     (dict(spec=_spec(g_max=0.0)), "outside"), (dict(spec=_spec(rounds=-3)), "rounds")):
        a = dict(g); a.update(kw)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*" + text):
            handle.tree_exp_pop_moves(a["pop"], a["spec"], 0.0, 1.0)
    with pytest.raises(d.EmatError, match="CAPACITY.*rounds"):
        handle.tree_exp_pop_moves(g["pop"], _spec(rounds=5000), 0.0, 1.0)


def test_the_skygrid_moves_still_refuse_an_exponential_model_with_their_old_text(handle):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_skygrid_moves: the population model is not a Skygrid"):
        handle.skygrid_moves(d.PopModel.exp(0.0, 3.0, 0.1), d.SkygridSpec(), 0.0, 0.5, -8, np.linspace(1.0, 4.0, 8), np.array([-3.9, -2.0, -0.01]), key=5)


def test_the_run_driver_checks_its_arguments_and_defaults_to_off():
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario("C1", num_tips=20, num_sites=300)
    run = d.EmatRun(None, sc.tree, sc.ref, 1)
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            run.exp_pop()                                   # no exponential model yet
        run.set_pop_model(d.PopModel.skygrid([-3.0, -1.0, 0.0], [1.0, 2.0, 3.0], True))
        with pytest.raises(d.EmatError, match="STATE"):
            run.exp_pop()
        run.set_pop_model(d.PopModel.exp(0.0, 3.0, 0.1, 0.5))
        assert run.exp_pop() == (3.0, 0.1)
        for bad in (dict(g_prior_scale=0.0), dict(g_prior_scale=INF), dict(g_min=1.0, g_max=0.0), dict(g_min=NAN), dict(g_prior_mu=NAN), dict(inv_n0_prior_alpha=INF),
                    dict(inv_n0_prior_beta=NAN), dict(rounds=-2)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
                run.set_exp_pop_moves(True, d.ExpPopSpec(**bad))
        run.set_exp_pop_moves(True, d.ExpPopSpec(rounds=2))
        assert run.exp_pop() == (3.0, 0.1)
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.exp_pop_moves()                             # no backend attached: the driver never runs moves itself
        lib = d.load_library()
        assert lib.emat_run_set_exp_pop_moves(run._h, 1, None) == 1 and lib.emat_run_exp_pop_moves(None, None) == 1 and lib.emat_run_get_exp_pop(None, None, None) == 1
    finally:
        run.close()
