"""The Skygrid population moves' engine calls on a handle without a device: every bad argument is refused with a text naming the first
offender before the device is asked for, good arguments get EMAT_ERR_NO_DEVICE (there is no CPU path), and the Python mirror has the
header's signatures.  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["emat_skygrid_moves", "emat_debug_pop_gradient", "emat_tree_coalescent_stats", "emat_tree_skygrid_moves", "emat_run_set_skygrid_moves", "emat_run_skygrid_moves",
       "emat_run_get_skygrid"]
CTYPE = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double),
         "int32_t*": C.POINTER(C.c_int32), "emat_run*": C.c_void_p, "emat_backend*": C.c_void_p, "const emat_pop_model*": C.POINTER(engine._PopModelC), "const emat_skygrid_spec*": C.POINTER(engine._SkygridSpecC),
         "emat_skygrid_result*": C.POINTER(engine._SkygridResultC)}
FIELD = {"double": C.c_double, "int32_t": C.c_int32, "double*": C.POINTER(C.c_double)}


def _header():
    return "".join(re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("emat_backend.h", "emat_host.h"))


def _declared(name):
    m = re.search(r"emat_status\s+" + name + r"\s*\((.*?)\);", _header(), flags=re.S)
    assert m, name + " is not declared"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", "*") for a in m.group(1).split(",")]


def _struct_fields(name):
    """[(field, C type)] of a typedef struct in the header, in order."""
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ty, names = decl.split(" ", 1)
        for nm in names.split(","):
            nm = nm.strip()
            out.append((nm.lstrip("*"), ty + ("*" if nm.startswith("*") or ty.endswith("*") else "")))
    return [(n, t.replace("**", "*")) for n, t in out]


@pytest.mark.parametrize("name", NEW)
def test_exported_and_mirrored_with_the_headers_signature(name):
    assert hasattr(C.CDLL(d.library_path()), name), "missing export: " + name
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


@pytest.mark.parametrize("name,mirror", [("emat_skygrid_spec", engine._SkygridSpecC), ("emat_skygrid_result", engine._SkygridResultC)])
def test_the_structs_mirror_the_header_field_for_field(name, mirror):
    want = [(n, FIELD[t]) for n, t in _struct_fields(name)]
    assert want == [(n, t) for n, t in mirror._fields_], name


@pytest.fixture()
def handle():
    b = d.EmatBackend(30, device=-1)
    yield b
    b.close()


def _good():
    pm = d.PopModel.skygrid([-3.0, -2.0, -1.0], [1.0, 2.0, 1.5], True)
    return dict(pop=pm, spec=d.SkygridSpec(low_gamma_barrier_enabled=True), t_ref=0.0, t_step=0.5, first_cell=-8, k_bar=np.linspace(1.0, 4.0, 8), inner_t=np.array([-3.9, -2.0, -0.01]), key=5)


def _call(b, **kw):
    a = _good(); a.update(kw)
    return b.skygrid_moves(a["pop"], a["spec"], a["t_ref"], a["t_step"], a["first_cell"], a["k_bar"], a["inner_t"], key=a["key"], trace=a.get("trace", False))


def test_good_arguments_reach_the_device_question_and_only_then(handle):
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle, trace=True)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.debug_pop_gradient(_good()["pop"], 3, 2, [0.0], [1.0])
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.debug_pop_gradient(_good()["pop"], 4, 0, [0.0], [0.0])


def _spec(**kw):
    return dataclasses.replace(_good()["spec"], **kw)


@pytest.mark.parametrize("kw,text", [
    (dict(pop=d.PopModel.const(3.0)), "not a Skygrid"),
    (dict(pop=d.PopModel.exp(0.0, 3.0, 0.1)), "not a Skygrid"),
    (dict(pop=d.PopModel.skygrid([0.0], [1.0])), "at least two knots"),
    (dict(pop=d.PopModel.skygrid([0.0, 0.0], [1.0, 1.0])), "strictly increasing"),
    (dict(pop=d.PopModel.skygrid([0.0, 1.0, 2.0], [1.0, float("nan"), 1.0])), "knot 1 "),
    (dict(spec=_spec(tau=0.0)), "tau"), (dict(spec=_spec(tau=-1.0)), "tau"), (dict(spec=_spec(tau=float("nan"))), "tau"), (dict(spec=_spec(tau=float("inf"))), "tau"),
    (dict(spec=_spec(low_gamma_barrier_scale=0.0)), "low_gamma_barrier_scale"), (dict(spec=_spec(low_gamma_barrier_scale=-0.3)), "low_gamma_barrier_scale"),
    (dict(spec=_spec(hmc_steps=-1)), "hmc_steps"), (dict(spec=_spec(hmc_mean_dt=0.0)), "hmc_mean_dt"), (dict(spec=_spec(hmc_mean_dt=-0.1)), "hmc_mean_dt"),
    (dict(t_step=0.0), "t_step"), (dict(t_ref=float("nan")), "t_ref"),
    (dict(k_bar=np.zeros(0)), "num_cells"), (dict(inner_t=np.zeros(0)), "num_inner"),
    (dict(k_bar=np.array([1.0, 2.0, -1e-300, 3.0, -1.0, 1.0, 1.0, 1.0])), "k_bar of cell 2 "),
    (dict(k_bar=np.array([1.0, 2.0, 2.0, 3.0, float("inf"), float("nan"), 1.0, 1.0])), "k_bar of cell 4 "),
    (dict(inner_t=np.array([-3.9, float("nan"), float("inf")])), "inner_t of node 1 is not finite"),
    (dict(inner_t=np.array([-3.9, -2.0, 0.0])), "inner_t of node 2 lies outside the grid"),
    (dict(inner_t=np.array([-4.0000001, -2.0, -0.1])), "inner_t of node 0 lies outside the grid"),
])
def test_every_refusal_names_its_offender(handle, kw, text):
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*" + re.escape(text)):
        _call(handle, **kw)


def test_a_zero_barrier_scale_is_fine_with_the_barrier_off(handle):
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle, spec=_spec(low_gamma_barrier_enabled=False, low_gamma_barrier_scale=0.0))


def test_capacity_of_knots_and_cells(handle):
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        _call(handle, pop=d.PopModel.skygrid(np.arange(1024.0), np.ones(1024)))
    with pytest.raises(d.EmatError, match="CAPACITY.*1025 knots"):
        _call(handle, pop=d.PopModel.skygrid(np.arange(1025.0), np.ones(1025)))
    nc = (1 << 22) + 1
    with pytest.raises(d.EmatError, match="CAPACITY.*cells"):
        _call(handle, first_cell=-nc, k_bar=np.ones(nc))


def test_null_pointers_and_a_trace_without_room(handle):
    lib = d.load_library()
    g = _good()
    m = g["pop"].c_struct(); sp = g["spec"].c_struct(); dp = C.POINTER(C.c_double)
    kb = np.ascontiguousarray(g["k_bar"]); ts = np.ascontiguousarray(g["inner_t"]); gam = np.zeros(3)
    res = engine._SkygridResultC(); res.gamma = gam.ctypes.data_as(dp)
    args = lambda **o: [o.get("h", handle.handle), o.get("m", C.byref(m)), o.get("sp", C.byref(sp)), 0.0, 0.5, -8, 8, o.get("kb", kb.ctypes.data_as(dp)), 3, o.get("ts", ts.ctypes.data_as(dp)), 5,
                        o.get("res", C.byref(res))]
    assert lib.emat_skygrid_moves(*args()) == 2                      # EMAT_ERR_NO_DEVICE: the arguments pass
    for o in (dict(h=None), dict(m=None), dict(sp=None), dict(kb=None), dict(ts=None), dict(res=None)):
        assert lib.emat_skygrid_moves(*args(**o)) == 1, o
    assert b"must not be null" in lib.emat_last_error(handle.handle)
    res.gamma = None
    assert lib.emat_skygrid_moves(*args()) == 1                      # no room for the new curve
    res.gamma = gam.ctypes.data_as(dp)
    tr = np.zeros((5 + 4 * 24, 3)); res.trace = tr.ctypes.data_as(dp); res.trace_capacity = 24    # 25 steps asked for
    assert lib.emat_skygrid_moves(*args()) == 1
    assert b"trace_capacity" in lib.emat_last_error(handle.handle)
    res.trace = None; res.trace_capacity = 0                         # no trace: its capacity does not matter
    assert lib.emat_skygrid_moves(*args()) == 2
    # the gradient's hook
    a = np.zeros(2)
    ok = [handle.handle, C.byref(m), 3, 0, 2, a.ctypes.data_as(dp), a.ctypes.data_as(dp), a.ctypes.data_as(dp)]
    assert lib.emat_debug_pop_gradient(*ok) == 2
    for i, v in ((0, None), (1, None), (5, None), (6, None), (7, None), (2, 2), (2, 5), (3, -1), (3, 3), (4, -1)):
        bad = list(ok); bad[i] = v
        assert lib.emat_debug_pop_gradient(*bad) == 1, (i, v)
    c = d.PopModel.const(1.0).c_struct()
    assert lib.emat_debug_pop_gradient(handle.handle, C.byref(c), 3, 0, 2, a.ctypes.data_as(dp), a.ctypes.data_as(dp), a.ctypes.data_as(dp)) == 1
    assert b"not a Skygrid" in lib.emat_last_error(handle.handle)


def test_emat_debug_pop_is_as_it_was(handle):
    assert _declared("emat_debug_pop") == ["emat_backend*", "const emat_pop_model*", "int32_t", "int32_t", "const double*", "const double*", "double*"]
    lib = d.load_library()
    m = _good()["pop"].c_struct(); a = np.zeros(1); dp = C.POINTER(C.c_double)
    for op in (3, 4, -1):                                            # the new ops are not smuggled into the old hook
        assert lib.emat_debug_pop(handle.handle, C.byref(m), op, 1, a.ctypes.data_as(dp), a.ctypes.data_as(dp), a.ctypes.data_as(dp)) == 1


def test_the_tree_calls_check_their_arguments_and_then_ask_for_the_device(handle):
    g = _good()
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.tree_coalescent_stats(0.0, 1.0)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.tree_skygrid_moves(g["pop"], g["spec"], 0.0, 1.0, key=1, trace=True)
    for bad in ((float("nan"), 1.0), (0.0, 0.0), (0.0, float("inf"))):
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*t_step"):
            handle.tree_coalescent_stats(*bad)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*t_step"):
            handle.tree_skygrid_moves(g["pop"], g["spec"], *bad)
    for kw, text in ((dict(pop=d.PopModel.const(3.0)), "not a Skygrid"), (dict(spec=_spec(tau=0.0)), "tau"), (dict(spec=_spec(hmc_steps=-1)), "hmc_steps"),
                     (dict(spec=_spec(hmc_mean_dt=0.0)), "hmc_mean_dt"), (dict(spec=_spec(low_gamma_barrier_scale=0.0)), "low_gamma_barrier_scale")):
        a = dict(g); a.update(kw)
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*" + text):
            handle.tree_skygrid_moves(a["pop"], a["spec"], 0.0, 1.0)
    with pytest.raises(d.EmatError, match="CAPACITY.*1025 knots"):
        handle.tree_skygrid_moves(d.PopModel.skygrid(np.arange(1025.0), np.ones(1025)), g["spec"], 0.0, 1.0)
    lib = d.load_library(); n = C.c_int32()
    assert lib.emat_tree_coalescent_stats(handle.handle, 0.0, 1.0, None, C.byref(n), None, 0, None, 0, C.byref(n)) == 1
    assert lib.emat_tree_coalescent_stats(None, 0.0, 1.0, C.byref(n), C.byref(n), None, 0, None, 0, C.byref(n)) == 1
    assert lib.emat_tree_skygrid_moves(handle.handle, None, None, 0.0, 1.0, 1, None) == 1


def test_cell_numbers_beyond_int32_are_refused(handle):
    with pytest.raises(d.EmatError, match="CAPACITY.*cells' numbers"):
        _call(handle, first_cell=(1 << 30) - 4, inner_t=np.array([0.5 * ((1 << 30) - 2)]), t_ref=0.0)
    with pytest.raises(d.EmatError, match="CAPACITY.*cells' numbers"):
        _call(handle, first_cell=-(1 << 30) - 8, inner_t=np.array([0.5 * (-(1 << 30) - 4)]), t_ref=0.0)


def test_the_run_driver_checks_its_arguments_and_defaults_to_off():
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario("C1", num_tips=20, num_sites=300)
    run = d.EmatRun(None, sc.tree, sc.ref, 1)
    try:
        with pytest.raises(d.EmatError, match="STATE"):
            run.skygrid()                                   # no Skygrid model yet
        run.set_pop_model(d.PopModel.skygrid([-3.0, -1.0, 0.0], [1.0, 2.0, 3.0], True))
        assert np.array_equal(run.skygrid()[0], [1.0, 2.0, 3.0])
        for bad in (dict(tau=0.0), dict(tau=float("inf")), dict(hmc_steps=-2), dict(hmc_mean_dt=-1.0), dict(low_gamma_barrier_enabled=True, low_gamma_barrier_scale=-1.0)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
                run.set_skygrid_moves(True, d.SkygridSpec(**bad))
        run.set_skygrid_moves(True, d.SkygridSpec(tau=0.7))
        assert run.skygrid()[1] == 0.7
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.skygrid_moves()                             # no backend attached: the driver never runs moves itself
        lib = d.load_library()
        assert lib.emat_run_set_skygrid_moves(run._h, 1, None) == 1 and lib.emat_run_skygrid_moves(None, None) == 1 and lib.emat_run_get_skygrid(None, None, None) == 1
    finally:
        run.close()
