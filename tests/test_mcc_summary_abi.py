"""The C-ABI of emat_mcc_node_times and emat_mcc_mutation_support: exported, mirrored in delphy_amd/engine.py with the header's signatures
and the header's result record, and refused on a handle without a device.  No GPU."""
import ctypes as C
import os
import re

import pytest

import delphy_amd as d
from delphy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["emat_mcc_node_times", "emat_mcc_mutation_support"]
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32),
         "int64_t*": C.POINTER(C.c_int64), "uint8_t*": C.POINTER(C.c_uint8), "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double),
         "emat_backend*": C.c_void_p, "emat_mcc_node_times_result*": C.POINTER(engine._MccNodeTimesResultC)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emat_backend.h")).read(), flags=re.S)


def _types(decls, sep):
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", "*") for a in decls.split(sep) if a.strip()]


def _declared(name):
    """The parameter types of `name` as include/emat_backend.h declares them."""
    m = re.search(r"emat_status\s+" + name + r"\s*\((.*?)\);", _header(), flags=re.S)
    assert m, name + " is not declared"
    return _types(m.group(1), ",")


def test_both_symbols_are_exported():
    lib = C.CDLL(d.library_path())
    for name in NEW:
        assert hasattr(lib, name), "missing export: " + name


@pytest.mark.parametrize("name", NEW)
def test_the_python_mirror_has_the_headers_signature(name):
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


def test_the_python_mirror_has_the_headers_result_record():
    m = re.search(r"typedef struct emat_mcc_node_times_result \{(.*?)\} emat_mcc_node_times_result;", _header(), flags=re.S)
    assert m, "emat_mcc_node_times_result is not declared"
    fields = [f for f in m.group(1).split(";") if f.strip()]
    names = [re.search(r"(\w+)\s*$", f).group(1) for f in fields]
    assert names == [f[0] for f in engine._MccNodeTimesResultC._fields_]
    assert [CTYPE[t] for t in _types(m.group(1), ";")] == [f[1] for f in engine._MccNodeTimesResultC._fields_]
    assert d.MccNodeTimes is engine.MccNodeTimes and d.MccMutationSupport is engine.MccMutationSupport


def test_both_calls_refuse_a_handle_without_a_device():
    b = d.EmatBackend(30, device=-1)
    try:
        for call in (lambda: b.mcc_node_times(), lambda: b.mcc_node_times([0], (0.5,), 0.95, True), lambda: b.mcc_mutation_support()):
            with pytest.raises(d.EmatError, match="EMAT_ERR_NO_DEVICE"):
                call()
        nm = C.c_int64(0)
        res = engine._MccNodeTimesResultC()
        assert b._lib.emat_mcc_node_times(b._h, 0, None, C.byref(res)) == b._lib.emat_mcc_mutation_support(b._h, 0, C.byref(nm), None, None, None, None) != 0
        assert "no CPU fallback" in b.last_error()
    finally:
        b.close()
