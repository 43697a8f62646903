"""The C-ABI of samples that keep their mutations and of the site-state prober over them: exported, refused on a handle without a
device, and mirrored in delphy_amd/engine.py with the header's signatures.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["emat_tree_samples_reserve_mutations", "emat_tree_sample_push_flat_mutations", "emat_tree_sample_get_mutations", "emat_tree_samples_mutation_info",
       "emat_tree_samples_probe_site_states", "emat_mcc_probe_site_states"]
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "uint8_t": C.c_uint8, "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32),
         "int64_t*": C.POINTER(C.c_int64), "const uint8_t*": C.POINTER(C.c_uint8), "uint8_t*": C.POINTER(C.c_uint8), "const double*": C.POINTER(C.c_double),
         "double*": C.POINTER(C.c_double), "emat_backend*": C.c_void_p, "const emat_pop_model*": C.POINTER(engine._PopModelC),
         "emat_samples_probe_result*": C.POINTER(engine._SamplesProbeResultC)}


def _declared(name):
    """The parameter types of `name` as include/emat_backend.h declares them."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emat_backend.h")).read(), flags=re.S)
    m = re.search(r"emat_status\s+" + name + r"\s*\((.*?)\);", text, flags=re.S)
    assert m, name + " is not declared"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", "*") for a in m.group(1).split(",")]


def test_every_new_symbol_is_exported():
    lib = C.CDLL(d.library_path())
    for name in NEW:
        assert hasattr(lib, name), "missing export: " + name


@pytest.mark.parametrize("name", NEW)
def test_the_python_mirror_has_the_headers_signature(name):
    fn = getattr(d.load_library(), name)
    assert [CTYPE[t] for t in _declared(name)] == list(fn.argtypes), name
    assert fn.restype is C.c_int


def test_every_new_call_refuses_a_handle_without_a_device():
    b = d.EmatBackend(30, device=-1)
    pop = d.PopModel.const(1.0)
    z = np.zeros(3, np.int32)
    try:
        for call in (lambda: b.tree_samples_reserve_mutations(10),
                     lambda: b.tree_sample_push_flat_mutations([-1, 0, 0], [1, -1, -1], [2, -1, -1], [0.0, 1.0, 1.0], 0, [0, 0, 0, 0], [], [], [], [], np.zeros(30, np.uint8)),
                     lambda: b.tree_samples_mutation_info(),
                     lambda: b.tree_sample_get_mutations(0),
                     lambda: b.tree_samples_probe_site_states(pop, [0], 0.0, 1.0, 2, count=1),
                     lambda: b.mcc_probe_site_states(pop, [0], 0.0, 1.0, 2)):
            with pytest.raises(d.EmatError, match="EMAT_ERR_NO_DEVICE"):
                call()
        nm = C.c_int64(0)
        assert b._lib.emat_tree_sample_get_mutations(b._h, 0, None, None, None, None, None, 0, None, C.byref(nm)) == b._lib.emat_tree_samples_reserve_mutations(b._h, 0) != 0
        assert "no CPU fallback" in b.last_error()
    finally:
        b.close()
    assert z.sum() == 0
