"""The site-rate moves' engine calls on a handle without a device: every bad argument is refused, with the offending site named,
before the device is asked for; good arguments get EMAT_ERR_NO_DEVICE (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import delphy_amd as d

L = 40


@pytest.fixture()
def handle():
    b = d.EmatBackend(L, device=-1)
    b.set_ref_sequence(np.zeros(L, np.uint8))
    b.set_hky(1e-3, 2.0, [0.25, 0.25, 0.25, 0.25])
    yield b
    b.close()


def _stats():
    return np.full(L, 3.0), np.arange(L, dtype=np.int32) % 3


def test_no_device_for_the_three_engine_calls(handle):
    T, M = _stats()
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.site_rate_moves(T, M, 1.0, 10, key=1)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.site_rate_moves(T, M, 1.0, 0, key=1, trace=False)
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.nu_l()
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        handle.debug_sample_gamma(1, 8, 0.5, 3.0)


@pytest.mark.parametrize("alpha", [0.0, -1.0, float("nan"), float("inf")])
def test_alpha_must_be_finite_and_positive(handle, alpha):
    T, M = _stats()
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*alpha"):
        handle.site_rate_moves(T, M, alpha, 10, key=1)


def test_steps_and_trace_capacity(handle):
    T, M = _stats()
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*num_alpha_steps"):
        handle.site_rate_moves(T, M, 1.0, -1, key=1)
    lib = d.load_library()
    from delphy_amd.engine import _SiteRateResultC, _SiteRateStepC
    res = _SiteRateResultC()
    buf = (_SiteRateStepC * 4)()
    res.trace = buf; res.trace_capacity = 4
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.emat_site_rate_moves(handle.handle, T.ctypes.data_as(dp), M.ctypes.data_as(ip), 1.0, 5, 1, C.byref(res)) == 1
    assert b"trace_capacity" in lib.emat_last_error(handle.handle)
    res.trace = None; res.trace_capacity = 0          # no trace: its capacity does not matter
    assert lib.emat_site_rate_moves(handle.handle, T.ctypes.data_as(dp), M.ctypes.data_as(ip), 1.0, 5, 1, C.byref(res)) == 2
    # null pointers
    assert lib.emat_site_rate_moves(handle.handle, None, M.ctypes.data_as(ip), 1.0, 5, 1, C.byref(res)) == 1
    assert lib.emat_site_rate_moves(handle.handle, T.ctypes.data_as(dp), None, 1.0, 5, 1, C.byref(res)) == 1
    assert lib.emat_site_rate_moves(handle.handle, T.ctypes.data_as(dp), M.ctypes.data_as(ip), 1.0, 5, 1, None) == 1
    assert lib.emat_site_rate_moves(None, T.ctypes.data_as(dp), M.ctypes.data_as(ip), 1.0, 5, 1, C.byref(res)) == 1
    assert lib.emat_get_nu_l(handle.handle, None) == 1
    assert lib.emat_debug_sample_gamma(handle.handle, 1, 4, 0.5, 3.0, None) == 1


@pytest.mark.parametrize("bad", [-1e-300, float("nan"), float("inf"), -float("inf")])
def test_a_bad_Ttwiddle_names_the_first_offending_site(handle, bad):
    T, M = _stats()
    T[17] = bad; T[31] = bad
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*Ttwiddle_l of site 17 "):
        handle.site_rate_moves(T, M, 1.0, 10, key=1)


def test_a_negative_count_names_the_first_offending_site(handle):
    T, M = _stats()
    M[9] = -1; M[12] = -5
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*num_muts_l of site 9 "):
        handle.site_rate_moves(T, M, 1.0, 10, key=1)
    T[11] = -1.0                                       # the first offending site, whichever array it is in
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*site 9 "):
        handle.site_rate_moves(T, M, 1.0, 10, key=1)
    T[3] = -1.0
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*site 3 "):
        handle.site_rate_moves(T, M, 1.0, 10, key=1)


def test_the_sampler_hook_refuses_bad_parameters(handle):
    for shape, rate in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, 0.0), (1.0, float("inf"))):
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
            handle.debug_sample_gamma(1, 8, shape, rate)
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
        handle.debug_sample_gamma(1, -1, 1.0, 1.0)


def test_the_run_driver_checks_its_arguments_and_defaults_to_off():
    from delphy_amd.scenarios import make_scenario
    sc = make_scenario("C1", num_tips=20, num_sites=300)
    run = d.EmatRun(None, sc.tree, sc.ref, 1)
    try:
        alpha, nu = run.site_rates()
        assert alpha == 1.0 and np.array_equal(nu, np.ones(sc.num_sites))
        for a in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
                run.set_site_rate_moves(True, a)
        run.set_site_rate_moves(True, 0.7)
        assert run.site_rates()[0] == 0.7
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.site_rate_moves()                      # no backend attached: the driver never runs moves itself
        nu0 = 0.5 + np.arange(sc.num_sites) / sc.num_sites
        run.set_hky(sc.mu, sc.kappa, sc.pi, nu0)
        assert np.array_equal(run.site_rates()[1], nu0)
    finally:
        run.close()
