"""ctypes mirror of include/emat_backend.h and include/emat_host.h.

Names and argument meaning follow the reference interface each call replaces (`Subrun` as driven by
`Run`, /root/reference core/subrun.h:16-135 and core/run.cpp:110-293,610-693); see the headers for the
file:line of every entry point.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
from dataclasses import dataclass, field, fields
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB_NAME = "libemat_hip.so"


class EmatError(RuntimeError):
    pass


STATUS_NAMES = {
    0: "EMAT_OK", 1: "EMAT_ERR_INVALID_ARGUMENT", 2: "EMAT_ERR_NO_DEVICE", 3: "EMAT_ERR_HIP", 4: "EMAT_ERR_STATE",
    5: "EMAT_ERR_CAPACITY", 6: "EMAT_ERR_INTERNAL", 7: "EMAT_ERR_BUFFER_TOO_SMALL", 8: "EMAT_ERR_IO",
}


def library_path() -> str:
    return os.environ.get("EMAT_LIB_PATH") or os.path.join(_HERE, _LIB_NAME)


def source_build_id() -> str:
    """The id csrc/Makefile would stamp into a library built from the sources as they are now: the files of its DEVSRC line, in its order."""
    import hashlib
    devsrc = [line for line in open(os.path.join(_CSRC, "Makefile")) if line.startswith("DEVSRC =")][0]
    h = hashlib.sha256()
    for f in devsrc.split("=", 1)[1].split("#")[0].split():
        h.update(open(os.path.join(_CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def library_build_id() -> str:
    """emat_build_id() of the loaded library: the device sources it was compiled from."""
    return load_library().emat_build_id().decode()


def build_library(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    path = library_path()
    if force and os.path.exists(path):
        os.remove(path)
    subprocess.run(["make", "-C", _CSRC], check=True, capture_output=not bool(os.environ.get("EMAT_VERBOSE_BUILD")))
    if not os.path.exists(path):
        raise EmatError("building %s failed" % _LIB_NAME)
    return path


class _FlatTreeC(C.Structure):
    _fields_ = [
        ("num_nodes", C.c_int32), ("root", C.c_int32),
        ("parent", C.POINTER(C.c_int32)), ("child0", C.POINTER(C.c_int32)), ("child1", C.POINTER(C.c_int32)),
        ("t", C.POINTER(C.c_double)), ("t_min", C.POINTER(C.c_float)), ("t_max", C.POINTER(C.c_float)),
        ("mut_offset", C.POINTER(C.c_int32)), ("mut_site", C.POINTER(C.c_int32)), ("mut_from", C.POINTER(C.c_uint8)),
        ("mut_to", C.POINTER(C.c_uint8)), ("mut_t", C.POINTER(C.c_double)),
        ("miss_offset", C.POINTER(C.c_int32)), ("miss_start", C.POINTER(C.c_int32)), ("miss_end", C.POINTER(C.c_int32)),
        ("mfs_offset", C.POINTER(C.c_int32)), ("mfs_site", C.POINTER(C.c_int32)), ("mfs_state", C.POINTER(C.c_uint8)),
        ("cap_muts", C.c_int32), ("cap_intervals", C.c_int32), ("cap_from_states", C.c_int32),
    ]


class _PopModelC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_double * 4), ("skygrid_type", C.c_int32), ("skygrid_num_knots", C.c_int32),
                ("skygrid_x", C.POINTER(C.c_double)), ("skygrid_gamma", C.POINTER(C.c_double))]


class _MccResultC(C.Structure):
    _fields_ = [("master_position", C.c_int32), ("master_index", C.c_int32), ("log_cc", C.POINTER(C.c_double)),
                ("parent", C.POINTER(C.c_int32)), ("child0", C.POINTER(C.c_int32)), ("child1", C.POINTER(C.c_int32)), ("root", C.c_int32),
                ("support", C.POINTER(C.c_double)), ("t", C.POINTER(C.c_double)), ("t_mrca", C.POINTER(C.c_double)), ("num_exact", C.POINTER(C.c_int32)),
                ("num_distinct_clades", C.c_int32), ("table_regrows", C.c_int32), ("table_slots", C.c_int64)]


class _SamplesProbeResultC(C.Structure):
    _fields_ = [("p", C.POINTER(C.c_double)), ("mean", C.POINTER(C.c_double)), ("num_ranks", C.c_int32), ("ranks", C.POINTER(C.c_int32)),
                ("order_stats", C.POINTER(C.c_double)), ("cells_to_skip", C.POINTER(C.c_int32))]


class _MccNodeTimesResultC(C.Structure):
    _fields_ = [("num_quantiles", C.c_int32), ("quantiles", C.POINTER(C.c_double)), ("hpd_mass", C.c_double),
                ("q_exact", C.POINTER(C.c_double)), ("q_mrca", C.POINTER(C.c_double)), ("hpd_exact", C.POINTER(C.c_double)), ("hpd_mrca", C.POINTER(C.c_double)),
                ("num_exact", C.POINTER(C.c_int32)), ("times", C.POINTER(C.c_double)), ("is_exact", C.POINTER(C.c_uint8))]


class _SiteRateStepC(C.Structure):
    _fields_ = [("proposed_alpha", C.c_double), ("log_p_proposed", C.c_double), ("log_metropolis", C.c_double), ("u", C.c_double), ("accepted", C.c_int32), ("pad_", C.c_int32)]


class _SiteRateResultC(C.Structure):
    _fields_ = [("alpha", C.c_double), ("log_p_alpha_start", C.c_double), ("num_accepted", C.c_int32), ("num_floored", C.c_int32),
                ("delta_log_G", C.c_double), ("delta_log_prior_alpha", C.c_double), ("delta_log_prior_nu", C.c_double),
                ("sum_nu_old", C.c_double), ("sum_nu_new", C.c_double), ("trace", C.POINTER(_SiteRateStepC)), ("trace_capacity", C.c_int32)]


SITE_RATE_STEP_DTYPE = np.dtype([("proposed_alpha", "f8"), ("log_p_proposed", "f8"), ("log_metropolis", "f8"), ("u", "f8"), ("accepted", "i4"), ("pad_", "i4")])
_SITE_RATE_TRACE = (_SiteRateResultC, _SiteRateStepC, SITE_RATE_STEP_DTYPE)   # what _traced_result_c makes a site-rate result of


def _traced_result(cls, res, trace):
    """A result dataclass of the global moves from its C struct: the struct's scalars under their names, in its order (a fixed array among them, the
    substitution result's pi, as a float64 array), then the trace."""
    values = [getattr(res, f.name) for f in fields(cls)[:-1]]
    return cls(*[np.array(list(v), np.float64) if isinstance(v, C.Array) else v for v in values], trace)


@dataclass
class SiteRateResult:
    """What emat_site_rate_moves returns (include/emat_backend.h: emat_site_rate_result)."""
    alpha: float                   # alpha after the steps
    log_p_alpha_start: float       # log p(alpha) at the alpha passed in
    num_accepted: int
    num_floored: int
    delta_log_G: float
    delta_log_prior_alpha: float
    delta_log_prior_nu: float
    sum_nu_old: float
    sum_nu_new: float
    trace: Optional[np.ndarray]    # [num_alpha_steps] records of SITE_RATE_STEP_DTYPE, or None when not asked for


_KEY_MASK = 0xFFFFFFFFFFFFFFFF   # a move key as the C ABI takes it: the low 64 bits


def _traced_call(owner, name: str, args, trace_of, steps: int, trace: bool, result):
    """The call `name` of the global moves on `owner` (a backend or a run): `args` after its handle, then a C result with room for `steps` trace records; the result's dataclass."""
    res, tr = _traced_result_c(*trace_of, steps, trace)
    owner._ck(getattr(owner._lib, name)(owner._h, *args, C.byref(res)), name)
    return _traced_result(result, res, tr)


def _traced_result_c(result_c, step_c, dtype, steps: int, trace: bool):
    """(a C result of the global moves with room for `steps` trace records when they are asked for, those records or None)."""
    res = result_c(); steps = max(0, int(steps))
    tr = np.zeros(max(1, steps), dtype) if trace else None
    if trace:
        res.trace = tr.ctypes.data_as(C.POINTER(step_c)); res.trace_capacity = steps
    return res, (None if tr is None else tr[:steps])


class _SkygridSpecC(C.Structure):
    _fields_ = [("tau", C.c_double), ("tau_move_enabled", C.c_int32), ("low_gamma_barrier_enabled", C.c_int32),
                ("tau_prior_alpha", C.c_double), ("tau_prior_beta", C.c_double), ("low_gamma_barrier_loc", C.c_double), ("low_gamma_barrier_scale", C.c_double),
                ("inv_nbar_prior_alpha", C.c_double), ("inv_nbar_prior_beta", C.c_double),
                ("do_tau", C.c_int32), ("do_zero_mode", C.c_int32), ("do_hmc", C.c_int32), ("hmc_steps", C.c_int32), ("hmc_mean_dt", C.c_double)]


_SKYGRID_RESULT_DOUBLES_1 = ("tau", "log_coalescent_prior_start", "log_coalescent_prior_end", "delta_log_other_priors", "tau_post_alpha", "tau_post_beta", "tau_draw",
                             "tau_delta_log_prior", "zero_B", "zero_shape", "zero_rate", "zero_I_bar", "zero_delta_gamma_bar", "zero_log_metropolis", "zero_u")
_SKYGRID_RESULT_DOUBLES_2 = ("hmc_dt", "hmc_K_old", "hmc_K_new", "hmc_U_prior_old", "hmc_U_prior_new", "hmc_U_coal_old", "hmc_U_coal_new", "hmc_log_metropolis", "hmc_u")
_SKYGRID_RESULT_INTS_1 = ("zero_accepted", "hmc_accepted")
_SKYGRID_RESULT_INTS_2 = ("hmc_K_exit_step", "hmc_nan", "hmc_steps_done")


class _SkygridResultC(C.Structure):
    _fields_ = ([("gamma", C.POINTER(C.c_double))] + [(f, C.c_double) for f in _SKYGRID_RESULT_DOUBLES_1] + [(f, C.c_int32) for f in _SKYGRID_RESULT_INTS_1] +
                [(f, C.c_double) for f in _SKYGRID_RESULT_DOUBLES_2] + [(f, C.c_int32) for f in _SKYGRID_RESULT_INTS_2] +
                [("trace_capacity", C.c_int32), ("trace", C.POINTER(C.c_double))])


@dataclass
class SkygridSpec:
    """The settings of the Skygrid population moves (include/emat_backend.h: emat_skygrid_spec); the defaults are the reference's."""
    tau: float = 1.0
    tau_move_enabled: bool = True
    low_gamma_barrier_enabled: bool = False
    tau_prior_alpha: float = 0.001
    tau_prior_beta: float = 0.001
    low_gamma_barrier_loc: float = 0.0
    low_gamma_barrier_scale: float = -math.log(0.70)
    inv_nbar_prior_alpha: float = 0.0
    inv_nbar_prior_beta: float = 0.0
    do_tau: bool = True
    do_zero_mode: bool = True
    do_hmc: bool = True
    hmc_steps: int = 25
    hmc_mean_dt: float = 2.0 * math.pi / 100.0

    def c_struct(self) -> "_SkygridSpecC":
        return _SkygridSpecC(float(self.tau), int(self.tau_move_enabled), int(self.low_gamma_barrier_enabled), float(self.tau_prior_alpha), float(self.tau_prior_beta),
                             float(self.low_gamma_barrier_loc), float(self.low_gamma_barrier_scale), float(self.inv_nbar_prior_alpha), float(self.inv_nbar_prior_beta),
                             int(self.do_tau), int(self.do_zero_mode), int(self.do_hmc), int(self.hmc_steps), float(self.hmc_mean_dt))


class SkygridMovesResult:
    """What emat_skygrid_moves returns (include/emat_backend.h: emat_skygrid_result): `gamma` [knots], every scalar of the result under
    its header name, and -- when asked for -- the trace taken apart: c_k, W_k, m_k, gamma_hmc_start, p_initial [knots] and, per leapfrog
    step made, gamma_half, f, p, gamma_after [hmc_steps_done][knots]."""

    def __init__(self, res: "_SkygridResultC", gamma: np.ndarray, trace):
        self.gamma = gamma
        for f in _SKYGRID_RESULT_DOUBLES_1 + _SKYGRID_RESULT_DOUBLES_2:
            setattr(self, f, float(getattr(res, f)))
        for f in _SKYGRID_RESULT_INTS_1 + _SKYGRID_RESULT_INTS_2:
            setattr(self, f, int(getattr(res, f)))
        self.trace = trace
        if trace is not None:
            self.c_k, self.W_k, self.m_k, self.gamma_hmc_start, self.p_initial = trace[:5]
            steps = trace[5: 5 + 4 * self.hmc_steps_done].reshape(self.hmc_steps_done, 4, trace.shape[1])
            self.gamma_half, self.f, self.p, self.gamma_after = steps[:, 0], steps[:, 1], steps[:, 2], steps[:, 3]


def _skygrid_result_c(num_knots: int, hmc_steps: int, trace: bool):
    """(the C result with room for the curve and, when asked for, the trace; the two arrays)."""
    dp = C.POINTER(C.c_double)
    gamma = np.zeros(max(1, num_knots)); res = _SkygridResultC(); res.gamma = gamma.ctypes.data_as(dp)
    tr = np.zeros((5 + 4 * max(0, int(hmc_steps)), max(1, num_knots))) if trace else None
    if trace:
        res.trace = tr.ctypes.data_as(dp); res.trace_capacity = max(0, int(hmc_steps))
    return res, gamma, tr


class _ExpPopSpecC(C.Structure):
    _fields_ = [("n0_move_enabled", C.c_int32), ("g_move_enabled", C.c_int32), ("inv_n0_prior_alpha", C.c_double), ("inv_n0_prior_beta", C.c_double),
                ("g_prior_mu", C.c_double), ("g_prior_scale", C.c_double), ("g_min", C.c_double), ("g_max", C.c_double), ("rounds", C.c_int32), ("pad_", C.c_int32)]


class _ExpPopStepC(C.Structure):
    _fields_ = [("proposed", C.c_double), ("log_coalescent_prior_proposed", C.c_double), ("log_prior_ratio", C.c_double), ("log_metropolis", C.c_double), ("u", C.c_double),
                ("accepted", C.c_int32), ("evaluated", C.c_int32)]


class _ExpPopResultC(C.Structure):
    _fields_ = [("n0", C.c_double), ("g", C.c_double), ("log_coalescent_prior_start", C.c_double), ("log_coalescent_prior_end", C.c_double), ("delta_log_other_priors", C.c_double),
                ("n0_accepted", C.c_int32), ("g_accepted", C.c_int32), ("g_out_of_bounds", C.c_int32), ("pad_", C.c_int32),
                ("trace", C.POINTER(_ExpPopStepC)), ("trace_capacity", C.c_int32)]


EXP_POP_STEP_DTYPE = np.dtype([("proposed", "f8"), ("log_coalescent_prior_proposed", "f8"), ("log_prior_ratio", "f8"), ("log_metropolis", "f8"), ("u", "f8"),
                               ("accepted", "i4"), ("evaluated", "i4")])
_EXP_POP_TRACE = (_ExpPopResultC, _ExpPopStepC, EXP_POP_STEP_DTYPE)   # ... and one of the Exponential population moves (steps = 2 * rounds)


@dataclass
class ExpPopSpec:
    """The settings of the Exponential population moves (include/emat_backend.h: emat_exp_pop_spec); the defaults are the reference's."""
    n0_move_enabled: bool = True
    g_move_enabled: bool = True
    inv_n0_prior_alpha: float = 0.0
    inv_n0_prior_beta: float = 0.0
    g_prior_mu: float = 0.001 / 365.0
    g_prior_scale: float = 30.701135 / 365.0
    g_min: float = -math.inf
    g_max: float = math.inf
    rounds: int = 50

    def c_struct(self) -> "_ExpPopSpecC":
        return _ExpPopSpecC(int(self.n0_move_enabled), int(self.g_move_enabled), float(self.inv_n0_prior_alpha), float(self.inv_n0_prior_beta),
                            float(self.g_prior_mu), float(self.g_prior_scale), float(self.g_min), float(self.g_max), int(self.rounds), 0)


@dataclass
class ExpPopMovesResult:
    """What emat_exp_pop_moves returns (include/emat_backend.h: emat_exp_pop_result)."""
    n0: float
    g: float
    log_coalescent_prior_start: float
    log_coalescent_prior_end: float
    delta_log_other_priors: float
    n0_accepted: int
    g_accepted: int
    g_out_of_bounds: int
    trace: Optional[np.ndarray]    # [2 * rounds] records of EXP_POP_STEP_DTYPE (even: n0 steps, odd: g steps), or None when not asked for


class _SubstSpecC(C.Structure):
    _fields_ = [("mu", C.c_double), ("kappa", C.c_double), ("pi", C.c_double * 4), ("mu_prior_alpha", C.c_double), ("mu_prior_beta", C.c_double),
                ("do_mu", C.c_int32), ("do_pi", C.c_int32), ("do_kappa", C.c_int32), ("rounds", C.c_int32)]


class _SubstStepC(C.Structure):
    _fields_ = [("kappa", C.c_double), ("pi", C.c_double * 4), ("proposal", C.c_double), ("delta_log_G", C.c_double), ("log_prior_ratio", C.c_double),
                ("log_metropolis", C.c_double), ("u", C.c_double), ("ia", C.c_int32), ("ib", C.c_int32), ("accepted", C.c_int32), ("evaluated", C.c_int32),
                ("left_unit", C.c_int32), ("force_rejected", C.c_int32)]


class _SubstResultC(C.Structure):
    _fields_ = [("mu", C.c_double), ("kappa", C.c_double), ("pi", C.c_double * 4), ("mu_post_shape", C.c_double), ("mu_post_rate", C.c_double), ("mu_draw", C.c_double),
                ("delta_log_G", C.c_double), ("delta_log_other_priors", C.c_double), ("mu_delta_log_G", C.c_double), ("mu_delta_log_other_priors", C.c_double),
                ("pi_accepted", C.c_int32), ("kappa_accepted", C.c_int32), ("pi_left_unit", C.c_int32), ("forced_rejections", C.c_int32),
                ("trace", C.POINTER(_SubstStepC)), ("trace_capacity", C.c_int32)]


SUBST_STEP_DTYPE = np.dtype([("kappa", "f8"), ("pi", "f8", (4,)), ("proposal", "f8"), ("delta_log_G", "f8"), ("log_prior_ratio", "f8"), ("log_metropolis", "f8"), ("u", "f8"),
                             ("ia", "i4"), ("ib", "i4"), ("accepted", "i4"), ("evaluated", "i4"), ("left_unit", "i4"), ("force_rejected", "i4")])
_SUBST_TRACE = (_SubstResultC, _SubstStepC, SUBST_STEP_DTYPE)   # ... and one of the substitution-model moves (steps = 2 * rounds)


@dataclass
class SubstSpec:
    """The settings of the substitution-model moves (include/emat_backend.h: emat_subst_spec) with the linked HKY model they start from; the
    defaults of the prior, the switches and the rounds are the reference's."""
    mu: float = 1e-3
    kappa: float = 1.0
    pi: Sequence[float] = (0.25, 0.25, 0.25, 0.25)
    mu_prior_alpha: float = 1.0
    mu_prior_beta: float = 0.0
    do_mu: bool = True
    do_pi: bool = True
    do_kappa: bool = True
    rounds: int = 10

    def c_struct(self) -> "_SubstSpecC":
        return _SubstSpecC(float(self.mu), float(self.kappa), (C.c_double * 4)(*[float(v) for v in self.pi]), float(self.mu_prior_alpha), float(self.mu_prior_beta),
                           int(self.do_mu), int(self.do_pi), int(self.do_kappa), int(self.rounds))


@dataclass
class SubstMovesResult:
    """What emat_subst_moves returns (include/emat_backend.h: emat_subst_result)."""
    mu: float
    kappa: float
    pi: np.ndarray                 # [4]
    mu_post_shape: float
    mu_post_rate: float
    mu_draw: float
    delta_log_G: float
    delta_log_other_priors: float
    mu_delta_log_G: float
    mu_delta_log_other_priors: float
    pi_accepted: int
    kappa_accepted: int
    pi_left_unit: int
    forced_rejections: int
    trace: Optional[np.ndarray]    # [2 * rounds] records of SUBST_STEP_DTYPE (even: pi steps, odd: kappa steps), or None when not asked for


class _MpoxSpecC(C.Structure):
    _fields_ = [("mu", C.c_double), ("mu_star", C.c_double), ("mu_prior_alpha", C.c_double), ("mu_prior_beta", C.c_double), ("do_mu", C.c_int32), ("rounds", C.c_int32)]


_MPOX_ROUND_DOUBLES = ("mu", "rho", "Ttwiddle_eff", "mu_shape", "mu_rate", "mu_draw", "mu_delta_log_G", "mu_delta_log_other_priors",
                       "alpha", "beta", "Q_lo", "Q_hi", "u", "rand_Q", "y", "k", "new_rho", "rho_delta_log_G")
_MPOX_ROUND_INTS = ("mu_done", "rho_done", "rho_degenerate", "reserved")


class _MpoxRoundC(C.Structure):
    _fields_ = [(f, C.c_double) for f in _MPOX_ROUND_DOUBLES] + [(f, C.c_int32) for f in _MPOX_ROUND_INTS]


class _MpoxResultC(C.Structure):
    _fields_ = [("mu", C.c_double), ("mu_star", C.c_double), ("M", C.c_double), ("M_star", C.c_double), ("Ttwiddle", C.c_double), ("Ttwiddle_star", C.c_double),
                ("delta_log_G", C.c_double), ("delta_log_other_priors", C.c_double), ("rho_skipped", C.c_int32), ("rho_degenerate", C.c_int32),
                ("trace", C.POINTER(_MpoxRoundC)), ("trace_capacity", C.c_int32)]


MPOX_ROUND_DTYPE = np.dtype([(f, "f8") for f in _MPOX_ROUND_DOUBLES] + [(f, "i4") for f in _MPOX_ROUND_INTS])
_MPOX_TRACE = (_MpoxResultC, _MpoxRoundC, MPOX_ROUND_DTYPE)   # ... and one of the APOBEC model's moves (steps = rounds)


@dataclass
class MpoxSpec:
    """The settings of the APOBEC (mpox) model's moves (include/emat_backend.h: emat_mpox_spec) with the mu and mu* they start from; the defaults of
    the prior, the switch and the rounds are the reference's."""
    mu: float = 1e-3
    mu_star: float = 0.0
    mu_prior_alpha: float = 1.0
    mu_prior_beta: float = 0.0
    do_mu: bool = True
    rounds: int = 10

    def c_struct(self) -> "_MpoxSpecC":
        return _MpoxSpecC(float(self.mu), float(self.mu_star), float(self.mu_prior_alpha), float(self.mu_prior_beta), int(self.do_mu), int(self.rounds))


@dataclass
class MpoxMovesResult:
    """What emat_mpox_moves returns (include/emat_backend.h: emat_mpox_result)."""
    mu: float
    mu_star: float
    M: float
    M_star: float
    Ttwiddle: float
    Ttwiddle_star: float
    delta_log_G: float
    delta_log_other_priors: float
    rho_skipped: int
    rho_degenerate: int
    trace: Optional[np.ndarray]    # [rounds] records of MPOX_ROUND_DTYPE, or None when not asked for


def mpox_q_matrices(rho: float):
    """(q0, q1) [4][4] of the APOBEC model at rho = mu* / mu: Run::derive_evo (reference run.cpp:407-432), as mpox_derive_q (csrc/emat_move_specs.hpp) spells it."""
    q0 = np.full((4, 4), 1.0 / 3.0); np.fill_diagonal(q0, -1.0)
    q1 = q0.copy()
    q1[1, 3] += 2 * rho; q1[1, 1] -= 2 * rho
    q1[2, 0] += 2 * rho; q1[2, 2] -= 2 * rho
    return q0, q1


@dataclass
class SamplesProbe:
    """What emat_tree_samples_probe_ancestors / emat_mcc_probe_ancestors return (include/emat_backend.h: emat_samples_probe_result).
    The site-state forms return the same with a site axis: `members` below reads [sites][4]."""
    p: Optional[np.ndarray]            # [count][members][cells] every chosen sample's probabilities, or None when not asked for
    mean: Optional[np.ndarray]         # [members][cells] their mean, added in sample order
    order_stats: Optional[np.ndarray]  # [ranks][members][cells] the ranks[j]-th smallest over the samples, or None without ranks
    cells_to_skip: np.ndarray          # [count] cells each sample's grid was extended by to reach its root


@dataclass
class MccTree:
    """What emat_mcc_derive returns (include/emat_backend.h: emat_mcc_result; reference Mcc_tree)."""
    master: int                 # which of the chosen samples is the master ...
    master_index: int           # ... and its slot in the store
    log_cc: np.ndarray          # [count] log clade credibility of every chosen sample
    parent: np.ndarray          # the MCC tree's topology = the master's
    child0: np.ndarray
    child1: np.ndarray
    root: int
    support: np.ndarray         # [n] posterior support = num_exact / count
    t: np.ndarray               # [n] mean time over the samples that have the node's clade
    t_mrca: np.ndarray          # [n] mean time of the MRCA of the node's tips over all samples
    num_exact: np.ndarray       # [n] samples that have the node's clade
    num_distinct_clades: int
    table_regrows: int
    table_slots: int


@dataclass
class MccNodeTimes:
    """What emat_mcc_node_times returns (include/emat_backend.h: emat_mcc_node_times_result): per node asked for, over the samples of the
    last derivation.  `exact`: the samples that have the node's clade; `mrca`: all of them."""
    nodes: np.ndarray                  # [nodes] the MCC nodes answered, as asked for
    quantiles: np.ndarray              # [q] as asked for
    hpd_mass: float
    num_exact: np.ndarray              # [nodes] samples that have the node's clade
    q_exact: Optional[np.ndarray]      # [q][nodes], or None without quantiles
    q_mrca: Optional[np.ndarray]
    hpd_exact: Optional[np.ndarray]    # [2][nodes]: lo, hi of the shortest interval holding hpd_mass of the values, or None with hpd_mass 0
    hpd_mrca: Optional[np.ndarray]
    times: Optional[np.ndarray]        # [nodes][count] the corresponding node's time in every sample, in sample order, or None unless per_sample
    is_exact: Optional[np.ndarray]     # [nodes][count] bool


@dataclass
class MccMutationSupport:
    """What emat_mcc_mutation_support returns: per mutation of the master, in the order tree_sample_get_mutations(master slot) lists them."""
    num_with: np.ndarray               # [records] samples that have the node's clade and the mutation on its branch
    mean_t: np.ndarray                 # [records] mean time of the mutation over those samples, summed in sample order
    t_min: np.ndarray                  # [records] its earliest ...
    t_max: np.ndarray                  # ... and latest time


class _TipDescsC(C.Structure):
    _fields_ = [("num_tips", C.c_int32), ("t_min", C.POINTER(C.c_float)), ("t_max", C.POINTER(C.c_float)),
                ("delta_offset", C.POINTER(C.c_int32)), ("delta_site", C.POINTER(C.c_int32)), ("delta_to", C.POINTER(C.c_uint8)),
                ("miss_offset", C.POINTER(C.c_int32)), ("miss_start", C.POINTER(C.c_int32)), ("miss_end", C.POINTER(C.c_int32))]


class TipDescs:
    """The builder's input (include/emat_backend.h: emat_tip_descs; reference Tip_desc): per tip a date range, its differences
    from the reference sequence (CSR, ascending sites) and its missing intervals (CSR)."""

    def __init__(self, t_min, t_max, delta_offset, delta_site, delta_to, miss_offset, miss_start, miss_end):
        self.t_min = np.ascontiguousarray(t_min, np.float32); self.t_max = np.ascontiguousarray(t_max, np.float32)
        self.delta_offset = np.ascontiguousarray(delta_offset, np.int32); self.delta_site = np.ascontiguousarray(delta_site, np.int32)
        self.delta_to = np.ascontiguousarray(delta_to, np.uint8)
        self.miss_offset = np.ascontiguousarray(miss_offset, np.int32); self.miss_start = np.ascontiguousarray(miss_start, np.int32)
        self.miss_end = np.ascontiguousarray(miss_end, np.int32)
        self.num_tips = int(self.t_min.shape[0])

    def c_struct(self) -> "_TipDescsC":
        return _TipDescsC(self.num_tips, _ptr(self.t_min, C.c_float), _ptr(self.t_max, C.c_float), _ptr(self.delta_offset, C.c_int32), _ptr(self.delta_site, C.c_int32),
                          _ptr(self.delta_to, C.c_uint8), _ptr(self.miss_offset, C.c_int32), _ptr(self.miss_start, C.c_int32), _ptr(self.miss_end, C.c_int32))


class _AlignReportC(C.Structure):
    _fields_ = [("num_rows", C.c_int64), ("num_tips", C.c_int32), ("num_invalid", C.c_int32), ("num_undated", C.c_int32),
                ("num_deltas", C.c_int64), ("num_intervals", C.c_int64), ("num_precision_loss", C.c_int64)]


class _AlignArraysC(C.Structure):
    _fields_ = [("delta_offset", C.POINTER(C.c_int32)), ("delta_site", C.POINTER(C.c_int32)), ("delta_to", C.POINTER(C.c_uint8)),
                ("miss_offset", C.POINTER(C.c_int32)), ("miss_start", C.POINTER(C.c_int32)), ("miss_end", C.POINTER(C.c_int32)),
                ("ref_sequence", C.POINTER(C.c_uint8)), ("counts", C.POINTER(C.c_int32)), ("row_status", C.POINTER(C.c_int32)),
                ("row_bad_site", C.POINTER(C.c_int32)), ("row_bad_byte", C.POINTER(C.c_uint8)), ("row_precision_loss", C.POINTER(C.c_int32))]


class _FastaReportC(C.Structure):
    _fields_ = [("num_records", C.c_int32), ("num_dated", C.c_int32), ("names_bytes", C.c_int64), ("rows", _AlignReportC)]


class Alignment:
    """What emat_align_finish made of the rows pushed (include/emat_backend.h: emat_align_report, emat_align_arrays): `tips`, a TipDescs
    without dates unless they were given; `ref`, the given reference sequence or the consensus; `counts` [L, 4]; per input row `row_status`
    (tip index, -1 undated, -2 invalid), `row_bad_site`, `row_bad_byte` and `row_precision_loss`; and the totals in `report`."""

    def __init__(self, tips, ref, counts, row_status, row_bad_site, row_bad_byte, row_precision_loss, report):
        self.tips = tips; self.ref = ref; self.counts = counts
        self.row_status = row_status; self.row_bad_site = row_bad_site; self.row_bad_byte = row_bad_byte; self.row_precision_loss = row_precision_loss
        self.report = report


class _ConfigC(C.Structure):
    _fields_ = [("device", C.c_int32), ("num_sites", C.c_int32), ("max_parts", C.c_int32), ("slab_slack", C.c_double),
                ("trace_moves", C.c_int32), ("use_lds", C.c_int32)]


class _PartStatsC(C.Structure):
    _fields_ = [("status", C.c_int32), ("num_nodes", C.c_int32), ("moves_done", C.c_int64), ("proposed", C.c_int64 * 5),
                ("accepted", C.c_int64 * 5), ("algorithmic_bytes", C.c_int64), ("rng_draws", C.c_int64), ("device_ticks", C.c_int64), ("algorithmic_write_bytes", C.c_int64)]


class _SynthParamsC(C.Structure):
    _fields_ = [("num_tips", C.c_int32), ("num_sites", C.c_int32), ("tip_span", C.c_double), ("tip_date_uncertainty", C.c_double),
                ("frac_uncertain_tips", C.c_double), ("pop_n0", C.c_double), ("pop_growth", C.c_double), ("mu", C.c_double),
                ("kappa", C.c_double), ("pi", C.c_double * 4), ("gaps_per_tip", C.c_int32), ("mean_gap_len", C.c_double), ("seed", C.c_uint64)]


def _ptr(a: np.ndarray, ct):
    return a.ctypes.data_as(C.POINTER(ct))


@dataclass
class FlatTree:
    """numpy owner of an `emat_flat_tree` (struct-of-arrays + CSR lists; include/emat_backend.h)."""
    root: int
    parent: np.ndarray
    child0: np.ndarray
    child1: np.ndarray
    t: np.ndarray
    t_min: np.ndarray
    t_max: np.ndarray
    mut_offset: np.ndarray
    mut_site: np.ndarray
    mut_from: np.ndarray
    mut_to: np.ndarray
    mut_t: np.ndarray
    miss_offset: np.ndarray
    miss_start: np.ndarray
    miss_end: np.ndarray
    mfs_offset: np.ndarray
    mfs_site: np.ndarray
    mfs_state: np.ndarray

    @property
    def num_nodes(self) -> int:
        return int(self.parent.shape[0])

    @staticmethod
    def empty(n: int, nm: int, ni: int, nf: int) -> "FlatTree":
        i32, f64, f32, u8 = np.int32, np.float64, np.float32, np.uint8
        return FlatTree(-1, np.full(n, -1, i32), np.full(n, -1, i32), np.full(n, -1, i32), np.zeros(n, f64), np.zeros(n, f32), np.zeros(n, f32),
                        np.zeros(n + 1, i32), np.zeros(max(nm, 1), i32), np.zeros(max(nm, 1), u8), np.zeros(max(nm, 1), u8), np.zeros(max(nm, 1), f64),
                        np.zeros(n + 1, i32), np.zeros(max(ni, 1), i32), np.zeros(max(ni, 1), i32),
                        np.zeros(n + 1, i32), np.zeros(max(nf, 1), i32), np.zeros(max(nf, 1), u8))

    def c_view(self) -> _FlatTreeC:
        v = _FlatTreeC()
        v.num_nodes = self.num_nodes
        v.root = self.root
        v.parent, v.child0, v.child1 = _ptr(self.parent, C.c_int32), _ptr(self.child0, C.c_int32), _ptr(self.child1, C.c_int32)
        v.t, v.t_min, v.t_max = _ptr(self.t, C.c_double), _ptr(self.t_min, C.c_float), _ptr(self.t_max, C.c_float)
        v.mut_offset, v.mut_site = _ptr(self.mut_offset, C.c_int32), _ptr(self.mut_site, C.c_int32)
        v.mut_from, v.mut_to, v.mut_t = _ptr(self.mut_from, C.c_uint8), _ptr(self.mut_to, C.c_uint8), _ptr(self.mut_t, C.c_double)
        v.miss_offset, v.miss_start, v.miss_end = _ptr(self.miss_offset, C.c_int32), _ptr(self.miss_start, C.c_int32), _ptr(self.miss_end, C.c_int32)
        v.mfs_offset, v.mfs_site, v.mfs_state = _ptr(self.mfs_offset, C.c_int32), _ptr(self.mfs_site, C.c_int32), _ptr(self.mfs_state, C.c_uint8)
        v.cap_muts, v.cap_intervals, v.cap_from_states = self.mut_site.shape[0], self.miss_start.shape[0], self.mfs_site.shape[0]
        return v

    def trimmed(self) -> "FlatTree":
        """Drop the padding of the variable-length arrays (after a download)."""
        n = self.num_nodes
        nm, ni, nf = int(self.mut_offset[n]), int(self.miss_offset[n]), int(self.mfs_offset[n])
        return FlatTree(self.root, self.parent, self.child0, self.child1, self.t, self.t_min, self.t_max,
                        self.mut_offset, self.mut_site[:nm].copy(), self.mut_from[:nm].copy(), self.mut_to[:nm].copy(), self.mut_t[:nm].copy(),
                        self.miss_offset, self.miss_start[:ni].copy(), self.miss_end[:ni].copy(),
                        self.mfs_offset, self.mfs_site[:nf].copy(), self.mfs_state[:nf].copy())

    @staticmethod
    def from_c_view(v: _FlatTreeC) -> "FlatTree":
        n = v.num_nodes
        def arr(p, cnt, dt):
            return np.ctypeslib.as_array(p, shape=(max(cnt, 1),)).astype(dt, copy=True)[:cnt] if cnt > 0 else np.zeros(0, dt)
        mo = arr(v.mut_offset, n + 1, np.int32)
        io = arr(v.miss_offset, n + 1, np.int32)
        fo = arr(v.mfs_offset, n + 1, np.int32)
        nm, ni, nf = int(mo[n]), int(io[n]), int(fo[n])
        def padded(a, dt):
            return a if a.shape[0] > 0 else np.zeros(1, dt)
        return FlatTree(v.root, arr(v.parent, n, np.int32), arr(v.child0, n, np.int32), arr(v.child1, n, np.int32),
                        arr(v.t, n, np.float64), arr(v.t_min, n, np.float32), arr(v.t_max, n, np.float32),
                        mo, padded(arr(v.mut_site, nm, np.int32), np.int32), padded(arr(v.mut_from, nm, np.uint8), np.uint8),
                        padded(arr(v.mut_to, nm, np.uint8), np.uint8), padded(arr(v.mut_t, nm, np.float64), np.float64),
                        io, padded(arr(v.miss_start, ni, np.int32), np.int32), padded(arr(v.miss_end, ni, np.int32), np.int32),
                        fo, padded(arr(v.mfs_site, nf, np.int32), np.int32), padded(arr(v.mfs_state, nf, np.uint8), np.uint8))


@dataclass
class PopModel:
    """Population model descriptor (reference core/pop_model.h): kind 0 const{pop}, 1 exp{t0,n0,g,min_pop}, 2 skygrid."""
    kind: int = 0
    p: Sequence[float] = (1.0, 0.0, 0.0, 0.0)
    skygrid_type: int = 1
    skygrid_x: Optional[np.ndarray] = None
    skygrid_gamma: Optional[np.ndarray] = None
    _keep: list = field(default_factory=list, repr=False)

    @staticmethod
    def const(pop: float) -> "PopModel":
        return PopModel(0, (pop, 0.0, 0.0, 0.0))

    @staticmethod
    def exp(t0: float, n0: float, g: float, min_pop: float = 0.0) -> "PopModel":
        return PopModel(1, (t0, n0, g, min_pop))

    @staticmethod
    def skygrid(x, gamma, log_linear: bool = False) -> "PopModel":
        return PopModel(2, (0.0, 0.0, 0.0, 0.0), 2 if log_linear else 1, np.ascontiguousarray(x, np.float64), np.ascontiguousarray(gamma, np.float64))

    def c_struct(self) -> _PopModelC:
        m = _PopModelC()
        m.kind = self.kind
        for i in range(4):
            m.p[i] = float(self.p[i])
        m.skygrid_type = self.skygrid_type
        if self.kind == 2:
            m.skygrid_num_knots = int(self.skygrid_x.shape[0])
            m.skygrid_x = _ptr(self.skygrid_x, C.c_double)
            m.skygrid_gamma = _ptr(self.skygrid_gamma, C.c_double)
        return m


@dataclass
class SynthParams:
    num_tips: int = 100
    num_sites: int = 30000
    tip_span: float = 365.0
    tip_date_uncertainty: float = 0.0
    frac_uncertain_tips: float = 0.0
    pop_n0: float = 365.0
    pop_growth: float = 0.0
    mu: float = 1e-3 / 365.0
    kappa: float = 5.0
    pi: Sequence[float] = (0.31, 0.19, 0.21, 0.29)
    gaps_per_tip: int = 2
    mean_gap_len: float = 150.0
    seed: int = 20261001


_lib = None


def load_library():
    """Load libemat_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise EmatError("%s is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback" % path)
    lib = C.CDLL(path)
    B, R, S = C.c_void_p, C.c_void_p, C.c_void_p
    i32, i64, u64, dbl = C.c_int32, C.c_int64, C.c_uint64, C.c_double
    P = C.POINTER
    sigs = {
        "emat_backend_create": [P(_ConfigC), P(B)], "emat_backend_destroy": [B],
        "emat_set_ref_sequence": [B, P(C.c_uint8), i32],
        "emat_set_evo": [B, i32, P(dbl), P(dbl), P(dbl), P(dbl), P(i32)],
        "emat_set_flags": [B, dbl, i32, i32],
        "emat_begin_upload": [B, i32], "emat_part_upload": [B, i32, P(_FlatTreeC), i32, u64], "emat_end_upload": [B],
        "emat_build_coalescent_parts": [B, P(_PopModelC), i32, dbl],
        "emat_coalescent_begin": [B, P(_PopModelC), i32, dbl, P(dbl), P(dbl)], "emat_coalescent_set_range": [B, dbl, dbl, P(i32)],
        "emat_coalescent_local_grid": [B, P(dbl), P(i32)], "emat_coalescent_sample": [B, P(dbl), P(i32), P(dbl)], "emat_coalescent_finish": [B, P(dbl)],
        "emat_run_local_moves": [B, i64], "emat_run_moves_per_part": [B, i64], "emat_synchronize": [B], "emat_recalc_derived": [B],
        "emat_get_totals": [B, P(dbl), P(dbl)], "emat_get_global_stats": [B, i32, P(dbl), P(i64), P(i64)],
        "emat_part_get_sizes": [B, i32, P(i32), P(i32), P(i32), P(i32)], "emat_part_download": [B, i32, P(_FlatTreeC)],
        "emat_part_get_derived": [B, i32, P(dbl), P(i32), P(dbl), P(dbl)], "emat_part_get_state_frequencies": [B, i32, P(i32), P(i32)],
        "emat_part_get_coalescent": [B, i32, P(i32), P(dbl), P(dbl), P(dbl), P(dbl), P(i32), P(dbl), P(dbl)],
        "emat_tree_build_usher_like": [B, P(_TipDescsC), u64], "emat_tree_build_default": [B, P(_TipDescsC), u64, P(i32)], "emat_tree_built_ref": [B, P(C.c_uint8)], "emat_tree_built_sizes": [B, P(i32), P(i32), P(i32), P(i32)], "emat_tree_built_get": [B, P(_FlatTreeC)],
        "emat_part_get_rng": [B, i32, P(u64), P(u64), P(u64), P(i32)], "emat_check_derived": [B, dbl, P(i32), P(dbl)], "emat_debug_slab_layout": [B, i32, P(C.c_uint32)],
        "emat_part_get_stats": [B, i32, P(_PartStatsC)], "emat_part_get_trace": [B, i32, P(i32), P(dbl)],
        "emat_last_run_ms": [B, P(dbl)], "emat_last_kernel_ms": [B, P(dbl), P(i32)],
        "emat_debug_gamma": [B, i32, i32, P(dbl), P(dbl), P(dbl)],
        "emat_debug_pop": [B, P(_PopModelC), i32, i32, P(dbl), P(dbl), P(dbl)], "emat_debug_interval_op": [B, i32, P(i32), i32, P(i32), i32, P(i32), P(i32)],
        "emat_debug_tree_query": [B, i32, i32, i32, P(i32), P(i32), P(i32)],
        "emat_set_option": [B, C.c_char_p, C.c_char_p], "emat_set_host_threads": [i32],
        "emat_debug_graft": [B, i32, i32, dbl, i32, i32, dbl, P(dbl), i32, P(i32)], "emat_debug_edit": [B, i32, i32, i32, P(i32), P(i32), P(dbl)],
        "emat_debug_sample_history": [B, i32, i32, P(i32), P(dbl), P(C.c_uint8), dbl, dbl, P(i32), P(dbl), i32, P(i32)],
        "emat_get_num_muts_l": [B, P(i32)], "emat_get_scalable_coalescent_log_prior": [B, dbl, dbl, P(dbl)],
        "emat_scalable_coalescent_partial": [B, dbl, dbl, i32, i32, P(dbl), P(dbl), P(i32)],
        "emat_scalable_coalescent_log_prior": [B, dbl, dbl, i32, i32, P(dbl), dbl, P(dbl)],
        "emat_synth_create": [P(_SynthParamsC), P(S)], "emat_synth_get": [S, P(_FlatTreeC), P(P(C.c_uint8)), P(dbl)],
        "emat_run_create": [B, P(_FlatTreeC), P(C.c_uint8), i32, u64, P(R)], "emat_run_destroy": [R],
        "emat_run_set_num_parts": [R, i32], "emat_run_set_max_part_nodes": [R, i32], "emat_run_partition_stats": [R, P(i32), P(i32), P(i32), P(i32)], "emat_run_debug_redraw_partition": [R, P(i32), P(i32)], "emat_run_follow_draws": [R, R], "emat_run_draw_partition": [R], "emat_run_set_hky": [R, dbl, dbl, P(dbl), P(dbl)], "emat_run_set_pop_model": [R, P(_PopModelC)],
        "emat_run_set_coalescent_t_step": [R, dbl], "emat_run_set_flags": [R, i32, i32],
        "emat_run_repartition": [R], "emat_run_num_parts": [R, P(i32), P(i32)],
        "emat_run_part_sizes": [R, i32, P(i32), P(i32), P(i32), P(i32)], "emat_run_part_get": [R, i32, P(_FlatTreeC), P(i32), P(u64)],
        "emat_run_part_put": [R, i32, P(_FlatTreeC)], "emat_run_push_params": [R], "emat_run_moves": [R, i64], "emat_run_reassemble": [R],
        "emat_run_set_shard": [R, i32, i32], "emat_run_shard_range": [R, P(i32), P(i32), P(i32)], "emat_run_coalescent_begin": [R, P(dbl), P(dbl)],
        "emat_run_moves_sharded": [R, i64], "emat_run_pack_local_parts": [R, P(C.c_uint8), u64, P(u64)], "emat_run_unpack_parts": [R, P(C.c_uint8), u64],
        "emat_run_moves_split": [B, i64, i64], "emat_run_get_Ttwiddle_l": [R, P(dbl)], "emat_run_Ttwiddle_ext": [R, P(dbl), P(i32), P(i32), P(dbl), i32, P(i32)],
        "emat_get_part_tree_lengths": [B, P(dbl)], "emat_Ttwiddle_l_partial": [B, P(i32), P(i32), P(dbl), P(dbl), P(dbl), P(dbl)],
        "emat_Ttwiddle_l_finish": [B, P(dbl), P(dbl), dbl, P(dbl)],
        "emat_run_do_mcmc_steps": [R, i64, i64], "emat_run_tree_sizes": [R, P(i32), P(i32), P(i32), P(i32)],
        "emat_run_tree_get": [R, P(_FlatTreeC), P(C.c_uint8)], "emat_run_t_max_tip": [R, P(dbl)],
        "emat_run_set_device_tree": [R, i32], "emat_run_moves_even": [B, i64, i32], "emat_debug_tree_counters": [B, P(i32)],
        "emat_tree_upload": [B, P(_FlatTreeC)], "emat_tree_get_sizes": [B, P(i32), P(i32), P(i32), P(i32)], "emat_tree_download": [B, P(_FlatTreeC), P(C.c_uint8)],
        "emat_tree_get_topology": [B, P(i32), P(i32), P(i32), P(dbl), P(i32)],
        "emat_tree_get_kids": [B, P(P(i32)), P(i32), P(i32), P(dbl)],
        "emat_tree_repartition": [B, i32, P(i32), P(i32), P(i32), P(i32), i32, P(u64), P(_PopModelC), dbl],
        "emat_tree_reassemble": [B, P(i32), P(i32), P(C.c_uint8), P(C.c_uint8), i32],
        "emat_tree_partition": [B, i32, P(i32), P(i32), P(i32), P(i32)], "emat_tree_get_partition": [B, P(i32), P(i32), P(i32), P(i32)],
        "emat_tree_repartition_range": [B, i32, P(i32), P(i32), P(i32), P(i32), i32, P(u64), P(_PopModelC), dbl, i32, i32],
        "emat_tree_get_root_deltas": [B, P(i32), P(i32), P(C.c_uint8), P(C.c_uint8), i32], "emat_tree_gather_local": [B, i32, P(i32), P(C.c_uint8), P(C.c_uint8)],
        "emat_tree_export_nodes": [B, P(C.c_uint8), u64, P(u64)], "emat_tree_apply_nodes": [B, P(C.c_uint8), u64], "emat_tree_reassemble_end": [B],
        "emat_tree_probe_ancestors": [B, P(_PopModelC), i32, P(i32), dbl, dbl, i32, P(dbl)], "emat_tree_probe_site_states": [B, P(_PopModelC), i32, dbl, dbl, i32, P(dbl)],
        "emat_tree_branch_counts": [B, i32, i32, P(i32), i32, dbl, dbl, i32, P(i32), P(i32), P(dbl), P(dbl), i64],
        "emat_tree_samples_reserve": [B, i32], "emat_tree_sample_push": [B, P(i32)], "emat_tree_sample_push_flat": [B, i32, P(i32), P(i32), P(i32), P(dbl), i32, P(i32)],
        "emat_tree_samples_count": [B, P(i32), P(i32), P(i32)], "emat_tree_samples_clear": [B], "emat_tree_sample_get": [B, i32, P(i32), P(i32), P(i32), P(dbl), P(i32)],
        "emat_mcc_derive": [B, i32, i32, i32, u64, P(_MccResultC)], "emat_mcc_get_correspondence": [B, i32, P(i32), P(C.c_uint8)],
        "emat_tree_samples_probe_ancestors": [B, P(_PopModelC), i32, i32, i32, i32, i32, P(i32), i32, dbl, dbl, i32, P(_SamplesProbeResultC)],
        "emat_mcc_probe_ancestors": [B, P(_PopModelC), i32, i32, P(i32), dbl, dbl, i32, P(_SamplesProbeResultC)], "emat_mcc_get_derivation": [B, P(i32), P(i32), P(i32)],
        "emat_tree_samples_reserve_mutations": [B, i64],
        "emat_tree_sample_push_flat_mutations": [B, i32, P(i32), P(i32), P(i32), P(dbl), i32, P(i32), P(i32), P(C.c_uint8), P(C.c_uint8), P(dbl), P(C.c_uint8), P(i32)],
        "emat_tree_sample_get_mutations": [B, i32, P(i32), P(i32), P(C.c_uint8), P(C.c_uint8), P(dbl), i64, P(C.c_uint8), P(i64)],
        "emat_tree_samples_mutation_info": [B, P(i64), P(i64), P(i32)],
        "emat_tree_samples_probe_site_states": [B, P(_PopModelC), i32, i32, i32, i32, i32, P(i32), dbl, dbl, i32, P(_SamplesProbeResultC)],
        "emat_mcc_probe_site_states": [B, P(_PopModelC), i32, i32, P(i32), dbl, dbl, i32, P(_SamplesProbeResultC)],
        "emat_mcc_node_times": [B, i32, P(i32), P(_MccNodeTimesResultC)], "emat_mcc_mutation_support": [B, i64, P(i64), P(i32), P(dbl), P(dbl), P(dbl)],
        "emat_run_note_device_reassembled": [R, i32, P(i32), P(C.c_uint8)], "emat_run_set_paranoid": [R, i32], "emat_run_set_reference_remainder": [R, i32],
        "emat_site_rate_moves": [B, P(dbl), P(i32), dbl, i32, u64, P(_SiteRateResultC)], "emat_get_nu_l": [B, P(dbl)], "emat_debug_sample_gamma": [B, u64, i32, dbl, dbl, P(dbl)],
        "emat_skygrid_moves": [B, P(_PopModelC), P(_SkygridSpecC), dbl, dbl, i32, i32, P(dbl), i32, P(dbl), u64, P(_SkygridResultC)],
        "emat_debug_pop_gradient": [B, P(_PopModelC), i32, i32, i32, P(dbl), P(dbl), P(dbl)],
        "emat_tree_coalescent_stats": [B, dbl, dbl, P(i32), P(i32), P(dbl), i32, P(dbl), i32, P(i32)],
        "emat_tree_skygrid_moves": [B, P(_PopModelC), P(_SkygridSpecC), dbl, dbl, u64, P(_SkygridResultC)],
        "emat_exp_pop_moves": [B, P(_PopModelC), P(_ExpPopSpecC), dbl, dbl, i32, i32, P(dbl), i32, P(dbl), u64, P(_ExpPopResultC)],
        "emat_tree_exp_pop_moves": [B, P(_PopModelC), P(_ExpPopSpecC), dbl, dbl, u64, P(_ExpPopResultC)],
        "emat_subst_moves": [B, P(_SubstSpecC), i32, P(dbl), P(i64), P(i64), u64, P(_SubstResultC)], "emat_parts_subst_stats": [B, P(dbl), P(i64), P(i64)],
        "emat_parts_subst_moves": [B, P(_SubstSpecC), u64, P(_SubstResultC)], "emat_get_evo": [B, P(i32), P(dbl), P(dbl), P(dbl)],
        "emat_mpox_moves": [B, P(_MpoxSpecC), P(dbl), P(i64), u64, P(_MpoxResultC)], "emat_parts_mpox_moves": [B, P(_MpoxSpecC), u64, P(_MpoxResultC)],
        "emat_run_set_mpox": [R, i32, P(_MpoxSpecC)], "emat_run_mpox_moves": [R, P(_MpoxResultC)], "emat_run_get_mpox": [R, P(dbl), P(dbl)], "emat_run_get_mpox_partition": [R, P(i32), P(i32)],
        "emat_run_set_subst_moves": [R, i32, P(_SubstSpecC)], "emat_run_subst_moves": [R, P(_SubstResultC)], "emat_run_get_hky": [R, P(dbl), P(dbl), P(dbl)],
        "emat_run_set_exp_pop_moves": [R, i32, P(_ExpPopSpecC)], "emat_run_exp_pop_moves": [R, P(_ExpPopResultC)], "emat_run_get_exp_pop": [R, P(dbl), P(dbl)],
        "emat_run_set_skygrid_moves": [R, i32, P(_SkygridSpecC)], "emat_run_skygrid_moves": [R, P(_SkygridResultC)], "emat_run_get_skygrid": [R, P(dbl), P(dbl)],
        "emat_run_set_site_rate_moves": [R, i32, dbl], "emat_run_site_rate_moves": [R, P(_SiteRateResultC)], "emat_run_get_site_rates": [R, P(dbl), P(dbl)],
        "emat_align_begin": [B, i64], "emat_align_row_buffer": [B, i32, i64, P(P(C.c_uint8))], "emat_align_push_rows": [B, i32, P(C.c_uint8), i64],
        "emat_align_finish": [B, P(C.c_uint8), P(C.c_uint8), P(_AlignReportC)], "emat_align_sizes": [B, P(_AlignReportC)], "emat_align_get": [B, P(_AlignArraysC)],
        "emat_align_attach": [B, C.c_void_p, C.c_void_p], "emat_align_refuse": [B, C.c_int, C.c_char_p],
        "emat_seq_id_date_range": [C.c_char_p, P(dbl), P(dbl), P(i32)], "emat_fasta_frame_memory": [B, P(C.c_uint8), i64, P(_FastaReportC)],
        "emat_fasta_load_memory": [B, P(C.c_uint8), i64, P(C.c_uint8), i32, P(_FastaReportC)], "emat_fasta_load": [B, C.c_char_p, P(C.c_uint8), i32, P(_FastaReportC)],
        "emat_fasta_sizes": [B, P(_FastaReportC)], "emat_fasta_get": [B, C.c_char_p, P(i64), P(C.c_float), P(C.c_float), P(C.c_uint8)],
    }
    M = C.c_void_p
    sigs.update({
        "emat_run_create_multi": [P(i32), i32, P(_ConfigC), P(_FlatTreeC), P(C.c_uint8), i32, u64, i32, P(M)], "emat_multi_destroy": [M],
        "emat_multi_set_num_parts": [M, i32], "emat_multi_set_max_part_nodes": [M, i32], "emat_multi_set_option": [M, C.c_char_p, C.c_char_p], "emat_multi_set_rccl_library": [C.c_char_p], "emat_multi_debug_rccl_load": [C.c_char_p, i32], "emat_multi_set_hky": [M, dbl, dbl, P(dbl), P(dbl)], "emat_multi_set_pop_model": [M, P(_PopModelC)],
        "emat_multi_set_coalescent_t_step": [M, dbl], "emat_multi_set_flags": [M, i32, i32], "emat_multi_set_paranoid": [M, i32],
        "emat_multi_repartition": [M], "emat_multi_run_moves": [M, i64], "emat_multi_check_derived": [M, dbl], "emat_multi_reassemble": [M],
        "emat_multi_get_totals": [M, P(dbl), P(dbl)], "emat_multi_do_mcmc_steps": [M, i64, i64],
        "emat_multi_tree_sizes": [M, P(i32), P(i32), P(i32), P(i32)], "emat_multi_tree_get": [M, i32, P(_FlatTreeC), P(C.c_uint8)],
    })
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.emat_last_error.argtypes = [B]
    lib.emat_last_error.restype = C.c_char_p
    if os.environ.get("EMAT_HOST_THREADS"):     # (the library reads no tuning from the environment: this mirror forwards it)
        lib.emat_set_host_threads(int(os.environ["EMAT_HOST_THREADS"]))
    lib.emat_build_id.argtypes = []
    lib.emat_build_id.restype = C.c_char_p
    lib.emat_run_last_error.argtypes = [R]
    lib.emat_run_last_error.restype = C.c_char_p
    lib.emat_multi_last_error.argtypes = [M]; lib.emat_multi_last_error.restype = C.c_char_p
    lib.emat_multi_exchange.argtypes = [M]; lib.emat_multi_exchange.restype = C.c_char_p
    lib.emat_multi_num_shards.argtypes = [M]; lib.emat_multi_num_shards.restype = C.c_int32
    lib.emat_multi_backend.argtypes = [M, i32]; lib.emat_multi_backend.restype = C.c_void_p
    lib.emat_multi_shard.argtypes = [M, i32]; lib.emat_multi_shard.restype = C.c_void_p
    lib.emat_align_attached.argtypes = [B]; lib.emat_align_attached.restype = C.c_void_p
    lib.emat_align_num_sites.argtypes = [B]; lib.emat_align_num_sites.restype = C.c_int32
    lib.emat_synth_destroy.argtypes = [S]
    lib.emat_synth_destroy.restype = None
    _lib = lib
    return lib


def seq_id_date_range(seq_id: str):
    """(t_min, t_max) in days since 2020-01-01 from the date at the end of a sequence id, or None (include/emat_host.h: emat_seq_id_date_range)."""
    lo, hi, ok = C.c_double(), C.c_double(), C.c_int32()
    st = load_library().emat_seq_id_date_range(seq_id.encode(), C.byref(lo), C.byref(hi), C.byref(ok))
    if st != 0:
        raise EmatError("emat_seq_id_date_range: %s" % STATUS_NAMES.get(st, st))
    return (lo.value, hi.value) if ok.value else None


def hky_q_matrix(kappa: float, pi: Sequence[float]) -> np.ndarray:
    """Normalised HKY rate matrix, q_ab = r_ab pi_b / (pi^T r pi) (reference core/evo_hky.cpp:7-50)."""
    pi = np.asarray(pi, np.float64)
    r = np.array([[0, 1, kappa, 1], [1, 0, 1, kappa], [kappa, 1, 0, 1], [1, kappa, 1, 0]], np.float64)
    rowv = np.array([sum(pi[a] * r[a][b] for a in range(4)) for b in range(4)])
    R = 0.0
    for b in range(4):
        R += rowv[b] * pi[b]
    q = np.zeros((4, 4))
    for a in range(4):
        for b in range(4):
            if a != b:
                q[a, b] = r[a, b] / R * pi[b]
                q[a, a] -= q[a, b]
    return q


def make_synthetic_emat(p: SynthParams):
    """Seeded synthetic EMAT.  Returns (FlatTree, ref_sequence uint8[L], t_max_tip)."""
    lib = load_library()
    sp = _SynthParamsC()
    for f in ("num_tips", "num_sites", "tip_span", "tip_date_uncertainty", "frac_uncertain_tips", "pop_n0", "pop_growth", "mu", "kappa",
              "gaps_per_tip", "mean_gap_len", "seed"):
        setattr(sp, f, getattr(p, f))
    for a in range(4):
        sp.pi[a] = float(p.pi[a])
    h = C.c_void_p()
    st = lib.emat_synth_create(C.byref(sp), C.byref(h))
    if st != 0:
        raise EmatError("emat_synth_create failed: %s" % STATUS_NAMES.get(st, st))
    try:
        v = _FlatTreeC()
        ref = C.POINTER(C.c_uint8)()
        tmax = C.c_double()
        lib.emat_synth_get(h, C.byref(v), C.byref(ref), C.byref(tmax))
        tree = FlatTree.from_c_view(v)
        refseq = np.ctypeslib.as_array(ref, shape=(p.num_sites,)).copy()
        return tree, refseq, float(tmax.value)
    finally:
        lib.emat_synth_destroy(h)


def decode_graft_output(v, mode: int) -> dict:
    """The doubles of emat_debug_graft (include/emat_backend.h) as {"status", "grafts": [graft...], "count_min_mutations",
    "count_closed_mutations", "closed_deltas"}; a graft is {"delta_log_G", "log_alpha_mut", "X", "S", "t_P", "branch_infos": [...]}
    with mutations as [from, site, to, t] and deltas as [site, from, to]."""
    pos = [0]
    def take():
        x = float(v[pos[0]]); pos[0] += 1; return x
    def graft():
        nbi = int(take()); g = {"delta_log_G": take(), "log_alpha_mut": take(), "X": int(take()), "S": int(take()), "t_P": take(), "branch_infos": []}
        for _ in range(nbi):
            b = {"A": int(take()), "B": int(take()), "is_open": take() != 0.0, "T_to_X": take(), "partial_lambda_at_A": take(), "partial_lambda_at_X": take()}
            b["warm_sites"] = [[int(take()), int(take())] for _ in range(int(take()))]
            b["hot_sites"] = [[int(take()), int(take())] for _ in range(int(take()))]
            muts = []
            for _ in range(int(take())):
                site, fr, to, t = int(take()), int(take()), int(take()), take()
                muts.append([fr, site, to, t])
            b["hot_muts_to_X"] = muts
            b["hot_deltas_to_X"] = [[int(take()), int(take()), int(take())] for _ in range(int(take()))]
            g["branch_infos"].append(b)
        return g
    out = {"status": int(take())}
    num = int(take())
    out["grafts"] = [graft()]
    if mode >= 1:
        out["count_min_mutations"] = int(take()); out["count_closed_mutations"] = int(take())
        out["closed_deltas"] = [[int(take()), int(take()), int(take())] for _ in range(int(take()))]
    if num == 2:
        out["grafts"].append(graft())
    assert pos[0] == len(v), "emat_debug_graft output not consumed exactly: %d of %d" % (pos[0], len(v))
    return out


# The library itself reads no tuning from the environment (emat_set_option per handle).  For A/B scripts and tests this mirror forwards
# EMAT_<NAME> variables of the process to every handle it creates -- the behaviour the library had built in until round 4.
OPTION_KEYS = ("slack", "heap_per_node", "lds_scratch", "lds_classes", "lds_max", "giants", "side_arena", "tree_host_coalescent", "ticket_taper", "chunks", "ticket_xcd_spread",
               "ticket_release", "ticket_weights", "single_ticket_parts", "parts_per_cu", "order_by_time", "build_blocks", "tree_tight", "fn_min_lists", "phase_extra", "no_uniform_sites")


def _forward_env_options(setter):
    for k in OPTION_KEYS:
        v = os.environ.get("EMAT_" + k.upper())
        if v is not None:
            setter(k, v)


class EmatBackend:
    """The engine behind include/emat_backend.h: one resident `Subrun` per partition part, on the GPU."""

    def __init__(self, num_sites: int, device: int = 0, trace_moves: int = 0, use_lds: bool = True, slab_slack: float = 0.0, max_parts: int = 0):
        self._lib = load_library()
        cfg = _ConfigC(device, num_sites, max_parts, slab_slack, trace_moves, 1 if use_lds else 0)
        self._h = C.c_void_p()
        st = self._lib.emat_backend_create(C.byref(cfg), C.byref(self._h))
        if st != 0:
            raise EmatError("emat_backend_create failed: %s (the engine needs a HIP device; there is no CPU fallback)" % STATUS_NAMES.get(st, st))
        self.num_sites = num_sites
        self._keep = []
        _forward_env_options(lambda k, v: self.set_option(k, v))

    def set_option(self, key: str, value):
        """A tuning / test option of this handle (include/emat_backend.h, emat_set_option), before the first launch."""
        self._ck(self._lib.emat_set_option(self._h, key.encode(), str(value).encode()), "emat_set_option(%s)" % key)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.emat_backend_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _ck(self, st: int, what: str):
        if st != 0:
            msg = self._lib.emat_last_error(self._h)
            raise EmatError("%s: %s (%s)" % (what, STATUS_NAMES.get(st, st), msg.decode() if msg else ""))

    def set_ref_sequence(self, ref: np.ndarray):
        ref = np.ascontiguousarray(ref, np.uint8)
        self._ck(self._lib.emat_set_ref_sequence(self._h, _ptr(ref, C.c_uint8), ref.shape[0]), "emat_set_ref_sequence")

    def set_evo(self, mu, pi, q, nu_l, partition_for_site):
        mu = np.ascontiguousarray(mu, np.float64).reshape(-1)
        P = mu.shape[0]
        pi = np.ascontiguousarray(pi, np.float64).reshape(P * 4)
        q = np.ascontiguousarray(q, np.float64).reshape(P * 16)
        nu_l = np.ascontiguousarray(nu_l, np.float64)
        pfs = np.ascontiguousarray(partition_for_site, np.int32)
        self._ck(self._lib.emat_set_evo(self._h, P, _ptr(mu, C.c_double), _ptr(pi, C.c_double), _ptr(q, C.c_double), _ptr(nu_l, C.c_double), _ptr(pfs, C.c_int32)), "emat_set_evo")

    def set_hky(self, mu: float, kappa: float, pi, nu_l=None):
        nu = np.ones(self.num_sites) if nu_l is None else nu_l
        self.set_evo([mu], [pi], [hky_q_matrix(kappa, pi)], nu, np.zeros(self.num_sites, np.int32))

    def set_flags(self, t_max_tip: float, only_displacing_inner_nodes: bool = False, topology_moves_enabled: bool = True):
        self._ck(self._lib.emat_set_flags(self._h, t_max_tip, int(only_displacing_inner_nodes), int(topology_moves_enabled)), "emat_set_flags")

    def upload_parts(self, parts: Sequence[FlatTree], includes_run_root: Sequence[bool], seeds: Sequence[int]):
        self._ck(self._lib.emat_begin_upload(self._h, len(parts)), "emat_begin_upload")
        for i, (t, r, s) in enumerate(zip(parts, includes_run_root, seeds)):
            v = t.c_view()
            self._ck(self._lib.emat_part_upload(self._h, i, C.byref(v), int(r), int(s)), "emat_part_upload")
        self._ck(self._lib.emat_end_upload(self._h), "emat_end_upload")

    def build_coalescent_parts(self, pop: PopModel, root_part_index: int, t_step: float):
        m = pop.c_struct()
        self._ck(self._lib.emat_build_coalescent_parts(self._h, C.byref(m), root_part_index, t_step), "emat_build_coalescent_parts")

    # staged form for parts sharded over several processes / GPUs
    def coalescent_begin(self, pop: PopModel, root_part_index: int, t_step: float):
        m = pop.c_struct()
        lo, hi = C.c_double(), C.c_double()
        self._ck(self._lib.emat_coalescent_begin(self._h, C.byref(m), root_part_index, t_step, C.byref(lo), C.byref(hi)), "emat_coalescent_begin")
        return float(lo.value), float(hi.value)

    def coalescent_set_range(self, all_t_min: float, all_t_max: float) -> int:
        n = C.c_int32()
        self._ck(self._lib.emat_coalescent_set_range(self._h, all_t_min, all_t_max, C.byref(n)), "emat_coalescent_set_range")
        self._coal_cells = n.value
        return n.value

    def coalescent_local_grid(self):
        kb = np.zeros(self._coal_cells)
        na = np.zeros(self._coal_cells, np.int32)
        self._ck(self._lib.emat_coalescent_local_grid(self._h, _ptr(kb, C.c_double), _ptr(na, C.c_int32)), "emat_coalescent_local_grid")
        return kb, na

    def coalescent_sample(self, k_bar: np.ndarray, num_active: np.ndarray) -> np.ndarray:
        k_bar = np.ascontiguousarray(k_bar, np.float64)
        num_active = np.ascontiguousarray(num_active, np.int32)
        kt = np.zeros(self._coal_cells)
        self._ck(self._lib.emat_coalescent_sample(self._h, _ptr(k_bar, C.c_double), _ptr(num_active, C.c_int32), _ptr(kt, C.c_double)), "emat_coalescent_sample")
        return kt

    def coalescent_finish(self, k_twiddle_bar: np.ndarray):
        k = np.ascontiguousarray(k_twiddle_bar, np.float64)
        self._ck(self._lib.emat_coalescent_finish(self._h, _ptr(k, C.c_double)), "emat_coalescent_finish")

    def run_local_moves(self, count: int):
        self._ck(self._lib.emat_run_local_moves(self._h, count), "emat_run_local_moves")

    def run_moves_split(self, moves_per_part: int, extra_moves_part0: int):
        self._ck(self._lib.emat_run_moves_split(self._h, moves_per_part, extra_moves_part0), "emat_run_moves_split")

    def run_moves_per_part(self, moves: int):
        self._ck(self._lib.emat_run_moves_per_part(self._h, moves), "emat_run_moves_per_part")

    def synchronize(self):
        self._ck(self._lib.emat_synchronize(self._h), "emat_synchronize")

    # ---- the whole tree resident in HBM (include/emat_backend.h: emat_tree_*) ----
    def tree_upload(self, tree: FlatTree):
        v = tree.c_view()
        self._ck(self._lib.emat_tree_upload(self._h, C.byref(v)), "emat_tree_upload")

    def tree_topology(self):
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_tree_get_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_tree_get_sizes")
        parent, c0, c1 = (np.zeros(n.value, np.int32) for _ in range(3))
        t = np.zeros(n.value); root = C.c_int32()
        self._ck(self._lib.emat_tree_get_topology(self._h, _ptr(parent, C.c_int32), _ptr(c0, C.c_int32), _ptr(c1, C.c_int32), _ptr(t, C.c_double), C.byref(root)), "emat_tree_get_topology")
        return parent, c0, c1, t, int(root.value)

    def tree_kids(self):
        """(child0, child1) of every node, the root and the root's time, from the backend's own mirror (emat_tree_get_kids): current as
        soon as emat_tree_reassemble has returned, while the lists of the tree may still be on their way.  A copy: the mirror itself
        is only valid until the next reassemble."""
        kp = C.POINTER(C.c_int32)(); n = C.c_int32(); root = C.c_int32(); t_root = C.c_double()
        self._ck(self._lib.emat_tree_get_kids(self._h, C.byref(kp), C.byref(n), C.byref(root), C.byref(t_root)), "emat_tree_get_kids")
        kids = np.ctypeslib.as_array(kp, shape=(n.value, 2)).copy()
        return kids, int(root.value), float(t_root.value)

    def tree_repartition(self, part_offset, orig, kid0, kid1, root_part: int, seeds, pop: PopModel, t_step: float):
        po, og, k0, k1 = (np.ascontiguousarray(a, np.int32) for a in (part_offset, orig, kid0, kid1))
        sd = np.ascontiguousarray(seeds, np.uint64)
        m = pop.c_struct()
        self._ck(self._lib.emat_tree_repartition(self._h, int(po.shape[0]) - 1, _ptr(po, C.c_int32), _ptr(og, C.c_int32), _ptr(k0, C.c_int32), _ptr(k1, C.c_int32),
                                                 root_part, _ptr(sd, C.c_uint64), C.byref(m), t_step), "emat_tree_repartition")

    def tree_reassemble(self, capacity: Optional[int] = None):
        capacity = self.num_sites if capacity is None else capacity   # at most one change of the root sequence per site
        n = C.c_int32()
        site = np.zeros(capacity, np.int32); frm = np.zeros(capacity, np.uint8); to = np.zeros(capacity, np.uint8)
        self._ck(self._lib.emat_tree_reassemble(self._h, C.byref(n), _ptr(site, C.c_int32), _ptr(frm, C.c_uint8), _ptr(to, C.c_uint8), capacity), "emat_tree_reassemble")
        k = n.value
        return site[:k].copy(), frm[:k].copy(), to[:k].copy()

    def tree_partition(self, cut_nodes):
        """partition_tree on the device: (num_parts, root_part, part_offset, orig, kid0, kid1) for the given cut nodes."""
        cuts = np.ascontiguousarray(cut_nodes, np.int32)
        n, r = C.c_int32(), C.c_int32()
        sizes = np.zeros(cuts.shape[0] + 1, np.int32)
        self._ck(self._lib.emat_tree_partition(self._h, int(cuts.shape[0]), _ptr(cuts, C.c_int32), C.byref(n), C.byref(r), _ptr(sizes, C.c_int32)), "emat_tree_partition")
        off = np.zeros(n.value + 1, np.int32)
        self._ck(self._lib.emat_tree_get_partition(self._h, _ptr(off, C.c_int32), None, None, None), "emat_tree_get_partition")
        orig, k0, k1 = (np.zeros(int(off[-1]), np.int32) for _ in range(3))
        self._ck(self._lib.emat_tree_get_partition(self._h, None, _ptr(orig, C.c_int32), _ptr(k0, C.c_int32), _ptr(k1, C.c_int32)), "emat_tree_get_partition")
        assert np.array_equal(np.diff(off), sizes[:n.value])
        return n.value, r.value, off, orig, k0, k1

    def tree_root_deltas(self, capacity: Optional[int] = None):
        """(site, from, to) on the process that holds the root part, None elsewhere."""
        capacity = self.num_sites if capacity is None else capacity
        n = C.c_int32()
        site = np.zeros(capacity, np.int32); frm = np.zeros(capacity, np.uint8); to = np.zeros(capacity, np.uint8)
        self._ck(self._lib.emat_tree_get_root_deltas(self._h, C.byref(n), _ptr(site, C.c_int32), _ptr(frm, C.c_uint8), _ptr(to, C.c_uint8), capacity), "emat_tree_get_root_deltas")
        return None if n.value < 0 else (site[:n.value].copy(), frm[:n.value].copy(), to[:n.value].copy())

    def tree_gather_local(self, site, frm, to):
        site = np.ascontiguousarray(site, np.int32); frm = np.ascontiguousarray(frm, np.uint8); to = np.ascontiguousarray(to, np.uint8)
        self._ck(self._lib.emat_tree_gather_local(self._h, int(site.shape[0]), _ptr(site, C.c_int32), _ptr(frm, C.c_uint8), _ptr(to, C.c_uint8)), "emat_tree_gather_local")

    def tree_export_nodes(self) -> np.ndarray:
        need = C.c_uint64()
        self._ck(self._lib.emat_tree_export_nodes(self._h, None, 0, C.byref(need)), "emat_tree_export_nodes")
        buf = np.zeros(int(need.value), np.uint8)
        self._ck(self._lib.emat_tree_export_nodes(self._h, _ptr(buf, C.c_uint8), buf.shape[0], C.byref(need)), "emat_tree_export_nodes")
        return buf

    def tree_apply_nodes(self, buf: np.ndarray):
        buf = np.ascontiguousarray(buf, np.uint8)
        self._ck(self._lib.emat_tree_apply_nodes(self._h, _ptr(buf, C.c_uint8), buf.shape[0]), "emat_tree_apply_nodes")

    # the same exchange on raw addresses -- device memory (e.g. a torch tensor's data_ptr()) or host memory
    def tree_export_size(self) -> int:
        need = C.c_uint64()
        self._ck(self._lib.emat_tree_export_nodes(self._h, None, 0, C.byref(need)), "emat_tree_export_nodes")
        return int(need.value)

    def tree_export_nodes_into(self, address: int, capacity: int) -> int:
        need = C.c_uint64()
        self._ck(self._lib.emat_tree_export_nodes(self._h, C.cast(C.c_void_p(address), C.POINTER(C.c_uint8)), capacity, C.byref(need)), "emat_tree_export_nodes")
        return int(need.value)

    def tree_apply_nodes_at(self, address: int, nbytes: int):
        self._ck(self._lib.emat_tree_apply_nodes(self._h, C.cast(C.c_void_p(address), C.POINTER(C.c_uint8)), nbytes), "emat_tree_apply_nodes")

    def tree_reassemble_end(self):
        self._ck(self._lib.emat_tree_reassemble_end(self._h), "emat_tree_reassemble_end")

    def tree_download(self):
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_tree_get_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_tree_get_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        ref = np.zeros(self.num_sites, np.uint8)
        self._ck(self._lib.emat_tree_download(self._h, C.byref(v), _ptr(ref, C.c_uint8)), "emat_tree_download")
        t.root = v.root
        return t.trimmed(), ref

    # ---- the tree probers on the resident tree (include/emat_backend.h: emat_tree_probe_*, emat_tree_branch_counts) ----
    def tree_probe_ancestors(self, pop: PopModel, marked_nodes, t_start: float, t_end: float, num_t_cells: int) -> np.ndarray:
        """probe_ancestors_on_tree: p [len(marked_nodes) + 1][num_t_cells]; the last member is "none of them", -1 marks nothing."""
        mk = np.ascontiguousarray(marked_nodes, np.int32).reshape(-1)
        out = np.zeros((mk.shape[0] + 1, max(num_t_cells, 1)))      # (a bad cell count is the library's to refuse)
        m = pop.c_struct()
        self._ck(self._lib.emat_tree_probe_ancestors(self._h, C.byref(m), int(mk.shape[0]), _ptr(mk, C.c_int32) if mk.shape[0] else None, t_start, t_end, num_t_cells,
                                                     _ptr(out, C.c_double)), "emat_tree_probe_ancestors")
        return out

    def tree_probe_site_states(self, pop: PopModel, site: int, t_start: float, t_end: float, num_t_cells: int) -> np.ndarray:
        """probe_site_states_on_tree: p [4][num_t_cells], states A, C, G, T."""
        out = np.zeros((4, max(num_t_cells, 1)))
        m = pop.c_struct()
        self._ck(self._lib.emat_tree_probe_site_states(self._h, C.byref(m), site, t_start, t_end, num_t_cells, _ptr(out, C.c_double)), "emat_tree_probe_site_states")
        return out

    def tree_branch_counts(self, t_start: float, t_end: float, num_t_cells: int, marked_nodes=None, site: Optional[int] = None):
        """The branch counts a prober hands to Tree_prober -- of the ancestral prober when `marked_nodes` is given, else of the site-state
        prober for `site`: (counts [members][cells], cells_to_skip, x_start), the cells prepended to reach the root included."""
        if (marked_nodes is None) == (site is None):
            raise ValueError("give marked_nodes or site")
        kind = 0 if site is None else 1
        mk = np.ascontiguousarray([] if marked_nodes is None else marked_nodes, np.int32).reshape(-1)
        args = (kind, int(mk.shape[0]), _ptr(mk, C.c_int32) if mk.shape[0] else None, 0 if site is None else site, t_start, t_end, num_t_cells)
        n, skip, x0 = C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self._lib.emat_tree_branch_counts(self._h, *args, C.byref(n), C.byref(skip), C.byref(x0), None, 0), "emat_tree_branch_counts")
        out = np.zeros((mk.shape[0] + 1 if kind == 0 else 4, n.value))
        self._ck(self._lib.emat_tree_branch_counts(self._h, *args, C.byref(n), C.byref(skip), C.byref(x0), _ptr(out, C.c_double), out.size), "emat_tree_branch_counts")
        return out, int(skip.value), float(x0.value)

    # ---- sampled trees kept in HBM and the MCC tree derived from them (include/emat_backend.h: emat_tree_sample_*, emat_mcc_*) ----
    def tree_samples_reserve(self, capacity: int) -> None:
        """Room for `capacity` samples of the resident tree's node count."""
        self._ck(self._lib.emat_tree_samples_reserve(self._h, capacity), "emat_tree_samples_reserve")

    def tree_sample_push(self) -> int:
        """Snapshot of the resident tree's topology and node times into the next slot, device to device; returns the slot."""
        i = C.c_int32(-1)
        self._ck(self._lib.emat_tree_sample_push(self._h, C.byref(i)), "emat_tree_sample_push")
        return int(i.value)

    def tree_sample_push_flat(self, parent, child0, child1, t, root: int) -> int:
        """The same from host arrays (checked: node count, binary, one root, consistent links, the tips of sample 0)."""
        pa = np.ascontiguousarray(parent, np.int32); a0 = np.ascontiguousarray(child0, np.int32); a1 = np.ascontiguousarray(child1, np.int32); tt = np.ascontiguousarray(t, np.float64)
        if not (pa.shape == a0.shape == a1.shape == tt.shape and pa.ndim == 1):
            raise ValueError("parent, child0, child1 and t must be one-dimensional and of one length")
        i = C.c_int32(-1)
        self._ck(self._lib.emat_tree_sample_push_flat(self._h, int(pa.shape[0]), _ptr(pa, C.c_int32), _ptr(a0, C.c_int32), _ptr(a1, C.c_int32), _ptr(tt, C.c_double), int(root), C.byref(i)), "emat_tree_sample_push_flat")
        return int(i.value)

    def tree_samples_count(self) -> int:
        return self.tree_samples_info()[0]

    def tree_samples_info(self):
        """(samples held, capacity in samples, nodes per sample)."""
        c, cap, n = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_tree_samples_count(self._h, C.byref(c), C.byref(cap), C.byref(n)), "emat_tree_samples_count")
        return int(c.value), int(cap.value), int(n.value)

    def tree_samples_clear(self) -> None:
        self._ck(self._lib.emat_tree_samples_clear(self._h), "emat_tree_samples_clear")

    def tree_sample_get(self, index: int):
        """(parent, child0, child1, t, root) of one slot."""
        n = self.tree_samples_info()[2]
        parent = np.zeros(n, np.int32); c0 = np.zeros(n, np.int32); c1 = np.zeros(n, np.int32); t = np.zeros(n); root = C.c_int32(-1)
        self._ck(self._lib.emat_tree_sample_get(self._h, index, _ptr(parent, C.c_int32), _ptr(c0, C.c_int32), _ptr(c1, C.c_int32), _ptr(t, C.c_double), C.byref(root)), "emat_tree_sample_get")
        return parent, c0, c1, t, int(root.value)

    def mcc_derive(self, first: int = 0, count: Optional[int] = None, stride: int = 1, seed: int = 0) -> "MccTree":
        """derive_mcc_tree over the samples first, first + stride, ... (`count` of them; default: as many as the store has from `first`)."""
        held, _, n = self.tree_samples_info()
        if count is None:
            count = max(0, (held - first + stride - 1) // stride) if stride >= 1 and first >= 0 else 0
        m = max(count, 1)
        r = MccTree(0, 0, np.zeros(m), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), -1, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int32), 0, 0, 0)
        c = _MccResultC(0, 0, _ptr(r.log_cc, C.c_double), _ptr(r.parent, C.c_int32), _ptr(r.child0, C.c_int32), _ptr(r.child1, C.c_int32), -1,
                        _ptr(r.support, C.c_double), _ptr(r.t, C.c_double), _ptr(r.t_mrca, C.c_double), _ptr(r.num_exact, C.c_int32), 0, 0, 0)
        self._ck(self._lib.emat_mcc_derive(self._h, first, count, stride, seed & (2 ** 64 - 1), C.byref(c)), "emat_mcc_derive")
        r.master, r.master_index, r.root = int(c.master_position), int(c.master_index), int(c.root)
        r.num_distinct_clades, r.table_regrows, r.table_slots = int(c.num_distinct_clades), int(c.table_regrows), int(c.table_slots)
        return r

    def mcc_correspondence(self, k: int):
        """(node_in_sample [n], is_exact [n] bool) of the k-th chosen sample of the last mcc_derive."""
        n = self.tree_samples_info()[2]
        node = np.zeros(n, np.int32); ex = np.zeros(n, np.uint8)
        self._ck(self._lib.emat_mcc_get_correspondence(self._h, k, _ptr(node, C.c_int32), _ptr(ex, C.c_uint8)), "emat_mcc_get_correspondence")
        return node, ex.astype(bool)

    def _samples_probe(self, call, what, pops, count, num_marked, num_t_cells, ranks, per_sample, mean, num_sites=None):
        """The outputs of a batched probe and the call itself: `call(pop_array, num_pops, result)` makes it.  With `num_sites`
        (the site-state forms) the member axis is two: [num_sites][4]."""
        pops = [pops] if isinstance(pops, PopModel) else list(pops)
        pop_c = (_PopModelC * max(len(pops), 1))(*[m.c_struct() for m in pops])
        m, cells = max(count, 1), max(num_t_cells, 1)
        members = (max(num_marked, 0) + 1,) if num_sites is None else (max(num_sites, 1), 4)
        rk = np.ascontiguousarray([] if ranks is None else ranks, np.int32)
        r = SamplesProbe(np.zeros((m,) + members + (cells,)) if per_sample else None, np.zeros(members + (cells,)) if mean else None,
                         np.zeros((rk.shape[0],) + members + (cells,)) if rk.shape[0] else None, np.zeros(m, np.int32))
        c = _SamplesProbeResultC(_ptr(r.p, C.c_double) if per_sample else None, _ptr(r.mean, C.c_double) if mean else None, int(rk.shape[0]),
                                 _ptr(rk, C.c_int32) if rk.shape[0] else None, _ptr(r.order_stats, C.c_double) if rk.shape[0] else None, _ptr(r.cells_to_skip, C.c_int32))
        self._ck(call(pop_c, len(pops), C.byref(c)), what)
        return r

    def tree_samples_probe_ancestors(self, pops, marked, t_start: float, t_end: float, num_t_cells: int, first: int = 0, count: Optional[int] = None, stride: int = 1,
                                     ranks=None, per_sample: bool = True, mean: bool = True) -> "SamplesProbe":
        """probe_ancestors_on_tree on the samples first, first + stride, ... of the store in one call.  `pops`: one PopModel or a list of `count`;
        `marked`: a list of nodes for all samples, or [count][num_marked] with one list per sample.  p[k] is what tree_probe_ancestors gives for
        sample k's tree, bit for bit; `mean` and the order statistics `ranks` (each in [0, count)) are made on the device."""
        held = self.tree_samples_info()[0]
        if count is None:
            count = max(0, (held - first + stride - 1) // stride) if stride >= 1 and first >= 0 else 0
        mk = np.ascontiguousarray(marked, np.int32)
        each = mk.ndim == 2
        num_marked = int(mk.shape[-1]) if mk.ndim else 0
        if each and mk.shape[0] != count:
            raise EmatError("tree_samples_probe_ancestors: %d lists of marked nodes for %d samples" % (mk.shape[0], count))
        return self._samples_probe(lambda pc, npc, res: self._lib.emat_tree_samples_probe_ancestors(self._h, pc, npc, first, count, stride, num_marked, _ptr(mk, C.c_int32) if mk.size else None,
                                                                                                     1 if each else 0, t_start, t_end, num_t_cells, res),
                                   "emat_tree_samples_probe_ancestors", pops, count, num_marked, num_t_cells, ranks, per_sample, mean)

    def mcc_probe_ancestors(self, pops, mcc_nodes, t_start: float, t_end: float, num_t_cells: int, ranks=None, per_sample: bool = True, mean: bool = True) -> "SamplesProbe":
        """The same on every base tree of the last mcc_derive, the marks of a base tree being the nodes that correspond to `mcc_nodes`."""
        mk = np.ascontiguousarray(mcc_nodes, np.int32).reshape(-1)
        count = C.c_int32(0)                         # (the outputs are sized by the derivation the library holds, not by what this mirror remembers)
        self._ck(self._lib.emat_mcc_get_derivation(self._h, None, C.byref(count), None), "emat_mcc_get_derivation")
        return self._samples_probe(lambda pc, npc, res: self._lib.emat_mcc_probe_ancestors(self._h, pc, npc, int(mk.shape[0]), _ptr(mk, C.c_int32) if mk.size else None, t_start, t_end, num_t_cells, res),
                                   "emat_mcc_probe_ancestors", pops, int(count.value), int(mk.shape[0]), num_t_cells, ranks, per_sample, mean)

    # ---- on the MCC tree: node-date spreads and the support of the master's mutations (include/emat_backend.h) ----
    def mcc_node_times(self, nodes=None, quantiles=(), hpd_mass: float = 0.0, per_sample: bool = False) -> "MccNodeTimes":
        """Over the samples of the last mcc_derive, for every MCC node of `nodes` (None: all, in node order): quantiles and the shortest interval
        holding `hpd_mass` of the node's dates, over the samples that have its clade (`exact`) and over all (`mrca`); with `per_sample` the dates themselves."""
        n = self.tree_samples_info()[2]
        count = C.c_int32(0)
        self._ck(self._lib.emat_mcc_get_derivation(self._h, None, C.byref(count), None), "emat_mcc_get_derivation")
        m = max(int(count.value), 1)
        nd = None if nodes is None else np.ascontiguousarray(nodes, np.int32).reshape(-1)
        cols = max(n, 1) if nd is None else max(int(nd.shape[0]), 1)
        q = np.ascontiguousarray(quantiles, np.float64).reshape(-1)
        nq, hpd = int(q.shape[0]), float(hpd_mass) != 0.0
        r = MccNodeTimes(np.arange(n, dtype=np.int32) if nd is None else nd, q, float(hpd_mass), np.zeros(cols, np.int32),
                         np.zeros((nq, cols)) if nq else None, np.zeros((nq, cols)) if nq else None, np.zeros((2, cols)) if hpd else None, np.zeros((2, cols)) if hpd else None,
                         np.zeros((cols, m)) if per_sample else None, np.zeros((cols, m), np.uint8) if per_sample else None)
        opt = lambda a, ct: None if a is None else _ptr(a, ct)
        c = _MccNodeTimesResultC(nq, _ptr(q, C.c_double) if nq else None, float(hpd_mass), opt(r.q_exact, C.c_double), opt(r.q_mrca, C.c_double), opt(r.hpd_exact, C.c_double), opt(r.hpd_mrca, C.c_double),
                                 _ptr(r.num_exact, C.c_int32), opt(r.times, C.c_double), opt(r.is_exact, C.c_uint8))
        self._ck(self._lib.emat_mcc_node_times(self._h, 0 if nd is None else int(nd.shape[0]), None if nd is None else (_ptr(nd, C.c_int32) if nd.size else _ptr(np.zeros(1, np.int32), C.c_int32)), C.byref(c)),
                 "emat_mcc_node_times")
        if per_sample:
            r.is_exact = r.is_exact.astype(bool)
        return r

    def mcc_mutation_support(self) -> "MccMutationSupport":
        """For every mutation of the last mcc_derive's master, in the order tree_sample_get_mutations(master slot) lists them: how many samples have
        the node's clade and the mutation on its branch, and the mean, earliest and latest of its times over those."""
        nm = C.c_int64(0)
        self._ck(self._lib.emat_mcc_mutation_support(self._h, 0, C.byref(nm), None, None, None, None), "emat_mcc_mutation_support")
        k = int(nm.value)
        r = MccMutationSupport(np.zeros(k, np.int32), np.zeros(k), np.zeros(k), np.zeros(k))
        if k:
            self._ck(self._lib.emat_mcc_mutation_support(self._h, k, C.byref(nm), _ptr(r.num_with, C.c_int32), _ptr(r.mean_t, C.c_double), _ptr(r.t_min, C.c_double), _ptr(r.t_max, C.c_double)),
                     "emat_mcc_mutation_support")
        return r

    # ---- samples that keep their mutations, and the site-state prober over them (include/emat_backend.h) ----
    def tree_samples_reserve_mutations(self, mutation_records: int) -> None:
        """On an empty store: room for every slot's list headers and reference sequence and an arena of `mutation_records` records
        shared by all slots (0 releases it).  From then on tree_sample_push keeps the resident tree's mutations too."""
        self._ck(self._lib.emat_tree_samples_reserve_mutations(self._h, int(mutation_records)), "emat_tree_samples_reserve_mutations")

    def tree_sample_push_flat_mutations(self, parent, child0, child1, t, root: int, mut_offset, mut_site, mut_from, mut_to, mut_t, ref_sequence) -> int:
        """tree_sample_push_flat for a tree that comes with its mutations (CSR lists per node) and its reference sequence."""
        pa = np.ascontiguousarray(parent, np.int32); a0 = np.ascontiguousarray(child0, np.int32); a1 = np.ascontiguousarray(child1, np.int32); tt = np.ascontiguousarray(t, np.float64)
        if not (pa.shape == a0.shape == a1.shape == tt.shape and pa.ndim == 1):
            raise ValueError("parent, child0, child1 and t must be one-dimensional and of one length")
        mo = np.ascontiguousarray(mut_offset, np.int32); ms = np.ascontiguousarray(mut_site, np.int32); mf = np.ascontiguousarray(mut_from, np.uint8)
        mt = np.ascontiguousarray(mut_to, np.uint8); mtt = np.ascontiguousarray(mut_t, np.float64); ref = np.ascontiguousarray(ref_sequence, np.uint8)
        if mo.shape != (pa.shape[0] + 1,) or not (ms.shape == mf.shape == mt.shape == mtt.shape and ms.ndim == 1) or ms.shape[0] < max(int(mo.max()), 0) or ref.shape != (self.num_sites,):
            raise ValueError("mut_offset must have num_nodes + 1 entries, the four mutation arrays its last entry, and ref_sequence num_sites")
        i = C.c_int32(-1)
        opt = lambda a, ct: _ptr(a, ct) if a.shape[0] else None
        self._ck(self._lib.emat_tree_sample_push_flat_mutations(self._h, int(pa.shape[0]), _ptr(pa, C.c_int32), _ptr(a0, C.c_int32), _ptr(a1, C.c_int32), _ptr(tt, C.c_double), int(root),
                                                                _ptr(mo, C.c_int32), opt(ms, C.c_int32), opt(mf, C.c_uint8), opt(mt, C.c_uint8), opt(mtt, C.c_double), _ptr(ref, C.c_uint8), C.byref(i)),
                 "emat_tree_sample_push_flat_mutations")
        return int(i.value)

    def tree_samples_mutation_info(self):
        """(records handed out, records of the arena -- 0 without mutation room --, the number of sites the room is bound to)."""
        used, cap, L = C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(self._lib.emat_tree_samples_mutation_info(self._h, C.byref(used), C.byref(cap), C.byref(L)), "emat_tree_samples_mutation_info")
        return int(used.value), int(cap.value), int(L.value)

    def tree_sample_get_mutations(self, index: int):
        """(mut_offset [n + 1], site, from, to, t, ref_sequence) of one slot: CSR in node order, every list in its stored order."""
        n = self.tree_samples_info()[2]
        L = self.tree_samples_mutation_info()[2]
        nm = C.c_int64(0)
        self._ck(self._lib.emat_tree_sample_get_mutations(self._h, index, None, None, None, None, None, 0, None, C.byref(nm)), "emat_tree_sample_get_mutations")
        k = int(nm.value)
        off = np.zeros(n + 1, np.int32); site = np.zeros(k, np.int32); frm = np.zeros(k, np.uint8); to = np.zeros(k, np.uint8); t = np.zeros(k); ref = np.zeros(max(L, 1), np.uint8)
        opt = lambda a, ct: _ptr(a, ct) if k else None
        self._ck(self._lib.emat_tree_sample_get_mutations(self._h, index, _ptr(off, C.c_int32), opt(site, C.c_int32), opt(frm, C.c_uint8), opt(to, C.c_uint8), opt(t, C.c_double), k,
                                                          _ptr(ref, C.c_uint8), C.byref(nm)), "emat_tree_sample_get_mutations")
        return off, site, frm, to, t, ref[:L]

    def tree_samples_probe_site_states(self, pops, sites, t_start: float, t_end: float, num_t_cells: int, first: int = 0, count: Optional[int] = None, stride: int = 1,
                                       ranks=None, per_sample: bool = True, mean: bool = True) -> "SamplesProbe":
        """probe_site_states_on_tree on the samples first, first + stride, ... of the store, for every site of `sites`, in one call.  p[k][i] is
        what tree_probe_site_states gives for sample k's tree and reference sequence and sites[i], bit for bit: p [count][sites][4][cells],
        mean [sites][4][cells], order_stats [ranks][sites][4][cells]."""
        held = self.tree_samples_info()[0]
        if count is None:
            count = max(0, (held - first + stride - 1) // stride) if stride >= 1 and first >= 0 else 0
        st = np.ascontiguousarray(sites, np.int32).reshape(-1)
        return self._samples_probe(lambda pc, npc, res: self._lib.emat_tree_samples_probe_site_states(self._h, pc, npc, first, count, stride, int(st.shape[0]), _ptr(st, C.c_int32) if st.size else None,
                                                                                                       t_start, t_end, num_t_cells, res),
                                   "emat_tree_samples_probe_site_states", pops, count, 0, num_t_cells, ranks, per_sample, mean, num_sites=int(st.shape[0]))

    def mcc_probe_site_states(self, pops, sites, t_start: float, t_end: float, num_t_cells: int, ranks=None, per_sample: bool = True, mean: bool = True) -> "SamplesProbe":
        """The same on every base tree of the last mcc_derive."""
        st = np.ascontiguousarray(sites, np.int32).reshape(-1)
        count = C.c_int32(0)
        self._ck(self._lib.emat_mcc_get_derivation(self._h, None, C.byref(count), None), "emat_mcc_get_derivation")
        return self._samples_probe(lambda pc, npc, res: self._lib.emat_mcc_probe_site_states(self._h, pc, npc, int(st.shape[0]), _ptr(st, C.c_int32) if st.size else None, t_start, t_end, num_t_cells, res),
                                   "emat_mcc_probe_site_states", pops, int(count.value), 0, num_t_cells, ranks, per_sample, mean, num_sites=int(st.shape[0]))

    def tree_counters(self):
        """(growths of the cut-state pools, growths of the list heaps, cut-point states that needed the large kernel) of the
        HBM-resident tree: testing aid."""
        out = np.zeros(3, np.int32)
        self._ck(self._lib.emat_debug_tree_counters(self._h, _ptr(out, C.c_int32)), "emat_debug_tree_counters")
        return int(out[0]), int(out[1]), int(out[2])

    def run_moves_even(self, moves_per_part: int, one_more_below: int):
        """`moves_per_part` moves on every part, one more on the parts [0, one_more_below) (not the reference's remainder rule)."""
        self._ck(self._lib.emat_run_moves_even(self._h, moves_per_part, one_more_below), "emat_run_moves_even")

    def recalc_derived(self):
        self._ck(self._lib.emat_recalc_derived(self._h), "emat_recalc_derived")

    def check_derived(self, tol_scale: float = 1.0):
        """The reference's check_derived_quantities on the device (raises EmatError when a part is off); returns (part, deviations)."""
        wp = C.c_int32(); w4 = (C.c_double * 4)()
        self._ck(self._lib.emat_check_derived(self._h, tol_scale, C.byref(wp), w4), "emat_check_derived")
        return wp.value, [float(x) for x in w4]

    def last_run_ms(self) -> float:
        ms = C.c_double()
        self._ck(self._lib.emat_last_run_ms(self._h, C.byref(ms)), "emat_last_run_ms")
        return float(ms.value)

    def last_kernel_ms(self):
        ms, n = C.c_double(), C.c_int32()
        self._ck(self._lib.emat_last_kernel_ms(self._h, C.byref(ms), C.byref(n)), "emat_last_kernel_ms")
        return float(ms.value), int(n.value)

    def totals(self):
        g, a = C.c_double(), C.c_double()
        self._ck(self._lib.emat_get_totals(self._h, C.byref(g), C.byref(a)), "emat_get_totals")
        return float(g.value), float(a.value)

    def global_stats(self, num_partitions: int = 1):
        """(Ttwiddle_beta_a [P][4], num_muts_beta_ab [P][4][4], num_muts) over the parts of this handle."""
        T = np.zeros((num_partitions, 4)); M = np.zeros((num_partitions, 4, 4), np.int64); nm = C.c_int64()
        self._ck(self._lib.emat_get_global_stats(self._h, num_partitions, T.ctypes.data_as(C.POINTER(C.c_double)), M.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nm)),
                 "emat_get_global_stats")
        return T, M, int(nm.value)

    def num_muts_l(self) -> np.ndarray:
        """calc_num_muts_l over the parts of this handle (mutations per site)."""
        out = np.zeros(self.num_sites, np.int32)
        self._ck(self._lib.emat_get_num_muts_l(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "emat_get_num_muts_l")
        return out

    def scalable_coalescent_log_prior(self, t_ref: float, t_step: float) -> float:
        """Scalable_coalescent_prior::calc_log_prior of the whole tree, from the parts of this handle."""
        v = C.c_double()
        self._ck(self._lib.emat_get_scalable_coalescent_log_prior(self._h, t_ref, t_step, C.byref(v)), "emat_get_scalable_coalescent_log_prior")
        return float(v.value)

    def part_tree_lengths(self, num_parts: int) -> np.ndarray:
        out = np.zeros(num_parts)
        self._ck(self._lib.emat_get_part_tree_lengths(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "emat_get_part_tree_lengths")
        return out

    def Ttwiddle_l_partial(self, ext_offset, ext_node, ext_length):
        """(S, R, total tree length if this handle holds the run's root else 0) over the parts of this handle."""
        off = np.ascontiguousarray(ext_offset, np.int32); node = np.ascontiguousarray(ext_node, np.int32); val = np.ascontiguousarray(ext_length, np.float64)
        if node.shape[0] == 0:
            node = np.zeros(1, np.int32); val = np.zeros(1)
        S = np.zeros(self.num_sites); Rv = np.zeros(self.num_sites); T = C.c_double(0.0); dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32)
        self._ck(self._lib.emat_Ttwiddle_l_partial(self._h, off.ctypes.data_as(ip), node.ctypes.data_as(ip), val.ctypes.data_as(dp), S.ctypes.data_as(dp), Rv.ctypes.data_as(dp), C.byref(T)),
                 "emat_Ttwiddle_l_partial")
        return S, Rv, float(T.value)

    def Ttwiddle_l_finish(self, S, R, tree_length: float) -> np.ndarray:
        S = np.ascontiguousarray(S, np.float64); R = np.ascontiguousarray(R, np.float64); out = np.zeros(self.num_sites); dp = C.POINTER(C.c_double)
        self._ck(self._lib.emat_Ttwiddle_l_finish(self._h, S.ctypes.data_as(dp), R.ctypes.data_as(dp), tree_length, out.ctypes.data_as(dp)), "emat_Ttwiddle_l_finish")
        return out

    def scalable_coalescent_partial(self, t_ref: float, t_step: float, first_cell: int, num_cells: int):
        """(partial k_bar grid over [first_cell, first_cell + num_cells), sum of -log N(t) over inner nodes, first cell needed)."""
        kb = np.zeros(max(num_cells, 1)); logs = C.c_double(); need = C.c_int32()
        self._ck(self._lib.emat_scalable_coalescent_partial(self._h, t_ref, t_step, first_cell, num_cells, kb.ctypes.data_as(C.POINTER(C.c_double)), C.byref(logs), C.byref(need)),
                 "emat_scalable_coalescent_partial")
        return kb[:num_cells], float(logs.value), int(need.value)

    def scalable_coalescent_log_prior_from_grid(self, t_ref: float, t_step: float, first_cell: int, k_bar_sum: np.ndarray, sum_neg_log_pop: float) -> float:
        kb = np.ascontiguousarray(k_bar_sum, np.float64); v = C.c_double()
        self._ck(self._lib.emat_scalable_coalescent_log_prior(self._h, t_ref, t_step, first_cell, kb.shape[0], kb.ctypes.data_as(C.POINTER(C.c_double)), sum_neg_log_pop, C.byref(v)),
                 "emat_scalable_coalescent_log_prior")
        return float(v.value)

    def debug_pop(self, pop: PopModel, op: int, a, b) -> np.ndarray:
        """Test hook: the device's pop_at_time (op 0) / pop_integral (op 1) / intensity_integral (op 2), point by point."""
        a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros_like(a)
        m = pop.c_struct(); dp = C.POINTER(C.c_double)
        self._ck(self._lib.emat_debug_pop(self._h, C.byref(m), op, a.shape[0], a.ctypes.data_as(dp), b.ctypes.data_as(dp), out.ctypes.data_as(dp)), "emat_debug_pop")
        return out

    def debug_interval_op(self, op: int, a, b):
        """Test hook: the device's interval-set algebra; sets as lists of [start, end).  Ops 7 and 8: the two lists of iv_split (a - b, and what is left of a)."""
        A = np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 2)); Bv = np.ascontiguousarray(np.asarray(b, np.int32).reshape(-1))
        nb = Bv.shape[0] if op == 5 else Bv.shape[0] // 2
        out = np.zeros((A.shape[0] + nb + 1, 2), np.int32); n = C.c_int32(); ip = C.POINTER(C.c_int32)
        self._ck(self._lib.emat_debug_interval_op(self._h, op, A.ctypes.data_as(ip), A.shape[0], Bv.ctypes.data_as(ip), nb, out.ctypes.data_as(ip), C.byref(n)), "emat_debug_interval_op")
        return out[: n.value].tolist() if op <= 3 or op in (7, 8) else bool(n.value)

    def debug_tree_query(self, part: int, op: int, a, b) -> np.ndarray:
        """Test hook: the moves' find_MRCA_of (op 0) / descends_from (op 1) on a resident part; -1 = no node."""
        a = np.ascontiguousarray(a, np.int32); b = np.ascontiguousarray(b, np.int32); out = np.zeros_like(a); ip = C.POINTER(C.c_int32)
        self._ck(self._lib.emat_debug_tree_query(self._h, part, op, a.shape[0], a.ctypes.data_as(ip), b.ctypes.data_as(ip), out.ctypes.data_as(ip)), "emat_debug_tree_query")
        return out

    def debug_graft(self, part: int, X: int, mu_proposal: float, mode: int = 0, new_sibling: int = 0, new_t_P: float = 0.0) -> dict:
        """Test hook: the moves' own graft analysis (mode 0), + peel (1), + apply (2), or a whole re-attachment with a proposed
        new graft (3) on a resident part; returns what emat_debug_graft writes out, decoded (decode_graft_output)."""
        out = np.zeros(4096); n = C.c_int32()
        self._ck(self._lib.emat_debug_graft(self._h, part, X, mu_proposal, mode, new_sibling, new_t_P, out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[0], C.byref(n)), "emat_debug_graft")
        return decode_graft_output(out[: n.value], mode)

    def debug_edit(self, part: int, X: int, ops):
        """Test hook: one tree-editing session on node X; ops = [["slide", t] | ["hop_up"] | ["flip"] | ["hop_down", node], ...]."""
        kind = np.array([{"slide": 0, "hop_up": 1, "flip": 2, "hop_down": 3}[o[0]] for o in ops], np.int32)
        node = np.array([int(o[1]) if o[0] == "hop_down" else -1 for o in ops], np.int32)
        t = np.array([float(o[1]) if o[0] == "slide" else 0.0 for o in ops], np.float64)
        self._ck(self._lib.emat_debug_edit(self._h, part, X, kind.shape[0], _ptr(kind, C.c_int32), _ptr(node, C.c_int32), _ptr(t, C.c_double)), "emat_debug_edit")

    def debug_sample_history(self, part: int, branch, t_end, start_seq, T: float, mu: float):
        """Test hook: one sampled mutational history per (branch[i], t_end[i]) on a resident part; returns a list of histories, each a
        list of [from, site, to, t]."""
        branch = np.ascontiguousarray(branch, np.int32); t_end = np.ascontiguousarray(t_end, np.float64); seq = np.ascontiguousarray(start_seq, np.uint8)
        n = branch.shape[0]; cap = 64 * n + 1024
        counts = np.zeros(max(n, 1), np.int32); muts = np.zeros((cap, 4)); tot = C.c_int32()
        self._ck(self._lib.emat_debug_sample_history(self._h, part, n, _ptr(branch, C.c_int32), _ptr(t_end, C.c_double), _ptr(seq, C.c_uint8), T, mu,
                                                     _ptr(counts, C.c_int32), _ptr(muts, C.c_double), cap, C.byref(tot)), "emat_debug_sample_history")
        out, k = [], 0
        for i in range(n):
            out.append([[int(m[1]), int(m[0]), int(m[2]), float(m[3])] for m in muts[k: k + counts[i]]]); k += int(counts[i])
        return out

    def site_rate_moves(self, Ttwiddle_l, num_muts_l, alpha: float, num_alpha_steps: int = 10, key: int = 0, trace: bool = True) -> "SiteRateResult":
        """alpha_moves + gibbs_sample_all_nus on the device (include/emat_backend.h: emat_site_rate_moves), from the run's summed statistics."""
        T = np.ascontiguousarray(Ttwiddle_l, np.float64); M = np.ascontiguousarray(num_muts_l, np.int32)
        if T.shape != (self.num_sites,) or M.shape != (self.num_sites,):
            raise ValueError("Ttwiddle_l and num_muts_l must have one entry per site")
        args = (T.ctypes.data_as(C.POINTER(C.c_double)), M.ctypes.data_as(C.POINTER(C.c_int32)), float(alpha), int(num_alpha_steps), int(key) & _KEY_MASK)
        return _traced_call(self, "emat_site_rate_moves", args, _SITE_RATE_TRACE, int(num_alpha_steps), trace and num_alpha_steps > 0, SiteRateResult)

    def _pop_moves(self, name: str, pop: PopModel, spec, t_ref: float, t_step: float, first_cell: int, k_bar, inner_t, key: int, res):
        """A population group's call emat_<name> on the statistics handed in, or emat_tree_<name> on the resident tree's own where `k_bar` is None."""
        m = pop.c_struct(); sp = spec.c_struct(); dp = C.POINTER(C.c_double); stats = ()
        if k_bar is not None:
            kb = np.ascontiguousarray(k_bar, np.float64).reshape(-1); ts = np.ascontiguousarray(inner_t, np.float64).reshape(-1)
            stats = (int(first_cell), kb.shape[0], kb.ctypes.data_as(dp), ts.shape[0], ts.ctypes.data_as(dp))
        name = ("emat_tree_" if k_bar is None else "emat_") + name
        self._ck(getattr(self._lib, name)(self._h, C.byref(m), C.byref(sp), float(t_ref), float(t_step), *stats, int(key) & _KEY_MASK, C.byref(res)), name)

    def skygrid_moves(self, pop: PopModel, spec: "SkygridSpec", t_ref: float, t_step: float, first_cell: int, k_bar, inner_t, key: int = 0, trace: bool = False) -> "SkygridMovesResult":
        """skygrid_tau_move + the zero mode's Gibbs move + the HMC on the gammas, on the device (include/emat_backend.h: emat_skygrid_moves), from the
        run's statistics: the lineage grid k_bar over the cells first_cell .. and the inner nodes' times."""
        n = int(pop.c_struct().skygrid_num_knots)
        res, gamma, tr = _skygrid_result_c(n, spec.hmc_steps, trace)
        self._pop_moves("skygrid_moves", pop, spec, t_ref, t_step, first_cell, k_bar, inner_t, key, res)
        return SkygridMovesResult(res, gamma[:n], tr)

    def tree_coalescent_stats(self, t_ref: float, t_step: float):
        """(first_cell, k_bar, inner_t) of the tree resident in HBM (emat_tree_coalescent_stats): Scalable_coalescent_prior's whole-tree grid over the
        cells from the root's to the latest tip's, and the inner nodes' times in node order."""
        fc, nc, ni = C.c_int32(), C.c_int32(), C.c_int32(); dp = C.POINTER(C.c_double)
        self._ck(self._lib.emat_tree_coalescent_stats(self._h, float(t_ref), float(t_step), C.byref(fc), C.byref(nc), None, 0, None, 0, C.byref(ni)), "emat_tree_coalescent_stats")
        kb = np.zeros(max(1, nc.value)); ts = np.zeros(max(1, ni.value))
        self._ck(self._lib.emat_tree_coalescent_stats(self._h, float(t_ref), float(t_step), C.byref(fc), C.byref(nc), kb.ctypes.data_as(dp), kb.shape[0], ts.ctypes.data_as(dp), ts.shape[0], C.byref(ni)),
                 "emat_tree_coalescent_stats")
        return fc.value, kb[: nc.value], ts[: ni.value]

    def tree_skygrid_moves(self, pop: PopModel, spec: "SkygridSpec", t_ref: float, t_step: float, key: int = 0, trace: bool = False) -> "SkygridMovesResult":
        """emat_skygrid_moves on the statistics of the tree resident in HBM, which never leave it (emat_tree_skygrid_moves)."""
        return self.skygrid_moves(pop, spec, t_ref, t_step, 0, None, None, key, trace)

    def exp_pop_moves(self, pop: PopModel, spec: "ExpPopSpec", t_ref: float, t_step: float, first_cell: int, k_bar, inner_t, key: int = 0, trace: bool = False) -> "ExpPopMovesResult":
        """`spec.rounds` times pop_size_move + pop_growth_rate_move on the device (include/emat_backend.h: emat_exp_pop_moves), from the run's
        statistics: the lineage grid k_bar over the cells first_cell .. and the inner nodes' times."""
        res, tr = _traced_result_c(*_EXP_POP_TRACE, 2 * spec.rounds, trace)
        self._pop_moves("exp_pop_moves", pop, spec, t_ref, t_step, first_cell, k_bar, inner_t, key, res)
        return _traced_result(ExpPopMovesResult, res, tr)

    def tree_exp_pop_moves(self, pop: PopModel, spec: "ExpPopSpec", t_ref: float, t_step: float, key: int = 0, trace: bool = False) -> "ExpPopMovesResult":
        """emat_exp_pop_moves on the statistics of the tree resident in HBM, which never leave it (emat_tree_exp_pop_moves)."""
        return self.exp_pop_moves(pop, spec, t_ref, t_step, 0, None, None, key, trace)

    def _parts_moves(self, name: str, spec, stats, key: int, trace_of, steps: int, trace: bool, result):
        """A parts' group's call emat_<name> on the statistics handed in (`stats`: the C arguments that carry them), or emat_parts_<name> on those of the parts on
        this handle where `stats` is None."""
        sp = spec.c_struct()
        return _traced_call(self, ("emat_parts_" if stats is None else "emat_") + name, (C.byref(sp), *(stats or ()), int(key) & _KEY_MASK), trace_of, steps, trace, result)

    def subst_moves(self, spec: "SubstSpec", Ttwiddle_beta_a, num_muts_beta_ab, root_state_counts, key: int = 0, trace: bool = False) -> "SubstMovesResult":
        """mu_move, then `spec.rounds` times hky_frequencies_move + hky_kappa_move on the device (include/emat_backend.h: emat_subst_moves), from the
        run's summed statistics: Ttwiddle_beta_a [P][4], num_muts_beta_ab [P][4][4] and the state counts at the run's root [4]."""
        T = np.ascontiguousarray(Ttwiddle_beta_a, np.float64); M = np.ascontiguousarray(num_muts_beta_ab, np.int64); Cn = np.ascontiguousarray(root_state_counts, np.int64)
        T = T.reshape(-1, 4); nP = T.shape[0]
        if M.size != 16 * nP or Cn.size != 4:
            raise ValueError("num_muts_beta_ab must be [P][4][4] for the P of Ttwiddle_beta_a, root_state_counts [4]")
        stats = (nP, T.ctypes.data_as(C.POINTER(C.c_double)), M.ctypes.data_as(C.POINTER(C.c_int64)), Cn.ctypes.data_as(C.POINTER(C.c_int64)))
        return self._parts_moves("subst_moves", spec, stats, key, _SUBST_TRACE, 2 * spec.rounds, trace, SubstMovesResult)

    def _model_partitions(self) -> int:
        """P of the model the handle holds: what a caller asks emat_get_evo first, to size what it fetches next."""
        n = C.c_int32(0)
        self._ck(self._lib.emat_get_evo(self._h, C.byref(n), None, None, None), "emat_get_evo")
        return n.value

    def parts_subst_stats(self, num_partitions: Optional[int] = None):
        """(Ttwiddle_beta_a [P][4], num_muts_beta_ab [P][4][4], root_state_counts [4]) of the parts on this handle, reduced on the device (emat_parts_subst_stats).
        The call writes for the P of the handle's model, so the arrays are sized by it (emat_get_evo); `num_partitions`, when given, must be that P."""
        nP = self._model_partitions()
        if num_partitions is not None and int(num_partitions) != nP:
            raise ValueError("num_partitions is %d, the handle's model has %d site partitions" % (num_partitions, nP))
        T = np.zeros((nP, 4)); M = np.zeros((nP, 4, 4), np.int64); Cn = np.zeros(4, np.int64)
        self._ck(self._lib.emat_parts_subst_stats(self._h, T.ctypes.data_as(C.POINTER(C.c_double)), M.ctypes.data_as(C.POINTER(C.c_int64)), Cn.ctypes.data_as(C.POINTER(C.c_int64))),
                 "emat_parts_subst_stats")
        return T, M, Cn

    def parts_subst_moves(self, spec: "SubstSpec", key: int = 0, trace: bool = False) -> "SubstMovesResult":
        """emat_subst_moves on the statistics of the parts on this handle, which never leave it (emat_parts_subst_moves)."""
        return self._parts_moves("subst_moves", spec, None, key, _SUBST_TRACE, 2 * spec.rounds, trace, SubstMovesResult)

    def mpox_moves(self, spec: "MpoxSpec", Ttwiddle_beta_a, num_muts_beta_ab, key: int = 0, trace: bool = False) -> "MpoxMovesResult":
        """`spec.rounds` rounds of the Gibbs draws of mu and rho = mu* / mu of the APOBEC model on the device (include/emat_backend.h: emat_mpox_moves), from the
        run's summed statistics of its two site partitions: Ttwiddle_beta_a [2][4] and num_muts_beta_ab [2][4][4]."""
        T = np.ascontiguousarray(Ttwiddle_beta_a, np.float64); M = np.ascontiguousarray(num_muts_beta_ab, np.int64)
        if T.size != 8 or M.size != 32:
            raise ValueError("Ttwiddle_beta_a must be [2][4] and num_muts_beta_ab [2][4][4]")
        stats = (T.ctypes.data_as(C.POINTER(C.c_double)), M.ctypes.data_as(C.POINTER(C.c_int64)))
        return self._parts_moves("mpox_moves", spec, stats, key, _MPOX_TRACE, spec.rounds, trace, MpoxMovesResult)

    def parts_mpox_moves(self, spec: "MpoxSpec", key: int = 0, trace: bool = False) -> "MpoxMovesResult":
        """emat_mpox_moves on the statistics of the parts on this handle, which never leave it (emat_parts_mpox_moves)."""
        return self._parts_moves("mpox_moves", spec, None, key, _MPOX_TRACE, spec.rounds, trace, MpoxMovesResult)

    def get_evo(self):
        """(mu [P], pi [P][4], q [P][4][4]) of the model the handle holds (emat_get_evo)."""
        nP = self._model_partitions(); n = C.c_int32(nP); dp = C.POINTER(C.c_double)
        mu = np.zeros(nP); pi = np.zeros((nP, 4)); q = np.zeros((nP, 4, 4))
        self._ck(self._lib.emat_get_evo(self._h, C.byref(n), mu.ctypes.data_as(dp), pi.ctypes.data_as(dp), q.ctypes.data_as(dp)), "emat_get_evo")
        return mu, pi, q

    def debug_pop_gradient(self, pop: PopModel, op: int, k: int, a, b) -> np.ndarray:
        """Test hook: the device's d log(integral of N over [a, b]) / d gamma_k (op 3) / d log N(a) / d gamma_k (op 4), point by point."""
        a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros_like(a)
        m = pop.c_struct(); dp = C.POINTER(C.c_double)
        self._ck(self._lib.emat_debug_pop_gradient(self._h, C.byref(m), int(op), int(k), a.shape[0], a.ctypes.data_as(dp), b.ctypes.data_as(dp), out.ctypes.data_as(dp)), "emat_debug_pop_gradient")
        return out

    def nu_l(self) -> np.ndarray:
        """The handle's relative site rates: what set_evo was given, or the last site-rate move's draws."""
        out = np.zeros(self.num_sites)
        self._ck(self._lib.emat_get_nu_l(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "emat_get_nu_l")
        return out

    def debug_sample_gamma(self, key: int, n: int, shape: float, rate: float) -> np.ndarray:
        """Test hook: n draws of the site-rate moves' gamma sampler, draw i from the stream (key, i)."""
        out = np.zeros(max(0, int(n)))
        self._ck(self._lib.emat_debug_sample_gamma(self._h, int(key) & _KEY_MASK, int(n), float(shape), float(rate), out.ctypes.data_as(C.POINTER(C.c_double))), "emat_debug_sample_gamma")
        return out

    def debug_gamma(self, mode: int, a, x_or_q) -> np.ndarray:
        """Test hook: the device's gamma_q (mode 0) / gamma_q_inv (mode 1), point by point."""
        a = np.ascontiguousarray(a, np.float64); x = np.ascontiguousarray(x_or_q, np.float64); out = np.zeros_like(a)
        dp = C.POINTER(C.c_double)
        self._ck(self._lib.emat_debug_gamma(self._h, mode, a.shape[0], a.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp)), "emat_debug_gamma")
        return out

    def part_download(self, part: int) -> FlatTree:
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_part_get_sizes(self._h, part, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_part_get_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        self._ck(self._lib.emat_part_download(self._h, part, C.byref(v)), "emat_part_download")
        t.root = v.root
        return t.trimmed()

    def part_derived(self, part: int, num_nodes: int):
        lam = np.zeros(num_nodes)
        nmiss = np.zeros(num_nodes, np.int32)
        g, a = C.c_double(), C.c_double()
        self._ck(self._lib.emat_part_get_derived(self._h, part, _ptr(lam, C.c_double), _ptr(nmiss, C.c_int32), C.byref(g), C.byref(a)), "emat_part_get_derived")
        return lam, nmiss, float(g.value), float(a.value)

    def part_state_frequencies(self, part: int) -> np.ndarray:
        """Subrun::state_frequencies_of_ref_sequence_per_partition (subrun.h:45): counts[site partition, state] of the reference sequence."""
        n = C.c_int32(8)
        counts = np.zeros((8, 4), np.int32)
        self._ck(self._lib.emat_part_get_state_frequencies(self._h, part, C.byref(n), _ptr(counts, C.c_int32)), "emat_part_get_state_frequencies")
        return counts[: n.value].copy()

    def part_coalescent(self, part: int, cap: int = 1 << 16):
        for _ in range(2):      # (a grid that outgrew `cap` -- a root that wandered for 100 000 moves over a fine grid -- reports its length: once more with that)
            n = C.c_int32(cap)
            kb, kt, k, ps = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap)
            na = np.zeros(cap, np.int32)
            tr, ts = C.c_double(), C.c_double()
            st = self._lib.emat_part_get_coalescent(self._h, part, C.byref(n), _ptr(kb, C.c_double), _ptr(kt, C.c_double), _ptr(k, C.c_double),
                                                    _ptr(ps, C.c_double), _ptr(na, C.c_int32), C.byref(tr), C.byref(ts))
            if st == 0 or n.value <= cap:
                break
            cap = n.value
        self._ck(st, "emat_part_get_coalescent")
        m = n.value
        return dict(k_bar_p=kb[:m], k_twiddle_bar_p=kt[:m], k_twiddle_bar=k[:m], popsize_bar=ps[:m], num_active_parts=na[:m], t_ref=tr.value, t_step=ts.value)

    def part_stats(self, part: int) -> dict:
        s = _PartStatsC()
        self._ck(self._lib.emat_part_get_stats(self._h, part, C.byref(s)), "emat_part_get_stats")
        return dict(status=s.status, num_nodes=s.num_nodes, moves_done=s.moves_done, proposed=list(s.proposed), accepted=list(s.accepted),
                    algorithmic_bytes=s.algorithmic_bytes, rng_draws=s.rng_draws, device_ticks=s.device_ticks, algorithmic_write_bytes=s.algorithmic_write_bytes)

    def build_usher_like(self, tips: "TipDescs", seed: int) -> "FlatTree":
        """the reference's UShER-like initial tree from tip descriptors (set_ref_sequence first); the graft loop runs on the device."""
        td = tips.c_struct()
        self._ck(self._lib.emat_tree_build_usher_like(self._h, C.byref(td), seed), "emat_tree_build_usher_like")
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_tree_built_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_tree_built_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        self._ck(self._lib.emat_tree_built_get(self._h, C.byref(v)), "emat_tree_built_get")
        t.root = v.root
        return t.trimmed()

    def build_default(self, tips: "TipDescs", seed: int):
        """the reference's DEFAULT initial tree (build_initial_phylo_tree: maximum-parsimony guide tree, nearest-first
        rebuilds, SPR refinement, regression rooting, dating) from tip descriptors (set_ref_sequence first).  Host code, as in the
        reference: works on a device = -1 handle.  Returns (tree, ref, report): the tree is written against `ref`, the ROOT's sequence."""
        td = tips.c_struct()
        rep = (C.c_int32 * 4)()
        self._ck(self._lib.emat_tree_build_default(self._h, C.byref(td), seed, rep), "emat_tree_build_default")
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_tree_built_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_tree_built_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        self._ck(self._lib.emat_tree_built_get(self._h, C.byref(v)), "emat_tree_built_get")
        t.root = v.root
        ref = np.zeros(self.num_sites, np.uint8)
        self._ck(self._lib.emat_tree_built_ref(self._h, ref.ctypes.data_as(C.POINTER(C.c_uint8))), "emat_tree_built_ref")
        return t.trimmed(), ref, dict(guide_deltas=rep[0], refined_deltas=rep[1], spr_deltas=rep[2], rooting="regression" if rep[3] == 0 else "midpoint")

    def align_begin(self, max_rows: int) -> None:
        """Binds the alignment store to `max_rows` rows of num_sites characters (include/emat_backend.h: emat_align_begin); 0 releases it."""
        self._ck(self._lib.emat_align_begin(self._h, max_rows), "emat_align_begin")

    def align_push(self, rows, row_stride: Optional[int] = None) -> None:
        """Pushes rows of ASCII characters: a (rows, >= num_sites) uint8 array whose row length is the stride, or bytes with `row_stride`."""
        a = np.frombuffer(rows, np.uint8) if isinstance(rows, (bytes, bytearray)) else np.ascontiguousarray(rows, np.uint8)
        if a.ndim == 2:
            n, stride = a.shape
        else:
            stride = self.num_sites if row_stride is None else row_stride
            n = 0 if a.size == 0 else (a.size - self.num_sites) // stride + 1
        self._ck(self._lib.emat_align_push_rows(self._h, n, _ptr(a, C.c_uint8), stride), "emat_align_push_rows")

    def align_finish(self, ref=None, row_dated=None) -> "Alignment":
        """The reference sequence (`ref`, or the consensus) and, of the rows that are valid and dated, the tip descriptors (emat_align_finish, emat_align_get)."""
        ref_c = None if ref is None else np.ascontiguousarray(ref, np.uint8)
        dated_c = None if row_dated is None else np.ascontiguousarray(row_dated, np.uint8)
        rep = _AlignReportC()
        self._ck(self._lib.emat_align_finish(self._h, None if ref_c is None else _ptr(ref_c, C.c_uint8), None if dated_c is None else _ptr(dated_c, C.c_uint8), C.byref(rep)), "emat_align_finish")
        return self._align_get(rep)

    def _align_get(self, rep: "_AlignReportC") -> "Alignment":
        T, R, L = rep.num_tips, int(rep.num_rows), self.num_sites
        d_off = np.zeros(T + 1, np.int32); d_site = np.zeros(rep.num_deltas, np.int32); d_to = np.zeros(rep.num_deltas, np.uint8)
        m_off = np.zeros(T + 1, np.int32); m_start = np.zeros(rep.num_intervals, np.int32); m_end = np.zeros(rep.num_intervals, np.int32)
        ref = np.zeros(L, np.uint8); counts = np.zeros((L, 4), np.int32)
        status = np.zeros(R, np.int32); bad_site = np.zeros(R, np.int32); bad_byte = np.zeros(R, np.uint8); loss = np.zeros(R, np.int32)
        arrays = _AlignArraysC(_ptr(d_off, C.c_int32), _ptr(d_site, C.c_int32), _ptr(d_to, C.c_uint8), _ptr(m_off, C.c_int32), _ptr(m_start, C.c_int32), _ptr(m_end, C.c_int32),
                               _ptr(ref, C.c_uint8), _ptr(counts, C.c_int32), _ptr(status, C.c_int32), _ptr(bad_site, C.c_int32), _ptr(bad_byte, C.c_uint8), _ptr(loss, C.c_int32))
        self._ck(self._lib.emat_align_get(self._h, C.byref(arrays)), "emat_align_get")
        nan = np.full(T, np.nan, np.float32)
        tips = TipDescs(nan, nan.copy(), d_off, d_site, d_to, m_off, m_start, m_end)
        report = {k: int(getattr(rep, k)) for k, _ in _AlignReportC._fields_}
        return Alignment(tips, ref, counts, status, bad_site, bad_byte, loss, report)

    def fasta_records(self):
        """What the last load or framing left on the handle: (names, lengths, t_min, t_max, dated), one entry per record (emat_fasta_get)."""
        rep = _FastaReportC()
        self._ck(self._lib.emat_fasta_sizes(self._h, C.byref(rep)), "emat_fasta_sizes")
        n = rep.num_records
        names = C.create_string_buffer(max(int(rep.names_bytes), 1))
        lengths = np.zeros(n, np.int64); t_min = np.zeros(n, np.float32); t_max = np.zeros(n, np.float32); dated = np.zeros(n, np.uint8)
        self._ck(self._lib.emat_fasta_get(self._h, names, _ptr(lengths, C.c_int64), _ptr(t_min, C.c_float), _ptr(t_max, C.c_float), _ptr(dated, C.c_uint8)), "emat_fasta_get")
        return [x.decode("utf-8", "replace") for x in names.raw[: int(rep.names_bytes)].split(b"\0")[:n]], lengths, t_min, t_max, dated

    def fasta_frame(self, text: bytes):
        """Frames the records of a FASTA text without a device (emat_fasta_frame_memory); returns what fasta_records returns."""
        a = np.frombuffer(text, np.uint8)
        self._ck(self._lib.emat_fasta_frame_memory(self._h, _ptr(a, C.c_uint8), a.size, None), "emat_fasta_frame_memory")
        return self.fasta_records()

    def load_fasta(self, path_or_bytes, ref=None, chunk_rows: int = 0) -> "TipDescs":
        """An aligned FASTA (a path, or its text as bytes) to tip descriptors, ready for build_usher_like / build_default after
        set_ref_sequence(tips.ref): the rows that are valid and dated, in input order, with `names`, the reference sequence `ref` (the one
        given, or the consensus of the valid rows), `report` (emat_fasta_report) and `alignment` (the per-row read-outs)."""
        ref_c = None if ref is None else np.ascontiguousarray(ref, np.uint8)
        ref_p = None if ref_c is None else _ptr(ref_c, C.c_uint8)
        rep = _FastaReportC()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            a = np.frombuffer(path_or_bytes, np.uint8)
            self._ck(self._lib.emat_fasta_load_memory(self._h, _ptr(a, C.c_uint8), a.size, ref_p, chunk_rows, C.byref(rep)), "emat_fasta_load_memory")
        else:
            self._ck(self._lib.emat_fasta_load(self._h, os.fsencode(path_or_bytes), ref_p, chunk_rows, C.byref(rep)), "emat_fasta_load")
        al = self._align_get(rep.rows)
        names, _, t_min, t_max, _ = self.fasta_records()
        is_tip = al.row_status >= 0
        tips = al.tips
        tips.t_min = np.ascontiguousarray(t_min[is_tip]); tips.t_max = np.ascontiguousarray(t_max[is_tip])
        tips.names = [nm for nm, k in zip(names, is_tip) if k]
        tips.ref = al.ref; tips.alignment = al
        tips.report = dict(num_records=rep.num_records, num_dated=rep.num_dated, **al.report)
        return tips

    def main_class_mask(self, num_parts: int) -> np.ndarray:
        """Debugging aid: which resident parts run in the main launch (k_run_moves) rather than in a side class (k_run_moves_side)."""
        out = np.zeros(num_parts, np.int32)
        self._lib.emat_debug_arena_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        self._ck(self._lib.emat_debug_arena_bytes(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "emat_debug_arena_bytes")
        return out >= 0

    def debug_slab_layout(self, part: int) -> dict:
        out = (C.c_uint32 * 8)()
        self._ck(self._lib.emat_debug_slab_layout(self._h, part, out), "emat_debug_slab_layout")
        return dict(zip(("header", "nodes", "cells", "trace", "heap_used", "heap_cap", "scratch", "num_cells"), [int(x) for x in out]))

    def part_rng(self, part: int) -> dict:
        """Where the part's Philox stream stands: key, blocks consumed, pending half block."""
        k, c, sp, hs = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
        self._ck(self._lib.emat_part_get_rng(self._h, part, C.byref(k), C.byref(c), C.byref(sp), C.byref(hs)), "emat_part_get_rng")
        return dict(key=int(k.value), counter=int(c.value), spare=int(sp.value), has_spare=bool(hs.value))

    def part_trace(self, part: int, cap: int) -> np.ndarray:
        n = C.c_int32(cap)
        tr = np.zeros((max(cap, 1), 4))
        self._ck(self._lib.emat_part_get_trace(self._h, part, C.byref(n), _ptr(tr, C.c_double)), "emat_part_get_trace")
        return tr[: n.value]

    def last_error(self) -> str:
        return self._lib.emat_last_error(self._h).decode()


class EmatRun:
    """Host-side driver above the boundary (include/emat_host.h): partitioning, repartition, reassemble."""

    def __init__(self, backend: Optional[EmatBackend], tree: FlatTree, ref_sequence: np.ndarray, seed: int):
        self._lib = load_library()
        self.backend = backend
        self._ref = np.ascontiguousarray(ref_sequence, np.uint8)
        self.num_sites = int(self._ref.shape[0])
        self._h = C.c_void_p()
        v = tree.c_view()
        st = self._lib.emat_run_create(backend.handle if backend is not None else None, C.byref(v), _ptr(self._ref, C.c_uint8), self.num_sites, int(seed), C.byref(self._h))
        if st != 0:
            raise EmatError("emat_run_create failed: %s" % STATUS_NAMES.get(st, st))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.emat_run_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st: int, what: str):
        if st != 0:
            msg = self._lib.emat_run_last_error(self._h)
            raise EmatError("%s: %s (%s)" % (what, STATUS_NAMES.get(st, st), msg.decode() if msg else ""))

    # What sizes the traces of the global moves' calls until a setter says otherwise: the Skygrid's knots and HMC steps, the rounds of the other groups.
    _sky_knots = 0; _sky_steps = 25; _xp_rounds = 0; _sb_rounds = 0; _mx_rounds = 0

    def _set_moves(self, name: str, on: bool, spec):
        """A group's setter emat_run_<name>; the C spec comes back, whose rounds (or steps) size the traces of the group's calls."""
        sp = spec.c_struct()
        self._ck(getattr(self._lib, name)(self._h, 1 if on else 0, C.byref(sp)), name)
        return sp

    def set_num_parts(self, n: int):
        self._ck(self._lib.emat_run_set_num_parts(self._h, n), "emat_run_set_num_parts")

    def set_max_part_nodes(self, n: int):
        """Not in the reference: parts larger than n nodes get further, randomly drawn cut nodes at every repartition
        (0 = off, the reference's rule exactly: the default; -1 = three times the mean part size)."""
        self._ck(self._lib.emat_run_set_max_part_nodes(self._h, n), "emat_run_set_max_part_nodes")

    def partition_stats(self) -> dict:
        """The last repartition: number of parts, nodes of the largest, cut nodes added by the size limit, the limit in effect."""
        a, b, c, e = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_run_partition_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(e)), "emat_run_partition_stats")
        return {"num_parts": a.value, "largest_part_nodes": b.value, "extra_cuts": c.value, "max_part_nodes": e.value}

    def follow_draws(self, leader: "Optional[EmatRun]"):
        """This run takes the partition draws of `leader` (same process, seed, tree, settings) instead of drawing them again (emat_multi's shards)."""
        self._ck(self._lib.emat_run_follow_draws(self._h, leader._h if leader is not None else None), "emat_run_follow_draws")

    def draw_partition(self):
        """The draw of the coming cycle's partition (stencil refresh, pick, part-size limit) ahead of emat_run_repartition."""
        self._ck(self._lib.emat_run_draw_partition(self._h), "emat_run_draw_partition")

    def debug_redraw_partition(self) -> np.ndarray:
        """Test hook: the sorted cut nodes the last repartition's draw (same stencil, same refinement stream) gives on the tree as it is now."""
        n = C.c_int32(0)
        self._lib.emat_run_debug_redraw_partition(self._h, None, C.byref(n))        # (asks for the count)
        cuts = np.zeros(max(1, n.value), np.int32); n = C.c_int32(cuts.shape[0])
        self._ck(self._lib.emat_run_debug_redraw_partition(self._h, _ptr(cuts, C.c_int32), C.byref(n)), "emat_run_debug_redraw_partition")
        return cuts[: n.value].copy()

    def set_hky(self, mu: float, kappa: float, pi, nu_l=None):
        pi = np.ascontiguousarray(pi, np.float64)
        nu = None if nu_l is None else np.ascontiguousarray(nu_l, np.float64)
        self._ck(self._lib.emat_run_set_hky(self._h, mu, kappa, _ptr(pi, C.c_double), None if nu is None else _ptr(nu, C.c_double)), "emat_run_set_hky")

    def set_pop_model(self, pop: PopModel):
        m = pop.c_struct()
        self._ck(self._lib.emat_run_set_pop_model(self._h, C.byref(m)), "emat_run_set_pop_model")
        self._sky_knots = int(m.skygrid_num_knots) if pop.kind == 2 else 0

    def set_coalescent_t_step(self, t_step: float):
        self._ck(self._lib.emat_run_set_coalescent_t_step(self._h, t_step), "emat_run_set_coalescent_t_step")

    def set_flags(self, only_displacing_inner_nodes: bool = False, topology_moves_enabled: bool = True):
        self._ck(self._lib.emat_run_set_flags(self._h, int(only_displacing_inner_nodes), int(topology_moves_enabled)), "emat_run_set_flags")

    def set_reference_remainder(self, on: bool = True):
        """The remainder of count / parts goes to part 0 as in Run::run_local_moves (default: one move each on the first parts)."""
        self._ck(self._lib.emat_run_set_reference_remainder(self._h, 1 if on else 0), "emat_run_set_reference_remainder")

    def set_paranoid(self, on: bool = True):
        self._ck(self._lib.emat_run_set_paranoid(self._h, 1 if on else 0), "emat_run_set_paranoid")

    def repartition(self):
        self._ck(self._lib.emat_run_repartition(self._h), "emat_run_repartition")

    def num_parts(self):
        n, r = C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_run_num_parts(self._h, C.byref(n), C.byref(r)), "emat_run_num_parts")
        return n.value, r.value

    def part(self, i: int):
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_run_part_sizes(self._h, i, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_run_part_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        incl, seed = C.c_int32(), C.c_uint64()
        self._ck(self._lib.emat_run_part_get(self._h, i, C.byref(v), C.byref(incl), C.byref(seed)), "emat_run_part_get")
        t.root = v.root
        return t.trimmed(), bool(incl.value), int(seed.value)

    def part_put(self, i: int, subtree: FlatTree):
        v = subtree.c_view()
        self._ck(self._lib.emat_run_part_put(self._h, i, C.byref(v)), "emat_run_part_put")

    def push_params(self):
        self._ck(self._lib.emat_run_push_params(self._h), "emat_run_push_params")

    def run_moves(self, count: int):
        self._ck(self._lib.emat_run_moves(self._h, count), "emat_run_moves")

    def reassemble(self):
        self._ck(self._lib.emat_run_reassemble(self._h), "emat_run_reassemble")

    def set_site_rate_moves(self, on: bool = True, alpha: float = 1.0):
        """Site-rate moves once per cycle of do_mcmc_steps (off by default); `alpha` is where the steps start (reference default 1.0)."""
        self._ck(self._lib.emat_run_set_site_rate_moves(self._h, 1 if on else 0, float(alpha)), "emat_run_set_site_rate_moves")

    def site_rate_moves(self, trace: bool = False) -> "SiteRateResult":
        """One round of site-rate moves while the parts are out (emat_run_site_rate_moves): ten alpha steps and the draw of every nu_l."""
        return _traced_call(self, "emat_run_site_rate_moves", (), _SITE_RATE_TRACE, 10, trace, SiteRateResult)

    def set_skygrid_moves(self, on: bool = True, spec: "SkygridSpec" = None):
        """The Skygrid population moves once per cycle of do_mcmc_steps, before the repartition (off by default); `spec`: Run's Skygrid settings and the tau to start from."""
        self._sky_steps = int(self._set_moves("emat_run_set_skygrid_moves", on, spec or SkygridSpec()).hmc_steps)

    def skygrid_moves(self, trace: bool = False) -> "SkygridMovesResult":
        """One round of the Skygrid moves on the assembled tree (emat_run_skygrid_moves): tau, the zero mode, the HMC on the gammas."""
        n = self._sky_knots
        res, gamma, tr = _skygrid_result_c(n, self._sky_steps, trace)
        self._ck(self._lib.emat_run_skygrid_moves(self._h, C.byref(res)), "emat_run_skygrid_moves")
        return SkygridMovesResult(res, gamma[:n], tr)

    def set_exp_pop_moves(self, on: bool = True, spec: "ExpPopSpec" = None):
        """The Exponential population moves once per cycle of do_mcmc_steps, before the repartition (off by default); `spec`: Run's settings of the two moves and the rounds."""
        self._xp_rounds = int(self._set_moves("emat_run_set_exp_pop_moves", on, spec or ExpPopSpec()).rounds)

    def exp_pop_moves(self, trace: bool = False) -> "ExpPopMovesResult":
        """One call of the Exponential population moves on the assembled tree (emat_run_exp_pop_moves): `rounds` times the n0 step and the g step."""
        return _traced_call(self, "emat_run_exp_pop_moves", (), _EXP_POP_TRACE, 2 * self._xp_rounds, trace, ExpPopMovesResult)

    def set_subst_moves(self, on: bool = True, spec: "SubstSpec" = None):
        """The substitution-model moves once per cycle of do_mcmc_steps, after the repartition and before the site-rate round (off by default); `spec`: Run's
        mu prior, the three switches and the rounds (its mu, kappa and pi are ignored: the run's own are used)."""
        self._sb_rounds = int(self._set_moves("emat_run_set_subst_moves", on, spec or SubstSpec()).rounds)

    def subst_moves(self, trace: bool = False) -> "SubstMovesResult":
        """One call of the substitution-model moves while the parts are out (emat_run_subst_moves): the mu draw, then `rounds` times the pi step and the kappa step."""
        return _traced_call(self, "emat_run_subst_moves", (), _SUBST_TRACE, 2 * self._sb_rounds, trace, SubstMovesResult)

    def set_mpox(self, on: bool = True, spec: "MpoxSpec" = None):
        """The APOBEC (mpox) model (emat_run_set_mpox): two site partitions cut by the APOBEC context of the sequence at node 0, and its moves once per cycle of
        do_mcmc_steps where the substitution-model moves run; `spec`: mu* to start from, Run's mu prior, its switch and the rounds (its mu is ignored: the run's
        own is used).  Off: one partition and the HKY model again."""
        self._mx_rounds = int(self._set_moves("emat_run_set_mpox", on, spec or MpoxSpec()).rounds)

    def mpox_moves(self, trace: bool = False) -> "MpoxMovesResult":
        """One call of the APOBEC model's moves while the parts are out (emat_run_mpox_moves): `rounds` times the mu draw and the rho draw."""
        return _traced_call(self, "emat_run_mpox_moves", (), _MPOX_TRACE, self._mx_rounds, trace, MpoxMovesResult)

    def mpox(self):
        """(mu, mu*) of the APOBEC model as the driver holds them."""
        mu, mu_star = C.c_double(), C.c_double()
        self._ck(self._lib.emat_run_get_mpox(self._h, C.byref(mu), C.byref(mu_star)), "emat_run_get_mpox")
        return mu.value, mu_star.value

    def mpox_partition(self):
        """(partition_for_site [L], the number of sites with APOBEC context) as drawn when the model was turned on."""
        pfs = np.zeros(self.num_sites, np.int32); n = C.c_int32()
        self._ck(self._lib.emat_run_get_mpox_partition(self._h, pfs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)), "emat_run_get_mpox_partition")
        return pfs, n.value

    def hky(self):
        """(mu, kappa, pi [4]) as the driver holds them."""
        mu, kappa = C.c_double(), C.c_double(); pi = np.zeros(4)
        self._ck(self._lib.emat_run_get_hky(self._h, C.byref(mu), C.byref(kappa), pi.ctypes.data_as(C.POINTER(C.c_double))), "emat_run_get_hky")
        return mu.value, kappa.value, pi

    def exp_pop(self):
        """(n0, g) of the exponential population model as the driver holds them."""
        n0, g = C.c_double(), C.c_double()
        self._ck(self._lib.emat_run_get_exp_pop(self._h, C.byref(n0), C.byref(g)), "emat_run_get_exp_pop")
        return n0.value, g.value

    def skygrid(self):
        """(gamma, tau) of the Skygrid curve as the driver holds them."""
        g = np.zeros(max(1, self._sky_knots)); tau = C.c_double()
        self._ck(self._lib.emat_run_get_skygrid(self._h, g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(tau)), "emat_run_get_skygrid")
        return g[: self._sky_knots], tau.value

    def site_rates(self):
        """(alpha, nu_l) as the driver holds them."""
        a = C.c_double(); nu = np.zeros(self.num_sites)
        self._ck(self._lib.emat_run_get_site_rates(self._h, C.byref(a), nu.ctypes.data_as(C.POINTER(C.c_double))), "emat_run_get_site_rates")
        return a.value, nu

    def Ttwiddle_l(self) -> np.ndarray:
        """calc_Ttwiddle_l of the whole tree, computed from the parts on the device (single process)."""
        out = np.zeros(self.num_sites)
        self._ck(self._lib.emat_run_get_Ttwiddle_l(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "emat_run_get_Ttwiddle_l")
        return out

    def Ttwiddle_ext(self, tree_length_of_part: np.ndarray, num_local_parts: int):
        """(ext_offset, ext_node, ext_length) of this rank's parts for emat_Ttwiddle_l_partial."""
        tl = np.ascontiguousarray(tree_length_of_part, np.float64)
        cap = tl.shape[0] + 1
        off = np.zeros(num_local_parts + 1, np.int32); node = np.zeros(cap, np.int32); val = np.zeros(cap); cnt = C.c_int32()
        self._ck(self._lib.emat_run_Ttwiddle_ext(self._h, tl.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int32)), node.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 val.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(cnt)), "emat_run_Ttwiddle_ext")
        return off, node[: cnt.value], val[: cnt.value]

    # ---- a run sharded over several processes (include/emat_host.h) ----
    def set_shard(self, rank: int, world: int):
        self._ck(self._lib.emat_run_set_shard(self._h, rank, world), "emat_run_set_shard")

    def shard_range(self):
        lo, hi, lr = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_run_shard_range(self._h, C.byref(lo), C.byref(hi), C.byref(lr)), "emat_run_shard_range")
        return lo.value, hi.value, lr.value

    def coalescent_begin(self):
        lo, hi = C.c_double(), C.c_double()
        self._ck(self._lib.emat_run_coalescent_begin(self._h, C.byref(lo), C.byref(hi)), "emat_run_coalescent_begin")
        return lo.value, hi.value

    def run_moves_sharded(self, count: int):
        self._ck(self._lib.emat_run_moves_sharded(self._h, count), "emat_run_moves_sharded")

    def pack_local_parts(self) -> np.ndarray:
        need = C.c_uint64()
        self._ck(self._lib.emat_run_pack_local_parts(self._h, None, 0, C.byref(need)), "emat_run_pack_local_parts")
        buf = np.zeros(int(need.value), np.uint8)
        self._ck(self._lib.emat_run_pack_local_parts(self._h, _ptr(buf, C.c_uint8), buf.shape[0], C.byref(need)), "emat_run_pack_local_parts")
        return buf

    def unpack_parts(self, buf: np.ndarray):
        buf = np.ascontiguousarray(buf, np.uint8)
        self._ck(self._lib.emat_run_unpack_parts(self._h, _ptr(buf, C.c_uint8), buf.shape[0]), "emat_run_unpack_parts")

    def set_device_tree(self, on: bool = True):
        """keep the authoritative tree in HBM; cycles then move only the partition and the topology."""
        self._ck(self._lib.emat_run_set_device_tree(self._h, int(on)), "emat_run_set_device_tree")

    def note_device_reassembled(self, site, to):
        site = np.ascontiguousarray(site, np.int32); to = np.ascontiguousarray(to, np.uint8)
        self._ck(self._lib.emat_run_note_device_reassembled(self._h, int(site.shape[0]), _ptr(site, C.c_int32), _ptr(to, C.c_uint8)), "emat_run_note_device_reassembled")

    def do_mcmc_steps(self, steps: int, local_moves_per_cycle: int = -1):
        self._ck(self._lib.emat_run_do_mcmc_steps(self._h, steps, local_moves_per_cycle), "emat_run_do_mcmc_steps")

    def tree(self):
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_run_tree_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_run_tree_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        ref = np.zeros(self.num_sites, np.uint8)
        self._ck(self._lib.emat_run_tree_get(self._h, C.byref(v), _ptr(ref, C.c_uint8)), "emat_run_tree_get")
        t.root = v.root
        return t.trimmed(), ref

    def t_max_tip(self) -> float:
        t = C.c_double()
        self._ck(self._lib.emat_run_t_max_tip(self._h, C.byref(t)), "emat_run_t_max_tip")
        return float(t.value)


class EmatMultiRun:
    """One run over several GPUs of ONE process (include/emat_host.h, emat_run_create_multi): n backends with the whole tree in the HBM
    of each, the exchanges of a cycle done in C++ over RCCL ("rccl"), through host buffers ("host"), or whichever applies ("auto")."""
    EXCHANGE = {"host": 0, "rccl": 1, "auto": 2}

    def __init__(self, devices: Sequence[int], tree: FlatTree, ref_sequence: np.ndarray, seed: int, exchange: str = "auto", trace_moves: int = 0, use_lds: bool = True):
        self._lib = load_library()
        self._ref = np.ascontiguousarray(ref_sequence, np.uint8)
        self.num_sites = int(self._ref.shape[0])
        dev = np.ascontiguousarray(devices, np.int32)
        cfg = _ConfigC(0, self.num_sites, 0, 0.0, trace_moves, 1 if use_lds else 0)
        self._h = C.c_void_p()
        v = tree.c_view()
        if os.environ.get("EMAT_RCCL_LIB"):
            self._lib.emat_multi_set_rccl_library(os.environ["EMAT_RCCL_LIB"].encode())
        st = self._lib.emat_run_create_multi(_ptr(dev, C.c_int32), int(dev.shape[0]), C.byref(cfg), C.byref(v), _ptr(self._ref, C.c_uint8), self.num_sites, int(seed),
                                             self.EXCHANGE[exchange], C.byref(self._h))
        if st != 0:
            raise EmatError("emat_run_create_multi failed: %s (the engine needs HIP devices; exchange \"rccl\" needs librccl.so and one device per shard)" % STATUS_NAMES.get(st, st))
        self.num_shards = int(self._lib.emat_multi_num_shards(self._h))
        _forward_env_options(lambda k, v: self._ck(self._lib.emat_multi_set_option(self._h, k.encode(), str(v).encode()), "emat_multi_set_option(%s)" % k))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.emat_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st: int, what: str):
        if st != 0:
            msg = self._lib.emat_multi_last_error(self._h)
            raise EmatError("%s: %s (%s)" % (what, STATUS_NAMES.get(st, st), msg.decode() if msg else ""))

    @property
    def exchange(self) -> str:
        return self._lib.emat_multi_exchange(self._h).decode()

    def backend_handle(self, shard: int):
        return self._lib.emat_multi_backend(self._h, shard)

    def set_num_parts(self, n: int):
        self._ck(self._lib.emat_multi_set_num_parts(self._h, n), "emat_multi_set_num_parts")

    def set_hky(self, mu: float, kappa: float, pi, nu_l=None):
        pi = np.ascontiguousarray(pi, np.float64)
        nu = None if nu_l is None else np.ascontiguousarray(nu_l, np.float64)
        self._ck(self._lib.emat_multi_set_hky(self._h, mu, kappa, _ptr(pi, C.c_double), None if nu is None else _ptr(nu, C.c_double)), "emat_multi_set_hky")

    def set_pop_model(self, pop: PopModel):
        m = pop.c_struct()
        self._ck(self._lib.emat_multi_set_pop_model(self._h, C.byref(m)), "emat_multi_set_pop_model")

    def set_coalescent_t_step(self, t_step: float):
        self._ck(self._lib.emat_multi_set_coalescent_t_step(self._h, t_step), "emat_multi_set_coalescent_t_step")

    def set_flags(self, only_displacing_inner_nodes: bool = False, topology_moves_enabled: bool = True):
        self._ck(self._lib.emat_multi_set_flags(self._h, int(only_displacing_inner_nodes), int(topology_moves_enabled)), "emat_multi_set_flags")

    def set_paranoid(self, on: bool = True):
        self._ck(self._lib.emat_multi_set_paranoid(self._h, int(on)), "emat_multi_set_paranoid")

    def repartition(self):
        self._ck(self._lib.emat_multi_repartition(self._h), "emat_multi_repartition")

    def run_moves(self, count: int):
        self._ck(self._lib.emat_multi_run_moves(self._h, count), "emat_multi_run_moves")

    def check_derived(self, tol_scale: float = 1.0):
        self._ck(self._lib.emat_multi_check_derived(self._h, tol_scale), "emat_multi_check_derived")

    def reassemble(self):
        self._ck(self._lib.emat_multi_reassemble(self._h), "emat_multi_reassemble")

    def totals(self):
        g, a = C.c_double(), C.c_double()
        self._ck(self._lib.emat_multi_get_totals(self._h, C.byref(g), C.byref(a)), "emat_multi_get_totals")
        return float(g.value), float(a.value)

    def do_mcmc_steps(self, steps: int, local_moves_per_cycle: int = -1):
        self._ck(self._lib.emat_multi_do_mcmc_steps(self._h, steps, local_moves_per_cycle), "emat_multi_do_mcmc_steps")

    def tree(self, shard: int = 0):
        n, nm, ni, nf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.emat_multi_tree_sizes(self._h, C.byref(n), C.byref(nm), C.byref(ni), C.byref(nf)), "emat_multi_tree_sizes")
        t = FlatTree.empty(n.value, nm.value, ni.value, nf.value)
        v = t.c_view()
        ref = np.zeros(self.num_sites, np.uint8)
        self._ck(self._lib.emat_multi_tree_get(self._h, shard, C.byref(v), _ptr(ref, C.c_uint8)), "emat_multi_tree_get")
        t.root = v.root
        return t.trimmed(), ref
