// emat_move_specs.hpp -- what a global-move spec must satisfy before any model is looked at: one function per spec, the text of the first fault or nullptr.
//
// No HIP in here: the backend's entry points (emat_skygrid_host.hpp, emat_exp_pop_host.hpp) and the run driver's setters (emat_run.cpp) both refuse with these texts.
#ifndef EMAT_MOVE_SPECS_HPP_
#define EMAT_MOVE_SPECS_HPP_

#include <cmath>
#include "../../include/emat_backend.h"

namespace emat {

inline bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }
inline const char* skygrid_spec_fault(const emat_skygrid_spec& s) {
  if (!finite_positive(s.tau)) return "tau must be finite and positive";
  if (s.low_gamma_barrier_enabled && !finite_positive(s.low_gamma_barrier_scale)) return "low_gamma_barrier_scale must be finite and positive with the barrier on";
  if (s.hmc_steps < 0) return "hmc_steps must not be negative";
  if (!finite_positive(s.hmc_mean_dt)) return "hmc_mean_dt must be finite and positive";
  return nullptr;
}

// `g`: the model's growth rate where the caller has a model (the backend), which must lie within the spec's bounds; the test sits where it has always fired.
inline const char* exp_pop_spec_fault(const emat_exp_pop_spec& s, const double* g = nullptr) {
  if (!(s.g_min <= s.g_max)) return "g_min must not exceed g_max, and neither may be NaN";
  if (g && (*g < s.g_min || *g > s.g_max)) return "g lies outside [g_min, g_max]";
  if (!finite_positive(s.g_prior_scale)) return "g_prior_scale must be finite and positive";
  if (!std::isfinite(s.g_prior_mu)) return "g_prior_mu must be finite";
  if (!std::isfinite(s.inv_n0_prior_alpha)) return "inv_n0_prior_alpha must be finite";
  if (!std::isfinite(s.inv_n0_prior_beta)) return "inv_n0_prior_beta must be finite";
  if (s.rounds < 0) return "rounds must not be negative";
  return nullptr;
}

}  // namespace emat

#endif  // EMAT_MOVE_SPECS_HPP_
