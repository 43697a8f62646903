// emat_move_specs.hpp -- what a global-move spec must satisfy before any model is looked at: one function per spec, the text of the first fault or nullptr.
//
// No HIP in here: the backend's entry points (emat_skygrid_host.hpp, emat_exp_pop_host.hpp, emat_subst_host.hpp) and the run driver's setters (emat_run.cpp) both refuse
// with these texts.  Also hky_derive_q, the q of an HKY model, which both derive.
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

// The substitution-model moves (emat_subst_host.hpp; the run driver's setter, which brings its own model, passes with_model = false).
constexpr int k_subst_max_rounds = 4096;
inline const char* subst_spec_fault(const emat_subst_spec& s, bool with_model = true) {
  if (with_model) {
    if (!finite_positive(s.mu)) return "mu must be finite and positive";
    if (!finite_positive(s.kappa)) return "kappa must be finite and positive";
    double sum = 0.0;
    for (int a = 0; a < 4; ++a) { if (!(s.pi[a] > 0.0 && s.pi[a] < 1.0)) return "every pi[a] must lie inside (0, 1)"; sum += s.pi[a]; }
    if (!(std::fabs(sum - 1.0) <= 1e-9)) return "the pi[a] must add up to 1 within 1e-9";
  }
  if (!std::isfinite(s.mu_prior_alpha)) return "mu_prior_alpha must be finite";
  if (!std::isfinite(s.mu_prior_beta)) return "mu_prior_beta must be finite";
  if (s.rounds < 0) return "rounds must not be negative";
  return nullptr;
}

// q of the HKY model (kappa, pi): Hky_model::derive_site_evo_model (reference evo_hky.cpp:7-50), statement for statement what the run
// driver's push_model has always sent -- the model a handle holds after the substitution-model moves is the one the next push sends.
inline void hky_derive_q(double kappa, const double pi[4], double q[16]) {
  const double k = kappa;
  double r[4][4] = {{0, 1, k, 1}, {1, 0, 1, k}, {k, 1, 0, 1}, {1, k, 1, 0}};
  double rowv[4]; for (int b = 0; b < 4; ++b) { rowv[b] = 0.0; for (int a = 0; a < 4; ++a) rowv[b] += pi[a] * r[a][b]; }
  double R = 0.0; for (int b = 0; b < 4; ++b) R += rowv[b] * pi[b];
  for (int a = 0; a < 4; ++a) { q[a * 4 + a] = 0.0; for (int b = 0; b < 4; ++b) if (a != b) { q[a * 4 + b] = r[a][b] / R * pi[b]; q[a * 4 + a] -= q[a * 4 + b]; } }
}

}  // namespace emat

#endif  // EMAT_MOVE_SPECS_HPP_
