// emat_move_specs.hpp -- what a global-move spec must satisfy before any model is looked at: one function per spec, the text of the first fault or nullptr.
//
// No HIP in here: the backend's entry points (emat_skygrid_host.hpp, emat_exp_pop_host.hpp, emat_subst_host.hpp, emat_mpox_host.hpp) and the run driver's setters (emat_run.cpp) both refuse
// with these texts.  Also what both derive alike: hky_derive_q, the q of an HKY model; mpox_derive_q and apobec_context_partition, the two q and the site partition of the APOBEC model.
#ifndef EMAT_MOVE_SPECS_HPP_
#define EMAT_MOVE_SPECS_HPP_

#include <cmath>
#include <string>
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

// THE sentence of a backend call asked for more rounds than its moves hold (EMAT_ERR_CAPACITY; the Exponential group's limit is its kernels' own, k_xp_max_rounds).
inline std::string rounds_beyond_text(int rounds, int max_rounds) { return std::to_string(rounds) + " rounds are more than the moves hold (" + std::to_string(max_rounds) + ")"; }

// The two groups that run as one wavefront, the substitution-model moves and the APOBEC model's: the rounds they hold, the run driver's setters' text for more, what their specs share.
constexpr int k_one_wave_max_rounds = 4096;
inline const char* rounds_limit_fault(int rounds) {
  static const std::string text = "rounds must not exceed " + std::to_string(k_one_wave_max_rounds);
  return rounds > k_one_wave_max_rounds ? text.c_str() : nullptr;
}
template <class Spec> inline const char* mu_prior_and_rounds_fault(const Spec& s) {
  if (!std::isfinite(s.mu_prior_alpha)) return "mu_prior_alpha must be finite";
  if (!std::isfinite(s.mu_prior_beta)) return "mu_prior_beta must be finite";
  if (s.rounds < 0) return "rounds must not be negative";
  return nullptr;
}

// The substitution-model moves (emat_subst_host.hpp; the run driver's setter, which brings its own model, passes with_model = false).
inline const char* subst_spec_fault(const emat_subst_spec& s, bool with_model = true) {
  if (with_model) {
    if (!finite_positive(s.mu)) return "mu must be finite and positive";
    if (!finite_positive(s.kappa)) return "kappa must be finite and positive";
    double sum = 0.0;
    for (int a = 0; a < 4; ++a) { if (!(s.pi[a] > 0.0 && s.pi[a] < 1.0)) return "every pi[a] must lie inside (0, 1)"; sum += s.pi[a]; }
    if (!(std::fabs(sum - 1.0) <= 1e-9)) return "the pi[a] must add up to 1 within 1e-9";
  }
  return mu_prior_and_rounds_fault(s);
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

// The APOBEC (mpox) model's moves (emat_mpox_host.hpp; the run driver's setter, which brings its own mu, passes with_model = false).
inline const char* mpox_spec_fault(const emat_mpox_spec& s, bool with_model = true) {
  if (with_model && !finite_positive(s.mu)) return "mu must be finite and positive";
  if (!(std::isfinite(s.mu_star) && s.mu_star >= 0.0)) return "mu_star must be finite and not negative";
  return mu_prior_and_rounds_fault(s);
}

// q of the APOBEC model's two site partitions (Run::derive_evo, reference run.cpp:407-432): Jukes-Cantor everywhere, and on the sites with
// APOBEC context (partition 1) the extra rate 2 rho of TC>TT and of GA>AA.  Letters: A, C, G, T = 0 .. 3.  pi is 0.25 and mu the same in both.
inline void mpox_derive_q(double rho, double q0[16], double q1[16]) {
  for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) q0[a * 4 + b] = (a == b) ? -1.0 : 1. / 3.;
  for (int k = 0; k < 16; ++k) q1[k] = q0[k];
  q1[1 * 4 + 3] += 2 * rho; q1[1 * 4 + 1] -= 2 * rho;
  q1[2 * 4 + 0] += 2 * rho; q1[2 * 4 + 2] -= 2 * rho;
}

// The site partition by APOBEC context of a sequence (Run::set_mpox_hack_enabled, reference run.cpp:370-382): site l is of partition 1 when
// it follows a T and holds C (not yet mutated) or T (already mutated), or precedes an A and holds G or A.  Returns how many are.
inline int apobec_context_partition(const uint8_t* seq, int L, int32_t* partition_for_site) {
  int count = 0;
  for (int l = 0; l != L; ++l) {
    const bool apobec_context = ((l != 0) && (seq[l - 1] == 3) && ((seq[l] == 1) || (seq[l] == 3))) ||
                                ((l + 1 != L) && (seq[l + 1] == 0) && ((seq[l] == 2) || (seq[l] == 0)));
    if (apobec_context) ++count;
    partition_for_site[l] = apobec_context ? 1 : 0;
  }
  return count;
}

}  // namespace emat

#endif  // EMAT_MOVE_SPECS_HPP_
