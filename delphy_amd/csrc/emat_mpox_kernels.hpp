// emat_mpox_kernels.hpp -- the APOBEC (mpox) model's moves on the device (reference core/run.cpp:703-719, the arm taken with the mpox model on):
// Run::mpox_hack_moves (:823-951), `rounds` rounds of an exact Gibbs draw of mu and of rho = mu* / mu through a truncated Gamma.
//
// Inputs are the statistics of the whole run in the record of the substitution-model moves (emat_subst_kernels.hpp: k_sb_T, k_sb_M; the root
// counts are not read), for the model's 2 site partitions.  The record comes from the caller, or from the parts on the handle without leaving HBM
// (k_subst_reduce_stats).
//   k_mpox_moves   ONE workgroup of one wavefront: the sums M, M*, Ttwiddle, Ttwiddle* (:854-905) and the whole chain of rounds (:908-947), statement
//                  for statement.  Every lane runs the same scalar arithmetic on the same numbers (its own copy of the streams), so all agree on
//                  every decision without a broadcast; lane 0 writes the trace and the result.  No atomics: the same bits from every launch.
// Random numbers: the (key, id) streams of emat_gamma_pure.hpp under two pseudo-ids, the next below the substitution-model moves': k_mx_stream_mu,
// round i's mu draw from word 256 i; k_mx_stream_rho, round i's uniform the word i.
//
// Included by emat_backend.hip after emat_subst_kernels.hpp (the record's layout; dev::gamma_q and dev::gamma_q_inv come with emat_part_kernels.hpp):
// everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_MPOX_KERNELS_HPP_
#define EMAT_MPOX_KERNELS_HPP_

#include "../../include/emat_backend.h"
#include "emat_gamma_pure.hpp"

namespace emat {

constexpr int k_mx_threads = 64;                    // k_mpox_moves: one wavefront
constexpr uint32_t k_mx_stream_mu = 0xFFFFFFF6u;    // the mu draws (Marsaglia-Tsang): round i from word k_mx_mu_words i
constexpr uint32_t k_mx_stream_rho = 0xFFFFFFF5u;   // to_oc: round i = word i
constexpr uint32_t k_mx_mu_words = 256;             // (a draw takes at most 3 k_gamma_max_rounds + 1 = 193 words)
// What k_mpox_moves leaves for the host (doubles)
enum { k_mx_mu = 0, k_mx_mu_star, k_mx_M, k_mx_M_star, k_mx_T, k_mx_T_star, k_mx_d_log_G, k_mx_d_other_priors, k_mx_rho_skipped, k_mx_rho_degenerate,
       k_mx_bad_posterior, k_mx_shape, k_mx_rate, k_mx_result_doubles };

struct MpoxArgs {
  emat_mpox_spec spec;
  const double* stats;                // [k_sb_stats_doubles], 2 site partitions
  uint64_t key;
  emat_mpox_round* trace;             // null, or [rounds]
  double* result;                     // [k_mx_result_doubles]
};

__global__ __launch_bounds__(k_mx_threads) void k_mpox_moves(MpoxArgs a) {
  const int lane = (int)threadIdx.x;
  const emat_mpox_spec& sp = a.spec;
  const double* T = a.stats + k_sb_T; const double* Mc = a.stats + k_sb_M;
  // run.cpp:854-866 (counts as doubles: integers below 2^53, exact in any order), :897-905
  double M = 0.0;
  for (int beta = 0; beta < 2; ++beta) for (int k = 0; k < 16; ++k) if ((k >> 2) != (k & 3)) M += Mc[16 * beta + k];
  const double M_star = Mc[16 + 4 * 1 + 3] + Mc[16 + 4 * 2 + 0];
  double Ttwiddle = 0.0;
  for (int beta = 0; beta < 2; ++beta) for (int s = 0; s < 4; ++s) Ttwiddle += T[4 * beta + s];
  const double Ttwiddle_star = T[4 + 1] + T[4 + 2];

  double mu = sp.mu, mu_star = sp.mu_star;
  double d_log_G = 0.0, d_other = 0.0, n_skipped = 0.0, n_degenerate = 0.0;
  for (int i = 0; i < sp.rounds; ++i) {
    emat_mpox_round r;
    const double rho = mu_star / mu;
    const double Ttwiddle_eff = Ttwiddle + 2 * rho * Ttwiddle_star;
    r.mu = mu; r.rho = rho; r.Ttwiddle_eff = Ttwiddle_eff;

    // ---- mu (:915-927)
    const double shape = M + sp.mu_prior_alpha - 1.0, rate = Ttwiddle_eff + sp.mu_prior_beta;
    const bool drawable = shape > 0.0 && rate > 0.0;   // (a NaN is not)
    double draw = __builtin_nan("");
    if (drawable) { SiteStream rs = site_stream(a.key, k_mx_stream_mu); rs.word = k_mx_mu_words * (uint32_t)i; draw = gamma_draw(shape, rate, rs); }
    if (sp.do_mu != 0 && !drawable) {   // the host refuses round 0's before the launch where it has the statistics; a later round's, or the parts', it learns of here
      if (lane == 0) { for (int j = 0; j < k_mx_result_doubles; ++j) a.result[j] = 0.0; a.result[k_mx_shape] = shape; a.result[k_mx_rate] = rate; a.result[k_mx_bad_posterior] = 1.0; }
      return;
    }
    r.mu_shape = shape; r.mu_rate = rate; r.mu_draw = draw;
    r.mu_delta_log_G = 0.0; r.mu_delta_log_other_priors = 0.0; r.mu_done = 0;
    if (sp.do_mu != 0) {
      const double old_mu = mu, new_mu = draw;
      mu = new_mu;
      r.mu_delta_log_G = -(new_mu - old_mu) * Ttwiddle_eff + M * ::log(new_mu / old_mu);
      r.mu_delta_log_other_priors = (sp.mu_prior_alpha - 1) * ::log(new_mu / old_mu) - sp.mu_prior_beta * (new_mu - old_mu);
      d_log_G += r.mu_delta_log_G; d_other += r.mu_delta_log_other_priors;
      r.mu_done = 1;
    }

    // ---- rho (:930-946), k = 1 + 6 rho by safe_sample_truncated_gamma(M* + 1, mu Ttwiddle* / 3, 1, inf) (safe_gamma_math.h:110-139)
    r.alpha = 0.0; r.beta = 0.0; r.Q_lo = 0.0; r.Q_hi = 0.0; r.u = 0.0; r.rand_Q = 0.0; r.y = 0.0; r.k = 0.0; r.new_rho = 0.0; r.rho_delta_log_G = 0.0;
    r.rho_done = 0; r.rho_degenerate = 0; r.reserved = 0;
    if (Ttwiddle_star > 0.0) {
      const double alpha = M_star + 1, beta = mu * Ttwiddle_star / 3;
      SiteStream rs = site_stream(a.key, k_mx_stream_rho); rs.word = (uint32_t)i & ~1u;   // (a stream is entered at a block's first word: the second comes out of the first's spare)
      uint64_t word = site_stream_next64(rs);
      if (i & 1) word = site_stream_next64(rs);
      const double u = to_oc(word);
      const double y_lo = beta * 1.0;
      const double Q_hi = dev::gamma_q(alpha, y_lo), Q_lo = 0.0;   // (y_hi = inf: Q = 0)
      r.alpha = alpha; r.beta = beta; r.Q_lo = Q_lo; r.Q_hi = Q_hi; r.u = u;
      if (!(beta > 0.0) || !(Q_lo < Q_hi)) { r.rho_degenerate = 1; n_degenerate += 1.0; }   // (the reference's CHECK_GT / CHECK_LT: rho stays)
      else {
        const double rand_Q = Q_lo + (Q_hi - Q_lo) * u;
        const double y = dev::gamma_q_inv(alpha, rand_Q);
        double k = y / beta;
        k = k < 1.0 ? 1.0 : k;   // std::clamp(x, lo, hi) with hi = inf
        const double old_rho = rho, new_rho = (k - 1) / 6.0;
        mu_star = mu * new_rho;
        r.rho_delta_log_G = -2 * mu * (new_rho - old_rho) * Ttwiddle_star + M_star * ::log((1 + 6 * new_rho) / (1 + 6 * old_rho));
        d_log_G += r.rho_delta_log_G;
        r.rand_Q = rand_Q; r.y = y; r.k = k; r.new_rho = new_rho; r.rho_done = 1;
      }
    } else n_skipped += 1.0;
    if (a.trace && lane == 0) a.trace[i] = r;
  }
  if (lane == 0) {
    double* o = a.result;
    o[k_mx_mu] = mu; o[k_mx_mu_star] = mu_star; o[k_mx_M] = M; o[k_mx_M_star] = M_star; o[k_mx_T] = Ttwiddle; o[k_mx_T_star] = Ttwiddle_star;
    o[k_mx_d_log_G] = d_log_G; o[k_mx_d_other_priors] = d_other; o[k_mx_rho_skipped] = n_skipped; o[k_mx_rho_degenerate] = n_degenerate;
    o[k_mx_bad_posterior] = 0.0; o[k_mx_shape] = 0.0; o[k_mx_rate] = 0.0;
  }
}

}  // namespace emat
#endif  // EMAT_MPOX_KERNELS_HPP_
