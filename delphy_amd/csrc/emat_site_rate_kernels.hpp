// emat_site_rate_kernels.hpp -- the site-rate moves on the device (reference core/run.cpp:1105-1235): the scaling Metropolis steps on
// the shape alpha of the site-rate prior, and the Gibbs draw of every site's relative rate nu_l that follows them.
//
// Inputs are the per-site sufficient statistics, already summed over every part of the run: Ttwiddle_l (calc_Ttwiddle_l) and M_l
// (calc_num_muts_l).  Three launches on the engine's stream, nothing in between returns to the host:
//   k_site_rate_alpha    one workgroup: log p(alpha) (calc_log_p_alpha, run.cpp:1157-1181) at the start and at every proposal, the steps
//                        themselves (:1193-1215) and the increment of the alpha prior from the OLD rates (:1218-1231)
//   k_site_rate_gibbs    one thread per site: nu_l ~ Gamma(M_l + alpha, mu_l Ttwiddle_l + alpha), floored at 1e-50 (:1114-1149)
//   k_site_rate_sums     one workgroup: the per-site increments of log G and of the nu prior added up (:1144-1151)
// Random numbers: streams named by (key, site), emat_gamma_pure.hpp.
// Sums: a thread adds the terms of its sites l = thread, thread + 1024, ... in ascending l, and a tree of fixed shape over LDS adds the
// 1 024 threads: the same bits from every launch and on every handle.  No atomics.
//
// Included by emat_backend.hip after the other kernel headers: everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_SITE_RATE_KERNELS_HPP_
#define EMAT_SITE_RATE_KERNELS_HPP_

#include "../../include/emat_backend.h"
#include "emat_gamma_pure.hpp"

namespace emat {

constexpr int k_sr_threads = 1024;          // of the two one-workgroup kernels
constexpr int k_sr_gibbs_threads = 256;
constexpr double k_sr_nu_floor = 1e-50;     // run.cpp:1140
constexpr double k_sr_mean_alpha = 1.0;     // exponential prior of alpha, run.cpp:1189
// What the alpha kernel leaves for the next two and for the host (doubles)
enum { k_sr_alpha = 0, k_sr_log_p_start, k_sr_num_accepted, k_sr_d_prior_alpha, k_sr_sum_nu_old, k_sr_sum_log_nu_old, k_sr_lgamma_before, k_sr_lgamma_after,
       k_sr_d_log_G, k_sr_d_prior_nu_sites, k_sr_sum_nu_old2, k_sr_sum_nu_new, k_sr_num_floored, k_sr_d_prior_nu, k_sr_result_doubles };

struct SiteRateArgs {
  int32_t L;
  const double* Ttwiddle_l;           // [L]
  const int32_t* num_muts_l;          // [L]
  const double* mu;                   // [P]
  const uint8_t* partition_for_site;  // [L]
  const double* nu_old;               // [L]
  double* nu_new;                     // [L]
  double* d_log_G_l;                  // [L] run.cpp:1144 per site
  double* d_prior_l;                  // [L] run.cpp:1148 per site
  double* result;                     // [k_sr_result_doubles]
  emat_site_rate_step* trace;         // [num_alpha_steps] or null
  double alpha;
  int32_t num_alpha_steps;
  uint64_t key;
};

// All 1 024 threads: the sum of every thread's `mine`, returned to every thread.  A fixed tree: 512 + 512, 256 + 256, ...
__device__ __forceinline__ double sr_block_sum(double mine, double* lds) {
  const int t = (int)threadIdx.x;
  lds[t] = mine;
  __syncthreads();
  for (int s = k_sr_threads / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  const double total = lds[0];
  __syncthreads();   // before the next use of `lds`
  return total;
}

// calc_log_p_alpha (run.cpp:1157-1181); `n_plus` = sites with mutations
__device__ __forceinline__ double sr_log_p_alpha(const SiteRateArgs& a, double alpha, double n_plus, double* lds) {
  double mine = 0.0;
  for (int l = (int)threadIdx.x; l < a.L; l += k_sr_threads) {
    const int M = a.num_muts_l[l];
    if (M > 0) mine += ::lgamma((double)M + alpha);
    mine -= ((double)M + alpha) * ::log(a.mu[a.partition_for_site[l]] * a.Ttwiddle_l[l] + alpha);
  }
  double result = sr_block_sum(mine, lds);
  result -= n_plus * ::lgamma(alpha) - (double)a.L * alpha * ::log(alpha);
  return result;
}

// Every thread runs the steps' scalar arithmetic on the same numbers (its own copy of the stream), so all agree on every decision
// without a broadcast; thread 0 writes.
__global__ __launch_bounds__(k_sr_threads) void k_site_rate_alpha(SiteRateArgs a) {
  __shared__ double lds[k_sr_threads];
  const int t = (int)threadIdx.x;
  double cnt = 0.0, s_nu = 0.0, s_log_nu = 0.0;
  for (int l = t; l < a.L; l += k_sr_threads) {
    if (a.num_muts_l[l] > 0) cnt += 1.0;
    const double nu = a.nu_old[l];
    s_nu += nu; s_log_nu += ::log(nu);
  }
  const double n_plus = sr_block_sum(cnt, lds);
  const double sum_nu = sr_block_sum(s_nu, lds), sum_log_nu = sr_block_sum(s_log_nu, lds);

  const double alpha_before = a.alpha;
  double alpha = a.alpha;
  double cur_log_p = sr_log_p_alpha(a, alpha, n_plus, lds);
  const double log_p_start = cur_log_p;
  SiteStream rs = site_stream(a.key, k_site_stream_alpha);
  int accepted_total = 0;
  for (int step = 0; step < a.num_alpha_steps; ++step) {   // run.cpp:1193-1215; block `step` of the stream: the scale, then the acceptance uniform
    const double scale_factor = 0.90;
    const double old_alpha = alpha;
    const double scale = scale_factor + (1.0 / scale_factor - scale_factor) * to_co(site_stream_next64(rs));
    const double u = to_co(site_stream_next64(rs));   // drawn whether needed or not: the stream's position depends on the step alone
    const double new_alpha = scale * old_alpha;
    const double n_to_o_over_o_to_n = old_alpha / new_alpha;
    const double log_prior_ratio = -(new_alpha - old_alpha) / k_sr_mean_alpha;
    const double new_log_p = sr_log_p_alpha(a, new_alpha, n_plus, lds);
    const double delta_log_posterior = log_prior_ratio + new_log_p - cur_log_p;
    const double log_metropolis = delta_log_posterior + ::log(n_to_o_over_o_to_n);
    const bool accept = log_metropolis > 0.0 || u < ::exp(log_metropolis);
    if (accept) { alpha = new_alpha; cur_log_p = new_log_p; ++accepted_total; }
    if (t == 0 && a.trace) {
      emat_site_rate_step r; r.proposed_alpha = new_alpha; r.log_p_proposed = new_log_p; r.log_metropolis = log_metropolis; r.u = u; r.accepted = accept ? 1 : 0; r.pad_ = 0;
      a.trace[step] = r;
    }
  }
  if (t == 0) {
    const double L = (double)a.L;
    const double lg_after = ::lgamma(alpha), lg_before = ::lgamma(alpha_before);
    const double d_prior = 0.0   // run.cpp:1226-1231
        + -(alpha - alpha_before) / k_sr_mean_alpha
        + L * (alpha * ::log(alpha) - alpha_before * ::log(alpha_before))
        - L * (lg_after - lg_before)
        + (alpha - alpha_before) * sum_log_nu
        - (alpha - alpha_before) * sum_nu;
    a.result[k_sr_alpha] = alpha; a.result[k_sr_log_p_start] = log_p_start; a.result[k_sr_num_accepted] = (double)accepted_total;
    a.result[k_sr_d_prior_alpha] = d_prior; a.result[k_sr_sum_nu_old] = sum_nu; a.result[k_sr_sum_log_nu_old] = sum_log_nu;
    a.result[k_sr_lgamma_before] = lg_before; a.result[k_sr_lgamma_after] = lg_after;
  }
}

// gibbs_sample_all_nus (run.cpp:1114-1149), one site per thread; alpha is what the steps left in result[k_sr_alpha]
__global__ __launch_bounds__(k_sr_gibbs_threads) void k_site_rate_gibbs(SiteRateArgs a) {
  const int l = (int)(blockIdx.x * (unsigned)k_sr_gibbs_threads + threadIdx.x);
  if (l >= a.L) return;
  const double alpha = a.result[k_sr_alpha];
  const int M = a.num_muts_l[l];
  const double mu_l = a.mu[a.partition_for_site[l]], T = a.Ttwiddle_l[l];
  SiteStream rs = site_stream(a.key, (uint32_t)l);
  const double drawn = gamma_draw((double)M + alpha, mu_l * T + alpha, rs);
  const double new_nu = drawn > k_sr_nu_floor ? drawn : k_sr_nu_floor;   // std::max(1e-50, draw)
  const double old_nu = a.nu_old[l];
  const double log_new_over_old = ::log(new_nu / old_nu);
  a.nu_new[l] = new_nu;
  a.d_log_G_l[l] = -mu_l * (new_nu - old_nu) * T + (double)M * log_new_over_old;
  a.d_prior_l[l] = (alpha - 1.0) * log_new_over_old;
}

__global__ __launch_bounds__(k_sr_threads) void k_site_rate_sums(SiteRateArgs a) {
  __shared__ double lds[k_sr_threads];
  double dG = 0.0, dP = 0.0, s_old = 0.0, s_new = 0.0, floored = 0.0;
  for (int l = (int)threadIdx.x; l < a.L; l += k_sr_threads) {
    dG += a.d_log_G_l[l]; dP += a.d_prior_l[l];
    s_old += a.nu_old[l];
    const double nu = a.nu_new[l];
    s_new += nu;
    if (nu == k_sr_nu_floor) floored += 1.0;
  }
  dG = sr_block_sum(dG, lds); dP = sr_block_sum(dP, lds); s_old = sr_block_sum(s_old, lds); s_new = sr_block_sum(s_new, lds); floored = sr_block_sum(floored, lds);
  if (threadIdx.x == 0) {
    const double alpha = a.result[k_sr_alpha];
    a.result[k_sr_d_log_G] = dG; a.result[k_sr_d_prior_nu_sites] = dP; a.result[k_sr_sum_nu_old2] = s_old; a.result[k_sr_sum_nu_new] = s_new; a.result[k_sr_num_floored] = floored;
    a.result[k_sr_d_prior_nu] = dP + -alpha * (s_new - s_old);   // run.cpp:1148 summed, then :1151
  }
}

// test hook (emat_debug_sample_gamma): draw i from the stream (key, i)
__global__ void k_debug_sample_gamma(uint64_t key, int32_t n, double shape, double rate, double* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  SiteStream rs = site_stream(key, (uint32_t)i);
  out[i] = gamma_draw(shape, rate, rs);
}

}  // namespace emat
#endif  // EMAT_SITE_RATE_KERNELS_HPP_
