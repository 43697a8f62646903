// emat_skygrid_kernels.hpp -- the Skygrid population moves on the device (reference core/run.cpp:766-778): skygrid_tau_move (:1321-1358),
// skygrid_gammas_zero_mode_gibbs_move (:2016-2189) and skygrid_gammas_hmc_move (:1360-2014), in that order, in ONE launch of ONE workgroup.
//
// Inputs are the statistics of the whole run: the lineage grid k_bar[c] of Scalable_coalescent_prior (scalable_coalescent.cpp:88-138) over
// cells [t_ref + j t_step, t_ref + (j + 1) t_step), j = first_cell .. first_cell + num_cells - 1, and the times of the inner nodes.
//   k_skygrid_node_stats   one workgroup per knot k scanning every inner time: c_k, the inner nodes whose clamped knot interval is k
//                          (run.cpp:1695-1702), and W_k = sum_i d log N(t_i) / d gamma_k.  log N(t) is linear in the gammas for both Skygrid
//                          types, so sum_i log N(t_i) = sum_k W_k gamma_k and the inner nodes' part of the force on knot k is -W_k for the whole
//                          trajectory: the nodes are read once, not at each of the 25 force and 3 prior evaluations (the reference's own
//                          TODO, run.cpp:1667-1674).  Both depend on the knot TIMES only.
//   k_skygrid_moves        one workgroup of 1 024 threads.  Thread k owns knot k (its p_k, m_k, W_k, c_k in registers; gamma in LDS, where
//                          every thread reads it through the population model's routines).  The cell averages popsize_bar[c] =
//                          pop_integral(cell) / t_step, 1e-100 where that is 0 (scalable_coalescent.cpp:150-154), go to a device scratch array,
//                          cells strided over the threads.  The coalescent force on knot k is summed by a group of G lanes of one wavefront,
//                          G = the largest power of two <= min(64, 1024 / knots): lane j of the group adds the cells c_min + j, c_min + j + G,
//                          ... of support_of_d_log_N_d_gamma(k) in ascending order, and a butterfly of fixed shape adds the lanes.
// Sums over cells and knots: a thread adds its terms (index = thread, thread + 1024, ...) in ascending order and a tree of fixed shape over
// LDS adds the threads (sr_block_sum).  No atomics: the same bits from every launch and on every handle.
// Every scalar decision (a move accepted, the K > 100 (M + 1) exit, a NaN) is taken by every thread from the same numbers: block sums that
// all threads read from one LDS word, and draws that every thread makes from its own copy of the same stream.  Every loop is bounded by
// an argument; nothing waits on memory another workgroup writes.
// Random numbers: the (key, id) streams of emat_gamma_pure.hpp.  Knot k's momentum is sqrt(m_k) x site_stream_normal of stream (key, k);
// the five scalar draws have pseudo-ids at the top of the id range (k_sky_stream_*), each the first draw(s) of its stream, and all are
// drawn whether needed or not.
//
// Included by emat_backend.hip after emat_gtree_kernels.hpp (GTreeDev) and emat_site_rate_kernels.hpp (sr_block_sum): everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_SKYGRID_KERNELS_HPP_
#define EMAT_SKYGRID_KERNELS_HPP_

#include "../../include/emat_backend.h"
#include "emat_gamma_pure.hpp"

namespace emat {

constexpr int k_sky_threads = k_sr_threads;         // 1 024: sr_block_sum's shape
constexpr int k_sky_max_knots = 1024;               // one thread per knot
constexpr int k_sky_max_cells = 1 << 22;
constexpr uint32_t k_sky_stream_tau = 0xFFFFFFFEu;      // gamma_draw: the new tau
constexpr uint32_t k_sky_stream_I_bar = 0xFFFFFFFDu;    // gamma_draw: the zero mode's I_bar
constexpr uint32_t k_sky_stream_zero_u = 0xFFFFFFFCu;   // to_co: the zero mode's acceptance uniform
constexpr uint32_t k_sky_stream_dt = 0xFFFFFFFBu;       // to_oc: dt = -mean log(u)
constexpr uint32_t k_sky_stream_hmc_u = 0xFFFFFFFAu;    // to_co: the HMC's acceptance uniform
// What k_skygrid_moves leaves for the host (doubles), in emat_skygrid_result's order
enum { k_sky_tau = 0, k_sky_log_prior_start, k_sky_log_prior_end, k_sky_d_other_priors,
       k_sky_tau_post_alpha, k_sky_tau_post_beta, k_sky_tau_draw, k_sky_tau_d_prior,
       k_sky_zm_B, k_sky_zm_shape, k_sky_zm_rate, k_sky_zm_I_bar, k_sky_zm_d_gamma_bar, k_sky_zm_log_metropolis, k_sky_zm_u, k_sky_zm_accepted,
       k_sky_hmc_dt, k_sky_hmc_K_old, k_sky_hmc_K_new, k_sky_hmc_U_prior_old, k_sky_hmc_U_prior_new, k_sky_hmc_U_coal_old, k_sky_hmc_U_coal_new,
       k_sky_hmc_log_metropolis, k_sky_hmc_u, k_sky_hmc_accepted, k_sky_hmc_K_exit_step, k_sky_hmc_nan, k_sky_hmc_steps_done, k_sky_result_doubles };
constexpr int k_sky_trace_head_rows = 5, k_sky_trace_step_rows = 4;   // emat_skygrid_result::trace

struct SkygridArgs {
  int32_t type, num_knots;            // skygrid_type (1 staircase, 2 log-linear)
  const double* x;                    // [num_knots] knot times
  const double* gamma_in;             // [num_knots]
  double inv_dx;                      // PopTable::skygrid_inv_dx
  double t_ref, t_step;
  int32_t first_cell, num_cells;
  const double* k_bar;                // [num_cells]
  double* popsize_bar;                // [num_cells] scratch
  int32_t num_inner;
  const double* inner_t;              // [num_inner]
  double* c_k; double* W_k;           // [num_knots] k_skygrid_node_stats -> k_skygrid_moves
  emat_skygrid_spec spec;
  uint64_t key;
  double* gamma_out;                  // [num_knots]
  double* result;                     // [k_sky_result_doubles]
  double* trace; int32_t trace_steps; // null, or [k_sky_trace_head_rows + k_sky_trace_step_rows * trace_steps][num_knots]
};

__device__ __forceinline__ PopTable sky_pop_table(const SkygridArgs& a, const double* x, const double* gamma) {
  PopTable pt{};
  pt.kind = 2; pt.skygrid_type = a.type; pt.skygrid_num_knots = a.num_knots; pt.skygrid_inv_dx = a.inv_dx;
  pt.skygrid_x = x; pt.skygrid_gamma = gamma; pt.skygrid_x0 = a.num_knots > 0 ? x[0] : 0.0;
  return pt;
}

// One workgroup per knot; gamma is not read.
__global__ __launch_bounds__(k_sky_threads) void k_skygrid_node_stats(SkygridArgs a) {
  __shared__ double lds[k_sky_threads];
  const int k = (int)blockIdx.x, M = a.num_knots - 1;
  const PopTable pt = sky_pop_table(a, a.x, a.x);
  double cnt = 0.0, w = 0.0;
  for (int i = (int)threadIdx.x; i < a.num_inner; i += k_sky_threads) {
    const double t = a.inner_t[i];
    int kk = dev::skygrid_interval(pt, t);
    kk = kk > M ? M : kk;                               // std::clamp(interval_containing_t(t), 0, M)
    if (kk == k) cnt += 1.0;
    w += dev::skygrid_d_log_N_d_gamma(pt, t, k);
  }
  cnt = sr_block_sum(cnt, lds); w = sr_block_sum(w, lds);
  if (threadIdx.x == 0) { a.c_k[k] = cnt; a.W_k[k] = w; }
}

// popsize_bars of every cell under the gammas in LDS (Scalable_coalescent_prior::pop_model_changed); ends on a barrier.
__device__ __forceinline__ void sky_update_popsize_bars(const SkygridArgs& a, const PopTable& pt) {
  for (int c = (int)threadIdx.x; c < a.num_cells; c += k_sky_threads) {
    const double lb = a.t_ref + (double)(a.first_cell + c) * a.t_step, ub = lb + a.t_step;
    double v = dev::pop_integral(pt, lb, ub) / a.t_step;
    if (v == 0.0) v = 1e-100;
    a.popsize_bar[c] = v;
  }
  __syncthreads();
}
// calc_log_prior (scalable_coalescent.cpp:163-187) with the inner nodes' sum as sum_k W_k gamma_k
__device__ __forceinline__ double sky_log_coalescent_prior(const SkygridArgs& a, double W, double gamma_mine, double* lds) {
  double cells = 0.0;
  for (int c = (int)threadIdx.x; c < a.num_cells; c += k_sky_threads) {
    const double kbar = a.k_bar[c];
    cells -= a.t_step * kbar * (kbar - 1) / (2.0 * a.popsize_bar[c]);
  }
  const double nodes = sr_block_sum((int)threadIdx.x < a.num_knots ? W * gamma_mine : 0.0, lds);
  return sr_block_sum(cells, lds) - nodes;
}
// calc_U_prior_from_gamma_k_s (run.cpp:1723-1753)
__device__ __forceinline__ double sky_U_prior(const SkygridArgs& a, const double* gamma, double tau, double* lds) {
  const int k = (int)threadIdx.x, M = a.num_knots - 1;
  const emat_skygrid_spec& s = a.spec;
  double d2 = 0.0, bar = 0.0, g = 0.0;
  if (k <= M) {
    g = gamma[k];
    if (k >= 1) { const double d = g - gamma[k - 1]; d2 = d * d; }
    if (s.low_gamma_barrier_enabled && g < s.low_gamma_barrier_loc) { const double e = (s.low_gamma_barrier_loc - g) / s.low_gamma_barrier_scale; bar = e * e; }
  }
  double U = sr_block_sum(d2, lds);
  U *= 0.5 * tau;
  U += sr_block_sum(bar, lds);
  const double gamma_bar = sr_block_sum(k <= M ? g : 0.0, lds) / (double)(M + 1);
  U += s.inv_nbar_prior_alpha * gamma_bar + s.inv_nbar_prior_beta * ::exp(-gamma_bar);
  return U;
}
// the low-gamma barrier's part of the log prior (run.cpp:2132-2143), 0 with the barrier off
__device__ __forceinline__ double sky_log_prior_bound(const SkygridArgs& a, double g, double* lds) {
  const emat_skygrid_spec& s = a.spec;
  double mine = 0.0;
  if ((int)threadIdx.x < a.num_knots && s.low_gamma_barrier_enabled && g < s.low_gamma_barrier_loc) { const double e = (s.low_gamma_barrier_loc - g) / s.low_gamma_barrier_scale; mine = e * e; }
  return -sr_block_sum(mine, lds);
}
// The cell of time t relative to the grid's first, clamped to [0, C - 1] (run.cpp:1788-1789 after Scalable_coalescent_prior::cell_for)
__device__ __forceinline__ int sky_clamped_cell(const SkygridArgs& a, double t) {
  const double c = ::floor((t - a.t_ref) / a.t_step) - (double)a.first_cell;
  return c > 0.0 ? (c < (double)(a.num_cells - 1) ? (int)c : a.num_cells - 1) : 0;   // NaN -> 0
}
// calc_f_k_s_from_gamma_k_s (run.cpp:1775-1843): the cells' sums by lane groups into f_lds, the rest by the knot's thread; returns f_k.
__device__ __forceinline__ double sky_force(const SkygridArgs& a, const PopTable& pt, const double* x, const double* gamma, int group_lanes, double tau, double W,
                                            double* f_lds, double* lds) {
  const int t = (int)threadIdx.x, M = a.num_knots - 1, C = a.num_cells;
  const emat_skygrid_spec& s = a.spec;
  {
    const int k = t / group_lanes, j = t % group_lanes;
    double mine = 0.0;
    if (k <= M) {
      const double t_min_coal = a.t_ref + (double)a.first_cell * a.t_step, t_max_coal = a.t_ref + (double)(a.first_cell + C) * a.t_step;
      const double t_min = k == 0 ? -dev::k_inf : x[k - 1];                                   // support_of_d_log_N_d_gamma (pop_model.cpp:227-245)
      const double t_max = k == M ? dev::k_inf : (a.type == 1 ? x[k] : x[k + 1]);
      const int c_min = t_min < t_min_coal ? 0 : sky_clamped_cell(a, t_min);
      const int c_max = t_max > t_max_coal ? C - 1 : sky_clamped_cell(a, t_max);
      for (int c = c_min + j; c <= c_max; c += group_lanes) {
        const double lb = a.t_ref + (double)(a.first_cell + c) * a.t_step, ub = lb + a.t_step;
        const double kc = a.k_bar[c];
        mine += 0.5 * a.t_step * kc * (kc - 1.0) / a.popsize_bar[c] * dev::skygrid_d_log_int_N_d_gamma(pt, lb, ub, k);
      }
    }
    for (int w = group_lanes >> 1; w > 0; w >>= 1) mine = mine + __shfl_xor(mine, w, 64);   // group_lanes <= 64 and a power of two: groups never straddle a wavefront
    if (k <= M && j == 0) f_lds[k] = mine;
  }
  __syncthreads();
  double f = 0.0, g = 0.0;
  if (t <= M) {
    g = gamma[t];
    f = f_lds[t];
    f -= W;
    if (t > 0) f -= tau * (g - gamma[t - 1]);
    if (t < M) f -= tau * (g - gamma[t + 1]);
    if (s.low_gamma_barrier_enabled && g < s.low_gamma_barrier_loc) {
      const double excess = s.low_gamma_barrier_loc - g;
      f += 2 * excess / (s.low_gamma_barrier_scale * s.low_gamma_barrier_scale);
    }
  }
  const double gamma_bar = sr_block_sum(t <= M ? g : 0.0, lds) / (double)(M + 1);
  const double f_invgamma = (-s.inv_nbar_prior_alpha + s.inv_nbar_prior_beta * ::exp(-gamma_bar)) / (double)(M + 1);
  return f + f_invgamma;
}

__global__ __launch_bounds__(k_sky_threads) void k_skygrid_moves(SkygridArgs a) {
  __shared__ double lds[k_sky_threads];
  __shared__ double s_gamma[k_sky_max_knots];
  __shared__ double s_x[k_sky_max_knots];
  __shared__ double s_f[k_sky_max_knots];
  const int t = (int)threadIdx.x, n = a.num_knots, M = n - 1;
  const bool mine = t < n;
  const emat_skygrid_spec& s = a.spec;
  if (mine) { s_gamma[t] = a.gamma_in[t]; s_x[t] = a.x[t]; }
  __syncthreads();
  const PopTable pt = sky_pop_table(a, s_x, s_gamma);
  const double W = mine ? a.W_k[t] : 0.0, c_k = mine ? a.c_k[t] : 0.0;
  double* res = a.result;

  sky_update_popsize_bars(a, pt);
  double log_prior = sky_log_coalescent_prior(a, W, mine ? s_gamma[t] : 0.0, lds);
  double d_other = 0.0;
  double tau = s.tau;
  if (t == 0) res[k_sky_log_prior_start] = log_prior;

  // ---- skygrid_tau_move (run.cpp:1321-1358) ----
  {
    double d2 = 0.0;
    if (mine && t >= 1) { const double d = s_gamma[t] - s_gamma[t - 1]; d2 = d * d; }
    const double sum_sq = sr_block_sum(d2, lds);
    const double post_alpha = s.tau_prior_alpha + 0.5 * (double)M, post_beta = s.tau_prior_beta + 0.5 * sum_sq;
    SiteStream rs = site_stream(a.key, k_sky_stream_tau);
    const double draw = gamma_draw(post_alpha, post_beta, rs);
    double d_prior = 0.0;
    if (s.do_tau && s.tau_move_enabled) {
      d_prior = (post_alpha - 1) * ::log(draw / tau) - post_beta * (draw - tau);
      tau = draw;
      d_other += d_prior;
    }
    if (t == 0) { res[k_sky_tau_post_alpha] = post_alpha; res[k_sky_tau_post_beta] = post_beta; res[k_sky_tau_draw] = draw; res[k_sky_tau_d_prior] = d_prior; }
  }

  // ---- skygrid_gammas_zero_mode_gibbs_move (run.cpp:2016-2189) ----
  {
    const double g_old = mine ? s_gamma[t] : 0.0;
    const double gamma_bar = sr_block_sum(g_old, lds) / (double)(M + 1);
    const double I_bar = ::exp(-gamma_bar);
    double B = 0.0;
    for (int c = t; c < a.num_cells; c += k_sky_threads) { const double kc = a.k_bar[c]; B += 0.5 * a.t_step * kc * (kc - 1.0) / a.popsize_bar[c]; }
    B = sr_block_sum(B, lds);
    B /= I_bar;
    const double shape = (double)a.num_inner + s.inv_nbar_prior_alpha, rate = B + s.inv_nbar_prior_beta;
    SiteStream rs = site_stream(a.key, k_sky_stream_I_bar);
    const double new_I_bar = gamma_draw(shape, rate, rs);
    SiteStream ru = site_stream(a.key, k_sky_stream_zero_u);
    const double u = to_co(site_stream_next64(ru));
    const double delta_gamma_bar = ::log(I_bar / new_I_bar);
    const double g_new = g_old + delta_gamma_bar;
    const double old_bound = sky_log_prior_bound(a, g_old, lds), new_bound = sky_log_prior_bound(a, g_new, lds);
    const double log_metropolis = new_bound - old_bound;
    const bool blew_up = sr_block_sum(mine && g_new != g_new ? 1.0 : 0.0, lds) > 0.0 || log_metropolis != log_metropolis;
    const bool accept = s.do_zero_mode && !blew_up && (log_metropolis >= 0 || u < ::exp(log_metropolis));
    if (accept) {
      const double new_gamma_bar = sr_block_sum(mine ? g_new : 0.0, lds) / (double)(M + 1);   // (every thread has read s_gamma[t] by now)
      if (mine) s_gamma[t] = g_new;
      __syncthreads();
      sky_update_popsize_bars(a, pt);
      log_prior = sky_log_coalescent_prior(a, W, g_new, lds);
      const double old_inv_nbar_prior = -s.inv_nbar_prior_alpha * gamma_bar - s.inv_nbar_prior_beta * ::exp(-gamma_bar);
      const double new_inv_nbar_prior = -s.inv_nbar_prior_alpha * new_gamma_bar - s.inv_nbar_prior_beta * ::exp(-new_gamma_bar);
      d_other += (new_inv_nbar_prior - old_inv_nbar_prior) + (new_bound - old_bound);
    }
    if (t == 0) {
      res[k_sky_zm_B] = B; res[k_sky_zm_shape] = shape; res[k_sky_zm_rate] = rate; res[k_sky_zm_I_bar] = new_I_bar; res[k_sky_zm_d_gamma_bar] = delta_gamma_bar;
      res[k_sky_zm_log_metropolis] = log_metropolis; res[k_sky_zm_u] = u; res[k_sky_zm_accepted] = accept ? 1.0 : 0.0;
    }
  }

  // ---- skygrid_gammas_hmc_move (run.cpp:1676-2014) ----
  {
    const double g_start = mine ? s_gamma[t] : 0.0;
    const double m_k = (t > 0 ? tau : 0.0) + (t < M ? tau : 0.0) + c_k;   // run.cpp:1708
    const double inv_m = 1.0 / m_k;
    SiteStream rp = site_stream(a.key, (uint32_t)t);
    double p = mine ? ::sqrt(m_k) * site_stream_normal(rp) : 0.0;
    SiteStream rd = site_stream(a.key, k_sky_stream_dt);
    const double dt = -s.hmc_mean_dt * ::log(to_oc(site_stream_next64(rd)));
    SiteStream ru = site_stream(a.key, k_sky_stream_hmc_u);
    const double u = to_co(site_stream_next64(ru));
    int group_lanes = 64;
    while (group_lanes * n > k_sky_threads) group_lanes >>= 1;
    double* tr = a.trace;
    if (tr && mine) { tr[t] = c_k; tr[n + t] = W; tr[2 * n + t] = m_k; tr[3 * n + t] = g_start; tr[4 * n + t] = p; }

    const double K_limit = 100.0 * (double)(M + 1);
    const double old_K = sr_block_sum(mine ? 0.5 * (p * p) * inv_m : 0.0, lds);
    const double old_U_prior = sky_U_prior(a, s_gamma, tau, lds);
    const double old_U_coal = -log_prior;
    const double old_H = old_K + old_U_prior + old_U_coal;
    double new_K = old_K, new_U_prior = old_U_prior, new_U_coal = old_U_coal, log_metropolis = 0.0;
    int exit_step = -1, steps_done = 0;
    bool nan_end = false, accept = false;
    if (s.do_hmc) {
      if (old_K > K_limit) exit_step = 0;
      for (int step = 0; exit_step < 0 && step < s.hmc_steps; ++step) {
        double g = mine ? s_gamma[t] : 0.0;
        g += 0.5 * dt * p * inv_m;
        if (mine) s_gamma[t] = g;
        __syncthreads();
        sky_update_popsize_bars(a, pt);
        const double f = sky_force(a, pt, s_x, s_gamma, group_lanes, tau, W, s_f, lds);
        if (mine) p += dt * f;
        const double K = sr_block_sum(mine ? 0.5 * (p * p) * inv_m : 0.0, lds);
        double* row = tr && step < a.trace_steps ? tr + (size_t)(k_sky_trace_head_rows + k_sky_trace_step_rows * step) * n : nullptr;
        if (row && mine) { row[t] = g; row[n + t] = f; row[2 * n + t] = p; row[3 * n + t] = g; }
        steps_done = step + 1;
        if (K > K_limit) { exit_step = step + 1; break; }
        g += 0.5 * dt * p * inv_m;
        if (mine) s_gamma[t] = g;
        if (row && mine) row[3 * n + t] = g;
        __syncthreads();
      }
      if (exit_step < 0) {
        sky_update_popsize_bars(a, pt);
        const double g = mine ? s_gamma[t] : 0.0;
        new_K = sr_block_sum(mine ? 0.5 * (p * p) * inv_m : 0.0, lds);
        new_U_prior = sky_U_prior(a, s_gamma, tau, lds);
        const double new_log_prior = sky_log_coalescent_prior(a, W, g, lds);
        new_U_coal = -new_log_prior;
        const double new_H = new_K + new_U_prior + new_U_coal;
        log_metropolis = old_H - new_H;
        nan_end = sr_block_sum(mine && g != g ? 1.0 : 0.0, lds) > 0.0 || log_metropolis != log_metropolis;
        accept = !nan_end && (log_metropolis > 0 || u < ::exp(log_metropolis));
        if (accept) { log_prior = new_log_prior; d_other += (-new_U_prior) - (-old_U_prior); }
      }
    }
    if (!accept && mine) s_gamma[t] = g_start;
    if (t == 0) {
      res[k_sky_hmc_dt] = dt; res[k_sky_hmc_K_old] = old_K; res[k_sky_hmc_K_new] = new_K; res[k_sky_hmc_U_prior_old] = old_U_prior; res[k_sky_hmc_U_prior_new] = new_U_prior;
      res[k_sky_hmc_U_coal_old] = old_U_coal; res[k_sky_hmc_U_coal_new] = new_U_coal; res[k_sky_hmc_log_metropolis] = log_metropolis; res[k_sky_hmc_u] = u;
      res[k_sky_hmc_accepted] = accept ? 1.0 : 0.0; res[k_sky_hmc_K_exit_step] = (double)exit_step; res[k_sky_hmc_nan] = nan_end ? 1.0 : 0.0; res[k_sky_hmc_steps_done] = (double)steps_done;
    }
  }
  if (mine) a.gamma_out[t] = s_gamma[t];
  if (t == 0) { res[k_sky_tau] = tau; res[k_sky_log_prior_end] = log_prior; res[k_sky_d_other_priors] = d_other; }
}

// ---- the whole-tree statistics from the tree resident in HBM (emat_tree_coalescent_stats) ----------------------------------------
// Scalable_coalescent_prior's grid of the tree as it stands (scalable_coalescent.cpp:88-138): every branch adds one lineage from its parent's
// time to its own, and one lineage runs from the lower bound of the root's cell to the root.  No atomics: cell c is ONE workgroup, thread j
// adds the branches of nodes j, j + 1 024, ... in ascending order (each branch's share of the cell formed as add_interval forms it) and
// sr_block_sum's fixed tree adds the threads.  400 cells x 200 000 nodes is 8e7 branch tests, all from L2.
// out[0] = the root's time, out[1] = the latest tip's (a maximum: order does not matter)
__global__ __launch_bounds__(k_sky_threads) void k_skygrid_tree_extent(GTreeDev g, double* out) {
  __shared__ double lds[k_sky_threads];
  const int t = (int)threadIdx.x;
  double m = -dev::k_inf;
  for (int v = t; v < g.n_nodes; v += k_sky_threads) if (g.c0[v] < 0) { const double tv = g.t[v]; m = tv > m ? tv : m; }
  lds[t] = m;
  __syncthreads();
  for (int s = k_sky_threads / 2; s > 0; s >>= 1) { if (t < s) lds[t] = lds[t] > lds[t + s] ? lds[t] : lds[t + s]; __syncthreads(); }
  if (t == 0) { out[0] = g.t[*g.root]; out[1] = lds[0]; }
}
__device__ __forceinline__ int sky_cell_of(double t, double t_ref, double t_step, int lo, int hi) {   // cell_for, clamped to the grid
  const double c = ::floor((t - t_ref) / t_step);
  return c > (double)lo ? (c < (double)hi ? (int)c : hi) : lo;
}
__global__ __launch_bounds__(k_sky_threads) void k_skygrid_tree_k_bar(GTreeDev g, double t_ref, double t_step, int32_t first_cell, int32_t num_cells, double* k_bar) {
  __shared__ double lds[k_sky_threads];
  const int j = first_cell + (int)blockIdx.x, last = first_cell + num_cells - 1, root = *g.root;
  const double lb = t_ref + (double)j * t_step, ub = t_ref + (double)(j + 1) * t_step;
  double mine = 0.0;
  for (int v = (int)threadIdx.x; v < g.n_nodes; v += k_sky_threads) {
    const double t_end = g.t[v];
    double t_start; int cs;
    if (v == root) { t_start = t_ref + (double)first_cell * t_step; cs = first_cell; }
    else { const int32_t p = g.parent[v]; if ((uint32_t)p >= (uint32_t)g.n_nodes) continue; t_start = g.t[p]; cs = sky_cell_of(t_start, t_ref, t_step, first_cell, last); }
    const int ce = sky_cell_of(t_end, t_ref, t_step, first_cell, last);
    if (j < cs || j > ce) continue;
    if (cs == ce) mine += (t_end - t_start) / t_step;
    else if (j == cs) mine += (ub - t_start) / t_step;
    else if (j == ce) mine += (t_end - lb) / t_step;
    else mine += 1.0;
  }
  mine = sr_block_sum(mine, lds);
  if (threadIdx.x == 0) k_bar[blockIdx.x] = mine;
}
// The times of the inner nodes in node order: thread j owns the nodes [j chunk, (j + 1) chunk), counts its inner nodes, thread 0 turns the
// counts into offsets, every thread writes its own.  One workgroup; *count = how many.
__global__ __launch_bounds__(k_sky_threads) void k_skygrid_tree_inner_times(GTreeDev g, double* inner_t, int32_t* count) {
  __shared__ int32_t off[k_sky_threads + 1];
  const int t = (int)threadIdx.x, chunk = (g.n_nodes + k_sky_threads - 1) / k_sky_threads;
  const int lo = t * chunk < g.n_nodes ? t * chunk : g.n_nodes, hi = lo + chunk < g.n_nodes ? lo + chunk : g.n_nodes;
  int32_t n = 0;
  for (int v = lo; v < hi; ++v) n += g.c0[v] >= 0 ? 1 : 0;
  off[t + 1] = n;
  __syncthreads();
  if (t == 0) { off[0] = 0; for (int i = 1; i <= k_sky_threads; ++i) off[i] += off[i - 1]; *count = off[k_sky_threads]; }
  __syncthreads();
  int32_t at = off[t];
  for (int v = lo; v < hi; ++v) if (g.c0[v] >= 0) inner_t[at++] = g.t[v];
}

// test hook (emat_debug_pop_gradient): op 3: d log(integral of N over [a[i], b[i]]) / d gamma_k; op 4: d log N(a[i]) / d gamma_k
__global__ void __launch_bounds__(64) k_debug_pop_gradient(PopTable pt, int op, int k, const double* a, const double* b, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = op == 3 ? dev::skygrid_d_log_int_N_d_gamma(pt, a[i], b[i], k) : dev::skygrid_d_log_N_d_gamma(pt, a[i], k);
}

}  // namespace emat
#endif  // EMAT_SKYGRID_KERNELS_HPP_
