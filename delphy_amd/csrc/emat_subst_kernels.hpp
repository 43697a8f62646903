// emat_subst_kernels.hpp -- the substitution-model moves on the device (reference core/run.cpp:703-719): Run::mu_move (:781-821), then `rounds`
// times Run::hky_frequencies_move (:953-1034) and Run::hky_kappa_move (:1036-1103), on the linked HKY model (mu, kappa, pi).
//
// Inputs are the statistics of the whole run in one record of k_sb_stats_doubles doubles: Ttwiddle_beta_a [P][4], num_muts_beta_ab [P][4][4] and the
// state counts at the run's root [4] (counts as doubles: integers below 2^53, exact in any order).  The record comes from the caller, or from the
// parts on the handle without leaving HBM:
//   k_subst_reduce_stats  one workgroup per column of k_global_stats' rows, 256 threads: thread j adds the rows j, j + 256, ... in ascending order,
//                         a tree of fixed shape over LDS adds the threads.  No atomics: the same bits from every launch.
//   k_subst_root_counts   one workgroup on the root part's root node: the reference sequence's counts less the root's deltas and missations
//                         (:996-1004), lane-parallel over its three lists and over the sites inside each missation interval.
//   k_subst_moves         ONE workgroup of one wavefront: the mu draw and the whole chain of 2 rounds steps.  Every lane runs the steps' scalar
//                         arithmetic on the same numbers (its own copy of the stream), so all agree on every decision without a broadcast; the
//                         16 (a, b) entries of q and the 16 + 4 P + 4 terms of a step's delta log G are formed one per lane, left in LDS and
//                         added by every lane in the reference's order.  Lane 0 writes the trace and the result.
// Random numbers: the (key, id) streams of emat_gamma_pure.hpp under two pseudo-ids, the next below the Exponential moves' one: k_sb_stream_mu, the
// mu draw from the stream's start; k_sb_stream_steps, step s the words 4 s .. 4 s + 3.
//
// Included by emat_backend.hip after emat_part_kernels.hpp (KernelArgs, the slab accessors, k_stats_row): everything in here is device code
// (csrc/Makefile: DEVSRC).
#ifndef EMAT_SUBST_KERNELS_HPP_
#define EMAT_SUBST_KERNELS_HPP_

#include "../../include/emat_backend.h"
#include "emat_gamma_pure.hpp"

namespace emat {

constexpr int k_sb_threads = 64;                    // k_subst_moves: one wavefront
constexpr int k_sb_reduce_threads = 256;            // k_subst_reduce_stats, k_subst_root_counts
constexpr uint32_t k_sb_stream_mu = 0xFFFFFFF8u;    // the mu draw (Marsaglia-Tsang, as the Skygrid's tau draw)
constexpr uint32_t k_sb_stream_steps = 0xFFFFFFF7u; // to_co x 4: step s = words 4 s .. 4 s + 3
// The statistics record (doubles): the arrays packed for the model's P, the rest zero
enum { k_sb_T = 0, k_sb_M = 4 * k_max_stats_partitions, k_sb_C = k_sb_M + 16 * k_max_stats_partitions, k_sb_stats_doubles = k_sb_C + 4 };
// What k_subst_moves leaves for the host (doubles)
enum { k_sb_mu = 0, k_sb_kappa, k_sb_pi, k_sb_shape = k_sb_pi + 4, k_sb_rate, k_sb_draw, k_sb_d_log_G, k_sb_d_other_priors, k_sb_mu_d_log_G, k_sb_mu_d_other_priors,
       k_sb_pi_accepted, k_sb_kappa_accepted, k_sb_pi_left_unit, k_sb_forced, k_sb_bad_posterior, k_sb_result_doubles };

struct SubstArgs {
  emat_subst_spec spec;
  int32_t P;                          // site partitions, 1 .. k_max_stats_partitions
  const double* stats;                // [k_sb_stats_doubles]
  uint64_t key;
  emat_subst_step* trace;             // null, or [2 rounds]
  double* result;                     // [k_sb_result_doubles]
};

__global__ __launch_bounds__(k_sb_reduce_threads) void k_subst_reduce_stats(const double* rows, int num_parts, int P, double* stats) {
  __shared__ double lds[k_sb_reduce_threads];
  const int t = (int)threadIdx.x, c = (int)blockIdx.x;   // c: a slot of the record below k_sb_C
  const bool is_T = c < k_sb_M;
  const bool used = is_T ? c < 4 * P : c - k_sb_M < 16 * P;
  const int col = is_T ? c : k_max_stats_partitions * 4 + (c - k_sb_M);   // where k_global_stats keeps it in a row
  double mine = 0.0;
  if (used) for (int p = t; p < num_parts; p += k_sb_reduce_threads) mine += rows[(size_t)p * k_stats_row + col];
  lds[t] = mine;
  __syncthreads();
  for (int s = k_sb_reduce_threads / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  if (t == 0) stats[c] = lds[0];
}

__global__ __launch_bounds__(k_sb_reduce_threads) void k_subst_root_counts(KernelArgs a, int root_part, double* stats) {
  __shared__ int lds[k_sb_reduce_threads][4];
  const int t = (int)threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[root_part];
  dev::Ctx c;
  init_ctx(c, slab, slab, a, nullptr);
  const int root = c.H->root;
  int d[4] = {0, 0, 0, 0};
  const auto bump = [&](int state, int by) { for (int s = 0; s < 4; ++s) if (s == state) d[s] += by; };
  const MutRec* m = dev::muts_of(c, root);
  for (int j = t; j < dev::nmuts(c, root); j += k_sb_reduce_threads) { bump(m[j].from, -1); bump(m[j].to, +1); }
  const IvRec* iv = dev::miss_of(c, root);
  for (int j = 0; j < (int)c.N[root].miss.cnt; ++j) {
    const int lo = iv[j].start < 0 ? 0 : iv[j].start, hi = iv[j].end > c.L ? c.L : iv[j].end;
    for (int l = lo + t; l < hi; l += k_sb_reduce_threads) bump((int)c.ref[l], -1);
  }
  const FsRec* fs = dev::mfs_of(c, root);   // (none at a run's root; counted as calc_log_root_prior counts them)
  for (int j = t; j < (int)c.N[root].mfs.cnt; j += k_sb_reduce_threads) { const int l = fs[j].site; if (l >= 0 && l < c.L) bump((int)c.ref[l], +1); bump((int)fs[j].state, -1); }
  for (int s = 0; s < 4; ++s) lds[t][s] = d[s];
  __syncthreads();
  if (t < 4) {
    long long n = 0;
    for (int p = 0; p < a.evo.num_partitions; ++p) n += a.ref_freqs[p * 4 + t];
    for (int r = 0; r < k_sb_reduce_threads; ++r) n += lds[r][t];
    stats[k_sb_C + t] = (double)n;
  }
}

__device__ __forceinline__ double sb_pick(const double v[4], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }

// Hky_model::derive_site_evo_model (evo_hky.cpp:7-50) into q[16] in LDS, as hky_derive_q (emat_move_specs.hpp) spells it: R by every lane, the
// off-diagonal entry (a, b) by lane 4 a + b, the diagonal of row a by lane a in the reference's order of b.  Ends on a barrier.
__device__ __forceinline__ void sb_derive_q(double kappa, const double pi[4], double* q, int lane) {
  double R = 0.0;
  for (int b = 0; b < 4; ++b) {
    double rowv = 0.0;
    for (int a = 0; a < 4; ++a) rowv += pi[a] * (a == b ? 0.0 : (((a ^ b) == 2) ? kappa : 1.0));
    R += rowv * pi[b];
  }
  if (lane < 16) {
    const int a = lane >> 2, b = lane & 3;
    q[lane] = a == b ? 0.0 : (((a ^ b) == 2) ? kappa : 1.0) / R * sb_pick(pi, b);
  }
  __syncthreads();
  if (lane < 4) {
    double diag = 0.0;
    for (int b = 0; b < 4; ++b) if (b != lane) diag -= q[4 * lane + b];
    q[5 * lane] = diag;
  }
  __syncthreads();
}

__global__ __launch_bounds__(k_sb_threads) void k_subst_moves(SubstArgs a) {
  __shared__ double q_old[16], q_new[16], term_branch[4 * k_max_stats_partitions], term_root[4], term_mut[16];
  const int lane = (int)threadIdx.x;
  const emat_subst_spec& sp = a.spec;
  const int W = 4 * a.P;
  const double* T = a.stats + k_sb_T; const double* M = a.stats + k_sb_M; const double* C = a.stats + k_sb_C;
  // this lane's statistics: Ttwiddle of (beta, a) = lane, the mutations a -> b = lane over all partitions (run.cpp's num_muts_ab_), the root's count of a = lane
  const double my_T = lane < W ? T[lane] : 0.0;
  double my_M = 0.0;
  if (lane < 16) for (int beta = 0; beta < a.P; ++beta) my_M += M[16 * beta + lane];
  const double my_C = lane < 4 ? C[lane] : 0.0;
  double num_muts = 0.0;
  for (int k = 0; k < 16; ++k) if ((k >> 2) != (k & 3)) for (int beta = 0; beta < a.P; ++beta) num_muts += M[16 * beta + k];

  double mu = sp.mu, kappa = sp.kappa, pi[4] = {sp.pi[0], sp.pi[1], sp.pi[2], sp.pi[3]};
  sb_derive_q(kappa, pi, q_old, lane);

  // ---- mu_move (run.cpp:797-820)
  double Ttwiddle = 0.0;
  for (int beta = 0; beta < a.P; ++beta) {
    double Ttwiddle_beta = 0.0;
    for (int s = 0; s < 4; ++s) Ttwiddle_beta += -q_old[5 * s] * T[4 * beta + s];
    Ttwiddle += Ttwiddle_beta;
  }
  const double shape = num_muts + sp.mu_prior_alpha, rate = Ttwiddle + sp.mu_prior_beta;
  const bool drawable = shape > 0.0 && rate > 0.0;   // (a NaN is not)
  double draw = __builtin_nan("");
  if (drawable) { SiteStream rs = site_stream(a.key, k_sb_stream_mu); draw = gamma_draw(shape, rate, rs); }
  double d_log_G = 0.0, d_other = 0.0, mu_d_log_G = 0.0, mu_d_other = 0.0;
  if (sp.do_mu != 0 && !drawable) {   // the host refuses this before the launch where it has the statistics; from the parts it learns of it here
    if (lane == 0) { for (int i = 0; i < k_sb_result_doubles; ++i) a.result[i] = 0.0; a.result[k_sb_shape] = shape; a.result[k_sb_rate] = rate; a.result[k_sb_bad_posterior] = 1.0; }
    return;
  }
  if (sp.do_mu != 0) {
    const double old_mu = mu, new_mu = draw;
    mu = new_mu;
    mu_d_log_G = -(new_mu - old_mu) * Ttwiddle + num_muts * ::log(new_mu / old_mu);
    mu_d_other = (sp.mu_prior_alpha - 1) * ::log(new_mu / old_mu) - sp.mu_prior_beta * (new_mu - old_mu);
    d_log_G += mu_d_log_G; d_other += mu_d_other;
  }

  // ---- the steps
  double n_pi_acc = 0.0, n_kappa_acc = 0.0, n_left = 0.0, n_forced = 0.0;
  const int steps = 2 * sp.rounds;
  for (int s = 0; s < steps; ++s) {
    SiteStream rs = site_stream(a.key, k_sb_stream_steps);
    rs.word = 4u * (uint32_t)s;
    const double u0 = to_co(site_stream_next64(rs)), u1 = to_co(site_stream_next64(rs)), u2 = to_co(site_stream_next64(rs)), u3 = to_co(site_stream_next64(rs));
    const bool is_pi = (s & 1) == 0;
    emat_subst_step r;
    r.kappa = kappa; for (int i = 0; i < 4; ++i) r.pi[i] = pi[i];
    r.delta_log_G = 0.0; r.log_prior_ratio = 0.0; r.log_metropolis = 0.0;
    r.ia = -1; r.ib = -1; r.accepted = 0; r.evaluated = 0; r.left_unit = 0; r.force_rejected = 0;
    double new_kappa = kappa, new_pi[4] = {pi[0], pi[1], pi[2], pi[3]};
    double log_prior_ratio = 0.0, log_hastings = 0.0;
    bool evaluated;
    if (is_pi) {   // run.cpp:964-979
      const double freq_delta = 0.01;
      const double d = freq_delta * u0;
      const int ia = (int)(4.0 * u1), ib = (ia + 1 + (int)(3.0 * u2)) & 3;
      r.proposal = d; r.ia = ia; r.ib = ib; r.u = u3;
      evaluated = sp.do_pi != 0;
      if (evaluated) {
        const double va = sb_pick(pi, ia) + d, vb = sb_pick(pi, ib) - d;
        if (va <= 0.0 || va >= 1.0 || vb <= 0.0 || vb >= 1.0) { evaluated = false; r.left_unit = 1; n_left += 1.0; }
        else for (int i = 0; i < 4; ++i) new_pi[i] = i == ia ? va : (i == ib ? vb : pi[i]);
      }
    } else {       // run.cpp:1049-1067
      const double scale_factor = 0.75;
      const double scale = scale_factor + (1.0 / scale_factor - scale_factor) * u0;
      r.proposal = scale; r.u = u1;
      evaluated = sp.do_kappa != 0;
      if (evaluated) {
        new_kappa = kappa * scale;
        const double mean_log_kappa = 1.0, sigma_log_kappa = 1.25;
        const double d_new = ::log(new_kappa) - mean_log_kappa, d_old = ::log(kappa) - mean_log_kappa;
        const double prior_new_over_prior_old = ::exp((-(d_new * d_new) - (-(d_old * d_old))) / (2 * sigma_log_kappa * sigma_log_kappa)) * kappa / new_kappa;
        log_prior_ratio = ::log(prior_new_over_prior_old);
        log_hastings = ::log(kappa / new_kappa);
      }
    }
    if (evaluated) {   // (the same for every lane: the barriers below are reached by all or none)
      r.evaluated = 1;
      sb_derive_q(new_kappa, new_pi, q_new, lane);
      int force = 0;
      // branch lengths (:988-992, :1073-1077): the term of (beta, a) = lane
      if (lane < W) { const int s4 = lane & 3; term_branch[lane] = mu * ((-q_new[5 * s4]) - (-q_old[5 * s4])) * my_T; }
      // root priors (:1005-1010), a pi step only
      if (lane < 4) {
        double v = 0.0;
        if (is_pi && my_C > 0.0) { const double pn = sb_pick(new_pi, lane); if (pn == 0) force = 1; else v = my_C * ::log(pn / sb_pick(pi, lane)); }
        term_root[lane] = v;
      }
      // mutations (:1013-1020, :1081-1088)
      if (lane < 16) {
        double v = 0.0;
        if ((lane >> 2) != (lane & 3) && my_M > 0.0) { if (q_new[lane] == 0) force = 1; else v = my_M * ::log(q_new[lane] / q_old[lane]); }
        term_mut[lane] = v;
      }
      const bool force_reject = __syncthreads_or(force) != 0;
      double delta_log_G = 0.0;
      for (int k = 0; k < W; ++k) delta_log_G -= term_branch[k];
      for (int k = 0; k < 4; ++k) delta_log_G += term_root[k];
      for (int k = 0; k < 16; ++k) delta_log_G += term_mut[k];
      bool accept = false;
      if (force_reject) { r.force_rejected = 1; n_forced += 1.0; }
      else {
        const double log_p_acc = is_pi ? delta_log_G : delta_log_G + log_prior_ratio + log_hastings;
        accept = log_p_acc > 0 || r.u < ::exp(log_p_acc);   // (a NaN rejects)
        r.delta_log_G = delta_log_G; r.log_prior_ratio = log_prior_ratio; r.log_metropolis = log_p_acc;
      }
      __syncthreads();   // every lane has read the terms and q_old's entries
      if (accept) {
        r.accepted = 1;
        kappa = new_kappa; for (int i = 0; i < 4; ++i) pi[i] = new_pi[i];
        if (lane < 16) q_old[lane] = q_new[lane];
        d_log_G += delta_log_G; d_other += log_prior_ratio;
        if (is_pi) n_pi_acc += 1.0; else n_kappa_acc += 1.0;
      }
      __syncthreads();
    }
    if (a.trace && lane == 0) a.trace[s] = r;
  }
  if (lane == 0) {
    double* o = a.result;
    o[k_sb_mu] = mu; o[k_sb_kappa] = kappa; for (int i = 0; i < 4; ++i) o[k_sb_pi + i] = pi[i];
    o[k_sb_shape] = shape; o[k_sb_rate] = rate; o[k_sb_draw] = draw;
    o[k_sb_d_log_G] = d_log_G; o[k_sb_d_other_priors] = d_other; o[k_sb_mu_d_log_G] = mu_d_log_G; o[k_sb_mu_d_other_priors] = mu_d_other;
    o[k_sb_pi_accepted] = n_pi_acc; o[k_sb_kappa_accepted] = n_kappa_acc; o[k_sb_pi_left_unit] = n_left; o[k_sb_forced] = n_forced; o[k_sb_bad_posterior] = 0.0;
  }
}

}  // namespace emat
#endif  // EMAT_SUBST_KERNELS_HPP_
