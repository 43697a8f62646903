// emat_exp_pop_kernels.hpp -- the Exponential population moves on the device (reference core/run.cpp:754-764): `rounds` times pop_size_move
// (:1237-1276) then pop_growth_rate_move (:1278-1319), each a Metropolis step that re-evaluates Scalable_coalescent_prior::calc_log_prior
// (scalable_coalescent.cpp:140-187) under the proposed Exp_pop_model.
//
// Inputs are the statistics of the whole run, as for the Skygrid moves (emat_skygrid_kernels.hpp): the lineage grid k_bar[c] and the times of
// the inner nodes.  With the min_pop barrier log N(t) = log max(min_pop, n0 e^{g (t - t0)}) is not linear in (n0, g), so every evaluation reads
// every node: 1 + 2 rounds evaluations of num_cells cell integrals and num_inner logarithms, too many for one workgroup.  The shape:
//   k_exp_pop_eval    launch e = 0 .. 2 rounds, G workgroups of 1 024 threads, G = min(256, ceil(max(num_inner, num_cells) / 1 024)) -- a function
//                     of the sizes only, never of the device.  Evaluation 0 is the prior of the model passed in, evaluation e >= 1 that of step
//                     e - 1's proposal (even steps: n0, odd steps: g).  Launch e first has EVERY workgroup re-derive the state after step e - 2
//                     from the state record launch e - 1 left and the G partials of evaluation e - 1 (xp_advance): all read the same numbers, so
//                     all take the same decision and none waits for another.  Workgroup 0 writes the new state record and the step's trace record.
//                     Every workgroup then forms step e - 1's proposal from that state and writes its own partial of the proposal's prior to
//                     partials[e][workgroup]; a step that needs no evaluation (its move disabled, g out of bounds) ends the launch there.
//   k_exp_pop_finish  one workgroup: the decision of the last step, and the result.
// Order between evaluations is the stream's; no kernel reads what another workgroup of the same launch writes, and every loop is bounded by an argument.
// Sums: thread j of workgroup b adds the terms b 1 024 + j, + 1 024 G, ... (cells first, then nodes) in ascending order, sr_block_sum's tree of
// fixed shape adds the threads, and the G partials are added in workgroup order.  No atomics: the same bits from every launch and on every handle.
// Random numbers: the (key, id) streams of emat_gamma_pure.hpp under ONE pseudo-id, k_xp_stream, the next below the Skygrid's five.  Step s takes
// block s of the stream: word 0 the proposal's uniform, word 1 the acceptance uniform, both in [0, 1), both drawn whether needed or not.
//
// Included by emat_backend.hip after emat_skygrid_kernels.hpp: everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_EXP_POP_KERNELS_HPP_
#define EMAT_EXP_POP_KERNELS_HPP_

#include "../../include/emat_backend.h"
#include "emat_gamma_pure.hpp"

namespace emat {

constexpr int k_xp_threads = k_sr_threads;          // 1 024: sr_block_sum's shape
constexpr int k_xp_max_groups = 256;
constexpr int k_xp_max_rounds = 4096;
constexpr uint32_t k_xp_stream = 0xFFFFFFF9u;       // to_co, to_co: block s = step s's proposal and acceptance uniforms
// The state a launch leaves for the next and k_exp_pop_finish leaves for the host (doubles)
enum { k_xp_n0 = 0, k_xp_g, k_xp_log_prior, k_xp_d_other_priors, k_xp_log_prior_start, k_xp_n0_accepted, k_xp_g_accepted, k_xp_g_out_of_bounds, k_xp_state_doubles };

struct ExpPopArgs {
  double t0, n0, g, min_pop;          // the model the round starts from
  emat_exp_pop_spec spec;
  double t_ref, t_step;
  int32_t first_cell, num_cells;
  const double* k_bar;                // [num_cells]
  int32_t num_inner, groups;          // groups: G, the workgroups of an evaluation
  const double* inner_t;              // [num_inner]
  uint64_t key;
  double* state;                      // [2 rounds + 1][k_xp_state_doubles]: record e is the state before step e - 1
  double* partials;                   // [2 rounds + 1][groups]
  emat_exp_pop_step* trace;           // null, or [2 rounds]
  double* result;                     // [k_xp_state_doubles]
};

inline int xp_groups(int32_t num_inner, int32_t num_cells) {
  const int64_t most = num_inner > num_cells ? num_inner : num_cells, g = (most + k_xp_threads - 1) / k_xp_threads;
  return (int)(g < 1 ? 1 : (g > k_xp_max_groups ? k_xp_max_groups : g));
}

// Step s's proposal from the state before it: pop_size_move (run.cpp:1249-1257) for even s, pop_growth_rate_move (:1289-1301) for odd s.
struct ExpPopProposal {
  double n0, g;                       // the proposed model (t0 and min_pop stay)
  double proposed, log_prior_ratio, log_hastings, u;
  bool evaluated, out_of_bounds;
};
__device__ __forceinline__ ExpPopProposal xp_propose(const ExpPopArgs& a, const double* st, int s) {
  const emat_exp_pop_spec& sp = a.spec;
  SiteStream rs = site_stream(a.key, k_xp_stream);
  rs.word = 2u * (uint32_t)s;
  const double u0 = to_co(site_stream_next64(rs));
  ExpPopProposal q;
  q.u = to_co(site_stream_next64(rs));
  q.n0 = st[k_xp_n0]; q.g = st[k_xp_g];
  q.log_prior_ratio = 0.0; q.log_hastings = 0.0; q.out_of_bounds = false;
  if ((s & 1) == 0) {
    q.proposed = q.n0;
    q.evaluated = sp.n0_move_enabled != 0;
    if (!q.evaluated) return q;
    const double scale_factor = 0.75;
    const double old_n0 = st[k_xp_n0];
    const double scale = scale_factor + (1 / scale_factor - scale_factor) * u0;
    const double new_n0 = scale * old_n0;
    q.log_prior_ratio = -(sp.inv_n0_prior_alpha + 1) * ::log(scale) - sp.inv_n0_prior_beta * (1.0 / new_n0 - 1.0 / old_n0);
    q.log_hastings = ::log(old_n0 / new_n0);
    q.n0 = new_n0; q.proposed = new_n0;
    return q;
  }
  q.proposed = q.g;
  q.evaluated = sp.g_move_enabled != 0;
  if (!q.evaluated) return q;
  const double window_size = 1.0 / 365.0;
  const double old_g = st[k_xp_g];
  const double delta = -window_size + (2 * window_size) * u0;
  const double new_g = old_g + delta;
  q.proposed = new_g;
  if (new_g < sp.g_min || new_g > sp.g_max) { q.evaluated = false; q.out_of_bounds = true; return q; }
  q.log_prior_ratio = (__builtin_fabs(old_g - sp.g_prior_mu) - __builtin_fabs(new_g - sp.g_prior_mu)) / sp.g_prior_scale;
  q.g = new_g;
  return q;
}

// The G partials of evaluation e, in workgroup order.
__device__ __forceinline__ double xp_sum_partials(const ExpPopArgs& a, int e) {
  const double* p = a.partials + (size_t)e * (size_t)a.groups;
  double v = p[0];
  for (int b = 1; b < a.groups; ++b) v += p[b];
  return v;
}

// The state before step e - 1 (e >= 1), from record e - 1 and evaluation e - 1: record 0 gets its prior, every later one the decision of
// step e - 2 (run.cpp:1265-1275, :1309-1318).  Every thread of every workgroup computes the same; the first thread of workgroup 0 writes the trace.
__device__ __forceinline__ void xp_advance(const ExpPopArgs& a, int e, double* st) {
  const double* prev = a.state + (size_t)(e - 1) * k_xp_state_doubles;
  for (int i = 0; i < k_xp_state_doubles; ++i) st[i] = prev[i];
  if (e == 1) { st[k_xp_log_prior] = st[k_xp_log_prior_start] = xp_sum_partials(a, 0); return; }
  const int s = e - 2;
  const ExpPopProposal q = xp_propose(a, st, s);
  double new_log_coal = 0.0, log_metropolis = 0.0;
  bool accept = false;
  if (q.evaluated) {
    const double old_log_coal = st[k_xp_log_prior];
    new_log_coal = xp_sum_partials(a, e - 1);
    log_metropolis = (new_log_coal - old_log_coal) + q.log_prior_ratio;
    if ((s & 1) == 0) log_metropolis += q.log_hastings;
    accept = log_metropolis > 0 || q.u < ::exp(log_metropolis);   // (a NaN rejects)
    if (accept) {
      st[k_xp_n0] = q.n0; st[k_xp_g] = q.g;
      st[k_xp_log_prior] = new_log_coal;
      st[k_xp_d_other_priors] += q.log_prior_ratio;
      st[(s & 1) == 0 ? k_xp_n0_accepted : k_xp_g_accepted] += 1.0;
    }
  }
  if (q.out_of_bounds) st[k_xp_g_out_of_bounds] += 1.0;
  if (a.trace && blockIdx.x == 0 && threadIdx.x == 0) {
    emat_exp_pop_step r;
    r.proposed = q.proposed; r.log_coalescent_prior_proposed = new_log_coal; r.log_prior_ratio = q.log_prior_ratio; r.log_metropolis = log_metropolis; r.u = q.u;
    r.accepted = accept ? 1 : 0; r.evaluated = q.evaluated ? 1 : 0;
    a.trace[s] = r;
  }
}

// This workgroup's share of calc_log_prior under Exp_pop_model{t0, n0, g, min_pop} (scalable_coalescent.cpp:140-187), t_c as the model's
// constructor derives it (pop_model.cpp:32-36).  Ends on a barrier.
__device__ __forceinline__ double xp_partial_log_prior(const ExpPopArgs& a, double n0, double g, double* lds) {
  PopTable pt{};
  pt.kind = 1; pt.p[0] = a.t0; pt.p[1] = n0; pt.p[2] = g; pt.p[3] = a.min_pop;
  pt.t_c = (a.min_pop > 0.0 && g != 0.0) ? a.t0 + ::log(a.min_pop / n0) / g : __builtin_nan("");
  const int first = (int)blockIdx.x * k_xp_threads + (int)threadIdx.x, stride = a.groups * k_xp_threads;
  double mine = 0.0;
  for (int c = first; c < a.num_cells; c += stride) {
    const double lb = a.t_ref + (double)(a.first_cell + c) * a.t_step, ub = lb + a.t_step;
    double popsize_bar = dev::pop_integral(pt, lb, ub) / a.t_step;
    if (popsize_bar == 0.0) popsize_bar = 1e-100;   // the reference's stopgap
    const double kbar = a.k_bar[c];
    mine -= a.t_step * kbar * (kbar - 1) / (2.0 * popsize_bar);
  }
  for (int i = first; i < a.num_inner; i += stride) mine -= ::log(dev::pop_at_time(pt, a.inner_t[i]));
  return sr_block_sum(mine, lds);
}

__global__ __launch_bounds__(k_xp_threads) void k_exp_pop_eval(ExpPopArgs a, int e) {
  __shared__ double lds[k_xp_threads];
  double st[k_xp_state_doubles];
  if (e == 0) {
    for (int i = 0; i < k_xp_state_doubles; ++i) st[i] = 0.0;
    st[k_xp_n0] = a.n0; st[k_xp_g] = a.g;
  } else xp_advance(a, e, st);
  if (blockIdx.x == 0 && threadIdx.x == 0) for (int i = 0; i < k_xp_state_doubles; ++i) a.state[(size_t)e * k_xp_state_doubles + i] = st[i];
  double n0 = st[k_xp_n0], g = st[k_xp_g];
  if (e > 0) {
    const ExpPopProposal q = xp_propose(a, st, e - 1);
    if (!q.evaluated) return;   // the same for every thread of every workgroup
    n0 = q.n0; g = q.g;
  }
  const double partial = xp_partial_log_prior(a, n0, g, lds);
  if (threadIdx.x == 0) a.partials[(size_t)e * (size_t)a.groups + blockIdx.x] = partial;
}

// `e` = 2 rounds + 1: the state after the last step.
__global__ __launch_bounds__(64) void k_exp_pop_finish(ExpPopArgs a, int e) {
  double st[k_xp_state_doubles];
  xp_advance(a, e, st);
  if (threadIdx.x == 0) for (int i = 0; i < k_xp_state_doubles; ++i) a.result[i] = st[i];
}

}  // namespace emat
#endif  // EMAT_EXP_POP_KERNELS_HPP_
