// emat_exp_pop_host.hpp -- the Exponential population moves' entry points: emat_exp_pop_moves and emat_tree_exp_pop_moves.
//
// Included by emat_backend.hip after emat_coal_stats_host.hpp (the statistics in h->coal, from the caller or from the tree in HBM); the kernels: emat_exp_pop_kernels.hpp.
#ifndef EMAT_EXP_POP_HOST_HPP_
#define EMAT_EXP_POP_HOST_HPP_

namespace {

// Both entry points: check the arguments (null pointers, the model, the spec, the trace, the grid's origin, the statistics handed in, the sizes), obtain the statistics
// (`host`, or those of the tree in HBM where it is null), run.
emat_status xp_moves(emat_backend* h, const std::string& w, const emat_pop_model* pm, const emat_exp_pop_spec* spec, double t_ref, double t_step, const CoalHostStats* host, uint64_t key, emat_exp_pop_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!pm || !spec || (host && (!host->k_bar || !host->inner_t)) || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec" + (host ? ", k_bar, inner_t" : "") + " and out must not be null");
  if (pm->kind != EMAT_POP_EXP) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the population model is not an exponential one");
  const double t0 = pm->p[0], n0 = pm->p[1], g = pm->p[2], min_pop = pm->p[3];
  if (!finite_positive(n0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "n0 must be finite and positive");
  if (!std::isfinite(g)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g must be finite");
  if (!std::isfinite(t0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t0 must be finite");
  if (!std::isfinite(min_pop) || min_pop < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "min_pop must be finite and not negative");
  if (const char* why = exp_pop_spec_fault(*spec, &g)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && (int64_t)out->trace_capacity < 2 * (int64_t)spec->rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than 2 * rounds");
  emat_status st = coal_check_origin(h, w, t_ref, t_step); if (st) return st;
  st = coal_check_host_values(h, w, t_ref, t_step, host); if (st) return st;
  st = host ? coal_check_capacity(h, w, host->first_cell, host->num_cells) : EMAT_OK; if (st) return st;
  if (spec->rounds > k_xp_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + rounds_beyond_text(spec->rounds, k_xp_max_rounds));
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  st = coal_obtain(h, w, t_ref, t_step, host); if (st) return st;
  // the launch chain on the statistics in h->coal; everything in the handle's own buffers
  const CoalStatsScratch& K = h->coal;
  ExpPopScratch& X = h->xp;
  const int steps = 2 * spec->rounds, G = xp_groups(K.num_inner, K.num_cells);
  const bool want_trace = out->trace != nullptr && steps > 0;
  HIP_TRY(X.state.alloc_roomy((size_t)(steps + 1) * k_xp_state_doubles)); HIP_TRY(X.partials.alloc_roomy((size_t)(steps + 1) * (size_t)G)); HIP_TRY(X.result.alloc((size_t)k_xp_state_doubles));
  if (want_trace) HIP_TRY(X.trace.alloc_roomy((size_t)steps));
  ExpPopArgs a{};
  a.t0 = t0; a.n0 = n0; a.g = g; a.min_pop = min_pop; a.spec = *spec;
  a.t_ref = t_ref; a.t_step = t_step; a.first_cell = K.first_cell; a.num_cells = K.num_cells; a.k_bar = K.k_bar.p; a.num_inner = K.num_inner; a.groups = G; a.inner_t = K.inner_t.p;
  a.key = key; a.state = X.state.p; a.partials = X.partials.p; a.trace = want_trace ? X.trace.p : nullptr; a.result = X.result.p;
  if (laps.on) HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("exp_pop_moves: 1 finish_pass, statistics to the device");
  for (int e = 0; e <= steps; ++e) hipLaunchKernelGGL(k_exp_pop_eval, dim3((unsigned)G), dim3(k_xp_threads), 0, h->stream, a, e);
  hipLaunchKernelGGL(k_exp_pop_finish, dim3(1), dim3(64), 0, h->stream, a, steps + 1);
  HIP_TRY(hipGetLastError());
  laps.mark("exp_pop_moves: 2 queueing the launch chain");
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("exp_pop_moves: 3 the launch chain");
  double r[k_xp_state_doubles];
  HIP_TRY(hipMemcpy(r, X.result.p, sizeof r, hipMemcpyDeviceToHost));
  if (want_trace) HIP_TRY(hipMemcpy(out->trace, X.trace.p, (size_t)steps * sizeof(emat_exp_pop_step), hipMemcpyDeviceToHost));
  out->n0 = r[k_xp_n0]; out->g = r[k_xp_g];
  out->log_coalescent_prior_start = r[k_xp_log_prior_start]; out->log_coalescent_prior_end = r[k_xp_log_prior]; out->delta_log_other_priors = r[k_xp_d_other_priors];
  out->n0_accepted = (int32_t)r[k_xp_n0_accepted]; out->g_accepted = (int32_t)r[k_xp_g_accepted]; out->g_out_of_bounds = (int32_t)r[k_xp_g_out_of_bounds]; out->pad_ = 0;
  laps.mark("exp_pop_moves: 4 copy-back");
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* pop_size_move + pop_growth_rate_move, `rounds` times, on the device (header: emat_exp_pop_moves) */
emat_status emat_exp_pop_moves(emat_backend* h, const emat_pop_model* pm, const emat_exp_pop_spec* spec, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                               const double* k_bar, int32_t num_inner, const double* inner_t, uint64_t key, emat_exp_pop_result* out) {
  const CoalHostStats host{first_cell, num_cells, k_bar, num_inner, inner_t};
  return xp_moves(h, "emat_exp_pop_moves: ", pm, spec, t_ref, t_step, &host, key, out);
}

/* the moves on the statistics of the tree in HBM, which never leave it (header: emat_tree_exp_pop_moves) */
emat_status emat_tree_exp_pop_moves(emat_backend* h, const emat_pop_model* pm, const emat_exp_pop_spec* spec, double t_ref, double t_step, uint64_t key, emat_exp_pop_result* out) {
  return xp_moves(h, "emat_tree_exp_pop_moves: ", pm, spec, t_ref, t_step, nullptr, key, out);
}

}  // extern "C"

#endif  // EMAT_EXP_POP_HOST_HPP_
