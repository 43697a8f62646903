// emat_exp_pop_host.hpp -- the Exponential population moves' entry points: emat_exp_pop_moves and emat_tree_exp_pop_moves.
//
// Included by emat_backend.hip after emat_skygrid_host.hpp (sky_tree_stats; the statistics live in h->sky.k_bar / h->sky.inner_t); the kernels: emat_exp_pop_kernels.hpp.
#ifndef EMAT_EXP_POP_HOST_HPP_
#define EMAT_EXP_POP_HOST_HPP_

namespace {

// The argument checks the two entry points share: the model, the spec, the grid's origin and the trace.
emat_status xp_check_model_and_spec(emat_backend* h, const std::string& w, const emat_pop_model* pm, const emat_exp_pop_spec* spec, double t_ref, double t_step, const emat_exp_pop_result* out) {
  if (pm->kind != EMAT_POP_EXP) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the population model is not an exponential one");
  const double t0 = pm->p[0], n0 = pm->p[1], g = pm->p[2], min_pop = pm->p[3];
  if (!std::isfinite(n0) || !(n0 > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "n0 must be finite and positive");
  if (!std::isfinite(g)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g must be finite");
  if (!std::isfinite(t0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t0 must be finite");
  if (!std::isfinite(min_pop) || min_pop < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "min_pop must be finite and not negative");
  const emat_exp_pop_spec& s = *spec;
  if (!(s.g_min <= s.g_max)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g_min must not exceed g_max, and neither may be NaN");
  if (g < s.g_min || g > s.g_max) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g lies outside [g_min, g_max]");
  if (!std::isfinite(s.g_prior_scale) || !(s.g_prior_scale > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g_prior_scale must be finite and positive");
  if (!std::isfinite(s.g_prior_mu)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "g_prior_mu must be finite");
  if (!std::isfinite(s.inv_n0_prior_alpha)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inv_n0_prior_alpha must be finite");
  if (!std::isfinite(s.inv_n0_prior_beta)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inv_n0_prior_beta must be finite");
  if (s.rounds < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "rounds must not be negative");
  if (out->trace && (int64_t)out->trace_capacity < 2 * (int64_t)s.rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than 2 * rounds");
  if (!std::isfinite(t_ref) || !std::isfinite(t_step) || !(t_step > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t_ref must be finite and t_step finite and positive");
  return EMAT_OK;
}
emat_status xp_check_capacity(emat_backend* h, const std::string& w, const emat_exp_pop_spec& s, int64_t first_cell, int64_t num_cells) {
  if (num_cells > k_sky_max_cells) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(num_cells) + " cells are more than the moves hold (" + std::to_string(k_sky_max_cells) + ")");
  if (first_cell < -(1ll << 30) || first_cell + num_cells > (1ll << 30)) return fail(h, EMAT_ERR_CAPACITY, w + "the cells' numbers leave [-2^30, 2^30): choose t_ref nearer the tree");
  if (s.rounds > k_xp_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(s.rounds) + " rounds are more than the moves hold (" + std::to_string(k_xp_max_rounds) + ")");
  return EMAT_OK;
}

// The launch chain on statistics that are in h->sky.k_bar / h->sky.inner_t already; everything in the handle's own buffers.
emat_status xp_run(emat_backend* h, const emat_pop_model& pm, const emat_exp_pop_spec& s, double t_ref, double t_step, int32_t first_cell, int32_t num_cells, int32_t num_inner,
                   uint64_t key, emat_exp_pop_result* out, HostLaps& laps) {
  SkygridScratch& S = h->sky;
  ExpPopScratch& X = h->xp;
  const int steps = 2 * s.rounds, G = xp_groups(num_inner, num_cells);
  const bool want_trace = out->trace != nullptr && steps > 0;
  HIP_TRY(X.state.alloc_roomy((size_t)(steps + 1) * k_xp_state_doubles)); HIP_TRY(X.partials.alloc_roomy((size_t)(steps + 1) * (size_t)G)); HIP_TRY(X.result.alloc((size_t)k_xp_state_doubles));
  if (want_trace) HIP_TRY(X.trace.alloc_roomy((size_t)steps));
  ExpPopArgs a{};
  a.t0 = pm.p[0]; a.n0 = pm.p[1]; a.g = pm.p[2]; a.min_pop = pm.p[3]; a.spec = s;
  a.t_ref = t_ref; a.t_step = t_step; a.first_cell = first_cell; a.num_cells = num_cells; a.k_bar = S.k_bar.p; a.num_inner = num_inner; a.groups = G; a.inner_t = S.inner_t.p;
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
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_exp_pop_moves: ";
  if (!pm || !spec || !k_bar || !inner_t || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec, k_bar, inner_t and out must not be null");
  emat_status st = xp_check_model_and_spec(h, w, pm, spec, t_ref, t_step, out); if (st) return st;
  if (num_cells < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_cells must be at least 1");
  if (num_inner < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_inner must be at least 1");
  for (int32_t c = 0; c < num_cells; ++c)
    if (!std::isfinite(k_bar[c]) || k_bar[c] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "k_bar of cell " + std::to_string(c) + " is negative or not finite");
  for (int32_t i = 0; i < num_inner; ++i) {
    if (!std::isfinite(inner_t[i])) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " is not finite");
    const double cell = std::floor((inner_t[i] - t_ref) / t_step);   // Scalable_coalescent_prior::cell_for
    if (cell < (double)first_cell || cell >= (double)first_cell + (double)num_cells) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " lies outside the grid");
  }
  st = xp_check_capacity(h, w, *spec, first_cell, num_cells); if (st) return st;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }
  SkygridScratch& S = h->sky;
  HIP_TRY(S.k_bar.alloc_roomy((size_t)num_cells)); HIP_TRY(S.inner_t.alloc_roomy((size_t)num_inner));
  HIP_TRY(hipMemcpyAsync(S.k_bar.p, k_bar, (size_t)num_cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(S.inner_t.p, inner_t, (size_t)num_inner * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return xp_run(h, *pm, *spec, t_ref, t_step, first_cell, num_cells, num_inner, key, out, laps);
}

/* the moves on the statistics of the tree in HBM, which never leave it (header: emat_tree_exp_pop_moves) */
emat_status emat_tree_exp_pop_moves(emat_backend* h, const emat_pop_model* pm, const emat_exp_pop_spec* spec, double t_ref, double t_step, uint64_t key, emat_exp_pop_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_exp_pop_moves: ";
  if (!pm || !spec || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec and out must not be null");
  emat_status st = xp_check_model_and_spec(h, w, pm, spec, t_ref, t_step, out); if (st) return st;
  st = xp_check_capacity(h, w, *spec, 0, 1); if (st) return st;
  HostLaps laps;
  st = sky_tree_stats(h, w, t_ref, t_step); if (st) return st;
  SkygridScratch& S = h->sky;
  if (S.num_inner < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the resident tree has no inner node");
  return xp_run(h, *pm, *spec, t_ref, t_step, S.first_cell, S.num_cells, S.num_inner, key, out, laps);
}

}  // extern "C"

#endif  // EMAT_EXP_POP_HOST_HPP_
