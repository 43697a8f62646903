// emat_skygrid_host.hpp -- the Skygrid population moves' entry points: emat_skygrid_moves, emat_tree_skygrid_moves and the gradient's test hook.
//
// Included by emat_backend.hip after emat_coal_stats_host.hpp (the statistics in h->coal, from the caller or from the tree in HBM); the kernels: emat_skygrid_kernels.hpp.
#ifndef EMAT_SKYGRID_HOST_HPP_
#define EMAT_SKYGRID_HOST_HPP_

namespace {

// Both entry points: check the arguments (null pointers, the model, the grid's origin, the spec, the trace, the statistics handed in, the sizes), obtain the statistics
// (`host`, or those of the tree in HBM where it is null), run.
emat_status sky_moves(emat_backend* h, const std::string& w, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, const CoalHostStats* host, uint64_t key, emat_skygrid_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!pm || !spec || (host && (!host->k_bar || !host->inner_t)) || !out || !out->gamma) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec, " + (host ? "k_bar, inner_t, " : "") + "out and out->gamma must not be null");
  if (pm->kind != EMAT_POP_SKYGRID) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the population model is not a Skygrid");
  HostPopModel hp;
  { const std::string why = probe_host_pop(*pm, hp); if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why); }
  for (size_t k = 0; k < hp.gamma.size(); ++k)
    if (!std::isfinite(hp.gamma[k]) || !std::isfinite(hp.x[k])) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "knot " + std::to_string(k) + " has a time or a gamma that is not finite");
  emat_status st = coal_check_origin(h, w, t_ref, t_step); if (st) return st;
  if (const char* why = skygrid_spec_fault(*spec)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && out->trace_capacity < spec->hmc_steps) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than hmc_steps");
  st = coal_check_host_values(h, w, t_ref, t_step, host); if (st) return st;
  if (hp.x.size() > (size_t)k_sky_max_knots) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(hp.x.size()) + " knots are more than the moves hold (" + std::to_string(k_sky_max_knots) + ")");
  st = host ? coal_check_capacity(h, w, host->first_cell, host->num_cells) : EMAT_OK; if (st) return st;
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase, each kernel waited for on its own)
  st = coal_obtain(h, w, t_ref, t_step, host); if (st) return st;
  // the two launches on the statistics in h->coal; everything in the handle's own buffers
  SkygridScratch& S = h->sky;
  const CoalStatsScratch& K = h->coal;
  const size_t n = hp.x.size();
  const bool want_trace = out->trace != nullptr;
  const size_t trace_doubles = want_trace ? (size_t)(k_sky_trace_head_rows + k_sky_trace_step_rows * spec->hmc_steps) * n : 0;
  HIP_TRY(S.x.alloc(n)); HIP_TRY(S.g.alloc(n)); HIP_TRY(S.c.alloc(n)); HIP_TRY(S.W.alloc(n)); HIP_TRY(S.gamma_out.alloc(n));
  HIP_TRY(S.popsize_bar.alloc_roomy((size_t)K.num_cells)); HIP_TRY(S.result.alloc((size_t)k_sky_result_doubles));
  HIP_TRY(hipMemcpyAsync(S.x.p, hp.x.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(S.g.p, hp.gamma.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (want_trace) { HIP_TRY(S.trace.alloc_roomy(trace_doubles)); HIP_TRY(hipMemsetAsync(S.trace.p, 0, trace_doubles * sizeof(double), h->stream)); }
  SkygridArgs a{};
  a.type = hp.skygrid_type; a.num_knots = (int32_t)n; a.x = S.x.p; a.gamma_in = S.g.p;
  a.inv_dx = probe_pop_table(hp, S.x.p, S.g.p).skygrid_inv_dx;
  a.t_ref = t_ref; a.t_step = t_step; a.first_cell = K.first_cell; a.num_cells = K.num_cells; a.k_bar = K.k_bar.p; a.popsize_bar = S.popsize_bar.p;
  a.num_inner = K.num_inner; a.inner_t = K.inner_t.p; a.c_k = S.c.p; a.W_k = S.W.p;
  a.spec = *spec; a.key = key; a.gamma_out = S.gamma_out.p; a.result = S.result.p; a.trace = want_trace ? S.trace.p : nullptr; a.trace_steps = want_trace ? spec->hmc_steps : 0;
  laps.mark("skygrid_moves: 1 finish_pass, model and statistics to the device");
  hipLaunchKernelGGL(k_skygrid_node_stats, dim3((unsigned)n), dim3(k_sky_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  if (laps.on) { HIP_TRY(hipStreamSynchronize(h->stream)); laps.mark("skygrid_moves: 2 k_skygrid_node_stats"); }
  hipLaunchKernelGGL(k_skygrid_moves, dim3(1), dim3(k_sky_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark(laps.on ? "skygrid_moves: 3 k_skygrid_moves" : "skygrid_moves: 2-3 the two kernels");
  double r[k_sky_result_doubles];
  HIP_TRY(hipMemcpy(r, S.result.p, sizeof r, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out->gamma, S.gamma_out.p, n * sizeof(double), hipMemcpyDeviceToHost));
  if (want_trace) HIP_TRY(hipMemcpy(out->trace, S.trace.p, trace_doubles * sizeof(double), hipMemcpyDeviceToHost));
  out->tau = r[k_sky_tau]; out->log_coalescent_prior_start = r[k_sky_log_prior_start]; out->log_coalescent_prior_end = r[k_sky_log_prior_end];
  out->delta_log_other_priors = r[k_sky_d_other_priors];
  out->tau_post_alpha = r[k_sky_tau_post_alpha]; out->tau_post_beta = r[k_sky_tau_post_beta]; out->tau_draw = r[k_sky_tau_draw]; out->tau_delta_log_prior = r[k_sky_tau_d_prior];
  out->zero_B = r[k_sky_zm_B]; out->zero_shape = r[k_sky_zm_shape]; out->zero_rate = r[k_sky_zm_rate]; out->zero_I_bar = r[k_sky_zm_I_bar];
  out->zero_delta_gamma_bar = r[k_sky_zm_d_gamma_bar]; out->zero_log_metropolis = r[k_sky_zm_log_metropolis]; out->zero_u = r[k_sky_zm_u];
  out->zero_accepted = (int32_t)r[k_sky_zm_accepted];
  out->hmc_accepted = (int32_t)r[k_sky_hmc_accepted]; out->hmc_dt = r[k_sky_hmc_dt]; out->hmc_K_old = r[k_sky_hmc_K_old]; out->hmc_K_new = r[k_sky_hmc_K_new];
  out->hmc_U_prior_old = r[k_sky_hmc_U_prior_old]; out->hmc_U_prior_new = r[k_sky_hmc_U_prior_new];
  out->hmc_U_coal_old = r[k_sky_hmc_U_coal_old]; out->hmc_U_coal_new = r[k_sky_hmc_U_coal_new];
  out->hmc_log_metropolis = r[k_sky_hmc_log_metropolis]; out->hmc_u = r[k_sky_hmc_u];
  out->hmc_K_exit_step = (int32_t)r[k_sky_hmc_K_exit_step]; out->hmc_nan = (int32_t)r[k_sky_hmc_nan]; out->hmc_steps_done = (int32_t)r[k_sky_hmc_steps_done];
  laps.mark("skygrid_moves: 4 copy-back");
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* skygrid_tau_move + skygrid_gammas_zero_mode_gibbs_move + skygrid_gammas_hmc_move on the device (header: emat_skygrid_moves) */
emat_status emat_skygrid_moves(emat_backend* h, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                               const double* k_bar, int32_t num_inner, const double* inner_t, uint64_t key, emat_skygrid_result* out) {
  const CoalHostStats host{first_cell, num_cells, k_bar, num_inner, inner_t};
  return sky_moves(h, "emat_skygrid_moves: ", pm, spec, t_ref, t_step, &host, key, out);
}

/* the moves on the statistics of the tree in HBM, which never leave it (header: emat_tree_skygrid_moves) */
emat_status emat_tree_skygrid_moves(emat_backend* h, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, uint64_t key, emat_skygrid_result* out) {
  return sky_moves(h, "emat_tree_skygrid_moves: ", pm, spec, t_ref, t_step, nullptr, key, out);
}

/* test hook (header: emat_debug_pop_gradient) */
emat_status emat_debug_pop_gradient(emat_backend* h, const emat_pop_model* pm, int32_t op, int32_t k, int32_t n, const double* a, const double* b, double* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_debug_pop_gradient: ";
  if (!pm || n < 0 || (n > 0 && (!a || !b || !out))) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model and, with n > 0, a, b and out must not be null; n must not be negative");
  if (op != 3 && op != 4) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "op must be 3 (d log int N / d gamma_k) or 4 (d log N / d gamma_k)");
  if (pm->kind != EMAT_POP_SKYGRID) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the population model is not a Skygrid");
  HostPopModel hp;
  { const std::string why = probe_host_pop(*pm, hp); if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why); }
  if (k < 0 || k >= (int32_t)hp.x.size()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "knot " + std::to_string(k) + " is outside [0, " + std::to_string(hp.x.size()) + ")");
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return EMAT_OK;
  DevBuf<double> dx, dg, da, db, dout;
  HIP_TRY(dx.upload(hp.x.data(), hp.x.size())); HIP_TRY(dg.upload(hp.gamma.data(), hp.gamma.size()));
  HIP_TRY(da.upload(a, (size_t)n)); HIP_TRY(db.upload(b, (size_t)n)); HIP_TRY(dout.alloc((size_t)n));
  hipLaunchKernelGGL(k_debug_pop_gradient, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, probe_pop_table(hp, dx.p, dg.p), (int)op, (int)k, da.p, db.p, dout.p, (int)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_SKYGRID_HOST_HPP_
