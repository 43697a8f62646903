// emat_skygrid_host.hpp -- the Skygrid population moves' entry points: emat_skygrid_moves, emat_tree_coalescent_stats, emat_tree_skygrid_moves and the gradient's test hook.
//
// Included by emat_backend.hip after emat_probe_host.hpp (probe_host_pop, probe_pop_table); the kernels: emat_skygrid_kernels.hpp.
#ifndef EMAT_SKYGRID_HOST_HPP_
#define EMAT_SKYGRID_HOST_HPP_

namespace {

// The argument checks the two entry points share: the model, the spec, the grid's origin and the trace.  "" or EMAT_OK; `hp` receives the model.
emat_status sky_check_model_and_spec(emat_backend* h, const std::string& w, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, const emat_skygrid_result* out, HostPopModel& hp) {
  if (pm->kind != EMAT_POP_SKYGRID) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the population model is not a Skygrid");
  { const std::string why = probe_host_pop(*pm, hp); if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why); }
  for (size_t k = 0; k < hp.gamma.size(); ++k)
    if (!std::isfinite(hp.gamma[k]) || !std::isfinite(hp.x[k])) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "knot " + std::to_string(k) + " has a time or a gamma that is not finite");
  if (!std::isfinite(t_ref) || !std::isfinite(t_step) || !(t_step > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t_ref must be finite and t_step finite and positive");
  const emat_skygrid_spec& s = *spec;
  if (!std::isfinite(s.tau) || !(s.tau > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "tau must be finite and positive");
  if (s.low_gamma_barrier_enabled && (!std::isfinite(s.low_gamma_barrier_scale) || !(s.low_gamma_barrier_scale > 0.0)))
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "low_gamma_barrier_scale must be finite and positive with the barrier on");
  if (s.hmc_steps < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "hmc_steps must not be negative");
  if (!std::isfinite(s.hmc_mean_dt) || !(s.hmc_mean_dt > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "hmc_mean_dt must be finite and positive");
  if (out->trace && out->trace_capacity < s.hmc_steps) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than hmc_steps");
  return EMAT_OK;
}
emat_status sky_check_capacity(emat_backend* h, const std::string& w, size_t knots, int64_t first_cell, int64_t num_cells) {
  if (knots > (size_t)k_sky_max_knots) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(knots) + " knots are more than the moves hold (" + std::to_string(k_sky_max_knots) + ")");
  if (num_cells > k_sky_max_cells) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(num_cells) + " cells are more than the moves hold (" + std::to_string(k_sky_max_cells) + ")");
  if (first_cell < -(1ll << 30) || first_cell + num_cells > (1ll << 30)) return fail(h, EMAT_ERR_CAPACITY, w + "the cells' numbers leave [-2^30, 2^30): choose t_ref nearer the tree");
  return EMAT_OK;
}

// The two launches on statistics that are in h->sky.k_bar / h->sky.inner_t already; everything in the handle's own buffers.
emat_status sky_run(emat_backend* h, const HostPopModel& hp, const emat_skygrid_spec& s, double t_ref, double t_step, int32_t first_cell, int32_t num_cells, int32_t num_inner,
                    uint64_t key, emat_skygrid_result* out, HostLaps& laps) {
  SkygridScratch& S = h->sky;
  const size_t n = hp.x.size();
  const bool want_trace = out->trace != nullptr;
  const size_t trace_doubles = want_trace ? (size_t)(k_sky_trace_head_rows + k_sky_trace_step_rows * s.hmc_steps) * n : 0;
  HIP_TRY(S.x.alloc(n)); HIP_TRY(S.g.alloc(n)); HIP_TRY(S.c.alloc(n)); HIP_TRY(S.W.alloc(n)); HIP_TRY(S.gamma_out.alloc(n));
  HIP_TRY(S.popsize_bar.alloc_roomy((size_t)num_cells)); HIP_TRY(S.result.alloc((size_t)k_sky_result_doubles));
  HIP_TRY(hipMemcpyAsync(S.x.p, hp.x.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(S.g.p, hp.gamma.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (want_trace) { HIP_TRY(S.trace.alloc_roomy(trace_doubles)); HIP_TRY(hipMemsetAsync(S.trace.p, 0, trace_doubles * sizeof(double), h->stream)); }
  SkygridArgs a{};
  a.type = hp.skygrid_type; a.num_knots = (int32_t)n; a.x = S.x.p; a.gamma_in = S.g.p;
  a.inv_dx = probe_pop_table(hp, S.x.p, S.g.p).skygrid_inv_dx;
  a.t_ref = t_ref; a.t_step = t_step; a.first_cell = first_cell; a.num_cells = num_cells; a.k_bar = S.k_bar.p; a.popsize_bar = S.popsize_bar.p;
  a.num_inner = num_inner; a.inner_t = S.inner_t.p; a.c_k = S.c.p; a.W_k = S.W.p;
  a.spec = s; a.key = key; a.gamma_out = S.gamma_out.p; a.result = S.result.p; a.trace = want_trace ? S.trace.p : nullptr; a.trace_steps = want_trace ? s.hmc_steps : 0;
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

// Scalable_coalescent_prior's grid and the inner nodes' times of the tree in HBM, into h->sky (k_bar, inner_t, first_cell, num_cells, num_inner).
emat_status sky_tree_stats(emat_backend* h, const std::string& w, double t_ref, double t_step) {
  emat_status st = gt_require_tree_home(h, false, w); if (st) return st;
  GTreeHost& G = h->gt;
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }
  SkygridScratch& S = h->sky;
  const GTreeDev T = G.dev();
  HIP_TRY(S.extent.alloc(2)); HIP_TRY(S.count.alloc(1)); HIP_TRY(S.inner_t.alloc_roomy((size_t)G.n));
  hipLaunchKernelGGL(k_skygrid_tree_extent, dim3(1), dim3(k_sky_threads), 0, h->stream, T, S.extent.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_skygrid_tree_inner_times, dim3(1), dim3(k_sky_threads), 0, h->stream, T, S.inner_t.p, S.count.p);
  HIP_TRY(hipGetLastError());
  double ext[2]; int32_t cnt = 0;
  HIP_TRY(hipMemcpyAsync(ext, S.extent.p, sizeof ext, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&cnt, S.count.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const double c_root = std::floor((ext[0] - t_ref) / t_step), c_tip = std::floor((ext[1] - t_ref) / t_step);   // Scalable_coalescent_prior::cell_for
  if (!std::isfinite(c_root) || !std::isfinite(c_tip) || c_tip < c_root) return fail(h, EMAT_ERR_INTERNAL, w + "the resident tree's root is later than its latest tip");
  const double cells = c_tip - c_root + 1.0;
  if (cells > (double)k_sky_max_cells) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string((long long)cells) + " cells are more than the moves hold (" + std::to_string(k_sky_max_cells) + ")");
  if (c_root < -(double)(1 << 30) || c_tip >= (double)(1 << 30)) return fail(h, EMAT_ERR_CAPACITY, w + "the cells' numbers leave [-2^30, 2^30): choose t_ref nearer the tree");
  S.first_cell = (int32_t)c_root; S.num_cells = (int32_t)cells; S.num_inner = cnt;
  HIP_TRY(S.k_bar.alloc_roomy((size_t)S.num_cells));
  hipLaunchKernelGGL(k_skygrid_tree_k_bar, dim3((unsigned)S.num_cells), dim3(k_sky_threads), 0, h->stream, T, t_ref, t_step, S.first_cell, S.num_cells, S.k_bar.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* skygrid_tau_move + skygrid_gammas_zero_mode_gibbs_move + skygrid_gammas_hmc_move on the device (header: emat_skygrid_moves) */
emat_status emat_skygrid_moves(emat_backend* h, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                               const double* k_bar, int32_t num_inner, const double* inner_t, uint64_t key, emat_skygrid_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_skygrid_moves: ";
  if (!pm || !spec || !k_bar || !inner_t || !out || !out->gamma) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec, k_bar, inner_t, out and out->gamma must not be null");
  HostPopModel hp;
  emat_status st = sky_check_model_and_spec(h, w, pm, spec, t_ref, t_step, out, hp); if (st) return st;
  if (num_cells < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_cells must be at least 1");
  if (num_inner < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_inner must be at least 1");
  for (int32_t c = 0; c < num_cells; ++c)
    if (!std::isfinite(k_bar[c]) || k_bar[c] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "k_bar of cell " + std::to_string(c) + " is negative or not finite");
  for (int32_t i = 0; i < num_inner; ++i) {
    if (!std::isfinite(inner_t[i])) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " is not finite");
    const double cell = std::floor((inner_t[i] - t_ref) / t_step);   // Scalable_coalescent_prior::cell_for
    if (cell < (double)first_cell || cell >= (double)first_cell + (double)num_cells) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " lies outside the grid");
  }
  st = sky_check_capacity(h, w, hp.x.size(), first_cell, num_cells); if (st) return st;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase, each kernel waited for on its own)
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }
  SkygridScratch& S = h->sky;
  HIP_TRY(S.k_bar.alloc_roomy((size_t)num_cells)); HIP_TRY(S.inner_t.alloc_roomy((size_t)num_inner));
  HIP_TRY(hipMemcpyAsync(S.k_bar.p, k_bar, (size_t)num_cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(S.inner_t.p, inner_t, (size_t)num_inner * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return sky_run(h, hp, *spec, t_ref, t_step, first_cell, num_cells, num_inner, key, out, laps);
}

/* the whole-tree statistics of the tree in HBM (header: emat_tree_coalescent_stats) */
emat_status emat_tree_coalescent_stats(emat_backend* h, double t_ref, double t_step, int32_t* first_cell, int32_t* num_cells, double* k_bar, int32_t k_bar_capacity,
                                       double* inner_t, int32_t inner_capacity, int32_t* num_inner) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_coalescent_stats: ";
  if (!first_cell || !num_cells || !num_inner) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "first_cell, num_cells and num_inner must not be null");
  if (!std::isfinite(t_ref) || !std::isfinite(t_step) || !(t_step > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t_ref must be finite and t_step finite and positive");
  emat_status st = sky_tree_stats(h, w, t_ref, t_step); if (st) return st;
  SkygridScratch& S = h->sky;
  *first_cell = S.first_cell; *num_cells = S.num_cells; *num_inner = S.num_inner;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (k_bar) {
    if (k_bar_capacity < S.num_cells) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, w + std::to_string(S.num_cells) + " cells, room for " + std::to_string(k_bar_capacity));
    HIP_TRY(hipMemcpy(k_bar, S.k_bar.p, (size_t)S.num_cells * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (inner_t) {
    if (inner_capacity < S.num_inner) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, w + std::to_string(S.num_inner) + " inner nodes, room for " + std::to_string(inner_capacity));
    HIP_TRY(hipMemcpy(inner_t, S.inner_t.p, (size_t)S.num_inner * sizeof(double), hipMemcpyDeviceToHost));
  }
  return EMAT_OK;
}

/* the moves on the statistics of the tree in HBM, which never leave it (header: emat_tree_skygrid_moves) */
emat_status emat_tree_skygrid_moves(emat_backend* h, const emat_pop_model* pm, const emat_skygrid_spec* spec, double t_ref, double t_step, uint64_t key, emat_skygrid_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_skygrid_moves: ";
  if (!pm || !spec || !out || !out->gamma) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "pop_model, spec, out and out->gamma must not be null");
  HostPopModel hp;
  emat_status st = sky_check_model_and_spec(h, w, pm, spec, t_ref, t_step, out, hp); if (st) return st;
  st = sky_check_capacity(h, w, hp.x.size(), 0, 1); if (st) return st;
  HostLaps laps;
  st = sky_tree_stats(h, w, t_ref, t_step); if (st) return st;
  SkygridScratch& S = h->sky;
  if (S.num_inner < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the resident tree has no inner node");
  return sky_run(h, hp, *spec, t_ref, t_step, S.first_cell, S.num_cells, S.num_inner, key, out, laps);
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
