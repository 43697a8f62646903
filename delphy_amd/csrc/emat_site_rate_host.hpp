// emat_site_rate_host.hpp -- the site-rate moves' entry points: emat_site_rate_moves, emat_get_nu_l and the sampler's test hook.
//
// Included by emat_backend.hip after the product entry points (the kernels: emat_site_rate_kernels.hpp).
#ifndef EMAT_SITE_RATE_HOST_HPP_
#define EMAT_SITE_RATE_HOST_HPP_

extern "C" {

/* alpha_moves + gibbs_sample_all_nus on the device (header: emat_site_rate_moves) */
emat_status emat_site_rate_moves(emat_backend* h, const double* Ttwiddle_l, const int32_t* num_muts_l, double alpha, int32_t num_alpha_steps, uint64_t key, emat_site_rate_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_site_rate_moves: ";
  if (!Ttwiddle_l || !num_muts_l || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_l, num_muts_l and out must not be null");
  if (!finite_positive(alpha)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "alpha must be finite and positive");
  if (num_alpha_steps < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_alpha_steps must not be negative");
  if (out->trace && out->trace_capacity < num_alpha_steps) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than num_alpha_steps");
  const size_t L = (size_t)h->L;
  for (size_t l = 0; l < L; ++l) {
    if (!std::isfinite(Ttwiddle_l[l]) || Ttwiddle_l[l] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_l of site " + std::to_string(l) + " is negative or not finite");
    if (num_muts_l[l] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_muts_l of site " + std::to_string(l) + " is negative");
  }
  if (h->host_only) return no_device(h);
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_site_rate_moves");
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase, each kernel waited for on its own)
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }   // a pass in flight reads d_nu
  emat_status st = sync_model_to_device(h); if (st) return st;                   // mu, the site partitions and the old rates
  SiteRateScratch& S = h->sr;
  HIP_TRY(S.T.upload(Ttwiddle_l, L)); HIP_TRY(S.M.upload(num_muts_l, L));
  HIP_TRY(S.nu_new.alloc(L)); HIP_TRY(S.d_log_G.alloc(L)); HIP_TRY(S.d_prior.alloc(L)); HIP_TRY(S.result.alloc((size_t)k_sr_result_doubles));
  const bool want_trace = out->trace != nullptr && num_alpha_steps > 0;
  if (want_trace) HIP_TRY(S.trace.alloc_roomy((size_t)num_alpha_steps));
  SiteRateArgs a{};
  a.L = h->L; a.Ttwiddle_l = S.T.p; a.num_muts_l = S.M.p; a.mu = h->d_mu.p; a.partition_for_site = h->d_part.p; a.nu_old = h->d_nu.p;
  a.nu_new = S.nu_new.p; a.d_log_G_l = S.d_log_G.p; a.d_prior_l = S.d_prior.p; a.result = S.result.p; a.trace = want_trace ? S.trace.p : nullptr;
  a.alpha = alpha; a.num_alpha_steps = num_alpha_steps; a.key = key;
  laps.mark("site_rate_moves: 1 finish_pass, model and statistics to the device");
  hipLaunchKernelGGL(k_site_rate_alpha, dim3(1), dim3(k_sr_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  if (laps.on) { HIP_TRY(hipStreamSynchronize(h->stream)); laps.mark("site_rate_moves: 2 k_site_rate_alpha"); }
  hipLaunchKernelGGL(k_site_rate_gibbs, dim3((unsigned)((L + k_sr_gibbs_threads - 1) / k_sr_gibbs_threads)), dim3(k_sr_gibbs_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_site_rate_sums, dim3(1), dim3(k_sr_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark(laps.on ? "site_rate_moves: 3 k_site_rate_gibbs + k_site_rate_sums" : "site_rate_moves: 2-3 the three kernels");
  double res[k_sr_result_doubles];
  std::vector<double> nu_new(L);
  HIP_TRY(hipMemcpy(res, S.result.p, sizeof res, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nu_new.data(), S.nu_new.p, L * sizeof(double), hipMemcpyDeviceToHost));
  if (want_trace) HIP_TRY(hipMemcpy(out->trace, S.trace.p, (size_t)num_alpha_steps * sizeof(emat_site_rate_step), hipMemcpyDeviceToHost));
  out->alpha = res[k_sr_alpha]; out->log_p_alpha_start = res[k_sr_log_p_start];
  out->num_accepted = (int32_t)res[k_sr_num_accepted]; out->num_floored = (int32_t)res[k_sr_num_floored];
  out->delta_log_G = res[k_sr_d_log_G]; out->delta_log_prior_alpha = res[k_sr_d_prior_alpha]; out->delta_log_prior_nu = res[k_sr_d_prior_nu];
  out->sum_nu_old = res[k_sr_sum_nu_old2]; out->sum_nu_new = res[k_sr_sum_nu_new];
  // the new rates become the model's
  h->nu_l.swap(nu_new);
  install_model(h);
  laps.mark("site_rate_moves: 4 copy-back + refresh_ref_derived");
  return EMAT_OK;
}

emat_status emat_get_nu_l(emat_backend* h, double* nu_l) {
  if (!h || !nu_l) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_get_nu_l");
  std::copy(h->nu_l.begin(), h->nu_l.end(), nu_l);
  return EMAT_OK;
}

/* test hook (header: emat_debug_sample_gamma) */
emat_status emat_debug_sample_gamma(emat_backend* h, uint64_t key, int32_t n, double shape, double rate, double* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (n < 0 || (n > 0 && !out) || !std::isfinite(shape) || !(shape > 0.0) || !std::isfinite(rate) || !(rate > 0.0))
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_sample_gamma: n >= 0, an output array, and a finite positive shape and rate");
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return EMAT_OK;
  DevBuf<double> d_out;
  HIP_TRY(d_out.alloc((size_t)n));
  hipLaunchKernelGGL(k_debug_sample_gamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, key, n, shape, rate, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_SITE_RATE_HOST_HPP_
