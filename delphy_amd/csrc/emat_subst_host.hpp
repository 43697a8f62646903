// emat_subst_host.hpp -- the substitution-model moves' entry points: emat_subst_moves, emat_parts_subst_stats, emat_parts_subst_moves and emat_get_evo.
//
// Included by emat_backend.hip after emat_exp_pop_host.hpp (the kernels: emat_subst_kernels.hpp; the spec's checks and the q of a model: emat_move_specs.hpp).
#ifndef EMAT_SUBST_HOST_HPP_
#define EMAT_SUBST_HOST_HPP_

namespace {

const char* const k_sb_bad_posterior_text = "the mu draw needs a positive shape (num_muts + mu_prior_alpha) and a positive rate (sum of q_a Ttwiddle_beta_a + mu_prior_beta)";

// The statistics of the parts on the handle into h->sb.stats, queued on the engine's stream: k_global_stats' rows reduced in a fixed order, the root
// part's root counts.  The caller has checked the model, the parts and the root part; nothing here waits for the device.
emat_status sb_queue_parts_stats(emat_backend* h, const std::string& w) {
  emat_status st = require_settled_parts(h); if (st) return st;
  const int W = 4 * h->num_partitions;
  for (auto& ph : h->parts)   // k_global_stats' per-node table lives in the part's scratch region
    if ((uint64_t)ph.n_nodes * W * 8u > (uint64_t)ph.scratch_bytes) return fail(h, EMAT_ERR_CAPACITY, w + "scratch region too small for the statistics table");
  const size_t n = h->parts.size();
  if (h->d_stats.n < n * k_stats_row) { std::vector<double> z(n * k_stats_row, 0.0); HIP_TRY(h->d_stats.upload(z.data(), z.size())); }
  HIP_TRY(h->sb.stats.alloc((size_t)k_sb_stats_doubles));
  hipLaunchKernelGGL(k_global_stats, dim3((unsigned)n), dim3(k_wave), 0, h->stream, make_args(h));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_subst_reduce_stats, dim3((unsigned)k_sb_C), dim3(k_sb_reduce_threads), 0, h->stream, (const double*)h->d_stats.p, (int)n, h->num_partitions, h->sb.stats.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_subst_root_counts, dim3(1), dim3(k_sb_reduce_threads), 0, h->stream, make_args(h), h->root_part, h->sb.stats.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

// What both parts calls refuse, after the arguments and before the device is asked for.
emat_status sb_check_parts(emat_backend* h, const std::string& w) {
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede " + w.substr(0, w.size() - 2));
  if (h->num_partitions > k_max_stats_partitions) return fail(h, EMAT_ERR_CAPACITY, w + "at most 4 site partitions");
  if (h->parts.empty() || h->uploads_expected != 0) return fail(h, EMAT_ERR_STATE, w + "no parts are out on this handle");
  if (h->root_part < 0) return fail(h, EMAT_ERR_STATE, w + "the root part is not on this handle");
  return EMAT_OK;
}

struct SubstHostStats { int32_t num_partitions; const double* T; const int64_t* M; const int64_t* C; };

// Both entry points: check the arguments, obtain the statistics (`host`, or those of the parts on the handle where it is null), run, install the model.
emat_status sb_moves(emat_backend* h, const std::string& w, const emat_subst_spec* spec, const SubstHostStats* host, uint64_t key, emat_subst_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!spec || (host && (!host->T || !host->M || !host->C)) || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "spec" + (host ? ", Ttwiddle_beta_a, num_muts_beta_ab, root_state_counts" : "") + " and out must not be null");
  if (const char* why = subst_spec_fault(*spec)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && (int64_t)out->trace_capacity < 2 * (int64_t)spec->rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than 2 * rounds");
  if (spec->rounds > k_subst_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(spec->rounds) + " rounds are more than the moves hold (" + std::to_string(k_subst_max_rounds) + ")");
  double stats[k_sb_stats_doubles] = {};
  if (host) {
    const int P = host->num_partitions;
    if (P > k_max_stats_partitions) return fail(h, EMAT_ERR_CAPACITY, w + "at most 4 site partitions");
    if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_subst_moves");
    if (P != h->num_partitions) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_partitions does not match emat_set_evo");
    for (int k = 0; k < 4 * P; ++k) {
      if (!std::isfinite(host->T[k]) || host->T[k] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_beta_a[" + std::to_string(k / 4) + "][" + std::to_string(k % 4) + "] is negative or not finite");
      stats[k_sb_T + k] = host->T[k];
    }
    double num_muts = 0.0;
    for (int k = 0; k < 16 * P; ++k) {
      if (host->M[k] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_muts_beta_ab[" + std::to_string(k / 16) + "][" + std::to_string(k / 4 % 4) + "][" + std::to_string(k % 4) + "] is negative");
      stats[k_sb_M + k] = (double)host->M[k];
      if (k / 4 % 4 != k % 4) num_muts += (double)host->M[k];
    }
    for (int s = 0; s < 4; ++s) {
      if (host->C[s] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "root_state_counts[" + std::to_string(s) + "] is negative");
      stats[k_sb_C + s] = (double)host->C[s];
    }
    if (spec->do_mu) {   // run.cpp:797-810 on the model passed in
      double q[16]; hky_derive_q(spec->kappa, spec->pi, q);
      double Ttwiddle = 0.0;
      for (int k = 0; k < 4 * P; ++k) Ttwiddle += -q[5 * (k % 4)] * host->T[k];
      if (!(num_muts + spec->mu_prior_alpha > 0.0) || !(Ttwiddle + spec->mu_prior_beta > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_sb_bad_posterior_text);
    }
  } else { emat_status st = sb_check_parts(h, w); if (st) return st; }
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }   // a pass in flight reads the model
  SubstScratch& S = h->sb;
  if (host) HIP_TRY(S.stats.upload(stats, (size_t)k_sb_stats_doubles));
  else { emat_status st = sb_queue_parts_stats(h, w); if (st) return st; }
  const int steps = 2 * spec->rounds;
  const bool want_trace = out->trace != nullptr && steps > 0;
  HIP_TRY(S.result.alloc((size_t)k_sb_result_doubles));
  if (want_trace) HIP_TRY(S.trace.alloc_roomy((size_t)steps));
  SubstArgs a{};
  a.spec = *spec; a.P = h->num_partitions; a.stats = S.stats.p; a.key = key; a.trace = want_trace ? S.trace.p : nullptr; a.result = S.result.p;
  if (laps.on) HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("subst_moves: 1 finish_pass, statistics");
  hipLaunchKernelGGL(k_subst_moves, dim3(1), dim3(k_sb_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("subst_moves: 2 k_subst_moves");
  double r[k_sb_result_doubles];
  HIP_TRY(hipMemcpy(r, S.result.p, sizeof r, hipMemcpyDeviceToHost));
  if (r[k_sb_bad_posterior] != 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_sb_bad_posterior_text);
  if (want_trace) HIP_TRY(hipMemcpy(out->trace, S.trace.p, (size_t)steps * sizeof(emat_subst_step), hipMemcpyDeviceToHost));
  out->mu = r[k_sb_mu]; out->kappa = r[k_sb_kappa]; for (int s = 0; s < 4; ++s) out->pi[s] = r[k_sb_pi + s];
  out->mu_post_shape = r[k_sb_shape]; out->mu_post_rate = r[k_sb_rate]; out->mu_draw = r[k_sb_draw];
  out->delta_log_G = r[k_sb_d_log_G]; out->delta_log_other_priors = r[k_sb_d_other_priors]; out->mu_delta_log_G = r[k_sb_mu_d_log_G]; out->mu_delta_log_other_priors = r[k_sb_mu_d_other_priors];
  out->pi_accepted = (int32_t)r[k_sb_pi_accepted]; out->kappa_accepted = (int32_t)r[k_sb_kappa_accepted]; out->pi_left_unit = (int32_t)r[k_sb_pi_left_unit]; out->forced_rejections = (int32_t)r[k_sb_forced];
  // the new model becomes the handle's, by emat_set_evo's rules: mu, pi and q of every partition; nu_l, the site partitions and the reference sequence stay
  for (int p = 0; p < h->num_partitions; ++p) {
    h->mu[(size_t)p] = out->mu;
    for (int s = 0; s < 4; ++s) h->pi[(size_t)p * 4 + s] = out->pi[s];
    hky_derive_q(out->kappa, out->pi, &h->q[(size_t)p * 16]);
  }
  refresh_ref_derived(h);
  h->model_changed();
  laps.mark("subst_moves: 3 copy-back + refresh_ref_derived");
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* mu_move, then `rounds` times hky_frequencies_move + hky_kappa_move, on the device (header: emat_subst_moves) */
emat_status emat_subst_moves(emat_backend* h, const emat_subst_spec* spec, int32_t num_partitions, const double* Ttwiddle_beta_a, const int64_t* num_muts_beta_ab,
                             const int64_t* root_state_counts, uint64_t key, emat_subst_result* out) {
  const SubstHostStats host{num_partitions, Ttwiddle_beta_a, num_muts_beta_ab, root_state_counts};
  return sb_moves(h, "emat_subst_moves: ", spec, &host, key, out);
}

/* the moves on the statistics of the parts on the handle, which never leave it (header: emat_parts_subst_moves) */
emat_status emat_parts_subst_moves(emat_backend* h, const emat_subst_spec* spec, uint64_t key, emat_subst_result* out) {
  return sb_moves(h, "emat_parts_subst_moves: ", spec, nullptr, key, out);
}

/* the statistics emat_parts_subst_moves reads (header: emat_parts_subst_stats) */
emat_status emat_parts_subst_stats(emat_backend* h, double* Ttwiddle_beta_a, int64_t* num_muts_beta_ab, int64_t* root_state_counts) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_parts_subst_stats: ";
  if (!Ttwiddle_beta_a || !num_muts_beta_ab || !root_state_counts) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_beta_a, num_muts_beta_ab and root_state_counts must not be null");
  emat_status st = sb_check_parts(h, w); if (st) return st;
  if (h->host_only) return no_device(h);
  st = sb_queue_parts_stats(h, w); if (st) return st;
  HIP_TRY(hipStreamSynchronize(h->stream));
  double stats[k_sb_stats_doubles];
  HIP_TRY(hipMemcpy(stats, h->sb.stats.p, sizeof stats, hipMemcpyDeviceToHost));
  const int P = h->num_partitions;
  for (int k = 0; k < 4 * P; ++k) Ttwiddle_beta_a[k] = stats[k_sb_T + k];
  for (int k = 0; k < 16 * P; ++k) num_muts_beta_ab[k] = (int64_t)stats[k_sb_M + k];
  for (int s = 0; s < 4; ++s) root_state_counts[s] = (int64_t)stats[k_sb_C + s];
  return EMAT_OK;
}

/* the model the handle holds (header: emat_get_evo) */
emat_status emat_get_evo(emat_backend* h, int32_t* num_partitions, double* mu, double* pi, double* q) {
  if (!h || !num_partitions) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_get_evo");
  const int P = h->num_partitions, room = *num_partitions;
  *num_partitions = P;
  if (room < P && (mu || pi || q)) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_get_evo: room for fewer site partitions than the model has");
  if (mu) std::copy(h->mu.begin(), h->mu.end(), mu);
  if (pi) std::copy(h->pi.begin(), h->pi.end(), pi);
  if (q) std::copy(h->q.begin(), h->q.end(), q);
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_SUBST_HOST_HPP_
