// emat_mpox_host.hpp -- the APOBEC (mpox) model's moves' entry points: emat_mpox_moves and emat_parts_mpox_moves.
//
// Included by emat_backend.hip after emat_subst_host.hpp, whose statistics of the parts (sb_queue_parts_stats, sb_check_parts) these read (the kernel:
// emat_mpox_kernels.hpp; the spec's checks and the q of a model: emat_move_specs.hpp).
#ifndef EMAT_MPOX_HOST_HPP_
#define EMAT_MPOX_HOST_HPP_

namespace {

const char* const k_mx_bad_posterior_text = "the mu draw needs a positive shape (num_muts + mu_prior_alpha - 1) and a positive rate (Ttwiddle + 2 rho Ttwiddle* + mu_prior_beta)";

struct MpoxHostStats { const double* T; const int64_t* M; };

// Both entry points: check the arguments, obtain the statistics (`host`, or those of the parts on the handle where it is null), run, install the model.
emat_status mx_moves(emat_backend* h, const std::string& w, const emat_mpox_spec* spec, const MpoxHostStats* host, uint64_t key, emat_mpox_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!spec || (host && (!host->T || !host->M)) || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "spec" + (host ? ", Ttwiddle_beta_a, num_muts_beta_ab" : "") + " and out must not be null");
  if (const char* why = mpox_spec_fault(*spec)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && (int64_t)out->trace_capacity < (int64_t)spec->rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than rounds");
  if (spec->rounds > k_mpox_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(spec->rounds) + " rounds are more than the moves hold (" + std::to_string(k_mpox_max_rounds) + ")");
  if (h->have_evo && h->num_partitions != 2) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the model on the handle has " + std::to_string(h->num_partitions) + " site partitions, the APOBEC model has 2");
  double stats[k_sb_stats_doubles] = {};
  if (host) {
    for (int k = 0; k < 8; ++k) {
      if (!std::isfinite(host->T[k]) || host->T[k] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_beta_a[" + std::to_string(k / 4) + "][" + std::to_string(k % 4) + "] is negative or not finite");
      stats[k_sb_T + k] = host->T[k];
    }
    double num_muts = 0.0;
    for (int k = 0; k < 32; ++k) {
      if (host->M[k] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_muts_beta_ab[" + std::to_string(k / 16) + "][" + std::to_string(k / 4 % 4) + "][" + std::to_string(k % 4) + "] is negative");
      stats[k_sb_M + k] = (double)host->M[k];
      if (k / 4 % 4 != k % 4) num_muts += (double)host->M[k];
    }
    if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_mpox_moves");
    if (spec->do_mu && spec->rounds > 0) {   // run.cpp:897-918 for the first round, on the model passed in
      double Ttwiddle = 0.0;
      for (int k = 0; k < 8; ++k) Ttwiddle += host->T[k];
      const double rho = spec->mu_star / spec->mu, Ttwiddle_eff = Ttwiddle + 2 * rho * (host->T[4 + 1] + host->T[4 + 2]);
      if (!(num_muts + spec->mu_prior_alpha - 1.0 > 0.0) || !(Ttwiddle_eff + spec->mu_prior_beta > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_mx_bad_posterior_text);
    }
  } else { emat_status st = sb_check_parts(h, w); if (st) return st; }
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }   // a pass in flight reads the model
  if (host) HIP_TRY(h->sb.stats.upload(stats, (size_t)k_sb_stats_doubles));
  else { emat_status st = sb_queue_parts_stats(h, w); if (st) return st; }
  MpoxScratch& S = h->mx;
  const int rounds = spec->rounds;
  const bool want_trace = out->trace != nullptr && rounds > 0;
  HIP_TRY(S.result.alloc((size_t)k_mx_result_doubles));
  if (want_trace) HIP_TRY(S.trace.alloc_roomy((size_t)rounds));
  MpoxArgs a{};
  a.spec = *spec; a.stats = h->sb.stats.p; a.key = key; a.trace = want_trace ? S.trace.p : nullptr; a.result = S.result.p;
  if (laps.on) HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("mpox_moves: 1 finish_pass, statistics");
  hipLaunchKernelGGL(k_mpox_moves, dim3(1), dim3(k_mx_threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark("mpox_moves: 2 k_mpox_moves");
  double r[k_mx_result_doubles];
  HIP_TRY(hipMemcpy(r, S.result.p, sizeof r, hipMemcpyDeviceToHost));
  if (r[k_mx_bad_posterior] != 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_mx_bad_posterior_text);
  if (want_trace) HIP_TRY(hipMemcpy(out->trace, S.trace.p, (size_t)rounds * sizeof(emat_mpox_round), hipMemcpyDeviceToHost));
  out->mu = r[k_mx_mu]; out->mu_star = r[k_mx_mu_star];
  out->M = r[k_mx_M]; out->M_star = r[k_mx_M_star]; out->Ttwiddle = r[k_mx_T]; out->Ttwiddle_star = r[k_mx_T_star];
  out->delta_log_G = r[k_mx_d_log_G]; out->delta_log_other_priors = r[k_mx_d_other_priors];
  out->rho_skipped = (int32_t)r[k_mx_rho_skipped]; out->rho_degenerate = (int32_t)r[k_mx_rho_degenerate];
  // the new model becomes the handle's, by emat_set_evo's rules (Run::derive_evo, run.cpp:407-432): mu and pi = 0.25 of both partitions, q0 and q1 of rho;
  // nu_l, the site partitions and the reference sequence stay
  for (int p = 0; p < 2; ++p) {
    h->mu[(size_t)p] = out->mu;
    for (int s = 0; s < 4; ++s) h->pi[(size_t)p * 4 + s] = 0.25;
  }
  mpox_derive_q(out->mu_star / out->mu, &h->q[0], &h->q[16]);
  refresh_ref_derived(h);
  h->model_changed();
  laps.mark("mpox_moves: 3 copy-back + refresh_ref_derived");
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* Run::mpox_hack_moves on the device (header: emat_mpox_moves) */
emat_status emat_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, const double* Ttwiddle_beta_a, const int64_t* num_muts_beta_ab, uint64_t key, emat_mpox_result* out) {
  const MpoxHostStats host{Ttwiddle_beta_a, num_muts_beta_ab};
  return mx_moves(h, "emat_mpox_moves: ", spec, &host, key, out);
}

/* the moves on the statistics of the parts on the handle, which never leave it (header: emat_parts_mpox_moves) */
emat_status emat_parts_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, uint64_t key, emat_mpox_result* out) {
  return mx_moves(h, "emat_parts_mpox_moves: ", spec, nullptr, key, out);
}

}  // extern "C"

#endif  // EMAT_MPOX_HOST_HPP_
