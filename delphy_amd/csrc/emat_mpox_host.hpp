// emat_mpox_host.hpp -- the APOBEC (mpox) model's moves' entry points: emat_mpox_moves and emat_parts_mpox_moves.
//
// Included by emat_backend.hip after emat_subst_stats_host.hpp: the statistics record, its checks, the frame of a call on it (the kernel: emat_mpox_kernels.hpp; the spec's checks and the q of a model: emat_move_specs.hpp).
#ifndef EMAT_MPOX_HOST_HPP_
#define EMAT_MPOX_HOST_HPP_

namespace {

const char* const k_mx_bad_posterior_text = "the mu draw needs a positive shape (num_muts + mu_prior_alpha - 1) and a positive rate (Ttwiddle + 2 rho Ttwiddle* + mu_prior_beta)";
const char* const k_mx_marks[3] = {"mpox_moves: 1 finish_pass, statistics", "mpox_moves: 2 k_mpox_moves", "mpox_moves: 3 copy-back + refresh_ref_derived"};   // the call's spans

// Both entry points: check the arguments, obtain the statistics (`host`, of 2 site partitions and without root counts, or those of the parts on the handle where it
// is null), run, install the model.
emat_status mx_moves(emat_backend* h, const std::string& w, const emat_mpox_spec* spec, const SubstHostStats* host, uint64_t key, emat_mpox_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!spec || (host && (!host->T || !host->M)) || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "spec" + (host ? ", Ttwiddle_beta_a, num_muts_beta_ab" : "") + " and out must not be null");
  if (const char* why = mpox_spec_fault(*spec)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && (int64_t)out->trace_capacity < (int64_t)spec->rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than rounds");
  if (spec->rounds > k_one_wave_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + rounds_beyond_text(spec->rounds, k_one_wave_max_rounds));
  if (h->have_evo && h->num_partitions != 2) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the model on the handle has " + std::to_string(h->num_partitions) + " site partitions, the APOBEC model has 2");
  double record[k_sb_stats_doubles] = {};
  if (host) {
    double num_muts = 0.0;
    emat_status st = sbs_check_host_values(h, w, *host, record, &num_muts); if (st) return st;
    if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_mpox_moves");
    if (spec->do_mu && spec->rounds > 0) {   // run.cpp:897-918 for the first round, on the model passed in
      double Ttwiddle = 0.0;
      for (int k = 0; k < 8; ++k) Ttwiddle += host->T[k];
      const double rho = spec->mu_star / spec->mu, Ttwiddle_eff = Ttwiddle + 2 * rho * (host->T[4 + 1] + host->T[4 + 2]);
      if (!(num_muts + spec->mu_prior_alpha - 1.0 > 0.0) || !(Ttwiddle_eff + spec->mu_prior_beta > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_mx_bad_posterior_text);
    }
  } else { emat_status st = sb_check_parts(h, w); if (st) return st; }
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  MpoxArgs a{};
  a.spec = *spec; a.key = key;
  double r[k_mx_result_doubles];
  emat_status st = one_wave_on_record(h, w, laps, k_mx_marks, host ? record : nullptr, h->mx, k_mpox_moves, k_mx_threads, a, out->trace, spec->rounds, r, k_mx_bad_posterior, k_mx_bad_posterior_text); if (st) return st;
  out->mu = r[k_mx_mu]; out->mu_star = r[k_mx_mu_star];
  out->M = r[k_mx_M]; out->M_star = r[k_mx_M_star]; out->Ttwiddle = r[k_mx_T]; out->Ttwiddle_star = r[k_mx_T_star];
  out->delta_log_G = r[k_mx_d_log_G]; out->delta_log_other_priors = r[k_mx_d_other_priors];
  out->rho_skipped = (int32_t)r[k_mx_rho_skipped]; out->rho_degenerate = (int32_t)r[k_mx_rho_degenerate];
  // the new model becomes the handle's (Run::derive_evo, run.cpp:407-432): mu and pi = 0.25 of both partitions, q0 and q1 of rho
  for (int p = 0; p < 2; ++p) {
    h->mu[(size_t)p] = out->mu;
    for (int s = 0; s < 4; ++s) h->pi[(size_t)p * 4 + s] = 0.25;
  }
  mpox_derive_q(out->mu_star / out->mu, &h->q[0], &h->q[16]);
  install_model(h);
  laps.mark(k_mx_marks[2]);
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* Run::mpox_hack_moves on the device (header: emat_mpox_moves) */
emat_status emat_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, const double* Ttwiddle_beta_a, const int64_t* num_muts_beta_ab, uint64_t key, emat_mpox_result* out) {
  const SubstHostStats host{2, Ttwiddle_beta_a, num_muts_beta_ab, nullptr};
  return mx_moves(h, "emat_mpox_moves: ", spec, &host, key, out);
}

/* the moves on the statistics of the parts on the handle, which never leave it (header: emat_parts_mpox_moves) */
emat_status emat_parts_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, uint64_t key, emat_mpox_result* out) {
  return mx_moves(h, "emat_parts_mpox_moves: ", spec, nullptr, key, out);
}

}  // extern "C"

#endif  // EMAT_MPOX_HOST_HPP_
