// emat_subst_host.hpp -- the substitution-model moves' entry points: emat_subst_moves and emat_parts_subst_moves.
//
// Included by emat_backend.hip after emat_subst_stats_host.hpp: the statistics record, its checks, the frame of a call on it (the kernel: emat_subst_kernels.hpp; the spec's checks and the q of a model: emat_move_specs.hpp).
#ifndef EMAT_SUBST_HOST_HPP_
#define EMAT_SUBST_HOST_HPP_

namespace {

const char* const k_sb_bad_posterior_text = "the mu draw needs a positive shape (num_muts + mu_prior_alpha) and a positive rate (sum of q_a Ttwiddle_beta_a + mu_prior_beta)";
const char* const k_sb_marks[3] = {"subst_moves: 1 finish_pass, statistics", "subst_moves: 2 k_subst_moves", "subst_moves: 3 copy-back + refresh_ref_derived"};   // the call's spans

// Both entry points: check the arguments, obtain the statistics (`host`, or those of the parts on the handle where it is null), run, install the model.
emat_status sb_moves(emat_backend* h, const std::string& w, const emat_subst_spec* spec, const SubstHostStats* host, uint64_t key, emat_subst_result* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!spec || (host && (!host->T || !host->M || !host->C)) || !out) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "spec" + (host ? ", Ttwiddle_beta_a, num_muts_beta_ab, root_state_counts" : "") + " and out must not be null");
  if (const char* why = subst_spec_fault(*spec)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + why);
  if (out->trace && (int64_t)out->trace_capacity < 2 * (int64_t)spec->rounds) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "trace_capacity is smaller than 2 * rounds");
  if (spec->rounds > k_one_wave_max_rounds) return fail(h, EMAT_ERR_CAPACITY, w + rounds_beyond_text(spec->rounds, k_one_wave_max_rounds));
  double record[k_sb_stats_doubles] = {};
  if (host) {
    if (host->P > k_max_stats_partitions) return fail(h, EMAT_ERR_CAPACITY, w + "at most 4 site partitions");
    if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_subst_moves");
    if (host->P != h->num_partitions) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_partitions does not match emat_set_evo");
    double num_muts = 0.0;
    emat_status st = sbs_check_host_values(h, w, *host, record, &num_muts); if (st) return st;
    if (spec->do_mu) {   // run.cpp:797-810 on the model passed in
      double q[16]; hky_derive_q(spec->kappa, spec->pi, q);
      double Ttwiddle = 0.0;
      for (int k = 0; k < 4 * host->P; ++k) Ttwiddle += -q[5 * (k % 4)] * host->T[k];
      if (!(num_muts + spec->mu_prior_alpha > 0.0) || !(Ttwiddle + spec->mu_prior_beta > 0.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + k_sb_bad_posterior_text);
    }
  } else { emat_status st = sb_check_parts(h, w); if (st) return st; }
  HostLaps laps;   // (EMAT_VERBOSE=spans: the call by phase)
  SubstArgs a{};
  a.spec = *spec; a.P = h->num_partitions; a.key = key;
  double r[k_sb_result_doubles];
  emat_status st = one_wave_on_record(h, w, laps, k_sb_marks, host ? record : nullptr, h->sb, k_subst_moves, k_sb_threads, a, out->trace, 2 * spec->rounds, r, k_sb_bad_posterior, k_sb_bad_posterior_text); if (st) return st;
  out->mu = r[k_sb_mu]; out->kappa = r[k_sb_kappa]; for (int s = 0; s < 4; ++s) out->pi[s] = r[k_sb_pi + s];
  out->mu_post_shape = r[k_sb_shape]; out->mu_post_rate = r[k_sb_rate]; out->mu_draw = r[k_sb_draw];
  out->delta_log_G = r[k_sb_d_log_G]; out->delta_log_other_priors = r[k_sb_d_other_priors]; out->mu_delta_log_G = r[k_sb_mu_d_log_G]; out->mu_delta_log_other_priors = r[k_sb_mu_d_other_priors];
  out->pi_accepted = (int32_t)r[k_sb_pi_accepted]; out->kappa_accepted = (int32_t)r[k_sb_kappa_accepted]; out->pi_left_unit = (int32_t)r[k_sb_pi_left_unit]; out->forced_rejections = (int32_t)r[k_sb_forced];
  // the new model becomes the handle's: mu, pi and q of every partition
  for (int p = 0; p < h->num_partitions; ++p) {
    h->mu[(size_t)p] = out->mu;
    for (int s = 0; s < 4; ++s) h->pi[(size_t)p * 4 + s] = out->pi[s];
    hky_derive_q(out->kappa, out->pi, &h->q[(size_t)p * 16]);
  }
  install_model(h);
  laps.mark(k_sb_marks[2]);
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

}  // extern "C"

#endif  // EMAT_SUBST_HOST_HPP_
