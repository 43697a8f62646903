// emat_subst_stats_host.hpp -- the substitution statistics of the parts that the substitution-model moves and the APOBEC model's moves read (h->sbs): a caller's
// statistics and their checks, those of the parts on the handle, and the frame of a one-wave group that runs on the record.
//
// Included by emat_backend.hip before the two groups (emat_subst_host.hpp, emat_mpox_host.hpp); the record's layout and the kernels that reduce it: emat_subst_kernels.hpp.
#ifndef EMAT_SUBST_STATS_HOST_HPP_
#define EMAT_SUBST_STATS_HOST_HPP_

namespace {

// Statistics in the caller's arrays: T [P][4], M [P][4][4], C [4] (null for the APOBEC group, which has no root term); a null pointer to one of these stands for
// "the parts on the handle".
struct SubstHostStats { int32_t P; const double* T; const int64_t* M; const int64_t* C; };

// What handed-in statistics must be, T, then M, then C: each check fills its share of `record`, the host's image of the record (k_sb_stats_doubles doubles that start
// at zero), as it goes.  `num_muts`: the sum of M off the diagonals, which both groups' mu posteriors begin with.
emat_status sbs_check_host_values(emat_backend* h, const std::string& w, const SubstHostStats& s, double* record, double* num_muts) {
  for (int k = 0; k < 4 * s.P; ++k) {
    if (!std::isfinite(s.T[k]) || s.T[k] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_beta_a[" + std::to_string(k / 4) + "][" + std::to_string(k % 4) + "] is negative or not finite");
    record[k_sb_T + k] = s.T[k];
  }
  *num_muts = 0.0;
  for (int k = 0; k < 16 * s.P; ++k) {
    if (s.M[k] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_muts_beta_ab[" + std::to_string(k / 16) + "][" + std::to_string(k / 4 % 4) + "][" + std::to_string(k % 4) + "] is negative");
    record[k_sb_M + k] = (double)s.M[k];
    if (k / 4 % 4 != k % 4) *num_muts += (double)s.M[k];
  }
  for (int a = 0; s.C && a < 4; ++a) {
    if (s.C[a] < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "root_state_counts[" + std::to_string(a) + "] is negative");
    record[k_sb_C + a] = (double)s.C[a];
  }
  return EMAT_OK;
}

// What every call on the parts' own statistics refuses, after the arguments and before the device is asked for.
emat_status sb_check_parts(emat_backend* h, const std::string& w) {
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede " + w.substr(0, w.size() - 2));
  if (h->num_partitions > k_max_stats_partitions) return fail(h, EMAT_ERR_CAPACITY, w + "at most 4 site partitions");
  if (h->parts.empty() || h->uploads_expected != 0) return fail(h, EMAT_ERR_STATE, w + "no parts are out on this handle");
  if (h->root_part < 0) return fail(h, EMAT_ERR_STATE, w + "the root part is not on this handle");
  return EMAT_OK;
}

// The statistics of the parts on the handle into the record, queued on the engine's stream: k_global_stats' rows reduced in a fixed order, the root
// part's root counts.  The caller has checked the model, the parts and the root part (sb_check_parts); nothing here waits for the device.
emat_status sb_queue_parts_stats(emat_backend* h, const std::string& w) {
  emat_status st = require_settled_parts(h); if (st) return st;
  const int W = 4 * h->num_partitions;
  for (auto& ph : h->parts)   // k_global_stats' per-node table lives in the part's scratch region
    if ((uint64_t)ph.n_nodes * W * 8u > (uint64_t)ph.scratch_bytes) return fail(h, EMAT_ERR_CAPACITY, w + "scratch region too small for the statistics table");
  const size_t n = h->parts.size();
  if (h->d_stats.n < n * k_stats_row) { std::vector<double> z(n * k_stats_row, 0.0); HIP_TRY(h->d_stats.upload(z.data(), z.size())); }
  HIP_TRY(h->sbs.record.alloc((size_t)k_sb_stats_doubles));
  hipLaunchKernelGGL(k_global_stats, dim3((unsigned)n), dim3(k_wave), 0, h->stream, make_args(h));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_subst_reduce_stats, dim3((unsigned)k_sb_C), dim3(k_sb_reduce_threads), 0, h->stream, (const double*)h->d_stats.p, (int)n, h->num_partitions, h->sbs.record.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_subst_root_counts, dim3(1), dim3(k_sb_reduce_threads), 0, h->stream, make_args(h), h->root_part, h->sbs.record.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

// THE frame of a group that runs as one wavefront on the record, after its checks: entering the device (a handle that has one, bound, no pass in flight, which reads
// the model; the call's spans begin once it is bound), obtaining the record (the caller's checked `record` uploaded, or the parts' queued where it is null), room for
// the result and, where asked for, the trace, the launch, the result's doubles into `r`, the first mu posterior that only the device could refuse (r[bad_posterior]),
// the trace into the caller's room.  `marks`: the call's three spans (EMAT_VERBOSE=spans); the third is the caller's, after it has installed the model.
template <class Step, class Args, size_t N>
emat_status one_wave_on_record(emat_backend* h, const std::string& w, HostLaps& laps, const char* const (&marks)[3], const double* record, OneWaveScratch<Step>& S, void (*kernel)(Args),
                               int threads, Args& a, Step* out_trace, int steps, double (&r)[N], int bad_posterior, const char* bad_posterior_text) {
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  laps.skip();
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }
  if (record) HIP_TRY(h->sbs.record.upload(record, (size_t)k_sb_stats_doubles));
  else { emat_status st = sb_queue_parts_stats(h, w); if (st) return st; }
  const bool want_trace = out_trace != nullptr && steps > 0;
  HIP_TRY(S.result.alloc(N));
  if (want_trace) HIP_TRY(S.trace.alloc_roomy((size_t)steps));
  a.stats = h->sbs.record.p; a.trace = want_trace ? S.trace.p : nullptr; a.result = S.result.p;
  if (laps.on) HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark(marks[0]);
  hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)threads), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  laps.mark(marks[1]);
  HIP_TRY(hipMemcpy(r, S.result.p, sizeof r, hipMemcpyDeviceToHost));
  if (r[bad_posterior] != 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + bad_posterior_text);
  if (want_trace) HIP_TRY(hipMemcpy(out_trace, S.trace.p, (size_t)steps * sizeof(Step), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* the statistics emat_parts_subst_moves reads (header: emat_parts_subst_stats) */
emat_status emat_parts_subst_stats(emat_backend* h, double* Ttwiddle_beta_a, int64_t* num_muts_beta_ab, int64_t* root_state_counts) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_parts_subst_stats: ";
  if (!Ttwiddle_beta_a || !num_muts_beta_ab || !root_state_counts) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "Ttwiddle_beta_a, num_muts_beta_ab and root_state_counts must not be null");
  emat_status st = sb_check_parts(h, w); if (st) return st;
  if (h->host_only) return no_device(h);
  st = sb_queue_parts_stats(h, w); if (st) return st;
  HIP_TRY(hipStreamSynchronize(h->stream));
  double record[k_sb_stats_doubles];
  HIP_TRY(hipMemcpy(record, h->sbs.record.p, sizeof record, hipMemcpyDeviceToHost));
  const int P = h->num_partitions;
  for (int k = 0; k < 4 * P; ++k) Ttwiddle_beta_a[k] = record[k_sb_T + k];
  for (int k = 0; k < 16 * P; ++k) num_muts_beta_ab[k] = (int64_t)record[k_sb_M + k];
  for (int a = 0; a < 4; ++a) root_state_counts[a] = (int64_t)record[k_sb_C + a];
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_SUBST_STATS_HOST_HPP_
