// emat_samples_probe_host.hpp -- the probers over many samples of the store, the ancestral one and the site-state one: what is
// specific to the store.  Argument and state checks, the chosen samples' root times (the one step the resident tree does not need),
// and the job -- one unit per (sample, site) -- handed to the driver every prober shares (emat_probe_host.hpp: probe_run_job).
//
// Included by emat_backend.hip after emat_probe_host.hpp (ProbeJob) and emat_mcc_host.hpp.
#ifndef EMAT_SAMPLES_PROBE_HOST_HPP_
#define EMAT_SAMPLES_PROBE_HOST_HPP_

namespace {

struct SamplesProbeRequest {
  const emat_pop_model* pops; int32_t num_pops;
  int32_t first, count, stride;
  int32_t num_marked; const int32_t* marks;
  bool per_sample;                   // marks [count][num_marked] rather than [num_marked]
  bool through_corr;                 // marks are MCC nodes: sample k's mark is corr[k][mark] (the last derivation's table)
  double t_start, t_end; int32_t num_t_cells;
  int32_t num_sites = 0; const int32_t* sites = nullptr;   // the site-state form (then no marks): the unit the chunks iterate over is a (sample, site) pair
};

emat_status samples_probe_run(emat_backend* h, const std::string& w, const SamplesProbeRequest& q, emat_samples_probe_result* out) {
  MccHost& X = h->mcc;
  ProbeScratch& S = h->probe;
  const int32_t n = X.n, M = q.count;
  // ---- arguments ----
  if (q.count < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": the number of samples must be positive, not " + std::to_string(q.count));
  if (q.stride < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": stride must be positive, not " + std::to_string(q.stride));
  if (q.first < 0 || (int64_t)q.first + (int64_t)(q.count - 1) * q.stride >= X.count)
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": samples " + std::to_string(q.first) + ", " + std::to_string(q.first) + " + " + std::to_string(q.stride) + ", ... (" + std::to_string(q.count) + " of them) are outside the valid range [0, " + std::to_string(X.count) + ")");
  if (!q.pops || (q.num_pops != 1 && q.num_pops != M))
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": pop_models must be given, one for all samples or one per chosen sample (" + std::to_string(M) + "), not " + std::to_string(q.num_pops));
  const bool by_site = q.sites != nullptr || q.num_sites != 0;
  if (by_site) {
    if (q.num_sites < 1 || !q.sites) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_sites must be positive and sites must be given, not " + std::to_string(q.num_sites));
    if (X.mut_capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve_mutations first (this store keeps topology and times only)");
    for (int i = 0; i < q.num_sites; ++i)
      if (q.sites[i] < 0 || q.sites[i] >= X.mut_L)
        return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": entry " + std::to_string(i) + ": site " + std::to_string(q.sites[i]) + " is outside the valid range [0, " + std::to_string(X.mut_L) + ")");
    for (int k = 0; k < M; ++k)
      if (X.mut_base[(size_t)(q.first + k * q.stride)] < 0)
        return fail(h, EMAT_ERR_STATE, w + ": sample " + std::to_string(k) + " (slot " + std::to_string(q.first + k * q.stride) + ") was pushed without mutations (emat_tree_sample_push_flat)");
  }
  else if (!q.per_sample) { emat_status st = probe_check_marks(h, w, q.num_marked, q.marks, n); if (st) return st; }
  else {
    if (q.num_marked < 0 || (q.num_marked > 0 && !q.marks)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_marked must not be negative, and marked_nodes must be given");
    for (int k = 0; k < M; ++k)
      for (int i = 0; i < q.num_marked; ++i) {
        const int32_t v = q.marks[(size_t)k * q.num_marked + i];
        if (v != EMAT_NO_NODE && (v < 0 || v >= n))
          return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": sample " + std::to_string(k) + ", entry " + std::to_string(i) + ": node " + std::to_string(v) + " is neither `none` (-1) nor inside the valid range [0, " + std::to_string(n) + ")");
      }
  }
  emat_status st = probe_check_window(h, w, q.t_start, q.t_end, q.num_t_cells); if (st) return st;
  if (out->num_ranks < 0 || (out->num_ranks > 0 && (!out->ranks || !out->order_stats)))
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_ranks must not be negative, and with num_ranks > 0 both ranks and order_stats must be given");
  for (int j = 0; j < out->num_ranks; ++j)
    if (out->ranks[j] < 0 || out->ranks[j] >= M) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": rank " + std::to_string(out->ranks[j]) + " is outside the valid range [0, " + std::to_string(M) + ")");
  const bool want_stats = out->num_ranks > 0;
  if (!out->p && !out->mean && !want_stats) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": nothing is asked for: p, mean and order_stats are all NULL");
  std::vector<HostPopModel> hps((size_t)q.num_pops);
  for (int i = 0; i < q.num_pops; ++i) {
    const std::string why = probe_host_pop(q.pops[i], hps[(size_t)i]);
    if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": population model " + std::to_string(i) + ": " + why);
  }
  if (want_stats && M > k_probe_sort_max)
    return fail(h, EMAT_ERR_CAPACITY, w + ": order statistics over " + std::to_string(M) + " samples, and the sort holds " + std::to_string(k_probe_sort_max));

  // ---- step 0: the chosen samples' root times; then the job, one unit per (sample, site) ----
  ProbeJob J;
  J.w = w; J.by_site = by_site; J.M = M; J.U = by_site ? q.num_sites : 1; J.members = by_site ? 4 : q.num_marked + 1;
  J.t_start = q.t_start; J.t_end = q.t_end; J.num_t_cells = q.num_t_cells;
  J.num_marked = q.num_marked; J.marks = q.marks; J.per_sample = q.per_sample; J.corr = q.through_corr ? X.corr.p : nullptr;
  J.hps = std::move(hps); J.out = *out;
  J.T.parent = X.parent.p; J.T.t = X.t.p; J.T.root = X.root.p; J.T.lists = X.mut_hdr.p; J.T.recs = X.mut_arena.p; J.T.ref = X.mut_ref.p; J.T.n = n; J.T.L = X.mut_L;
  HIP_TRY(S.root_t.alloc_roomy((size_t)M)); HIP_TRY(S.status.alloc_roomy((size_t)M));
  HIP_TRY(hipMemsetAsync(S.status.p, 0, (size_t)M * 4, h->stream));
  hipLaunchKernelGGL(k_probe_roots, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, J.T, q.first, q.stride, M, S.root_t.p, S.status.p);
  HIP_TRY(hipGetLastError());
  std::vector<double> root_t((size_t)M); std::vector<int32_t> status((size_t)M);
  HIP_TRY(hipMemcpyAsync(root_t.data(), S.root_t.p, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(status.data(), S.status.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  J.units.resize((size_t)M * J.U);
  for (int k = 0; k < M; ++k)
    for (int i = 0; i < J.U; ++i) {
      ProbeUnit& u = J.units[(size_t)k * J.U + i];
      u = ProbeUnit{};
      u.slot = q.first + k * q.stride; u.pop = q.num_pops == 1 ? 0 : k; u.sample = k; u.ref_state = -1;   // (the root starts from the sequence the slot kept)
      if (by_site) { u.site = q.sites[i]; u.seg_base = (long long)X.mut_base[(size_t)u.slot]; u.seg_len = X.mut_len[(size_t)u.slot]; }
    }
  for (int k = 0; k < M; ++k)
    if (status[(size_t)k]) return fail(h, EMAT_ERR_INTERNAL, w + ": the root of " + J.which(k) + " is outside the tree");
  st = probe_plan_grids(h, J, root_t.data()); if (st) return st;
  return probe_run_job(h, J);
}

}  // namespace

extern "C" {

/* probe_ancestors_on_tree on every chosen sample (header: emat_tree_samples_probe_ancestors) */
emat_status emat_tree_samples_probe_ancestors(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models, int32_t first, int32_t count, int32_t stride,
                                              int32_t num_marked, const int32_t* marked_nodes, int32_t marks_per_sample, double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_samples_probe_ancestors";
  emat_status st = gt_require(h, false, true); if (st) return st;
  if (marks_per_sample != 0 && marks_per_sample != 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": marks_per_sample is 0 (one list for all samples) or 1 (one list per sample), not " + std::to_string(marks_per_sample));
  const SamplesProbeRequest q{pop_models, num_pop_models, first, count, stride, num_marked, marked_nodes, marks_per_sample == 1, false, t_start, t_end, num_t_cells};
  return samples_probe_run(h, w, q, out);
}

/* the same on every base tree of the last derivation, the marks being the nodes that correspond to the MCC nodes picked
   (tools/delphy_wasm.cpp:1828-1849) (header: emat_mcc_probe_ancestors) */
emat_status emat_mcc_probe_ancestors(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models, int32_t num_marked, const int32_t* mcc_nodes,
                                     double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_probe_ancestors";
  emat_status st = gt_require(h, false, true); if (st) return st;
  const MccHost& X = h->mcc;
  if (X.derived_M == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_mcc_derive first (its table is dropped by the next derive, emat_tree_samples_clear and emat_tree_samples_reserve)");
  const SamplesProbeRequest q{pop_models, num_pop_models, X.derived_first, X.derived_M, X.derived_stride, num_marked, mcc_nodes, false, true, t_start, t_end, num_t_cells};
  return samples_probe_run(h, w, q, out);
}

/* probe_site_states_on_tree (core/site_states_tree_prober.cpp:40-92) on every chosen sample, for every site asked for (header: emat_tree_samples_probe_site_states) */
emat_status emat_tree_samples_probe_site_states(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models, int32_t first, int32_t count, int32_t stride,
                                                int32_t num_sites, const int32_t* sites, double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_samples_probe_site_states";
  emat_status st = gt_require(h, false, true); if (st) return st;
  if (num_sites < 1 || !sites) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_sites must be positive and sites must be given, not " + std::to_string(num_sites));
  const SamplesProbeRequest q{pop_models, num_pop_models, first, count, stride, 0, nullptr, false, false, t_start, t_end, num_t_cells, num_sites, sites};
  return samples_probe_run(h, w, q, out);
}

/* the same on every base tree of the last derivation, as a front end runs it (tools/delphy_wasm.cpp:1809); sites are the same in
   every base tree, so the correspondence table plays no part (header: emat_mcc_probe_site_states) */
emat_status emat_mcc_probe_site_states(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models, int32_t num_sites, const int32_t* sites,
                                       double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_probe_site_states";
  emat_status st = gt_require(h, false, true); if (st) return st;
  const MccHost& X = h->mcc;
  if (num_sites < 1 || !sites) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_sites must be positive and sites must be given, not " + std::to_string(num_sites));
  if (X.derived_M == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_mcc_derive first (its table is dropped by the next derive, emat_tree_samples_clear and emat_tree_samples_reserve)");
  const SamplesProbeRequest q{pop_models, num_pop_models, X.derived_first, X.derived_M, X.derived_stride, 0, nullptr, false, false, t_start, t_end, num_t_cells, num_sites, sites};
  return samples_probe_run(h, w, q, out);
}

/* which samples emat_mcc_probe_ancestors would probe (header: emat_mcc_get_derivation) */
emat_status emat_mcc_get_derivation(emat_backend* h, int32_t* first, int32_t* count, int32_t* stride) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const MccHost& X = h->mcc;
  if (first) *first = X.derived_M ? X.derived_first : 0;
  if (count) *count = X.derived_M;
  if (stride) *stride = X.derived_M ? X.derived_stride : 1;
  return EMAT_OK;
}

}  // extern "C"
#endif  // EMAT_SAMPLES_PROBE_HOST_HPP_
