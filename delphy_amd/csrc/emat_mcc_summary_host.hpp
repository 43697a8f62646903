// emat_mcc_summary_host.hpp -- host side of emat_mcc_node_times and emat_mcc_mutation_support (emat_mcc_summary_kernels.hpp): argument and
// state checks, the chunks of nodes sized from the free device memory, the launches, and the copies of what was asked for.
//
// Both calls work on the last valid derivation (its first / count / stride, master and correspondence table) and touch only the store.
//
// Included by emat_backend.hip after emat_mcc_host.hpp (mcc_store_dev, mcc_mb) and emat_samples_probe_host.hpp.
#ifndef EMAT_MCC_SUMMARY_HOST_HPP_
#define EMAT_MCC_SUMMARY_HOST_HPP_

namespace {

constexpr int64_t k_mccs_max_per_sample_values = (int64_t)1 << 26;   // times / is_exact are for the handful of nodes whose histogram is drawn

const char* const k_mccs_derive_first = ": emat_mcc_derive first (its table is dropped by the next derive, emat_tree_samples_clear and emat_tree_samples_reserve)";

// The flags of a call, [3][M]: bad links, times that are not finite, lists outside their segment.
emat_status mccs_flags_reset(emat_backend* h, int32_t M, MccsFlags& F) {
  MccSummaryScratch& W = h->mcs;
  HIP_TRY(W.flags.alloc_roomy(3 * (size_t)M));
  HIP_TRY(hipMemsetAsync(W.flags.p, 0, 3 * (size_t)M * 4, h->stream));
  F.bad_link = W.flags.p; F.not_finite = W.flags.p + M; F.bad_list = W.flags.p + 2 * (size_t)M;
  return EMAT_OK;
}
// After the launches: EMAT_ERR_INTERNAL naming the first sample a kernel stumbled over.  Synchronises the stream.
emat_status mccs_flags_check(emat_backend* h, const std::string& w, int32_t M) {
  const MccHost& X = h->mcc;
  std::vector<int32_t> f(3 * (size_t)M);
  HIP_TRY(hipMemcpyAsync(f.data(), h->mcs.flags.p, f.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int32_t k = 0; k < M; ++k) {
    const std::string which = "sample " + std::to_string(k) + " (slot " + std::to_string(X.derived_first + k * X.derived_stride) + ")";
    if (f[(size_t)k]) return fail(h, EMAT_ERR_INTERNAL, w + ": the correspondence table leaves the tree in " + which);
    if (f[(size_t)M + k]) return fail(h, EMAT_ERR_INTERNAL, w + ": " + which + " holds a node time that is not finite");
    if (f[2 * (size_t)M + k]) return fail(h, EMAT_ERR_INTERNAL, w + ": a list of " + which + " lies outside its segment");
  }
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* the spread of every MCC node's date over the base trees (header: emat_mcc_node_times) */
emat_status emat_mcc_node_times(emat_backend* h, int32_t num_nodes, const int32_t* mcc_nodes, emat_mcc_node_times_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_node_times";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  MccSummaryScratch& W = h->mcs;
  if (X.derived_M == 0) return fail(h, EMAT_ERR_STATE, w + k_mccs_derive_first);
  const int32_t n = X.derived_n, M = X.derived_M;
  // ---- arguments ----
  if (mcc_nodes) {
    if (num_nodes < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_nodes must be positive with a list of nodes, not " + std::to_string(num_nodes));
    for (int32_t i = 0; i < num_nodes; ++i)
      if (mcc_nodes[i] < 0 || mcc_nodes[i] >= n)
        return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": entry " + std::to_string(i) + ": node " + std::to_string(mcc_nodes[i]) + " is outside the valid range [0, " + std::to_string(n) + ")");
  }
  const int32_t nq = out->num_quantiles;
  if (nq < 0 || (nq > 0 && !out->quantiles)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_quantiles must not be negative, and with num_quantiles > 0 quantiles must be given");
  for (int32_t j = 0; j < nq; ++j)
    if (!(out->quantiles[j] >= 0.0 && out->quantiles[j] <= 1.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": quantile " + std::to_string(j) + " is " + std::to_string(out->quantiles[j]) + ", outside [0, 1]");
  if (!(out->hpd_mass >= 0.0 && out->hpd_mass <= 1.0)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": hpd_mass is " + std::to_string(out->hpd_mass) + ", outside [0, 1] (0: no HPD)");
  const bool want_q = out->q_exact || out->q_mrca, want_hpd = out->hpd_exact || out->hpd_mrca, want_per_sample = out->times || out->is_exact;
  if (!want_q && !want_hpd && !out->num_exact && !want_per_sample)
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": nothing is asked for: q_exact, q_mrca, hpd_exact, hpd_mrca, num_exact, times and is_exact are all NULL");
  if (want_q && nq == 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": q_exact / q_mrca are asked for without quantiles (num_quantiles = 0)");
  if (want_hpd && out->hpd_mass == 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": hpd_exact / hpd_mrca are asked for without hpd_mass (0)");
  if (M > k_probe_sort_max) return fail(h, EMAT_ERR_CAPACITY, w + ": the derivation has " + std::to_string(M) + " samples, and the sort holds " + std::to_string(k_probe_sort_max));
  const size_t cols = mcc_nodes ? (size_t)num_nodes : (size_t)n, Ms = (size_t)M;
  if (want_per_sample && (int64_t)cols * M > k_mccs_max_per_sample_values)
    return fail(h, EMAT_ERR_CAPACITY, w + ": times / is_exact of " + std::to_string(cols) + " nodes x " + std::to_string(M) + " samples are more than " + std::to_string(k_mccs_max_per_sample_values) + " values: pick the nodes whose histogram is drawn");

  // ---- the chunk: nodes whose (M x B) times and flags, 9 bytes each, fit half of what is free ----
  size_t B = std::min<size_t>(h->cfg_mcc_summary_chunk > 0 ? (size_t)h->cfg_mcc_summary_chunk : cols, cols);
  if (B * Ms > W.x.n || B * Ms > W.e.n) {          // it has to grow: only then is the device asked what it has
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t avail = free_b + W.x.n * 8 + W.e.n, per_node = Ms * 9;
    if (2 * per_node > avail)
      return fail(h, EMAT_ERR_CAPACITY, w + ": the times of one node over " + std::to_string(M) + " samples need " + mcc_mb(per_node) + " twice over; the device has " + mcc_mb(free_b) + " free of " + mcc_mb(total_b));
    if (h->cfg_mcc_summary_chunk <= 0) B = std::max<size_t>(1, std::min(cols, avail / 2 / per_node));
    if (B * Ms > W.x.n || B * Ms > W.e.n) {
      HIP_TRY(hipStreamSynchronize(h->stream));
      MccSummaryScratch::drop(W.x); MccSummaryScratch::drop(W.e); W.x.n_grown = false; W.e.n_grown = false;   // (freed first and allocated exactly: the room asked for is the room needed)
      HIP_TRY(W.x.alloc(B * Ms)); HIP_TRY(W.e.alloc(B * Ms));
    }
  }
  if (mcc_nodes) { HIP_TRY(W.nodes.alloc_roomy(cols)); HIP_TRY(hipMemcpyAsync(W.nodes.p, mcc_nodes, cols * 4, hipMemcpyHostToDevice, h->stream)); }
  if (nq) { HIP_TRY(W.quantiles.alloc_roomy((size_t)nq)); HIP_TRY(hipMemcpyAsync(W.quantiles.p, out->quantiles, (size_t)nq * 8, hipMemcpyHostToDevice, h->stream)); }
  MccsNodeOut O{};
  O.cols = cols;
  if (out->q_exact) { HIP_TRY(W.q_exact.alloc_roomy((size_t)nq * cols)); O.q_exact = W.q_exact.p; }
  if (out->q_mrca) { HIP_TRY(W.q_mrca.alloc_roomy((size_t)nq * cols)); O.q_mrca = W.q_mrca.p; }
  if (out->hpd_exact) { HIP_TRY(W.hpd_exact.alloc_roomy(2 * cols)); O.hpd_exact = W.hpd_exact.p; }
  if (out->hpd_mrca) { HIP_TRY(W.hpd_mrca.alloc_roomy(2 * cols)); O.hpd_mrca = W.hpd_mrca.p; }
  if (out->num_exact) { HIP_TRY(W.num_exact.alloc_roomy(cols)); O.num_exact = W.num_exact.p; }
  const bool want_stats = want_q || want_hpd || out->num_exact;
  MccsFlags F{};
  st = mccs_flags_reset(h, M, F); if (st) return st;
  int padded = 1;
  while (padded < M) padded *= 2;
  const MccStore S = mcc_store_dev(X);
  const MccPick pick{X.derived_first, X.derived_stride, M};
  std::vector<double> hx; std::vector<uint8_t> he;
  for (size_t v0 = 0; v0 < cols; v0 += B) {
    const size_t b = std::min(B, cols - v0);
    hipLaunchKernelGGL(k_mccs_gather, dim3((unsigned)((b + 255) / 256), (unsigned)std::min(M, 65535)), dim3(256), 0, h->stream, S, pick, (const int32_t*)X.corr.p, (const uint8_t*)X.exact.p,
                       mcc_nodes ? (const int32_t*)(W.nodes.p + v0) : (const int32_t*)nullptr, (int32_t)v0, (int32_t)b, W.x.p, W.e.p, F);
    HIP_TRY(hipGetLastError());
    if (want_stats) {
      O.col0 = v0;
      hipLaunchKernelGGL(k_mccs_node_stats, dim3((unsigned)std::min<size_t>(b, 1 << 16)), dim3(k_mccs_threads), (size_t)padded * sizeof(double), h->stream,
                         (const double*)W.x.p, (const uint8_t*)W.e.p, M, padded, (int)b, (const double*)W.quantiles.p, nq, out->hpd_mass, O);
      HIP_TRY(hipGetLastError());
    }
    if (want_per_sample) {           // [M][b] on the device, [node][M] for the caller
      HIP_TRY(hipStreamSynchronize(h->stream));
      if (out->times) { hx.resize(b * Ms); HIP_TRY(hipMemcpy(hx.data(), W.x.p, b * Ms * 8, hipMemcpyDeviceToHost)); for (size_t j = 0; j < b; ++j) for (size_t k = 0; k < Ms; ++k) out->times[(v0 + j) * Ms + k] = hx[k * b + j]; }
      if (out->is_exact) { he.resize(b * Ms); HIP_TRY(hipMemcpy(he.data(), W.e.p, b * Ms, hipMemcpyDeviceToHost)); for (size_t j = 0; j < b; ++j) for (size_t k = 0; k < Ms; ++k) out->is_exact[(v0 + j) * Ms + k] = he[k * b + j]; }
    }
  }
  st = mccs_flags_check(h, w, M); if (st) return st;
  if (out->q_exact) HIP_TRY(hipMemcpy(out->q_exact, W.q_exact.p, (size_t)nq * cols * 8, hipMemcpyDeviceToHost));
  if (out->q_mrca) HIP_TRY(hipMemcpy(out->q_mrca, W.q_mrca.p, (size_t)nq * cols * 8, hipMemcpyDeviceToHost));
  if (out->hpd_exact) HIP_TRY(hipMemcpy(out->hpd_exact, W.hpd_exact.p, 2 * cols * 8, hipMemcpyDeviceToHost));
  if (out->hpd_mrca) HIP_TRY(hipMemcpy(out->hpd_mrca, W.hpd_mrca.p, 2 * cols * 8, hipMemcpyDeviceToHost));
  if (out->num_exact) HIP_TRY(hipMemcpy(out->num_exact, W.num_exact.p, cols * 4, hipMemcpyDeviceToHost));
  return EMAT_OK;
}

/* in how many base trees each of the master's mutations occurs, and when (header: emat_mcc_mutation_support) */
emat_status emat_mcc_mutation_support(emat_backend* h, int64_t capacity, int64_t* num_mutations, int32_t* num_with, double* mean_t, double* t_min, double* t_max) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_mutation_support";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  MccSummaryScratch& W = h->mcs;
  if (X.derived_M == 0) return fail(h, EMAT_ERR_STATE, w + k_mccs_derive_first);
  if (X.mut_capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve_mutations first (this store keeps topology and times only)");
  const int32_t n = X.derived_n, M = X.derived_M;
  std::vector<long long> seg_base((size_t)M); std::vector<uint32_t> seg_len((size_t)M);
  for (int32_t k = 0; k < M; ++k) {
    const size_t slot = (size_t)(X.derived_first + k * X.derived_stride);
    if (X.mut_base[slot] < 0)
      return fail(h, EMAT_ERR_STATE, w + ": sample " + std::to_string(k) + " (slot " + std::to_string(slot) + ") was pushed without mutations (emat_tree_sample_push_flat)");
    seg_base[(size_t)k] = (long long)X.mut_base[slot]; seg_len[(size_t)k] = X.mut_len[slot];
  }
  // the master's lists in node order: where each starts among the records of the answer
  const int32_t master = X.derived_master;
  const size_t master_slot = (size_t)(X.derived_first + master * X.derived_stride), len = (size_t)X.mut_len[master_slot];
  std::vector<GList> hdr((size_t)n);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(hdr.data(), X.mut_hdr.p + master_slot * (size_t)n, (size_t)n * sizeof(GList), hipMemcpyDeviceToHost));
  std::vector<int32_t> rec_offset((size_t)n + 1, 0);
  size_t records = 0;
  for (size_t v = 0; v < (size_t)n; ++v) {
    if ((size_t)hdr[v].off + hdr[v].cnt > len || records + hdr[v].cnt > len) return fail(h, EMAT_ERR_INTERNAL, w + ": a list of the master (slot " + std::to_string(master_slot) + ") lies outside its segment");
    records += hdr[v].cnt; rec_offset[v + 1] = (int32_t)records;
  }
  if (num_mutations) *num_mutations = (int64_t)records;
  if (!num_with && !mean_t && !t_min && !t_max) return EMAT_OK;   // (the count alone: what sizes the arrays)
  if (capacity < (int64_t)records) return fail(h, EMAT_ERR_CAPACITY, w + ": the master (slot " + std::to_string(master_slot) + ") has " + std::to_string(records) + " mutations, room for " + std::to_string(capacity));
  if (records == 0) return EMAT_OK;
  HIP_TRY(W.rec_offset.alloc_roomy((size_t)n + 1)); HIP_TRY(W.seg_base.alloc_roomy((size_t)M)); HIP_TRY(W.seg_len.alloc_roomy((size_t)M));
  HIP_TRY(hipMemcpy(W.rec_offset.p, rec_offset.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(W.seg_base.p, seg_base.data(), (size_t)M * 8, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(W.seg_len.p, seg_len.data(), (size_t)M * 4, hipMemcpyHostToDevice));
  if (num_with) HIP_TRY(W.num_with.alloc_roomy(records));
  if (mean_t) HIP_TRY(W.mean_t.alloc_roomy(records));
  if (t_min) HIP_TRY(W.t_min.alloc_roomy(records));
  if (t_max) HIP_TRY(W.t_max.alloc_roomy(records));
  MccsFlags F{};
  st = mccs_flags_reset(h, M, F); if (st) return st;
  MccsMuts Q{}; Q.lists = X.mut_hdr.p; Q.recs = X.mut_arena.p; Q.seg_base = W.seg_base.p; Q.seg_len = W.seg_len.p;
  const MccPick pick{X.derived_first, X.derived_stride, M};
  hipLaunchKernelGGL(k_mccs_mutation_support, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, h->stream, mcc_store_dev(X), pick, master, (const int32_t*)X.corr.p, (const uint8_t*)X.exact.p, Q,
                     (const int32_t*)W.rec_offset.p, (int32_t)records, num_with ? W.num_with.p : nullptr, mean_t ? W.mean_t.p : nullptr, t_min ? W.t_min.p : nullptr, t_max ? W.t_max.p : nullptr, F);
  HIP_TRY(hipGetLastError());
  st = mccs_flags_check(h, w, M); if (st) return st;
  if (num_with) HIP_TRY(hipMemcpy(num_with, W.num_with.p, records * 4, hipMemcpyDeviceToHost));
  if (mean_t) HIP_TRY(hipMemcpy(mean_t, W.mean_t.p, records * 8, hipMemcpyDeviceToHost));
  if (t_min) HIP_TRY(hipMemcpy(t_min, W.t_min.p, records * 8, hipMemcpyDeviceToHost));
  if (t_max) HIP_TRY(hipMemcpy(t_max, W.t_max.p, records * 8, hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"
#endif  // EMAT_MCC_SUMMARY_HOST_HPP_
