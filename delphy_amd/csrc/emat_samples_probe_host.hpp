// emat_samples_probe_host.hpp -- host side of the probers over many samples of the store (emat_samples_probe_kernels.hpp), the ancestral
// one and the site-state one, which differ in where the labels come from, in the branches and in the chain's start, and share the rest:
// argument and state checks, the per-sample grids (emat_probe_host.hpp: probe_extend_grid, the single-tree call's arithmetic), the
// population tables of all models in one upload (probe_pop_table), the chunks, the summaries, and the copies of what was asked for.
//
// Included by emat_backend.hip after emat_probe_host.hpp and emat_mcc_host.hpp (mcc_check_room, mcc_store_dev).
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
  size_t knots = 0;
  for (int i = 0; i < q.num_pops; ++i) {
    const std::string why = probe_host_pop(q.pops[i], hps[(size_t)i]);
    if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": population model " + std::to_string(i) + ": " + why);
    knots += hps[(size_t)i].x.size();
  }
  if (want_stats && M > k_sprobe_sort_max)
    return fail(h, EMAT_ERR_CAPACITY, w + ": order statistics over " + std::to_string(M) + " samples, and the sort holds " + std::to_string(k_sprobe_sort_max));
  const int32_t members = by_site ? 4 : q.num_marked + 1;
  const int32_t U = by_site ? q.num_sites : 1;               // units of a sample
  const size_t values = (size_t)U * (size_t)members * (size_t)q.num_t_cells;

  // ---- step 0: roots, grids ----
  const MccStore D = mcc_store_dev(X);
  const MccPick pick{q.first, q.stride, M};
  const dim3 b256(256);
  HIP_TRY(S.sp_root_t.alloc_roomy((size_t)M)); HIP_TRY(S.sp_status.alloc_roomy((size_t)M));
  HIP_TRY(hipMemsetAsync(S.sp_status.p, 0, (size_t)M * 4, h->stream));
  hipLaunchKernelGGL(k_sprobe_roots, dim3((unsigned)((M + 255) / 256)), b256, 0, h->stream, D, pick, S.sp_root_t.p, S.sp_status.p);
  HIP_TRY(hipGetLastError());
  std::vector<double> root_t((size_t)M); std::vector<int32_t> status((size_t)M);
  HIP_TRY(hipMemcpyAsync(root_t.data(), S.sp_root_t.p, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(status.data(), S.sp_status.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::vector<SProbeSample> samples((size_t)M * U);        // one descriptor per unit, sample-major
  std::vector<SProbeSeg> segs(by_site ? (size_t)M : 0);
  int64_t stride_cells = 0;
  for (int k = 0; k < M; ++k) {
    const std::string which = "sample " + std::to_string(k) + " (slot " + std::to_string(q.first + k * q.stride) + ")";
    if (status[(size_t)k]) return fail(h, EMAT_ERR_INTERNAL, w + ": the root of " + which + " is outside the tree");
    SProbeSample& s = samples[(size_t)k * U];
    s = SProbeSample{};
    int64_t num_cells = 0;
    if (!probe_extend_grid(q.t_start, q.t_end, q.num_t_cells, root_t[(size_t)k], n, members, s.grid, num_cells, s.cells_to_skip))
      return fail(h, EMAT_ERR_CAPACITY, w + ": " + which + ": " + probe_grid_too_large(members, num_cells, root_t[(size_t)k]));
    s.slot = q.first + k * q.stride; s.pop = q.num_pops == 1 ? 0 : k;
    stride_cells = std::max(stride_cells, num_cells);
    if (out->cells_to_skip) out->cells_to_skip[k] = s.cells_to_skip;
    for (int i = 1; i < U; ++i) samples[(size_t)k * U + i] = s;
    if (by_site) segs[(size_t)k] = SProbeSeg{(long long)X.mut_base[(size_t)s.slot], X.mut_len[(size_t)s.slot], 0};
  }

  // ---- room: what is kept for the whole call, and the chunk ----
  const size_t nc = (size_t)stride_cells;
  const size_t per_sample = (size_t)U * ((size_t)n * 12 + (size_t)members * nc * 16 + (size_t)members * (nc + 1) * 4 + nc * 16);
  const size_t whole_call = (size_t)M * values * 8 + (out->mean ? values * 8 : 0) + (want_stats ? (size_t)out->num_ranks * (values * 8 + 4) : 0) +
                            (size_t)M * ((size_t)U * sizeof(SProbeSample) + 12 + (q.per_sample ? (size_t)q.num_marked * 4 : 0) + (by_site ? sizeof(SProbeSeg) : 0)) + (size_t)q.num_pops * sizeof(PopTable) + knots * 16 +
                            (size_t)q.num_marked * 4 + (by_site ? (size_t)U * 4 : 0);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t avail = free_b + S.samples_bytes();          // (what the last call left is reused or replaced)
  if (whole_call + per_sample > avail)
    return fail(h, EMAT_ERR_CAPACITY, w + ": the results of " + std::to_string(M) + " samples x " + (by_site ? std::to_string(U) + " sites x " : std::string()) + std::to_string(members) + " members x " + std::to_string(q.num_t_cells) + " cells need " + mcc_mb(whole_call) +
                                      " and the working room of one sample" + (by_site ? " with all its sites " : " ") + mcc_mb(per_sample) + "; the device has " + mcc_mb(free_b) + " free of " + mcc_mb(total_b));
  int64_t B = h->cfg_samples_probe_chunk;
  if (B <= 0) B = (int64_t)std::max<size_t>(1, (avail - whole_call) / 2 / per_sample);   // half of what is left: buffers that grow take a quarter more than asked
  B = std::min<int64_t>(B, M);
  if (S.samples_bytes() + free_b < whole_call + (size_t)B * per_sample) B = 1;
  const size_t BU = (size_t)B * U;                           // units of a chunk
  const size_t Bn = BU * (size_t)n, Bv = BU * members * nc, Bd = BU * members * (nc + 1), Bc = BU * nc;
  if (Bn > S.sp_val.n || Bv > S.sp_fix.n || (size_t)M * values > S.sp_p.n) { HIP_TRY(hipStreamSynchronize(h->stream)); S.release_samples(); }   // (freed first, so that the room asked for is the room needed)
  HIP_TRY(S.sp_root_t.alloc((size_t)M)); HIP_TRY(S.sp_status.alloc((size_t)M));
  HIP_TRY(S.sp_val.alloc(Bn)); HIP_TRY(S.sp_jump_a.alloc(Bn)); HIP_TRY(S.sp_jump_b.alloc(Bn));
  HIP_TRY(S.sp_fix.alloc(Bv)); HIP_TRY(S.sp_counts.alloc(Bv)); HIP_TRY(S.sp_diff.alloc(Bd)); HIP_TRY(S.sp_total.alloc(Bc)); HIP_TRY(S.sp_p_coalesce.alloc(Bc));
  HIP_TRY(S.sp_p.alloc((size_t)M * values)); HIP_TRY(S.sp_samples.alloc((size_t)M * U)); HIP_TRY(S.sp_pops.alloc((size_t)q.num_pops));
  HIP_TRY(hipMemsetAsync(S.sp_status.p, 0, (size_t)M * 4, h->stream));

  // ---- uploads: descriptors, population tables with the knots of all models one after the other, marks ----
  HIP_TRY(hipMemcpy(S.sp_samples.p, samples.data(), (size_t)M * U * sizeof(SProbeSample), hipMemcpyHostToDevice));
  if (by_site) { HIP_TRY(S.sp_segs.upload(segs.data(), (size_t)M)); HIP_TRY(S.sp_sites.upload(q.sites, (size_t)U)); }
  {
    std::vector<double> xs, gs; xs.reserve(knots); gs.reserve(knots);
    for (const HostPopModel& hp : hps) { xs.insert(xs.end(), hp.x.begin(), hp.x.end()); gs.insert(gs.end(), hp.gamma.begin(), hp.gamma.end()); }
    if (knots) { HIP_TRY(S.sp_sky_x.upload(xs.data(), knots)); HIP_TRY(S.sp_sky_g.upload(gs.data(), knots)); }
    std::vector<PopTable> pts; pts.reserve(hps.size());
    size_t o = 0;
    for (const HostPopModel& hp : hps) { pts.push_back(probe_pop_table(hp, S.sp_sky_x.p + o, S.sp_sky_g.p + o)); o += hp.x.size(); }
    HIP_TRY(hipMemcpy(S.sp_pops.p, pts.data(), pts.size() * sizeof(PopTable), hipMemcpyHostToDevice));
  }
  const size_t num_marks = by_site ? 0 : (size_t)q.num_marked * (q.per_sample ? (size_t)M : 1);
  if (num_marks) HIP_TRY(S.sp_marks.upload(q.marks, num_marks));

  // ---- steps 1 to 3, chunk by chunk ----
  const int32_t* corr = q.through_corr ? X.corr.p : nullptr;
  const MccMuts Mu = mcc_muts_dev(X);
  for (int64_t k0 = 0; k0 < M; k0 += B) {
    const int32_t Bk = (int32_t)std::min<int64_t>(B, M - k0) * U;   // the chunk's units: what the kernels index
    SProbeChunk C{}; C.samples = S.sp_samples.p; C.k0 = (int32_t)k0 * U; C.B = Bk; C.n = n; C.num_members = members; C.stride_cells = (int32_t)stride_cells;
    const unsigned gy = (unsigned)std::min(Bk, 65535);
    const dim3 per_node((unsigned)((n + 255) / 256), gy);
    if (!by_site) HIP_TRY(hipMemsetAsync(S.sp_val.p, 0xff, (size_t)Bk * n * 4, h->stream));
    HIP_TRY(hipMemsetAsync(S.sp_fix.p, 0, (size_t)Bk * members * nc * 8, h->stream));
    HIP_TRY(hipMemsetAsync(S.sp_diff.p, 0, (size_t)Bk * members * (nc + 1) * 4, h->stream));
    if (by_site) {
      hipLaunchKernelGGL(k_sprobe_site_flags, per_node, b256, 0, h->stream, D, Mu, C, (const SProbeSeg*)S.sp_segs.p, (const int32_t*)S.sp_sites.p, (int)U, S.sp_val.p, S.sp_status.p);
      HIP_TRY(hipGetLastError());
    } else if (q.num_marked > 0) {
      hipLaunchKernelGGL(k_sprobe_marks, dim3((unsigned)((q.num_marked + 255) / 256), gy), b256, 0, h->stream, C, (const int32_t*)S.sp_marks.p, (int)q.num_marked, q.per_sample ? (int)q.num_marked : 0, corr, S.sp_val.p);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sprobe_jump_init, per_node, b256, 0, h->stream, D, C, members - 1, S.sp_val.p, S.sp_jump_a.p);
    HIP_TRY(hipGetLastError());
    int32_t* cur = S.sp_jump_a.p; int32_t* nxt = S.sp_jump_b.p;
    for (int64_t reach = 1; reach < n; reach *= 2) {   // ceil(log2 n) rounds cover any depth
      hipLaunchKernelGGL(k_sprobe_jump_double, per_node, b256, 0, h->stream, n, Bk, (const int32_t*)cur, nxt);
      HIP_TRY(hipGetLastError());
      std::swap(cur, nxt);
    }
    if (by_site) hipLaunchKernelGGL(k_sprobe_site_branches, per_node, b256, 0, h->stream, D, C, (int)U, (const int32_t*)S.sp_val.p, (const int32_t*)cur, S.sp_fix.p, S.sp_diff.p, S.sp_status.p);
    else hipLaunchKernelGGL(k_sprobe_branches, per_node, b256, 0, h->stream, D, C, (const int32_t*)S.sp_val.p, (const int32_t*)cur, S.sp_fix.p, S.sp_diff.p, S.sp_status.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sprobe_counts, dim3((unsigned)members, gy), dim3(k_wave), 0, h->stream, C, (const unsigned long long*)S.sp_fix.p, (const int32_t*)S.sp_diff.p, S.sp_counts.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sprobe_cells, dim3((unsigned)((stride_cells + 63) / 64), gy), dim3(64), 0, h->stream, C, (const PopTable*)S.sp_pops.p, (const double*)S.sp_counts.p, S.sp_total.p, S.sp_p_coalesce.p);
    HIP_TRY(hipGetLastError());
    if (by_site) hipLaunchKernelGGL(k_sprobe_site_chain, dim3((unsigned)((members + 63) / 64), gy), dim3(64), 0, h->stream, D, C, (int)q.num_t_cells, (const int32_t*)S.sp_val.p, (const double*)S.sp_counts.p, (const double*)S.sp_total.p, (const double*)S.sp_p_coalesce.p, S.sp_p.p);
    else hipLaunchKernelGGL(k_sprobe_chain, dim3((unsigned)((members + 63) / 64), gy), dim3(64), 0, h->stream, C, (int)q.num_t_cells, (const double*)S.sp_counts.p, (const double*)S.sp_total.p, (const double*)S.sp_p_coalesce.p, S.sp_p.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(status.data(), S.sp_status.p, (size_t)M * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < M; ++k) {
    const std::string which = "sample " + std::to_string(k) + " (slot " + std::to_string(q.first + k * q.stride) + ")";
    if (status[(size_t)k] & k_sprobe_bad_link) return fail(h, EMAT_ERR_INTERNAL, w + ": a link of " + which + " leaves the tree");
    if (status[(size_t)k] & k_sprobe_bad_list) return fail(h, EMAT_ERR_INTERNAL, w + ": a mutation list of " + which + " lies outside the sample's segment of the arena");
    if (status[(size_t)k] & k_sprobe_negative_branch) return fail(h, EMAT_ERR_INTERNAL, w + ": a node of " + which + " is earlier than its parent (the reference's add_boxcar refuses left > right)");
  }

  // ---- step 4: summaries, and the copies ----
  if (out->mean) {
    HIP_TRY(S.sp_mean.alloc(values));
    hipLaunchKernelGGL(k_sprobe_mean, dim3((unsigned)((values + 255) / 256)), b256, 0, h->stream, (const double*)S.sp_p.p, (int)M, values, S.sp_mean.p);
    HIP_TRY(hipGetLastError());
  }
  if (want_stats) {
    HIP_TRY(S.sp_stats.alloc((size_t)out->num_ranks * values)); HIP_TRY(S.sp_ranks.upload(out->ranks, (size_t)out->num_ranks));
    int padded = 1; while (padded < M) padded *= 2;
    hipLaunchKernelGGL(k_sprobe_order_stats, dim3((unsigned)std::min<size_t>(values, 1 << 16)), dim3(k_sprobe_sort_threads), (size_t)padded * sizeof(double), h->stream,
                       (const double*)S.sp_p.p, (int)M, padded, values, (const int32_t*)S.sp_ranks.p, (int)out->num_ranks, S.sp_stats.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out->p) HIP_TRY(hipMemcpy(out->p, S.sp_p.p, (size_t)M * values * 8, hipMemcpyDeviceToHost));
  if (out->mean) HIP_TRY(hipMemcpy(out->mean, S.sp_mean.p, values * 8, hipMemcpyDeviceToHost));
  if (want_stats) HIP_TRY(hipMemcpy(out->order_stats, S.sp_stats.p, (size_t)out->num_ranks * values * 8, hipMemcpyDeviceToHost));
  return EMAT_OK;
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
