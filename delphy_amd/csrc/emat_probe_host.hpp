// emat_probe_host.hpp -- host side of the tree probers (emat_probe_kernels.hpp): ONE driver, cut into stages over a list of units
// (ProbeJob), for the samples of the store (emat_samples_probe_host.hpp) and for the resident tree, whose entry points are at the end
// of this file: thin callers with one unit -- slot 0 of a store of one, the root time from the host's mirror, the root's state from
// the host's sequence.  Here too: the argument checks the reference's constructors and probers make, and the grid (with the
// reference's crude extension towards a root that lies before t_start).
//
//   plan             probe_plan_grids: every unit's grid from its root time; probe_plan_room: room, chunk size, the call's one upload
//   labels + counts  probe_counts: steps 1-2 of the kernels for one chunk; emat_tree_branch_counts stops here
//   cells + chain    probe_chain: step 3 for the same chunk
//   summaries        probe_finish: the status words, step 4, the copies of what was asked for
//
// Included by emat_backend.hip after its entry points, after emat_gtree_host.hpp (gt_require) and emat_mcc_host.hpp (mcc_mb).
#ifndef EMAT_PROBE_HOST_HPP_
#define EMAT_PROBE_HOST_HPP_

namespace {

constexpr int64_t k_probe_max_cells = 1 << 22;          // cells of one member, the ones prepended to reach the root included
constexpr int64_t k_probe_max_values = 1 << 26;         // members x cells

struct ProbeRequest {
  int kind;                          // EMAT_PROBE_ANCESTORS / EMAT_PROBE_SITE_STATES
  int32_t num_marked; const int32_t* marked; int32_t site;
  double t_start, t_end; int32_t num_t_cells;
};

// The reference's checks of the marked nodes and of the window (ancestral_tree_prober.cpp:36-50, staircase.h:27-34), for one tree and for many.
emat_status probe_check_marks(emat_backend* h, const std::string& w, int32_t num_marked, const int32_t* marked, int32_t n) {
  if (num_marked < 0 || (num_marked > 0 && !marked)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_marked must not be negative, and marked_nodes must be given");
  for (int i = 0; i < num_marked; ++i)
    if (marked[i] != EMAT_NO_NODE && (marked[i] < 0 || marked[i] >= n))
      return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": node " + std::to_string(marked[i]) + " is neither `none` (-1) nor inside the valid range [0, " + std::to_string(n) + ")");
  return EMAT_OK;
}
emat_status probe_check_window(emat_backend* h, const std::string& w, double t_start, double t_end, int32_t num_t_cells) {
  if (!std::isfinite(t_start) || !std::isfinite(t_end) || !(t_start < t_end))
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": invalid domain: need t_start < t_end, but t_start=" + std::to_string(t_start) + " and t_end=" + std::to_string(t_end));
  if (num_t_cells <= 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": number of cells should be positive, not " + std::to_string(num_t_cells));
  return EMAT_OK;
}
// The grid of the branch counts of a tree of n nodes whose root is at root_t: ancestral_tree_prober.cpp:52-61 / site_states_tree_prober.cpp:60-69,
// to the letter: the same subtractions give the same doubles.  False when it outgrows what the prober holds (`num_cells` is then where it stopped).
bool probe_extend_grid(double t_start, double t_end, int32_t num_t_cells, double root_t, int32_t n, int32_t members, ProbeGrid& g, int64_t& num_cells, int32_t& cells_to_skip) {
  double real_t_start = t_start;
  int64_t skip = 0;
  num_cells = num_t_cells;
  if (t_start > root_t) {
    const double cell_size = (t_end - t_start) / num_t_cells;
    while (real_t_start > root_t) {
      real_t_start -= cell_size; ++num_cells; ++skip;
      if (num_cells > k_probe_max_cells) break;
    }
  }
  if (num_cells > k_probe_max_cells || (int64_t)members * num_cells > k_probe_max_values) return false;
  g = ProbeGrid{};
  g.x_start = real_t_start; g.num_cells = (int32_t)num_cells;
  g.cell_size = (t_end - real_t_start) / g.num_cells;            // Staircase's constructor
  g.x_end = g.x_start + g.num_cells * g.cell_size;               // Staircase::x_end()
  int bits = 0; while (((int64_t)1 << bits) < (int64_t)n + 1) ++bits;
  g.frac_bits = std::min(52, 61 - bits);
  g.scale = std::ldexp(1.0, g.frac_bits); g.inv_scale = std::ldexp(1.0, -g.frac_bits);
  cells_to_skip = (int32_t)skip;
  return true;
}
std::string probe_grid_too_large(int32_t members, int64_t num_cells, double root_t) {
  return std::to_string(members) + " members x " + std::to_string(num_cells) + " cells (the cells it takes to reach back to the root at " + std::to_string(root_t) +
         " included) is more than the prober holds (" + std::to_string(k_probe_max_cells) + " cells, " + std::to_string(k_probe_max_values) + " values)";
}
// A population model as the kernels read it; its Skygrid knots are at sky_x / sky_g on the device.
PopTable probe_pop_table(const HostPopModel& hp, const double* sky_x, const double* sky_g) {
  PopTable pt{};
  pt.kind = hp.kind; pt.skygrid_type = hp.skygrid_type; pt.skygrid_num_knots = (int)hp.x.size();
  for (int i = 0; i < 4; ++i) pt.p[i] = hp.p[i];
  pt.t_c = hp.t_c;
  pt.skygrid_x = sky_x; pt.skygrid_gamma = sky_g;
  pt.skygrid_inv_dx = (hp.x.size() >= 2 && hp.x.back() > hp.x.front()) ? (double)(hp.x.size() - 1) / (hp.x.back() - hp.x.front()) : 0.0;
  pt.skygrid_x0 = hp.x.empty() ? 0.0 : hp.x.front();
  return pt;
}
// "" or why the model cannot be built: a Skygrid without its knots, or what its constructor refuses.
std::string probe_host_pop(const emat_pop_model& pm, HostPopModel& hp) {
  if (pm.kind == EMAT_POP_SKYGRID && pm.skygrid_num_knots > 0 && (!pm.skygrid_x || !pm.skygrid_gamma)) return "a Skygrid model without its knots";
  try { hp = HostPopModel::from_c(pm); } catch (const std::exception& ex) { return ex.what(); }
  return "";
}

// A call: its units over the trees `T`, what it asks for, and what each stage leaves for the next.  The entry point fills the first
// block (of a unit: everything but grid and cells_to_skip).
struct ProbeJob {
  std::string w;                     // the entry point, for the texts
  ProbeTrees T{};
  bool resident = false, by_site = false;
  int32_t M = 1, U = 1;              // samples, and units (sites) of a sample: unit k * U + i
  int32_t members = 0, num_t_cells = 0;
  double t_start = 0.0, t_end = 0.0;
  std::vector<ProbeUnit> units;      // [M * U]
  int32_t num_marked = 0; const int32_t* marks = nullptr; bool per_sample = false;   // marks [num_marked], or [M][num_marked]
  const int32_t* corr = nullptr;     // marks are MCC nodes: sample k's mark is corr[k][mark] (device: the last derivation's table)
  std::vector<HostPopModel> hps;     // one for all samples or one per sample; none: the call stops at the counts
  emat_samples_probe_result out{};   // what is asked for; cells_to_skip [M] is filled by probe_plan_grids
  // probe_plan_grids, probe_plan_room:
  int64_t stride_cells = 0, B = 1;   // the largest cell count of any unit; samples of a chunk
  const ProbeUnit* d_units = nullptr; const PopTable* d_pops = nullptr; const int32_t* d_marks = nullptr; const int32_t* d_ranks = nullptr;

  bool chain() const { return !hps.empty(); }
  size_t values() const { return (size_t)U * (size_t)members * (size_t)num_t_cells; }
  std::string which(int k) const { return resident ? "the resident tree" : "sample " + std::to_string(k) + " (slot " + std::to_string(units[(size_t)k * U].slot) + ")"; }
  ProbeChunk chunk(int64_t k0) const {   // in units: what the kernels index
    ProbeChunk C{}; C.units = d_units; C.k0 = (int32_t)k0 * U; C.B = (int32_t)std::min<int64_t>(B, M - k0) * U; C.n = T.n; C.num_members = members; C.stride_cells = (int32_t)stride_cells;
    return C;
  }
};

// Plan, on the host alone: the grid of every sample from its root time, with the arithmetic of one function for every caller.
emat_status probe_plan_grids(emat_backend* h, ProbeJob& J, const double* root_t) {
  J.stride_cells = 0;
  for (int k = 0; k < J.M; ++k) {
    ProbeUnit& u = J.units[(size_t)k * J.U];
    int64_t num_cells = 0;
    if (!probe_extend_grid(J.t_start, J.t_end, J.num_t_cells, root_t[k], J.T.n, J.members, u.grid, num_cells, u.cells_to_skip))
      return fail(h, EMAT_ERR_CAPACITY, J.w + ": " + (J.resident ? std::string() : J.which(k) + ": ") + probe_grid_too_large(J.members, num_cells, root_t[k]));
    J.stride_cells = std::max(J.stride_cells, num_cells);
    if (J.out.cells_to_skip) J.out.cells_to_skip[k] = u.cells_to_skip;
    for (int i = 1; i < J.U; ++i) { ProbeUnit& v = J.units[(size_t)k * J.U + i]; v.grid = u.grid; v.cells_to_skip = u.cells_to_skip; }
  }
  return EMAT_OK;
}

// Plan, on the device: what is kept for the whole call, the chunk, and ONE upload of everything the kernels read from the host --
// descriptors, population tables with the knots of all models one after the other, marks, ranks.
emat_status probe_plan_room(emat_backend* h, ProbeJob& J) {
  ProbeScratch& S = h->probe;
  const size_t M = (size_t)J.M, U = (size_t)J.U, n = (size_t)J.T.n, members = (size_t)J.members, nc = (size_t)J.stride_cells, values = J.values();
  const size_t num_ranks = (size_t)J.out.num_ranks, num_marks = J.by_site ? 0 : (size_t)J.num_marked * (J.per_sample ? M : 1);
  size_t knots = 0;
  for (const HostPopModel& hp : J.hps) knots += hp.x.size();
  static_assert(sizeof(ProbeUnit) % 8 == 0 && sizeof(PopTable) % 8 == 0, "the doubles behind them in the upload stay aligned");
  const size_t o_pops = M * U * sizeof(ProbeUnit), o_x = o_pops + J.hps.size() * sizeof(PopTable), o_g = o_x + knots * 8, o_marks = o_g + knots * 8, o_ranks = o_marks + num_marks * 4, bytes = o_ranks + num_ranks * 4;
  const size_t per_sample = U * (n * 12 + members * nc * 16 + members * (nc + 1) * 4 + nc * 16);
  const size_t whole_call = (J.chain() ? M * values * 8 : 0) + (J.out.mean ? values * 8 : 0) + num_ranks * values * 8 + M * 12 + bytes;
  auto holds = [&](size_t B) {       // the scratch as it stands takes chunks of B samples
    return B * U * n <= S.val.n && B * U * members * nc <= S.fix.n && B * U * members * (nc + 1) <= S.diff.n && B * U * nc <= S.total.n && (!J.chain() || M * values <= S.p.n) &&
           (!J.out.mean || values <= S.mean.n) && num_ranks * values <= S.stats.n && bytes <= S.args.n && M <= S.status.n;
  };
  J.B = std::min<int64_t>(h->cfg_samples_probe_chunk > 0 ? h->cfg_samples_probe_chunk : J.M, J.M);
  if (!holds((size_t)J.B)) {          // it has to grow: only then is the device asked what it has (a call like the last one asks nothing)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t avail = free_b + S.samples_bytes();          // (what the last call left is reused or replaced)
    if (whole_call + per_sample > avail)
      return fail(h, EMAT_ERR_CAPACITY, J.w + ": the results of " + std::to_string(M) + " samples x " + (J.by_site ? std::to_string(U) + " sites x " : std::string()) + std::to_string(members) + " members x " + std::to_string(J.num_t_cells) + " cells need " + mcc_mb(whole_call) +
                                        " and the working room of one sample" + (J.by_site ? " with all its sites " : " ") + mcc_mb(per_sample) + "; the device has " + mcc_mb(free_b) + " free of " + mcc_mb(total_b));
    J.B = h->cfg_samples_probe_chunk;
    if (J.B <= 0) J.B = (int64_t)std::max<size_t>(1, (avail - whole_call) / 2 / per_sample);   // half of what is left: buffers that grow take a quarter more than asked
    J.B = std::min<int64_t>(J.B, J.M);
    if (avail < whole_call + (size_t)J.B * per_sample) J.B = 1;
    if ((size_t)J.B * U * n > S.val.n || (size_t)J.B * U * members * nc > S.fix.n || (J.chain() && M * values > S.p.n)) { HIP_TRY(hipStreamSynchronize(h->stream)); S.release_samples(); }   // (freed first, so that the room asked for is the room needed)
  }
  const size_t BU = (size_t)J.B * U, Bn = BU * n, Bv = BU * members * nc, Bd = BU * members * (nc + 1), Bc = BU * nc;
  HIP_TRY(S.status.alloc(M));
  HIP_TRY(S.val.alloc(Bn)); HIP_TRY(S.jump_a.alloc(Bn)); HIP_TRY(S.jump_b.alloc(Bn));
  HIP_TRY(S.fix.alloc(Bv)); HIP_TRY(S.counts.alloc(Bv)); HIP_TRY(S.diff.alloc(Bd)); HIP_TRY(S.total.alloc(Bc)); HIP_TRY(S.p_coalesce.alloc(Bc));
  if (J.chain()) HIP_TRY(S.p.alloc(M * values));
  if (J.out.mean) HIP_TRY(S.mean.alloc(values));
  HIP_TRY(S.stats.alloc(num_ranks * values));
  HIP_TRY(S.args.alloc(bytes));
  HIP_TRY(hipMemsetAsync(S.status.p, 0, M * 4, h->stream));

  std::vector<uint8_t> args(bytes);
  std::memcpy(args.data(), J.units.data(), o_pops);
  size_t o = 0;
  for (size_t i = 0; i < J.hps.size(); ++i) {
    const HostPopModel& hp = J.hps[i];
    const PopTable pt = probe_pop_table(hp, (const double*)(S.args.p + o_x) + o, (const double*)(S.args.p + o_g) + o);
    std::memcpy(args.data() + o_pops + i * sizeof(PopTable), &pt, sizeof(PopTable));
    if (!hp.x.empty()) { std::memcpy(args.data() + o_x + o * 8, hp.x.data(), hp.x.size() * 8); std::memcpy(args.data() + o_g + o * 8, hp.gamma.data(), hp.x.size() * 8); }
    o += hp.x.size();
  }
  if (num_marks) std::memcpy(args.data() + o_marks, J.marks, num_marks * 4);
  if (num_ranks) std::memcpy(args.data() + o_ranks, J.out.ranks, num_ranks * 4);
  HIP_TRY(hipMemcpy(S.args.p, args.data(), bytes, hipMemcpyHostToDevice));
  J.d_units = (const ProbeUnit*)S.args.p; J.d_pops = (const PopTable*)(S.args.p + o_pops); J.d_marks = (const int32_t*)(S.args.p + o_marks); J.d_ranks = (const int32_t*)(S.args.p + o_ranks);
  return EMAT_OK;
}

// Steps 1 and 2 for the chunk that starts at sample k0: its branch counts, left in h->probe.counts on the engine's stream.
emat_status probe_counts(emat_backend* h, const ProbeJob& J, int64_t k0) {
  ProbeScratch& S = h->probe;
  const ProbeChunk C = J.chunk(k0);
  const int32_t n = J.T.n, members = J.members;
  const size_t nc = (size_t)J.stride_cells;
  const unsigned gy = (unsigned)std::min(C.B, 65535);
  const dim3 per_node((unsigned)((n + 255) / 256), gy), b256(256);
  if (!J.by_site) HIP_TRY(hipMemsetAsync(S.val.p, 0xff, (size_t)C.B * n * 4, h->stream));
  HIP_TRY(hipMemsetAsync(S.fix.p, 0, (size_t)C.B * members * nc * 8, h->stream));
  HIP_TRY(hipMemsetAsync(S.diff.p, 0, (size_t)C.B * members * (nc + 1) * 4, h->stream));
  if (J.by_site) {
    hipLaunchKernelGGL(k_probe_site_flags, per_node, b256, 0, h->stream, J.T, C, S.val.p, S.status.p);
    HIP_TRY(hipGetLastError());
  } else if (J.num_marked > 0) {
    hipLaunchKernelGGL(k_probe_marks, dim3((unsigned)((J.num_marked + 255) / 256), gy), b256, 0, h->stream, C, J.d_marks, (int)J.num_marked, J.per_sample ? (int)J.num_marked : 0, J.corr, S.val.p);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_probe_jump_init, per_node, b256, 0, h->stream, J.T, C, members - 1, S.val.p, S.jump_a.p);
  HIP_TRY(hipGetLastError());
  int32_t* cur = S.jump_a.p; int32_t* nxt = S.jump_b.p;
  for (int64_t reach = 1; reach < n; reach *= 2) {   // after a round every jump reaches twice as far: ceil(log2 n) rounds cover any depth
    hipLaunchKernelGGL(k_probe_jump_double, per_node, b256, 0, h->stream, (int)n, (int)C.B, (const int32_t*)cur, nxt);
    HIP_TRY(hipGetLastError());
    std::swap(cur, nxt);
  }
  if (J.by_site) hipLaunchKernelGGL((k_probe_branches<true>), per_node, b256, 0, h->stream, J.T, C, (const int32_t*)S.val.p, (const int32_t*)cur, S.fix.p, S.diff.p, S.status.p);
  else hipLaunchKernelGGL((k_probe_branches<false>), per_node, b256, 0, h->stream, J.T, C, (const int32_t*)S.val.p, (const int32_t*)cur, S.fix.p, S.diff.p, S.status.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_probe_counts, dim3((unsigned)members, gy), dim3(k_wave), 0, h->stream, C, (const unsigned long long*)S.fix.p, (const int32_t*)S.diff.p, S.counts.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

// Step 3, Tree_prober, on the counts probe_counts left behind for the same chunk; into h->probe.p [M][U][members][num_t_cells].
emat_status probe_chain(emat_backend* h, const ProbeJob& J, int64_t k0) {
  ProbeScratch& S = h->probe;
  const ProbeChunk C = J.chunk(k0);
  const unsigned gy = (unsigned)std::min(C.B, 65535);
  const dim3 per_member((unsigned)((J.members + 63) / 64), gy);
  hipLaunchKernelGGL(k_probe_cells, dim3((unsigned)((J.stride_cells + 63) / 64), gy), dim3(64), 0, h->stream, C, J.d_pops, (const double*)S.counts.p, S.total.p, S.p_coalesce.p);
  HIP_TRY(hipGetLastError());
  if (J.by_site) hipLaunchKernelGGL((k_probe_chain<true>), per_member, dim3(64), 0, h->stream, J.T, C, (int)J.num_t_cells, (const int32_t*)S.val.p, (const double*)S.counts.p, (const double*)S.total.p, (const double*)S.p_coalesce.p, S.p.p);
  else hipLaunchKernelGGL((k_probe_chain<false>), per_member, dim3(64), 0, h->stream, J.T, C, (int)J.num_t_cells, (const int32_t*)S.val.p, (const double*)S.counts.p, (const double*)S.total.p, (const double*)S.p_coalesce.p, S.p.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

// Waits for the stream and reads the status words: one per sample, the bits of ProbeStatus.
emat_status probe_check_status(emat_backend* h, const ProbeJob& J) {
  std::vector<int32_t> status((size_t)J.M);
  HIP_TRY(hipMemcpyAsync(status.data(), h->probe.status.p, (size_t)J.M * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < J.M; ++k) {
    if (status[(size_t)k] & k_probe_bad_link) return fail(h, EMAT_ERR_INTERNAL, J.w + ": a link of " + J.which(k) + " leaves the tree");
    if (status[(size_t)k] & k_probe_bad_list) return fail(h, EMAT_ERR_INTERNAL, J.w + ": a mutation list of " + J.which(k) + " lies outside the sample's segment of the arena");
    if (status[(size_t)k] & k_probe_negative_branch) return fail(h, EMAT_ERR_INTERNAL, J.w + ": a node of " + J.which(k) + " is earlier than its parent (the reference's add_boxcar refuses left > right)");
  }
  return EMAT_OK;
}

// Step 4: summaries of the per-sample results, and the copies of what was asked for.
emat_status probe_finish(emat_backend* h, const ProbeJob& J) {
  ProbeScratch& S = h->probe;
  const emat_samples_probe_result& out = J.out;
  const size_t values = J.values();
  emat_status st = probe_check_status(h, J); if (st) return st;
  if (out.mean) {
    hipLaunchKernelGGL(k_probe_mean, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, h->stream, (const double*)S.p.p, (int)J.M, values, S.mean.p);
    HIP_TRY(hipGetLastError());
  }
  if (out.num_ranks > 0) {
    int padded = 1; while (padded < J.M) padded *= 2;
    hipLaunchKernelGGL(k_probe_order_stats, dim3((unsigned)std::min<size_t>(values, 1 << 16)), dim3(k_probe_sort_threads), (size_t)padded * sizeof(double), h->stream,
                       (const double*)S.p.p, (int)J.M, padded, values, J.d_ranks, (int)out.num_ranks, S.stats.p);
    HIP_TRY(hipGetLastError());
  }
  if (out.mean || out.num_ranks > 0) HIP_TRY(hipStreamSynchronize(h->stream));
  if (out.p) HIP_TRY(hipMemcpy(out.p, S.p.p, (size_t)J.M * values * 8, hipMemcpyDeviceToHost));
  if (out.mean) HIP_TRY(hipMemcpy(out.mean, S.mean.p, values * 8, hipMemcpyDeviceToHost));
  if (out.num_ranks > 0) HIP_TRY(hipMemcpy(out.order_stats, S.stats.p, (size_t)out.num_ranks * values * 8, hipMemcpyDeviceToHost));
  return EMAT_OK;
}

// All stages of a job whose grids are planned.
emat_status probe_run_job(emat_backend* h, ProbeJob& J) {
  emat_status st = probe_plan_room(h, J); if (st) return st;
  for (int64_t k0 = 0; k0 < J.M; k0 += J.B) {
    st = probe_counts(h, J, k0); if (st) return st;
    st = probe_chain(h, J, k0); if (st) return st;
  }
  return probe_finish(h, J);
}

// ---- the resident tree: one unit ---------------------------------------------------------------------------------------------------
// The reference's argument checks, and the job: the tree as slot 0 of a store of one, its lists in the used part of its own heap.
emat_status probe_resident_job(emat_backend* h, const char* what, const ProbeRequest& q, ProbeJob& J) {
  J.w = what;
  const std::string& w = J.w;
  emat_status st = gt_require_tree_home(h, false, w + ": "); if (st) return st;
  GTreeHost& G = h->gt;
  const int n = G.n;
  ProbeUnit u{};
  if (q.kind == EMAT_PROBE_ANCESTORS) {
    st = probe_check_marks(h, w, q.num_marked, q.marked, n); if (st) return st;
    J.num_marked = q.num_marked; J.marks = q.marked;
  } else if (q.kind == EMAT_PROBE_SITE_STATES) {
    if (q.site < 0 || q.site >= h->L) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": site " + std::to_string(q.site) + " is outside the valid range [0, " + std::to_string(h->L) + ")");
    if (!h->have_ref) return fail(h, EMAT_ERR_STATE, w + ": emat_set_ref_sequence first (the root's state starts from it)");
    J.by_site = true;
    u.site = q.site; u.ref_state = (int32_t)h->ref[(size_t)q.site];   // (the host's sequence: the device's copy may be a launch behind)
    u.seg_len = G.used[0];
  } else return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": kind is neither EMAT_PROBE_ANCESTORS nor EMAT_PROBE_SITE_STATES");
  st = probe_check_window(h, w, q.t_start, q.t_end, q.num_t_cells); if (st) return st;
  J.resident = true;
  J.T.parent = G.parent.p; J.T.t = G.t.p; J.T.root = G.root.p; J.T.lists = G.muts.p; J.T.recs = G.mut_heap.p; J.T.n = n; J.T.L = h->L;
  J.members = J.by_site ? 4 : q.num_marked + 1;
  J.t_start = q.t_start; J.t_end = q.t_end; J.num_t_cells = q.num_t_cells;
  J.units.assign(1, u);
  return probe_plan_grids(h, J, &G.h_root_t);
}

emat_status probe_run(emat_backend* h, const char* what, const emat_pop_model* pm, const ProbeRequest& q, double* p) {
  if (!h || !pm || !p) return EMAT_ERR_INVALID_ARGUMENT;
  ProbeJob J;
  J.hps.resize(1);
  { const std::string why = probe_host_pop(*pm, J.hps[0]); if (!why.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, std::string(what) + ": " + why); }
  emat_status st = probe_resident_job(h, what, q, J); if (st) return st;
  J.out.p = p;
  return probe_run_job(h, J);
}

}  // namespace

extern "C" {

/* probe_ancestors_on_tree (header: emat_tree_probe_ancestors) */
emat_status emat_tree_probe_ancestors(emat_backend* h, const emat_pop_model* pop_model, int32_t num_marked, const int32_t* marked_nodes,
                                      double t_start, double t_end, int32_t num_t_cells, double* p) {
  const ProbeRequest q{EMAT_PROBE_ANCESTORS, num_marked, marked_nodes, 0, t_start, t_end, num_t_cells};
  return probe_run(h, "emat_tree_probe_ancestors", pop_model, q, p);
}
/* probe_site_states_on_tree (header: emat_tree_probe_site_states) */
emat_status emat_tree_probe_site_states(emat_backend* h, const emat_pop_model* pop_model, int32_t site, double t_start, double t_end, int32_t num_t_cells, double* p) {
  const ProbeRequest q{EMAT_PROBE_SITE_STATES, 0, nullptr, site, t_start, t_end, num_t_cells};
  return probe_run(h, "emat_tree_probe_site_states", pop_model, q, p);
}
/* the Staircase_family the two probers hand to Tree_prober (header: emat_tree_branch_counts) */
emat_status emat_tree_branch_counts(emat_backend* h, int32_t kind, int32_t num_marked, const int32_t* marked_nodes, int32_t site, double t_start, double t_end, int32_t num_t_cells,
                                    int32_t* num_cells, int32_t* cells_to_skip, double* x_start, double* counts, int64_t counts_capacity) {
  if (!h || !num_cells) return EMAT_ERR_INVALID_ARGUMENT;
  const ProbeRequest q{kind, num_marked, marked_nodes, site, t_start, t_end, num_t_cells};
  ProbeJob J;
  emat_status st = probe_resident_job(h, "emat_tree_branch_counts", q, J); if (st) return st;
  const ProbeUnit& u = J.units[0];
  *num_cells = u.grid.num_cells;
  if (cells_to_skip) *cells_to_skip = u.cells_to_skip;
  if (x_start) *x_start = u.grid.x_start;
  if (!counts) return EMAT_OK;
  const int64_t values = (int64_t)J.members * u.grid.num_cells;
  if (counts_capacity < values) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_tree_branch_counts: " + std::to_string(values) + " values, room for " + std::to_string(counts_capacity));
  st = probe_plan_room(h, J); if (st) return st;
  st = probe_counts(h, J, 0); if (st) return st;
  st = probe_check_status(h, J); if (st) return st;
  HIP_TRY(hipMemcpy(counts, h->probe.counts.p, (size_t)values * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"
#endif  // EMAT_PROBE_HOST_HPP_
