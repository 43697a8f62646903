// emat_slab_host.hpp -- a part between its host record and its slab (layout: emat_slab.hpp): encode and decode, the capacities a
// slab is given, and the size classes that decide which parts share a launch and an LDS staging area.
//
// Included by emat_backend.hip after emat_state_host.hpp.
#ifndef EMAT_SLAB_HOST_HPP_
#define EMAT_SLAB_HOST_HPP_

namespace {

uint32_t a16(uint32_t x) { return (x + 15u) & ~15u; }

// Encode one part into its slab (layout: emat_slab.hpp).
void encode_slab(const PartHost& ph, uint8_t* slab, uint32_t slab_bytes, uint32_t heap_bytes, uint32_t scratch_bytes, int cell_cap, int trace_cap) {
  std::memset(slab, 0, slab_bytes - scratch_bytes);   // scratch (the slab's tail) is transient: never read before written
  const FlatTree& t = ph.tree;
  const int n = t.num_nodes();
  SlabHeader* H = (SlabHeader*)slab;
  H->magic = k_slab_magic; H->slab_bytes = slab_bytes; H->n_nodes = n; H->root = t.root;
  H->flags = ph.includes_run_root ? k_flag_includes_run_root : 0u;
  H->status = 0; H->rng_key = ph.rng.key; H->rng_counter = ph.rng.counter; H->rng_spare = ph.rng.spare; H->rng_has_spare = ph.rng.has_spare ? 1u : 0u;
  uint32_t off = sizeof(SlabHeader);
  H->off_nodes = off; off += (uint32_t)n * (uint32_t)sizeof(NodeRec);
  { uint64_t* dl = (uint64_t*)(slab + off); for (int i = 0; i < n; ++i) dl[i] = k_miss_dl_unknown; off += miss_dl_bytes_for((uint32_t)n); }   // nothing remembered: the moves fill it in as they ask
  H->off_cells = off; off += a16((uint32_t)cell_cap * cell_bytes_for(ph.includes_run_root));
  H->off_trace = off; off += a16((uint32_t)trace_cap * 32u);
  H->heap_begin = off; H->heap_end = off + heap_bytes;
  H->scratch_begin = H->heap_end; H->scratch_end = H->scratch_begin + scratch_bytes;
  H->cell_first = ph.coal.cell_first; H->n_cells = (int)ph.coal.k_bar_p.size(); H->cell_cap = cell_cap; H->n_cells_total = ph.coal.n_cells_total;
  H->t_ref = ph.coal.t_ref; H->t_step = ph.coal.t_step;
  H->trace_cap = trace_cap; H->trace_len = std::min<int>(trace_cap, (int)(ph.trace.size() / 4));
  if (H->trace_len > 0) std::memcpy(slab + H->off_trace, ph.trace.data(), (size_t)H->trace_len * 32);
  NodeRec* N = (NodeRec*)(slab + H->off_nodes);
  uint32_t top = H->heap_begin;
  for (int i = 0; i < n; ++i) {
    NodeRec& r = N[i];
    r.parent = t.parent[i]; r.child0 = t.child0[i]; r.child1 = t.child1[i];
    r.t_min = t.t_min[i]; r.t_max = t.t_max[i]; r.t = t.t[i]; r.lambda = 0.0; r.n_missing = 0;
    int nm = t.mut_offset[i + 1] - t.mut_offset[i], ni = t.miss_offset[i + 1] - t.miss_offset[i], nf = t.mfs_offset[i + 1] - t.mfs_offset[i];
    // (counts were checked against k_max_list_len by the caller, materialize)
    r.muts.off = top; r.muts.cnt = (uint16_t)nm; r.muts.cap = list_cap_for(a16(nm * 16u), 16u);
    MutRec* m = (MutRec*)(slab + top);
    for (int k = 0; k < nm; ++k) { int s = t.mut_offset[i] + k; m[k].t = t.mut_t[s]; m[k].site = t.mut_site[s]; m[k].from = t.mut_from[s]; m[k].to = t.mut_to[s]; m[k].pad = 0; }
    top += a16(nm * 16u);
    r.miss.off = top; r.miss.cnt = (uint16_t)ni; r.miss.cap = list_cap_for(a16(ni * 8u), 8u);
    IvRec* iv = (IvRec*)(slab + top);
    for (int k = 0; k < ni; ++k) { int s = t.miss_offset[i] + k; iv[k].start = t.miss_start[s]; iv[k].end = t.miss_end[s]; }
    top += a16(ni * 8u);
    r.mfs.off = top; r.mfs.cnt = (uint16_t)nf; r.mfs.cap = list_cap_for(a16(nf * 8u), 8u);
    FsRec* fs = (FsRec*)(slab + top);
    for (int k = 0; k < nf; ++k) { int s = t.mfs_offset[i] + k; fs[k].site = t.mfs_site[s]; fs[k].state = t.mfs_state[s]; }
    top += a16(nf * 8u);
  }
  H->heap_top = top;
  double* cb = (double*)(slab + H->off_cells);
  const int nc = (int)ph.coal.k_bar_p.size();
  for (int w = 0; w < nc; ++w) {
    cb[w] = ph.coal.k_bar_p[w]; cb[cell_cap + w] = ph.coal.k_twiddle_bar_p[w];
    if (!ph.includes_run_root) continue;      // the run-wide arrays live once per device (SharedCells); the root part, which may append cells, keeps its own
    cb[2 * cell_cap + w] = ph.coal.k_twiddle_bar[w]; cb[3 * cell_cap + w] = ph.coal.popsize_bar[w];
    cb[4 * cell_cap + w] = ph.coal.t_step / ph.coal.popsize_bar[w];   // the factor every cell term starts with, divided once
    ((int32_t*)(cb + 5 * cell_cap))[w] = ph.coal.num_active_parts[w];
  }
}

uint32_t heap_content_bytes(const FlatTree& t) {
  uint32_t b = 0;
  for (int i = 0; i < t.num_nodes(); ++i)
    b += a16((t.mut_offset[i + 1] - t.mut_offset[i]) * 16u) + a16((t.miss_offset[i + 1] - t.miss_offset[i]) * 8u) + a16((t.mfs_offset[i + 1] - t.mfs_offset[i]) * 8u);
  return b;
}

// Decode the device image of a part back into its host FlatTree + coalescent window + rng + stats.
void decode_slab(PartHost& ph, const uint8_t* slab, const double* shared_ktw, const double* shared_popsize, const int32_t* shared_nact) {
  const SlabHeader* H = (const SlabHeader*)slab;
  const NodeRec* N = (const NodeRec*)(slab + H->off_nodes);
  const int n = H->n_nodes;
  FlatTree& t = ph.tree;
  int nm = 0, ni = 0, nf = 0;
  for (int i = 0; i < n; ++i) { nm += N[i].muts.cnt; ni += N[i].miss.cnt; nf += N[i].mfs.cnt; }
  t.allocate(n, nm, ni, nf);
  t.root = H->root;
  int km = 0, ki = 0, kf = 0;
  for (int i = 0; i < n; ++i) {
    const NodeRec& r = N[i];
    t.parent[i] = r.parent; t.child0[i] = r.child0; t.child1[i] = r.child1; t.t[i] = r.t; t.t_min[i] = r.t_min; t.t_max[i] = r.t_max;
    const MutRec* m = (const MutRec*)(slab + r.muts.off);
    for (int k = 0; k < r.muts.cnt; ++k) { t.mut_site[km] = m[k].site; t.mut_from[km] = m[k].from; t.mut_to[km] = m[k].to; t.mut_t[km] = m[k].t; ++km; }
    const IvRec* iv = (const IvRec*)(slab + r.miss.off);
    for (int k = 0; k < r.miss.cnt; ++k) { t.miss_start[ki] = iv[k].start; t.miss_end[ki] = iv[k].end; ++ki; }
    const FsRec* fs = (const FsRec*)(slab + r.mfs.off);
    for (int k = 0; k < r.mfs.cnt; ++k) { t.mfs_site[kf] = fs[k].site; t.mfs_state[kf] = fs[k].state; ++kf; }
    t.mut_offset[i + 1] = km; t.miss_offset[i + 1] = ki; t.mfs_offset[i + 1] = kf;
  }
  ph.rng.counter = H->rng_counter; ph.rng.spare = H->rng_spare; ph.rng.has_spare = H->rng_has_spare != 0;
  { const double* tr = (const double*)(slab + H->off_trace); ph.trace.assign(tr, tr + (size_t)4 * H->trace_len); }
  const int nc = H->n_cells, cap = H->cell_cap;
  const double* cb = (const double*)(slab + H->off_cells);
  ph.coal.n_cells_total = H->n_cells_total;
  ph.coal.k_bar_p.assign(cb, cb + nc); ph.coal.k_twiddle_bar_p.assign(cb + cap, cb + cap + nc);
  if ((H->flags & k_flag_includes_run_root) != 0) {
    ph.coal.k_twiddle_bar.assign(cb + 2 * cap, cb + 2 * cap + nc); ph.coal.popsize_bar.assign(cb + 3 * cap, cb + 3 * cap + nc);
    const int32_t* na = (const int32_t*)(cb + 5 * cap); ph.coal.num_active_parts.assign(na, na + nc);
  } else if (shared_ktw != nullptr) {   // the window of the device's shared arrays (they do not change while the parts run)
    const int f = H->cell_first;
    ph.coal.k_twiddle_bar.assign(shared_ktw + f, shared_ktw + f + nc); ph.coal.popsize_bar.assign(shared_popsize + f, shared_popsize + f + nc);
    ph.coal.num_active_parts.assign(shared_nact + f, shared_nact + f + nc);
  }
}

// Capacities of one part's slab: what a move may need on top of the part's present content.
struct SlabGeo { uint32_t heap, scratch; int cell_cap; uint32_t bytes; };
SlabGeo slab_geometry(const emat_backend* h, int n, int num_muts, uint32_t content, int nc, bool includes_run_root, double space_boost, int cell_boost = 1) {
  const double slack = h->cfg.slab_slack > 0 ? h->cfg.slab_slack : 3.0;
  const int trace_cap = h->cfg.trace_moves > 0 ? h->cfg.trace_moves : 0;
  SlabGeo g;
  g.heap = a16((uint32_t)(space_boost * std::max<double>(2048.0, content * slack + h->cfg_heap_per_node * n)));
  // worst case of one move: an unlimited SPR scan visits every (branch, inter-mutation segment) region of the
  // part (48 B each) with a DFS stack of up to 4 items per region (12 B each), next to two graft analyses
  const uint32_t regions_max = (uint32_t)n + (uint32_t)num_muts;
  g.scratch = a16((uint32_t)(space_boost * std::max<uint32_t>(8192u, 128u * regions_max + 4u * content + 256u * (uint32_t)n)));
  g.cell_cap = includes_run_root ? nc + cell_boost * std::max(512, nc) : nc;   // room for the root part's grid to grow into the past (a part that outgrows it stops with status 103 / 105)
  g.bytes = (uint32_t)sizeof(SlabHeader) + (uint32_t)n * (uint32_t)sizeof(NodeRec) + miss_dl_bytes_for((uint32_t)n) + a16((uint32_t)g.cell_cap * cell_bytes_for(includes_run_root)) + a16((uint32_t)trace_cap * 32u) + g.heap + g.scratch;
  return g;
}
// What the handle books per part about a slab of geometry g (the size classes and the staging variants read these) ...
void book_slab_bytes(emat_backend* h, size_t p, const SlabGeo& g, uint32_t content_bytes) {
  if (h->used_bytes.size() <= p) h->used_bytes.resize(p + 1, 0u);
  h->used_bytes[p] = g.bytes - g.scratch - g.heap + content_bytes;
  h->persistent_bytes[p] = g.bytes - g.scratch;
  h->prefix_bytes[p] = g.bytes - g.scratch - g.heap;
  h->max_slab_bytes = std::max(h->max_slab_bytes, g.bytes);
}
// ... and where the slab goes, into the part's record (a repartition on the device writes its records later, in its one pass over them)
void place_slab(emat_backend* h, size_t p, const SlabGeo& g, uint64_t& off, uint32_t content_bytes) {
  book_slab_bytes(h, p, g, content_bytes);
  PartHost& ph = h->parts[p];
  ph.slab_off = off; ph.slab_bytes = g.bytes; ph.scratch_bytes = g.scratch; off += g.bytes;
}
// Size classes: which parts share a launch and an LDS staging area.  Class 0 has the largest area; the last class (the
// "main" one) holds the bulk of the parts.  Sets h->class_of / class_lds / class_begin; build_order lays the launch
// order out class by class.
void assign_size_classes(emat_backend* h) {
  const size_t n = h->parts.size();
  const bool verbose = verbose_reports();
  std::vector<uint32_t> v = h->persistent_bytes;
  const bool by_percentiles = h->cfg.use_lds && n != 0 && h->cfg_class_pct.size() > 1;
  if (by_percentiles || verbose) std::sort(v.begin(), v.end());   // (the default rule needs one order statistic: nth_element below)
  h->class_of.assign(n, 0);
  std::vector<uint32_t> areas;   // per class, descending
  const uint32_t lds_cu = 160u * 1024u, overhead = k_lds_static_bytes + (h->cfg.use_lds ? h->cfg_lds_scratch : 0u);
  auto area_for = [&](uint32_t k) {   // the staging area of a workgroup when k of them share a CU (LDS is allocated in 512-byte granules)
    const uint32_t share = (lds_cu / k) & ~511u;
    return share <= overhead ? 0u : std::min<uint32_t>((share - overhead) & ~15u, h->cfg_lds_max & ~15u);
  };
  if (!h->cfg.use_lds || n == 0) areas.push_back(0u);
  else if (h->cfg_class_pct.size() > 1) {
    // option "lds_classes" = "p1,p2,..." (tuning knob): classes by rank of persistent size, class c closing at percentile p_c and
    // staging that percentile's size
    std::vector<std::pair<uint32_t, uint32_t>> asc;   // (largest persistent size of the class, staging bytes), ascending
    size_t lo = 0;
    for (size_t ci = 0; ci < h->cfg_class_pct.size(); ++ci) {
      const int pct = h->cfg_class_pct[ci];
      const bool last = ci + 1 == h->cfg_class_pct.size() || (int)asc.size() + 1 == emat_backend::k_max_classes;
      size_t hi = std::min(n, (n * (size_t)pct + 99) / 100);
      if (pct >= 100 || last) hi = n;
      if (hi <= lo) { if (last) break; continue; }
      uint32_t need = (v[(last ? std::min(n, (n * (size_t)pct + 99) / 100) : hi) - 1] + 511u) & ~511u;
      if (need > h->cfg_lds_max) need = h->cfg_lds_max & ~511u;   // larger parts: prefix-staged or HBM only
      asc.push_back({v[hi - 1], need});
      lo = hi;
      if (last) break;
    }
    if (asc.empty()) asc.push_back({v.back(), 0u});
    const int nc = (int)asc.size();
    for (int c = 0; c < nc; ++c) areas.push_back(asc[nc - 1 - c].second);
    for (size_t p = 0; p < n; ++p) { int c = 0; while (c + 1 < nc && h->persistent_bytes[p] > asc[c].first) ++c; h->class_of[p] = nc - 1 - c; }
  } else {
    // The default.  The percentile only says which parts MUST fit whole.  LDS is the resource that limits residency, so
    // take the most workgroups per CU (up to the 16 the VGPR budget allows) whose share of the 160 KiB still holds that
    // percentile, and give every workgroup its whole share: larger parts than asked for get staged whole at no cost in
    // occupancy, the rest stage their prefix.
    const int pct = h->cfg_class_pct.empty() ? 60 : h->cfg_class_pct[0];
    const size_t hi = pct >= 100 ? n : std::max<size_t>(1, std::min(n, (n * (size_t)pct + 99) / 100));
    if (!verbose) std::nth_element(v.begin(), v.begin() + (hi - 1), v.end());
    const uint32_t need = std::min<uint32_t>((v[hi - 1] + 511u) & ~511u, h->cfg_lds_max & ~511u);
    uint32_t main_area = 0;
    for (uint32_t k = 4u * EMAT_WAVES_PER_EU; k >= 1; --k) {   // 4 SIMDs x waves per SIMD allowed by the VGPR budget (one wave per workgroup)
      const uint32_t area = area_for(k);
      if (area == 0) continue;
      if (area >= need || k == 1) { main_area = area; break; }
    }
    if (h->cfg_parts_per_cu > 0 && area_for((uint32_t)h->cfg_parts_per_cu) != 0) main_area = area_for((uint32_t)h->cfg_parts_per_cu);   // option "parts_per_cu"
    // Giants: a part whose fixed-size prefix (header, nodes, cells) does not fit the area would run entirely out of HBM,
    // at less than half the speed, and -- every part doing the same number of moves -- hold up the whole pass.  They
    // get launches of their own, with areas for 8 and for 1 workgroup per CU: each giant takes the smaller area if it
    // holds its prefix.  (One area sized for the largest giant, as in round 1, put every giant at one workgroup per CU,
    // and a partition that has drifted for a while holds hundreds of them: passes of 52 ms instead of 32 at C4.  More
    // than two side launches would need more concurrent streams than the runtime has hardware queues -- four by default,
    // GPU_MAX_HW_QUEUES -- and streams that share a queue run one after the other.)
    std::vector<uint32_t> ladder;
    if (h->cfg_giants) for (uint32_t k : {8u, 1u}) { const uint32_t a = area_for(k); if (a > main_area && (ladder.empty() || a > ladder.back())) ladder.push_back(a); }
    std::vector<int> rung_of(n, -1); std::vector<int> used(ladder.size(), 0);
    if (!ladder.empty())
      for (size_t p = 0; p < n; ++p) if (h->prefix_bytes[p] > main_area || (h->cfg_side_arena != 0 && p < h->used_bytes.size() && h->used_bytes[p] + k_lds_heap_room + h->cfg_side_arena > main_area)) {
        size_t r = 0; while (r + 1 < ladder.size() && ladder[r] < h->prefix_bytes[p]) ++r;
        rung_of[p] = (int)r; used[r] = 1;
      }
    std::vector<int> class_of_rung(ladder.size(), -1);
    for (int r = (int)ladder.size() - 1; r >= 0; --r) if (used[r] && (int)areas.size() + 1 < emat_backend::k_max_classes) { class_of_rung[r] = (int)areas.size(); areas.push_back(ladder[r]); }
    const int main_class = (int)areas.size();
    areas.push_back(main_area);
    for (size_t p = 0; p < n; ++p) h->class_of[p] = rung_of[p] >= 0 && class_of_rung[rung_of[p]] >= 0 ? class_of_rung[rung_of[p]] : main_class;
  }
  h->num_classes = (int)areas.size();
  std::vector<int> count(h->num_classes, 0);
  for (size_t p = 0; p < n; ++p) ++count[h->class_of[p]];
  h->class_begin[0] = 0;
  for (int c = 0; c < h->num_classes; ++c) { h->class_lds[c] = areas[c]; h->class_begin[c + 1] = h->class_begin[c] + count[c]; }
  if (verbose && n > 0) {
    fprintf(stderr, "[emat] parts %zu persistent bytes p50 %u p90 %u p99 %u max %u | classes:", n, v[n / 2], v[n * 9 / 10], v[n * 99 / 100], v.back());
    for (int c = 0; c < h->num_classes; ++c) fprintf(stderr, " [%d parts, LDS %u]", h->class_begin[c + 1] - h->class_begin[c], h->class_lds[c]);
    fprintf(stderr, "\n");
  }
}

}  // namespace

#endif  // EMAT_SLAB_HOST_HPP_
