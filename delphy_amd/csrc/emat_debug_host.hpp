// emat_debug_host.hpp -- the emat_debug_* test hooks and the profiling builds' read-outs: entry points that are no part of the product.
//
// Included by emat_backend.hip after the product entry points.
#ifndef EMAT_DEBUG_HOST_HPP_
#define EMAT_DEBUG_HOST_HPP_

namespace {

// What a hook that runs device code on one part needs first: the last pass checked, the model and the slabs on the device, and --
// `need_derived`, for the hooks that start from the nodes' lambda_i and missing-site counts as a move does -- those recalculated.
emat_status debug_settle(emat_backend* h, bool need_derived) {
  emat_status st = emat_synchronize(h); if (st) return st;
  st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  return need_derived && !h->derived_valid ? launch_recalc(h) : EMAT_OK;
}

}  // namespace

extern "C" {

emat_status emat_debug_slab_layout(emat_backend* h, int32_t part_id, uint32_t* out8) {
  if (!h || !out8 || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_coal) return fail(h, EMAT_ERR_STATE, "no coalescent parts built");
  const PartHost& ph = h->parts[part_id];
  const int trace_cap = h->cfg.trace_moves > 0 ? h->cfg.trace_moves : 0;
  const uint32_t content = heap_content_bytes(ph.tree);
  const SlabGeo g = slab_geometry(h, ph.tree.num_nodes(), ph.tree.num_muts(), content, (int)ph.coal.k_bar_p.size(), ph.includes_run_root, ph.space_boost, ph.cell_boost);
  out8[0] = (uint32_t)sizeof(SlabHeader); out8[1] = (uint32_t)ph.tree.num_nodes() * (uint32_t)sizeof(NodeRec) + miss_dl_bytes_for((uint32_t)ph.tree.num_nodes()); out8[2] = a16((uint32_t)g.cell_cap * cell_bytes_for(ph.includes_run_root));
  out8[3] = a16((uint32_t)trace_cap * 32u); out8[4] = content; out8[5] = g.heap; out8[6] = g.scratch; out8[7] = (uint32_t)g.cell_cap;
  return EMAT_OK;
}
/* test hook (header: emat_debug_gamma) */
emat_status emat_debug_gamma(emat_backend* h, int32_t mode, int32_t n, const double* a, const double* x_or_q, double* out) {
  if (!h || n < 0 || (mode != 0 && mode != 1) || (n > 0 && (!a || !x_or_q || !out))) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return EMAT_OK;
  DevBuf<double> da, dx, dout;
  HIP_TRY(da.upload(a, (size_t)n)); HIP_TRY(dx.upload(x_or_q, (size_t)n)); HIP_TRY(dout.upload(x_or_q, (size_t)n));
  hipLaunchKernelGGL(k_debug_gamma, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, da.p, dx.p, dout.p, n, mode);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
/* test hooks (header: emat_debug_pop, emat_debug_interval_op) */
emat_status emat_debug_pop(emat_backend* h, const emat_pop_model* pm, int32_t op, int32_t n, const double* a, const double* b, double* out) {
  if (!h || !pm || n < 0 || op < 0 || op > 2 || (n > 0 && (!a || !b || !out))) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (n == 0) return EMAT_OK;
  HostPopModel hp;
  try { hp = HostPopModel::from_c(*pm); } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  DevBuf<double> dx, dg, da, db, dout;
  HIP_TRY(dx.upload(hp.x.data(), hp.x.size())); HIP_TRY(dg.upload(hp.gamma.data(), hp.gamma.size()));
  HIP_TRY(da.upload(a, (size_t)n)); HIP_TRY(db.upload(b, (size_t)n)); HIP_TRY(dout.alloc((size_t)n));
  PopTable pt{};
  pt.kind = hp.kind; pt.skygrid_type = hp.skygrid_type; pt.skygrid_num_knots = (int)hp.x.size();
  for (int i = 0; i < 4; ++i) pt.p[i] = hp.p[i];
  pt.t_c = hp.t_c; pt.skygrid_x = dx.p; pt.skygrid_gamma = dg.p;
  pt.skygrid_inv_dx = (hp.x.size() >= 2 && hp.x.back() > hp.x.front()) ? (double)(hp.x.size() - 1) / (hp.x.back() - hp.x.front()) : 0.0;
  pt.skygrid_x0 = hp.x.empty() ? 0.0 : hp.x.front();
  hipLaunchKernelGGL(k_debug_pop, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, pt, (int)op, da.p, db.p, dout.p, (int)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
emat_status emat_debug_interval_op(emat_backend* h, int32_t op, const int32_t* a, int32_t na, const int32_t* b, int32_t nb, int32_t* out, int32_t* n_out) {
  if (!h || !n_out || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b) || !out) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  DevBuf<IvRec> dA, dB, dO; DevBuf<int> dn;
  HIP_TRY(dA.upload((const IvRec*)a, (size_t)na)); HIP_TRY(dB.upload((const IvRec*)b, (size_t)(op == 5 ? 0 : nb))); HIP_TRY(dO.alloc(2 * (size_t)(na + nb + 1))); HIP_TRY(dn.alloc(1));
  hipLaunchKernelGGL(k_debug_interval_op, dim3(1), dim3(64), 0, h->stream, (int)op, dA.p, (int)na, dB.p, (int)(op == 5 ? 0 : nb), op == 5 && nb > 0 ? b[0] : 0, dO.p, dn.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  int cnt = 0;
  HIP_TRY(hipMemcpy(&cnt, dn.p, sizeof(int), hipMemcpyDeviceToHost));
  if (cnt < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_interval_op: unknown op");
  *n_out = cnt;
  if ((op <= 3 || op == 7 || op == 8) && cnt > 0) HIP_TRY(hipMemcpy(out, dO.p, (size_t)cnt * sizeof(IvRec), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
/* test hook (header: emat_debug_tree_query) */
emat_status emat_debug_tree_query(emat_backend* h, int32_t part_id, int32_t op, int32_t n, const int32_t* a, const int32_t* b, int32_t* out) {
  if (!h || n < 0 || (op != 0 && op != 1) || (n > 0 && (!a || !b || !out))) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  const int nn = h->parts[part_id].n_nodes;
  for (int i = 0; i < n; ++i) if (a[i] < -1 || a[i] >= nn || b[i] < -1 || b[i] >= nn) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_tree_query: node index out of range");
  if (n == 0) return EMAT_OK;
  emat_status st = debug_settle(h, false); if (st) return st;
  DevBuf<int32_t> da, db, dout;
  HIP_TRY(da.upload(a, (size_t)n)); HIP_TRY(db.upload(b, (size_t)n)); HIP_TRY(dout.alloc((size_t)n));
  KernelArgs ka = make_args(h);
  hipLaunchKernelGGL(k_debug_tree_query, dim3(1), dim3(k_wave), 0, h->stream, ka, (int)part_id, (int)op, da.p, db.p, dout.p, (int)n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
/* test hook (header: emat_debug_miss_dl_check) */
emat_status emat_debug_miss_dl_check(emat_backend* h, int32_t* out_2n) {
  if (!h || !out_2n) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->parts.empty()) return EMAT_OK;
  emat_status st = debug_settle(h, false); if (st) return st;   // (no recalculation: it would forget what is to be checked)
  DevBuf<int32_t> dout;
  HIP_TRY(dout.alloc(2 * h->parts.size()));
  return run_over_parts(h, k_debug_miss_dl_check, dout.p, out_2n, 2 * h->parts.size(), dout.p);
}
/* test hook (header: emat_debug_graft) */
emat_status emat_debug_graft(emat_backend* h, int32_t part_id, int32_t X, double mu_proposal, int32_t mode, int32_t new_sibling, double new_t_P,
                             double* out, int32_t out_cap, int32_t* out_len) {
  if (!h || !out || !out_len || out_cap < 2 || mode < 0 || mode > 3) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  const int nn = h->parts[part_id].n_nodes;
  if (X < 0 || X >= nn || (mode == 3 && (new_sibling < 0 || new_sibling >= nn))) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_graft: node index out of range");
  emat_status st = debug_settle(h, true); if (st) return st;
  DevBuf<double> dout; DevBuf<int32_t> dlen;
  HIP_TRY(dout.alloc((size_t)out_cap)); HIP_TRY(dlen.alloc(1));
  KernelArgs ka = make_args(h);
  hipLaunchKernelGGL(k_debug_graft, dim3(1), dim3(k_wave), 0, h->stream, ka, (int)part_id, (int)X, mu_proposal, (int)mode, (int)new_sibling, new_t_P, dout.p, (int)out_cap, dlen.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_len, dlen.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)std::min(*out_len, out_cap) * sizeof(double), hipMemcpyDeviceToHost));
  if (mode >= 1) h->device_wrote_slabs();   // the part's slab was edited on the device
  if (out[0] != 0.0) return fail(h, EMAT_ERR_INTERNAL, "emat_debug_graft: the device code stopped with part status " + std::to_string((int)out[0]));
  return *out_len > out_cap ? fail(h, EMAT_ERR_CAPACITY, "emat_debug_graft: out_cap too small") : EMAT_OK;
}
/* test hook (header: emat_debug_sample_history) */
emat_status emat_debug_sample_history(emat_backend* h, int32_t part_id, int32_t n, const int32_t* branch, const double* t_end, const uint8_t* start_seq, double T, double mu,
                                      int32_t* counts, double* muts, int32_t muts_cap, int32_t* num_muts) {
  if (!h || n < 0 || !branch || !t_end || !start_seq || !counts || !muts || muts_cap < 0 || !num_muts) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  const int nn = h->parts[part_id].n_nodes;
  for (int i = 0; i < n; ++i) if (branch[i] < 0 || branch[i] >= nn) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_sample_history: node index out of range");
  emat_status st = debug_settle(h, true); if (st) return st;
  DevBuf<int32_t> db, dc, ds; DevBuf<double> dt, dm; DevBuf<uint8_t> dseq;
  HIP_TRY(db.upload(branch, (size_t)std::max(n, 1))); HIP_TRY(dt.upload(t_end, (size_t)std::max(n, 1))); HIP_TRY(dseq.upload(start_seq, (size_t)h->cfg.num_sites));
  HIP_TRY(dc.alloc((size_t)std::max(n, 1))); HIP_TRY(dm.alloc((size_t)std::max(muts_cap, 1) * 4)); HIP_TRY(ds.alloc(2));
  KernelArgs ka = make_args(h);
  hipLaunchKernelGGL(k_debug_sample_history, dim3(1), dim3(k_wave), 0, h->stream, ka, (int)part_id, (int)n, db.p, dt.p, dseq.p, T, mu, dc.p, dm.p, (int)muts_cap, ds.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  int32_t status[2];
  HIP_TRY(hipMemcpy(status, ds.p, sizeof status, hipMemcpyDeviceToHost));
  h->device_wrote_slabs();   // the part's random stream moved on
  if (status[0] != 0) return fail(h, EMAT_ERR_INTERNAL, "emat_debug_sample_history: the device code stopped with part status " + std::to_string(status[0]));
  *num_muts = status[1];
  if (n > 0) HIP_TRY(hipMemcpy(counts, dc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (status[1] > 0) HIP_TRY(hipMemcpy(muts, dm.p, (size_t)std::min(status[1], muts_cap) * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return status[1] > muts_cap ? fail(h, EMAT_ERR_CAPACITY, "emat_debug_sample_history: muts_cap too small") : EMAT_OK;
}
/* test hook (header: emat_debug_edit) */
emat_status emat_debug_edit(emat_backend* h, int32_t part_id, int32_t X, int32_t n_ops, const int32_t* op_kind, const int32_t* op_node, const double* op_t) {
  if (!h || n_ops < 0 || (n_ops > 0 && (!op_kind || !op_node || !op_t))) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  const int nn = h->parts[part_id].n_nodes;
  if (X < 0 || X >= nn) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_edit: node index out of range");
  for (int i = 0; i < n_ops; ++i) if (op_kind[i] < 0 || op_kind[i] > 3 || (op_kind[i] == 3 && (op_node[i] < 0 || op_node[i] >= nn))) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_debug_edit: bad step");
  emat_status st = debug_settle(h, true); if (st) return st;
  DevBuf<int32_t> dk, dn, ds; DevBuf<double> dt;
  HIP_TRY(dk.upload(op_kind, (size_t)std::max(n_ops, 1))); HIP_TRY(dn.upload(op_node, (size_t)std::max(n_ops, 1))); HIP_TRY(dt.upload(op_t, (size_t)std::max(n_ops, 1))); HIP_TRY(ds.alloc(1));
  KernelArgs ka = make_args(h);
  hipLaunchKernelGGL(k_debug_edit, dim3(1), dim3(k_wave), 0, h->stream, ka, (int)part_id, (int)X, (int)n_ops, dk.p, dn.p, dt.p, ds.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  int32_t status = 0;
  HIP_TRY(hipMemcpy(&status, ds.p, sizeof status, hipMemcpyDeviceToHost));
  h->device_wrote_slabs();
  if (status != 0) return fail(h, EMAT_ERR_INTERNAL, "emat_debug_edit: the device code stopped with part status " + std::to_string(status));
  return EMAT_OK;
}
/* debugging aid (not part of the boundary): how many parts the next launch runs with each code variant
 * (out3 = {whole slab staged in LDS, prefix staged, HBM only}); mirrors the kernel's per-part decision (single class). */
emat_status emat_debug_variant_counts(emat_backend* h, int32_t* out3) {
  if (!h || !out3 || h->host_only) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  st = pull_from_device(h); if (st) return st;
  out3[0] = out3[1] = out3[2] = 0;
  const uint32_t area = h->class_lds[h->num_classes - 1];
  const bool tables = h->num_partitions <= k_max_lds_partitions;
  for (auto& ph : h->parts) {
    const SlabHeader* H = (const SlabHeader*)(h->h_slabs.data() + ph.slab_off);
    const bool can = tables && area != 0 && H->off_nodes == (uint32_t)sizeof(SlabHeader);
    if (can && (H->heap_end <= area || H->heap_top + k_lds_heap_room <= area)) ++out3[0]; else if (can && H->heap_begin <= area) ++out3[1]; else ++out3[2];
  }
  return EMAT_OK;
}
/* debugging aid (profiling builds): bytes the moves' arena handed out per allocating source line, [line & 2047][LDS, HBM] */
emat_status emat_debug_arena_sites(emat_backend* h, uint64_t* out_4096) {
  if (!h || !out_4096 || h->host_only) return EMAT_ERR_INVALID_ARGUMENT;
#ifdef EMAT_PROFILE_PHASES
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpyFromSymbol(out_4096, HIP_SYMBOL(::emat::g_arena_site_bytes), sizeof(unsigned long long) * 4096));
  return EMAT_OK;
#else
  return fail(h, EMAT_ERR_STATE, "built without -DEMAT_PROFILE_PHASES");
#endif
}
/* debugging aid (profiling builds): inclusive ticks and calls of the EMAT_TIMED scopes, [header * 2048 + line & 2047][ticks, calls]; read and cleared */
emat_status emat_debug_fn_ticks(emat_backend* h, uint64_t* out_12288) {
  if (!h || !out_12288 || h->host_only) return EMAT_ERR_INVALID_ARGUMENT;
#if defined(EMAT_PROFILE_PHASES) || defined(EMAT_COUNT_CALLS)
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> z((size_t)12288 * ::emat::k_fn_replicas, 0);
  HIP_TRY(hipMemcpyFromSymbol(z.data(), HIP_SYMBOL(::emat::g_fn_ticks), sizeof(unsigned long long) * z.size()));
  for (int k = 0; k < 12288; ++k) { unsigned long long sum = 0; for (int r = 0; r < ::emat::k_fn_replicas; ++r) sum += z[(size_t)r * 12288 + k]; out_12288[k] = sum; }
  std::fill(z.begin(), z.end(), 0ull);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(::emat::g_fn_ticks), z.data(), sizeof(unsigned long long) * z.size()));
  const unsigned min_lists = h->cfg_fn_min_lists;   // from the next pass on: only parts whose lists take at least this many bytes
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(::emat::g_fn_min_list_bytes), &min_lists, sizeof(min_lists)));
  return EMAT_OK;
#else
  return fail(h, EMAT_ERR_STATE, "built without -DEMAT_PROFILE_PHASES");
#endif
}
/* debugging aid: how much LDS arena the moves of every main-class part start with (bytes; -1 for parts of side classes) */
emat_status emat_debug_arena_bytes(emat_backend* h, int32_t* out_n) {
  if (!h || !out_n || h->host_only) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  st = pull_from_device(h); if (st) return st;
  const uint32_t area = h->class_lds[h->num_classes - 1];
  for (size_t p = 0; p < h->parts.size(); ++p) {
    const SlabHeader* H = (const SlabHeader*)(h->h_slabs.data() + h->parts[p].slab_off);
    if (h->class_of[p] != h->num_classes - 1) { out_n[p] = -1; continue; }
    const uint32_t want = (H->heap_top + k_lds_heap_room + 15u) & ~15u;
    uint32_t used;
    if (H->heap_end <= area) used = std::min(H->heap_end, want); else if (want <= area) used = want; else used = (H->heap_begin + 15u) & ~15u;
    out_n[p] = used <= area ? (int32_t)(area - ((used + 15u) & ~15u)) : 0;
  }
  return EMAT_OK;
}
/* debugging aid (not part of the boundary): duration and start tick (100 MHz wall clock) of every part in the last pass */
emat_status emat_debug_part_ticks(emat_backend* h, int64_t* out_2n) {
  if (!h || !out_2n || h->host_only || !h->slabs_on_device) return EMAT_ERR_INVALID_ARGUMENT;
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  { emat_status js = wait_for_side_classes(h); if (js) return js; }
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_2n, h->d_part_ticks.p, sizeof(int64_t) * 2 * h->parts.size(), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
/* debugging aid: workgroup entry and exit ticks (100 MHz) of the first 8 tickets of every part in the last pass, out[(2 * ticket + {0, 1}) * num_parts + part] */
emat_status emat_debug_ticket_ticks(emat_backend* h, int64_t* out_16n) {
  if (!h || !out_16n || h->host_only || !h->slabs_on_device) return EMAT_ERR_INVALID_ARGUMENT;
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  { emat_status js = wait_for_side_classes(h); if (js) return js; }
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_16n, h->d_part_ticks.p + 2 * h->parts.size(), sizeof(int64_t) * 2 * k_ticket_log * h->parts.size(), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
/* debugging aid (not part of the boundary): phase profile of a part, see EMAT_PROFILE_PHASES */
emat_status emat_debug_phase_ticks(emat_backend* h, int32_t part_id, int64_t* out16) {
  if (!h || !out16 || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = pull_from_device(h); if (st) return st;
  const SlabHeader* H = (const SlabHeader*)(h->h_slabs.data() + h->parts[part_id].slab_off);
#ifdef EMAT_PROFILE_PHASES
  for (int i = 0; i < 16; ++i) out16[i] = H->phase_ticks[i];
  if (h->cfg_phase_extra) for (int i = 0; i < 16; ++i) out16[i] = ((const int64_t*)H->reserved)[i];   // scan and arena counters instead
#else
  (void)H; for (int i = 0; i < 16; ++i) out16[i] = 0;   // phase counters exist only in -DEMAT_PROFILE_PHASES builds
#endif
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_DEBUG_HOST_HPP_
