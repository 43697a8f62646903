// emat_pass_host.hpp -- a pass over the parts: model and slabs onto the device (sync_model_to_device, materialize), the launches
// (launch_recalc, launch_moves, build_order), what follows a launch (finish_pass) and the two ways back to the host (pull_from_device,
// pull_headers).
//
// Included by emat_backend.hip after emat_slab_host.hpp.
#ifndef EMAT_PASS_HOST_HPP_
#define EMAT_PASS_HOST_HPP_

namespace {

// The streams the side launches of a pass fork onto: one small pool per device for the whole process.  The runtime maps
// streams onto a handful of hardware queues (four by default) and two streams on one queue run one after the other, so
// handles that come and go must not each bring streams of their own.  (The current device is the caller's.)
hipStream_t side_stream(int device, int i) {
  static std::mutex mu;
  static std::vector<std::array<hipStream_t, emat_backend::k_max_classes - 1>> pool;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)pool.size() <= device) pool.resize((size_t)device + 1, std::array<hipStream_t, emat_backend::k_max_classes - 1>{});
  if (!pool[device][i] && hipStreamCreate(&pool[device][i]) != hipSuccess) return nullptr;
  return pool[device][i];
}

emat_status sync_model_to_device(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return no_device(h);
  if (!h->model_dirty) return EMAT_OK;
  auto& B = *h;
  HIP_TRY(B.d_ref.upload(B.ref.data(), B.ref.size()));
  HIP_TRY(B.d_part.upload(B.partition_for_site.data(), B.partition_for_site.size()));
  HIP_TRY(B.d_nu.upload(B.nu_l.data(), B.nu_l.size()));
  HIP_TRY(B.d_cumQ.upload(B.cumQ.data(), B.cumQ.size()));
  HIP_TRY(B.d_cum_nu.upload(B.cum_nu.data(), B.cum_nu.size()));
  HIP_TRY(B.d_mu.upload(B.mu.data(), B.mu.size()));
  HIP_TRY(B.d_pi.upload(B.pi.data(), B.pi.size()));
  HIP_TRY(B.d_q.upload(B.q.data(), B.q.size()));
  HIP_TRY(B.d_ref_freqs.upload(B.ref_freqs.data(), B.ref_freqs.size()));
  HIP_TRY(B.d_sky_x.upload(B.pop.x.data(), B.pop.x.size()));
  HIP_TRY(B.d_sky_g.upload(B.pop.gamma.data(), B.pop.gamma.size()));
  PopTable pt{};
  pt.kind = B.pop.kind; pt.skygrid_type = B.pop.skygrid_type; pt.skygrid_num_knots = (int)B.pop.x.size();
  for (int i = 0; i < 4; ++i) pt.p[i] = B.pop.p[i];
  pt.t_c = B.pop.t_c; pt.skygrid_x = B.d_sky_x.p; pt.skygrid_gamma = B.d_sky_g.p;
  pt.skygrid_inv_dx = (B.pop.x.size() >= 2 && B.pop.x.back() > B.pop.x.front()) ? (double)(B.pop.x.size() - 1) / (B.pop.x.back() - B.pop.x.front()) : 0.0;
  pt.skygrid_x0 = B.pop.x.empty() ? 0.0 : B.pop.x.front();
  HIP_TRY(B.d_pop.upload(&pt, 1));
  B.model_dirty = false;
  return EMAT_OK;
}

// reference_cum_Q and state frequencies of the reference sequence (phylo_tree_calc.cpp:379-388, :95-106)
void refresh_ref_derived(emat_backend* h) {
  const int L = h->L;
  h->cumQ.assign(L + 1, 0.0);
  double so_far = 0.0;
  for (int l = 0; l < L; ++l) {
    const int p = h->partition_for_site[l];
    so_far += h->mu[p] * h->nu_l[l] * (-h->q[p * 16 + h->ref[l] * 5]);
    h->cumQ[l + 1] = so_far;
  }
  {   // prefix table for k_global_stats: cum_nu[k][beta][a] = sum over sites l < k of partition beta with reference state a of nu_l
    const int W = 4 * h->num_partitions;
    h->cum_nu.assign((size_t)(L + 1) * W, 0.0);
    for (int l = 0; l < L; ++l) {
      const double* prev = &h->cum_nu[(size_t)l * W]; double* next = &h->cum_nu[(size_t)(l + 1) * W];
      for (int k = 0; k < W; ++k) next[k] = prev[k];
      next[4 * h->partition_for_site[l] + h->ref[l]] += h->nu_l[l];
    }
  }
  h->uniform_sites = h->num_partitions == 1 && !h->cfg_no_uniform_sites && std::all_of(h->nu_l.begin(), h->nu_l.end(), [](double x) { return x == 1.0; });
  h->ref_freqs.assign((size_t)h->num_partitions * 4, 0);
  for (int l = 0; l < L; ++l) ++h->ref_freqs[h->partition_for_site[l] * 4 + h->ref[l]];
  h->model_dirty = true;
}
// THE tail of every call that wrote a model into h->mu, pi, q or nu_l (emat_set_evo and the moves that draw one), by emat_set_evo's rules: what is derived from it
// with the reference sequence follows, and what the slabs maintain belongs to the old one (Subrun::set_evo, subrun.h:29-30).  The site partitions and the sequence stay.
void install_model(emat_backend* h) { refresh_ref_derived(h); h->model_changed(); }

KernelArgs make_args(emat_backend* h) {
  KernelArgs a{};
  a.slabs = h->d_slabs.p; a.slab_off = h->d_slab_off.p; a.order = h->d_order.p; a.part_status = h->d_part_status.p; a.moves_for_part = nullptr; a.part_ticks = h->d_part_ticks.p; a.ref_freqs = h->d_ref_freqs.p; a.cum_nu = h->d_cum_nu.p; a.stats_out = h->d_stats.p;
  a.evo.num_sites = h->L; a.evo.num_partitions = h->num_partitions; a.evo.uniform_sites = h->uniform_sites ? 1 : 0; a.evo.pad_ = 0;
  a.evo.ref_sequence = h->d_ref.p; a.evo.partition_for_site = h->d_part.p; a.evo.nu_l = h->d_nu.p; a.evo.cum_Q_l = h->d_cumQ.p;
  a.evo.mu = h->d_mu.p; a.evo.pi = h->d_pi.p; a.evo.q = h->d_q.p;
  a.pop = h->d_pop.p; a.shared = h->shared_dev; a.flags = h->flags; a.num_parts = (int)h->parts.size();
  a.lds_slab_bytes = 0; a.lds_scratch_bytes = 0; a.moves_per_part = 0; a.extra_moves_part0 = 0; a.one_more_below = 0; a.chunks = 1; a.class_count = 0; a.class_stride = 0; a.chunk_done = nullptr; a.snaps = nullptr;
  return a;
}

// Launch order for the NEXT passes from the durations measured in the last one: within each size class, the part that
// took longest goes first.  The dispatcher hands workgroups to free slots in index order, so this is longest-processing-
// time-first list scheduling with real times instead of the size proxy (correlation 0.44 at C4); a chain's cost changes
// slowly from pass to pass.  Called with the stream idle.
emat_status refresh_order_from_ticks(emat_backend* h) {
  const size_t n = h->parts.size();
  if (!h->order_valid || n == 0 || !h->cfg_order_by_time) return EMAT_OK;
  std::vector<int64_t> ticks(n);
  HIP_TRY(hipMemcpy(ticks.data(), h->d_part_ticks.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int32_t>& order = h->h_order;
  for (int c = 0; c < h->num_classes; ++c)
    std::stable_sort(order.begin() + h->class_begin[c], order.begin() + h->class_begin[c + 1], [&](int a, int b) { return ticks[a] > ticks[b]; });
  HIP_TRY(h->d_order.upload(order.data(), order.size()));
  return EMAT_OK;
}

// The side classes of a pass run on streams of their own and the engine's stream does not wait for them when the pass is launched
// (the next pass of the main class need not, and they are the longest chains of a pass): whoever is about to read or change
// slabs on the engine's stream joins them first -- and the side streams must then see what it did there before their next launches
// (sides_must_fork, whatever becomes of the join: emat_begin_upload goes on after a failed one).  The two read-outs of the parts'
// ticks, which put no work on the engine's stream, only wait.
emat_status wait_for_side_classes(emat_backend* h) {
  if (!h->sides_in_flight) return EMAT_OK;
  for (int c = 1; c < emat_backend::k_max_classes; ++c) if (h->class_stream[c]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join[c], 0));
  h->sides_in_flight = false;
  return EMAT_OK;
}
emat_status join_side_classes(emat_backend* h) { h->sides_must_fork = true; return wait_for_side_classes(h); }

// The run-wide coalescent cell arrays (SharedCells, emat_slab.hpp) from the host's copies of the parts: every part carries the
// run's values over its own window, and the windows agree where they overlap.
emat_status upload_shared_cells(emat_backend* h) {
  int total = 0;
  for (const PartHost& ph : h->parts) total = std::max(total, ph.coal.cell_first + (int)ph.coal.k_twiddle_bar.size());
  const double nan = std::numeric_limits<double>::quiet_NaN();
  h->sh_ktw.assign((size_t)total, nan); h->sh_popsize.assign((size_t)total, nan); h->sh_tsop.assign((size_t)total, nan); h->sh_nact.assign((size_t)total, -1);
  for (const PartHost& ph : h->parts) {
    const HostCoalPart& c = ph.coal;
    for (size_t w = 0; w < c.k_twiddle_bar.size(); ++w) {
      const size_t i = (size_t)c.cell_first + w;
      if (ph.includes_run_root && h->sh_nact[i] >= 0) continue;   // (cells the root part appended carry its own values: never over another part's)
      h->sh_ktw[i] = c.k_twiddle_bar[w]; h->sh_popsize[i] = c.popsize_bar[w]; h->sh_tsop[i] = c.t_step / c.popsize_bar[w]; h->sh_nact[i] = c.num_active_parts[w];
    }
  }
  HIP_TRY(h->d_sh_ktw.upload(h->sh_ktw.data(), h->sh_ktw.size())); HIP_TRY(h->d_sh_tsop.upload(h->sh_tsop.data(), h->sh_tsop.size())); HIP_TRY(h->d_sh_nact.upload(h->sh_nact.data(), h->sh_nact.size()));
  h->shared_dev = SharedCells{h->d_sh_ktw.p, h->d_sh_tsop.p, h->d_sh_nact.p, total};
  h->grid_mirrors_on_device = false;
  return EMAT_OK;
}

// The per-part device words of a pass, sized for `parts` parts and zeroed on the engine's stream: the status of every part, and its ticks
// (entry / exit of the part, + entry / exit of the first k_ticket_log tickets of every part).
emat_status reset_part_words(emat_backend* h, size_t parts) {
  const size_t ticks = (2 + 2 * k_ticket_log) * parts;
  HIP_TRY(h->d_part_ticks.alloc(ticks)); HIP_TRY(hipMemsetAsync(h->d_part_ticks.p, 0, ticks * sizeof(int64_t), h->stream));
  HIP_TRY(h->d_part_status.alloc(parts)); HIP_TRY(hipMemsetAsync(h->d_part_status.p, 0, parts * sizeof(int32_t), h->stream));
  return EMAT_OK;
}

// Encode all parts and push them to the device.
emat_status materialize(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return no_device(h);
  if (h->slabs_on_device) return EMAT_OK;
  if (!h->have_ref || !h->have_evo) return fail(h, EMAT_ERR_STATE, "set_ref_sequence and set_evo must precede running");
  if (!h->have_coal) return fail(h, EMAT_ERR_STATE, "emat_build_coalescent_parts must precede running");
  const int trace_cap = h->cfg.trace_moves > 0 ? h->cfg.trace_moves : 0;
  const bool may_keep = h->derived_valid;   // (a model or reference sequence set since then invalidates what finish_pass kept)
  uint64_t off = 0; h->max_slab_bytes = 0; h->persistent_bytes.assign(h->parts.size(), 0); h->prefix_bytes.assign(h->parts.size(), 0);
  std::vector<SlabGeo> geo(h->parts.size());
  for (size_t p = 0; p < h->parts.size(); ++p) {
    PartHost& ph = h->parts[p];
    // encode_slab writes 16-bit list counts: what reaches it was accepted at upload (<= k_max_list_upload) or came back from the
    // device (whose lists stop at k_max_list_len: k_part_list_limit) -- checked here all the same, so that no count is ever cut
    { emat_flat_tree v = ph.tree.view(); const std::string lim = flat_tree_list_limit(v, (int32_t)k_max_list_len); if (!lim.empty()) return fail(h, EMAT_ERR_CAPACITY, "part " + std::to_string(p) + ": " + lim); }
    const uint32_t content = heap_content_bytes(ph.tree);
    geo[p] = slab_geometry(h, ph.tree.num_nodes(), ph.tree.num_muts(), content, (int)ph.coal.k_bar_p.size(), ph.includes_run_root, ph.space_boost, ph.cell_boost);
    place_slab(h, p, geo[p], off, content);
  }
  HIP_TRY(h->h_slabs.resize(off)); h->slab_bytes_total = off;
  std::vector<uint64_t> offs(h->parts.size());
  parallel_for((int)h->parts.size(), [&](int p) {
    PartHost& ph = h->parts[p];
    offs[p] = ph.slab_off;
    encode_slab(ph, h->h_slabs.data() + ph.slab_off, ph.slab_bytes, geo[p].heap, geo[p].scratch, geo[p].cell_cap, trace_cap);
    // carry the statistics over re-materialisations
    SlabHeader* H = (SlabHeader*)(h->h_slabs.data() + ph.slab_off);
    H->moves_done = ph.stats.moves_done; for (int k = 0; k < 5; ++k) { H->proposed[k] = ph.stats.proposed[k]; H->accepted[k] = ph.stats.accepted[k]; }
    H->alg_bytes = ph.stats.algorithmic_bytes; H->alg_write16 = (uint32_t)(ph.stats.algorithmic_write_bytes / 16); H->device_ticks = ph.stats.device_ticks;
    if (may_keep && ph.derived_kept && (int)ph.kept_lambda.size() == H->n_nodes) {   // a re-materialisation in the middle of a pass: the maintained values go on as they are (PartHost)
      NodeRec* N = (NodeRec*)(h->h_slabs.data() + ph.slab_off + H->off_nodes);
      for (int i = 0; i < H->n_nodes; ++i) { N[i].lambda = ph.kept_lambda[(size_t)i]; N[i].n_missing = ph.kept_n_missing[(size_t)i]; }
      H->log_G = ph.kept_log_G; H->log_aug_prior = ph.kept_log_aug_prior;
      if ((int)ph.kept_miss_dl.size() == H->n_nodes) std::memcpy(N + H->n_nodes, ph.kept_miss_dl.data(), (size_t)H->n_nodes * 8);   // (bits, the "not known" ones included)
    } else ph.derived_kept = false;
  });
  bool all_kept = !h->parts.empty();
  for (PartHost& ph : h->parts) { all_kept = all_kept && ph.derived_kept; ph.derived_kept = false; }
  assign_size_classes(h);
  h->order_valid = false;
  { emat_status st = upload_shared_cells(h); if (st) return st; }
  HIP_TRY(h->d_slabs.upload(h->h_slabs.data(), h->h_slabs.size()));
  HIP_TRY(h->d_slab_off.upload(offs.data(), offs.size()));
  { emat_status st = reset_part_words(h, h->parts.size()); if (st) return st; }
  HIP_TRY(hipStreamSynchronize(h->stream));   // (everything else here is a blocking copy: the zeros have landed too when this returns, whichever stream runs the parts next)
  h->slabs_on_device = true; h->host_slabs_current = true; h->derived_valid = all_kept;
  return EMAT_OK;
}

// How this device deals the workgroups of a launch to its XCDs: the number of XCDs if workgroup b runs on XCD b mod that number
// (what MI300-class parts do in their default partition mode), 1 if there is one XCD, 0 if the pattern is anything else.  Asked
// once per device and process; the kernels' own per-ticket check (run_moves_body) is what a pass relies on.
// (On the caller's stream, never the null stream: once a process has used the null stream it holds one of the runtime's four hardware
// queues for good, and with two handles alive -- bench.py's engine and its run driver -- a main stream then shares a queue with a
// side stream and waits 15-19 ms per pass for that stream's kernel: whole cycles of 48 ms instead of 29.)
int probe_xcc_dealing(int device, hipStream_t stream) {
  static std::mutex mu; static int known[64]; static bool asked[64] = {};
  std::lock_guard<std::mutex> lock(mu);
  if (device < 0 || device >= 64) return 0;
  if (asked[device]) return known[device];
  asked[device] = true; known[device] = 0;
  const int nb = 2048;
  int32_t* d = nullptr; std::vector<int32_t> x((size_t)nb, -1);
  if (hipMalloc((void**)&d, nb * sizeof(int32_t)) != hipSuccess) return 0;
  hipLaunchKernelGGL(k_probe_xcc, dim3(nb), dim3(64), 0, stream, d);
  const bool ok = hipMemcpyAsync(x.data(), d, nb * sizeof(int32_t), hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
  (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); return 0; }
  int nx = 0; for (int v : x) nx = std::max(nx, v + 1);
  if (nx <= 0 || nx > 16) return 0;
  for (int b = 0; b < nb; ++b) if (x[(size_t)b] != (x[0] + b) % nx) nx = -1;
  if (verbose_reports()) fprintf(stderr, "[emat] device %d: workgroups are dealt to %s\n", device, nx > 0 ? (std::to_string(nx) + " XCD(s) round robin").c_str() : "the XCDs in no pattern the tickets can rely on: full releases");
  known[device] = nx > 0 ? nx : 0;
  return known[device];
}

emat_status launch_recalc(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  emat_status st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  // the kernel rewrites lambda, missing-site counts and the totals of EVERY part, the parts of the side classes included: their
  // launches of the last pass must have ended, and their next ones must follow this one (every caller -- emat_recalc_derived
  // directly after emat_run_* as well -- goes through here)
  st = join_side_classes(h); if (st) return st;
  KernelArgs a = make_args(h);
  hipLaunchKernelGGL(k_recalc_derived, dim3((unsigned)h->parts.size()), dim3(k_wave), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  h->device_recalculated();
  return EMAT_OK;
}

// Launch order: one workgroup per part, largest persistent state first.  The hardware dispatcher hands workgroups to
// free slots in index order, which makes it a longest-processing-time-first list scheduler (size and duration of a
// part correlate at 0.85); packing lists of parts per workgroup on the host was measured slower twice.  The order only
// decides WHEN a part's chain runs; every chain is independent (own RNG stream, own slab).
// (`queued`: the copy goes onto the engine's stream behind whatever is running there -- for a caller that knows nothing in flight
// reads the order -- instead of waiting for the stream first.)
emat_status build_order(emat_backend* h, bool queued = false) {
  const int n = (int)h->parts.size();
  // by class, then by persistent size, largest first, ties in index order: a stable radix sort (three passes of 12 bits) on
  // (class, ~size); the comparison sort this replaces took half a millisecond of every cycle at 13 000 parts
  std::vector<uint64_t> key((size_t)n), key2((size_t)n);
  std::vector<int32_t> order((size_t)n), order2((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  auto sort_key = [&](int i) { return ((uint64_t)h->class_of[(size_t)i] << 32) | (uint64_t)(0xFFFFFFFFu - h->persistent_bytes[(size_t)i]); };   // 36 bits (k_max_classes <= 16)
  for (int i = 0; i < n; ++i) key[(size_t)i] = sort_key(i);
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = 12 * pass;
    uint32_t count[4097] = {};
    for (int i = 0; i < n; ++i) ++count[((key[(size_t)i] >> shift) & 0xFFFu) + 1];
    for (int d = 0; d < 4096; ++d) count[d + 1] += count[d];
    for (int i = 0; i < n; ++i) { const uint32_t at = count[(key[(size_t)i] >> shift) & 0xFFFu]++; key2[at] = key[(size_t)i]; order2[at] = order[(size_t)i]; }
    key.swap(key2); order.swap(order2);
  }
  h->h_order = order;
  // (from the pageable member: measured in round 6 against a page-locked staging copy, which gained nothing here and made the
  // like copies of emat_tree_partition WAIT for the stream; h_order lives as long as the handle)
  if (queued) { HIP_TRY(h->d_order.alloc(order.size())); HIP_TRY(hipMemcpyAsync(h->d_order.p, h->h_order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream)); }
  else { HIP_TRY(hipStreamSynchronize(h->stream)); HIP_TRY(h->d_order.upload(order.data(), order.size())); }
  h->order_valid = true;
  return EMAT_OK;
}

emat_status launch_moves(emat_backend* h, int64_t per_part, int64_t extra0, const std::vector<int64_t>* counts = nullptr, int32_t one_more_below = 0) {
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  if (h->fatal_status != EMAT_OK) return fail(h, h->fatal_status, h->fatal_message);
  HostLaps laps;
  emat_status st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  laps.mark("launch_moves: 1 model + materialize");
  if (!h->derived_valid) { st = join_side_classes(h); if (st) return st; st = launch_recalc(h); if (st) return st; }
  laps.mark("launch_moves: 2 launch_recalc");
  const uint32_t lds_scratch = h->cfg.use_lds ? h->cfg_lds_scratch : 0u;
  // the dynamic block: the slab image beyond its header + the arena; tables, context and the header image are static LDS
  auto shmem_for = [&](uint32_t slab_area) { return (size_t)(slab_area > (uint32_t)sizeof(SlabHeader) ? slab_area - (uint32_t)sizeof(SlabHeader) : 0u) + lds_scratch; };
  for (int c = 0; c < h->num_classes; ++c)
    if (shmem_for(h->class_lds[c]) + k_lds_static_bytes + sizeof(SlabHeader) > 160 * 1024) return fail(h, EMAT_ERR_CAPACITY, "LDS request exceeds 160 KiB: lower EMAT_LDS_MAX or disable use_lds");
  if (!h->order_valid) { st = build_order(h); if (st) return st; }
  laps.mark("launch_moves: 3 build_order (sort, wait for the stream, H2D)");
  HIP_TRY(h->d_snaps.alloc(h->d_slabs.n));   // (as roomy as the slabs: grows when they do)
  laps.mark("launch_moves: 4 snapshot allocation");
  KernelArgs a = make_args(h);
  a.moves_per_part = per_part; a.extra_moves_part0 = extra0; a.one_more_below = one_more_below;
  a.lds_scratch_bytes = lds_scratch; a.snaps = h->d_snaps.p;
  if (counts) { st = join_side_classes(h); if (st) return st; HIP_TRY(hipStreamSynchronize(h->stream)); HIP_TRY(h->d_moves_for_part.upload(counts->data(), counts->size())); a.moves_for_part = h->d_moves_for_part.p; }
  else { h->expected_moves.resize(h->parts.size(), 0); for (size_t p = 0; p < h->parts.size(); ++p) h->expected_moves[p] += per_part + (p == 0 ? extra0 : 0) + ((int64_t)p < one_more_below ? 1 : 0); }
  h->pass_pending = true;
  h->last_launch_uniform = counts == nullptr;
  HIP_TRY(hipEventRecord(h->ev_start, h->stream));
  {
    const size_t sh_max = shmem_for(*std::max_element(h->class_lds, h->class_lds + h->num_classes));
    if (sh_max > 48 * 1024) {
      // the attribute belongs to the kernel on this device, not to the handle: raised when a request exceeds what any handle of
      // the process has asked for so far (two driver calls that used to sit in front of every pass)
      static std::mutex mu; static size_t granted[64] = {};
      std::lock_guard<std::mutex> lock(mu);
      size_t& g = granted[h->cfg.device & 63];
      if (sh_max > g) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_run_moves, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh_max));
        HIP_TRY(hipFuncSetAttribute((const void*)k_run_moves_side, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh_max));
        g = sh_max;
      }
    }
    const int main_class = h->num_classes - 1;   // the last class holds the bulk of the parts
    // Order matters: a side class holds few, large workgroups (tens of KB of LDS each), which can only be placed while
    // the CUs are not yet packed with the 10 KB workgroups of the main class -- arriving second they would wait for
    // several neighbours to finish (measured: the root part started 10-15 ms into the pass).  So the side classes are
    // launched first, largest area first, each on a stream of its own, the main class last on the engine's stream.  The
    // engine's stream does not wait for them here (join_side_classes): a side class only ever follows its own previous launch
    // -- the parts of different classes have nothing to do with each other -- so that in back-to-back passes the main class of the
    // next pass starts when the main class of this one ends, and the side launches of the next pass, queued behind their
    // predecessors, find their LDS while this pass's main class drains.  They wait for the engine's stream only when it did
    // something since the last pass was checked (uploads, recalculation: sides_must_fork).  The timing events bracket the main class.
    // Tickets pay when there are more parts than wave slots (4 waves x 4 SIMDs per CU): with fewer, every part has a slot to
    // itself from the start and a second ticket could only wait behind its first while holding another slot.
    const int main_count = h->class_begin[h->num_classes] - h->class_begin[h->num_classes - 1];
    const int chunks = (counts == nullptr && per_part >= 4 * h->cfg_chunks && (h->cfg_chunks_forced || main_count > 4 * EMAT_WAVES_PER_EU * h->num_cus)) ? h->cfg_chunks : 1;
    if (chunks > 1) { HIP_TRY(h->d_chunk_done.alloc(h->parts.size() + 130)); HIP_TRY(hipMemsetAsync(h->d_chunk_done.p, 0, (h->parts.size() + 130) * sizeof(int32_t), h->stream)); }   // + 64 eight-byte counters of waiting time
    // (the counter the side workgroups of a synchronised pass report to, zeroed before the event the side streams wait for)
    int side_wgs = 0; for (int c = 0; c + 1 < h->num_classes; ++c) side_wgs += h->class_begin[c + 1] - h->class_begin[c];
    const bool hold_main = h->sides_must_fork && side_wgs > 0;
    if (hold_main) { HIP_TRY(h->d_side_started.alloc(1)); HIP_TRY(hipMemsetAsync(h->d_side_started.p, 0, sizeof(int32_t), h->stream)); }
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    for (int c = 0; c < h->num_classes; ++c) {
      const int lo = h->class_begin[c], cnt = h->class_begin[c + 1] - lo;
      if (cnt <= 0) continue;
      KernelArgs b = a;
      b.order = a.order + lo; b.lds_slab_bytes = h->class_lds[c];
      // (only the main class: a side class has fewer workgroups than the device has room for, so all its tickets would be
      // resident at once and the waiting ones would sit on tens of KB of LDS each -- measured: cycles of 72 ms instead of 37)
      b.taper = h->cfg_taper ? 1 : 0;
      for (int k = 0; k < 8; ++k) b.cum_w[k] = 0;
      if (h->cfg_taper && chunks == 4) { b.cum_w[0] = 10; b.cum_w[1] = 16; b.cum_w[2] = 19; b.cum_w[3] = 20; }   // 10 : 6 : 3 : 1 (measured best of the ratios tried)
      if (const char* e = h->cfg_ticket_weights.empty() ? nullptr : h->cfg_ticket_weights.c_str()) { int acc = 0, k = 0; for (const char* q = e; *q && k < 8;) { acc += std::max(1, atoi(q)); b.cum_w[k++] = acc; while (*q && *q != ',') ++q; if (*q == ',') ++q; } if (k != chunks) for (int j = 0; j < 8; ++j) b.cum_w[j] = 0; }
      b.chunks = c == main_class ? chunks : 1; b.class_count = cnt; b.class_stride = (cnt + 7) & ~7; b.chunk_done = h->d_chunk_done.p;
      // Testing knobs.  Option "ticket_xcd_spread" = 1 makes the stride odd, so that consecutive tickets of a part land on DIFFERENT XCDs
      // (workgroups go round the eight XCDs by index): the hand-over then has to cross L2s, which the default placement avoids
      // but does not rely on -- what a ticket hands over goes out through agent-scope write-through stores and the next ticket
      // acquires at agent scope.  Option "ticket_release" = "full" takes the plain agent-scope release for every ticket.
      if (h->cfg_ticket_spread) b.class_stride = cnt | 1;
      // the cheap hand-over only where a part's tickets share an XCD: workgroups are dealt to the XCDs round robin (verified on this
      // device by probe_xcc_dealing, and re-checked by every ticket), so the stride must be a multiple of their number
      b.single_below = (c == main_class && chunks > 1) ? std::min(h->cfg_single_ticket_parts, cnt) : 0;
      b.full_release = (h->cfg_ticket_full_release || h->xcc_count <= 0 || b.class_stride % h->xcc_count != 0) ? 1 : 0;
      const unsigned grid = b.chunks > 1 ? (unsigned)(b.chunks * b.class_stride) : (unsigned)cnt;
      const bool side = c != main_class;
      hipStream_t sm = side ? h->class_stream[c + 1] : h->stream;
      if (side && h->sides_must_fork) HIP_TRY(hipStreamWaitEvent(sm, h->ev_fork, 0));
      b.side_started = (side && hold_main) ? h->d_side_started.p : nullptr;
      if (c == main_class && hold_main) { hipLaunchKernelGGL(k_wait_side_start, dim3(1), dim3(64), 0, sm, h->d_side_started.p, side_wgs); HIP_TRY(hipGetLastError()); }
      if (c == main_class) hipLaunchKernelGGL(k_run_moves, dim3(grid), dim3(k_wave), shmem_for(h->class_lds[c]), sm, b);
      else hipLaunchKernelGGL(k_run_moves_side, dim3(grid), dim3(k_wave), shmem_for(h->class_lds[c]), sm, b);
      HIP_TRY(hipGetLastError());
      if (side) { HIP_TRY(hipEventRecord(h->ev_join[c + 1], sm)); h->sides_in_flight = true; }
    }
    h->sides_must_fork = false;
  }
  HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
  laps.mark("launch_moves: 5 expected moves, events, memsets, launches");
  h->device_wrote_slabs();
  return EMAT_OK;
}

emat_status pull_from_device_impl(emat_backend* h) {
  if (h->host_only || !h->slabs_on_device || h->host_slabs_current) return EMAT_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->grid_mirrors_on_device) {   // the run-wide cell arrays of a grid built on the device: decode_slab reads them
    const size_t nc = (size_t)h->shared_dev.num_cells;
    h->sh_ktw.resize(nc); h->sh_popsize.resize(nc); h->sh_tsop.resize(nc); h->sh_nact.resize(nc);
    HIP_TRY(hipMemcpy(h->sh_ktw.data(), h->shared_dev.k_twiddle_bar, nc * 8, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(h->sh_popsize.data(), h->gt.co_popsize.p, nc * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->sh_tsop.data(), h->shared_dev.ts_over_pop, nc * 8, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(h->sh_nact.data(), h->shared_dev.num_active_parts, nc * 4, hipMemcpyDeviceToHost));
    h->grid_mirrors_on_device = false;
  }
  HIP_TRY(h->h_slabs.resize(h->slab_bytes_total));   // (grow-only; a repartition on the device does not touch the host mirror)
  HIP_TRY(hipMemcpy(h->h_slabs.data(), h->d_slabs.p, h->h_slabs.size(), hipMemcpyDeviceToHost));
  parallel_for((int)h->parts.size(), [&](int p) {
    PartHost& ph = h->parts[p];
    const uint8_t* slab = h->h_slabs.data() + ph.slab_off;
    const SlabHeader* H = (const SlabHeader*)slab;
    decode_slab(ph, slab, h->sh_ktw.empty() ? nullptr : h->sh_ktw.data(), h->sh_popsize.data(), h->sh_nact.data());
    ph.stats.status = H->status; ph.stats.num_nodes = H->n_nodes; ph.stats.moves_done = H->moves_done;
    for (int k = 0; k < 5; ++k) { ph.stats.proposed[k] = H->proposed[k]; ph.stats.accepted[k] = H->accepted[k]; }
    ph.stats.algorithmic_bytes = H->alg_bytes; ph.stats.algorithmic_write_bytes = 16 * (int64_t)H->alg_write16; ph.stats.rng_draws = (int64_t)H->rng_counter; ph.stats.device_ticks = H->device_ticks;
  });
  h->host_slabs_current = true;
  return EMAT_OK;
}

// After a launch: did every part run its chain to completion?  A part that ran out of list-heap or scratch space
// stops BEFORE a move with its state intact (status 101): it is given twice the room and the rest of its moves, up
// to four times.  Any other status means an invariant broke inside a move; that is reported, loudly, and the caller
// must not use the part's tree.
emat_status finish_pass(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->fatal_status != EMAT_OK) return fail(h, h->fatal_status, h->fatal_message);
  if (h->host_only || !h->pass_pending || !h->slabs_on_device) return EMAT_OK;
  const size_t n = h->parts.size();
  std::vector<int32_t> status(n);
  for (int round = 0; round < 5; ++round) {
    HostLaps laps;
    { emat_status js = join_side_classes(h); if (js) return js; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    laps.mark("finish_pass: 1 wait for the moves");
    HIP_TRY(hipMemcpy(status.data(), h->d_part_status.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    laps.mark("finish_pass: 2 status D2H");
    h->pass_pending = false;
    size_t stopped = 0, fatal = n;
    for (size_t p = 0; p < n; ++p) if (status[p] != 0) { ++stopped; if (status[p] != k_part_need_space && status[p] != k_part_need_cells && fatal == n) fatal = p; }
    if (stopped == 0 && verbose_reports()) {   // what bounded the pass: the slowest chains next to the mean
      std::vector<int64_t> ticks(2 * n);
      HIP_TRY(hipMemcpy(ticks.data(), h->d_part_ticks.p, 2 * n * sizeof(int64_t), hipMemcpyDeviceToHost));
      std::vector<int> idx(n); std::iota(idx.begin(), idx.end(), 0);
      std::partial_sort(idx.begin(), idx.begin() + std::min<size_t>(4, n), idx.end(), [&](int a, int b) { return ticks[a] > ticks[b]; });
      double sum = 0; int64_t first = INT64_MAX, last = 0;
      for (size_t p = 0; p < n; ++p) { sum += (double)ticks[p]; first = std::min(first, ticks[n + p]); last = std::max(last, ticks[n + p] + ticks[p]); }
      float kms = 0.f; (void)hipEventElapsedTime(&kms, h->ev_start, h->ev_stop);
      if (h->d_chunk_done.n >= n + 130) {
        std::vector<int32_t> w(130); HIP_TRY(hipMemcpy(w.data(), h->d_chunk_done.p + n, 130 * sizeof(int32_t), hipMemcpyDeviceToHost));
        double wait = 0; for (int i = 0; i < 64; ++i) { unsigned long long v; memcpy(&v, &w[(n & 1) + 2 * i], 8); wait += (double)v; }   // (the counters start at the next even index)
        fprintf(stderr, "[emat] tickets waited %.2f s of slot time for their predecessors (%.1f %% of %d slots x pass)\n", wait / 1e8, 100.0 * wait / 1e5 / (kms * 16.0 * h->num_cus), 16 * h->num_cus);
      }
      fprintf(stderr, "[emat] pass: main class %.1f ms on the device (all chains: first start to last end %.1f ms) | chains: mean %.2f ms, slowest", kms, (last - first) / 1e5, sum / n / 1e5);
      for (size_t k = 0; k < std::min<size_t>(4, n); ++k) fprintf(stderr, " %.1f ms from %.1f (part %d, %d nodes%s)", ticks[idx[k]] / 1e5, (ticks[n + idx[k]] - first) / 1e5, idx[k], h->parts[idx[k]].n_nodes, idx[k] == h->root_part ? ", root part" : "");
      std::partial_sort(idx.begin(), idx.begin() + std::min<size_t>(3, n), idx.end(), [&](int a, int b) { return ticks[n + a] + ticks[a] > ticks[n + b] + ticks[b]; });
      fprintf(stderr, " | last to end:");
      for (size_t k = 0; k < std::min<size_t>(3, n); ++k) fprintf(stderr, " part %d (%d nodes, %u B) %.1f ms from %.1f", idx[k], h->parts[idx[k]].n_nodes, h->persistent_bytes[idx[k]], ticks[idx[k]] / 1e5, (ticks[n + idx[k]] - first) / 1e5);
      fprintf(stderr, "\n");
    }
    if (stopped == 0) { if (round == 0 && h->last_launch_uniform) (void)refresh_order_from_ticks(h); laps.mark("finish_pass: 3 status scan + refresh_order_from_ticks"); return EMAT_OK; }
    h->device_wrote_slabs();
    emat_status st = pull_from_device_impl(h); if (st) return st;   // (bound, not failed, nothing pending: pull_from_device's own checks hold here)
    if (fatal != n) {
      const SlabHeader* H = (const SlabHeader*)(h->h_slabs.data() + h->parts[fatal].slab_off);
      h->fatal_status = (status[fatal] == k_part_cell_overflow || status[fatal] == k_part_list_limit) ? EMAT_ERR_CAPACITY : EMAT_ERR_INTERNAL;
      h->fatal_message = "part " + std::to_string(fatal) + " stopped inside a move with status " + std::to_string(status[fatal]) + " (device source line " + std::to_string(H->fail_line) +
                         "); " + std::to_string(stopped) + " part(s) stopped in all";
      if (H->fail_line == -3)
        h->fatal_message += ": the dynamic LDS block of k_run_moves does not start where the device code was compiled to find it (k_lds_dyn_base): the library was not built with "
                            "-mllvm -amdgpu-lower-module-lds-strategy=module (csrc/Makefile)";
      else if (H->fail_line == k_fail_line_other_xcd)
        h->fatal_message += ": a ticket found that its predecessor had handed the part over on another XCD (the cheap hand-over is only valid behind one L2; the device did not "
                            "deal this launch's workgroups to its XCDs as probed): run with EMAT_TICKET_RELEASE=full";
      if (status[fatal] == k_part_list_limit)
        h->fatal_message += ": a per-node list would exceed " + std::to_string(k_max_list_len) + " entries (16-bit list counts, emat_slab.hpp): nothing was truncated, the run cannot continue";
      return fail(h, h->fatal_status, h->fatal_message);
    }
    if (round == 4) return fail(h, EMAT_ERR_CAPACITY, std::to_string(stopped) + " part(s) still out of slab space after four doublings");
    std::vector<int64_t> counts(n, 0);
    for (size_t p = 0; p < n; ++p) if (status[p] != 0) {
      PartHost& ph = h->parts[p];
      if (status[p] == k_part_need_cells) ph.cell_boost *= 4; else ph.space_boost *= 2.0;
      counts[p] = h->expected_moves[p] - ph.stats.moves_done;
      ph.stats.status = 0;
    }
    if (verbose_reports()) fprintf(stderr, "[emat] %zu part(s) ran out of slab space or grid cells: re-materialising with more room and running the rest of their moves\n", stopped);
    if (h->derived_valid) {   // (h_slabs is what pull_from_device just decoded: the slabs as the pass left them)
      parallel_for((int)n, [&](int p) {
        PartHost& ph = h->parts[(size_t)p];
        const uint8_t* slab = h->h_slabs.data() + ph.slab_off;
        const SlabHeader* H = (const SlabHeader*)slab; const NodeRec* N = (const NodeRec*)(slab + H->off_nodes);
        ph.kept_lambda.resize((size_t)H->n_nodes); ph.kept_n_missing.resize((size_t)H->n_nodes);
        for (int i = 0; i < H->n_nodes; ++i) { ph.kept_lambda[(size_t)i] = N[i].lambda; ph.kept_n_missing[(size_t)i] = N[i].n_missing; }
        { const uint64_t* dl = (const uint64_t*)(N + H->n_nodes); ph.kept_miss_dl.assign(dl, dl + H->n_nodes); }
        ph.kept_log_G = H->log_G; ph.kept_log_aug_prior = H->log_aug_prior; ph.derived_kept = true;
      });
    }
    h->parts_need_encoding(true);   // every part is re-encoded from its decoded state (tree, RNG, cells, statistics, derived quantities)
    st = launch_moves(h, 0, 0, &counts, 0); if (st) return st;
  }
  return EMAT_OK;
}

emat_status pull_from_device(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->fatal_status != EMAT_OK) return fail(h, h->fatal_status, h->fatal_message);
  if (h->host_only || !h->slabs_on_device) return EMAT_OK;
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }
  return pull_from_device_impl(h);
}

// Runs a kernel that reads the settled parts -- one wavefront per part, the parts' KernelArgs first, then `args` -- on the engine's
// stream, waits for it, and copies the `count` elements it left at `d_rows` to `rows`.
template <class K, class T, class... A> emat_status run_over_parts(emat_backend* h, K kernel, const T* d_rows, T* rows, size_t count, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)h->parts.size()), dim3(k_wave), 0, h->stream, make_args(h), args...);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rows, d_rows, count * sizeof(T), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

// Dense copy of the parts' headers: what emat_get_totals / emat_part_get_stats need is 256 bytes per part, not the slabs.
emat_status pull_headers(emat_backend* h) {
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->fatal_status != EMAT_OK) return fail(h, h->fatal_status, h->fatal_message);
  if (h->host_only || !h->slabs_on_device) return EMAT_OK;
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }
  if (h->headers_current) return EMAT_OK;
  const size_t n = h->parts.size();
  h->h_headers.resize(n * sizeof(SlabHeader));
  if (h->host_slabs_current) {
    for (size_t p = 0; p < n; ++p) std::memcpy(h->h_headers.data() + p * sizeof(SlabHeader), h->h_slabs.data() + h->parts[p].slab_off, sizeof(SlabHeader));
  } else {
    HIP_TRY(h->d_headers.alloc(n * sizeof(SlabHeader)));
    emat_status st = run_over_parts(h, k_gather_headers, h->d_headers.p, h->h_headers.data(), n * sizeof(SlabHeader), h->d_headers.p); if (st) return st;
  }
  h->headers_current = true;
  return EMAT_OK;
}
inline const SlabHeader* header_of(const emat_backend* h, size_t part) { return (const SlabHeader*)(h->h_headers.data() + part * sizeof(SlabHeader)); }

// What a kernel that only READS the parts needs before it is launched: the settled parts, on the device.
emat_status require_settled_parts(emat_backend* h) {
  if (h->host_only) return no_device(h);                                             // nothing to launch on
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");        // nothing to launch over
  emat_status st = sync_model_to_device(h); if (st) return st;                       // the model the kernel reads
  st = materialize(h); if (st) return st;                                            // the slabs, if the parts are still host records
  return h->pass_pending ? finish_pass(h) : EMAT_OK;                                 // chains that finished their moves, or a loud failure
}

}  // namespace

#endif  // EMAT_PASS_HOST_HPP_
