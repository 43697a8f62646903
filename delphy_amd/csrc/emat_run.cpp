// emat_run.cpp -- host-side driver above the engine boundary (include/emat_host.h).
//
// Restates, on the host and in plain C++, the part of reference `Run` that orchestrates the local-move
// hot path: random partition stencils (core/tree_partitioning.h:139-194), partition_tree (:196-239),
// Run::repartition (core/run.cpp:110-193), Run::normalize_root (:258-265), Run::push_global_params_to_subruns
// (:267-275), Run::run_local_moves (:682-693) and Run::reassemble (:195-256).  Global moves
// (run.cpp:695-1235) are out of scope and are not here.
//
// One translation unit, cut by concern into headers included in this order:
//   emat_run_partition.hpp   compact topology, stencils, part-size refinement, partition_tree, the draw of a cycle (PartitionDraw)
//   emat_run_tree.hpp        the host tree model (HTree), normalize_root, cut-point states, subtree builder, gather
//   emat_run_exchange.hpp    the exchange format of part subtrees between processes
// This file keeps the driver's state and its transitions, the two cycles (host-owned tree, tree resident in HBM) and the C-ABI.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/emat_host.h"
#include "emat_gamma_pure.hpp"     // the generator the global moves' keys are drawn from
#include "emat_move_specs.hpp"     // what their specs must satisfy, in the backend's words
#include "flat_tree.hpp"
#include "host_parallel.hpp"
#include "synth.hpp"
#include "emat_run_partition.hpp"
#include "emat_run_tree.hpp"
#include "emat_run_exchange.hpp"

#define EMAT_TRY(expr) do { if (emat_status emat_try_st_ = (expr)) return emat_try_st_; } while (0)   // a failed step ends the entry point with its status

namespace emat {

struct RunDriver {
  emat_backend* backend = nullptr;
  std::string last_error;
  HTree tree;
  std::vector<uint8_t> ref;
  int L = 0;
  uint64_t seed = 0;
  int num_parts = 1;
  int max_part_nodes = 0;   // 0 = the reference's partition rule exactly (the default, so that a drop-in Run reproduces the reference / oracle partition); opt-in, not in the reference (see refine_stencil, emat_run_partition.hpp): > 0 = parts larger than this are cut further at every repartition, -1 = three times the mean part size
  int last_num_parts = 0, last_largest_part = 0;   // of the last repartition (emat_run_partition_stats)
  // model
  bool have_hky = false; double hky_mu = 0, hky_kappa = 1, hky_pi[4] = {0.25, 0.25, 0.25, 0.25};
  std::vector<double> nu_l;
  bool site_rate_moves_on = false; double site_rate_alpha = 1.0; uint64_t site_rate_rounds = 0;   // Run::alpha_ and how many rounds of site-rate moves have drawn a key
  bool have_pop = false; emat_pop_model pop{}; std::vector<double> sky_x, sky_g;
  bool skygrid_moves_on = false; emat_skygrid_spec sky_spec{}; uint64_t skygrid_rounds = 0;   // Run's Skygrid settings with skygrid_tau_, and how many rounds of the Skygrid moves have drawn a key
  bool exp_pop_moves_on = false; emat_exp_pop_spec xp_spec{}; uint64_t exp_pop_rounds = 0;      // Run's Exp_pop_model settings, and how many rounds of the Exponential moves have drawn a key
  bool subst_moves_on = false; emat_subst_spec sb_spec{}; uint64_t subst_rounds = 0;            // Run's mu prior and switches (the model is hky_* above), and how many rounds of the substitution-model moves have drawn a key
  // The APOBEC (mpox) model (Run::set_mpox_hack_enabled, run.cpp:359-398): two site partitions cut by the APOBEC context of the sequence at node 0, mu and mu* of its own
  // (hky_mu is handed over at enabling and handed back at disabling), Run's mu prior with its switch and the number of rounds, and how many rounds of its moves have drawn a key
  bool mpox_on = false; emat_mpox_spec mx_spec{}; double mpox_mu = 0, mpox_mu_star = 0; std::vector<int32_t> mpox_partition_for_site; int mpox_context_sites = 0; uint64_t mpox_rounds = 0;
  double t_step = 1.0; bool t_step_set = false;
  int only_displacing_inner_nodes = 0, topology_moves_enabled = 1;
  bool reference_remainder = false;   // the remainder of count / parts goes to part 0 as in Run::run_local_moves (run.cpp:683-689), instead of one move per part
  bool paranoid = false;   // Run::paranoid (run.h:220-224): check the incrementally maintained quantities of every part after every pass
  // partition state
  Topology tp;               // of the tree as of the last sync_topology / fetch_device_topology
  PartitionDraw draw;        // this run's draws: its own, or taken from `follow` (emat_run_follow_draws: same process, same seed, same tree)
  const PartitionDraw* follow = nullptr;
  std::vector<PartMap> parts; PartKids part_kids; std::vector<FlatTree> subtrees; std::vector<uint64_t> part_seeds;   // parts stay flat (SoA + CSR) end to end
  int root_part = -1;
  uint64_t epoch = 0;
  // A run sharded over several processes (one GPU each): every process holds the whole tree and cuts it
  // identically; the attached backend only gets the parts [part_lo, part_hi) (backend part id = part - part_lo).
  int shard_rank = 0, shard_world = 1, part_lo = 0, part_hi = 0;
  std::vector<uint64_t> part_epoch;   // epoch at which each part's subtree was last refreshed (downloaded or received)
  // The whole tree resident in HBM (emat_tree_* of the backend): this driver then only sees topology and
  // node times (tp); `tree` is brought up to date on demand (ensure_host_tree).
  bool device_tree = false;

  // ---- Where things stand.  Six flags, written only by the transitions below them.
  bool parts_uploaded = false;         // the parts of the current partition are out on the device
  bool model_pushed = false;           // the backend has the reference sequence, evolution model and flags as they are here
  bool coal_built = false;             // ... and coalescent parts built from the population model as it is here
  bool device_tree_uploaded = false;   // device_tree: the tree has gone to the device
  bool host_tree_stale = false;        // device_tree: the device's tree has moved on since `tree` was last brought up to date
  bool partition_on_device = false;    // the current partition was made by emat_tree_partition: parts[p].orig / part_kids are filled on demand
  bool tree_cut = false;               // between a repartition and the reassemble that follows it: the parts, not `tree` / the tree in HBM, hold the state (a host tree's parts stay uploaded after it)
  void model_changed() { model_pushed = false; }                 // HKY parameters, flags, or the reference sequence (hence cum_Q)
  void model_went_out() { model_pushed = true; }
  void pop_model_changed() { coal_built = false; }
  void coalescent_built() { coal_built = true; }                 // (a sharded run: begun here, the caller finishes the stages on the backend)
  void parts_cut(bool on_device) { partition_on_device = on_device; }
  void host_parts_rebuilt() { parts_uploaded = false; coal_built = false; }                       // new subtrees on the host: nothing of them on the device yet
  void parts_went_out() { parts_uploaded = true; }
  void device_parts_went_out() { parts_uploaded = true; coal_built = true; host_tree_stale = true; }   // emat_tree_repartition: slabs and coalescent tables, cut from the device's tree, which the moves now change
  void device_parts_came_back() { parts_uploaded = false; host_tree_stale = true; }               // the device gathered them into its tree
  void tree_went_to_device() { device_tree_uploaded = true; host_tree_stale = false; }
  void host_copy_refreshed() { host_tree_stale = false; }
  void device_tree_switched(bool on) { device_tree = on; device_tree_uploaded = false; }          // on: uploaded at the next repartition
  void shard_changed() { parts_uploaded = false; }

  emat_status fail(emat_status st, const std::string& m) { last_error = m; return st; }
  emat_status bk(emat_status st) { if (st != EMAT_OK) last_error = std::string("backend: ") + emat_last_error(backend); return st; }

  // ---- Preconditions, one owner each.  An entry point states the ones it has, in the order in which they have always fired.
  static constexpr const char* kMovesNeedBackend = "no backend attached: the host driver never runs moves itself";
  static constexpr const char* kDeviceTreeNeedsBackend = "a device-resident tree needs a backend";
  emat_status need_backend(const char* msg = "no backend attached") { return backend ? EMAT_OK : fail(EMAT_ERR_NO_DEVICE, msg); }
  emat_status need_parts_out() { return parts_uploaded ? EMAT_OK : fail(EMAT_ERR_STATE, "repartition first"); }
  emat_status need_parts_back() { return !parts_uploaded ? EMAT_OK : fail(EMAT_ERR_STATE, "reassemble first"); }
  emat_status need_pop_model() { return have_pop ? EMAT_OK : fail(EMAT_ERR_STATE, "emat_run_set_pop_model must be called first"); }
  emat_status need_local_parts() { return part_hi > part_lo ? EMAT_OK : fail(EMAT_ERR_STATE, "this rank holds no parts: fewer parts than processes"); }

  // ---- What the backend is handed with the parts, one owner each.
  emat_pop_model pop_view() const { emat_pop_model pm = pop; pm.skygrid_x = sky_x.data(); pm.skygrid_gamma = sky_g.data(); return pm; }   // (the knots are this object's copies)
  double default_t_step() const {   // Run keeps ~400 cells over the tree span (run.cpp:20, :734-747)
    double lo = device_tree && tp.n > 0 ? tp.root_t : tree.nodes[tree.root].t, hi = tree.t_max_tip();
    double span = hi - lo; if (!(span > 0)) span = 1.0;
    return std::max(span / 400.0, 1.0 / 400.0);
  }
  double coalescent_step() const { return t_step_set ? t_step : default_t_step(); }
  int local_root_part() const { return (root_part >= part_lo && root_part < part_hi) ? root_part - part_lo : -1; }   // the root part as this rank's backend knows it
  uint64_t seed_for_part(int p) const {   // a fresh RNG stream per part and cycle
    uint64_t z = seed ^ (0x9E3779B97F4A7C15ull * (epoch + 1)) ^ ((uint64_t)p << 32 | (uint64_t)p);
    SplitMix64 sm(z);
    return sm.next();
  }
  void draw_part_seeds() { part_seeds.assign(parts.size(), 0); for (size_t p = 0; p < parts.size(); ++p) part_seeds[p] = seed_for_part((int)p); }
  void shard_block(int n) {   // contiguous block of the parts for this process (sizes differ by at most one)
    const int base = n / shard_world, rem = n % shard_world;
    part_lo = shard_rank * base + std::min(shard_rank, rem);
    part_hi = part_lo + base + (shard_rank < rem ? 1 : 0);
  }
  int effective_limit() const { return effective_max_part_nodes(max_part_nodes, num_parts, (size_t)tp.n); }   // needs tp

  // ---- The tree and its topology, wherever the authoritative copy lives.
  emat_status fetch_device_topology() {   // device-resident tree: what the backend mirrored at its last upload / reassemble
    static_assert(sizeof(Kids) == 2 * sizeof(int32_t), "Kids is a pair of int32");
    const int32_t* k = nullptr; int32_t n = 0;
    EMAT_TRY(bk(emat_tree_get_kids(backend, &k, &n, &tp.root, &tp.root_t)));
    tp.kids = (const Kids*)k; tp.n = n;
    return EMAT_OK;
  }
  // `tree` (and `ref`) as of the last reassemble, when the authoritative copy lives on the device
  emat_status ensure_host_tree() {
    if (!device_tree || !host_tree_stale) return EMAT_OK;
    int32_t nn, nm, ni, nf;
    EMAT_TRY(bk(emat_tree_get_sizes(backend, &nn, &nm, &ni, &nf)));
    FlatTree f; f.allocate(nn, nm, ni, nf);
    emat_flat_tree v = f.view();
    EMAT_TRY(bk(emat_tree_download(backend, &v, ref.data())));
    tree = HTree::from_view(v);
    host_copy_refreshed();
    return EMAT_OK;
  }
  void normalize_root_of_host_tree() { if (normalize_root(tree, ref)) model_changed(); }
  emat_status ensure_partition_on_host() {
    if (!partition_on_device || parts.empty() || !parts[0].orig.empty()) return EMAT_OK;
    const int P = (int)parts.size();
    std::vector<int32_t> off((size_t)P + 1);
    EMAT_TRY(bk(emat_tree_get_partition(backend, off.data(), nullptr, nullptr, nullptr)));
    std::vector<int32_t> orig((size_t)off[P]), k0((size_t)off[P]), k1((size_t)off[P]);
    EMAT_TRY(bk(emat_tree_get_partition(backend, nullptr, orig.data(), k0.data(), k1.data())));
    part_kids.assign(P, {});
    for (int p = 0; p < P; ++p) {
      parts[p].orig.assign(orig.begin() + off[p], orig.begin() + off[p + 1]);
      part_kids[p].resize((size_t)(off[p + 1] - off[p]));
      for (int s = 0; s < off[p + 1] - off[p]; ++s) part_kids[p][s] = {k0[off[p] + s], k1[off[p] + s]};
    }
    return EMAT_OK;
  }

  // ---- The draw of a cycle's partition (PartitionDraw, emat_run_partition.hpp).  Needs tp.
  void draw_partition() { draw.draw(tp, num_parts, seed, epoch, effective_limit()); }
  emat_status ensure_draw() {   // the cut nodes of the partition of this epoch in draw.drawn
    if (follow) {
      if (!follow->has(epoch)) return fail(EMAT_ERR_STATE, "this run takes its partition draws from another one (emat_run_follow_draws), which has not drawn this cycle's yet (emat_run_draw_partition on the leader first)");
      draw.take(*follow);
      return EMAT_OK;
    }
    if (!draw.has(epoch)) draw_partition();
    return EMAT_OK;
  }
  void note_partition_stats() { last_num_parts = (int)parts.size(); last_largest_part = 0; for (auto& pm : parts) last_largest_part = std::max(last_largest_part, (int)pm.orig.size()); }

  // ---- What goes to the backend.
  emat_status push_model() {
    if (!backend) return EMAT_OK;
    if (mpox_on) return push_mpox_model();
    if (!have_hky) return fail(EMAT_ERR_STATE, "emat_run_set_hky must be called first");
    EMAT_TRY(bk(emat_set_ref_sequence(backend, ref.data(), L)));
    // Hky_model::derive_site_evo_model (evo_hky.cpp:7-50)
    const double* pi = hky_pi;
    double q[16];
    hky_derive_q(hky_kappa, pi, q);   // (emat_move_specs.hpp: the backend derives the same q after its substitution-model moves)
    std::vector<int32_t> pfs(L, 0);
    std::vector<double> nu = nu_l.empty() ? std::vector<double>(L, 1.0) : nu_l;
    EMAT_TRY(bk(emat_set_evo(backend, 1, &hky_mu, pi, q, nu.data(), pfs.data())));
    EMAT_TRY(bk(emat_set_flags(backend, tree.t_max_tip(), only_displacing_inner_nodes, topology_moves_enabled)));
    model_went_out();
    return EMAT_OK;
  }
  emat_status push_mpox_model() {   // push_model with the APOBEC model on: Run::derive_evo's other arm (run.cpp:405-432)
    EMAT_TRY(bk(emat_set_ref_sequence(backend, ref.data(), L)));
    const double mu[2] = {mpox_mu, mpox_mu}, pi[8] = {0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25};
    double q[32];
    mpox_derive_q(mpox_mu_star / mpox_mu, q, q + 16);   // (emat_move_specs.hpp: the backend derives the same q after its moves)
    std::vector<double> nu = nu_l.empty() ? std::vector<double>(L, 1.0) : nu_l;
    EMAT_TRY(bk(emat_set_evo(backend, 2, mu, pi, q, nu.data(), mpox_partition_for_site.data())));
    EMAT_TRY(bk(emat_set_flags(backend, tree.t_max_tip(), only_displacing_inner_nodes, topology_moves_enabled)));
    model_went_out();
    return EMAT_OK;
  }
  emat_status build_coalescent() {   // Run::reset_very_scalable_coalescent_parts (run.cpp:277-293)
    if (!backend) return EMAT_OK;
    EMAT_TRY(need_pop_model());
    const emat_pop_model pm = pop_view();
    EMAT_TRY(bk(emat_build_coalescent_parts(backend, &pm, root_part, coalescent_step())));
    coalescent_built();
    return EMAT_OK;
  }
  emat_status upload_parts() {
    if (!backend) return EMAT_OK;
    EMAT_TRY(need_local_parts());
    const int nloc = part_hi - part_lo;
    EMAT_TRY(bk(emat_begin_upload(backend, nloc)));
    std::atomic<int> bad{EMAT_OK};
    parallel_for(nloc, [&](int q) {   // emat_part_upload is safe to call concurrently for distinct parts
      const int p = part_lo + q;
      emat_flat_tree v = subtrees[p].view();
      emat_status s1 = emat_part_upload(backend, q, &v, p == root_part ? 1 : 0, part_seeds[p]);
      if (s1 != EMAT_OK) bad.store(s1);
    });
    if (bad.load() != EMAT_OK) return bk((emat_status)bad.load());
    EMAT_TRY(bk(emat_end_upload(backend)));
    parts_went_out();
    return EMAT_OK;
  }
  // Bring the subtrees of the local parts up to date with the device.
  emat_status download_local_parts() {
    if (!(backend && parts_uploaded)) return EMAT_OK;
    int32_t nn0, nm0, ni0, nf0;
    EMAT_TRY(bk(emat_part_get_sizes(backend, 0, &nn0, &nm0, &ni0, &nf0)));   // one D2H of all slabs, before the threads start
    std::atomic<int> bad{EMAT_OK};
    parallel_for(part_hi - part_lo, [&](int q) {
      int32_t nn, nm, ni, nf;
      emat_status st = emat_part_get_sizes(backend, q, &nn, &nm, &ni, &nf); if (st) { bad.store(st); return; }
      FlatTree f; f.allocate(nn, nm, ni, nf);
      emat_flat_tree v = f.view();
      st = emat_part_download(backend, q, &v); if (st) { bad.store(st); return; }
      f.root = v.root;
      subtrees[part_lo + q] = std::move(f);
      part_epoch[part_lo + q] = epoch;
    });
    if (bad.load() != EMAT_OK) return bk((emat_status)bad.load());
    return EMAT_OK;
  }
  // The exchange of part subtrees between processes (the format: emat_run_exchange.hpp)
  emat_status pack_local_parts(uint8_t* buf, uint64_t cap, uint64_t* needed) {
    EMAT_TRY(download_local_parts());
    uint64_t tot = 0;
    for (int p = part_lo; p < part_hi; ++p) tot += packed_bytes(subtrees[p]);
    if (needed) *needed = tot;
    if (!buf || cap < tot) return buf ? fail(EMAT_ERR_BUFFER_TOO_SMALL, "emat_run_pack_local_parts: buffer too small") : EMAT_OK;
    uint8_t* w = buf;
    for (int p = part_lo; p < part_hi; ++p) pack_part(w, p, subtrees[p]);
    return EMAT_OK;
  }
  emat_status unpack_parts(const uint8_t* buf, uint64_t bytes) {
    const uint8_t* r = buf; const uint8_t* end = buf + bytes;
    while (r < end) {
      if ((uint64_t)(end - r) < kPartHeaderBytes) return fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_unpack_parts: truncated part header");
      int32_t hdr[8]; std::memcpy(hdr, r, kPartHeaderBytes); r += kPartHeaderBytes;
      const int p = hdr[0];
      if (p < 0 || p >= (int)subtrees.size() || hdr[1] != (int)parts[p].orig.size() || hdr[2] < 0 || hdr[3] < 0 || hdr[4] < 0) return fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_unpack_parts: part does not belong to the current partition");
      FlatTree t; t.root = hdr[5];
      if (!unpack_arrays(r, end, FlatTree::Shape{hdr[1], hdr[2], hdr[3], hdr[4]}, t)) return fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_unpack_parts: truncated part");
      emat_flat_tree v = t.view();
      if (!validate_flat_tree(v, L).empty()) return fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_unpack_parts: part " + std::to_string(p) + " is not a valid tree");
      subtrees[p] = std::move(t);
      part_epoch[p] = epoch;
    }
    return EMAT_OK;
  }

  // ---- The cycle with the whole tree resident in HBM: the host draws the stencil on the topology alone; nodes, mutations and
  // missations never leave the device.  The cut itself, partition_tree, runs on the device (one thread per part, which then holds the
  // part maps already) unless the parts are few and large, where one host thread per part is the better fit and the parts are handed
  // over as four int arrays.  Everything after the cut is the same for both.
  emat_status repartition_device() {
    HostLaps laps(verbose_reports());
    EMAT_TRY(need_backend(kDeviceTreeNeedsBackend));
    EMAT_TRY(need_pop_model());
    if (!device_tree_uploaded) {
      normalize_root_of_host_tree();
      if (!model_pushed) EMAT_TRY(push_model());
      FlatTree f = tree.to_flat();
      emat_flat_tree v = f.view();
      EMAT_TRY(bk(emat_tree_upload(backend, &v)));
      tree_went_to_device();
    }
    if (!model_pushed) EMAT_TRY(push_model());
    { EMAT_SPAN("run.repartition: fetch_device_topology"); EMAT_TRY(fetch_device_topology()); }
    laps.lap(); laps.skip();
    try {
      EMAT_TRY(ensure_draw());
      const std::vector<int32_t>& stencil = *draw.drawn;
      laps.mark("run.repartition: stencil pick + refine_stencil");
      part_kids.clear();
      const size_t N = (size_t)tp.n;
      if (stencil.size() + 1 >= 64 && N / (stencil.size() + 1) <= 2048) {
        int32_t P = 0, rp = -1;
        std::vector<int32_t> psz(stencil.size() + 1, 0);
        EMAT_TRY(bk(emat_tree_partition(backend, (int32_t)stencil.size(), stencil.data(), &P, &rp, psz.data())));
        last_num_parts = P; last_largest_part = 0; for (int p = 0; p < P; ++p) last_largest_part = std::max(last_largest_part, (int)psz[(size_t)p]);
        laps.mark("run.repartition: emat_tree_partition + largest part");
        parts.assign((size_t)P, PartMap{});
        for (int p = 0; p < P; ++p) parts[p].cut_point = p < (int)stencil.size() ? stencil[p] : tp.root;
        root_part = rp; parts_cut(true);
        laps.mark("run.repartition: part maps");
      } else { root_part = partition_tree(tp, stencil, parts, part_kids); parts_cut(false); note_partition_stats(); }
      ++epoch;
    } catch (const std::exception& ex) { return fail(EMAT_ERR_INTERNAL, ex.what()); }
    laps.lap();
    const int P = (int)parts.size();
    const bool handed_over = !partition_on_device;
    std::vector<int32_t> part_off, orig, kid0, kid1;   // a partition cut on the host, flattened
    if (handed_over) {
      part_off.assign(P + 1, 0);
      for (int p = 0; p < P; ++p) part_off[p + 1] = part_off[p] + (int32_t)parts[p].orig.size();
      orig.resize(part_off[P]); kid0.resize(part_off[P]); kid1.resize(part_off[P]);
      parallel_for(P, [&](int p) {
        const int b = part_off[p], n = (int)parts[p].orig.size();
        for (int s = 0; s < n; ++s) { orig[b + s] = parts[p].orig[s]; kid0[b + s] = part_kids[p][s].first; kid1[b + s] = part_kids[p][s].second; }
      }, 64);
      laps.mark("run.repartition: partition_tree + flatten");
    }
    draw_part_seeds();
    subtrees.clear();
    shard_block(P);
    EMAT_TRY(need_local_parts());
    part_epoch.assign(P, 0);
    const emat_pop_model pm = pop_view();
    laps.lap(); laps.mark("run.repartition: seeds, shard block");
    // (a sharded run: every process has the whole tree in its HBM and cuts it identically; it builds the slabs of its own block of parts only)
    EMAT_TRY(bk(emat_tree_repartition_range(backend, P, handed_over ? part_off.data() : nullptr, handed_over ? orig.data() : nullptr, handed_over ? kid0.data() : nullptr, handed_over ? kid1.data() : nullptr,
                                            root_part, part_seeds.data(), &pm, coalescent_step(), part_lo, part_hi)));
    device_parts_went_out();
    laps.lap();
    if (laps.report) fprintf(stderr, "[emat_run] repartition (device tree): upload / topology %.1f ms | stencil + %s %.1f ms | %s %.1f ms | emat_tree_repartition %.1f ms\n",
                             laps.ms(0), handed_over ? "partition_tree" : "emat_tree_partition", laps.ms(1), handed_over ? "flatten" : "seeds", laps.ms(2), laps.ms(3));
    return EMAT_OK;
  }
  emat_status reassemble_device() {
    EMAT_TRY(need_parts_out());
    if (shard_world > 1) return fail(EMAT_ERR_STATE, "a sharded run with the tree on the devices gathers in steps, with the exchange between them (emat_tree_get_root_deltas ... emat_tree_reassemble_end, then emat_run_note_device_reassembled)");
    int32_t nd = 0;   // at most one change per site
    std::vector<int32_t> site(ref.size()); std::vector<uint8_t> from(ref.size()), to(ref.size());
    EMAT_TRY(bk(emat_tree_reassemble(backend, &nd, site.data(), from.data(), to.data(), (int32_t)ref.size())));
    for (int k = 0; k < nd; ++k) ref[site[k]] = to[k];
    device_parts_came_back();
    return EMAT_OK;
  }

  // Run::run_local_moves (run.cpp:682-693) with the remainder of count / parts spread one move per part instead of all
  // on part 0 (emat_run_moves_even explains why)
  emat_status run_moves(int64_t count) {
    const int64_t P = shard_world > 1 ? (int64_t)(part_hi - part_lo) : (int64_t)parts.size(), sub = count / P;   // (a sharded run goes through emat_run_moves_sharded)
    if (reference_remainder) return bk(emat_run_local_moves(backend, count));
    return bk(emat_run_moves_even(backend, sub, (int32_t)(count - P * sub)));
  }

  // ---- The cycle with the tree owned by the host.
  void build_subtrees_of_parts() {   // run.cpp:131-184
    HostLaps laps(verbose_reports());
    std::vector<CutState> states;
    cut_point_states(tree, parts, tp, states);
    laps.lap();
    if (laps.report) fprintf(stderr, "[emat_run] cut_point_states %.1f ms\n", laps.ms(0));
    build_subtrees(tree, ref, parts, part_kids, states, subtrees);
    draw_part_seeds();
  }
  emat_status repartition() { emat_status st = repartition_(); if (st == EMAT_OK) tree_cut = true; return st; }
  emat_status reassemble() { emat_status st = reassemble_(); if (st == EMAT_OK) tree_cut = false; return st; }
  emat_status repartition_() {   // run.cpp:110-193 (+ refresh_partition_stencils :87-108)
    if (device_tree) return repartition_device();
    HostLaps laps(verbose_reports());
    parts_cut(false);
    try {
      sync_topology(tp, tree);
      EMAT_TRY(ensure_draw());
      const std::vector<int32_t>& stencil = *draw.drawn;
      part_kids.clear();
      laps.lap();
      root_part = partition_tree(tp, stencil, parts, part_kids);
      note_partition_stats();
      if (!tree.nodes[tree.root].mfs.empty()) return fail(EMAT_ERR_INTERNAL, "root missations carry from_states");
      normalize_root_of_host_tree();
      ++epoch;
      laps.lap();
      build_subtrees_of_parts();
      laps.lap();
    } catch (const std::exception& ex) { return fail(EMAT_ERR_INTERNAL, ex.what()); }
    host_parts_rebuilt();
    shard_block((int)subtrees.size());
    part_epoch.assign(subtrees.size(), 0);
    if (backend) {
      if (!model_pushed) EMAT_TRY(push_model());
      laps.lap();
      EMAT_TRY(upload_parts());
      laps.lap();
      // a sharded run builds the coalescent parts in stages, with all-reduces the caller owns in between (emat_run_coalescent_begin)
      if (shard_world == 1) EMAT_TRY(build_coalescent());
      laps.lap();
    }
    if (laps.report) fprintf(stderr, "[emat_run] repartition: stencils %.1f ms | partition_tree + normalize_root %.1f ms | build_subtrees %.1f ms | push_model %.1f ms | upload_parts %.1f ms | build_coalescent %.1f ms\n",
                             laps.ms(0), laps.ms(1), laps.ms(2), laps.ms(3), laps.ms(4), laps.ms(5));
    return EMAT_OK;
  }

  emat_status reassemble_() {   // run.cpp:195-256
    if (device_tree) return reassemble_device();
    HostLaps laps(verbose_reports());
    try {
      EMAT_TRY(download_local_parts());
      laps.lap();
      if (shard_world > 1 && backend)
        for (size_t p = 0; p < subtrees.size(); ++p)
          if (part_epoch[p] != epoch) return fail(EMAT_ERR_STATE, "part " + std::to_string(p) + " of another rank was not received this cycle (emat_run_unpack_parts)");
      laps.lap();
      for (size_t p = 0; p < subtrees.size(); ++p) if ((size_t)subtrees[p].num_nodes() != parts[p].orig.size()) return fail(EMAT_ERR_INTERNAL, "subtree size changed");
      gather_parts(tree, parts, subtrees, root_part);
    } catch (const std::exception& ex) { return fail(EMAT_ERR_INTERNAL, ex.what()); }
    laps.lap();
    if (laps.report) fprintf(stderr, "[emat_run] reassemble: D2H + decode %.1f ms | per-part download %.1f ms | gather %.1f ms\n", laps.ms(0), laps.ms(1), laps.ms(2));
    return EMAT_OK;
  }

  // ---- The global moves: five groups (substitution model or the APOBEC model, site rates, Skygrid, Exponential population), one owner for each rule they share.
  static constexpr const char* kShardedStatistics = "a sharded run gathers the part lengths and sums S, R across ranks itself (see emat_backend.h)";
  // The five key tags (keyed_round).  A group that reads the parts out on the backend carries its tag with the noun of its texts, a population group with its own two and the model's kind.
  struct PartsGroup { const char* moves; uint64_t tag; };
  struct PopGroup { int32_t kind; const char* moves; const char* model; uint64_t tag; };
  static constexpr uint64_t kSiteRateKeyTag = 0x5349544552415445ull;                                                  // "SITERATE"
  static constexpr PartsGroup kSubstGroup{"the substitution-model moves", 0x5355425354303031ull};                   // "SUBST001"
  static constexpr PartsGroup kMpoxGroup{"the APOBEC model's moves", 0x4D504F584D4F5631ull};                        // "MPOXMOV1"
  static constexpr PopGroup kSkygridGroup{EMAT_POP_SKYGRID, "the Skygrid moves", "a Skygrid population model", 0x534B594752494431ull};                  // "SKYGRID1"
  static constexpr PopGroup kExpPopGroup{EMAT_POP_EXP, "the Exponential population moves", "an exponential population model", 0x455850504F503031ull};   // "EXPPOP01"
  // What a setter asks of its spec: there, and passing the backend's own checks (emat_move_specs.hpp), refused in its words behind the setter's name `w`.
  template <class Spec, class Fault> emat_status check_moves_spec(const std::string& w, const Spec* spec, Fault fault) {
    if (!spec) return fail(EMAT_ERR_INVALID_ARGUMENT, w + "spec must not be null");
    if (const char* why = fault(*spec)) return fail(EMAT_ERR_INVALID_ARGUMENT, w + why);
    return EMAT_OK;
  }
  // One round of a group: the key from the group's counter under its tag, the caller's trace buffer handed through, the counter bumped only when the backend did the round.
  template <class Result, class Call> emat_status keyed_round(uint64_t& rounds, uint64_t tag, const Result* out, Result& res, Call&& call) {
    uint32_t w[4]; philox4x32_10_pure(rounds, seed ^ tag, w);
    if (out) { res.trace = out->trace; res.trace_capacity = out->trace_capacity; }
    const emat_status st = bk(call((uint64_t)w[0] | ((uint64_t)w[1] << 32)));
    if (st == EMAT_OK) ++rounds;
    return st;
  }

  // Run::alpha_moves + gibbs_sample_all_nus (run.cpp:1105-1235) on the device, from the statistics the device computes.
  emat_status Ttwiddle_ext(const double* tree_length_of_part, int32_t* ext_offset, int32_t* ext_node, double* ext_length, int32_t capacity, int32_t* count);   // (both below, with the tree of parts)
  emat_status get_Ttwiddle_l(double* Ttwiddle_l);
  emat_status site_rate_moves(emat_site_rate_result* out) {
    EMAT_TRY(need_backend());
    EMAT_TRY(need_parts_out());
    if (shard_world > 1) return fail(EMAT_ERR_STATE, kShardedStatistics);
    std::vector<double> Tt((size_t)L); std::vector<int32_t> M((size_t)L);
    EMAT_TRY(get_Ttwiddle_l(Tt.data()));
    EMAT_TRY(bk(emat_get_num_muts_l(backend, M.data())));
    emat_site_rate_result res{};
    EMAT_TRY(keyed_round(site_rate_rounds, kSiteRateKeyTag, out, res, [&](uint64_t key) { return emat_site_rate_moves(backend, Tt.data(), M.data(), site_rate_alpha, 10 /* run.cpp:1193 */, key, &res); }));
    // the backend holds the new rates already; kept here so that the next push sends the same values
    site_rate_alpha = res.alpha;
    nu_l.resize((size_t)L);
    EMAT_TRY(bk(emat_get_nu_l(backend, nu_l.data())));
    if (out) *out = res;
    return EMAT_OK;
  }

  // One round of a group that runs on the device from the statistics of the parts out there, which never leave it: the preconditions, the backend's call, the tail.  The group's
  // caller brings the spec with the run's model in it and takes the new model out of `res`: the backend holds it already, the next push sends it again.
  template <class Spec, class Result, class OnParts>
  emat_status parts_round(const PartsGroup& g, uint64_t& rounds, const Spec& spec, Result* out, Result& res, OnParts on_parts) {
    EMAT_TRY(need_backend());
    EMAT_TRY(need_parts_out());
    if (!tree_cut) return fail(EMAT_ERR_STATE, std::string(g.moves) + " read the parts: repartition first");
    if (shard_world > 1) return fail(EMAT_ERR_STATE, kShardedStatistics);
    EMAT_TRY(keyed_round(rounds, g.tag, out, res, [&](uint64_t key) { return on_parts(backend, &spec, key, &res); }));
    if (out) *out = res;
    return EMAT_OK;
  }
  // Run::mu_move, then sb_spec.rounds times hky_frequencies_move + hky_kappa_move (run.cpp:703-719): emat_parts_subst_moves.
  emat_status subst_moves(emat_subst_result* out) {
    EMAT_TRY(mpox_bars_subst_moves());
    emat_subst_spec spec = sb_spec;
    spec.mu = hky_mu; spec.kappa = hky_kappa; for (int a = 0; a < 4; ++a) spec.pi[a] = hky_pi[a];
    emat_subst_result res{};
    EMAT_TRY(parts_round(kSubstGroup, subst_rounds, spec, out, res, emat_parts_subst_moves));
    hky_mu = res.mu; hky_kappa = res.kappa; for (int a = 0; a < 4; ++a) hky_pi[a] = res.pi[a];
    return EMAT_OK;
  }

  // ---- The APOBEC (mpox) model: Run::set_mpox_hack_enabled (run.cpp:359-398) and Run::mpox_hack_moves (:823-951).
  // The model's mu IS the run's mu, and the substitution-model moves would draw it a second time and install an HKY q: the two groups are the two arms of
  // one branch (run.cpp:703-719).  Both directions of the exclusion are decided here.
  emat_status mpox_bars_subst_moves() { return mpox_on ? fail(EMAT_ERR_STATE, "the APOBEC model is on (emat_run_set_mpox): its moves take the place of the substitution-model moves") : EMAT_OK; }
  emat_status set_mpox(int32_t on, const emat_mpox_spec* spec) {
    const std::string w = "emat_run_set_mpox: ";
    if (!on) {   // :389-396
      if (!mpox_on) return EMAT_OK;
      mpox_on = false; mpox_partition_for_site.clear(); mpox_context_sites = 0;
      hky_mu = mpox_mu;
      model_changed();
      return EMAT_OK;
    }
    EMAT_TRY(check_moves_spec(w, spec, [](const emat_mpox_spec& s) { const char* why = mpox_spec_fault(s, false); return why ? why : rounds_limit_fault(s.rounds); }));
    if (subst_moves_on) return fail(EMAT_ERR_STATE, w + "the substitution-model moves are on (emat_run_set_subst_moves): the APOBEC model's moves take their place");
    if (mpox_on) { const double mu_star = mx_spec.mu_star; mx_spec = *spec; mx_spec.mu_star = mu_star; return EMAT_OK; }   // already on (:360): the switches alone; the partition, mu and mu* stay
    if (!have_hky) return fail(EMAT_ERR_STATE, w + "emat_run_set_hky must be called first");
    if (!finite_positive(hky_mu)) return fail(EMAT_ERR_INVALID_ARGUMENT, w + "the run's mu must be finite and positive");
    if (tree_cut) return fail(EMAT_ERR_STATE, w + "the sequence at node 0 is read from the assembled tree: reassemble first");
    EMAT_TRY(ensure_host_tree());
    if (tree.nodes.empty() || !tree.nodes[0].is_tip()) return fail(EMAT_ERR_STATE, w + "node 0 of the tree is not a tip");   // :365-366
    // view_of_sequence_at(tree_, 0) (phylo_tree_calc.cpp:19-35): the reference sequence with the mutations from the root down to node 0 applied in order
    std::vector<int32_t> path;
    for (int32_t v = 0; v != EMAT_NO_NODE; v = tree.nodes[(size_t)v].parent) { path.push_back(v); if (path.size() > tree.nodes.size()) return fail(EMAT_ERR_INTERNAL, w + "the tree has a cycle"); }
    std::vector<uint8_t> seq = ref;
    for (size_t k = path.size(); k-- > 0;) for (const HMut& m : tree.nodes[(size_t)path[k]].muts) if (m.site >= 0 && m.site < L) seq[(size_t)m.site] = m.to;
    mpox_partition_for_site.assign((size_t)L, 0);
    mpox_context_sites = apobec_context_partition(seq.data(), L, mpox_partition_for_site.data());   // :369-382
    mx_spec = *spec;
    mpox_mu = hky_mu; mpox_mu_star = spec->mu_star;   // :387-388 (the reference starts mu* at 0)
    mpox_on = true;
    model_changed();
    return EMAT_OK;
  }
  // `rounds` rounds of the Gibbs draws of mu and rho: emat_parts_mpox_moves.
  emat_status mpox_moves(emat_mpox_result* out) {
    EMAT_TRY(need_backend());   // (asked here as well: a run without a backend is told so before it is told that the model is off)
    if (!mpox_on) return fail(EMAT_ERR_STATE, "the APOBEC model is off: emat_run_set_mpox first");
    emat_mpox_spec spec = mx_spec;
    spec.mu = mpox_mu; spec.mu_star = mpox_mu_star;
    emat_mpox_result res{};
    EMAT_TRY(parts_round(kMpoxGroup, mpox_rounds, spec, out, res, emat_parts_mpox_moves));
    mpox_mu = res.mu; mpox_mu_star = res.mu_star;
    return EMAT_OK;
  }

  // The population moves (run.cpp:754-778) run on the device, on the ASSEMBLED tree, in one process, on a model of their own kind: from the tree in HBM
  // where it lives there, else from the two statistics made here from the host's tree (scalable_coalescent.cpp:88-138).
  void host_tree_coalescent_stats(double t_ref, double ts, int32_t& first_cell, std::vector<double>& k_bar, std::vector<double>& inner_t) const {
    const auto cell = [&](double t) { return (int64_t)std::floor((t - t_ref) / ts); };
    double t_last = -INFINITY;
    for (auto& n : tree.nodes) if (n.is_tip() && n.t > t_last) t_last = n.t;
    const int64_t c0 = cell(tree.nodes[tree.root].t), c1 = std::max(c0, cell(t_last));
    first_cell = (int32_t)c0; k_bar.assign((size_t)(c1 - c0 + 1), 0.0); inner_t.clear();
    const auto add = [&](double a, int64_t cs, double b) {   // add_interval(a, b, +1), :88-116
      int64_t ce = std::min(std::max(cell(b), c0), c1); cs = std::min(std::max(cs, c0), c1);
      if (cs == ce) { k_bar[(size_t)(cs - c0)] += (b - a) / ts; return; }
      k_bar[(size_t)(cs - c0)] += ((t_ref + (double)(cs + 1) * ts) - a) / ts;
      k_bar[(size_t)(ce - c0)] += (b - (t_ref + (double)ce * ts)) / ts;
      for (int64_t c = cs + 1; c < ce; ++c) k_bar[(size_t)(c - c0)] += 1.0;
    };
    for (size_t v = 0; v < tree.nodes.size(); ++v) {
      const HNode& n = tree.nodes[v];
      if (!n.is_tip()) inner_t.push_back(n.t);
      if ((int)v == tree.root) add(t_ref + (double)c0 * ts, c0, n.t);   // one lineage before the root inside its cell (:56)
      else if (n.parent != EMAT_NO_NODE) add(tree.nodes[(size_t)n.parent].t, cell(tree.nodes[(size_t)n.parent].t), n.t);
    }
  }
  // One round of a population group: the preconditions, the statistics' source, the call (the backend's on the tree, or on statistics), the tail.  The group's caller writes the new parameters into the model.
  template <class Spec, class Result, class OnTree, class OnStats>
  emat_status pop_round(const PopGroup& g, uint64_t& rounds, const Spec& spec, Result* out, Result& res, OnTree on_tree, OnStats on_stats) {
    EMAT_TRY(need_backend());
    if (tree_cut) return fail(EMAT_ERR_STATE, std::string(g.moves) + " need the tree assembled: reassemble first");
    if (shard_world > 1) return fail(EMAT_ERR_STATE, kShardedStatistics);
    EMAT_TRY(need_pop_model());
    if (pop.kind != g.kind) return fail(EMAT_ERR_INVALID_ARGUMENT, std::string(g.moves) + " need " + g.model);
    const emat_pop_model pm = pop_view();
    const double t_ref = tree.t_max_tip(), ts = coalescent_step();
    EMAT_TRY(keyed_round(rounds, g.tag, out, res, [&](uint64_t key) {
      if (device_tree && device_tree_uploaded) return on_tree(backend, &pm, &spec, t_ref, ts, key, &res);
      int32_t first_cell = 0; std::vector<double> k_bar, inner_t;
      host_tree_coalescent_stats(t_ref, ts, first_cell, k_bar, inner_t);
      return on_stats(backend, &pm, &spec, t_ref, ts, first_cell, (int32_t)k_bar.size(), k_bar.data(), (int32_t)inner_t.size(), inner_t.data(), key, &res);
    }));
    pop_model_changed();
    if (out) *out = res;
    return EMAT_OK;
  }
  // Run::skygrid_tau_move + skygrid_gammas_zero_mode_gibbs_move + skygrid_gammas_hmc_move (run.cpp:766-778)
  emat_status skygrid_moves(emat_skygrid_result* out) {
    std::vector<double> gamma(sky_g.size());
    double* user_gamma = out ? out->gamma : nullptr;
    emat_skygrid_result res{};
    res.gamma = gamma.data();
    EMAT_TRY(pop_round(kSkygridGroup, skygrid_rounds, sky_spec, out, res, emat_tree_skygrid_moves, emat_skygrid_moves));
    sky_g = gamma; sky_spec.tau = res.tau;
    if (out) { out->gamma = user_gamma; if (user_gamma) std::copy(gamma.begin(), gamma.end(), user_gamma); }   // (the curve goes to the caller's room, not the pointer to this one)
    return EMAT_OK;
  }
  // Run::pop_size_move + pop_growth_rate_move, xp_spec.rounds times (run.cpp:754-764)
  emat_status exp_pop_moves(emat_exp_pop_result* out) {
    emat_exp_pop_result res{};
    EMAT_TRY(pop_round(kExpPopGroup, exp_pop_rounds, xp_spec, out, res, emat_tree_exp_pop_moves, emat_exp_pop_moves));
    pop.p[1] = res.n0; pop.p[2] = res.g;
    return EMAT_OK;
  }

  // One cycle after another (run.cpp:622-657; of the global moves, the substitution-model, the site-rate, the Skygrid and the Exponential groups when they are on)
  emat_status do_mcmc_steps(int64_t steps, int64_t per_cycle) {
    EMAT_TRY(need_backend());
    if (shard_world > 1) return fail(EMAT_ERR_STATE, "a sharded run is cycled by its caller, who owns the collectives (see emat_host.h)");
    if (per_cycle <= 0) per_cycle = 50 * (int64_t)tree.nodes.size();
    for (int64_t done = 0; done < steps;) {
      HostLaps laps(verbose_reports());
      if (skygrid_moves_on) EMAT_TRY(skygrid_moves(nullptr));   // on the whole tree, BEFORE the repartition, which then builds the parts' tables from the new curve (emat_host.h)
      if (exp_pop_moves_on) EMAT_TRY(exp_pop_moves(nullptr));   // likewise
      EMAT_TRY(repartition());
      laps.lap(); laps.mark("cycle: 1 repartition");
      if (subst_moves_on) EMAT_TRY(subst_moves(nullptr));           // groups 1 and 2 of run_global_moves, before the site rates as there (run.cpp:703-732)
      if (mpox_on) EMAT_TRY(mpox_moves(nullptr));                   // ... or their other arm, the APOBEC model's (:717-719)
      if (site_rate_moves_on) EMAT_TRY(site_rate_moves(nullptr));   // where the reference runs its global moves (run.cpp:635-641)
      const int64_t k = std::min(per_cycle, steps - done);
      EMAT_TRY(run_moves(k));
      if (paranoid) EMAT_TRY(bk(emat_check_derived(backend, 1.0, nullptr, nullptr)));
      laps.lap(); laps.mark("cycle: 2 run_moves (launch)");
      EMAT_TRY(reassemble());
      laps.lap(); laps.mark("cycle: 3 reassemble (waits for the moves)");
      done += k;
      if (laps.report) fprintf(stderr, "[emat_run] cycle: repartition %.1f ms | launch of the moves %.1f ms | reassemble (waits for the moves) %.1f ms\n", laps.ms(0), laps.ms(1), laps.ms(2));
    }
    if (!device_tree) normalize_root_of_host_tree();   // (a device-resident tree is normalised by every reassemble)
    return EMAT_OK;
  }
};

}  // namespace emat

using namespace emat;

struct emat_synth { SynthResult res; };
struct emat_run { RunDriver d; };

extern "C" {

emat_status emat_synth_create(const emat_synth_params* p, emat_synth** out) {
  if (!p || !out || p->num_tips < 2 || p->num_sites < 1) return EMAT_ERR_INVALID_ARGUMENT;
  SynthParams sp;
  sp.num_tips = p->num_tips; sp.num_sites = p->num_sites; sp.tip_span = p->tip_span; sp.tip_date_uncertainty = p->tip_date_uncertainty;
  sp.frac_uncertain_tips = p->frac_uncertain_tips; sp.pop_n0 = p->pop_n0; sp.pop_growth = p->pop_growth; sp.mu = p->mu; sp.kappa = p->kappa;
  for (int a = 0; a < 4; ++a) sp.pi[a] = p->pi[a];
  sp.gaps_per_tip = p->gaps_per_tip; sp.mean_gap_len = p->mean_gap_len; sp.seed = p->seed;
  auto* s = new emat_synth;
  try { s->res = make_synthetic_emat(sp); } catch (...) { delete s; return EMAT_ERR_INTERNAL; }
  *out = s;
  return EMAT_OK;
}
void emat_synth_destroy(emat_synth* s) { delete s; }
emat_status emat_synth_get(emat_synth* s, emat_flat_tree* tree_view, const uint8_t** ref, double* t_max_tip) {
  if (!s) return EMAT_ERR_INVALID_ARGUMENT;
  if (tree_view) *tree_view = s->res.tree.view();
  if (ref) *ref = s->res.ref_sequence.data();
  if (t_max_tip) *t_max_tip = s->res.t_max_tip;
  return EMAT_OK;
}

emat_status emat_run_create(emat_backend* backend, const emat_flat_tree* tree, const uint8_t* ref, int32_t L, uint64_t seed, emat_run** out) {
  if (!tree || !ref || !out || L <= 0) return EMAT_ERR_INVALID_ARGUMENT;
  if (!validate_flat_tree(*tree, L).empty()) return EMAT_ERR_INVALID_ARGUMENT;
  auto* r = new emat_run;
  r->d.backend = backend; r->d.tree = HTree::from_view(*tree); r->d.ref.assign(ref, ref + L); r->d.L = L; r->d.seed = seed; r->d.draw.bitgen = SplitMix64(seed ^ 0xD1B54A32D192ED03ull);
  *out = r;
  return EMAT_OK;
}
emat_status emat_run_destroy(emat_run* r) { delete r; return EMAT_OK; }
const char* emat_run_last_error(const emat_run* r) { return r ? r->d.last_error.c_str() : "null run"; }

emat_status emat_run_set_max_part_nodes(emat_run* r, int32_t n) { if (!r || n < -1) return EMAT_ERR_INVALID_ARGUMENT; r->d.max_part_nodes = n; return EMAT_OK; }
/* Test hook: the cut nodes the LAST repartition's draw (same stencil, same random stream of the refinement) gives on the tree AS IT IS NOW.
 * Between a repartition and the reassemble that follows a pass, the moves only re-hang and re-time nodes within parts; refine_stencil
 * (emat_run_partition.hpp) reads nothing such a pass can change, so the draw on the tree after the pass must be the draw on the tree before it -- the premise of
 * the argument that the part-size limit leaves the sampler's stationary distribution alone (refine_stencil).  Changes no state. */
emat_status emat_run_debug_redraw_partition(emat_run* r, int32_t* cut_nodes, int32_t* num_cut_nodes) {
  if (!r || !num_cut_nodes) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  if (d.follow) return d.fail(EMAT_ERR_STATE, "this run takes its draws from another one (emat_run_follow_draws): ask that one");
  if (d.draw.last_pick < 0 || d.draw.last_pick >= (int)d.draw.stencils.size()) return d.fail(EMAT_ERR_STATE, "emat_run_repartition first");
  if (d.device_tree) EMAT_TRY(d.fetch_device_topology()); else sync_topology(d.tp, d.tree);
  std::vector<int32_t> cuts;
  try { cuts = refine_stencil(d.tp, d.draw.stencils[(size_t)d.draw.last_pick], d.seed, d.draw.last_refine_epoch, d.effective_limit()).cuts; } catch (const std::exception& ex) { return d.fail(EMAT_ERR_INTERNAL, ex.what()); }
  std::sort(cuts.begin(), cuts.end());
  const int32_t cap = *num_cut_nodes; *num_cut_nodes = (int32_t)cuts.size();
  if (cap < (int32_t)cuts.size() || !cut_nodes) return d.fail(EMAT_ERR_BUFFER_TOO_SMALL, "emat_run_debug_redraw_partition: array too small");
  std::copy(cuts.begin(), cuts.end(), cut_nodes);
  return EMAT_OK;
}
emat_status emat_run_partition_stats(emat_run* r, int32_t* num_parts, int32_t* largest_part_nodes, int32_t* extra_cuts, int32_t* max_part_nodes_in_effect) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (num_parts) *num_parts = r->d.last_num_parts;
  if (largest_part_nodes) *largest_part_nodes = r->d.last_largest_part;
  if (extra_cuts) *extra_cuts = r->d.draw.last_extra_cuts;
  if (max_part_nodes_in_effect) *max_part_nodes_in_effect = effective_max_part_nodes(r->d.max_part_nodes, r->d.num_parts, r->d.device_tree ? (size_t)r->d.tp.n : r->d.tree.nodes.size());
  return EMAT_OK;
}
emat_status emat_run_set_num_parts(emat_run* r, int32_t n) { if (!r || n < 1) return EMAT_ERR_INVALID_ARGUMENT; r->d.num_parts = n; r->d.draw.stencils.clear(); return EMAT_OK; }
emat_status emat_run_set_hky(emat_run* r, double mu, double kappa, const double pi[4], const double* nu_l) {
  if (!r || !pi || !(mu >= 0) || !(kappa > 0)) return EMAT_ERR_INVALID_ARGUMENT;
  r->d.hky_mu = mu; r->d.hky_kappa = kappa; for (int a = 0; a < 4; ++a) r->d.hky_pi[a] = pi[a];
  if (nu_l) r->d.nu_l.assign(nu_l, nu_l + r->d.L); else r->d.nu_l.clear();
  r->d.have_hky = true; r->d.model_changed();
  return EMAT_OK;
}
emat_status emat_run_set_pop_model(emat_run* r, const emat_pop_model* pm) {
  if (!r || !pm) return EMAT_ERR_INVALID_ARGUMENT;
  r->d.pop = *pm;
  if (pm->kind == EMAT_POP_SKYGRID) { r->d.sky_x.assign(pm->skygrid_x, pm->skygrid_x + pm->skygrid_num_knots); r->d.sky_g.assign(pm->skygrid_gamma, pm->skygrid_gamma + pm->skygrid_num_knots); }
  r->d.have_pop = true; r->d.pop_model_changed();
  return EMAT_OK;
}
emat_status emat_run_set_coalescent_t_step(emat_run* r, double t_step) { if (!r || !(t_step > 0)) return EMAT_ERR_INVALID_ARGUMENT; r->d.t_step = t_step; r->d.t_step_set = true; return EMAT_OK; }
emat_status emat_run_set_flags(emat_run* r, int32_t odin, int32_t topo) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; r->d.only_displacing_inner_nodes = odin; r->d.topology_moves_enabled = topo; r->d.model_changed(); return EMAT_OK; }

emat_status emat_run_set_device_tree(emat_run* r, int32_t on) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  if (on) {
    EMAT_TRY(d.need_backend(RunDriver::kDeviceTreeNeedsBackend));
    EMAT_TRY(d.need_parts_back());
    d.device_tree_switched(true);
    return EMAT_OK;
  }
  if (d.device_tree) {
    EMAT_TRY(d.need_parts_back());
    EMAT_TRY(d.ensure_host_tree());
    d.device_tree_switched(false);
  }
  return EMAT_OK;
}
emat_status emat_run_note_device_reassembled(emat_run* r, int32_t num_root_deltas, const int32_t* site, const uint8_t* to) {
  if (!r || num_root_deltas < 0 || (num_root_deltas > 0 && (!site || !to))) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  if (!d.device_tree || !d.parts_uploaded) return d.fail(EMAT_ERR_STATE, "no device-resident parts are out");
  for (int k = 0; k < num_root_deltas; ++k) { if (site[k] < 0 || site[k] >= d.L || to[k] > 3) return EMAT_ERR_INVALID_ARGUMENT; d.ref[site[k]] = to[k]; }
  d.device_parts_came_back();
  return EMAT_OK;
}
emat_status emat_run_repartition(emat_run* r) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.repartition(); }   // (sets tree_cut)
emat_status emat_run_num_parts(emat_run* r, int32_t* n, int32_t* root_part) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; if (n) *n = (int)r->d.parts.size(); if (root_part) *root_part = r->d.root_part; return EMAT_OK; }
emat_status emat_run_part_sizes(emat_run* r, int32_t p, int32_t* nn, int32_t* nm, int32_t* ni, int32_t* nf) {
  if (r && r->d.device_tree) return r->d.fail(EMAT_ERR_STATE, "with a device-resident tree the parts exist only on the device (emat_part_get_sizes / emat_part_download of the backend)");
  if (!r || p < 0 || p >= (int)r->d.subtrees.size()) return EMAT_ERR_INVALID_ARGUMENT;
  const FlatTree& t = r->d.subtrees[p];
  if (nn) *nn = t.num_nodes(); if (nm) *nm = t.num_muts(); if (ni) *ni = t.num_intervals(); if (nf) *nf = t.num_from_states();
  return EMAT_OK;
}
emat_status emat_run_part_get(emat_run* r, int32_t p, emat_flat_tree* out, int32_t* incl_root, uint64_t* seed) {
  if (!r || !out || p < 0 || p >= (int)r->d.subtrees.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (incl_root) *incl_root = p == r->d.root_part ? 1 : 0;
  if (seed) *seed = r->d.part_seeds[p];
  return r->d.subtrees[p].copy_out(out);
}
emat_status emat_run_part_put(emat_run* r, int32_t p, const emat_flat_tree* st) {
  if (!r || !st || p < 0 || p >= (int)r->d.subtrees.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (!validate_flat_tree(*st, r->d.L).empty() || st->num_nodes != (int)r->d.parts[p].orig.size()) return EMAT_ERR_INVALID_ARGUMENT;
  r->d.subtrees[p] = FlatTree::from_view(*st);
  return EMAT_OK;
}
emat_status emat_run_push_params(emat_run* r) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.backend) return EMAT_OK;
  EMAT_TRY(r->d.push_model());
  EMAT_TRY(r->d.need_parts_out());
  return r->d.build_coalescent();   // run.cpp:267-275 rebuilds the coalescent parts at every push
}
emat_status emat_run_moves(emat_run* r, int64_t count) {
  if (!r || count < 0) return EMAT_ERR_INVALID_ARGUMENT;
  EMAT_TRY(r->d.need_backend(RunDriver::kMovesNeedBackend));
  EMAT_TRY(r->d.need_parts_out());
  return r->d.run_moves(count);
}
emat_status emat_run_reassemble(emat_run* r) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.reassemble(); }

/* Drivers of one process that are bound to draw the same partitions (same seed, same tree: emat_multi's shards) draw once: `follower` takes
 * the cut nodes `leader` drew for the same cycle instead of drawing them again.  The leader draws at its own emat_run_repartition, or ahead of
 * it with emat_run_draw_partition (so that leader and followers can then cut side by side).  NULL leader = draw for itself again. */
emat_status emat_run_follow_draws(emat_run* follower, emat_run* leader) {
  if (!follower || follower == leader) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& f = follower->d;
  if (leader) {
    const RunDriver& l = leader->d;
    if (l.seed != f.seed || l.tree.nodes.size() != f.tree.nodes.size() || l.epoch != f.epoch || l.num_parts != f.num_parts || l.max_part_nodes != f.max_part_nodes)
      return f.fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_follow_draws: leader and follower must be runs of the same seed, tree, cycle and partition settings");
    if (l.follow) return f.fail(EMAT_ERR_INVALID_ARGUMENT, "emat_run_follow_draws: the leader itself follows another run");
  }
  f.follow = leader ? &leader->d.draw : nullptr;
  return EMAT_OK;
}
emat_status emat_run_draw_partition(emat_run* r) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  if (d.follow) return d.fail(EMAT_ERR_STATE, "emat_run_draw_partition: this run takes its draws from another one");
  if (d.draw.has(d.epoch)) return EMAT_OK;   // already drawn for the cycle to come
  try {
    if (d.device_tree && d.device_tree_uploaded) EMAT_TRY(d.fetch_device_topology());
    else { if (d.device_tree) d.normalize_root_of_host_tree(); sync_topology(d.tp, d.tree); }   // (before the first upload: the host's copy is the tree)
    d.draw_partition();
  } catch (const std::exception& ex) { return d.fail(EMAT_ERR_INTERNAL, ex.what()); }
  return EMAT_OK;
}
emat_status emat_run_set_shard(emat_run* r, int32_t rank, int32_t world) {
  if (!r || world < 1 || rank < 0 || rank >= world) return EMAT_ERR_INVALID_ARGUMENT;
  r->d.shard_rank = rank; r->d.shard_world = world; r->d.shard_changed();
  return EMAT_OK;
}
emat_status emat_run_shard_range(emat_run* r, int32_t* part_lo, int32_t* part_hi, int32_t* local_root_part) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (part_lo) *part_lo = r->d.part_lo;
  if (part_hi) *part_hi = r->d.part_hi;
  if (local_root_part) *local_root_part = r->d.local_root_part();
  return EMAT_OK;
}
emat_status emat_run_coalescent_begin(emat_run* r, double* local_t_min, double* local_t_max) {
  if (!r || !local_t_min || !local_t_max) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  EMAT_TRY(d.need_backend());
  EMAT_TRY(d.need_parts_out());
  EMAT_TRY(d.need_pop_model());
  const emat_pop_model pm = d.pop_view();
  EMAT_TRY(d.bk(emat_coalescent_begin(d.backend, &pm, d.local_root_part(), d.coalescent_step(), local_t_min, local_t_max)));
  d.coalescent_built();
  return EMAT_OK;
}
emat_status emat_run_moves_sharded(emat_run* r, int64_t count) {   // Run::run_local_moves (run.cpp:682-693) over ALL parts of the run
  if (!r || count < 0) return EMAT_ERR_INVALID_ARGUMENT;
  RunDriver& d = r->d;
  EMAT_TRY(d.need_backend(RunDriver::kMovesNeedBackend));
  EMAT_TRY(d.need_parts_out());
  const int64_t P = (int64_t)d.parts.size(), sub = count / P, rem = count - P * sub;
  // the remainder is spread one move per part over the first parts of the run (see emat_run_moves_even)
  return d.bk(emat_run_moves_even(d.backend, sub, (int32_t)std::max<int64_t>(0, std::min<int64_t>(rem - d.part_lo, d.part_hi - d.part_lo))));
}
// For calc_Ttwiddle_l: the whole-tree branch length hanging below every boundary tip of the LOCAL parts, from the lengths
// inside every part of the run and the tree of parts (a part's boundary tips are the cut nodes of the parts below it).
}  // extern "C"
emat_status emat::RunDriver::Ttwiddle_ext(const double* tree_length_of_part, int32_t* ext_offset, int32_t* ext_node, double* ext_length, int32_t capacity, int32_t* count) {
  RunDriver& d = *this;
  EMAT_TRY(d.ensure_partition_on_host());
  const int P = (int)d.parts.size();
  if (P == 0 || (int)d.part_kids.size() != P) return d.fail(EMAT_ERR_STATE, "repartition first");
  std::vector<int32_t> part_of_cut(d.tree.nodes.size(), -1);
  for (int p = 0; p < P; ++p) part_of_cut[d.parts[p].cut_point] = p;
  // children of each part in the tree of parts: (subtree node, part below).  A part's tips stay tips whatever the moves
  // do, so the partition's own record of them (which also exists when the parts themselves live only on the device) serves.
  std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(P);
  for (int p = 0; p < P; ++p) {
    const auto& pk = d.part_kids[p];
    for (int s = 1; s < (int)pk.size(); ++s) if (pk[s].first == EMAT_NO_NODE) { const int q = part_of_cut[d.parts[p].orig[s]]; if (q >= 0 && q != p) kids[p].push_back({s, q}); }
  }
  // total length below each part's cut node: its own branches plus everything below its boundary tips (children first)
  std::vector<double> below(P, -1.0);
  std::vector<std::pair<int, size_t>> stack; stack.push_back({d.root_part, 0});
  while (!stack.empty()) {
    auto& [p, k] = stack.back();
    if (k < kids[p].size()) { const int q = kids[p][k].second; ++k; stack.push_back({q, 0}); }
    else { double t = tree_length_of_part[p]; for (auto& kv : kids[p]) t += below[kv.second]; below[p] = t; stack.pop_back(); }
  }
  int32_t n = 0;
  for (int p = d.part_lo; p < d.part_hi; ++p) {
    ext_offset[p - d.part_lo] = n;
    for (auto& kv : kids[p]) { if (n < capacity) { ext_node[n] = kv.first; ext_length[n] = below[kv.second]; } ++n; }
  }
  ext_offset[d.part_hi - d.part_lo] = n;
  *count = n;
  return n <= capacity ? EMAT_OK : d.fail(EMAT_ERR_BUFFER_TOO_SMALL, "emat_run_Ttwiddle_ext: arrays too small");
}
// calc_Ttwiddle_l of the whole tree from the parts on the device (single process).
emat_status emat::RunDriver::get_Ttwiddle_l(double* Ttwiddle_l) {
  RunDriver& d = *this;
  EMAT_TRY(d.need_backend());
  EMAT_TRY(d.need_parts_out());
  if (d.shard_world > 1) return d.fail(EMAT_ERR_STATE, RunDriver::kShardedStatistics);
  const int P = (int)d.parts.size();
  std::vector<double> len(P);
  EMAT_TRY(d.bk(emat_get_part_tree_lengths(d.backend, len.data())));
  std::vector<int32_t> off(P + 1), node(P); std::vector<double> val(P); int32_t cnt = 0;
  EMAT_TRY(Ttwiddle_ext(len.data(), off.data(), node.data(), val.data(), P, &cnt));
  std::vector<double> S(d.L), R(d.L); double T = 0.0;
  EMAT_TRY(d.bk(emat_Ttwiddle_l_partial(d.backend, off.data(), node.data(), val.data(), S.data(), R.data(), &T)));
  return d.bk(emat_Ttwiddle_l_finish(d.backend, S.data(), R.data(), T, Ttwiddle_l));
}
// A group's setter whose spec is all it keeps: checked (check_moves_spec), then the switch and the spec.
template <class Spec, class Fault> emat_status set_moves_spec(emat_run* r, const std::string& w, int32_t on, const Spec* spec, Fault fault, bool emat::RunDriver::*is_on, Spec emat::RunDriver::*kept) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  EMAT_TRY(r->d.check_moves_spec(w, spec, fault));
  r->d.*is_on = on != 0; r->d.*kept = *spec;
  return EMAT_OK;
}
extern "C" {
emat_status emat_run_Ttwiddle_ext(emat_run* r, const double* tree_length_of_part, int32_t* ext_offset, int32_t* ext_node, double* ext_length, int32_t capacity, int32_t* count) {
  if (!r || !tree_length_of_part || !ext_offset || !count || capacity < 0 || (capacity > 0 && (!ext_node || !ext_length))) return EMAT_ERR_INVALID_ARGUMENT;
  return r->d.Ttwiddle_ext(tree_length_of_part, ext_offset, ext_node, ext_length, capacity, count);
}
emat_status emat_run_get_Ttwiddle_l(emat_run* r, double* Ttwiddle_l) { if (!r || !Ttwiddle_l) return EMAT_ERR_INVALID_ARGUMENT; return r->d.get_Ttwiddle_l(Ttwiddle_l); }
emat_status emat_run_set_site_rate_moves(emat_run* r, int32_t on, double alpha) {
  if (!r || !std::isfinite(alpha) || !(alpha > 0.0)) return EMAT_ERR_INVALID_ARGUMENT;
  r->d.site_rate_moves_on = on != 0; r->d.site_rate_alpha = alpha;
  return EMAT_OK;
}
emat_status emat_run_site_rate_moves(emat_run* r, emat_site_rate_result* out) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.site_rate_moves(out); }
emat_status emat_run_set_skygrid_moves(emat_run* r, int32_t on, const emat_skygrid_spec* spec) {
  return set_moves_spec(r, "emat_run_set_skygrid_moves: ", on, spec, [](const emat_skygrid_spec& s) { return skygrid_spec_fault(s); }, &RunDriver::skygrid_moves_on, &RunDriver::sky_spec);
}
emat_status emat_run_skygrid_moves(emat_run* r, emat_skygrid_result* out) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.skygrid_moves(out); }
emat_status emat_run_get_skygrid(emat_run* r, double* gamma, double* tau) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.have_pop || r->d.pop.kind != EMAT_POP_SKYGRID) return r->d.fail(EMAT_ERR_STATE, "emat_run_get_skygrid: the run has no Skygrid population model");
  if (gamma) std::copy(r->d.sky_g.begin(), r->d.sky_g.end(), gamma);
  if (tau) *tau = r->d.sky_spec.tau;
  return EMAT_OK;
}
emat_status emat_run_set_exp_pop_moves(emat_run* r, int32_t on, const emat_exp_pop_spec* spec) {
  return set_moves_spec(r, "emat_run_set_exp_pop_moves: ", on, spec, [](const emat_exp_pop_spec& s) { return exp_pop_spec_fault(s); }, &RunDriver::exp_pop_moves_on, &RunDriver::xp_spec);
}
emat_status emat_run_exp_pop_moves(emat_run* r, emat_exp_pop_result* out) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.exp_pop_moves(out); }
emat_status emat_run_get_exp_pop(emat_run* r, double* n0, double* g) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.have_pop || r->d.pop.kind != EMAT_POP_EXP) return r->d.fail(EMAT_ERR_STATE, "emat_run_get_exp_pop: the run has no exponential population model");
  if (n0) *n0 = r->d.pop.p[1];
  if (g) *g = r->d.pop.p[2];
  return EMAT_OK;
}
emat_status emat_run_set_subst_moves(emat_run* r, int32_t on, const emat_subst_spec* spec) {   // (mu, kappa and pi of the spec are ignored: the run's own are used)
  if (r && on) EMAT_TRY(r->d.mpox_bars_subst_moves());
  return set_moves_spec(r, "emat_run_set_subst_moves: ", on, spec, [](const emat_subst_spec& s) { const char* why = rounds_limit_fault(s.rounds); return why ? why : subst_spec_fault(s, false); }, &RunDriver::subst_moves_on, &RunDriver::sb_spec);
}
emat_status emat_run_subst_moves(emat_run* r, emat_subst_result* out) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.subst_moves(out); }
emat_status emat_run_get_hky(emat_run* r, double* mu, double* kappa, double* pi) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.have_hky) return r->d.fail(EMAT_ERR_STATE, "emat_run_get_hky: emat_run_set_hky must be called first");
  if (mu) *mu = r->d.hky_mu;
  if (kappa) *kappa = r->d.hky_kappa;
  if (pi) std::copy(r->d.hky_pi, r->d.hky_pi + 4, pi);
  return EMAT_OK;
}
emat_status emat_run_set_mpox(emat_run* r, int32_t on, const emat_mpox_spec* spec) {   // (mu of the spec is ignored: the run's own is used)
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  try { return r->d.set_mpox(on, spec); } catch (const std::exception& ex) { return r->d.fail(EMAT_ERR_INTERNAL, ex.what()); }
}
emat_status emat_run_mpox_moves(emat_run* r, emat_mpox_result* out) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; return r->d.mpox_moves(out); }
emat_status emat_run_get_mpox(emat_run* r, double* mu, double* mu_star) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.mpox_on) return r->d.fail(EMAT_ERR_STATE, "emat_run_get_mpox: the APOBEC model is off");
  if (mu) *mu = r->d.mpox_mu;
  if (mu_star) *mu_star = r->d.mpox_mu_star;
  return EMAT_OK;
}
emat_status emat_run_get_mpox_partition(emat_run* r, int32_t* partition_for_site, int32_t* count) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (!r->d.mpox_on) return r->d.fail(EMAT_ERR_STATE, "emat_run_get_mpox_partition: the APOBEC model is off");
  if (partition_for_site) std::copy(r->d.mpox_partition_for_site.begin(), r->d.mpox_partition_for_site.end(), partition_for_site);
  if (count) *count = r->d.mpox_context_sites;
  return EMAT_OK;
}
emat_status emat_run_get_site_rates(emat_run* r, double* alpha, double* nu_l) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  if (alpha) *alpha = r->d.site_rate_alpha;
  if (nu_l) { if (r->d.nu_l.empty()) std::fill(nu_l, nu_l + r->d.L, 1.0); else std::copy(r->d.nu_l.begin(), r->d.nu_l.end(), nu_l); }
  return EMAT_OK;
}

emat_status emat_run_pack_local_parts(emat_run* r, uint8_t* buf, uint64_t capacity, uint64_t* bytes_needed) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  try { return r->d.pack_local_parts(buf, capacity, bytes_needed); } catch (const std::exception& ex) { return r->d.fail(EMAT_ERR_INTERNAL, ex.what()); }
}
emat_status emat_run_unpack_parts(emat_run* r, const uint8_t* buf, uint64_t bytes) {
  if (!r || (!buf && bytes)) return EMAT_ERR_INVALID_ARGUMENT;
  try { return r->d.unpack_parts(buf, bytes); } catch (const std::exception& ex) { return r->d.fail(EMAT_ERR_INTERNAL, ex.what()); }
}
emat_status emat_run_set_reference_remainder(emat_run* r, int32_t on) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; r->d.reference_remainder = on != 0; return EMAT_OK; }
emat_status emat_run_set_paranoid(emat_run* r, int32_t on) { if (!r) return EMAT_ERR_INVALID_ARGUMENT; r->d.paranoid = on != 0; return EMAT_OK; }
emat_status emat_run_do_mcmc_steps(emat_run* r, int64_t steps, int64_t per_cycle) {   // run.cpp:622-657 minus global moves
  if (!r || steps < 0) return EMAT_ERR_INVALID_ARGUMENT;
  return r->d.do_mcmc_steps(steps, per_cycle);
}
emat_status emat_run_tree_sizes(emat_run* r, int32_t* nn, int32_t* nm, int32_t* ni, int32_t* nf) {
  if (!r) return EMAT_ERR_INVALID_ARGUMENT;
  EMAT_TRY(r->d.ensure_host_tree());
  int m = 0, i = 0, f = 0; for (auto& nd : r->d.tree.nodes) { m += (int)nd.muts.size(); i += (int)nd.miss.size(); f += (int)nd.mfs.size(); }
  if (nn) *nn = (int)r->d.tree.nodes.size(); if (nm) *nm = m; if (ni) *ni = i; if (nf) *nf = f;
  return EMAT_OK;
}
emat_status emat_run_tree_get(emat_run* r, emat_flat_tree* out, uint8_t* ref) {
  if (!r || !out) return EMAT_ERR_INVALID_ARGUMENT;
  EMAT_TRY(r->d.ensure_host_tree());
  if (ref) std::copy(r->d.ref.begin(), r->d.ref.end(), ref);
  return r->d.tree.to_flat().copy_out(out);
}
emat_status emat_run_t_max_tip(emat_run* r, double* t) { if (!r || !t) return EMAT_ERR_INVALID_ARGUMENT; *t = r->d.tree.t_max_tip(); return EMAT_OK; }

}  // extern "C"
