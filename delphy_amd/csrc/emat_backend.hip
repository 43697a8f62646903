// emat_backend.hip -- the translation unit of the MI355X-native EMAT local-move engine: the kernel headers, the host layer
// (emat_state_host.hpp, emat_slab_host.hpp, emat_pass_host.hpp) and, in this file itself, the product entry points of the C-ABI.
//
// Boundary: include/emat_backend.h (each entry point cites the reference call it replaces).
// Execution model: one 64-lane wavefront (= one workgroup) per partition part.  A part's working set
// is one slab (emat_slab.hpp); `k_run_moves` streams it into LDS when it fits, runs the requested
// number of `Subrun::mcmc_sub_iteration` steps (reference core/subrun.cpp:98-121) there, and streams it
// back.  `k_recalc_derived` is the whole-part recomputation of reference core/subrun.cpp:17-26.
// There is no CPU fallback: without a HIP device every entry point fails with EMAT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>
#include <map>
#include <stdexcept>

#include "../../include/emat_backend.h"
#include "emat_move_specs.hpp"      // what the global moves' specs must satisfy (shared with the run driver)
#include "emat_part_kernels.hpp"    // the per-part kernels, and the move headers they are compiled from
#include "emat_host_model.hpp"
#include "flat_tree.hpp"
#include "host_parallel.hpp"
#include "emat_gtree_kernels.hpp"   // the whole tree in HBM: cutting it into part slabs and gathering the parts back
#include "emat_build.hpp"           // initial-tree construction: the graft loop as a kernel, the finishing passes on the host
#include "emat_probe_kernels.hpp"   // the tree probers, one family for the resident tree and the kept samples: lineage and site-state prevalence over time
#include "emat_mcc_kernels.hpp"     // sampled trees kept in HBM, and the maximum-clade-credibility tree derived from them
#include "emat_mcc_summary_kernels.hpp"   // on the MCC tree: the spread of every node's date over the samples, and the support of the master's mutations
#include "emat_site_rate_kernels.hpp"   // the site-rate moves: steps on alpha and the Gibbs draw of every nu_l
#include "emat_skygrid_kernels.hpp"     // the Skygrid population moves: tau, the zero mode and the HMC on the gammas
#include "emat_exp_pop_kernels.hpp"     // the Exponential population moves: n0 and the growth rate
#include "emat_subst_kernels.hpp"       // the substitution-model moves: mu, the HKY frequencies and kappa
#include "emat_mpox_kernels.hpp"        // the APOBEC (mpox) model's moves: Gibbs rounds of mu and rho = mu* / mu
#include "emat_align_kernels.hpp"       // aligned sequences in: packed rows, site counts, the consensus, every tip's deltas and missing runs
#include "emat_state_host.hpp"      // buffers, host records, emat_backend and the transitions of its part state
#include "emat_slab_host.hpp"       // slab codec, geometry, size classes
#include "emat_pass_host.hpp"       // materialize, launch_moves, finish_pass, the two pulls

// =================================================================================================
// C-ABI
// =================================================================================================
namespace { emat_status gt_finish_gather(emat_backend* h); }   // (emat_gtree_host.hpp, included at the end of this file)
extern "C" {

emat_status emat_backend_create(const emat_config* cfg, emat_backend** out) {
  if (!cfg || !out || cfg->num_sites <= 0) return EMAT_ERR_INVALID_ARGUMENT;
  if (cfg->device == -1) {   // host-only handle: can stage data and build coalescent parts, can never run a move
    auto h = std::make_unique<emat_backend>();
    h->cfg = *cfg; h->L = cfg->num_sites; h->host_only = true;
    *out = h.release();
    return EMAT_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return EMAT_ERR_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= ndev) return EMAT_ERR_INVALID_ARGUMENT;
  if (hipSetDevice(cfg->device) != hipSuccess) return EMAT_ERR_HIP;
  auto h = std::make_unique<emat_backend>();
  h->cfg = *cfg; h->L = cfg->num_sites;
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return EMAT_ERR_HIP; h->num_cus = prop.multiProcessorCount; }
  if (hipStreamCreate(&h->stream) != hipSuccess) return EMAT_ERR_HIP;
  h->xcc_count = probe_xcc_dealing(cfg->device, h->stream);
  for (hipEvent_t* e : {&h->ev_start, &h->ev_stop}) if (hipEventCreate(e) != hipSuccess) return EMAT_ERR_HIP;
  if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) return EMAT_ERR_HIP;
  for (int c = 1; c < emat_backend::k_max_classes; ++c) {
    if (!(h->class_stream[c] = side_stream(cfg->device, c - 1))) return EMAT_ERR_HIP;
    if (hipEventCreateWithFlags(&h->ev_join[c], hipEventDisableTiming) != hipSuccess) return EMAT_ERR_HIP;
  }
  *out = h.release();
  return EMAT_OK;
}
emat_status emat_backend_destroy(emat_backend* h) {
  if (!h) return EMAT_OK;
  if (h->host_only) { delete h; return EMAT_OK; }
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  for (int c = 1; c < emat_backend::k_max_classes; ++c) {
    if (h->class_stream[c]) (void)hipStreamSynchronize(h->class_stream[c]);   // shared with the other handles of the device: never destroyed
    if (h->ev_join[c]) (void)hipEventDestroy(h->ev_join[c]);
  }
  for (hipEvent_t e : {h->ev_start, h->ev_stop, h->ev_fork}) if (e) (void)hipEventDestroy(e);
  HostSpans::instance().report();
  delete h;
  return EMAT_OK;
}
/* Tuning and test options of one handle (header: emat_set_option).  Until round 4 these were environment variables read at
 * emat_backend_create; a process that embeds the library sets them per handle instead, and nothing in its environment reaches them. */
emat_status emat_set_option(emat_backend* h, const char* key, const char* value) {
  if (!h || !key || !value) return EMAT_ERR_INVALID_ARGUMENT;
  if (strcmp(key, "debug_fail_gather") == 0) { h->cfg_debug_fail_gather = atoi(value) != 0; return EMAT_OK; }   // (a test hook that is armed in the middle of a run)
  if (strcmp(key, "mcc_table_log2") == 0) { h->cfg_mcc_table_log2 = std::max(0, std::min(32, atoi(value))); return EMAT_OK; }   // (read by every emat_mcc_derive)
  if (strcmp(key, "samples_probe_chunk") == 0) { h->cfg_samples_probe_chunk = std::max(0, atoi(value)); return EMAT_OK; }   // (read by every emat_tree_samples_probe_ancestors / emat_mcc_probe_ancestors)
  if (strcmp(key, "mcc_summary_chunk") == 0) { h->cfg_mcc_summary_chunk = std::max(0, atoi(value)); return EMAT_OK; }   // (read by every emat_mcc_node_times)
  if (h->slabs_on_device) return fail(h, EMAT_ERR_STATE, "emat_set_option: options are set before the first launch");
  const std::string k(key);
  const char* e = value;
  if (k == "slack") h->cfg.slab_slack = atof(e);
  else if (k == "heap_per_node") h->cfg_heap_per_node = atof(e);
  else if (k == "lds_scratch") h->cfg_lds_scratch = (uint32_t)atoi(e) & ~15u;
  else if (k == "lds_classes") {   // e.g. "60,90,99,100"
    h->cfg_class_pct.clear();
    for (const char* q = e; *q;) { h->cfg_class_pct.push_back(std::max(1, std::min(100, atoi(q)))); while (*q && *q != ',') ++q; if (*q == ',') ++q; }
  }
  else if (k == "lds_max") h->cfg_lds_max = (uint32_t)atoi(e) & ~511u;
  else if (k == "giants") h->cfg_giants = atoi(e) != 0;
  else if (k == "side_arena") h->cfg_side_arena = (uint32_t)atoi(e);
  else if (k == "tree_host_coalescent") h->cfg_gt_host_coal = atoi(e) != 0;
  else if (k == "ticket_taper") h->cfg_taper = atoi(e) != 0;
  else if (k == "chunks") { h->cfg_chunks = std::max(1, std::min(64, atoi(e))); h->cfg_chunks_forced = true; }
  else if (k == "ticket_xcd_spread") h->cfg_ticket_spread = atoi(e) != 0;
  else if (k == "ticket_release") h->cfg_ticket_full_release = strcmp(e, "full") == 0;
  else if (k == "ticket_weights") h->cfg_ticket_weights = e;
  else if (k == "single_ticket_parts") h->cfg_single_ticket_parts = std::max(0, atoi(e));
  else if (k == "parts_per_cu") h->cfg_parts_per_cu = std::max(0, std::min(4 * EMAT_WAVES_PER_EU, atoi(e)));
  else if (k == "order_by_time") h->cfg_order_by_time = atoi(e) != 0;
  else if (k == "build_blocks") h->cfg_build_blocks = std::max(0, atoi(e));
  else if (k == "tree_tight") h->cfg_tree_tight = atoi(e) != 0;
  else if (k == "no_uniform_sites") { h->cfg_no_uniform_sites = atoi(e) != 0; if (h->have_evo && h->have_ref) refresh_ref_derived(h); }
  else if (k == "fn_min_lists") h->cfg_fn_min_lists = (unsigned)std::max(0, atoi(e));
  else if (k == "phase_extra") h->cfg_phase_extra = atoi(e) != 0;
  else return fail(h, EMAT_ERR_INVALID_ARGUMENT, "emat_set_option: unknown option '" + k + "'");
  return EMAT_OK;
}
/* Size of the host thread pool of this library (per process; takes effect if called before the first parallel loop; 0 = default). */
emat_status emat_set_host_threads(int32_t n) { if (n < 0) return EMAT_ERR_INVALID_ARGUMENT; host_threads_override() = n; return EMAT_OK; }
const char* emat_last_error(const emat_backend* h) { return h ? h->last_error.c_str() : "null backend"; }
#ifndef EMAT_BUILD_ID
#define EMAT_BUILD_ID "unstamped"
#endif
const char* emat_build_id(void) { return EMAT_BUILD_ID; }

emat_status emat_set_ref_sequence(emat_backend* h, const uint8_t* ref, int32_t num_sites) {
  if (!h || !ref || num_sites != h->L) return EMAT_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < num_sites; ++l) if (ref[l] > 3) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "reference sequence states must be 0..3");
  h->ref.assign(ref, ref + num_sites); h->have_ref = true;
  if (h->have_evo) refresh_ref_derived(h);
  h->model_changed();
  return EMAT_OK;
}
emat_status emat_set_evo(emat_backend* h, int32_t P, const double* mu, const double* pi, const double* q, const double* nu_l, const int32_t* pfs) {
  if (!h || P <= 0 || P > 255 || !mu || !pi || !q || !nu_l || !pfs) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_ref) return fail(h, EMAT_ERR_STATE, "emat_set_ref_sequence must precede emat_set_evo");
  h->partition_for_site.resize(h->L);
  for (int l = 0; l < h->L; ++l) { if (pfs[l] < 0 || pfs[l] >= P) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "partition_for_site out of range"); h->partition_for_site[l] = (uint8_t)pfs[l]; }
  h->num_partitions = P;
  h->mu.assign(mu, mu + P); h->pi.assign(pi, pi + 4 * P); h->q.assign(q, q + 16 * P); h->nu_l.assign(nu_l, nu_l + h->L);
  h->have_evo = true;
  install_model(h);
  return EMAT_OK;
}
/* the model the handle holds (header: emat_get_evo) */
emat_status emat_get_evo(emat_backend* h, int32_t* num_partitions, double* mu, double* pi, double* q) {
  if (!h || !num_partitions) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_evo) return fail(h, EMAT_ERR_STATE, "emat_set_evo must precede emat_get_evo");
  const int P = h->num_partitions, room = *num_partitions;
  *num_partitions = P;
  if (room < P && (mu || pi || q)) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_get_evo: room for fewer site partitions than the model has");
  if (mu) std::copy(h->mu.begin(), h->mu.end(), mu);
  if (pi) std::copy(h->pi.begin(), h->pi.end(), pi);
  if (q) std::copy(h->q.begin(), h->q.end(), q);
  return EMAT_OK;
}
emat_status emat_set_flags(emat_backend* h, double t_max_tip, int32_t only_displacing_inner_nodes, int32_t topology_moves_enabled) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  h->flags.t_max_tip = t_max_tip; h->flags.only_displacing_inner_nodes = only_displacing_inner_nodes; h->flags.topology_moves_enabled = topology_moves_enabled;
  return EMAT_OK;
}

emat_status emat_begin_upload(emat_backend* h, int32_t num_parts) {
  if (!h || num_parts <= 0) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->cfg.max_parts > 0 && num_parts > h->cfg.max_parts) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "more parts than cfg.max_parts");
  if (h->stream) { (void)join_side_classes(h); (void)hipStreamSynchronize(h->stream); }   // (a pass still in flight is discarded with the parts, but not written over)
  h->coal_builder.reset();
  h->fatal_status = EMAT_OK; h->fatal_message.clear(); h->pass_pending = false;
  h->parts.clear(); h->parts.resize(num_parts);
  h->expected_moves.assign((size_t)num_parts, 0);
  h->uploads_expected = num_parts; h->root_part = -1; h->gt.parts_came_back();   // (host parts replace whatever the resident tree had out)
  h->parts_replaced();
  return EMAT_OK;
}
emat_status emat_part_upload(emat_backend* h, int32_t part_id, const emat_flat_tree* subtree, int32_t includes_run_root, uint64_t seed) {
  if (!h || !subtree || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->uploads_expected <= 0) return fail(h, EMAT_ERR_STATE, "emat_begin_upload must precede emat_part_upload");
  std::string msg = validate_flat_tree(*subtree, h->L);
  if (!msg.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "part " + std::to_string(part_id) + ": " + msg);
  msg = flat_tree_list_limit(*subtree, (int32_t)k_max_list_upload);
  if (!msg.empty()) return fail(h, EMAT_ERR_CAPACITY, "part " + std::to_string(part_id) + ": " + msg);
  PartHost& ph = h->parts[part_id];
  if (ph.uploaded) return fail(h, EMAT_ERR_STATE, "part uploaded twice");
  ph.tree = FlatTree::from_view(*subtree); ph.n_nodes = subtree->num_nodes;
  ph.includes_run_root = includes_run_root != 0;
  ph.rng.key = seed; ph.rng.counter = 0; ph.rng.spare = 0; ph.rng.has_spare = false;
  ph.uploaded = true; ph.stats = emat_part_stats{}; ph.space_boost = 1.0; ph.cell_boost = 1; ph.trace.clear();
  if (ph.includes_run_root) h->root_part = part_id;
  return EMAT_OK;
}
emat_status emat_end_upload(emat_backend* h) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  for (auto& ph : h->parts) if (!ph.uploaded) return fail(h, EMAT_ERR_STATE, "emat_end_upload before every part was uploaded");
  h->uploads_expected = 0;
  return EMAT_OK;
}

emat_status emat_build_coalescent_parts(emat_backend* h, const emat_pop_model* pm, int32_t root_part_index, double t_step) {
  if (!h || !pm || !(t_step > 0.0)) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty() || h->uploads_expected != 0) return fail(h, EMAT_ERR_STATE, "upload parts first");
  if (root_part_index < 0 || root_part_index >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  try {
    emat_status st = pull_from_device(h); if (st) return st;   // the trees (node times) may have moved on the device
    h->pop = HostPopModel::from_c(*pm);
    std::vector<const FlatTree*> trees; std::vector<HostRng*> rngs;
    for (auto& ph : h->parts) { trees.push_back(&ph.tree); rngs.push_back(&ph.rng); }
    auto cps = make_coalescent_parts(trees, root_part_index, h->pop, rngs, t_step);
    for (size_t p = 0; p < h->parts.size(); ++p) h->parts[p].coal = std::move(cps[p]);
  } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  h->have_pop = true; h->have_coal = true; h->model_dirty = true;
  h->parts_need_encoding(false);   // with the new cell tables
  return EMAT_OK;
}

// ---- staged form of emat_build_coalescent_parts for runs sharded over several GPUs ---------------
emat_status emat_coalescent_begin(emat_backend* h, const emat_pop_model* pm, int32_t root_part_index, double t_step, double* local_t_min, double* local_t_max) {
  if (!h || !pm || !(t_step > 0.0) || !local_t_min || !local_t_max) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty() || h->uploads_expected != 0) return fail(h, EMAT_ERR_STATE, "upload parts first");
  if (root_part_index < -1 || root_part_index >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  try {
    emat_status st = pull_from_device(h); if (st) return st;
    h->pop = HostPopModel::from_c(*pm);
    h->coal_builder = std::make_unique<CoalBuilder>();
    h->coal_builder->pop = h->pop; h->coal_builder->t_step = t_step;
    for (size_t p = 0; p < h->parts.size(); ++p) h->coal_builder->add_part(&h->parts[p].tree, &h->parts[p].rng, (int)p == root_part_index);
    h->coal_builder->local_range(*local_t_min, *local_t_max);
  } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  return EMAT_OK;
}
emat_status emat_coalescent_set_range(emat_backend* h, double all_t_min, double all_t_max, int32_t* num_cells) {
  if (!h || !num_cells) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->coal_builder) return fail(h, EMAT_ERR_STATE, "emat_coalescent_begin first");
  *num_cells = h->coal_builder->set_range(all_t_min, all_t_max);
  return EMAT_OK;
}
emat_status emat_coalescent_local_grid(emat_backend* h, double* k_bar, int32_t* num_active) {
  if (!h || !k_bar || !num_active) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->coal_builder) return fail(h, EMAT_ERR_STATE, "emat_coalescent_begin first");
  try {
    std::vector<double> kb; std::vector<int32_t> na;
    h->coal_builder->local_grid(kb, na);
    std::copy(kb.begin(), kb.end(), k_bar); std::copy(na.begin(), na.end(), num_active);
  } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  return EMAT_OK;
}
emat_status emat_coalescent_sample(emat_backend* h, const double* k_bar, const int32_t* num_active, double* k_twiddle_bar_local) {
  if (!h || !k_bar || !num_active || !k_twiddle_bar_local) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->coal_builder) return fail(h, EMAT_ERR_STATE, "emat_coalescent_begin first");
  try {
    const int n = h->coal_builder->num_cells;
    std::vector<double> kt;
    h->coal_builder->sample(std::vector<double>(k_bar, k_bar + n), std::vector<int32_t>(num_active, num_active + n), kt);
    std::copy(kt.begin(), kt.end(), k_twiddle_bar_local);
  } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  return EMAT_OK;
}
emat_status emat_coalescent_finish(emat_backend* h, const double* k_twiddle_bar) {
  if (!h || !k_twiddle_bar) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->coal_builder) return fail(h, EMAT_ERR_STATE, "emat_coalescent_begin first");
  try {
    const int n = h->coal_builder->num_cells;
    auto cps = h->coal_builder->finish(std::vector<double>(k_twiddle_bar, k_twiddle_bar + n));
    for (size_t p = 0; p < h->parts.size(); ++p) h->parts[p].coal = std::move(cps[p]);
  } catch (const std::exception& ex) { return fail(h, EMAT_ERR_INVALID_ARGUMENT, ex.what()); }
  h->coal_builder.reset();
  h->have_pop = true; h->have_coal = true; h->model_dirty = true;
  h->parts_need_encoding(false);
  return EMAT_OK;
}

emat_status emat_run_local_moves(emat_backend* h, int64_t count) {
  if (!h || count < 0) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  const int64_t P = (int64_t)h->parts.size();
  const int64_t sub = count / P;   // run.cpp:683-689
  return launch_moves(h, sub, count - P * sub);
}
emat_status emat_run_moves_per_part(emat_backend* h, int64_t moves_per_part) {
  if (!h || moves_per_part < 0) return EMAT_ERR_INVALID_ARGUMENT;
  return launch_moves(h, moves_per_part, 0);
}
emat_status emat_run_moves_split(emat_backend* h, int64_t moves_per_part, int64_t extra_moves_part0) {
  if (!h || moves_per_part < 0 || extra_moves_part0 < 0) return EMAT_ERR_INVALID_ARGUMENT;
  return launch_moves(h, moves_per_part, extra_moves_part0);
}
emat_status emat_run_moves_even(emat_backend* h, int64_t moves_per_part, int32_t one_more_below) {
  if (!h || moves_per_part < 0 || one_more_below < 0 || one_more_below > (int64_t)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  return launch_moves(h, moves_per_part, 0, nullptr, one_more_below);
}
emat_status emat_synchronize(emat_backend* h) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return EMAT_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return finish_pass(h);
}
emat_status emat_recalc_derived(emat_backend* h) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  return launch_recalc(h);
}

// The reference's Subrun::check_derived_quantities (subrun.cpp:28-56) for every part, on the device, without the oracle and
// without touching the state: `tol_scale` multiplies the reference's own tolerances (1e-8 per site on lambda_i, 1e-6 on
// log_G, 1e-5 on the augmented coalescent prior; missing-site counts exact).
emat_status emat_check_derived(emat_backend* h, double tol_scale, int32_t* worst_part, double* worst4) {
  if (!h || !(tol_scale > 0.0)) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return no_device(h);
  emat_status st = emat_synchronize(h); if (st) return st;
  if (!h->slabs_on_device || !h->derived_valid) return fail(h, EMAT_ERR_STATE, "emat_check_derived: nothing has been maintained incrementally yet (run moves first)");
  st = sync_model_to_device(h); if (st) return st;
  const size_t n = h->parts.size();
  for (auto& ph : h->parts) if ((uint64_t)ph.tree.num_nodes() * 12u > (uint64_t)ph.scratch_bytes) return fail(h, EMAT_ERR_CAPACITY, "scratch region too small for the check");
  DevBuf<double> d_out; HIP_TRY(d_out.alloc(4 * n));
  std::vector<double> out(4 * n);
  st = run_over_parts(h, k_check_derived, d_out.p, out.data(), out.size(), d_out.p); if (st) return st;
  const double tol[4] = {1e-8 * tol_scale, 1e-6 * tol_scale, 1e-5 * tol_scale, 0.5};
  static const char* what[4] = {"lambda_i (per site)", "log_G", "log_augmented_coalescent_prior", "num_sites_missing (nodes that differ)"};
  int bad_part = -1, bad_q = -1; double worst_ratio = -1.0; int wp = 0;
  for (size_t p = 0; p < n; ++p) for (int q = 0; q < 4; ++q) {
    const double v = out[4 * p + q], ratio = v / tol[q];
    if (!(ratio <= worst_ratio)) { worst_ratio = ratio; wp = (int)p; }      // NaN counts as worst
    if (!(v < tol[q]) && bad_part < 0) { bad_part = (int)p; bad_q = q; }
  }
  if (worst_part) *worst_part = bad_part >= 0 ? bad_part : wp;
  if (worst4) for (int q = 0; q < 4; ++q) worst4[q] = out[4 * (size_t)(bad_part >= 0 ? bad_part : wp) + q];
  if (bad_part >= 0) {
    char buf[256]; snprintf(buf, sizeof buf, "emat_check_derived: part %d: incremental %s differs from its recomputation by %.3g (tolerance %.3g)", bad_part, what[bad_q], out[4 * (size_t)bad_part + bad_q], tol[bad_q]);
    return fail(h, EMAT_ERR_INTERNAL, buf);
  }
  return EMAT_OK;
}

emat_status emat_get_totals(emat_backend* h, double* log_G, double* log_aug) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  emat_status st;
  if (!h->slabs_on_device || !h->derived_valid) { st = launch_recalc(h); if (st) return st; }
  st = pull_headers(h); if (st) return st;   // 256 bytes per part through a gather kernel; the slabs stay where they are
  double g = 0.0, a = 0.0;
  for (size_t p = 0; p < h->parts.size(); ++p) { const SlabHeader* H = header_of(h, p); g += H->log_G; a += H->log_aug_prior; }   // part order: reproducible
  if (log_G) *log_G = g;
  if (log_aug) *log_aug = a;
  return EMAT_OK;
}
emat_status emat_part_get_sizes(emat_backend* h, int32_t part_id, int32_t* nn, int32_t* nm, int32_t* ni, int32_t* nf) {
  if (!h || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = pull_from_device(h); if (st) return st;
  const FlatTree& t = h->parts[part_id].tree;
  if (nn) *nn = t.num_nodes(); if (nm) *nm = t.num_muts(); if (ni) *ni = t.num_intervals(); if (nf) *nf = t.num_from_states();
  return EMAT_OK;
}
emat_status emat_part_download(emat_backend* h, int32_t part_id, emat_flat_tree* out) {
  if (!h || !out || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = pull_from_device(h); if (st) return st;
  const FlatTree& t = h->parts[part_id].tree;
  const int n = t.num_nodes();
  if (out->num_nodes < n || out->cap_muts < t.num_muts() || out->cap_intervals < t.num_intervals() || out->cap_from_states < t.num_from_states())
    return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_part_download: output arrays too small (see emat_part_get_sizes)");
  out->num_nodes = n; out->root = t.root;
  std::copy(t.parent.begin(), t.parent.end(), out->parent); std::copy(t.child0.begin(), t.child0.end(), out->child0); std::copy(t.child1.begin(), t.child1.end(), out->child1);
  std::copy(t.t.begin(), t.t.end(), out->t); std::copy(t.t_min.begin(), t.t_min.end(), out->t_min); std::copy(t.t_max.begin(), t.t_max.end(), out->t_max);
  std::copy(t.mut_offset.begin(), t.mut_offset.end(), out->mut_offset); std::copy(t.mut_site.begin(), t.mut_site.end(), out->mut_site);
  std::copy(t.mut_from.begin(), t.mut_from.end(), out->mut_from); std::copy(t.mut_to.begin(), t.mut_to.end(), out->mut_to); std::copy(t.mut_t.begin(), t.mut_t.end(), out->mut_t);
  std::copy(t.miss_offset.begin(), t.miss_offset.end(), out->miss_offset); std::copy(t.miss_start.begin(), t.miss_start.end(), out->miss_start); std::copy(t.miss_end.begin(), t.miss_end.end(), out->miss_end);
  std::copy(t.mfs_offset.begin(), t.mfs_offset.end(), out->mfs_offset); std::copy(t.mfs_site.begin(), t.mfs_site.end(), out->mfs_site); std::copy(t.mfs_state.begin(), t.mfs_state.end(), out->mfs_state);
  return EMAT_OK;
}
emat_status emat_part_get_derived(emat_backend* h, int32_t part_id, double* lambda_i, int32_t* num_missing, double* log_G, double* log_aug) {
  if (!h || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st;
  if (!h->slabs_on_device || !h->derived_valid) { st = launch_recalc(h); if (st) return st; }
  st = pull_from_device(h); if (st) return st;
  const uint8_t* slab = h->h_slabs.data() + h->parts[part_id].slab_off;
  const SlabHeader* H = (const SlabHeader*)slab; const NodeRec* N = (const NodeRec*)(slab + H->off_nodes);
  for (int i = 0; i < H->n_nodes; ++i) { if (lambda_i) lambda_i[i] = N[i].lambda; if (num_missing) num_missing[i] = N[i].n_missing; }
  if (log_G) *log_G = H->log_G;
  if (log_aug) *log_aug = H->log_aug_prior;
  return EMAT_OK;
}
emat_status emat_part_get_state_frequencies(emat_backend* h, int32_t part_id, int32_t* num_partitions, int32_t* counts) {
  if (!h || !num_partitions || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_ref || !h->have_evo) return fail(h, EMAT_ERR_STATE, "set_ref_sequence and set_evo first");
  if (h->gt.gather_pending) { emat_status st = gt_finish_gather(h); if (st) return st; }   // (a gather on its way may still move the reference sequence with the root's)
  const int P = h->num_partitions;
  if (*num_partitions < P || !counts) { *num_partitions = P; return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_part_get_state_frequencies: room for fewer site partitions than the model has"); }
  *num_partitions = P;
  std::copy(h->ref_freqs.begin(), h->ref_freqs.begin() + (size_t)P * 4, counts);   // the host's copy of the table the kernels read (d_ref_freqs)
  return EMAT_OK;
}
emat_status emat_part_get_coalescent(emat_backend* h, int32_t part_id, int32_t* num_cells, double* k_bar_p, double* k_tw_p, double* k_tw,
                                     double* popsize_bar, int32_t* num_active, double* t_ref, double* t_step) {
  if (!h || !num_cells || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_coal) return fail(h, EMAT_ERR_STATE, "no coalescent parts built");
  emat_status st = pull_from_device(h); if (st) return st;
  const HostCoalPart& cp = h->parts[part_id].coal;
  const int n = cp.n_cells_total;
  if (*num_cells < n) { *num_cells = n; return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, "emat_part_get_coalescent: arrays too small"); }
  *num_cells = n;
  // expand the window back to the logical vectors of the reference (zeros outside the window; the three
  // shared vectors are only known inside it)
  for (int i = 0; i < n; ++i) {
    int w = i - cp.cell_first; bool in = w >= 0 && w < (int)cp.k_bar_p.size();
    if (k_bar_p) k_bar_p[i] = in ? cp.k_bar_p[w] : 0.0;
    if (k_tw_p) k_tw_p[i] = in ? cp.k_twiddle_bar_p[w] : 0.0;
    if (k_tw) k_tw[i] = in ? cp.k_twiddle_bar[w] : __builtin_nan("");
    if (popsize_bar) popsize_bar[i] = in ? cp.popsize_bar[w] : __builtin_nan("");
    if (num_active) num_active[i] = in ? cp.num_active_parts[w] : -1;
  }
  if (t_ref) *t_ref = cp.t_ref;
  if (t_step) *t_step = cp.t_step;
  return EMAT_OK;
}
emat_status emat_part_get_rng(emat_backend* h, int32_t part_id, uint64_t* key, uint64_t* counter, uint64_t* spare, int32_t* has_spare) {
  if (!h || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  if (h->host_only || !h->slabs_on_device) return fail(h, EMAT_ERR_STATE, "emat_part_get_rng: the parts are not on a device");
  emat_status st = pull_headers(h); if (st) return st;
  const SlabHeader* H = header_of(h, (size_t)part_id);
  if (key) *key = H->rng_key;
  if (counter) *counter = H->rng_counter;
  if (spare) *spare = H->rng_spare;
  if (has_spare) *has_spare = (int32_t)H->rng_has_spare;
  return EMAT_OK;
}
emat_status emat_part_get_stats(emat_backend* h, int32_t part_id, emat_part_stats* out) {
  if (!h || !out || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = pull_headers(h); if (st) return st;
  *out = h->parts[part_id].stats;
  if (h->slabs_on_device && !h->host_only) {
    const SlabHeader* H = header_of(h, (size_t)part_id);
    out->status = H->status; out->num_nodes = H->n_nodes; out->moves_done = H->moves_done;
    for (int k = 0; k < 5; ++k) { out->proposed[k] = H->proposed[k]; out->accepted[k] = H->accepted[k]; }
    out->algorithmic_bytes = H->alg_bytes; out->algorithmic_write_bytes = 16 * (int64_t)H->alg_write16; out->rng_draws = (int64_t)H->rng_counter; out->device_ticks = H->device_ticks;
    if (H->status != 0) h->set_error("part " + std::to_string(part_id) + " stopped with status " + std::to_string(H->status) + " at device line " + std::to_string(H->fail_line));
  }
  return EMAT_OK;
}
emat_status emat_part_get_trace(emat_backend* h, int32_t part_id, int32_t* num_moves, double* trace) {
  if (!h || !num_moves || !trace || part_id < 0 || part_id >= (int)h->parts.size()) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = pull_from_device(h); if (st) return st;
  if (!h->slabs_on_device) { *num_moves = 0; return EMAT_OK; }
  const uint8_t* slab = h->h_slabs.data() + h->parts[part_id].slab_off;
  const SlabHeader* H = (const SlabHeader*)slab;
  int n = std::min(*num_moves, H->trace_len);
  std::memcpy(trace, slab + H->off_trace, (size_t)n * 32);
  *num_moves = n;
  return EMAT_OK;
}
/* Sufficient statistics of the global moves over the parts of this handle (header: emat_get_global_stats). */
emat_status emat_get_global_stats(emat_backend* h, int32_t num_partitions, double* Ttwiddle_beta_a, int64_t* num_muts_beta_ab, int64_t* num_muts) {
  if (!h || !Ttwiddle_beta_a || !num_muts_beta_ab) return EMAT_ERR_INVALID_ARGUMENT;
  // (require_settled_parts' sequence, spelled out: the two checks of num_partitions answer before materialize does)
  if (h->host_only) return no_device(h);
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  emat_status st = sync_model_to_device(h); if (st) return st;
  if (num_partitions != h->num_partitions) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "num_partitions does not match emat_set_evo");
  if (num_partitions > k_max_stats_partitions) return fail(h, EMAT_ERR_CAPACITY, "emat_get_global_stats supports at most 4 site partitions");
  st = materialize(h); if (st) return st;
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }   // statistics of chains that finished their moves, or a loud failure
  const int W = 4 * num_partitions;
  for (auto& ph : h->parts)   // the per-node table lives in the part's scratch region
    if ((uint64_t)ph.n_nodes * W * 8u > (uint64_t)ph.scratch_bytes) return fail(h, EMAT_ERR_CAPACITY, "scratch region too small for the statistics table");
  const size_t n = h->parts.size();
  if (h->d_stats.n < n * k_stats_row) { std::vector<double> z(n * k_stats_row, 0.0); HIP_TRY(h->d_stats.upload(z.data(), z.size())); }
  std::vector<double> rows(n * k_stats_row);
  st = run_over_parts(h, k_global_stats, h->d_stats.p, rows.data(), rows.size()); if (st) return st;   // (the kernel finds d_stats in its KernelArgs)
  for (int k = 0; k < W; ++k) Ttwiddle_beta_a[k] = 0.0;
  for (int k = 0; k < 4 * W; ++k) num_muts_beta_ab[k] = 0;
  int64_t nm = 0;
  for (size_t p = 0; p < n; ++p) {   // fixed order: reproducible sums
    const double* r = rows.data() + p * k_stats_row;
    for (int k = 0; k < W; ++k) Ttwiddle_beta_a[k] += r[k];
    for (int k = 0; k < 4 * W; ++k) num_muts_beta_ab[k] += (int64_t)r[k_max_stats_partitions * 4 + k];
    nm += (int64_t)r[k_stats_row - 1];
  }
  if (num_muts) *num_muts = nm;
  return EMAT_OK;
}
/* calc_num_muts_l on the device (header: emat_get_num_muts_l) */
emat_status emat_get_num_muts_l(emat_backend* h, int32_t* num_muts_l) {
  if (!h || !num_muts_l) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = require_settled_parts(h); if (st) return st;
  DevBuf<int32_t> d_out;
  HIP_TRY(d_out.alloc((size_t)h->L));
  HIP_TRY(hipMemsetAsync(d_out.p, 0, (size_t)h->L * sizeof(int32_t), h->stream));
  return run_over_parts(h, k_num_muts_l, d_out.p, num_muts_l, (size_t)h->L, d_out.p);
}

/* calc_Ttwiddle_l on the device (header: emat_get_part_tree_lengths / emat_Ttwiddle_l_partial / emat_Ttwiddle_l_finish) */
emat_status emat_get_part_tree_lengths(emat_backend* h, double* tree_length_of_part) {
  if (!h || !tree_length_of_part) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = require_settled_parts(h); if (st) return st;
  const size_t n = h->parts.size();
  DevBuf<double> d_out; HIP_TRY(d_out.alloc(n));
  return run_over_parts(h, k_part_lengths, d_out.p, tree_length_of_part, n, d_out.p);
}
emat_status emat_Ttwiddle_l_partial(emat_backend* h, const int32_t* ext_offset, const int32_t* ext_node, const double* ext_length,
                                    double* S, double* R, double* tree_length_below_root) {
  if (!h || !ext_offset || !S || !R) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = require_settled_parts(h); if (st) return st;
  const size_t n = h->parts.size(); const size_t L = (size_t)h->L;
  const int32_t n_ext = ext_offset[n];
  if (n_ext < 0 || (n_ext > 0 && (!ext_node || !ext_length))) return EMAT_ERR_INVALID_ARGUMENT;
  for (size_t p = 0; p < n; ++p) {
    if (ext_offset[p] > ext_offset[p + 1]) return EMAT_ERR_INVALID_ARGUMENT;
    for (int32_t k = ext_offset[p]; k < ext_offset[p + 1]; ++k) if (ext_node[k] < 0 || ext_node[k] >= h->parts[p].n_nodes) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "ext_node out of range");
    if ((uint64_t)h->parts[p].n_nodes * 8u > (uint64_t)h->parts[p].scratch_bytes) return fail(h, EMAT_ERR_CAPACITY, "scratch region too small for the length table");
  }
  DevBuf<int32_t> d_off, d_node; DevBuf<double> d_val, d_S, d_D, d_T;
  HIP_TRY(d_off.upload(ext_offset, n + 1)); HIP_TRY(d_node.upload(ext_node, (size_t)n_ext)); HIP_TRY(d_val.upload(ext_length, (size_t)n_ext));
  HIP_TRY(d_S.alloc(L)); HIP_TRY(d_D.alloc(L + 1)); HIP_TRY(d_T.alloc(1));
  HIP_TRY(hipMemsetAsync(d_S.p, 0, L * sizeof(double), h->stream)); HIP_TRY(hipMemsetAsync(d_D.p, 0, (L + 1) * sizeof(double), h->stream)); HIP_TRY(hipMemsetAsync(d_T.p, 0, sizeof(double), h->stream));
  KernelArgs a = make_args(h);
  hipLaunchKernelGGL(k_ttwiddle_l, dim3((unsigned)n), dim3(k_wave), 0, h->stream, a, d_off.p, d_node.p, d_val.p, d_S.p, d_D.p, d_T.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::vector<double> D(L + 1);
  HIP_TRY(hipMemcpy(S, d_S.p, L * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(D.data(), d_D.p, (L + 1) * sizeof(double), hipMemcpyDeviceToHost));
  double run = 0.0;
  for (size_t l = 0; l < L; ++l) { run += D[l]; R[l] = run; }
  if (tree_length_below_root && h->root_part >= 0) HIP_TRY(hipMemcpy(tree_length_below_root, d_T.p, sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}
emat_status emat_Ttwiddle_l_finish(emat_backend* h, const double* S_sum, const double* R_sum, double tree_length, double* Ttwiddle_l) {
  if (!h || !S_sum || !R_sum || !Ttwiddle_l) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_ref || !h->have_evo) return fail(h, EMAT_ERR_STATE, "set_ref_sequence and set_evo first");
  for (int l = 0; l < h->L; ++l) {
    const double q_ref = -h->q[(size_t)h->partition_for_site[l] * 16 + (size_t)h->ref[l] * 5];   // q^(l)_a of the reference state
    Ttwiddle_l[l] = q_ref * (tree_length - R_sum[l]) + S_sum[l];
  }
  return EMAT_OK;
}

/* Scalable_coalescent_prior on the device (header: emat_scalable_coalescent_partial / _log_prior / emat_get_scalable_coalescent_log_prior) */
emat_status emat_scalable_coalescent_partial(emat_backend* h, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                                             double* k_bar_partial, double* sum_neg_log_pop, int32_t* first_cell_needed) {
  if (!h || !(t_step > 0.0) || num_cells < 0 || (num_cells > 0 && !k_bar_partial)) return EMAT_ERR_INVALID_ARGUMENT;
  // (require_settled_parts' sequence, spelled out: a missing population model answers before the model is sent and materialize asks for cell tables)
  if (h->host_only) return no_device(h);
  if (h->parts.empty()) return fail(h, EMAT_ERR_STATE, "no parts uploaded");
  if (!h->have_pop) return fail(h, EMAT_ERR_STATE, "no population model: emat_build_coalescent_parts (or the staged form) first");
  emat_status st = sync_model_to_device(h); if (st) return st;
  st = materialize(h); if (st) return st;
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }
  const size_t n = h->parts.size();
  // a part's nodes span about as many cells of this grid as of its very-scalable window (same cell width, other origin)
  std::vector<uint64_t> off(n); std::vector<uint32_t> cap(n); uint64_t tot = 0;
  const double ratio = h->parts[0].coal.t_step > 0.0 ? h->parts[0].coal.t_step / t_step : 1.0;
  for (size_t p = 0; p < n; ++p) {
    const PartHost& ph = h->parts[p];
    const size_t window = (size_t)std::max(0, ph.coal.n_cells_total - ph.coal.cell_first);   // (= k_bar_p.size(); the vectors themselves may live only on the device)
    const double cells_vs = (double)(ph.includes_run_root ? 2 * window + 512 : window);
    cap[p] = (uint32_t)std::min<double>(1e7, std::ceil(cells_vs * ratio) + 4.0);
    off[p] = tot; tot += cap[p];
  }
  DevBuf<uint64_t> d_off; DevBuf<uint32_t> d_cap; DevBuf<double> d_out, d_meta;
  HIP_TRY(d_off.upload(off.data(), n)); HIP_TRY(d_cap.upload(cap.data(), n)); HIP_TRY(d_out.alloc((size_t)tot)); HIP_TRY(d_meta.alloc(n * 4));
  KernelArgs a = make_args(h);
  hipLaunchKernelGGL(k_scalable_prior, dim3((unsigned)n), dim3(k_wave), 0, h->stream, a, t_ref, t_step, d_off.p, d_cap.p, d_out.p, d_meta.p);
  HIP_TRY(hipGetLastError());
  std::vector<double> rows((size_t)tot), meta(n * 4);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rows.data(), d_out.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(meta.data(), d_meta.p, meta.size() * sizeof(double), hipMemcpyDeviceToHost));
  int first_needed = 0;
  for (size_t p = 0; p < n; ++p) {
    if (meta[4 * p + 3] != 0.0) return fail(h, EMAT_ERR_CAPACITY, "part " + std::to_string(p) + " spans more grid cells than expected");
    if (meta[4 * p + 1] > 0.0) first_needed = std::min(first_needed, (int)meta[4 * p]);
  }
  if (first_cell_needed) *first_cell_needed = first_needed;
  for (int j = 0; j < num_cells; ++j) k_bar_partial[j] = 0.0;
  double logs = 0.0;
  for (size_t p = 0; p < n; ++p) {   // part order: reproducible sums
    const int jlo = (int)meta[4 * p], cnt = (int)meta[4 * p + 1];
    logs += meta[4 * p + 2];
    if (num_cells == 0) continue;
    if (cnt > 0 && (jlo < first_cell || jlo + cnt > first_cell + num_cells)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, "the cell range given does not cover every node (ask with num_cells = 0 for first_cell_needed)");
    const double* row = rows.data() + off[p];
    for (int k = 0; k < cnt; ++k) k_bar_partial[jlo - first_cell + k] += row[k];
    if (h->parts[p].includes_run_root) for (int j = jlo + cnt; j < first_cell + num_cells && j < 0; ++j) k_bar_partial[j - first_cell] -= 1.0;   // the root part's constant tail
  }
  if (sum_neg_log_pop) *sum_neg_log_pop = logs;
  return EMAT_OK;
}
emat_status emat_scalable_coalescent_log_prior(emat_backend* h, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                                               const double* k_bar_partial_sum, double sum_neg_log_pop, double* log_prior) {
  if (!h || !(t_step > 0.0) || num_cells < 0 || (num_cells > 0 && !k_bar_partial_sum) || !log_prior) return EMAT_ERR_INVALID_ARGUMENT;
  if (!h->have_pop) return fail(h, EMAT_ERR_STATE, "no population model: emat_build_coalescent_parts (or the staged form) first");
  double r = 0.0;
  for (int k = 0; k < num_cells; ++k) {   // scalable_coalescent.cpp:163-187, cells in increasing time
    const int j = first_cell + k;
    if (j >= 0) break;
    const double lb = t_ref + (double)j * t_step, ub = lb + t_step;
    double popsize_bar = h->pop.pop_integral(lb, ub) / t_step;
    if (popsize_bar == 0.0) popsize_bar = 1e-100;   // the reference's stopgap (:62-64)
    const double kbar = 1.0 + k_bar_partial_sum[k];   // cells before t_ref start at one lineage (:56)
    r -= t_step * kbar * (kbar - 1) / (2.0 * popsize_bar);
  }
  *log_prior = r + sum_neg_log_pop;
  return EMAT_OK;
}
emat_status emat_get_scalable_coalescent_log_prior(emat_backend* h, double t_ref, double t_step, double* log_prior) {
  if (!h || !log_prior) return EMAT_ERR_INVALID_ARGUMENT;
  int32_t first = 0;
  emat_status st = emat_scalable_coalescent_partial(h, t_ref, t_step, 0, 0, nullptr, nullptr, &first); if (st) return st;
  std::vector<double> kb((size_t)(-first)); double logs = 0.0;
  st = emat_scalable_coalescent_partial(h, t_ref, t_step, first, -first, kb.data(), &logs, nullptr); if (st) return st;
  return emat_scalable_coalescent_log_prior(h, t_ref, t_step, first, -first, kb.data(), logs, log_prior);
}

/* Duration of the k_run_moves launch of the last pass, from HIP events around that launch on its stream. */
emat_status emat_last_kernel_ms(emat_backend* h, double* ms, int32_t* num_parts_in_kernel) {
  if (!h || !ms) return EMAT_ERR_INVALID_ARGUMENT;
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return fail(h, EMAT_ERR_NO_DEVICE, "host-only handle");
  HIP_TRY(hipEventSynchronize(h->ev_stop));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, h->ev_start, h->ev_stop));
  *ms = f;
  if (num_parts_in_kernel) *num_parts_in_kernel = (int)h->parts.size();
  return EMAT_OK;
}
emat_status emat_last_run_ms(emat_backend* h, double* ms) {
  if (!h || !ms) return EMAT_ERR_INVALID_ARGUMENT;
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->host_only) return fail(h, EMAT_ERR_NO_DEVICE, "host-only handle");
  HIP_TRY(hipEventSynchronize(h->ev_stop));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, h->ev_start, h->ev_stop));
  h->last_run_ms = f; *ms = f;
  return EMAT_OK;
}

}  // extern "C"

#include "emat_debug_host.hpp"      // the emat_debug_* hooks and the profiling builds' read-outs
#include "emat_gtree_host.hpp"
#include "emat_mcc_host.hpp"
#include "emat_probe_host.hpp"          // the probers' driver and the resident tree's entry points
#include "emat_samples_probe_host.hpp"  // the store's entry points
#include "emat_mcc_summary_host.hpp"    // node-age spreads and mutation support on the last derivation
#include "emat_build_host.hpp"
#include "emat_utree_host.hpp"
#include "emat_site_rate_host.hpp"
#include "emat_coal_stats_host.hpp"
#include "emat_skygrid_host.hpp"
#include "emat_exp_pop_host.hpp"
#include "emat_subst_stats_host.hpp"    // the parts' substitution statistics and the frame of the two groups that read them
#include "emat_subst_host.hpp"
#include "emat_mpox_host.hpp"
#include "emat_align_host.hpp"          // the alignment store's entry points
