// emat_state_host.hpp -- what a handle holds: device and page-locked buffers, the host records of the parts, of the HBM-resident
// tree, of the probers and of the sample store, and `emat_backend` itself with the transitions of its part state.
//
// Included by emat_backend.hip after the kernel headers.
#ifndef EMAT_STATE_HOST_HPP_
#define EMAT_STATE_HOST_HPP_

namespace emat {

// =================================================================================================
// Host side
// =================================================================================================
// (reports through the handle `h` of the function it is used in)
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { h->set_error(std::string(#expr) + ": " + hipGetErrorString(_e)); return EMAT_ERR_HIP; } } while (0)

template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  // Room for `count` elements, contents undefined.  A buffer that must grow grows by a quarter more than asked: two dozen buffers are sized by the
  // number of parts, which creeps up from cycle to cycle within a stencil period (8 000 -> 14 000 at C4 with the part-size limit), and growing to the
  // exact need re-allocated a dozen of them EVERY cycle -- hipFree is 54 us a call (rocprofv3 --hip-trace of 40 whole cycles, round 6: 496 hipFree).
  hipError_t alloc(size_t count) {
    if (count > n) { if (p) (void)hipFree(p); p = nullptr; n = 0; const size_t want = count + (n_grown ? count / 4 : 0); hipError_t e = hipMalloc((void**)&p, std::max<size_t>(want, 1) * sizeof(T)); if (e != hipSuccess) return e; n = want; n_grown = true; }
    return hipSuccess;
  }
  bool n_grown = false;   // the first allocation is exact (most buffers are allocated once); every later one has room to spare
  hipError_t alloc_roomy(size_t count) { return count > n ? alloc(count + count / 4) : hipSuccess; }   // for buffers whose need creeps up from cycle to cycle: a quarter more than asked, so that most new maxima fit
  hipError_t upload(const T* src, size_t count) {
    hipError_t e = alloc(count); if (e != hipSuccess) return e;
    if (count) return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
    return hipSuccess;
  }
};

// Host mirror of the device slabs in page-locked memory (grow-only): the per-cycle 64 MB H2D / D2H of C4 run at PCIe
// speed instead of being staged through a bounce buffer.  Not zero-filled: encode_slab initialises what it owns.
struct PinnedBytes {
  uint8_t* p = nullptr; size_t n = 0, cap = 0;
  ~PinnedBytes() { if (p) (void)hipHostFree(p); }
  uint8_t* data() { return p; }
  const uint8_t* data() const { return p; }
  size_t size() const { return n; }
  hipError_t resize(size_t bytes) {
    if (bytes > cap) {
      if (p) (void)hipHostFree(p);
      p = nullptr; cap = 0;
      const size_t want = bytes + bytes / 8;
      hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
      if (e != hipSuccess) return e;
      cap = want;
    }
    n = bytes;
    return hipSuccess;
  }
};

struct PartHost {
  FlatTree tree;
  bool includes_run_root = false;
  HostRng rng;
  HostCoalPart coal;
  bool uploaded = false;
  // slab geometry
  uint64_t slab_off = 0;
  uint32_t slab_bytes = 0, scratch_bytes = 0;
  int32_t n_nodes = 0;             // (the tree itself may live only on the device: emat_tree_repartition)
  emat_part_stats stats{};
  std::vector<double> trace;       // the part's move trace so far (4 doubles per move), carried over re-materialisations
  double space_boost = 1.0;        // multiplier of the heap and scratch capacities; doubled when the part ran out of space
  int cell_boost = 1;              // multiplier of the room the root part's grid gets to grow into; quadrupled when it ran out
  // What the moves maintain INCREMENTALLY (lambda_i and the missing-site count of every node, log_G, the partial coalescent prior), kept across a
  // re-materialisation in the middle of a pass (finish_pass: some part ran out of slab space or grid cells).  The reference recomputes these when a Subrun
  // is made and never again (subrun.cpp:17-26); recomputing them half way gives the same numbers up to rounding -- and a chain that can tell: a node whose
  // d log G / dt cancels exactly (every site missing below one child or the other) takes the uniform branch of the bounded exponential with the maintained
  // lambda_i and the other branch with a recomputed one that is two units in the last place off (EMAT_FUZZ_SEED=6202, case 53, found in round 6).
  std::vector<double> kept_lambda; std::vector<int32_t> kept_n_missing; std::vector<uint64_t> kept_miss_dl; double kept_log_G = 0.0, kept_log_aug_prior = 0.0;
  bool derived_kept = false;       // set by finish_pass just before it re-materialises, consumed (and cleared) by materialize
};

// The whole tree in HBM (emat_gtree_kernels.hpp) with the host mirrors the partitioner and the coalescent builder need:
// topology and node times, a few MB per cycle instead of every list of every node.
struct GTreeHost {
  bool resident = false;            // emat_tree_upload was called
  bool parts_live = false;          // the slabs hold the parts of `partition` (between emat_tree_repartition and emat_tree_reassemble)
  int32_t n = 0;
  DevBuf<int32_t> parent, c0, c1, root; DevBuf<double> t; DevBuf<float> t_min, t_max; DevBuf<GList> muts, miss, mfs;
  DevBuf<MutRec> mut_heap; DevBuf<IvRec> iv_heap; DevBuf<FsRec> fs_heap; DevBuf<uint32_t> tops; DevBuf<int32_t> status;
  uint32_t used[3] = {0, 0, 0};     // records in use in the three heaps
  int32_t pool_regrows = 0, heap_regrows = 0, large_measures = 0;
  // current partition
  int32_t P = 0, root_part = -1, lo = 0, hi = 0;   // this process runs the parts [lo, hi) of the partition
  std::vector<int32_t> h_part_off, h_orig, h_kid0, h_kid1;   // host copies (h_orig / h_kid* only when the partition came from the host or was asked for)
  bool partition_on_device = false;   // made by emat_tree_partition
  DevBuf<int32_t> lidx;
  DevBuf<uint8_t> d_is_cut; DevBuf<int32_t> d_cut, d_sizes, d_part_status;   // emat_tree_partition's inputs and counts (kept: three allocations less per cycle)
  PinnedBytes pin_sizes, pin_measure;                                         // where its sizes + offsets, and the measures queued behind it, land
  hipEvent_t ev_sizes = nullptr, ev_measure = nullptr;
  bool measure_queued = false;      // k_gt_measure of the current partition was launched by emat_tree_partition, its results are on their way to pin_measure
  ~GTreeHost() { if (ev_sizes) (void)hipEventDestroy(ev_sizes); if (ev_measure) (void)hipEventDestroy(ev_measure); }
  DevBuf<GRootDelta> root_deltas_in;
  DevBuf<int32_t> part_off, orig, kid0, kid1, lpar;
  DevBuf<double> co_kbar, co_ktw, co_k_bar, co_k_tw, co_popsize, co_tsop; DevBuf<int32_t> co_num_active;   // the coalescent grid, when it is built on the device
  DevBuf<int32_t> measure_list;
  DevBuf<GMeasure> measure; DevBuf<MutRec> pool_muts; DevBuf<IvRec> pool_ivs; DevBuf<uint32_t> pool_tops;
  DevBuf<GPartDesc> desc; DevBuf<uint8_t> cells;
  DevBuf<GRootDelta> root_deltas; DevBuf<int32_t> n_root_deltas;
  // host mirrors
  std::vector<int32_t> h_parent, h_c0, h_c1; std::vector<double> h_t; std::vector<float> h_t_min, h_t_max; int32_t h_root = EMAT_NO_NODE;
  // Kept current by every reassemble: the children of every node, packed (pin_kids: n pairs), the root and its time -- what a cycle's
  // partitioner needs.  The arrays above follow only when somebody asks for them (gt_full_mirrors).
  DevBuf<int2> d_kids; PinnedBytes pin_kids; double h_root_t = 0.0; bool full_mirrors_stale = false;
  DevBuf<GClimb> climb; bool climb_current = false;   // GClimb records of every node (k_gt_pack_climb), remade before a measuring pass if lists or links were written since
  bool d_kids_current = false;      // d_kids holds every node's children (k_gt_gather_links only rewrites the inner nodes of the parts it sees)
  DevBuf<double> d_root_t; PinnedBytes pin_small;   // the root's time; { int32 root, int32 n_root_deltas, double t_root } on their way to the host
  // emat_tree_reassemble of a single process returns once topology and root are on the host: k_gt_gather may still be running.
  // Whoever touches the device-resident tree next (gt_require) waits for it and checks how it went (gt_finish_gather).
  bool gather_pending = false; std::vector<GRootDelta> gather_rd;
  emat_status gather_failed = EMAT_OK; std::string gather_failed_text;   // a deferred gather that failed: sticky until emat_tree_upload (gt_require)
  // The flags above (resident, parts_live, P, partition_on_device, measure_queued, d_kids_current, full_mirrors_stale, climb_current,
  // gather_pending, gather_failed) are written only by the transitions below.
  void tree_uploaded() {            // a new tree: no partition (one made of the tree that was here says nothing about this one), no parts, mirrors as uploaded
    resident = true; parts_live = false; P = 0; partition_on_device = false; measure_queued = false;
    full_mirrors_stale = false; d_kids_current = false; climb_current = false;
    gather_pending = false; gather_failed = EMAT_OK; gather_failed_text.clear();
  }
  void partition_made(int32_t parts, int32_t root) { P = parts; root_part = root; partition_on_device = true; measure_queued = false; h_orig.clear(); h_kid0.clear(); }   // by emat_tree_partition, on the device
  void measure_was_queued() { measure_queued = true; }                       // ... with k_gt_measure behind it
  void partition_dropped() { P = 0; partition_on_device = false; measure_queued = false; }   // ... which the device then refused
  bool take_queued_measure() { const bool q = measure_queued; measure_queued = false; return q; }   // a repartition uses the queued measures, or makes its own
  void parts_recalled(int32_t parts, int32_t root) { P = parts; root_part = root; parts_live = false; }   // a repartition begins: whatever was out on slabs is about to be rebuilt
  void partition_handed_in() { partition_on_device = false; }                // as arrays: the host copies are the caller's
  void parts_went_out() { parts_live = true; }                               // k_gt_build wrote the slabs
  void parts_came_back() { parts_live = false; }                             // gathered (or about to be: a deferred gather), or replaced by host parts (emat_begin_upload)
  void kids_packed() { d_kids_current = true; }                              // k_gt_pack_kids filled d_kids
  void links_fetched() { d_kids_current = true; full_mirrors_stale = true; } // new links in d_kids / pin_kids, root and root time on the host; the separate arrays lag
  void mirrors_refreshed() { full_mirrors_stale = false; }
  void lists_or_links_rewritten() { climb_current = false; }                 // (a gather, an apply)
  void climb_remade() { climb_current = true; }
  void gather_deferred() { gather_pending = true; }                          // launched, not yet waited for
  void gather_finished() { gather_pending = false; }
  void gather_went_wrong(emat_status st, const std::string& text) { gather_failed = st; gather_failed_text = text; }   // stays pending and failed until tree_uploaded
  // The three list heaps in one place: f(heap, k) with used[k] the records in use; the record type is the heap's element type.
  template <class F> emat_status for_each_heap(F&& f) {
    if (emat_status st = f(mut_heap, 0)) return st;
    if (emat_status st = f(iv_heap, 1)) return st;
    return f(fs_heap, 2);
  }
  const int32_t* kids() const { return (const int32_t*)pin_kids.data(); }   // [2 v] = child0, [2 v + 1] = child1
  GTreeDev dev() {
    GTreeDev g{};
    g.n_nodes = n; g.climb = climb.p; g.root = root.p; g.parent = parent.p; g.c0 = c0.p; g.c1 = c1.p; g.t = t.p; g.t_min = t_min.p; g.t_max = t_max.p;
    g.muts = muts.p; g.miss = miss.p; g.mfs = mfs.p; g.mut_heap = mut_heap.p; g.iv_heap = iv_heap.p; g.fs_heap = fs_heap.p;
    g.mut_cap = (uint32_t)mut_heap.n; g.iv_cap = (uint32_t)iv_heap.n; g.fs_cap = (uint32_t)fs_heap.n; g.tops = tops.p;
    return g;
  }
  GPartition partition() { GPartition q{}; q.num_parts = P; q.root_part = root_part; q.part_off = part_off.p; q.orig = orig.p; q.kid0 = kid0.p; q.kid1 = kid1.p; q.lpar = lpar.p; return q; }
  GPools pools() { GPools q{}; q.muts = pool_muts.p; q.ivs = pool_ivs.p; q.mut_cap = (uint32_t)pool_muts.n; q.iv_cap = (uint32_t)pool_ivs.n; q.tops = pool_tops.p; return q; }
};

// The whole-tree coalescent statistics both population groups read (emat_coal_stats_host.hpp), from the caller or from the tree in HBM, and their grid: grow-only, the numbers are the last call's.
struct CoalStatsScratch {
  DevBuf<double> k_bar, inner_t, extent;
  DevBuf<int32_t> count;
  int32_t first_cell = 0, num_cells = 0, num_inner = 0;
};

// What the Skygrid population moves work in (emat_skygrid_kernels.hpp, emat_skygrid_host.hpp): grow-only, kept from call to call.
struct SkygridScratch {
  DevBuf<double> x, g, popsize_bar, c, W, gamma_out, result, trace;
};

// What the Exponential population moves work in (emat_exp_pop_kernels.hpp, emat_exp_pop_host.hpp): grow-only.
struct ExpPopScratch {
  DevBuf<double> state, partials, result;
  DevBuf<emat_exp_pop_step> trace;
};

// The substitution statistics both groups below read (emat_subst_stats_host.hpp), from the caller or from the parts on the handle: k_sb_stats_doubles doubles, the last call's.
struct SubstStatsScratch { DevBuf<double> record; };

// What a group that runs as one wavefront on that record works in, the substitution-model moves (emat_subst_kernels.hpp, emat_subst_host.hpp) and the APOBEC
// model's (emat_mpox_kernels.hpp, emat_mpox_host.hpp): the result's doubles and the trace's steps; grow-only.
template <class Step> struct OneWaveScratch {
  DevBuf<double> result; DevBuf<Step> trace;
};
using SubstScratch = OneWaveScratch<emat_subst_step>;
using MpoxScratch = OneWaveScratch<emat_mpox_round>;

// What the site-rate moves work in (emat_site_rate_kernels.hpp, emat_site_rate_host.hpp): grow-only, sized by the handle's L at the first call.
struct SiteRateScratch {
  DevBuf<double> T, nu_new, d_log_G, d_prior, result; DevBuf<int32_t> M;
  DevBuf<emat_site_rate_step> trace;
};

// Scratch of the tree probers (emat_probe_kernels.hpp, emat_probe_host.hpp), one set for the resident tree and for the samples of the store:
// the working room of a chunk of units, the per-unit results the summaries are made from, and `args`, everything a call brings from the
// host in one upload.  Allocated at the first call, grown on demand; released with the store, which sized the largest of it, and back
// at the next call.
struct ProbeScratch {
  DevBuf<int32_t> val, jump_a, jump_b, diff, status;
  DevBuf<unsigned long long> fix;
  DevBuf<double> counts, total, p_coalesce, p, mean, stats, root_t;
  DevBuf<uint8_t> args;   // descriptors, population tables and their knots, marks, ranks
  template <class T> static void drop(DevBuf<T>& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.n = 0; }
  size_t samples_bytes() const { return (val.n + jump_a.n + jump_b.n + diff.n + status.n) * 4 + (fix.n + counts.n + total.n + p_coalesce.n + p.n + mean.n + stats.n + root_t.n) * 8 + args.n; }
  void release_samples() { drop(val); drop(jump_a); drop(jump_b); drop(diff); drop(status); drop(fix); drop(counts); drop(total); drop(p_coalesce); drop(p); drop(mean); drop(stats); drop(root_t); drop(args); }
};

// The store of sampled trees and what emat_mcc_derive works in (emat_mcc_kernels.hpp, emat_mcc_host.hpp).  The store is sized by
// emat_tree_samples_reserve; the derivation's buffers are allocated at the first call and grown on demand.
struct MccHost {
  int32_t capacity = 0, n = 0, count = 0;             // slots, nodes of every sample, slots in use
  DevBuf<int32_t> parent, c0, c1, root; DevBuf<double> t;
  std::vector<uint8_t> is_tip;                         // of sample 0: every later sample has the same tips
  DevBuf<unsigned long long> fp, keys; DevBuf<int32_t> ntips, arrive, corr, counts, hist, info, num_exact; DevBuf<uint8_t> exact;
  DevBuf<double> support, t_out, t_mrca;
  MccTable table{}; int32_t table_regrows = 0; int table_log2_hint = 0;   // the table of clade counts of the last derivation; the size it ended with is where the next one starts
  int32_t derived_M = 0, derived_n = 0;                // the (M x n) correspondence table of the last derivation is valid
  int32_t derived_first = 0, derived_stride = 1;       // ... and belongs to the samples derived_first + k * derived_stride (emat_mcc_probe_ancestors probes those)
  int32_t derived_master = 0;                          // ... of which this one (a position, not a slot) is the master (emat_mcc_mutation_support reads its mutations)
  // Opt-in (emat_tree_samples_reserve_mutations): what a slot keeps of its mutations, for the site-state prober over samples.  Per slot
  // the per-node list headers and the reference sequence; the records of all slots in one arena, a slot's in one segment handed out
  // here on the host (mut_base / mut_len; base -1: the sample came without mutations).  The headers' offsets are relative to the segment.
  int64_t mut_capacity = 0, mut_used = 0;              // records of the arena, and how many are handed out; capacity 0: no room
  int32_t mut_L = 0, mut_slots = 0, mut_n = 0;         // sites, slots and nodes the room was made for
  DevBuf<GList> mut_hdr; DevBuf<uint8_t> mut_ref; DevBuf<MutRec> mut_arena;
  std::vector<int64_t> mut_base; std::vector<uint32_t> mut_len;
  template <class T> static void drop(DevBuf<T>& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.n = 0; }
  void release_mutations() { drop(mut_hdr); drop(mut_ref); drop(mut_arena); mut_capacity = 0; mut_used = 0; mut_L = 0; mut_slots = 0; mut_n = 0; mut_base.clear(); mut_len.clear(); }
  void release() { drop(parent); drop(c0); drop(c1); drop(root); drop(t); drop(fp); drop(keys); drop(ntips); drop(arrive); drop(corr); drop(counts); drop(hist); drop(exact); release_mutations(); capacity = 0; count = 0; derived_M = 0; table_log2_hint = 0; }
};

// What emat_mcc_node_times and emat_mcc_mutation_support work in (emat_mcc_summary_kernels.hpp, emat_mcc_summary_host.hpp): the chunk's
// (M x B) times and flags, the call's outputs and what it uploads.  Grow-only; released with the store, which sizes the largest of it.
struct MccSummaryScratch {
  DevBuf<double> x, quantiles, q_exact, q_mrca, hpd_exact, hpd_mrca, mean_t, t_min, t_max;
  DevBuf<uint8_t> e;
  DevBuf<int32_t> flags, nodes, num_exact, rec_offset, num_with;
  DevBuf<long long> seg_base; DevBuf<uint32_t> seg_len;
  template <class T> static void drop(DevBuf<T>& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.n = 0; }
  void release() { drop(x); drop(e); drop(q_exact); drop(q_mrca); drop(hpd_exact); drop(hpd_mrca); drop(num_exact); drop(nodes); drop(rec_offset); drop(num_with); drop(mean_t); drop(t_min); drop(t_max); }
};

// The alignment store and what emat_align_finish works in (emat_align_kernels.hpp, emat_align_host.hpp).  The store is sized by emat_align_begin, exactly;
// everything else is grow-only.  `attached` is the FASTA loader's record of the rows (names, dates: emat_fasta.cpp), which lives and dies with the store.
struct AlignHost {
  bool bound = false, finished = false;
  int64_t max_rows = 0, rows = 0, row_bytes = 0;
  DevBuf<uint8_t> packed, chars, ref, delta_to; DevBuf<unsigned long long> bad; DevBuf<long long> totals;
  DevBuf<int32_t> counts, tip_row, n_delta, n_iv, n_not_n, delta_off, miss_off, delta_site, miss_start, miss_end;
  PinnedBytes row_buf[2]; hipEvent_t row_ev[2] = {nullptr, nullptr}, copy_ev = nullptr; bool row_ev_pending[2] = {false, false};   // emat_align_row_buffer
  std::vector<int32_t> row_status, row_bad_site, row_not_n; std::vector<uint8_t> row_bad_byte;                                      // the last finish's, per input row
  emat_align_report report{};
  void* attached = nullptr; void (*attached_free)(void*) = nullptr;
  void drop_attached() { if (attached && attached_free) attached_free(attached); attached = nullptr; attached_free = nullptr; }
  template <class T> static void drop(DevBuf<T>& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.n = 0; b.n_grown = false; }
  void release() {
    drop(packed); drop(chars); drop(ref); drop(delta_to); drop(bad); drop(totals); drop(counts); drop(tip_row); drop(n_delta); drop(n_iv); drop(n_not_n);
    drop(delta_off); drop(miss_off); drop(delta_site); drop(miss_start); drop(miss_end);
    bound = false; finished = false; max_rows = 0; rows = 0;
  }
  ~AlignHost() { drop_attached(); for (hipEvent_t e : {row_ev[0], row_ev[1], copy_ev}) if (e) (void)hipEventDestroy(e); }
};

}  // namespace emat

using namespace emat;

struct emat_backend {
  emat_config cfg{};
  std::string last_error;
  int L = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  int num_cus = 0;
  int xcc_count = 0;                // XCDs that workgroups are dealt to round robin (probe_xcc_dealing); 0: not so, or unknown -> tickets always hand over with a full release
  // size classes: parts sorted by persistent size; class c stages up to class_lds[c] bytes per part and runs on its own stream
  static constexpr int k_max_classes = 3;
  hipStream_t class_stream[k_max_classes] = {};   // class 0 runs on `stream`; the others on streams shared by every handle of the device (side_stream)
  hipEvent_t ev_fork = nullptr, ev_join[k_max_classes] = {};
  int num_classes = 1; int class_begin[k_max_classes + 1] = {}; uint32_t class_lds[k_max_classes] = {};
  std::vector<int> class_of;        // per part
  std::vector<int64_t> expected_moves;   // per part: moves requested of it since its upload (apart from the part records: every launch adds to all of them)
  std::vector<int> cfg_class_pct{60};                // option "lds_classes" (tuning knob): percentiles of persistent size that close each class; the last
                                                     // class always extends to the largest part (its staging area is still that percentile's size)
  uint32_t cfg_lds_max = 96 * 1024;                  // option "lds_max" (tuning knob): largest staging area; larger parts run out of HBM
  bool order_valid = false;         // d_order holds the current parts, largest first
  std::vector<int32_t> h_order;     // host copy of d_order
  bool last_launch_uniform = false; // the last launch ran the same number of moves on every part (its durations are comparable)
  bool cfg_order_by_time = false;   // option "order_by_time" (tuning knob): re-sort the launch order by measured durations at every synchronisation
  std::string cfg_ticket_weights;   // option "ticket_weights": "w1,w2,..." the tickets' ratio, as many numbers as tickets
  int cfg_build_blocks = 0;         // option "build_blocks": workgroups of the initial-tree builder's launch (0 = by tree size)
  bool cfg_debug_fail_gather = false;   // option "debug_fail_gather" (testing aid): the next deferred gather of the device-resident tree reports k_gt_inconsistent
  bool cfg_tree_tight = false;      // option "tree_tight" (testing aid): the device-resident tree gets no spare room, so that the growth paths run
  unsigned cfg_fn_min_lists = 0;    // option "fn_min_lists" (profiling builds): function timers count only parts whose lists take at least this many bytes
  bool cfg_phase_extra = false;     // option "phase_extra" (profiling builds): emat_debug_phase_ticks returns the scan and arena counters
                                    // (measured at C4: 292 vs 296 M moves/s -- with two parts per slot the slot that ran the longest part
                                    // still takes one more; off by default)
  bool pass_pending = false;        // a launch has not been checked for stopped parts yet (finish_pass)
  bool sides_in_flight = false;     // side-class launches that the engine's own stream has not been made to wait for yet (join_side_classes)
  bool sides_must_fork = true;      // the side streams have not seen what the engine's stream did since the last pass was checked
  emat_status fatal_status = EMAT_OK;   // a part stopped INSIDE a move: its tree is untrustworthy, and every run / getter keeps
  std::string fatal_message;            // failing with this until the parts are uploaded afresh (emat_begin_upload)
  double last_run_ms = 0.0;
  // model
  std::vector<uint8_t> ref, partition_for_site;
  std::vector<double> nu_l, cumQ, cum_nu, mu, pi, q;
  std::vector<int32_t> ref_freqs;
  bool uniform_sites = false;       // one site partition, every nu_l == 1.0: EvoTable::uniform_sites
  bool cfg_no_uniform_sites = false;   // option "no_uniform_sites" (A/B and tests): the moves read the per-site arrays even then
  int num_partitions = 0;
  RunFlags flags{0.0, 0, 1};
  bool have_ref = false, have_evo = false, have_pop = false, have_coal = false;
  HostPopModel pop;
  DevBuf<uint8_t> d_ref, d_part; DevBuf<double> d_nu, d_cumQ, d_cum_nu, d_stats, d_mu, d_pi, d_q, d_sky_x, d_sky_g; DevBuf<int32_t> d_ref_freqs; DevBuf<PopTable> d_pop;
  bool model_dirty = true;
  // parts
  std::vector<PartHost> parts;
  int uploads_expected = 0;
  int root_part = -1;
  PinnedBytes h_slabs;
  size_t slab_bytes_total = 0;      // bytes of all slabs on the device (h_slabs is brought to this size when somebody pulls)
  DevBuf<uint8_t> d_slabs, d_snaps; DevBuf<uint64_t> d_slab_off; DevBuf<int32_t> d_order, d_part_status; DevBuf<int64_t> d_part_ticks, d_moves_for_part;
  // Which copy of the parts is current.  Written only by the transitions below, by materialize (host records -> slabs on the device)
  // and by the two pulls (pull_from_device: h_slabs and the records follow the device; pull_headers: h_headers does).
  bool slabs_on_device = false;     // device slabs are materialised
  bool host_slabs_current = false;  // h_slabs mirrors the device
  bool derived_valid = false;       // lambda_i, missing-site counts, log_G and the coalescent prior of the slabs are the moves' own (or k_recalc_derived's)
  void parts_replaced() { parts_need_encoding(false); have_coal = false; }          // new part records (emat_begin_upload, emat_tree_repartition): nothing on the device, no cell tables yet
  void parts_need_encoding(bool keep_derived) {                                     // the records changed on the host (new cell tables; more room after a stopped pass, which keeps
    slabs_on_device = false; host_slabs_current = false; headers_current = false;   // the derived values it decoded): the next materialize encodes them again
    if (!keep_derived) derived_valid = false;
  }
  void model_changed() { derived_valid = false; }                                   // reference sequence or evolution model set: what the slabs maintain belongs to the old one
  void device_wrote_slabs() { host_slabs_current = false; headers_current = false; }   // a kernel changed the slabs (moves, recalculation, an editing test hook)
  void device_recalculated() { device_wrote_slabs(); derived_valid = true; }        // ... and that kernel was k_recalc_derived
  void device_built_slabs() { slabs_on_device = true; device_wrote_slabs(); derived_valid = false; }   // the repartition kernels wrote the slabs of new parts: nothing derived in them yet
  void device_build_failed() { slabs_on_device = false; }                           // ... or stopped half way: there are no slabs
  uint32_t max_slab_bytes = 0;
  std::vector<uint32_t> persistent_bytes;   // per part: slab size without scratch
  std::vector<uint32_t> prefix_bytes;       // per part: header + nodes + cells + trace (what the prefix-staged variant keeps in LDS)
  std::vector<uint32_t> used_bytes;         // per part: prefix + list content (what a part staged whole brings into LDS)
  // SharedCells: host mirror (absolute cell index) and the device copy the kernels read
  std::vector<double> sh_ktw, sh_popsize, sh_tsop; std::vector<int32_t> sh_nact;
  bool grid_mirrors_on_device = false;   // the grid was built on the device (emat_tree_repartition) and the four vectors above have not been fetched yet
  DevBuf<double> d_sh_ktw, d_sh_tsop; DevBuf<int32_t> d_sh_nact;
  SharedCells shared_dev{nullptr, nullptr, nullptr, 0};   // what make_args hands the kernels (the HBM-resident tree points it at its own grid arrays)
  uint32_t cfg_side_arena = 1;              // option "side_arena" (tuning knob; 0 = off): a part that would be left with less arena than this in the main area joins the giants' 8-per-CU class.  The default, 1 byte, moves exactly the parts that cannot be staged WHOLE there (0.5 % at C4): with their lists in HBM they were the last chains of every pass (19.6 ms where the rest was done by 19.9: pass 21.5 -> 20.1 ms); 1-4 KB moves hundreds and loses
  bool cfg_giants = true;                   // option "giants" (tuning knob): parts that cannot even stage their prefix get a class of their own
  double cfg_heap_per_node = 64.0;  // option "heap_per_node": heap bytes per node on top of slack x content
  uint32_t cfg_lds_scratch = 0;     // option "lds_scratch" (tuning knob): per-part LDS scratch arena; 0 = all scratch in HBM (measured best at C4)
  bool host_only = false;           // cfg.device == -1: uploads / coalescent staging only, every launch fails with EMAT_ERR_NO_DEVICE
  std::unique_ptr<CoalBuilder> coal_builder;
  // dense copy of every part's slab header (k_gather_headers): what the scalar getters read instead of the slabs
  DevBuf<uint8_t> d_headers; std::vector<uint8_t> h_headers; bool headers_current = false;
  GTreeHost gt;                     // the whole tree, when it lives in HBM (emat_tree_upload)
  ProbeScratch probe;               // what emat_tree_probe_* / emat_tree_branch_counts work in
  CoalStatsScratch coal;            // the statistics the population moves read (emat_tree_coalescent_stats, or uploaded by the caller)
  SkygridScratch sky;               // what emat_skygrid_moves works in
  ExpPopScratch xp;                 // what emat_exp_pop_moves works in
  SiteRateScratch sr;               // what emat_site_rate_moves works in
  SubstStatsScratch sbs;            // the statistics the two groups below read (emat_parts_subst_stats, or uploaded by the caller)
  SubstScratch sb;                  // what emat_subst_moves works in
  MpoxScratch mx;                   // what emat_mpox_moves works in
  MccHost mcc;                      // the sampled trees kept in HBM (emat_tree_sample_*) and what emat_mcc_derive works in
  MccSummaryScratch mcs;            // what emat_mcc_node_times and emat_mcc_mutation_support work in
  AlignHost al;                     // the aligned rows kept in HBM (emat_align_*) and the tip descriptors made from them
  int cfg_mcc_summary_chunk = 0;    // "mcc_summary_chunk" (testing aid): MCC nodes emat_mcc_node_times works on at a time (0: as many as half the free memory holds)
  int cfg_samples_probe_chunk = 0;  // "samples_probe_chunk" (testing aid): samples the batched probers (emat_tree_samples_probe_ancestors, emat_tree_samples_probe_site_states) work on at a time (0: as many as half the free memory holds)
  int cfg_mcc_table_log2 = 0;       // "mcc_table_log2" (testing aid): log2 of the slots the table of clade counts starts with (0: four per node), so that its growth runs
  BuiltTree built;                  // what emat_tree_build_usher_like made, until it is fetched (emat_tree_built_get)
  bool cfg_taper = true;            // option "ticket_taper": tickets of a part shrink (10 : 6 : 3 : 1 for four tickets, else n : ... : 1) instead of being equal
  int cfg_chunks = 4;               // option "chunks" (tuning knob): tickets per part and pass (main class; measured at C4 once a ticket's release no longer wrote the L2 back, equal tickets: 2 -> 378, 3 -> 384, 6 -> 382, 10 -> 379, 16 -> 365, 32 -> 322 M moves/s; tapered: 3 -> 390, 4 -> 392, 5 -> 388; before: 1 -> 311, 2 -> 338, 3 -> 340, 4 -> 331, 8 -> 301)
  bool cfg_ticket_spread = false;   // option "ticket_xcd_spread" = 1 (tests): odd ticket stride, a part's tickets on different XCDs
  int cfg_single_ticket_parts = 0;        // option "single_ticket_parts" (tuning knob): how many of the largest main-class parts run their pass as one ticket
  bool cfg_ticket_full_release = false;   // option "ticket_release" = "full": agent-scope release at every hand-over
  bool cfg_chunks_forced = false;   // option "chunks" was given: tickets also when the parts are fewer than the wave slots (tests)
  DevBuf<int32_t> d_chunk_done, d_side_started;
  int cfg_parts_per_cu = 0;         // option "parts_per_cu" (tuning knob): workgroups of the main class per CU, instead of the percentile rule
  bool cfg_gt_host_coal = false;    // option "tree_host_coalescent" = 1: emat_tree_repartition builds the coalescent tables on the host (bit-identical to the host cycle; tests)

  void set_error(const std::string& s) { last_error = s; }
};

namespace {

emat_status fail(emat_backend* h, emat_status st, const std::string& msg) { h->set_error(msg); return st; }
emat_status no_device(emat_backend* h) { return fail(h, EMAT_ERR_NO_DEVICE, "host-only handle (device = -1): the engine has no CPU fallback"); }

// Several handles may live in one process, one per GPU: every entry point that talks to the device selects its own first.
inline bool bind_device(emat_backend* h) { return h->host_only || hipSetDevice(h->cfg.device) == hipSuccess; }

}  // namespace

#endif  // EMAT_STATE_HOST_HPP_
