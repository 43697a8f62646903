// emat_part_kernels.hpp -- the per-part kernels: the move kernels (k_run_moves, k_run_moves_side), the whole-part recomputation and
// check of the derived quantities, the getters' kernels and the test hooks' kernels, with the three compilations of the move
// headers they call into and the profiling builds' device globals.
//
// Included by emat_backend.hip, first: everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_PART_KERNELS_HPP_
#define EMAT_PART_KERNELS_HPP_

#if defined(EMAT_PROFILE_PHASES) || defined(EMAT_COUNT_CALLS)
namespace emat {
constexpr int k_fn_replicas = 64;                          // (one table per workgroup index mod 64: eight thousand waves adding to ONE word per scope made the profiling build 5.6 x slower than the real one)
__device__ unsigned long long g_fn_ticks[k_fn_replicas * 3 * 2048][2];   // EMAT_TIMED scopes: [replica][header * 2048 + line][ticks, calls], all parts
__device__ unsigned g_fn_min_list_bytes = 0;              // ... or only the parts whose lists take at least this much (EMAT_FN_MIN_LISTS: the heavy parts near the root)
__shared__ int s_fn_count_me;
struct FnTimer {   // inclusive ticks and calls of the enclosing scope, keyed by (header, source line); lane 0 only
  int key; long long t0;
  __device__ FnTimer(int k) : key(k), t0(clock64()) {}
  __device__ void stop() { if (key >= 0) { this->~FnTimer(); key = -1; } }
  __device__ ~FnTimer() { if (key >= 0 && threadIdx.x == 0 && s_fn_count_me) { const long long dt = clock64() - t0; unsigned long long* e = g_fn_ticks[(blockIdx.x & (k_fn_replicas - 1)) * (3 * 2048) + key]; atomicAdd(&e[0], (unsigned long long)dt); atomicAdd(&e[1], 1ull); } }
};
}
#endif
#ifdef EMAT_PROFILE_PHASES
namespace emat { __device__ unsigned long long g_arena_site_bytes[2048][2]; }   // [source line & 2047][0 = LDS arena, 1 = HBM scratch], all parts
#endif
// The device code is compiled three times (see emat_device_core.hpp): `dev_lds` for parts whose whole persistent slab
// is staged in LDS, `dev_mix` for larger parts of which only header + nodes + cells are staged, and `dev` for parts
// that run entirely on their HBM slab (and for k_recalc_derived).
#define EMAT_DEV_NS dev_lds
#define EMAT_VARIANT_LDS 1
#include "emat_device_moves.hpp"
#undef EMAT_DEV_NS
#undef EMAT_VARIANT_LDS
#define EMAT_DEV_NS dev_mix
#define EMAT_VARIANT_LDS 2
#include "emat_device_moves.hpp"
#undef EMAT_DEV_NS
#undef EMAT_VARIANT_LDS
#define EMAT_DEV_NS dev
#define EMAT_VARIANT_LDS 0
#include "emat_device_moves.hpp"

namespace emat {

// =================================================================================================
// Kernels
// =================================================================================================
struct KernelArgs {
  uint8_t* slabs;                 // all slabs, back to back
  const uint64_t* slab_off;       // [num_parts] byte offset of each part's slab
  const int32_t* order;           // [parts of this launch] part ids, largest first: workgroup b runs part order[b]
  int64_t* part_ticks;            // [2][num_parts] wall-clock ticks and start tick of each part's last run (occupancy timelines)
  const int32_t* ref_freqs;       // [P][4]
  const double* cum_nu;           // [L + 1][P][4]: nu-weighted counts of reference states per site partition over sites < k (k_global_stats)
  double* stats_out;              // [num_parts][k_stats_row]: per-part output of k_global_stats
  EvoTable evo;
  const PopTable* pop;
  SharedCells shared;             // the run-wide coalescent cell arrays (every part but the root part reads them here)
  RunFlags flags;
  int32_t num_parts;
  uint32_t lds_slab_bytes;        // capacity of the LDS staging area (0 = never stage)
  uint32_t lds_scratch_bytes;     // size of the per-part LDS scratch arena
  int64_t moves_per_part;
  const int64_t* moves_for_part;  // [num_parts] or null: per-part counts of a recovery launch (overrides moves_per_part / extra_moves_part0)
  int32_t* part_status;           // [num_parts] status every part ended its chain with (0 = ran to completion)
  int64_t extra_moves_part0;      // remainder of Run::run_local_moves goes to part 0 (run.cpp:683-689)
  int32_t one_more_below;         // parts [0, one_more_below) do one move more (emat_run_moves_even)
  // A pass cut into `chunks` tickets per part (EMAT_CHUNKS): workgroup b runs ticket b / class_stride of part order[b % class_stride];
  // ticket c of a part starts when ticket c - 1 has written the slab back (chunk_done[part] == c).  Shorter tickets pack the
  // slots better at the end of a pass; the chain -- one RNG stream per part, state in the slab -- is the same chain.
  int32_t chunks, class_count, class_stride, taper;
  int32_t* side_started;          // side classes of a synchronised pass: every workgroup counts itself in as it starts (k_wait_side_start), else nullptr
  int32_t single_below;           // the first `single_below` slots of the launch order (the parts expected to run longest) do their whole pass in ONE ticket, from the start of the pass: longest jobs first and unsplit, the many short chains -- in tickets -- fill in around them
  int32_t full_release;           // EMAT_TICKET_RELEASE=full: every ticket hands its part over with an agent-scope RELEASE (the path that needs no assumption about where workgroups run)
  int32_t cum_w[8];               // cumulative ticket weights (EMAT_TICKET_WEIGHTS) or zeros
  int32_t* chunk_done;            // [num_parts], zeroed before the launch
  // Room for a copy of every slab's persistent prefix, at the slab's own offset: a leg that runs on the HBM slab itself (part
  // not staged whole) saves it there first, so that a container overflowing INSIDE a move can be answered by putting the
  // leg's starting state back and asking the host for more room, as for a staged leg (which never touches the HBM copy).
  uint8_t* snaps;
};

constexpr int k_wave = 64;
constexpr int k_ticket_log = 8;   // tickets per part whose workgroup entry / exit ticks are kept (emat_debug_ticket_ticks)

__device__ inline void wave_copy16(uint8_t* dst, const uint8_t* src, uint32_t bytes, int lane) {
  const uint4* s = (const uint4*)src; uint4* d = (uint4*)dst;
  for (uint32_t i = lane; i < bytes / 16; i += k_wave) d[i] = s[i];
}
// The same copy with stores that are written through to where every XCD sees them (agent-scope atomics, 8 bytes each): what a
// ticket hands to the next one goes out this way, so that handing over needs no write-back of the XCD's whole L2 (below).
__device__ inline void wave_copy8_through(uint8_t* dst, const uint8_t* src, uint32_t bytes, int lane) {
  const uint64_t* s = (const uint64_t*)src; uint64_t* d = (uint64_t*)dst;
  for (uint32_t i = lane; i < bytes / 8; i += k_wave) __hip_atomic_store(&d[i], s[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double wave_sum(double x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, k_wave);
  return __shfl(x, 0, k_wave);
}

// Fills the model pointers of a context; HKY tables come from LDS when they were staged.
// `slab` = where slab offsets resolve for the generic code variant (the HBM slab); the LDS variants address header, nodes and
// lists through compile-time LDS addresses and only need `H` here, to pick up the RNG position and flags.
template <class CtxT> __device__ inline void init_ctx(CtxT& c, uint8_t* slab, uint8_t* gslab, const KernelArgs& a, const double* lds_tables, SlabHeader* H = nullptr) {
  c.S = slab; c.G = gslab; c.H = H != nullptr ? H : (SlabHeader*)slab; c.N = (NodeRec*)(slab + c.H->off_nodes);
  c.L = a.evo.num_sites;
  c.ref = (const __attribute__((address_space(1))) uint8_t*)a.evo.ref_sequence; c.part = (const __attribute__((address_space(1))) uint8_t*)a.evo.partition_for_site;
  c.nu = (const __attribute__((address_space(1))) double*)a.evo.nu_l; c.cumQ = (const __attribute__((address_space(1))) double*)a.evo.cum_Q_l;
  c.have_logq = lds_tables != nullptr;
  c.uniform_sites = a.evo.uniform_sites != 0;
  if (lds_tables) { c.mu = lds_tables; c.pi = lds_tables + k_max_lds_partitions; c.q = lds_tables + k_max_lds_partitions * 5; }
  else { c.mu = a.evo.mu; c.pi = a.evo.pi; c.q = a.evo.q; }
  c.pop = a.pop;
  c.sh_ktw = a.shared.k_twiddle_bar; c.sh_tsop = a.shared.ts_over_pop; c.sh_nact = a.shared.num_active_parts;
  c.t_max_tip = a.flags.t_max_tip;
  c.only_displacing_inner_nodes = a.flags.only_displacing_inner_nodes != 0;
  c.topology_moves_enabled = a.flags.topology_moves_enabled != 0;
  c.includes_run_root = (c.H->flags & k_flag_includes_run_root) != 0;
  rng_enter_leg(c, *c.H);   // (nothing computed ahead yet: the chain's first step asks the wave for it)
  c.phase = 0; c.svc = 0; c.frame = nullptr;
  c.mu_prop = 0.0; c.sc_top = c.H->scratch_begin; c.A = nullptr; c.a_top = 0; c.a_end = 0; c.failed = false; c.bytes = 0; c.bytes_w = 0;
  c.tr_kind = -1; c.tr_node = -1; c.tr_acc = -1; c.tr_log_mh = 0.0; c.heap_limit = 0; c.mix_total = 0.0;   // (the last two: dev::begin_leg, once the leg has set the heap's end)
}
__device__ inline const double* stage_tables(const KernelArgs& a, double* lds_tables, int lane) {
  if (a.evo.num_partitions > k_max_lds_partitions) return nullptr;
  const int P = a.evo.num_partitions;
  for (int i = lane; i < P; i += k_wave) lds_tables[i] = a.evo.mu[i];
  for (int i = lane; i < P * 4; i += k_wave) lds_tables[k_max_lds_partitions + i] = a.evo.pi[i];
  for (int i = lane; i < P * 16; i += k_wave) lds_tables[k_max_lds_partitions * 5 + i] = a.evo.q[i];
  for (int i = lane; i < P * 16; i += k_wave) { const double arg = a.evo.mu[i / 16] * 1.0 * a.evo.q[i]; emat_lds_logq[i] = arg > 0.0 ? dev::m_log(arg) : 0.0; }   // (the diagonal is never asked for)
  return lds_tables;
}

// ---- the hot path: `moves` sub-iterations on every part -------------------------------------------------
// One wavefront (= one workgroup) per part.  Every part is its own Markov chain with its own RNG stream, so the
// launch schedule does not change any result.  The chain itself is serial and runs on lane 0; all 64 lanes move the
// slab between HBM and LDS.  LDS layout: static [HKY tables], static [context], dynamic [staged slab][optional scratch arena]; all
// first three sit at compile-time offsets, which is what lets the `dev_lds` variant address them with DS instructions.
#ifndef EMAT_WAVES_PER_EU
#define EMAT_WAVES_PER_EU 4
#endif
// Every kernel that calls into the out-of-line device functions carries the same occupancy target: the register budget
// of a callee is the tightest one among its callers' targets only if ALL its callers have one (the debug kernels share
// `dev::` code with k_run_moves).  HIP's __launch_bounds__ second argument is ignored by the AMDGPU backend.
#define EMAT_OCCUPANCY __attribute__((amdgpu_waves_per_eu(EMAT_WAVES_PER_EU, EMAT_WAVES_PER_EU)))
// Room the list heap of an LDS-staged part keeps above its used size (measured at C4: 2048 -> 288, 1024 -> 296, 768 -> 287,
// 512 -> 282 M moves/s: less room leaves more LDS to the moves' scratch arena, too little sends parts through heap
// compactions and the HBM fall-back leg).
constexpr uint32_t k_lds_heap_room = 1024;

// Which XCD (accelerator complex) this wavefront runs on: hardware register XCC_ID (id 20, bits 3:0).  The eight XCDs of an
// MI355X have an L2 each, and what a ticket hands to its successor through write-through stores is only guaranteed to be seen by a
// successor behind the SAME L2 (a cross-XCD hand-over through that path was caught reading a stale slab by
// tests/test_parity_gpu.py::test_tickets_handed_over_across_xcds..., about once in twenty passes): the cheap hand-over is therefore
// only taken when the launch puts a part's tickets on one XCD -- checked, not assumed: the host verifies once per device how
// workgroups are dealt to XCDs (k_probe_xcc), and every ticket checks that its predecessor ran where it runs itself.
__device__ __forceinline__ int xcc_id() { return (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11)) & 15u); }
__global__ void k_probe_xcc(int32_t* out) { if (threadIdx.x == 0) out[blockIdx.x] = xcc_id(); }

template <bool kSide> __device__ __forceinline__ void run_moves_body(const KernelArgs& a) {
  const int lane = threadIdx.x;
  if (kSide && a.side_started != nullptr && lane == 0) __hip_atomic_fetch_add(a.side_started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // resident: the main class may come
  double* lds_tables = (double*)emat_lds_tables;
  const bool tables_staged = stage_tables(a, lds_tables, lane) != nullptr;
  uint8_t* lds_slab = emat_lds;
  int* lds_flag = (int*)(emat_lds_ctx + k_lds_ctx_bytes - 16);   // spare tail of the context slot: lane 0 -> all lanes
  const int chunk = a.chunks > 1 ? (int)blockIdx.x / a.class_stride : 0, slot = a.chunks > 1 ? (int)blockIdx.x % a.class_stride : (int)blockIdx.x;
  if (a.chunks > 1 && slot >= a.class_count) return;   // padding: the stride is a multiple of 8 so that a part's tickets land on one XCD
  const bool single = a.chunks > 1 && slot < a.single_below;   // this part's pass is one ticket: its later tickets have nothing to do
  if (single && chunk > 0) return;
  const int part = a.order[slot];
  // Per-part words that one ticket of a part writes and the next reads (status, chain ticks): agent-scope atomics, which every
  // XCD sees without a cache write-back.
  if (lane == 0 && chunk < k_ticket_log) a.part_ticks[(size_t)(2 + 2 * chunk) * a.num_parts + part] = (int64_t)wall_clock64();   // the workgroup is resident from here ...
  auto st_status = [&](int32_t v) { __hip_atomic_store(&a.part_status[part], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto ld_status = [&]() -> int32_t { return __hip_atomic_load(&a.part_status[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto st_ticks = [&](int64_t v) { __hip_atomic_store(&a.part_ticks[part], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto ld_ticks = [&]() -> int64_t { return __hip_atomic_load(&a.part_ticks[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  uint8_t* gslab = a.slabs + a.slab_off[part];
  SlabHeader* gh = (SlabHeader*)gslab;
#if !defined(EMAT_PROFILE_PHASES) && !defined(EMAT_COUNT_CALLS)
  // the staged variants address the dynamic LDS block at a constant (k_lds_dyn_base, emat_device_core.hpp; the profiling and
  // call-counting builds take the symbol instead): is it where they think it is?
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)emat_lds != k_lds_dyn_base) {
    if (lane == 0) { gh->fail_line = -3; st_status(k_part_internal); if (a.chunks > 1) __hip_atomic_store(&a.chunk_done[part], a.chunks, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
    return;
  }
#endif
  const int64_t pass_target = a.moves_for_part ? a.moves_for_part[part] : a.moves_per_part + (part == 0 ? a.extra_moves_part0 : 0) + (part < a.one_more_below ? 1 : 0);
  int64_t target = pass_target, done_at_start;
  if (a.chunks > 1) {
    if (chunk > 0) {   // the ticket before this one must have written the part's slab back
      // (workgroups are dispatched in index order, so that ticket is running or done: the wait cannot deadlock; it is
      // bounded all the same, and a part whose turn never came is reported, not waited for)
      if (lane == 0) {
        // (bounded by wall-clock time -- two minutes of the 100 MHz counter -- not by a number of polls: a forced ticket count on a
        // handful of huge parts that run out of HBM makes the earlier tickets of a part take seconds, found by the fuzz rounds)
        const uint64_t w0 = wall_clock64();
        bool waited = false, gave_up = false;
        int32_t seen;
        while (((seen = __hip_atomic_load(&a.chunk_done[part], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) & 0xff) < chunk) {
          __builtin_amdgcn_s_sleep(64); waited = true;
          if (wall_clock64() - w0 > 12000000000ull) { gave_up = true; break; }
        }
        // the predecessor handed the part over without writing its L2 back: it must have run behind this very L2
        if (!gave_up && (seen & 0x100) != 0 && ((seen >> 12) & 15) != xcc_id()) { gave_up = true; gh->fail_line = k_fail_line_other_xcd; }
        if (waited) atomicAdd((unsigned long long*)&a.chunk_done[((a.num_parts + 1) & ~1) + 2 * (blockIdx.x & 63)], (unsigned long long)(wall_clock64() - w0));   // (EMAT_VERBOSE: slot time spent waiting)
        // (a ticket that gives up says so to its successors as well: they would each wait out their own two minutes -- ADVICE round 4)
        if (gave_up) { st_status(k_part_internal); __hip_atomic_store(&a.chunk_done[part], a.chunks, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); *lds_flag = -1; } else *lds_flag = 0;
      }
      __syncthreads();
      if (*lds_flag == -1) return;
    } else if (lane == 0) __hip_atomic_store(&gh->pad0, (uint32_t)gh->moves_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // where the pass picked the part up (low bits: a pass is far shorter than 2^32 moves); written through like everything else a later ticket reads
    __syncthreads();
    // cumulative over the tickets so far.  The tickets of a part shrink in the ratio n : n-1 : ... : 1, so that the jobs that start
    // last -- the ones a pass ends with -- are the shortest (equal tickets: EMAT_TICKET_TAPER=0)
    if (single) target = pass_target;
    else if (a.cum_w[0] > 0) target = chunk + 1 == a.chunks ? pass_target : pass_target * a.cum_w[chunk] / a.cum_w[a.chunks - 1];   // a table of weights (the default for four tickets, or EMAT_TICKET_WEIGHTS="w1,w2,...")
    else if (a.taper) { const int64_t nn = a.chunks, done_w = (int64_t)(chunk + 1) * (2 * nn - chunk), all_w = nn * (nn + 1); target = chunk + 1 == a.chunks ? pass_target : pass_target * done_w / all_w; }
    else target = pass_target * (chunk + 1) / a.chunks;
    done_at_start = gh->moves_done - (int64_t)(uint32_t)((uint32_t)gh->moves_done - gh->pad0);
  } else done_at_start = gh->moves_done;
  const uint32_t area = a.lds_slab_bytes;
#if defined(EMAT_PROFILE_PHASES) || defined(EMAT_COUNT_CALLS)
  if (lane == 0) s_fn_count_me = (gh->heap_top - gh->heap_begin) >= g_fn_min_list_bytes ? 1 : 0;
#endif
  const bool can_stage = tables_staged && area != 0 && gh->off_nodes == (uint32_t)sizeof(SlabHeader);
  if (lane == 0 && chunk == 0) { st_ticks(0); a.part_ticks[a.num_parts + part] = (int64_t)wall_clock64(); }   // duration, start (emat_debug_part_ticks)
  // Up to two legs: a part whose USED state fits the staging area but whose heap capacity does not is staged whole with
  // an LDS-local heap limit; should its lists outgrow that, it is written back and finishes with its heap in HBM.
  bool allow_whole = true;
  bool plain_hbm_writes = false;   // some leg of this ticket changed the part's state in HBM with ordinary (cached) stores
  for (int leg = 0; leg < 2; ++leg) {
    __syncthreads();
    const uint32_t hbm_heap_end = gh->heap_end;
    uint32_t lds_heap_end = 0;
    if (can_stage && allow_whole) {
      // the list heap keeps k_lds_heap_room bytes to grow into (or its whole capacity, if smaller); what is left of the
      // area is the moves' LDS scratch arena -- without one, every temporary of an SPR move is an HBM round trip
      const uint32_t want = (gh->heap_top + k_lds_heap_room + 15u) & ~15u;
      if (hbm_heap_end <= area) lds_heap_end = hbm_heap_end < want ? hbm_heap_end : want;
      else if (want <= area) lds_heap_end = want;
    }
    const bool staged = lds_heap_end != 0;
    if (!staged) plain_hbm_writes = true;   // this leg edits lists (or everything) in the HBM slab itself, with ordinary stores
    const bool prefix = can_stage && !staged && gh->heap_begin <= area;
    // stage the persistent state (header, nodes, cells, trace, list heap) -- or, for a part too large for that, its
    // fixed-size prefix up to the list heap; scratch always stays in HBM
    const uint32_t staged_bytes = staged ? gh->heap_top : (prefix ? gh->heap_begin : 0u);
    if (staged_bytes) { wave_copy16(emat_lds_hdr, gslab, (uint32_t)sizeof(SlabHeader), lane); wave_copy16(lds_slab, gslab + sizeof(SlabHeader), staged_bytes - (uint32_t)sizeof(SlabHeader), lane); }
    // a leg that works on the HBM slab itself keeps a copy of what it found (header, nodes, cells, trace, lists in use)
    uint8_t* const snap = (!staged && a.snaps != nullptr) ? a.snaps + a.slab_off[part] : nullptr;
    if (snap != nullptr) wave_copy16(snap, gslab, (gh->heap_top + 15u) & ~15u, lane);
    __syncthreads();
    SlabHeader* const lds_hdr = (SlabHeader*)emat_lds_hdr;
    SlabHeader* H = (staged || prefix) ? lds_hdr : gh;
    // The root part is one chain like any other, but its moves walk long runs of coalescent cells (deep branches span
    // hundreds of cells): compute-bound, the longest chain of its launch.  Let its wave win issue arbitration on its SIMD.
    // (So are the parts of the side classes -- the giants of a partition, a few dozen among thousands: at the reference's
    // rule every part does the same number of moves, theirs cost two or three times a small part's, and the pass waits for them.)
    const bool raise_prio = kSide || (gh->flags & k_flag_includes_run_root) != 0;
    uint64_t tick0 = 0;
    if (lane == 0) {
      // The context lives in LDS, not in private memory: it is touched by almost every instruction.
      if (staged) {
        dev_lds::Ctx& c = *(dev_lds::Ctx*)(emat_lds_ctx);
        init_ctx(c, gslab, gslab, a, lds_tables, lds_hdr);
        H->heap_end = lds_heap_end;
        dev_lds::begin_leg(c);
        // whatever the part leaves unused of the staging area (plus the optional extra arena) serves as the first-level
        // scratch arena of its moves; scratch that does not fit goes to the part's HBM scratch region as before
        const uint32_t used = (lds_heap_end + 15u) & ~15u;
        c.A = lds_slab + (used - (uint32_t)sizeof(SlabHeader)); c.a_end = area + a.lds_scratch_bytes - used;
      } else if (prefix) {
        // the prefix leaves the rest of the staging area free: the moves' first-level arena, as for a staged part (before
        // round 2's end these parts -- 40-60 nodes, the slowest chains of a pass -- ran every candidate scan through HBM)
        dev_mix::Ctx& c = *(dev_mix::Ctx*)(emat_lds_ctx);
        init_ctx(c, gslab, gslab, a, lds_tables, lds_hdr);
        dev_mix::begin_leg(c);
        const uint32_t used = (gh->heap_begin + 15u) & ~15u;
        c.A = lds_slab + (used - (uint32_t)sizeof(SlabHeader)); c.a_end = area + a.lds_scratch_bytes - used;
      } else {
        dev::Ctx& c = *(dev::Ctx*)(emat_lds_ctx);
        init_ctx(c, gslab, gslab, a, tables_staged ? lds_tables : nullptr);
        dev::begin_leg(c);
        if (area + a.lds_scratch_bytes > (uint32_t)sizeof(SlabHeader)) { c.A = lds_slab; c.a_end = area + a.lds_scratch_bytes - (uint32_t)sizeof(SlabHeader); }   // nothing of the part is staged: the whole dynamic block is arena
      }
      // (a later ticket of a part whose earlier one had to stop does nothing: the host gives the part more room and the rest of its moves)
      const bool stopped_before = chunk > 0 && ld_status() != 0;
      ((dev::Ctx*)(emat_lds_ctx))->moves_left = (H->status == 0 && !stopped_before) ? target - (H->moves_done - done_at_start) : 0;   // the three Ctx types share one layout
      tick0 = wall_clock64();
      if (raise_prio) __builtin_amdgcn_s_setprio(3);
    }
    __syncthreads();
    // The chain: stretches of moves on lane 0; whenever a move parks itself for work the whole wave shares (the candidate
    // scan and study of an SPR move), all 64 lanes do that work and lane 0 picks the move up again.
    for (;;) {
      if (lane == 0) {
        if (staged) dev_lds::run_chain_loop(*(dev_lds::Ctx*)(emat_lds_ctx));
        else if (prefix) dev_mix::run_chain_loop(*(dev_mix::Ctx*)(emat_lds_ctx));
        else dev::run_chain_loop(*(dev::Ctx*)(emat_lds_ctx));
      }
      __syncthreads();
      const int svc = ((const dev::Ctx*)(emat_lds_ctx))->svc;
      if (svc == 0) break;
      if (svc == 2) dev::rng_fill(*(dev::Ctx*)(emat_lds_ctx), lane);      // (the three Ctx types share one layout)
      else if (staged) dev_lds::wave_scan_and_study(*(dev_lds::Ctx*)(emat_lds_ctx));
      else if (prefix) dev_mix::wave_scan_and_study(*(dev_mix::Ctx*)(emat_lds_ctx));
      else dev::wave_scan_and_study(*(dev::Ctx*)(emat_lds_ctx));
      __syncthreads();
    }
    if (lane == 0) {
      if (raise_prio) __builtin_amdgcn_s_setprio(0);
      const dev::Ctx& c = *(const dev::Ctx*)(emat_lds_ctx);
      dev::rng_leave_leg(c, *H);
      H->alg_bytes += c.bytes; H->alg_write16 += (uint32_t)((c.bytes_w + 8) >> 4);
      const int64_t dt = (int64_t)(wall_clock64() - tick0);
      H->device_ticks += dt;
      st_ticks(ld_ticks() + dt);
      if (!(chunk > 0 && ld_status() != 0)) st_status(H->status);   // an idle ticket leaves the earlier ticket's verdict alone
      int again = 0;
      if (staged) {
        H->heap_end = hbm_heap_end;
        if (H->status == k_part_need_space && lds_heap_end < hbm_heap_end && H->heap_top <= hbm_heap_end) { H->status = 0; st_status(0); again = 1; }
        // A list outgrew the LDS-local heap limit INSIDE a move: the staged state is lost, but nothing of this leg has
        // reached the HBM copy of the slab yet (moves only write HBM scratch), and the chain is a deterministic function
        // of that copy.  Drop the LDS state and run the leg again from HBM with the heap at its full capacity there.
        else if (H->status == k_part_overflow && lds_heap_end < hbm_heap_end) { st_status(0); again = 2; }
        // The root part's coalescent grid outgrew its capacity (the root wandered further into the past than the room the
        // host left): the same argument -- the HBM copy still is the consistent state this launch found -- lets the
        // host re-materialise the part with more cells and run its moves again (first leg only: a second leg follows a
        // write-back).
        else if (H->status == k_part_cell_overflow && leg == 0) { st_status(k_part_need_cells); again = 3; }
        // Anything else that overflowed inside a move of a staged leg (the heap at its full capacity, the scratch region):
        // the HBM copy is the leg's starting state just the same -- more room from the host, and the moves again.
        else if (H->status == k_part_overflow) { st_status(k_part_need_space); again = 3; }
      } else if (snap != nullptr && (H->status == k_part_overflow || H->status == k_part_cell_overflow)) {
        // the leg ran on the HBM slab: its starting state goes back in from the copy taken above
        st_status(H->status == k_part_cell_overflow ? k_part_need_cells : k_part_need_space); again = 4;
      }
      *lds_flag = again;
    }
    __syncthreads();
    const int again_all = *lds_flag;
    if (again_all < 2) {
      const uint32_t out_bytes = staged ? ((const SlabHeader*)emat_lds_hdr)->heap_top : (prefix ? staged_bytes : 0u);
      if (out_bytes && a.chunks > 1 && !single) { wave_copy8_through(gslab, emat_lds_hdr, (uint32_t)sizeof(SlabHeader), lane); wave_copy8_through(gslab + sizeof(SlabHeader), lds_slab, out_bytes - (uint32_t)sizeof(SlabHeader), lane); }
      else if (out_bytes) { wave_copy16(gslab, emat_lds_hdr, (uint32_t)sizeof(SlabHeader), lane); wave_copy16(gslab + sizeof(SlabHeader), lds_slab, out_bytes - (uint32_t)sizeof(SlabHeader), lane); }
    }
    if (again_all == 4) { wave_copy16(gslab, snap, (((const SlabHeader*)snap)->heap_top + 15u) & ~15u, lane); break; }
    if (again_all == 0 || again_all == 3) break;
    allow_whole = false;
  }
  if (lane == 0 && chunk < k_ticket_log) a.part_ticks[(size_t)(3 + 2 * chunk) * a.num_parts + part] = (int64_t)wall_clock64();   // ... to here
  if (a.chunks > 1 && !single) {   // hand the part to its next ticket: the slab is in HBM again
    __syncthreads();
    // An agent-scope release writes back every dirty line of this XCD's L2 -- among them the private-memory lines of the 500
    // other chains resident there -- once per ticket: half of a pass's HBM write traffic.  A ticket whose
    // part was staged has sent everything the next ticket reads through write-through stores (the slab image, status, ticks):
    // it only waits for those to be acknowledged.  One that edited lists in HBM directly keeps the full release.
    if (lane == 0) {
      if (plain_hbm_writes || a.full_release) __hip_atomic_store(&a.chunk_done[part], chunk + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_waitcnt(0); __hip_atomic_store(&a.chunk_done[part], (chunk + 1) | 0x100 | (xcc_id() << 12), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
  }
}
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY EMAT_NOTAIL k_run_moves(KernelArgs a) { run_moves_body<false>(a); }
// Same body under another name for the side launches of the size classes (the "giants", §4 of DESIGN.md), so that
// profiles keep the statistics of the main launch -- the one bench.py's roofline is about -- apart.
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY EMAT_NOTAIL k_run_moves_side(KernelArgs a) { run_moves_body<true>(a); }
// A side class holds a few workgroups of tens of KB of LDS each -- the root part's wants most of a CU -- and the main class 30 000 of
// ten KB: once the main class is on the device a large workgroup only fits when a CU happens to drain, which is at the tail of the
// pass.  Launch order alone does not settle who is placed first (two streams, two queues: a race the side classes lost in one process
// in three, rocprofv3 --kernel-trace: root part's kernel 27 ms instead of 9 in the first pass); and a side class that starts at the
// tail of a pass ends in the next one, starts again at ITS tail, and so on: every later pass of that process carries the lag, which the
// final synchronisation then waits for (0.9 ms per pass over ten passes -- the 400-against-418 M moves/s coin flip of rounds 3 and 4).
// So on a synchronised pass the engine's stream holds the main class back until every side workgroup has reported itself resident:
// microseconds on an idle device, and bounded (2 ms of the 100 MHz counter) in case something else holds the CUs.
__global__ void k_wait_side_start(const int32_t* started, int32_t expected) {
  if (threadIdx.x != 0) return;
  const uint64_t w0 = wall_clock64();
  while (__hip_atomic_load(started, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expected && wall_clock64() - w0 < 200000ull) __builtin_amdgcn_s_sleep(8);
}

// ---- sufficient statistics of the global moves (calc_Ttwiddle_beta_a phylo_tree_calc.cpp:288-369, calc_num_muts_beta_ab
//      :599-610, calc_num_muts :577-585), one part per workgroup ---------------------------------------------------------
// n^beta_a(node) = nu-weighted number of sites of partition beta present in state a at the node.  Its change across a
// branch comes from the branch's missation intervals (two gathers into a prefix table over the reference sequence
// instead of the reference's site-by-site loop), from_states and mutations: lane-parallel over the nodes.  The
// values themselves follow from a pre-order accumulation (lane 0), and the statistics are sums over the non-root
// branches, again lane-parallel, reduced across lanes in a fixed order so that the result is reproducible.
constexpr int k_max_stats_partitions = 4;
constexpr int k_stats_row = k_max_stats_partitions * (4 + 16) + 1;   // Ttwiddle[P][4], num_muts[P][4][4], num_muts
__global__ void __launch_bounds__(k_wave) k_global_stats(KernelArgs a) {
  __shared__ double sh_T[k_wave][k_max_stats_partitions * 4];
  __shared__ int sh_M[k_wave][k_max_stats_partitions * 16];
  const int lane = threadIdx.x;
  const int part = blockIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  dev::Ctx c;
  init_ctx(c, slab, slab, a, nullptr);
  const int P = a.evo.num_partitions, W = 4 * P;
  const int n = c.H->n_nodes, root = c.H->root;
  double* D = (double*)(slab + c.H->scratch_begin);   // [n][W]: per-branch change, then the value at the node
  // phase A: change of n^beta_a across every branch
  for (int i = lane; i < n; i += k_wave) {
    double* d = D + (size_t)i * W;
    for (int k = 0; k < W; ++k) d[k] = 0.0;
    const IvRec* iv = dev::miss_of(c, i);
    for (int j = 0; j < (int)c.N[i].miss.cnt; ++j) {
      const double* hi = a.cum_nu + (size_t)iv[j].end * W; const double* lo = a.cum_nu + (size_t)iv[j].start * W;
      for (int k = 0; k < W; ++k) d[k] -= hi[k] - lo[k];
    }
    const FsRec* fs = dev::mfs_of(c, i);
    for (int j = 0; j < (int)c.N[i].mfs.cnt; ++j) { const int l = fs[j].site, b = c.part[l]; d[4 * b + c.ref[l]] += c.nu[l]; d[4 * b + fs[j].state] -= c.nu[l]; }
    const MutRec* m = dev::muts_of(c, i);
    for (int j = 0; j < dev::nmuts(c, i); ++j) { const int l = m[j].site, b = c.part[l]; d[4 * b + m[j].from] -= c.nu[l]; d[4 * b + m[j].to] += c.nu[l]; }
  }
  __syncthreads();
  // phase B: pre-order accumulation from the reference sequence's counts (the last row of the prefix table)
  if (lane == 0) {
    const double* ref_row = a.cum_nu + (size_t)c.L * W;
    for (int k = 0; k < W; ++k) D[(size_t)root * W + k] += ref_row[k];
    int cur = root;
    while (cur != dev::k_no_node) {
      if (!dev::is_tip(c, cur)) {
        for (int kk = 0; kk < 2; ++kk) {
          const int ch = kk == 0 ? c.N[cur].child0 : c.N[cur].child1;
          for (int k = 0; k < W; ++k) D[(size_t)ch * W + k] += D[(size_t)cur * W + k];
        }
        cur = c.N[cur].child0;
      } else {
        int prev = cur; cur = c.N[cur].parent;
        while (cur != dev::k_no_node && c.N[cur].child1 == prev) { prev = cur; cur = c.N[cur].parent; }
        if (cur != dev::k_no_node) cur = c.N[cur].child1;
      }
    }
  }
  __syncthreads();
  // phase C: sums over the non-root branches
  for (int k = 0; k < W; ++k) sh_T[lane][k] = 0.0;
  for (int k = 0; k < 4 * W; ++k) sh_M[lane][k] = 0;
  for (int i = lane; i < n; i += k_wave) {
    if (i == root) continue;   // "mutations" above the root are deltas from the reference sequence
    const double t_P = c.N[c.N[i].parent].t, len = c.N[i].t - t_P;
    const double* d = D + (size_t)i * W;
    for (int k = 0; k < W; ++k) sh_T[lane][k] += d[k] * len;
    const MutRec* m = dev::muts_of(c, i);
    for (int j = dev::nmuts(c, i) - 1; j >= 0; --j) {
      const int l = m[j].site, b = c.part[l];
      sh_T[lane][4 * b + m[j].to] -= c.nu[l] * (m[j].t - t_P);
      sh_T[lane][4 * b + m[j].from] += c.nu[l] * (m[j].t - t_P);
      sh_M[lane][16 * b + 4 * m[j].from + m[j].to] += 1;
    }
  }
  __syncthreads();
  double* out = a.stats_out + (size_t)part * k_stats_row;
  for (int k = lane; k < W; k += k_wave) { double sum = 0.0; for (int r = 0; r < k_wave; ++r) sum += sh_T[r][k]; out[k] = sum; }
  for (int k = lane; k < 4 * W; k += k_wave) { long long sum = 0; for (int r = 0; r < k_wave; ++r) sum += sh_M[r][k]; out[k_max_stats_partitions * 4 + k] = (double)sum; }
  if (lane == 0) {
    long long nm = 0;
    for (int k = 0; k < 4 * W; ++k) for (int r = 0; r < k_wave; ++r) nm += sh_M[r][k];
    out[k_stats_row - 1] = (double)nm;
  }
}

// ---- whole-part derived quantities (Subrun::recalc_derived_quantities, subrun.cpp:17-26) ---------------------
// Lanes stride over the part's nodes: branch-local work (delta lambda across the branch, missing-site count,
// branch log-G, log N(t)) is embarrassingly parallel; only the pre-order accumulation of lambda_i /
// n_missing down the tree is a dependent chain, walked by lane 0 without a stack.
// kCheck = true is the reference's check_derived_quantities (subrun.cpp:28-56; forced in release builds by --v0-paranoid,
// run.h:220-224): the same recomputation, but into the part's scratch region, compared with what the moves maintained
// incrementally, and reported per part in check_out[part][4] = {max |d lambda_i| / L, |d log_G|, |d log prior|, number of
// nodes whose missing-site count differs}; the slab itself is left as it is.
template <bool kCheck> __device__ __forceinline__ void recalc_derived_body(const KernelArgs& a, double* check_out) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int lane = threadIdx.x;
  const int part = blockIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  const int n = c.H->n_nodes, root = c.H->root;
  // where the recomputed per-node values go: the node records themselves, or (check) two arrays in the scratch region
  double* lam_of = kCheck ? (double*)(slab + c.H->scratch_begin) : nullptr;
  int32_t* nmiss_of = kCheck ? (int32_t*)(slab + c.H->scratch_begin + (size_t)n * 8u) : nullptr;
  auto LAM = [&](int i) -> double& { return kCheck ? lam_of[i] : c.N[i].lambda; };
  auto NMISS = [&](int i) -> int32_t& { return kCheck ? nmiss_of[i] : c.N[i].n_missing; };
  // phase A: per-branch deltas
  for (int i = lane; i < n; i += k_wave) {
    // <false>: without the nodes' remembered values -- the check must leave the slab as it is, and the recalculation forgets them below
    LAM(i) = dev::delta_lambda_across_branch<false>(c, i);
    NMISS(i) = dev::iv_num_sites(dev::miss_of(c, i), (int)c.N[i].miss.cnt);
    // what the moves remembered of the nodes' missation rate changes (emat_slab.hpp) may belong to another model or reference sequence
    if (!kCheck) dev::miss_dl_forget(c, i);
  }
  __syncthreads();
  // phase B: pre-order prefix (phylo_tree_calc.cpp:420-436, :67-76)
  if (lane == 0) {
    int cur = root;
    LAM(root) = c.cumQ[c.L] + LAM(root);
    while (cur != dev::k_no_node) {
      if (!dev::is_tip(c, cur)) {
        for (int k = 0; k < 2; ++k) {
          int ch = k == 0 ? c.N[cur].child0 : c.N[cur].child1;
          LAM(ch) = LAM(cur) + LAM(ch);
          NMISS(ch) = NMISS(cur) + NMISS(ch);
        }
        cur = c.N[cur].child0;
      } else {
        // climb until we arrive from a first child, then step to its sibling
        int prev = cur; cur = c.N[cur].parent;
        while (cur != dev::k_no_node && c.N[cur].child1 == prev) { prev = cur; cur = c.N[cur].parent; }
        if (cur != dev::k_no_node) cur = c.N[cur].child1;
      }
    }
  }
  __syncthreads();
  // phase C: log G and the coalescent partial prior
  double acc_G = 0.0, acc_prior = 0.0;
  for (int i = lane; i < n; i += k_wave) {
    if (i != root) acc_G += dev::branch_log_G(c, c.N[c.N[i].parent].t, c.N[i].t, LAM(i), dev::muts_of(c, i), dev::nmuts(c, i));
    if (!dev::is_tip(c, i)) acc_prior -= log(dev::pop_at_time(*c.pop, c.N[i].t));
  }
  {
    // (lanes take different cells here: the shared arrays are read with ordinary loads, not through the scalar cache)
    const int cap = c.H->cell_cap, first = c.H->cell_first;
    const double* base = (const double*)(slab + c.H->off_cells);
    const double* kbar_p = base; const double* ktw_p = base + cap;
    for (int w = lane; w < c.H->n_cells; w += k_wave) {   // very_scalable_coalescent.cpp:355-386
      double na, tsop, ktw;
      if (c.includes_run_root) { na = (double)((const int32_t*)(base + 5 * cap))[w]; tsop = base[4 * cap + w]; ktw = base[2 * cap + w]; }
      else { na = (double)a.shared.num_active_parts[first + w]; tsop = a.shared.ts_over_pop[first + w]; ktw = a.shared.k_twiddle_bar[first + w]; }
      acc_prior -= tsop * (+0.5 * (kbar_p[w] * kbar_p[w]) * na - (ktw_p[w] * na - ktw + 0.5) * kbar_p[w]);
    }
  }
  acc_G = wave_sum(acc_G); acc_prior = wave_sum(acc_prior);
  double dev_lambda = 0.0; int bad_missing = 0;
  if (kCheck) {
    for (int i = lane; i < n; i += k_wave) {
      const double dl = fabs(c.N[i].lambda - lam_of[i]) / (double)c.L;
      if (!(dl <= dev_lambda)) dev_lambda = dl;                     // (a NaN on either side shows as NaN)
      if (c.N[i].n_missing != nmiss_of[i]) ++bad_missing;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(dev_lambda, off, k_wave); if (!(o <= dev_lambda)) dev_lambda = o;
      bad_missing += __shfl_down(bad_missing, off, k_wave);
    }
  }
  if (lane == 0) {
    double lg = acc_G;
    if (c.includes_run_root) lg = dev::calc_log_root_prior(c, a.ref_freqs, a.evo.num_partitions) + acc_G;
    if (kCheck) {
      double* o = check_out + 4 * (size_t)part;
      o[0] = dev_lambda; o[1] = fabs(c.H->log_G - lg); o[2] = fabs(c.H->log_aug_prior - acc_prior); o[3] = (double)bad_missing;
      if (c.H->log_G == lg) o[1] = 0.0;                             // (-inf on both sides is agreement)
    } else {
      c.H->log_G = lg;
      c.H->log_aug_prior = acc_prior;
    }
  }
}
__global__ void __launch_bounds__(k_wave) k_recalc_derived(KernelArgs a) { recalc_derived_body<false>(a, nullptr); }
__global__ void __launch_bounds__(k_wave) k_check_derived(KernelArgs a, double* check_out) { recalc_derived_body<true>(a, check_out); }
// test hook (emat_debug_miss_dl_check): the remembered missation rate change of every node (emat_slab.hpp) against a fresh evaluation
// of the same function on the node's lists as they stand.  out[2 part] = entries that are known and differ from it in bits,
// out[2 part + 1] = entries that are known.
__global__ void __launch_bounds__(k_wave) k_debug_miss_dl_check(KernelArgs a, int32_t* out) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int lane = threadIdx.x;
  const int part = blockIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  int bad = 0, known = 0;
  for (int i = lane; i < c.H->n_nodes; i += k_wave) {
    const uint64_t bits = dev::miss_dl_of(c)[i];
    if (bits == k_miss_dl_unknown) continue;
    ++known;
    if (bits != (uint64_t)__double_as_longlong(dev::delta_lambda_across_node_missations_fresh(c, i))) ++bad;
  }
  for (int off = 32; off > 0; off >>= 1) { bad += __shfl_down(bad, off, k_wave); known += __shfl_down(known, off, k_wave); }
  if (lane == 0) { out[2 * part] = bad; out[2 * part + 1] = known; }
}
// test hook (emat_debug_tree_query): the moves' own find_MRCA_of / descends_from on one part's slab, query by query
__global__ void __launch_bounds__(k_wave) k_debug_tree_query(KernelArgs a, int part, int op, const int32_t* qa, const int32_t* qb, int32_t* out, int n) {
  if (threadIdx.x != 0) return;
  uint8_t* slab = a.slabs + a.slab_off[part];
  dev::Ctx c;
  init_ctx(c, slab, slab, a, nullptr);
  for (int i = 0; i < n; ++i) out[i] = op == 0 ? dev::find_MRCA_of(c, qa[i], qb[i]) : (dev::descends_from(c, qa[i], qb[i]) ? 1 : 0);
}

// test hook (emat_debug_graft): the moves' own graft analysis, peel, re-attachment, proposal and apply on one part's slab, on
// lane 0 as inside a chain, with everything the analysis found written out as numbers (layout: emat_backend.h).
struct GraftOut { double* p; int cap; int n; };
__device__ inline void go_put(GraftOut& o, double v) { if (o.n < o.cap) o.p[o.n] = v; ++o.n; }
__device__ inline void go_graft(GraftOut& o, const dev::Graft& g) {
  go_put(o, (double)g.nbi); go_put(o, g.delta_log_G); go_put(o, g.log_alpha_mut); go_put(o, (double)g.X); go_put(o, (double)g.S); go_put(o, g.t_P);
  for (int i = 0; i < g.nbi; ++i) {
    const dev::BranchInfo& b = g.bi[i];
    go_put(o, (double)b.A); go_put(o, (double)b.B); go_put(o, b.is_open ? 1.0 : 0.0); go_put(o, b.T_to_X); go_put(o, b.pl_A); go_put(o, b.pl_X);
    go_put(o, (double)b.warm.n); for (int k = 0; k < b.warm.n; ++k) { go_put(o, (double)b.warm.p[k].start); go_put(o, (double)b.warm.p[k].end); }
    go_put(o, (double)b.hot.n); for (int k = 0; k < b.hot.n; ++k) { go_put(o, (double)b.hot.p[k].start); go_put(o, (double)b.hot.p[k].end); }
    go_put(o, (double)b.hot_muts.n); for (int k = 0; k < b.hot_muts.n; ++k) { const MutRec& m = b.hot_muts.p[k]; go_put(o, (double)m.site); go_put(o, (double)m.from); go_put(o, (double)m.to); go_put(o, m.t); }
    go_put(o, (double)b.hot_deltas.n); for (int k = 0; k < b.hot_deltas.n; ++k) { const dev::SdRec& d = b.hot_deltas.p[k]; go_put(o, (double)d.site); go_put(o, (double)d.from); go_put(o, (double)d.to); }
  }
}
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY k_debug_graft(KernelArgs a, int part, int X, double mu_proposal, int mode, int new_S, double new_t_P, double* out, int out_cap, int32_t* out_len) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  if (lane != 0) return;
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  dev::sc_reset(c);
  c.mu_prop = mu_proposal;
  GraftOut o; o.p = out; o.cap = out_cap; o.n = 0;
  go_put(o, 0.0);                                   // [0]: the part's status afterwards
  go_put(o, mode == 3 ? 2.0 : 1.0);                 // [1]: grafts written out
  dev::Graft* g = (dev::Graft*)dev::sc_alloc(c, (uint32_t)(2 * sizeof(dev::Graft)));
  if (!c.failed) {
    dev::analyze_graft(c, X, g[0]);                 // Spr_move::analyze_graft (spr_move.cpp:9-36)
    if (!c.failed) go_graft(o, g[0]);
    if (mode >= 1 && !c.failed) {
      dev::peel_graft(c, g[0]);                     // Spr_move::peel_graft (:38-62)
      if (!c.failed) {
        go_put(o, (double)dev::count_min_mutations(c, g[0]));                      // count_min_mutations (spr_move.cpp:64-71)
        { int closed = 0; if (g[0].rooty) closed = g[0].bi[dev::k_SPX].hot_muts.n; else for (int i = 0; i < g[0].nbi; ++i) if (!g[0].bi[i].is_open) closed += g[0].bi[i].hot_muts.n;
          go_put(o, (double)closed); }                                             // count_closed_mutations (:73-89; not needed by a move)
        const dev::SVec<dev::SdRec> d = dev::summarize_closed_mutations(c, g[0], 0);      // summarize_closed_mutations (:1126-1156)
        go_put(o, (double)d.n); for (int k = 0; k < d.n; ++k) { go_put(o, (double)d.p[k].site); go_put(o, (double)d.p[k].from); go_put(o, (double)d.p[k].to); }
      }
    }
    if (mode == 2 && !c.failed) dev::apply_graft(c, g[0]);                         // Spr_move::apply_graft (:64-89)
    if (mode == 3 && !c.failed) {
      // the middle of an SPR move without its candidate study (subrun.cpp:580-640): re-attach at (new_S, new_t_P), propose the new
      // graft's mutations from the part's random stream, apply them, and account for the change of log G as an accepted move does
      dev::spr_move_topology(c, X, new_S, new_t_P);                                // Spr_move::move (spr_move.cpp:1071-1099)
      if (!c.failed) dev::propose_new_graft(c, X, g[1]);
      if (!c.failed) { go_graft(o, g[1]); dev::apply_graft(c, g[1]); }
      if (!c.failed) { c.H->log_G -= g[0].delta_log_G; c.H->log_G += g[1].delta_log_G; }
    }
  }
  dev::rng_leave_leg(c, *c.H);
  out[0] = (double)(c.failed ? (c.H->status != 0 ? c.H->status : k_part_internal) : 0);
  *out_len = o.n;
}

// test hook (emat_debug_sample_history): the proposal's JC69 history sampler, history by history, as the reference's own statistical
// test drives it (tests/spr_move_tests.cpp:1795-1961): for history i the path ends at (branch[i], t_end[i]); the deltas are where
// `start_seq` differs from the tree's sequence there; sample_mutational_history + adjust_mutational_history; every mutation written out.
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY k_debug_sample_history(KernelArgs a, int part, int n, const int32_t* branch, const double* t_end, const uint8_t* start_seq,
                                                                                double T, double mu, int32_t* counts, double* muts, int muts_cap, int32_t* status) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  if (lane != 0) return;
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  int written = 0;
  for (int i = 0; i < n && !c.failed; ++i) {
    dev::sc_reset(c);
    dev::SVec<dev::SdRec> deltas = dev::sc_vec<dev::SdRec>(c, c.L + 1);
    for (int l = 0; l < c.L && !c.failed; ++l) { const int e = dev::calc_site_state_at(c, branch[i], t_end[i], l); if (e != (int)start_seq[l]) dev::sd_push_back(c, deltas, l, (int)start_seq[l], e); }
    if (c.failed) break;
    dev::SVec<MutRec> h = dev::sample_mutational_history(c, c.L, T, mu, deltas);
    if (c.failed) break;
    dev::adjust_mutational_history(c, h, deltas, branch[i], t_end[i]);
    counts[i] = h.n;
    for (int k = 0; k < h.n; ++k, ++written) if (written < muts_cap) { double* o = muts + 4 * (size_t)written; o[0] = (double)h.p[k].site; o[1] = (double)h.p[k].from; o[2] = (double)h.p[k].to; o[3] = h.p[k].t; }
  }
  dev::rng_leave_leg(c, *c.H);
  status[0] = c.failed ? (c.H->status != 0 ? c.H->status : k_part_internal) : 0;
  status[1] = written;
}

// test hook (emat_debug_edit): one tree-editing session on node X of one part's slab, step by step as the caller lists them
// (Tree_editing_session, reference tree_editing.cpp:7-302): 0 slide_P_along_branch(t), 1 hop_up, 2 flip, 3 hop_down(node); then end().
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY k_debug_edit(KernelArgs a, int part, int X, int n_ops, const int32_t* op_kind, const int32_t* op_node, const double* op_t, int32_t* status) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  if (lane != 0) return;
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  dev::sc_reset(c);
  dev::Edit e;
  int cap = 8;
  for (int i = 0; i < c.H->n_nodes; ++i) cap += dev::nmuts(c, i);
  dev::edit_begin(c, e, X, cap);
  for (int i = 0; i < n_ops && !c.failed; ++i) {
    if (op_kind[i] == 0) dev::edit_slide_P_along_branch(c, e, op_t[i]);
    else if (op_kind[i] == 1) dev::edit_do_hop_up(c, X);
    else if (op_kind[i] == 2) dev::edit_flip(c, e);
    else dev::edit_hop_down(c, e, op_node[i]);
  }
  dev::edit_end(c, e);
  status[0] = c.failed ? (c.H->status != 0 ? c.H->status : k_part_internal) : 0;
}

// ---- compact copies of what the host reads most often, so that it does not have to download the slabs for them ----------
// Every part's 256-byte header (status, counters, log_G, log prior, RNG position) into one dense array.
__global__ void __launch_bounds__(k_wave) k_gather_headers(KernelArgs a, uint8_t* out) {
  const int part = blockIdx.x, lane = threadIdx.x;
  const uint4* src = (const uint4*)(a.slabs + a.slab_off[part]);
  uint4* dst = (uint4*)(out + (size_t)part * sizeof(SlabHeader));
  for (int i = lane; i < (int)(sizeof(SlabHeader) / 16); i += k_wave) dst[i] = src[i];
}

// calc_num_muts_l (phylo_tree_calc.cpp:612-622): mutations per site over the non-root branches of every part (integer
// atomics: the result does not depend on the order).
__global__ void __launch_bounds__(k_wave) k_num_muts_l(KernelArgs a, int32_t* out) {
  const int part = blockIdx.x, lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  dev::Ctx c;
  init_ctx(c, slab, slab, a, nullptr);
  const int n = c.H->n_nodes, root = c.H->root;
  for (int i = lane; i < n; i += k_wave) {
    if (i == root) continue;   // "mutations" above a part's root are deltas from the reference sequence
    const MutRec* m = dev::muts_of(c, i);
    for (int j = 0; j < dev::nmuts(c, i); ++j) atomicAdd(&out[m[j].site], 1);
  }
}

// ---- calc_Ttwiddle_l (phylo_tree_calc.cpp:176-222) over a partitioned tree ----------------------------------------------
// The reference starts every site at q_ref T_total and corrects it per mutation / missation with the branch length BELOW
// that point -- a quantity that crosses part boundaries.  A part gets, for every tip that is the cut node of a part below
// it, the total branch length hanging there (`ext`; the run driver computes it from k_part_lengths' sums and the tree of
// parts); with that its nodes' "length below" follow from one post-order pass, and the corrections are local again:
//   S[site]   += (q_to - q_from) T_below(mutation)                      and  (q_ref - q_from) T_below(branch) per from_state
//   D[start]  += T_below(branch),  D[end] -= T_below(branch)            per missing interval (the host's prefix sum over D
//                                                                       is R[l], and Ttwiddle_l = q_ref (T_total - R) + S)
// A part's root is skipped unless it is the run's root: a cut node's own branch belongs to the part above it.
__global__ void __launch_bounds__(k_wave) k_part_lengths(KernelArgs a, double* out) {
  const int part = blockIdx.x, lane = threadIdx.x;
  const uint8_t* slab = a.slabs + a.slab_off[part];
  const SlabHeader* H = (const SlabHeader*)slab; const NodeRec* N = (const NodeRec*)(slab + H->off_nodes);
  double acc = 0.0;
  for (int i = lane; i < H->n_nodes; i += k_wave) if (i != H->root) acc += N[i].t - N[N[i].parent].t;
  acc = wave_sum(acc);
  if (lane == 0) out[part] = acc;
}
__global__ void __launch_bounds__(k_wave) k_ttwiddle_l(KernelArgs a, const int32_t* ext_off, const int32_t* ext_node, const double* ext_val, double* S, double* D, double* t_root_out) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int part = blockIdx.x, lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  const int n = c.H->n_nodes, root = c.H->root;
  double* Tw = (double*)(slab + c.H->scratch_begin);   // [n]: total branch length of the WHOLE tree below each node
  for (int i = lane; i < n; i += k_wave) Tw[i] = 0.0;
  __syncthreads();
  for (int k = ext_off[part] + lane; k < ext_off[part + 1]; k += k_wave) Tw[ext_node[k]] = ext_val[k];
  __syncthreads();
  if (lane == 0) {   // children before parents, without a stack
    int cur = root, from = dev::k_no_node;   // `from`: the node we arrived from (parent on the way down, a child on the way up)
    while (cur != dev::k_no_node) {
      const int par = c.N[cur].parent;
      int next;
      if (from == par && !dev::is_tip(c, cur)) next = c.N[cur].child0;
      else if (!dev::is_tip(c, cur) && from == c.N[cur].child0) next = c.N[cur].child1;
      else {   // a tip, or both children done: the node is complete
        if (cur != root) Tw[par] += (c.N[cur].t - c.N[par].t) + Tw[cur];
        next = cur == root ? dev::k_no_node : par;
      }
      from = cur; cur = next;
    }
    if (c.includes_run_root && t_root_out) *t_root_out = Tw[root];
  }
  __syncthreads();
  for (int i = lane; i < n; i += k_wave) {
    if (i == root && !c.includes_run_root) continue;
    const bool top = i == root;
    const double t_i = c.N[i].t, below = Tw[i];
    const MutRec* m = dev::muts_of(c, i);
    for (int j = 0; j < dev::nmuts(c, i); ++j) {
      const int l = m[j].site;
      const double T_below_mut = below + (top ? 0.0 : t_i - m[j].t);
      atomicAdd(&S[l], (dev::q_a(c, l, m[j].to) - dev::q_a(c, l, m[j].from)) * T_below_mut);
    }
    const double T_below_miss = below + (top ? 0.0 : t_i - c.N[c.N[i].parent].t);
    const IvRec* iv = dev::miss_of(c, i);
    for (int j = 0; j < (int)c.N[i].miss.cnt; ++j) { atomicAdd(&D[iv[j].start], T_below_miss); atomicAdd(&D[iv[j].end], -T_below_miss); }
    const FsRec* fs = dev::mfs_of(c, i);
    for (int j = 0; j < (int)c.N[i].mfs.cnt; ++j) { const int l = fs[j].site; atomicAdd(&S[l], (dev::q_a(c, l, c.ref[l]) - dev::q_a(c, l, fs[j].state)) * T_below_miss); }
  }
}

// ---- Scalable_coalescent_prior (scalable_coalescent.cpp:88-138, 163-187), one part per workgroup ----------------------
// The whole-tree grid prior is -sum_cells dt kbar (kbar - 1) / (2 Nbar) - sum_inner log N(t), where kbar_j, the mean number
// of lineages in cell j = [t_ref + j dt, t_ref + (j + 1) dt), j < 0, is 1 (the lineage above the root) plus, for every
// coalescence at t_i, the overlap of [t_i, t_ref] with the cell, minus the same for every tip.  That sum is additive over
// nodes, hence over parts: a cut node is the root of the part below it (counted there, as the coalescence it is) and a
// frozen tip of the part above it (which cannot tell it from a real tip and subtracts it), so the part below adds it once
// more.  With that, a part without the run's root contributes exactly nothing outside the cells its own nodes span, and
// the root part a constant -1 after them.  Lanes take cells; every lane walks the part's nodes in index order, so the
// partial sums are reproducible.  meta[part] = {first cell, number of cells, sum over inner nodes of -log N(t), status}.
__global__ void __launch_bounds__(k_wave) k_scalable_prior(KernelArgs a, double t_ref, double t_step, const uint64_t* out_off, const uint32_t* out_cap, double* out, double* meta) {
  __shared__ __attribute__((aligned(16))) double lds_tables[k_lds_tables_bytes / 8];
  const int part = blockIdx.x, lane = threadIdx.x;
  uint8_t* slab = a.slabs + a.slab_off[part];
  const double* tables = stage_tables(a, lds_tables, lane);
  __syncthreads();
  dev::Ctx c;
  init_ctx(c, slab, slab, a, tables);
  const int n = c.H->n_nodes, root = c.H->root;
  const bool root_part = c.includes_run_root;
  double tmin = dev::k_inf, tmax = -dev::k_inf, acc = 0.0;
  for (int i = lane; i < n; i += k_wave) {
    const double t = c.N[i].t;
    tmin = tmin < t ? tmin : t; tmax = tmax > t ? tmax : t;
    if (!dev::is_tip(c, i)) acc -= log(dev::pop_at_time(*c.pop, t));
  }
  for (int off = 32; off > 0; off >>= 1) { double o = __shfl_down(tmin, off, k_wave); tmin = tmin < o ? tmin : o; o = __shfl_down(tmax, off, k_wave); tmax = tmax > o ? tmax : o; }
  tmin = __shfl(tmin, 0, k_wave); tmax = __shfl(tmax, 0, k_wave);
  acc = wave_sum(acc);
  auto cell_of = [&](double t) { return (int)floor((t - t_ref) / t_step); };
  const int jlo = cell_of(tmin);
  int jhi = cell_of(tmax); if (jhi > -1) jhi = -1;   // cell 0 and later: no lineage of the tree lives after t_ref
  const int cnt = jhi >= jlo ? jhi - jlo + 1 : 0;
  double* row = out + out_off[part];
  const bool fits = (uint32_t)cnt <= out_cap[part];
  if (fits) {
    for (int j = jlo + lane; j <= jhi; j += k_wave) {
      const double ub_j = t_ref + (double)(j + 1) * t_step;
      double sum = 0.0;
      for (int i = 0; i < n; ++i) {
        const double t = c.N[i].t;
        const int cs = cell_of(t);
        if (j < cs) continue;
        double w = dev::is_tip(c, i) ? -1.0 : +1.0;
        if (i == root && !root_part) w += 1.0;
        sum += (j == cs) ? w * (ub_j - t) / t_step : w;   // add_interval: partial first cell, whole cells after it (:100-115)
      }
      row[j - jlo] = sum;
    }
  }
  if (lane == 0) { double* m = meta + (size_t)part * 4; m[0] = (double)jlo; m[1] = (double)cnt; m[2] = acc; m[3] = fits ? 0.0 : 1.0; }
}

// ---- test hook: the device's incomplete-gamma routines evaluated point by point (emat_debug_gamma) ----------------------
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY k_debug_gamma(const double* a, const double* x, double* out, int n, int mode) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = mode == 0 ? dev::gamma_q(a[i], x[i]) : dev::gamma_q_inv(a[i], x[i]);
}

// ---- test hooks: the device's population-model and interval-set routines on plain inputs (emat_debug_pop, _interval_op) --
__global__ void __launch_bounds__(k_wave) EMAT_OCCUPANCY k_debug_pop(PopTable pt, int op, const double* a, const double* b, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = op == 0 ? dev::pop_at_time(pt, a[i]) : op == 1 ? dev::pop_integral(pt, a[i], b[i]) : dev::pop_intensity_integral(pt, a[i], b[i]);
}
__global__ void k_debug_interval_op(int op, const IvRec* A, int nA, const IvRec* B, int nB, int site, IvRec* out, int* n_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (op == 1) *n_out = dev::iv_merge(out, A, nA, B, nB);
  else if (op == 2) *n_out = dev::iv_intersect(out, A, nA, B, nB);
  else if (op == 3) *n_out = dev::iv_subtract(out, A, nA, B, nB);
  else if (op == 5) *n_out = dev::iv_contains(A, nA, site) ? 1 : 0;
  else if (op == 6) *n_out = dev::iv_intersects(A, nA, B, nB) ? 1 : 0;
  else if (op == 7 || op == 8) {   // iv_split: 7 = its difference, 8 = its remainder (`out` holds two lists of nA + nB + 1)
    IvRec* rest = out + nA + nB + 1; int nd = 0, nr = 0;
    dev::iv_split(out, nd, rest, nr, A, nA, B, nB);
    if (op == 8) for (int k = 0; k < nr; ++k) out[k] = rest[k];
    *n_out = op == 7 ? nd : nr;
  }
  else *n_out = -1;
}

}  // namespace emat

#endif  // EMAT_PART_KERNELS_HPP_
