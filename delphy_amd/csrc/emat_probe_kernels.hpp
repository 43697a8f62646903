// emat_probe_kernels.hpp -- the tree probers: where, over time, a fresh lineage would coalesce.  ONE kernel family for trees in the slots
// of a store (emat_mcc_kernels.hpp) and for the tree resident in HBM, which is a store of capacity 1: slot 0, its segment of the
// mutation arena the used part of the tree's own heap.  A single-tree call is the batched call with one unit.
//
// Reference: probe_ancestors_on_tree (core/ancestral_tree_prober.cpp), probe_site_states_on_tree (core/site_states_tree_prober.cpp),
// both through Tree_prober (core/tree_prober.h) on a Staircase_family of branch counts (core/staircase.{h,cpp}: add_boxcar,
// add_trapezoid); over the base trees of an MCC tree as tools/delphy_wasm.cpp:1809-1849 runs them.  The UNIT of work is a tree and, in
// the site-state form, a site of it: one ProbeUnit each (unit-major: sample k, entry i of the sites is unit k * num_sites + i), with
// the unit's own grid, slot, population model and where the root's state comes from.  Every step is a launch over (units of a chunk x
// nodes) or (units x members x cells) whose count does not depend on the number of units:
//
// 0. Roots (store only): the chosen samples' root times, one copy to the host, which makes every unit's grid (emat_probe_host.hpp:
//    probe_extend_grid).  The resident tree's root time is on the host already.
// 1. A label for every node: the member (closest marked ancestor, or state of the site) its branch starts in.  Both probers ask the
//    same question -- the nearest FLAGGED node at or above a node's parent -- where the reference carries the answer down a recursion.
//    Here: pointer doubling over the parent array.  `val[v]` >= 0 flags v and is what it hands to the branches below it (the root is
//    always flagged); jump[v] starts as v for a flagged node and parent[v] otherwise, and every round replaces jump[v] by jump[jump[v]]
//    (two buffers, so a round reads only the previous round's values and the result does not depend on scheduling).  After
//    ceil(log2 n) rounds every jump[v] is the nearest flagged node at or above v, and the label of v's branch is val[jump[parent[v]]].
//    Chosen over the depth / visiting order the partitioner's kernels have because those walk PARTS serially, one thread per part:
//    there are no parts here.  Cost: 18 rounds of two 4-byte accesses per node at 200 000 nodes.  Marks come from a host array -- one
//    for all units or one per unit -- or through the correspondence table of the last derivation (first entry wins: atomicMin).
// 2. Branch counts, one thread per (unit, branch).  A cell a boxcar of height 1 covers whole gets +1 through a per-member difference
//    array (int32, one prefix sum at the end: exact).  Every other contribution -- the two end cells of a boxcar, every cell of a
//    trapezoid -- is a fraction in [0, 1] and is added in 64-BIT FIXED POINT with integer atomics, so the sum is the same bits
//    whatever order the branches arrive in.  Quantum 2^-f, f = min(52, 61 - ceil(log2(n + 1))) for a tree of n nodes (52 up to 511
//    nodes, 43 at 200 000): a cell receives fewer than n whole units and fewer than n fractions of at most 1 + 2^-50 each, so
//    |sum| < 2 n 2^f (1 + 2^-50) <= 2^62 fits an int64.  Each term is rounded to the quantum once (error <= 2^-(f+1)); the cell's
//    total, whole part shifted in, is converted to double once.
// 3. Tree_prober's recurrence: per (unit, cell) the total over members, summed in member order as the reference does, and the
//    probability of coalescing in the cell with the unit's PopTable; then per (unit, member) the chain over cells.
// 4. Summaries of the per-unit results [count][values], values = (sites x) members x cells: the mean, one thread per value adding the
//    samples in sample order and dividing once; order statistics, one workgroup per value, which brings the count values into LDS,
//    sorts them with a bitonic network padded with +inf (exact: only compares and swaps) and writes the ranks asked for.
//
// A chunk is B units; unit j of a chunk owns val / jump [j n], fix / counts [j members stride], diff [j members (stride + 1)] and
// total / p_coalesce [j stride], stride = the largest cell count of any unit, and inside its region a unit uses its OWN compact layout
// (member * num_cells + cell), which is what probe_add_frac addresses.  Nothing depends on B.
//
// Where the reference is undefined these kernels and tests/prober_model.py choose the same, stated thing: a cell index that
// rounding puts outside [0, cells) is clamped (the reference asserts), and a boxcar or trapezoid whose last cell comes out
// BEFORE its first (both ends within rounding of one cell boundary; the reference would run off its array) is entered as if
// both ends lay in the first.
//
// Cross-workgroup accumulation is by integer atomics only.  Bounds: a link or root outside [0, n) is never followed and sets the
// sample's status word, as does a branch that ends before it starts (the reference throws) and a mutation list that leaves its
// segment, which is not read; no loop runs without a bound it checks.  The sort's LDS is dynamic shared memory sized by the launch:
// the library's static LDS objects keep their fixed addresses.
//
// Included by emat_backend.hip after emat_gtree_kernels.hpp (GList, MutRec, wave_incl_scan_u32), ahead of emat_mcc_kernels.hpp: the
// family knows trees in slots (ProbeTrees), not the store.
#ifndef EMAT_PROBE_KERNELS_HPP_
#define EMAT_PROBE_KERNELS_HPP_

namespace emat {

struct ProbeGrid {                   // the Staircase_family of branch counts (staircase.h:21-52)
  double x_start, cell_size, x_end;  // x_end = x_start + num_cells * cell_size, as Staircase::x_end() computes it
  int32_t num_cells;                 // the cells the caller asked for plus the ones prepended to reach the root (cells_to_skip)
  int32_t frac_bits;                 // f above
  double scale, inv_scale;           // 2^f, 2^-f
};

__device__ inline int probe_clamp_cell(const ProbeGrid& g, int c) { return c < 0 ? 0 : (c >= g.num_cells ? g.num_cells - 1 : c); }
// cell_for_lbound / cell_for_ubound / cell_lbound (staircase.h:70-88)
__device__ inline int probe_cell_for_lbound(const ProbeGrid& g, double x) { return probe_clamp_cell(g, (int)floor((x - g.x_start) / g.cell_size)); }
__device__ inline int probe_cell_for_ubound(const ProbeGrid& g, double x) { return probe_clamp_cell(g, g.num_cells - 1 - (int)floor((g.x_end - x) / g.cell_size)); }
__device__ inline double probe_cell_lbound(const ProbeGrid& g, int cell) { return g.x_start + cell * g.cell_size; }

__device__ inline void probe_add_frac(const ProbeGrid& g, unsigned long long* fix, int member, int cell, double v) {
  const long long q = __double2ll_rn(v * g.scale);   // (the product is exact: a power of two)
  if (q != 0) atomicAdd(&fix[(size_t)member * g.num_cells + cell], (unsigned long long)q);
}
// add_boxcar(staircase, left, right, 1.0) (staircase.cpp:5-40)
__device__ inline void probe_add_boxcar(const ProbeGrid& g, unsigned long long* fix, int32_t* diff, int member, double left, double right) {
  if (left > g.x_end || right < g.x_start) return;
  left = left < g.x_start ? g.x_start : left;
  right = g.x_end < right ? g.x_end : right;
  if (left == right) return;
  const int cs = probe_cell_for_lbound(g, left), ce = probe_cell_for_ubound(g, right);
  if (ce <= cs) { probe_add_frac(g, fix, member, cs, (right - left) / g.cell_size); return; }
  probe_add_frac(g, fix, member, cs, ((probe_cell_lbound(g, cs) + g.cell_size) - left) / g.cell_size);
  probe_add_frac(g, fix, member, ce, (right - probe_cell_lbound(g, ce)) / g.cell_size);
  if (ce > cs + 1) {   // the cells in between, whole: +1 on [cs + 1, ce)
    int32_t* d = diff + (size_t)member * (g.num_cells + 1);
    atomicAdd(&d[cs + 1], 1); atomicAdd(&d[ce], -1);
  }
}
// add_trapezoid (staircase.cpp:42-100)
__device__ inline void probe_add_trapezoid(const ProbeGrid& g, unsigned long long* fix, int member, double left, double right, double left_height, double right_height) {
  const double m = (right_height - left_height) / (right - left);
  const double c = left_height - m * left;
  if (left > g.x_end || right < g.x_start) return;
  if (left < g.x_start) { left = g.x_start; left_height = m * left + c; }
  if (right > g.x_end) { right = g.x_end; right_height = m * right + c; }
  if (left == right) return;
  const int cs = probe_cell_for_lbound(g, left), ce = probe_cell_for_ubound(g, right);
  if (ce <= cs) { probe_add_frac(g, fix, member, cs, 0.5 * (left_height + right_height) * (right - left) / g.cell_size); return; }
  const double first_ubound = probe_cell_lbound(g, cs) + g.cell_size;
  probe_add_frac(g, fix, member, cs, 0.5 * ((m * left + c) + (m * first_ubound + c)) * (first_ubound - left) / g.cell_size);
  const double last_lbound = probe_cell_lbound(g, ce);
  probe_add_frac(g, fix, member, ce, 0.5 * ((m * last_lbound + c) + (m * right + c)) * (right - last_lbound) / g.cell_size);
  double lb = first_ubound;
  for (int cell = cs + 1; cell < ce; ++cell) {
    const double ub = lb + g.cell_size;
    probe_add_frac(g, fix, member, cell, 0.5 * ((m * lb + c) + (m * ub + c)));
    lb = ub;
  }
}


struct ProbeTrees {                  // trees in slots, slot-major: the store's, or the resident tree as slot 0 of a store of one
  const int32_t* parent;             // [slots * n]
  const double* t;                   // [slots * n]
  const int32_t* root;               // [slots]
  const GList* lists;                // [slots * n] per-node mutation lists: records [off, off + cnt) of the unit's segment (site-state form)
  const MutRec* recs;                // the segments of all slots
  const uint8_t* ref;                // [slots * L] the sequence a slot's root starts from; not read by a unit that brings its ref_state
  int32_t n, L;
};
struct ProbeUnit {                   // one unit: where its tree is, its grid, its population model; in the site-state form its site
  ProbeGrid grid;
  int32_t slot;
  int32_t cells_to_skip;
  int32_t pop;                       // index into the PopTable array
  int32_t ref_state;                 // the state the root starts from (the resident tree: the host's sequence is the current one), or -1: ref[slot][site]
  int32_t sample;                    // whose status word: the unit's sample, status [count]
  int32_t site;
  uint32_t seg_len, pad;             // the slot's segment: recs [seg_base, seg_base + seg_len)
  long long seg_base;
};
struct ProbeChunk {                  // the units [k0, k0 + B) of a call and the layout of their working room
  const ProbeUnit* units;            // [count (x sites)]
  int32_t k0, B, n, num_members;
  int32_t stride_cells, pad;
};
enum ProbeStatus : int32_t { k_probe_ok = 0, k_probe_negative_branch = 1, k_probe_bad_link = 2, k_probe_bad_list = 4 };
constexpr int k_probe_sort_max = 4096;        // samples the order statistics hold: 32 KB of LDS for a workgroup
constexpr int k_probe_sort_threads = 256;

// ---- step 0 -----------------------------------------------------------------------------------------------------------------------
// The root times of the slots first + k * stride, k < M.  root_t [M]; status [M] zeroed before the launch.
__global__ void __launch_bounds__(256) k_probe_roots(ProbeTrees T, int32_t first, int32_t stride, int32_t M, double* root_t, int32_t* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const int32_t slot = first + k * stride;
  const int32_t r = T.root[slot];
  if ((uint32_t)r >= (uint32_t)T.n) { atomicOr(&status[k], (int32_t)k_probe_bad_link); root_t[k] = 0.0; return; }
  root_t[k] = T.t[(size_t)slot * T.n + r];
}

// ---- step 1 -----------------------------------------------------------------------------------------------------------------------
// Ancestors: val [B * n] was filled with -1; marked node i gets the smallest index it appears under (std::ranges::find: the first wins).
// `marks` [num_marked] (marks_stride 0) or [count][num_marked] (marks_stride num_marked); with `corr` ([count][n], the last
// derivation's table) a mark is an MCC node and stands for the sample's corresponding node.
__global__ void __launch_bounds__(256) k_probe_marks(ProbeChunk C, const int32_t* marks, int num_marked, int marks_stride, const int32_t* corr, int32_t* val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_marked) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const size_t k = (size_t)(C.k0 + j);
    int32_t v = marks[k * marks_stride + i];
    if (corr && v >= 0 && v < C.n) v = corr[k * C.n + v];
    if (v >= 0 && v < C.n) atomicMin((unsigned int*)&val[(size_t)j * C.n + v], (unsigned int)i);   // (-1 is the largest unsigned value)
  }
}
// Site states: val[v] = the state the first mutation of the unit's site on v's branch leads to, -1 when there is none; the root hands
// down the state of the reference sequence, changed by every mutation of the site on its own list (site_states_tree_prober.cpp:73-79).
// A list that leaves its segment is not read: it sets the status word.
__global__ void __launch_bounds__(256) k_probe_site_flags(ProbeTrees T, ProbeChunk C, int32_t* val, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeUnit& u = C.units[C.k0 + j];
    const int32_t site = u.site, slot = u.slot;
    GList l = T.lists[(size_t)slot * C.n + v];
    if ((unsigned long long)l.off + l.cnt > u.seg_len) { atomicOr(&status[u.sample], (int32_t)k_probe_bad_list); l.cnt = 0; }
    const MutRec* r = T.recs + u.seg_base + l.off;
    int32_t s = -1;
    if (v == T.root[slot]) {
      s = u.ref_state >= 0 ? u.ref_state : (int32_t)T.ref[(size_t)slot * T.L + site];
      for (uint32_t i = 0; i < l.cnt; ++i) if (r[i].site == site) s = r[i].to;
    } else {
      for (uint32_t i = 0; i < l.cnt; ++i) if (r[i].site == site) { s = r[i].to; break; }
    }
    val[(size_t)j * C.n + v] = s;
  }
}
// `root_val`: what an unflagged root hands down (ancestors: the "none" member).
__global__ void __launch_bounds__(256) k_probe_jump_init(ProbeTrees T, ProbeChunk C, int32_t root_val, int32_t* val, int32_t* jump) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const int32_t slot = C.units[C.k0 + j].slot;
    const size_t o = (size_t)j * C.n + v;
    int32_t f = val[o];
    const int32_t p = T.parent[(size_t)slot * C.n + v];
    if (v == T.root[slot] && f < 0) { f = root_val; val[o] = f; }
    jump[o] = (f >= 0 || (uint32_t)p >= (uint32_t)C.n) ? v : p;
  }
}
__global__ void __launch_bounds__(256) k_probe_jump_double(int n, int B, const int32_t* in, int32_t* out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  for (int j = blockIdx.y; j < B; j += gridDim.y) {
    const int32_t* row = in + (size_t)j * n;
    out[(size_t)j * n + v] = row[row[v]];
  }
}

// ---- step 2 -----------------------------------------------------------------------------------------------------------------------
// fix / diff zeroed before the launch; status [count].  kSites: a branch whose own node is flagged carries the mutation: the state above
// fades out along it, the state below fades in (site_states_tree_prober.cpp:19-33).  Ancestors: a marked node's own branch still belongs
// to the member above it, and val[v] is not loaded.
template <bool kSites>
__global__ void __launch_bounds__(256) k_probe_branches(ProbeTrees T, ProbeChunk C, const int32_t* val, const int32_t* jump, unsigned long long* fix, int32_t* diff, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeUnit& u = C.units[C.k0 + j];
    const size_t in = (size_t)u.slot * C.n, o = (size_t)j * C.n;
    if (v == T.root[u.slot]) continue;
    const int32_t p = T.parent[in + v];
    if ((uint32_t)p >= (uint32_t)C.n) { atomicOr(&status[u.sample], (int32_t)k_probe_bad_link); continue; }
    const int32_t top = val[o + jump[o + p]];
    if ((uint32_t)top >= (uint32_t)C.num_members) continue;   // (a "none" that has no member of its own cannot occur: the root always has one)
    const double left = T.t[in + p], right = T.t[in + v];
    if (!(left <= right)) { atomicOr(&status[u.sample], (int32_t)k_probe_negative_branch); continue; }
    const ProbeGrid g = u.grid;
    unsigned long long* f = fix + (size_t)j * C.num_members * C.stride_cells;
    const int32_t own = kSites ? val[o + v] : -1;
    if (own >= 0 && own < C.num_members) {
      probe_add_trapezoid(g, f, top, left, right, 1.0, 0.0);
      probe_add_trapezoid(g, f, own, left, right, 0.0, 1.0);
    } else probe_add_boxcar(g, f, diff + (size_t)j * C.num_members * (C.stride_cells + 1), top, left, right);
  }
}
// One wavefront per (member, unit): prefix sum of the whole-cell differences, joined with the fixed-point fractions, to double once.
__global__ void __launch_bounds__(64) k_probe_counts(ProbeChunk C, const unsigned long long* fix, const int32_t* diff, double* counts) {
  const int m = blockIdx.x, lane = threadIdx.x;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeGrid grid = C.units[C.k0 + j].grid;
    const size_t base_v = (size_t)j * C.num_members * C.stride_cells + (size_t)m * grid.num_cells;
    const int32_t* d = diff + (size_t)j * C.num_members * (C.stride_cells + 1) + (size_t)m * (grid.num_cells + 1);
    long long carry = 0;
    for (int base = 0; base < grid.num_cells; base += k_wave) {
      const int c = base + lane;
      const uint32_t incl = wave_incl_scan_u32(c < grid.num_cells ? (uint32_t)d[c] : 0u, lane);
      const long long whole = carry + (long long)(int32_t)incl;
      if (c < grid.num_cells) {
        const long long total = whole * (1ll << grid.frac_bits) + (long long)fix[base_v + c];
        counts[base_v + c] = (double)total * grid.inv_scale;
      }
      carry += (long long)(int32_t)__shfl(incl, k_wave - 1, k_wave);
    }
  }
}

// ---- step 3 (tree_prober.h:56-95) -------------------------------------------------------------------------------------------------
// total / p_coalesce [B * stride_cells].
__global__ void __launch_bounds__(64) k_probe_cells(ProbeChunk C, const PopTable* pops, const double* counts, double* total, double* p_coalesce) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeUnit& u = C.units[C.k0 + j];
    const ProbeGrid grid = u.grid;
    if (c >= grid.num_cells) continue;
    const PopTable pt = pops[u.pop];
    const double* cnt = counts + (size_t)j * C.num_members * C.stride_cells;
    const double t_lbound = probe_cell_lbound(grid, c), t_ubound = t_lbound + grid.cell_size;
    const double intensity = dev::pop_intensity_integral(pt, t_lbound, t_ubound);
    double tot = 0.0;
    for (int m = 0; m < C.num_members; ++m) tot += cnt[(size_t)m * grid.num_cells + c];
    total[(size_t)j * C.stride_cells + c] = tot;
    p_coalesce[(size_t)j * C.stride_cells + c] = 1.0 - dev::m_exp(-tot * intensity);
  }
}
// The member that starts at probability 1 (every other at 0): ancestors, "none of them" (the last member); kSites, the state of the
// unit's root (val of the root, as k_probe_site_flags left it).  p_all [units][num_members][out_cells].
template <bool kSites>
__global__ void __launch_bounds__(64) k_probe_chain(ProbeTrees T, ProbeChunk C, int out_cells, const int32_t* val, const double* counts, const double* total, const double* p_coalesce, double* p_all) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= C.num_members) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeUnit& u = C.units[C.k0 + j];
    const int num_cells = u.grid.num_cells, cells_to_skip = u.cells_to_skip;
    int32_t initial = C.num_members - 1;
    if (kSites) {
      const int32_t r = T.root[u.slot];
      initial = (uint32_t)r < (uint32_t)C.n ? val[(size_t)j * C.n + r] : -1;
    }
    const double* cnt = counts + (size_t)j * C.num_members * C.stride_cells + (size_t)m * num_cells;
    const double* tt = total + (size_t)j * C.stride_cells;
    const double* pp = p_coalesce + (size_t)j * C.stride_cells;
    double* p_out = p_all + ((size_t)(C.k0 + j) * C.num_members + m) * out_cells;
    double p = m == initial ? 1.0 : 0.0;
    for (int c = 0; c < num_cells; ++c) {
      const double tot = tt[c], pc = pp[c];
      const double pc_cat = tot == 0.0 ? 0.0 : pc * (cnt[c] / tot);
      p = pc_cat + (1.0 - pc) * p;
      if (c >= cells_to_skip && c - cells_to_skip < out_cells) p_out[c - cells_to_skip] = p;
    }
  }
}

// ---- step 4 -----------------------------------------------------------------------------------------------------------------------
// p_all [count][values].
__global__ void __launch_bounds__(256) k_probe_mean(const double* p_all, int count, size_t values, double* mean) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= values) return;
  double s = p_all[i];
  for (int k = 1; k < count; ++k) s += p_all[(size_t)k * values + i];
  mean[i] = s / count;
}
// The bitonic network every sort over the samples goes through (the order statistics below, the MCC nodes' dates in emat_mcc_summary_kernels.hpp):
// the `padded` (a power of two) doubles of `sorted`, in LDS and complete (a __syncthreads behind their last write), ascending; called by the whole workgroup.
__device__ inline void probe_bitonic_sort(double* sorted, int padded) {
  for (int size = 2; size <= padded; size *= 2) {
    for (int gap = size / 2; gap > 0; gap /= 2) {
      for (int k = threadIdx.x; k < padded; k += blockDim.x) {
        const int partner = k ^ gap;
        if (partner > k) {
          const double a = sorted[k], b = sorted[partner];
          const bool ascending = (k & size) == 0;
          if ((a > b) == ascending) { sorted[k] = b; sorted[partner] = a; }
        }
      }
      __syncthreads();
    }
  }
}
// `padded`: the power of two >= count (<= k_probe_sort_max); dynamic LDS: padded doubles.  order_stats [num_ranks][values].
__global__ void __launch_bounds__(k_probe_sort_threads) k_probe_order_stats(const double* p_all, int count, int padded, size_t values, const int32_t* ranks, int num_ranks, double* order_stats) {
  extern __shared__ __attribute__((aligned(16))) double probe_sorted[];
  for (size_t i = blockIdx.x; i < values; i += gridDim.x) {   // (uniform over the workgroup)
    for (int k = threadIdx.x; k < padded; k += blockDim.x) probe_sorted[k] = k < count ? p_all[(size_t)k * values + i] : __builtin_inf();
    __syncthreads();
    probe_bitonic_sort(probe_sorted, padded);
    for (int r = threadIdx.x; r < num_ranks; r += blockDim.x) {
      const int32_t q = ranks[r];
      if (q >= 0 && q < count) order_stats[(size_t)r * values + i] = probe_sorted[q];
    }
    __syncthreads();
  }
}

}  // namespace emat
#endif  // EMAT_PROBE_KERNELS_HPP_
