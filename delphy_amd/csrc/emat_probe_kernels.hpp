// emat_probe_kernels.hpp -- the tree probers on the tree resident in HBM: where, over time, a fresh sample would coalesce.
//
// Reference: probe_ancestors_on_tree (core/ancestral_tree_prober.cpp), probe_site_states_on_tree
// (core/site_states_tree_prober.cpp), both through Tree_prober (core/tree_prober.h) on a Staircase_family of branch counts
// (core/staircase.{h,cpp}: add_boxcar, add_trapezoid).  Three steps, each a few small launches on the engine's stream:
//
// 1. A label for every node: the member (closest marked ancestor, or state of the site) its branch starts in.  Both probers
//    ask the same question -- the nearest FLAGGED node at or above a node's parent -- where the reference carries the answer
//    down a recursion.  Here: pointer doubling over the parent array.  `val[v]` >= 0 flags v and is what it hands to the
//    branches below it (the root is always flagged); jump[v] starts as v for a flagged node and parent[v] otherwise, and
//    every round replaces jump[v] by jump[jump[v]] (two buffers, so a round reads only the previous round's values and the
//    result does not depend on scheduling).  After ceil(log2 n) rounds every jump[v] is the nearest flagged node at or above
//    v, and the label of v's branch is val[jump[parent[v]]].  Chosen over the depth / visiting order the partitioner's
//    kernels have because those walk PARTS serially, one thread per part: there are no parts here, and a walk of the whole
//    tree by one thread is what is to be avoided.  Cost: 18 rounds of two 4-byte accesses per node at 200 000 nodes.
// 2. Branch counts, one thread per branch.  A cell a boxcar of height 1 covers whole gets +1 through a per-member
//    difference array (int32, one prefix sum at the end: exact).  Every other contribution -- the two end cells of a boxcar,
//    every cell of a trapezoid -- is a fraction in [0, 1] and is added in 64-BIT FIXED POINT with integer atomics, so the
//    sum is the same bits whatever order the branches arrive in.  Quantum 2^-f, f = min(52, 61 - ceil(log2(n + 1))) for a
//    tree of n nodes (52 up to 511 nodes, 43 at 200 000): a cell receives fewer than n whole units and fewer than n
//    fractions of at most 1 + 2^-50 each, so |sum| < 2 n 2^f (1 + 2^-50) <= 2^62 fits an int64.  Each term is rounded to
//    the quantum once (error <= 2^-(f+1)); the cell's total, whole part shifted in, is converted to double once.
// 3. Tree_prober's recurrence: per cell (parallel) the total over members, summed in member order as the reference does,
//    and the probability of coalescing in the cell; then per member (parallel) the chain over cells.
//
// Where the reference is undefined these kernels and tests/prober_model.py choose the same, stated thing: a cell index that
// rounding puts outside [0, cells) is clamped (the reference asserts), and a boxcar or trapezoid whose last cell comes out
// BEFORE its first (both ends within rounding of one cell boundary; the reference would run off its array) is entered as if
// both ends lay in the first.  A branch that ends before it starts (the reference throws) sets the status word.
//
// Included by emat_backend.hip after emat_gtree_kernels.hpp (GTreeDev, wave_incl_scan_u32).
#ifndef EMAT_PROBE_KERNELS_HPP_
#define EMAT_PROBE_KERNELS_HPP_

namespace emat {

struct ProbeGrid {                   // the Staircase_family of branch counts (staircase.h:21-52)
  double x_start, cell_size, x_end;  // x_end = x_start + num_cells * cell_size, as Staircase::x_end() computes it
  int32_t num_cells;                 // the cells the caller asked for plus the ones prepended to reach the root (cells_to_skip)
  int32_t frac_bits;                 // f above
  double scale, inv_scale;           // 2^f, 2^-f
};
enum ProbeStatus : int32_t { k_probe_ok = 0, k_probe_negative_branch = 1 };

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

// ---- step 1 ---------------------------------------------------------------------------------------------------------
// Ancestors: val was filled with -1; marked node i gets the smallest index it appears under (std::ranges::find: the first wins).
__global__ void __launch_bounds__(256) k_probe_marks(int32_t* val, const int32_t* marked, int num_marked, int n_nodes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_marked) return;
  const int32_t v = marked[i];
  if (v >= 0 && v < n_nodes) atomicMin((unsigned int*)&val[v], (unsigned int)i);   // (-1 is the largest unsigned value)
}
// Site states: val[v] = the state the first mutation of `site` on v's branch leads to, -1 when there is none; the root hands down the
// state of the reference sequence, changed by every mutation of the site on its own list (site_states_tree_prober.cpp:73-79).
__global__ void __launch_bounds__(256) k_probe_site_flags(GTreeDev g, int32_t site, int32_t ref_state, int32_t* val) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= g.n_nodes) return;
  const GList l = g.muts[v];
  const MutRec* r = g.mut_heap + l.off;
  if (v == *g.root) {
    int32_t s = ref_state;
    for (uint32_t k = 0; k < l.cnt; ++k) if (r[k].site == site) s = r[k].to;
    val[v] = s;
    return;
  }
  int32_t s = -1;
  for (uint32_t k = 0; k < l.cnt; ++k) if (r[k].site == site) { s = r[k].to; break; }
  val[v] = s;
}
// `root_val`: what an unflagged root hands down (ancestors: the "none" member).
__global__ void __launch_bounds__(256) k_probe_jump_init(GTreeDev g, int32_t* val, int32_t root_val, int32_t* jump) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= g.n_nodes) return;
  int32_t f = val[v];
  const int32_t p = g.parent[v];
  if (v == *g.root && f < 0) { f = root_val; val[v] = f; }
  jump[v] = (f >= 0 || (uint32_t)p >= (uint32_t)g.n_nodes) ? v : p;
}
__global__ void __launch_bounds__(256) k_probe_jump_double(int n_nodes, const int32_t* in, int32_t* out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n_nodes) out[v] = in[in[v]];
}

// ---- step 2 ---------------------------------------------------------------------------------------------------------
// kSites: a branch whose own node is flagged carries the mutation: the state above fades out along it, the state below fades in
// (site_states_tree_prober.cpp:19-33).  Ancestors: a marked node's own branch still belongs to the member above it.
template <bool kSites>
__global__ void __launch_bounds__(256) k_probe_branches(GTreeDev g, ProbeGrid grid, const int32_t* val, const int32_t* jump, int num_members,
                                                        unsigned long long* fix, int32_t* diff, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= g.n_nodes || v == *g.root) return;
  const int32_t p = g.parent[v];
  if ((uint32_t)p >= (uint32_t)g.n_nodes) return;
  const int32_t top = val[jump[p]];
  if ((uint32_t)top >= (uint32_t)num_members) return;   // (a "none" that has no member of its own cannot occur: the root always has one)
  const double left = g.t[p], right = g.t[v];
  if (!(left <= right)) { atomicMax(status, (int32_t)k_probe_negative_branch); return; }
  const int32_t own = kSites ? val[v] : -1;
  if (own >= 0 && own < num_members) {
    probe_add_trapezoid(grid, fix, top, left, right, 1.0, 0.0);
    probe_add_trapezoid(grid, fix, own, left, right, 0.0, 1.0);
  } else probe_add_boxcar(grid, fix, diff, top, left, right);
}
// One wavefront per member: prefix sum of the whole-cell differences, joined with the fixed-point fractions, to double once.
__global__ void __launch_bounds__(64) k_probe_counts(ProbeGrid grid, const unsigned long long* fix, const int32_t* diff, double* counts) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int32_t* d = diff + (size_t)m * (grid.num_cells + 1);
  long long carry = 0;
  for (int base = 0; base < grid.num_cells; base += k_wave) {
    const int c = base + lane;
    const uint32_t incl = wave_incl_scan_u32(c < grid.num_cells ? (uint32_t)d[c] : 0u, lane);
    const long long whole = carry + (long long)(int32_t)incl;
    if (c < grid.num_cells) {
      const long long total = whole * (1ll << grid.frac_bits) + (long long)fix[(size_t)m * grid.num_cells + c];
      counts[(size_t)m * grid.num_cells + c] = (double)total * grid.inv_scale;
    }
    carry += (long long)(int32_t)__shfl(incl, k_wave - 1, k_wave);
  }
}

// ---- step 3 (tree_prober.h:56-95) -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_probe_cells(ProbeGrid grid, PopTable pt, int num_members, const double* counts, double* total, double* p_coalesce) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= grid.num_cells) return;
  const double t_lbound = probe_cell_lbound(grid, c), t_ubound = t_lbound + grid.cell_size;
  const double intensity = dev::pop_intensity_integral(pt, t_lbound, t_ubound);
  double tot = 0.0;
  for (int m = 0; m < num_members; ++m) tot += counts[(size_t)m * grid.num_cells + c];
  total[c] = tot;
  p_coalesce[c] = 1.0 - dev::m_exp(-tot * intensity);
}
// `initial`: the member that starts at probability 1 (every other at 0); read from *initial_ptr when that is given (the root's state).
__global__ void __launch_bounds__(64) k_probe_chain(ProbeGrid grid, int num_members, int cells_to_skip, const double* counts, const double* total, const double* p_coalesce,
                                                    int32_t initial, const int32_t* initial_ptr, double* p_out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= num_members) return;
  if (initial_ptr) initial = *initial_ptr;
  const int out_cells = grid.num_cells - cells_to_skip;
  double p = m == initial ? 1.0 : 0.0;
  for (int c = 0; c < grid.num_cells; ++c) {
    const double tot = total[c], pc = p_coalesce[c];
    const double pc_cat = tot == 0.0 ? 0.0 : pc * (counts[(size_t)m * grid.num_cells + c] / tot);
    p = pc_cat + (1.0 - pc) * p;
    if (c >= cells_to_skip) p_out[(size_t)m * out_cells + (c - cells_to_skip)] = p;
  }
}

}  // namespace emat
#endif  // EMAT_PROBE_KERNELS_HPP_
