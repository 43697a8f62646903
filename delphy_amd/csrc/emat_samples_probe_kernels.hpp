// emat_samples_probe_kernels.hpp -- the ancestral prober over MANY sampled trees of the store at once, and the spread of its answers;
// further down the site-state prober in the same shape, over (sample, site) pairs, for samples that kept their mutations.
//
// Reference: probe_ancestors_on_tree (core/ancestral_tree_prober.cpp:31-77) run on every base tree of an MCC tree, the marked nodes
// of a base tree being the nodes that correspond to the MCC nodes picked (tools/delphy_wasm.cpp:1828-1849).  A sample of the store
// (emat_mcc_kernels.hpp: MccStore) holds exactly what that prober reads -- parent, times, root -- so nothing new is stored.  The
// steps are those of emat_probe_kernels.hpp, each over (samples of a chunk x nodes) or (samples x members x cells), every step a
// launch of its own whose count does not depend on the number of samples:
//
// 0. Roots: the chosen samples' root times, one copy to the host, which makes every sample's grid with the arithmetic the
//    single-tree call uses (emat_probe_host.hpp: probe_extend_grid) and uploads the descriptors (SProbeSample) as one array.
// 1. Marks into a per-sample val (first entry wins: atomicMin), from a host array -- one for all or one per sample -- or through
//    the correspondence table of the last derivation; then jump-doubling over B n entries between two buffers, ceil(log2 n) rounds.
// 2. One thread per (sample, branch): probe_add_boxcar UNCHANGED into that sample's difference array and fixed-point cells, so the
//    counts are the single-tree call's bits; prefix sum and fixed-point join as k_probe_counts.
// 3. Per (sample, cell) the total in member order and the probability of coalescing, with that sample's PopTable; per (sample,
//    member) the chain over cells: the expressions of k_probe_cells / k_probe_chain, compiled without contraction as they are.
// 4. Summaries of the per-sample results [count][values], values = members x cells: the mean, one thread per value adding the
//    samples in sample order and dividing once; order statistics, one workgroup per value, which brings the count values into LDS,
//    sorts them with a bitonic network padded with +inf (exact: only compares and swaps) and writes the ranks asked for.
//
// A chunk is B samples; sample j of a chunk owns val / jump [j n], fix / counts [j members stride], diff [j members (stride + 1)]
// and total / p_coalesce [j stride], stride = the largest cell count of any chosen sample, and inside its region a sample uses
// its OWN compact layout (member * num_cells + cell), which is what probe_add_frac addresses.  Nothing depends on B.
//
// Cross-workgroup accumulation is by integer atomics only.  Bounds: a link or root outside [0, n) is never followed and sets the
// sample's status word, as does a branch that ends before it starts; no loop runs without a bound it checks.  The sort's LDS is
// dynamic shared memory sized by the launch: the library's static LDS objects keep their fixed addresses.
//
// Included by emat_backend.hip after emat_probe_kernels.hpp (ProbeGrid, probe_add_boxcar) and emat_mcc_kernels.hpp (MccStore, MccPick).
#ifndef EMAT_SAMPLES_PROBE_KERNELS_HPP_
#define EMAT_SAMPLES_PROBE_KERNELS_HPP_

namespace emat {

struct SProbeSample {                // one chosen sample: where it is, its grid, its population model
  ProbeGrid grid;
  int32_t slot;                      // first + k * stride
  int32_t cells_to_skip;
  int32_t pop;                       // index into the PopTable array
  int32_t pad;
};
struct SProbeChunk {                 // the samples [k0, k0 + B) of a call and the layout of their working room
  const SProbeSample* samples;       // [count]
  int32_t k0, B, n, num_members;
  int32_t stride_cells, pad;
};
enum SProbeStatus : int32_t { k_sprobe_ok = 0, k_sprobe_negative_branch = 1, k_sprobe_bad_link = 2, k_sprobe_bad_list = 4 };
constexpr int k_sprobe_sort_max = 4096;       // samples the order statistics hold: 32 KB of LDS for a workgroup
constexpr int k_sprobe_sort_threads = 256;

// Step 0.  root_t [count]; status [count] zeroed before the launch.
__global__ void __launch_bounds__(256) k_sprobe_roots(MccStore S, MccPick pick, double* root_t, int32_t* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= pick.M) return;
  const int32_t slot = pick.first + k * pick.stride;
  const int32_t r = S.root[slot];
  if ((uint32_t)r >= (uint32_t)S.n) { atomicOr(&status[k], (int32_t)k_sprobe_bad_link); root_t[k] = 0.0; return; }
  root_t[k] = S.t[(size_t)slot * S.n + r];
}

// Step 1.  val [B * n] was filled with -1.  `marks` [num_marked] (marks_stride 0) or [count][num_marked] (marks_stride num_marked);
// with `corr` ([count][n], the last derivation's table) a mark is an MCC node and stands for the sample's corresponding node.
__global__ void __launch_bounds__(256) k_sprobe_marks(SProbeChunk C, const int32_t* marks, int num_marked, int marks_stride, const int32_t* corr, int32_t* val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_marked) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const size_t k = (size_t)(C.k0 + j);
    int32_t v = marks[k * marks_stride + i];
    if (corr && v >= 0 && v < C.n) v = corr[k * C.n + v];
    if (v >= 0 && v < C.n) atomicMin((unsigned int*)&val[(size_t)j * C.n + v], (unsigned int)i);   // (-1 is the largest unsigned value)
  }
}
// k_probe_jump_init on a slot of the store; an unflagged root hands down `root_val`.
__global__ void __launch_bounds__(256) k_sprobe_jump_init(MccStore S, SProbeChunk C, int32_t root_val, int32_t* val, int32_t* jump) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const int32_t slot = C.samples[C.k0 + j].slot;
    const size_t o = (size_t)j * C.n + v;
    int32_t f = val[o];
    const int32_t p = S.parent[(size_t)slot * C.n + v];
    if (v == S.root[slot] && f < 0) { f = root_val; val[o] = f; }
    jump[o] = (f >= 0 || (uint32_t)p >= (uint32_t)C.n) ? v : p;
  }
}
__global__ void __launch_bounds__(256) k_sprobe_jump_double(int n, int B, const int32_t* in, int32_t* out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  for (int j = blockIdx.y; j < B; j += gridDim.y) {
    const int32_t* row = in + (size_t)j * n;
    out[(size_t)j * n + v] = row[row[v]];
  }
}

// Step 2.  k_probe_branches<false> on a slot of the store; fix / diff zeroed before the launch; status [count].
__global__ void __launch_bounds__(256) k_sprobe_branches(MccStore S, SProbeChunk C, const int32_t* val, const int32_t* jump, unsigned long long* fix, int32_t* diff, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const SProbeSample& s = C.samples[C.k0 + j];
    const size_t in = (size_t)s.slot * C.n, o = (size_t)j * C.n;
    if (v == S.root[s.slot]) continue;
    const int32_t p = S.parent[in + v];
    if ((uint32_t)p >= (uint32_t)C.n) { atomicOr(&status[C.k0 + j], (int32_t)k_sprobe_bad_link); continue; }
    const int32_t top = val[o + jump[o + p]];
    if ((uint32_t)top >= (uint32_t)C.num_members) continue;
    const double left = S.t[in + p], right = S.t[in + v];
    if (!(left <= right)) { atomicOr(&status[C.k0 + j], (int32_t)k_sprobe_negative_branch); continue; }
    const ProbeGrid g = s.grid;
    probe_add_boxcar(g, fix + (size_t)j * C.num_members * C.stride_cells, diff + (size_t)j * C.num_members * (C.stride_cells + 1), top, left, right);
  }
}
// k_probe_counts: one wavefront per (member, sample).
__global__ void __launch_bounds__(64) k_sprobe_counts(SProbeChunk C, const unsigned long long* fix, const int32_t* diff, double* counts) {
  const int m = blockIdx.x, lane = threadIdx.x;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const ProbeGrid grid = C.samples[C.k0 + j].grid;
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

// Step 3.  k_probe_cells with the sample's own PopTable; total / p_coalesce [B * stride_cells].
__global__ void __launch_bounds__(64) k_sprobe_cells(SProbeChunk C, const PopTable* pops, const double* counts, double* total, double* p_coalesce) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const SProbeSample& s = C.samples[C.k0 + j];
    const ProbeGrid grid = s.grid;
    if (c >= grid.num_cells) continue;
    const PopTable pt = pops[s.pop];
    const double* cnt = counts + (size_t)j * C.num_members * C.stride_cells;
    const double t_lbound = probe_cell_lbound(grid, c), t_ubound = t_lbound + grid.cell_size;
    const double intensity = dev::pop_intensity_integral(pt, t_lbound, t_ubound);
    double tot = 0.0;
    for (int m = 0; m < C.num_members; ++m) tot += cnt[(size_t)m * grid.num_cells + c];
    total[(size_t)j * C.stride_cells + c] = tot;
    p_coalesce[(size_t)j * C.stride_cells + c] = 1.0 - dev::m_exp(-tot * intensity);
  }
}
// k_probe_chain, starting in "none of them" (the last member); p_all [count][num_members][out_cells].
__global__ void __launch_bounds__(64) k_sprobe_chain(SProbeChunk C, int out_cells, const double* counts, const double* total, const double* p_coalesce, double* p_all) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= C.num_members) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const SProbeSample& s = C.samples[C.k0 + j];
    const int num_cells = s.grid.num_cells, cells_to_skip = s.cells_to_skip;
    const double* cnt = counts + (size_t)j * C.num_members * C.stride_cells + (size_t)m * num_cells;
    const double* tt = total + (size_t)j * C.stride_cells;
    const double* pp = p_coalesce + (size_t)j * C.stride_cells;
    double* p_out = p_all + ((size_t)(C.k0 + j) * C.num_members + m) * out_cells;
    double p = m == C.num_members - 1 ? 1.0 : 0.0;
    for (int c = 0; c < num_cells; ++c) {
      const double tot = tt[c], pc = pp[c];
      const double pc_cat = tot == 0.0 ? 0.0 : pc * (cnt[c] / tot);
      p = pc_cat + (1.0 - pc) * p;
      if (c >= cells_to_skip && c - cells_to_skip < out_cells) p_out[c - cells_to_skip] = p;
    }
  }
}

// ---- the site-state form ---------------------------------------------------------------------------------------------------
// probe_site_states_on_tree (core/site_states_tree_prober.cpp:40-92) on samples that kept their mutations (emat_mcc_host.hpp:
// emat_tree_samples_reserve_mutations).  The unit of work is a (sample, site) pair: the descriptor array holds one SProbeSample per
// unit, sample-major (unit u = k * num_sites + i: sample k, entry i of `sites`), the 4 states are the members, and a unit owns the
// working room a sample owns above.  So k_sprobe_jump_init, k_sprobe_jump_double, k_sprobe_counts and k_sprobe_cells run on units
// as they are, and the results land as [count][num_sites][4][cells]; what differs is where the labels come from (the slot's lists),
// the branches (trapezoids for a branch that carries a mutation of the site) and the chain's initial member (the root's state).
// The status word stays one per SAMPLE: status [count].
struct MccMuts {                     // what a slot keeps of its mutations
  const GList* hdr;                  // [capacity * n] per-node lists: records [off, off + cnt) of the slot's segment
  const uint8_t* ref;                // [capacity * L] the reference sequence the slot's root starts from
  const MutRec* arena;               // the segments of all slots
  int32_t L, pad;
};
struct SProbeSeg { long long base; uint32_t len, pad; };   // a chosen sample's segment: arena [base, base + len)

// k_probe_site_flags on the lists of a slot.  A list that leaves its segment is not read: it sets the status word.
__global__ void __launch_bounds__(256) k_sprobe_site_flags(MccStore S, MccMuts Mu, SProbeChunk C, const SProbeSeg* segs, const int32_t* sites, int num_sites, int32_t* val, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const int u = C.k0 + j, k = u / num_sites;
    const int32_t site = sites[u - k * num_sites], slot = C.samples[u].slot;
    const SProbeSeg seg = segs[k];
    GList l = Mu.hdr[(size_t)slot * C.n + v];
    if ((unsigned long long)l.off + l.cnt > seg.len) { atomicOr(&status[k], (int32_t)k_sprobe_bad_list); l.cnt = 0; }
    const MutRec* r = Mu.arena + seg.base + l.off;
    int32_t s = -1;
    if (v == S.root[slot]) {
      s = Mu.ref[(size_t)slot * Mu.L + site];
      for (uint32_t i = 0; i < l.cnt; ++i) if (r[i].site == site) s = r[i].to;
    } else {
      for (uint32_t i = 0; i < l.cnt; ++i) if (r[i].site == site) { s = r[i].to; break; }
    }
    val[(size_t)j * C.n + v] = s;
  }
}
// k_probe_branches<true> on a slot of the store (4 members).
__global__ void __launch_bounds__(256) k_sprobe_site_branches(MccStore S, SProbeChunk C, int num_sites, const int32_t* val, const int32_t* jump, unsigned long long* fix, int32_t* diff, int32_t* status) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= C.n) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const int u = C.k0 + j, k = u / num_sites;
    const SProbeSample& s = C.samples[u];
    const size_t in = (size_t)s.slot * C.n, o = (size_t)j * C.n;
    if (v == S.root[s.slot]) continue;
    const int32_t p = S.parent[in + v];
    if ((uint32_t)p >= (uint32_t)C.n) { atomicOr(&status[k], (int32_t)k_sprobe_bad_link); continue; }
    const int32_t top = val[o + jump[o + p]];
    if ((uint32_t)top >= (uint32_t)C.num_members) continue;
    const double left = S.t[in + p], right = S.t[in + v];
    if (!(left <= right)) { atomicOr(&status[k], (int32_t)k_sprobe_negative_branch); continue; }
    const ProbeGrid g = s.grid;
    unsigned long long* f = fix + (size_t)j * C.num_members * C.stride_cells;
    const int32_t own = val[o + v];
    if (own >= 0 && own < C.num_members) {
      probe_add_trapezoid(g, f, top, left, right, 1.0, 0.0);
      probe_add_trapezoid(g, f, own, left, right, 0.0, 1.0);
    } else probe_add_boxcar(g, f, diff + (size_t)j * C.num_members * (C.stride_cells + 1), top, left, right);
  }
}
// k_probe_chain, starting in the state of the unit's root (val of the root, as k_sprobe_site_flags left it); p_all [units][4][out_cells].
__global__ void __launch_bounds__(64) k_sprobe_site_chain(MccStore S, SProbeChunk C, int out_cells, const int32_t* val, const double* counts, const double* total, const double* p_coalesce, double* p_all) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= C.num_members) return;
  for (int j = blockIdx.y; j < C.B; j += gridDim.y) {
    const SProbeSample& s = C.samples[C.k0 + j];
    const int num_cells = s.grid.num_cells, cells_to_skip = s.cells_to_skip;
    const int32_t r = S.root[s.slot];
    const int32_t initial = (uint32_t)r < (uint32_t)C.n ? val[(size_t)j * C.n + r] : -1;
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

// Step 4.  p_all [count][values].
__global__ void __launch_bounds__(256) k_sprobe_mean(const double* p_all, int count, size_t values, double* mean) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= values) return;
  double s = p_all[i];
  for (int k = 1; k < count; ++k) s += p_all[(size_t)k * values + i];
  mean[i] = s / count;
}
// `padded`: the power of two >= count (<= k_sprobe_sort_max); dynamic LDS: padded doubles.  order_stats [num_ranks][values].
__global__ void __launch_bounds__(k_sprobe_sort_threads) k_sprobe_order_stats(const double* p_all, int count, int padded, size_t values, const int32_t* ranks, int num_ranks, double* order_stats) {
  extern __shared__ __attribute__((aligned(16))) double sprobe_sorted[];
  for (size_t i = blockIdx.x; i < values; i += gridDim.x) {   // (uniform over the workgroup)
    for (int k = threadIdx.x; k < padded; k += blockDim.x) sprobe_sorted[k] = k < count ? p_all[(size_t)k * values + i] : __builtin_inf();
    __syncthreads();
    for (int size = 2; size <= padded; size *= 2) {
      for (int gap = size / 2; gap > 0; gap /= 2) {
        for (int k = threadIdx.x; k < padded; k += blockDim.x) {
          const int partner = k ^ gap;
          if (partner > k) {
            const double a = sprobe_sorted[k], b = sprobe_sorted[partner];
            const bool ascending = (k & size) == 0;
            if ((a > b) == ascending) { sprobe_sorted[k] = b; sprobe_sorted[partner] = a; }
          }
        }
        __syncthreads();
      }
    }
    for (int r = threadIdx.x; r < num_ranks; r += blockDim.x) {
      const int32_t q = ranks[r];
      if (q >= 0 && q < count) order_stats[(size_t)r * values + i] = sprobe_sorted[q];
    }
    __syncthreads();
  }
}

}  // namespace emat
#endif  // EMAT_SAMPLES_PROBE_KERNELS_HPP_
