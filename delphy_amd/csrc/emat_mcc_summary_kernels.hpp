// emat_mcc_summary_kernels.hpp -- what a front end draws ON the MCC tree, made from the last derivation's correspondence table where it
// lies: the spread of every MCC node's date over the samples (quantiles and the shortest interval holding a given share of them), and in
// how many samples each of the master's mutations occurs, with its mean, earliest and latest time.
//
// Reference: the MCC tree exposes its base trees and, per base tree, the corresponding node and whether it matches exactly
// (core/mcc_tree.h:91-98), exported (tools/delphy_wasm.cpp:1503-1523) so that a front end loops over every base tree.  Here that loop
// would pull the (M x n) table and every sample to the host; the kernels below read them in HBM.
// M = samples of the derivation, sample k = slot first + k * stride, n = nodes; for MCC node v: c(k, v) = corr[k][v], x(k, v) = t[c(k, v)] of sample k.
//
// 1. k_mccs_gather: for a chunk of B nodes, x(k, v) and exact[k][v] sample-major ([M][B]: 9 bytes per sample and node).  Thread j of a row
//    reads corr[k n + v] next to its neighbours' and follows it into the sample's times.  Every c is checked against [0, n) before it is
//    followed; a c outside, or a time that is not finite (+inf is the sort's padding), raises the sample's flag instead.
// 2. k_mccs_node_stats: one workgroup per node.  The column goes into LDS, padded with +inf to a power of two, and through the bitonic
//    network of the probers' order statistics (probe_bitonic_sort, emat_probe_kernels.hpp); then, with s the first m entries:
//      quantile j = s[floor(q_j (double)(m - 1))];
//      HPD: w = min(m, max(1, ceil(mass (double)m))), i* the SMALLEST i in [0, m - w] that minimises s[i + w - 1] - s[i]: every thread
//      keeps the first minimum of its own ascending i, and the workgroup reduces the pairs (width, i) lexicographically, so the first
//      minimum wins whatever the shape of the reduction.
//    Twice: once over all M samples (`mrca`, the spread behind t_mrca), once with +inf where the sample does not have the node's clade
//    (`exact`, m = num_exact, the spread behind t).  The second load of the column comes from L2.
//    Every output is one of the store's doubles; nothing is added or interpolated, so the results are the same bits for every chunk size.
// 3. k_mccs_mutation_support: one thread per record of the master, in the CSR order emat_tree_sample_get_mutations returns them, loops
//    over the samples IN ORDER (as k_mcc_derived does): where exact[k][v], the first record of the list of c(k, v) with the same site,
//    from and to gives the time.  Every header is checked against its sample's segment before its list is read.
//
// Plain launches, no cooperative groups and no atomics: a flag is a plain store of 1, which every thread that raises it writes alike.
//
// Included by emat_backend.hip after emat_mcc_kernels.hpp (MccStore, MccPick) and emat_probe_kernels.hpp (probe_bitonic_sort).
#ifndef EMAT_MCC_SUMMARY_KERNELS_HPP_
#define EMAT_MCC_SUMMARY_KERNELS_HPP_

namespace emat {

constexpr int k_mccs_threads = k_probe_sort_threads;

struct MccsFlags { int32_t* bad_link; int32_t* not_finite; int32_t* bad_list; };   // each [M], zeroed before a call: which samples a kernel stumbled over

// Step 1.  nodes [B] (the chunk's MCC nodes) or NULL: v0, v0 + 1, ...; x, e [M][B].  grid (ceil(B / 256), <= M).
__global__ void __launch_bounds__(256) k_mccs_gather(MccStore S, MccPick pick, const int32_t* corr, const uint8_t* exact, const int32_t* nodes, int32_t v0, int32_t B,
                                                      double* x, uint8_t* e, MccsFlags F) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = S.n;
  if (j >= B) return;
  const int32_t v = nodes ? nodes[j] : v0 + j;             // (checked by the host)
  for (int k = blockIdx.y; k < pick.M; k += gridDim.y) {
    const size_t in = (size_t)(pick.first + (size_t)k * pick.stride) * n, tab = (size_t)k * n, out = (size_t)k * B + j;
    const int32_t c = corr[tab + v];
    double tc = __builtin_inf();
    if ((uint32_t)c >= (uint32_t)n) F.bad_link[k] = 1;
    else { tc = S.t[in + c]; if (!(fabs(tc) < __builtin_inf())) F.not_finite[k] = 1; }
    x[out] = tc; e[out] = exact[tab + v];
  }
}

// The shortest window of w of the m sorted values, the first on ties: (lo, hi) by thread 0.  red_w / red_i: a slot per thread.
__device__ inline void mccs_hpd(const double* s, int m, int w, double* red_w, int32_t* red_i, double* lo, double* hi) {
  double best_w = __builtin_inf(); int32_t best_i = 0x7fffffff;
  for (int i = threadIdx.x; i + w <= m; i += blockDim.x) {   // (ascending: a later equal width does not replace an earlier one)
    const double width = s[i + w - 1] - s[i];
    if (width < best_w || best_i == 0x7fffffff) { best_w = width; best_i = i; }
  }
  red_w[threadIdx.x] = best_w; red_i[threadIdx.x] = best_i;
  __syncthreads();
  for (int half = blockDim.x / 2; half > 0; half /= 2) {
    if ((int)threadIdx.x < half) {
      const double ow = red_w[threadIdx.x + half]; const int32_t oi = red_i[threadIdx.x + half];
      const double mw = red_w[threadIdx.x]; const int32_t mi = red_i[threadIdx.x];
      const bool other_has = oi != 0x7fffffff, mine_has = mi != 0x7fffffff;
      if (other_has && (!mine_has || ow < mw || (ow == mw && oi < mi))) { red_w[threadIdx.x] = ow; red_i[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { const int32_t i = red_i[0]; *lo = s[i]; *hi = s[i + w - 1]; }   // (w <= m and m >= 1: thread 0's i = 0 is always a candidate)
  __syncthreads();
}

struct MccsNodeOut {                 // device arrays of the whole call, column `col0 + j` of `cols` for node j of the chunk; any may be NULL
  double* q_exact; double* q_mrca;   // [num_quantiles][cols]
  double* hpd_exact; double* hpd_mrca;   // [2][cols]
  int32_t* num_exact;                // [cols]
  size_t cols, col0;
};

// Step 2.  x, e [M][B]; `padded`: the power of two >= M (<= k_probe_sort_max); dynamic LDS: padded doubles.
__global__ void __launch_bounds__(k_mccs_threads) k_mccs_node_stats(const double* x, const uint8_t* e, int M, int padded, int B, const double* quantiles, int num_quantiles, double hpd_mass, MccsNodeOut O) {
  extern __shared__ __attribute__((aligned(16))) double mccs_sorted[];
  __shared__ double red_w[k_mccs_threads];
  __shared__ int32_t red_i[k_mccs_threads];
  for (int j = blockIdx.x; j < B; j += gridDim.x) {        // (uniform over the workgroup)
    const size_t col = O.col0 + (size_t)j;
    for (int kind = 0; kind < 2; ++kind) {                 // 0: mrca, 1: exact
      double* q_out = kind ? O.q_exact : O.q_mrca; double* hpd_out = kind ? O.hpd_exact : O.hpd_mrca;
      if (!q_out && !hpd_out && !(kind && O.num_exact)) continue;   // (uniform)
      int32_t mine = 0;
      for (int k = threadIdx.x; k < padded; k += blockDim.x) {
        double val = __builtin_inf();
        if (k < M && (!kind || e[(size_t)k * B + j])) { val = x[(size_t)k * B + j]; ++mine; }
        mccs_sorted[k] = val;
      }
      int m = M;
      if (kind) {                                          // m = how many samples have the clade: an integer sum, any order
        red_i[threadIdx.x] = mine;
        __syncthreads();
        for (int half = blockDim.x / 2; half > 0; half /= 2) { if ((int)threadIdx.x < half) red_i[threadIdx.x] += red_i[threadIdx.x + half]; __syncthreads(); }
        m = red_i[0];
        __syncthreads();
        if (O.num_exact && threadIdx.x == 0) O.num_exact[col] = m;
      }
      if ((!q_out && !hpd_out) || m < 1) { __syncthreads(); continue; }   // (uniform; m < 1 only where the gather raised a flag)
      __syncthreads();
      probe_bitonic_sort(mccs_sorted, padded);
      if (q_out)
        for (int r = threadIdx.x; r < num_quantiles; r += blockDim.x) q_out[(size_t)r * O.cols + col] = mccs_sorted[(int)floor(quantiles[r] * (double)(m - 1))];
      if (hpd_out) {
        const int w = min(m, max(1, (int)ceil(hpd_mass * (double)m)));
        mccs_hpd(mccs_sorted, m, w, red_w, red_i, &hpd_out[col], &hpd_out[O.cols + col]);
      }
      __syncthreads();
    }
  }
}

struct MccsMuts {                    // the store's mutations and, per chosen sample, its segment of the arena
  const GList* lists; const MutRec* recs;   // lists [slots][n], offsets relative to the slot's segment
  const long long* seg_base; const uint32_t* seg_len;   // [M]
};

// Step 3.  rec_offset [n + 1]: the master's records in node order (a prefix sum of its list lengths); master_k: its position.
__global__ void __launch_bounds__(256) k_mccs_mutation_support(MccStore S, MccPick pick, int32_t master_k, const int32_t* corr, const uint8_t* exact, MccsMuts Q, const int32_t* rec_offset, int32_t num_records,
                                                                int32_t* num_with, double* mean_t, double* t_min, double* t_max, MccsFlags F) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = S.n;
  if (j >= num_records) return;
  int lo = 0, hi = n;                                      // the node v with rec_offset[v] <= j < rec_offset[v + 1]
  while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (rec_offset[mid] <= j) lo = mid; else hi = mid; }
  const int32_t v = lo;
  const GList mh = Q.lists[(size_t)(pick.first + (size_t)master_k * pick.stride) * n + v];   // (checked against the master's segment by the host)
  const MutRec want = Q.recs[Q.seg_base[master_k] + mh.off + (uint32_t)(j - rec_offset[v])];
  int32_t hits = 0;
  double sum = 0.0, first_t = __builtin_inf(), last_t = -__builtin_inf();
  for (int k = 0; k < pick.M; ++k) {
    const size_t tab = (size_t)k * n;
    if (!exact[tab + v]) continue;
    const int32_t c = corr[tab + v];
    if ((uint32_t)c >= (uint32_t)n) { F.bad_link[k] = 1; continue; }
    const GList l = Q.lists[(size_t)(pick.first + (size_t)k * pick.stride) * n + c];
    if ((unsigned long long)l.off + l.cnt > Q.seg_len[k]) { F.bad_list[k] = 1; continue; }
    const MutRec* r = Q.recs + Q.seg_base[k] + l.off;
    for (uint32_t i = 0; i < l.cnt; ++i)
      if (r[i].site == want.site && r[i].from == want.from && r[i].to == want.to) {   // the first in stored order
        const double t = r[i].t;
        sum += t; ++hits; first_t = t < first_t ? t : first_t; last_t = t > last_t ? t : last_t;
        break;
      }
  }
  if (num_with) num_with[j] = hits;
  if (mean_t) mean_t[j] = sum / hits;
  if (t_min) t_min[j] = first_t;
  if (t_max) t_max[j] = last_t;
}

}  // namespace emat
#endif  // EMAT_MCC_SUMMARY_KERNELS_HPP_
