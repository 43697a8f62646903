// emat_mcc_kernels.hpp -- the maximum-clade-credibility (MCC) tree of the sampled trees kept in HBM.
//
// Reference: derive_mcc_tree and Mcc_tree::calculate_derived_quantities (core/mcc_tree.cpp:58-181), on base trees that here are
// slots of a store of (parent, child0, child1, t, root) snapshots of the resident tree, 20 bytes a node (emat_mcc_host.hpp).
// M = number of chosen samples, n = nodes of every sample; sample k of a derivation is slot first + k * stride.
//
// 1. Tip fingerprints (mcc_tree.cpp:70-76): 64 bits from a counter-based generator of (seed, node index): the SplitMix64
//    finaliser of seed + (node + 1) * 0x9e3779b97f4a7c15.  Nothing is stored: whoever needs a tip's fingerprint computes it.
//    A clade's fingerprint is the XOR of its tips', so two DIFFERENT clades among the (at most M n) of a derivation share one
//    with probability ~ (M n)^2 / 2^65 (3e-4 at M = 1000, n = 1e5), as in the reference, which uses the same 64 bits.
// 2. Clade fingerprints and tip counts of every node of every sample (calc_inner_node_clade_fingerprints, :30-41): a climb
//    with an arrival counter (k_mcc_climb_clades).  One thread per (sample, tip) walks towards the root; at a parent it XORs
//    its fingerprint into the parent's word and then adds its tip count to the parent's count.  That add is the arrival
//    counter: tip counts are positive, so whoever gets 0 back came first and stops, and whoever gets something else back
//    came second, knows the node's tip count (old + own), fetches the combined fingerprint and carries on.  No thread waits
//    for another.  Every word two workgroups share within the launch is touched by agent-scope atomics only -- the per-XCD
//    L2s are not coherent for plain accesses -- and the add is acquire-release, so the first arriver's XOR is ahead of it.
//    XOR and integer addition have no order, so the bits do not depend on the schedule.
// 3. Clade counts (count_base_trees_for_each_clade, :43-56): an open-addressing table in HBM keyed by fingerprint, 64-bit
//    compare-and-swap to claim a slot, 32-bit integer add to count (k_mcc_count).  Chosen over sort + run lengths because the
//    library links nothing beyond the HIP runtime and a table is two dozen lines, where a 64-bit radix sort of M n keys is a
//    library of its own; and because most keys repeat (a clade that is in every sample is one entry, not M), so the table is
//    sized by the DISTINCT clades.  The empty slot is key 0; fingerprint 0 is counted in a word of its own.  A probe sequence
//    longer than k_mcc_max_probe, or more distinct keys than half the slots, makes the host quadruple the table and refill it.
// 4. Per sample the histogram hist[k][c] = number of inner nodes whose clade occurs in c samples (k_mcc_hist; :78-103): integers,
//    summed per block in LDS and then with integer atomics.  The host turns it into log clade credibility and picks the master.
// 5. Corresponding nodes (:118-147): a second climb with an arrival counter, over the MCC tree (= the master's topology), one thread
//    per (sample, tip) (k_mcc_climb_corr).  What travels up is the node of the sample that is the MRCA of the tips below the MCC node;
//    a thread EXCHANGES its value (+ 1) into the MCC parent's word: 0 back means first, stop; anything else is the sibling's value,
//    and the second arriver walks the two up to their MRCA in the sample and carries on.  One atomic word is both counter and
//    payload.  The walk does not compare node times as find_MRCA_of does (phylo_tree.cpp:204-240; equal times need its special
//    case) but the tip counts of step 2, which grow STRICTLY towards the root: the node with the smaller count cannot be an
//    ancestor of the other, so it steps up; with equal counts and different nodes neither can, so both do.  The MRCA is unique,
//    so the result is find_MRCA_of's.  Exact match = fingerprints equal.
// 6. Derived quantities (:158-179): one thread per MCC node loops over the samples IN ORDER, so support, t and t_mrca are the
//    doubles the reference's loop gives (k_mcc_derived).
//
// Bounds: every climb and every walk is a loop of at most n steps that checks the node index it is about to follow; the host
// has validated every tree that came from host arrays, and a step outside the tree sets the status word instead of being taken.
//
// Included by emat_backend.hip after emat_gtree_kernels.hpp (GTreeDev).
#ifndef EMAT_MCC_KERNELS_HPP_
#define EMAT_MCC_KERNELS_HPP_

namespace emat {

struct MccStore {                    // the slots: arrays of capacity * n, slot-major
  int32_t* parent; int32_t* c0; int32_t* c1; double* t; int32_t* root;
  int32_t n;
};
struct MccPick { int32_t first, stride, M; };                    // the samples of one derivation
struct MccTable { unsigned long long* keys; int32_t* counts; int32_t* info; uint32_t mask; int32_t shift; };   // info: [0] status, [1] distinct keys, [2] count of fingerprint 0
enum MccStatus : int32_t { k_mcc_ok = 0, k_mcc_table_full = 1, k_mcc_bad_link = 2, k_mcc_key_missing = 4 };
constexpr uint32_t k_mcc_max_probe = 256;
constexpr int k_mcc_lds_hist = 2048;

#define EMAT_MCC_AGENT __HIP_MEMORY_SCOPE_AGENT

__device__ inline unsigned long long mcc_tip_fingerprint(unsigned long long seed, int32_t node) {
  unsigned long long z = seed + (unsigned long long)(node + 1) * 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ inline uint32_t mcc_slot_of(const MccTable& T, unsigned long long key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> T.shift) & T.mask; }

// emat_tree_sample_push: the resident tree's links and times into a slot.
__global__ void __launch_bounds__(256) k_mcc_push(GTreeDev g, MccStore S, int32_t slot) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= S.n) return;
  const size_t o = (size_t)slot * S.n + v;
  S.parent[o] = g.parent[v]; S.c0[o] = g.c0[v]; S.c1[o] = g.c1[v]; S.t[o] = g.t[v];
  if (v == 0) S.root[slot] = g.root[0];
}

// Step 2.  fp / ntips [M * n], zeroed before the launch.
__global__ void __launch_bounds__(256) k_mcc_climb_clades(MccStore S, MccPick pick, unsigned long long seed, unsigned long long* fp, int32_t* ntips, int32_t* info) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = S.n;
  if (v >= n) return;
  for (int k = blockIdx.y; k < pick.M; k += gridDim.y) {
    const size_t in = (size_t)(pick.first + (size_t)k * pick.stride) * n, out = (size_t)k * n;
    if (S.c0[in + v] >= 0) continue;                       // tips climb
    unsigned long long f = mcc_tip_fingerprint(seed, v);
    int32_t cnt = 1, u = v;
    fp[out + v] = f; ntips[out + v] = 1;                   // (a tip's own words: nobody else touches them in this launch)
    for (int step = 0; step < n; ++step) {
      const int32_t p = S.parent[in + u];
      if (p < 0) break;
      if (p >= n) { atomicOr(&info[0], (int32_t)k_mcc_bad_link); break; }
      __hip_atomic_fetch_xor(&fp[out + p], f, __ATOMIC_RELAXED, EMAT_MCC_AGENT);
      const int32_t old = __hip_atomic_fetch_add(&ntips[out + p], cnt, __ATOMIC_ACQ_REL, EMAT_MCC_AGENT);
      if (old == 0) break;                                 // first to arrive: the other child's thread carries on from here
      cnt += old;
      f = __hip_atomic_fetch_xor(&fp[out + p], 0ull, __ATOMIC_RELAXED, EMAT_MCC_AGENT);   // the combined value, from where the atomics are made
      u = p;
    }
  }
}

// Step 3.  Every node of every sample, tips included, as the reference counts them.
__global__ void __launch_bounds__(256) k_mcc_count(int32_t n, int32_t M, const unsigned long long* fp, MccTable T) {
  const size_t total = (size_t)n * M;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = fp[i];
    if (key == 0ull) { atomicAdd(&T.info[2], 1); continue; }
    uint32_t s = mcc_slot_of(T, key), probe = 0;
    for (;; s = (s + 1) & T.mask) {
      unsigned long long seen = __hip_atomic_load(&T.keys[s], __ATOMIC_RELAXED, EMAT_MCC_AGENT);
      if (seen == 0ull) {
        unsigned long long expected = 0ull;
        if (__hip_atomic_compare_exchange_strong(&T.keys[s], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, EMAT_MCC_AGENT)) { seen = key; atomicAdd(&T.info[1], 1); }
        else seen = expected;
      }
      if (seen == key) { atomicAdd(&T.counts[s], 1); break; }
      if (++probe > k_mcc_max_probe || probe > T.mask) { atomicOr(&T.info[0], (int32_t)k_mcc_table_full); break; }
    }
  }
}
__device__ inline int32_t mcc_count_of(const MccTable& T, unsigned long long key) {
  if (key == 0ull) return T.info[2];
  uint32_t s = mcc_slot_of(T, key);
  for (uint32_t probe = 0; probe <= k_mcc_max_probe + 1 && probe <= T.mask; ++probe, s = (s + 1) & T.mask) {
    const unsigned long long seen = T.keys[s];
    if (seen == key) return T.counts[s];
    if (seen == 0ull) break;
  }
  return -1;
}

// Step 4.  hist [M * (M + 1)], zeroed before the launch; blockIdx.y strides over the samples, blockIdx.x over their nodes.
__global__ void __launch_bounds__(256) k_mcc_hist(MccStore S, MccPick pick, const unsigned long long* fp, MccTable T, int32_t* hist) {
  __shared__ int32_t lh[k_mcc_lds_hist];
  const int n = S.n, M = pick.M;
  const bool in_lds = M + 1 <= k_mcc_lds_hist;             // (uniform)
  for (int k = blockIdx.y; k < M; k += gridDim.y) {
    const size_t in = (size_t)(pick.first + (size_t)k * pick.stride) * n, out = (size_t)k * n;
    int32_t* gh = hist + (size_t)k * (M + 1);
    if (in_lds) { for (int c = threadIdx.x; c <= M; c += blockDim.x) lh[c] = 0; __syncthreads(); }
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
      if (S.c0[in + v] < 0) continue;                      // (all tips contribute equally: the reference leaves them out)
      const int32_t c = mcc_count_of(T, fp[out + v]);
      if (c < 1 || c > M) { atomicOr(&T.info[0], (int32_t)k_mcc_key_missing); continue; }
      if (in_lds) atomicAdd(&lh[c], 1); else atomicAdd(&gh[c], 1);
    }
    if (in_lds) {
      __syncthreads();
      for (int c = threadIdx.x; c <= M; c += blockDim.x) if (lh[c]) atomicAdd(&gh[c], lh[c]);
      __syncthreads();
    }
  }
}

// find_MRCA_of(sample, a, b) by tip counts (header, step 5); -1 if a link leaves the tree.
__device__ inline int32_t mcc_mrca(const int32_t* parent, const int32_t* ntips, int32_t n, int32_t a, int32_t b) {
  for (int step = 0; step < 2 * n && a != b; ++step) {
    const int32_t na = ntips[a], nb = ntips[b];
    if (na <= nb) { a = parent[a]; if (a < 0 || a >= n) return -1; }
    if (nb <= na) { b = parent[b]; if (b < 0 || b >= n) return -1; }
  }
  return a == b ? a : -1;
}

// Step 5.  arrive [M * n] zeroed before the launch; corr [M * n], exact [M * n] written for every node.  `master` is the slot whose
// topology the MCC tree has; master_fp its rows of fp (sample position `master_k`).
__global__ void __launch_bounds__(256) k_mcc_climb_corr(MccStore S, MccPick pick, int32_t master_k, const unsigned long long* fp, const int32_t* ntips,
                                                         int32_t* arrive, int32_t* corr, uint8_t* exact, int32_t* info) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = S.n;
  if (v >= n) return;
  const size_t min_ = (size_t)(pick.first + (size_t)master_k * pick.stride) * n;
  if (S.c0[min_ + v] >= 0) return;                         // tips of the MCC tree (the same nodes in every sample) climb
  const int32_t* mpar = S.parent + min_;
  const unsigned long long* mfp = fp + (size_t)master_k * n;
  for (int k = blockIdx.y; k < pick.M; k += gridDim.y) {
    const size_t in = (size_t)(pick.first + (size_t)k * pick.stride) * n, out = (size_t)k * n;
    corr[out + v] = v; exact[out + v] = 1;                 // tips correspond to themselves, always
    int32_t mine = v, u = v;
    for (int step = 0; step < n; ++step) {
      const int32_t p = mpar[u];
      if (p < 0) break;
      if (p >= n) { atomicOr(&info[0], (int32_t)k_mcc_bad_link); break; }
      const int32_t other = __hip_atomic_exchange(&arrive[out + p], mine + 1, __ATOMIC_ACQ_REL, EMAT_MCC_AGENT);
      if (other == 0) break;                               // first to arrive
      mine = mcc_mrca(S.parent + in, ntips + out, n, mine, other - 1);
      if (mine < 0) { atomicOr(&info[0], (int32_t)k_mcc_bad_link); break; }
      corr[out + p] = mine; exact[out + p] = fp[out + mine] == mfp[p] ? 1 : 0;   // (read by later launches only)
      u = p;
    }
  }
}

// Step 6.  One thread per MCC node, the samples in order.
__global__ void __launch_bounds__(256) k_mcc_derived(MccStore S, MccPick pick, const int32_t* corr, const uint8_t* exact,
                                                      double* support, double* t, double* t_mrca, int32_t* num_exact) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = S.n;
  if (v >= n) return;
  double sum_t = 0.0, sum_t_mrca = 0.0;
  int32_t hits = 0;
  for (int k = 0; k < pick.M; ++k) {
    const size_t in = (size_t)(pick.first + (size_t)k * pick.stride) * n, out = (size_t)k * n;
    const int32_t c = corr[out + v];
    const double tc = S.t[in + c];
    sum_t_mrca += tc;
    if (exact[out + v]) { sum_t += tc; ++hits; }
  }
  support[v] = (double)hits / pick.M;
  t[v] = sum_t / hits;
  t_mrca[v] = sum_t_mrca / pick.M;
  num_exact[v] = hits;
}

}  // namespace emat
#endif  // EMAT_MCC_KERNELS_HPP_
