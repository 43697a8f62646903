// emat_align_kernels.hpp -- an aligned FASTA's rows on the device: coding and packing, per-site state counts, the consensus, and every
// tip's differences from the reference sequence and missing intervals (reference core/io.cpp:14-97 read_fasta, core/cmdline.cpp:26-85
// fasta_to_maple, core/sequence_utils.h:44-80 deduce_consensus_sequence, core/sequence_utils.cpp:30-64 calculate_delta_from_reference).
//
// The store holds a row as 4-bit codes, Seq_letters' bit sets (core/sequence.h:21-29: A 1, C 2, G 4, T 8, N 15), two sites a byte, site 2k in
// the low half of byte k; a row takes ceil(L/2) bytes and starts on a byte.  Code 0 stands for a character that is no sequence letter.
//   k_al_code       a chunk of ASCII rows -> packed codes.  A lane owns one byte of a row = two sites, over k_al_tile_rows rows; a character that
//                   fails is_valid_seq_letter leaves (site << 8 | byte) in the row's `bad` word through atomicMin: the smallest site wins.
//   k_al_count      counts[site][state] += unambiguous states over the chunk's rows whose `bad` word is untouched.  Per-lane registers over the
//                   rows of a tile, then one integer atomicAdd per (site, state) and workgroup: the same counts from every chunking and launch shape.
//   k_al_consensus  per site the state with the largest count, ties to A, C, G, T in that order, an all-zero site A.
//   k_al_tip_count  one wavefront per tip: deltas, intervals and ambiguous codes other than N of its row.  A lane owns 16 sites through one
//                   8-byte load; an interval starts at an ambiguous site whose left neighbour is not (or at site 0), and ends at a site that is
//                   not ambiguous (or at L) whose left neighbour is.  Counts and ranks are popcounts of the lane's masks and a prefix over the wave.
//   k_al_scan       exclusive scan of the two per-tip counts, in 64 bits (the host refuses totals beyond int32 before anything is written).
//   k_al_tip_write  the walk of k_al_tip_count again, placing every record at offset[tip] + its rank within the row.
// No floating point, no data-dependent loop, no spinning: every trip count is a function of L and of the row counts.
//
// Included by emat_backend.hip after the other kernel headers: everything in here is device code (csrc/Makefile: DEVSRC).
#ifndef EMAT_ALIGN_KERNELS_HPP_
#define EMAT_ALIGN_KERNELS_HPP_

#include <hip/hip_runtime.h>
#include <cstdint>

namespace emat {

constexpr int k_al_threads = 256;                       // k_al_code, k_al_count: 256 lanes x 2 sites
constexpr int k_al_tile_sites = 2 * k_al_threads;
constexpr int k_al_tile_rows = 64;                      // rows a workgroup of those two walks
constexpr int k_al_wave = 64;                           // k_al_tip_count, k_al_tip_write: one wavefront per tip
constexpr int k_al_lane_sites = 16;                     // ... each lane 16 sites = 8 packed bytes
constexpr int k_al_pass_sites = k_al_wave * k_al_lane_sites;
constexpr int k_al_scan_threads = 1024;
constexpr int k_al_row_pad = 8;                         // bytes after the last row, so that its last 8-byte load stays inside the store
constexpr unsigned long long k_al_row_ok = ~0ull;       // a row's `bad` word while every character was a sequence letter

// to_seq_letter's table (core/sequence.h:115-153), 0 where is_valid_seq_letter (:77-113) says no.  Case-insensitive; U = T; N - ? . all N.
__host__ __device__ inline uint8_t al_code_of(unsigned c) {
  if (c >= 'a' && c <= 'z') c -= 'a' - 'A';
  switch (c) {
    case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': case 'U': return 8;
    case 'R': return 1 | 4; case 'Y': return 2 | 8; case 'S': return 4 | 2; case 'W': return 1 | 8; case 'K': return 4 | 8; case 'M': return 1 | 2;
    case 'B': return 2 | 4 | 8; case 'D': return 1 | 4 | 8; case 'H': return 1 | 2 | 8; case 'V': return 1 | 2 | 4;
    case 'N': case '-': case '?': case '.': return 15;
    default: return 0;
  }
}

struct AlignStore {
  int32_t L; int64_t row_bytes;          // sites; ceil(L / 2)
  uint8_t* packed;                       // [max_rows x row_bytes + k_al_row_pad]
  unsigned long long* bad;               // [max_rows] k_al_row_ok, or (first bad site << 8 | its byte)
  int32_t* counts;                       // [L][4]
};

__global__ __launch_bounds__(k_al_threads) void k_al_code(AlignStore s, const uint8_t* chars, int64_t row_stride, int64_t first_row, int32_t num_rows, int32_t site_tiles) {
  __shared__ uint8_t table[256];
  table[threadIdx.x] = al_code_of(threadIdx.x);
  __syncthreads();
  const int64_t tile = (int64_t)blockIdx.x / site_tiles;
  const int32_t site = (int32_t)(blockIdx.x % (unsigned)site_tiles) * k_al_tile_sites + 2 * (int32_t)threadIdx.x;
  if (site >= s.L) return;
  const bool two = site + 1 < s.L;
  const int32_t r0 = (int32_t)(tile * k_al_tile_rows);
  for (int k = 0; k < k_al_tile_rows; ++k) {
    const int32_t r = r0 + k;
    if (r >= num_rows) break;
    const uint8_t* row = chars + (int64_t)r * row_stride;
    const unsigned c0 = row[site], c1 = two ? row[site + 1] : (unsigned)'A';
    const unsigned a = table[c0], b = two ? table[c1] : 0u;
    s.packed[(first_row + r) * s.row_bytes + (site >> 1)] = (uint8_t)(a | (b << 4));
    if (a == 0 || (two && b == 0)) {
      const unsigned long long w = a == 0 ? ((unsigned long long)site << 8 | c0) : ((unsigned long long)(site + 1) << 8 | c1);
      atomicMin(&s.bad[first_row + r], w);
    }
  }
}

__device__ inline void al_count_code(unsigned code, int32_t (&n)[4]) {
  n[0] += code == 1; n[1] += code == 2; n[2] += code == 4; n[3] += code == 8;
}

__global__ __launch_bounds__(k_al_threads) void k_al_count(AlignStore s, int64_t first_row, int32_t num_rows, int32_t site_tiles) {
  const int64_t tile = (int64_t)blockIdx.x / site_tiles;
  const int32_t site = (int32_t)(blockIdx.x % (unsigned)site_tiles) * k_al_tile_sites + 2 * (int32_t)threadIdx.x;
  if (site >= s.L) return;
  const int32_t r0 = (int32_t)(tile * k_al_tile_rows);
  int32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
  for (int k = 0; k < k_al_tile_rows; ++k) {
    const int32_t r = r0 + k;
    if (r >= num_rows) break;
    if (s.bad[first_row + r] != k_al_row_ok) continue;   // (the same for every lane)
    const unsigned v = s.packed[(first_row + r) * s.row_bytes + (site >> 1)];
    al_count_code(v & 15u, lo); al_count_code(v >> 4, hi);   // (the upper half of an odd L's last byte is code 0)
  }
  for (int a = 0; a < 4; ++a) {
    if (lo[a]) atomicAdd(&s.counts[(int64_t)site * 4 + a], lo[a]);
    if (hi[a]) atomicAdd(&s.counts[(int64_t)(site + 1) * 4 + a], hi[a]);   // (hi stays 0 beyond L)
  }
}

__global__ __launch_bounds__(k_al_threads) void k_al_consensus(const int32_t* counts, uint8_t* ref, int32_t L) {
  const int64_t l = (int64_t)blockIdx.x * k_al_threads + threadIdx.x;
  if (l >= L) return;
  int32_t best = counts[l * 4]; uint8_t state = 0;
  for (int a = 1; a < 4; ++a) { const int32_t c = counts[l * 4 + a]; if (c > best) { best = c; state = (uint8_t)a; } }
  ref[l] = state;
}

// What a lane knows of its 16 sites l0 .. l0 + 15 of one row: bit i belongs to site l0 + i.
struct AlLaneMasks { unsigned amb, delta, not_n; uint64_t codes; };

__device__ inline AlLaneMasks al_lane_masks(const uint8_t* row, const uint8_t* ref, int32_t l0, int32_t L) {
  AlLaneMasks m{0u, 0u, 0u, 0ull};
  if (l0 >= L) return m;
  __builtin_memcpy(&m.codes, row + (l0 >> 1), 8);   // (l0 is a multiple of 16; the row itself starts on any byte)
  uint8_t r[k_al_lane_sites];
  __builtin_memcpy(r, ref + l0, k_al_lane_sites);    // (ref has room for a multiple of 16 sites)
  const int n = L - l0 < k_al_lane_sites ? L - l0 : k_al_lane_sites;
#pragma unroll
  for (int i = 0; i < k_al_lane_sites; ++i) {
    const unsigned c = (unsigned)(m.codes >> (4 * i)) & 15u;
    const bool in = i < n, amb = (c & (c - 1u)) != 0u;
    m.amb |= (unsigned)(in && amb) << i;
    m.not_n |= (unsigned)(in && amb && c != 15u) << i;
    m.delta |= (unsigned)(in && !amb && c != (1u << r[i])) << i;
  }
  return m;
}

__device__ inline int al_wave_inclusive(int v, int lane) {
#pragma unroll
  for (int d = 1; d < k_al_wave; d <<= 1) { const int o = __shfl_up(v, d, k_al_wave); if (lane >= d) v += o; }
  return v;
}

struct AlignTips {
  int32_t L; int64_t row_bytes; int32_t num_tips;
  const uint8_t* packed; const uint8_t* ref; const int32_t* tip_row;
  int32_t* n_delta; int32_t* n_iv; int32_t* n_not_n;     // [num_tips]
  const int32_t* delta_off; const int32_t* miss_off;     // [num_tips + 1], k_al_scan's
  int32_t* delta_site; uint8_t* delta_to; int32_t* miss_start; int32_t* miss_end;
};

// One wavefront over one tip's row: sites 0 .. L, L standing for a site that is not ambiguous (it ends a run that reaches L - 1).
template <bool write> __device__ inline void al_walk_tip(const AlignTips& a) {
  const int tip = (int)blockIdx.x, lane = (int)threadIdx.x;
  const uint8_t* row = a.packed + (int64_t)a.tip_row[tip] * a.row_bytes;
  const int passes = (int)(((int64_t)a.L + 1 + k_al_pass_sites - 1) / k_al_pass_sites);
  int nd = 0, ni = 0, nn = 0;          // records of the passes before this one (the same in every lane)
  unsigned carry = 0;                  // was the last site of the pass before ambiguous?
  int d_base = 0, m_base = 0;
  if (write) { d_base = a.delta_off[tip]; m_base = a.miss_off[tip]; }
  for (int p = 0; p < passes; ++p) {
    const int32_t l0 = p * k_al_pass_sites + lane * k_al_lane_sites;
    const AlLaneMasks m = al_lane_masks(row, a.ref, l0, a.L);
    const unsigned top = m.amb >> (k_al_lane_sites - 1);
    unsigned left = (unsigned)__shfl_up((int)top, 1, k_al_wave);
    if (lane == 0) left = carry;
    carry = (unsigned)__shfl((int)top, k_al_wave - 1, k_al_wave);
    const unsigned shifted = ((m.amb << 1) | left) & 0xFFFFu;   // bit i: site l0 + i - 1 is ambiguous
    const unsigned starts = m.amb & ~shifted;
    const unsigned ends = ~m.amb & shifted;                      // (a site at or beyond L is never ambiguous: of those only L itself can end a run)
    const int cd = __popc(m.delta), cs = __popc(starts), ce = __popc(ends);
    const int sd = al_wave_inclusive(cd, lane), ss = al_wave_inclusive(cs, lane), se = al_wave_inclusive(ce, lane);
    if (write) {
      int k = d_base + nd + sd - cd;
      for (unsigned b = m.delta; b; b &= b - 1u) {
        const int i = __ffs((int)b) - 1;
        a.delta_site[k] = l0 + i; a.delta_to[k] = (uint8_t)(__ffs((int)((unsigned)(m.codes >> (4 * i)) & 15u)) - 1); ++k;
      }
      k = m_base + ni + ss - cs;
      for (unsigned b = starts; b; b &= b - 1u) a.miss_start[k++] = l0 + __ffs((int)b) - 1;
      k = m_base + nn + se - ce;
      for (unsigned b = ends; b; b &= b - 1u) a.miss_end[k++] = l0 + __ffs((int)b) - 1;
      nn += __shfl(se, k_al_wave - 1, k_al_wave);
    } else {
      nn += __shfl(al_wave_inclusive(__popc(m.not_n), lane), k_al_wave - 1, k_al_wave);
    }
    nd += __shfl(sd, k_al_wave - 1, k_al_wave); ni += __shfl(ss, k_al_wave - 1, k_al_wave);
  }
  if (!write && lane == 0) { a.n_delta[tip] = nd; a.n_iv[tip] = ni; a.n_not_n[tip] = nn; }
}

__global__ __launch_bounds__(k_al_wave) void k_al_tip_count(AlignTips a) { al_walk_tip<false>(a); }
__global__ __launch_bounds__(k_al_wave) void k_al_tip_write(AlignTips a) { al_walk_tip<true>(a); }

// ONE workgroup: off[t] = sum of n[< t] for both count arrays, as int32 (meaningful only while the totals fit, which the host checks), totals[0..1] in 64 bits.
__global__ __launch_bounds__(k_al_scan_threads) void k_al_scan(const int32_t* n_delta, const int32_t* n_iv, int32_t num_tips, int32_t* delta_off, int32_t* miss_off, long long* totals) {
  __shared__ long long part[2][k_al_scan_threads];
  __shared__ long long base[2];
  const int t = (int)threadIdx.x;
  if (t == 0) { base[0] = 0; base[1] = 0; }
  __syncthreads();
  const int rounds = (num_tips + k_al_scan_threads - 1) / k_al_scan_threads;
  for (int r = 0; r < rounds; ++r) {
    const int i = r * k_al_scan_threads + t;
    const long long vd = i < num_tips ? n_delta[i] : 0, vi = i < num_tips ? n_iv[i] : 0;
    part[0][t] = vd; part[1][t] = vi;
    __syncthreads();
    for (int d = 1; d < k_al_scan_threads; d <<= 1) {   // Hillis-Steele, inclusive
      const long long od = t >= d ? part[0][t - d] : 0, oi = t >= d ? part[1][t - d] : 0;
      __syncthreads();
      part[0][t] += od; part[1][t] += oi;
      __syncthreads();
    }
    if (i < num_tips) { delta_off[i] = (int32_t)(base[0] + part[0][t] - vd); miss_off[i] = (int32_t)(base[1] + part[1][t] - vi); }
    __syncthreads();
    if (t == k_al_scan_threads - 1) { base[0] += part[0][t]; base[1] += part[1][t]; }
    __syncthreads();
  }
  if (t == 0) { delta_off[num_tips] = (int32_t)base[0]; miss_off[num_tips] = (int32_t)base[1]; totals[0] = base[0]; totals[1] = base[1]; }
}

}  // namespace emat

#endif  // EMAT_ALIGN_KERNELS_HPP_
