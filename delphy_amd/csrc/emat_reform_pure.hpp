// emat_reform_pure.hpp -- the arithmetic of a branch reform that re-times at most four mutations, without the context: the order of
// two mutation records, the stable insertion sort of N of them and the two sums of the move's log G difference.
//
// Plain C++ on emat_slab.hpp's records, compiled for the device (branch_reform_small, emat_device_moves.hpp) and for the host
// (scripts/micro/reform_small_host.cpp, which holds it bit for bit to the general path's sequence: records that carry their source index
// in `pad`, sort_muts in memory, the two loops over arrays).  Everything is indexed with compile-time constants after unrolling, so on the
// device the records and factors stay in registers: an index known only at run time would put the array in private memory.
#ifndef EMAT_REFORM_PURE_HPP_
#define EMAT_REFORM_PURE_HPP_

#include "emat_slab.hpp"

#if defined(__HIPCC__)
#define EMAT_HD __host__ __device__ __forceinline__
#else
#define EMAT_HD inline
#endif

namespace emat {

// mutations.h:41-43: by time, then by site (strict)
EMAT_HD bool mut_before(const MutRec& a, const MutRec& b) { return a.t < b.t || (a.t == b.t && a.site < b.site); }

// A mutation of the branch with its two factors (mut_factors): the factors travel with the record through the sort, so the sum over
// the sorted list needs no look-up by source index.
struct ReformMut { MutRec m; double A, B; };

// `a` if `first`, else `b`: field by field, so that neither needs an address
EMAT_HD ReformMut reform_either(bool first, const ReformMut& a, const ReformMut& b) {
  ReformMut r;
  r.m.t = first ? a.m.t : b.m.t; r.m.site = first ? a.m.site : b.m.site; r.m.from = first ? a.m.from : b.m.from; r.m.to = first ? a.m.to : b.m.to; r.m.pad = first ? a.m.pad : b.m.pad;
  r.A = first ? a.A : b.A; r.B = first ? a.B : b.B;
  return r;
}

// sort_muts (emat_device_core.hpp) unrolled: element i walks down while it is before its lower neighbour and stops at the first that it
// is not before -- the same comparisons with the same outcomes, so records that compare equal keep their order exactly as there.
template <int N> EMAT_HD void sort_muts_small(ReformMut (&m)[N]) {
#pragma unroll
  for (int i = 1; i < N; ++i) {
    bool walking = true;
#pragma unroll
    for (int j = i - 1; j >= 0; --j) {
      walking = walking && mut_before(m[j + 1].m, m[j].m);
      const ReformMut a = m[j], b = m[j + 1];
      m[j] = reform_either(walking, b, a); m[j + 1] = reform_either(walking, a, b);
    }
  }
}

// log G of the branch with the re-timed list minus log G with the old one (branch_reform_body's two loops): `old` in the list's order,
// `nw` sorted; both hold the same mutations with the same factors.
template <int N> EMAT_HD double reform_delta_small(const ReformMut (&old)[N], const ReformMut (&nw)[N], double lam, double t_X, double t_P) {
  double g_new = -lam * (t_X - t_P), g_old = g_new;
#pragma unroll
  for (int i = N - 1; i >= 0; --i) { g_new -= nw[i].A * (nw[i].m.t - t_P); g_new += nw[i].B; }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) { g_old -= old[i].A * (old[i].m.t - t_P); g_old += old[i].B; }
  return g_new - g_old;
}

}  // namespace emat
#endif
