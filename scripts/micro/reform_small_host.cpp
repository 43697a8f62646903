// reform_small_host.cpp -- the register path of a short branch reform (delphy_amd/csrc/emat_reform_pure.hpp: sort_muts_small,
// reform_delta_small) against a literal host copy of the general path's sequence (emat_device_moves.hpp: records that carry their
// source index in `pad`, sort_muts in memory, the two loops of branch_reform_body), bit for bit: the sorted records and the log G
// difference, on random cases per N = 1..4 that include equal new times (with the sites in either order) and new times equal to t_P
// or t_X.
//
//   c++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I delphy_amd/csrc \
//       scripts/micro/reform_small_host.cpp -o reform_small_host && ./reform_small_host [cases per N, default 1000000]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "emat_reform_pure.hpp"

using emat::MutRec;

// ---- today's sequence, copied word for word from the device headers (Ctx-free parts) -------------------------------------------------
static bool mut_less(const MutRec& a, const MutRec& b) { return a.t < b.t || (a.t == b.t && a.site < b.site); }
static void sort_muts(MutRec* p, int n) {
  for (int i = 1; i < n; ++i) { MutRec x = p[i]; int j = i - 1; while (j >= 0 && mut_less(x, p[j])) { p[j + 1] = p[j]; --j; } p[j + 1] = x; }
}
static double general_delta(const double* A, const double* B, const MutRec* old, int n, const MutRec* nm, double lam, double t_X, double t_P) {
  double g_new = -lam * (t_X - t_P), g_old = g_new;
  { const MutRec* m = nm; for (int i = n - 1; i >= 0; --i) { const int j = (int)m[i].pad; g_new -= A[j] * (m[i].t - t_P); g_new += B[j]; } }
  { const MutRec* m = old; for (int i = n - 1; i >= 0; --i) { g_old -= A[i] * (m[i].t - t_P); g_old += B[i]; } }
  return g_new - g_old;
}

// ---- cases ---------------------------------------------------------------------------------------------------------------------------
static uint64_t s_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() { uint64_t z = (s_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static double u01() { return (double)(next64() >> 11) * 0x1.0p-53; }
static MutRec rec(double t, int site, int from, int to, int pad) { MutRec m; m.t = t; m.site = site; m.from = (uint8_t)from; m.to = (uint8_t)to; m.pad = (uint16_t)pad; return m; }

static uint64_t s_ties = 0, s_at_ends = 0, s_moved = 0;

template <int N> static int run(long cases) {
  for (long it = 0; it < cases; ++it) {
    const double t_P = (u01() - 0.5) * 2000.0, t_X = t_P + (next64() % 8 == 0 ? 1e-9 : 1.0) * (0.001 + 300.0 * u01());
    const double lam = 1e-3 * (1.0 + 30.0 * u01());
    double A[N], B[N]; MutRec old[N], nw[N];
    int sites[N];
    for (int i = 0; i < N; ++i) { bool again; do { sites[i] = (int)(next64() % 30000); again = false; for (int k = 0; k < i; ++k) again = again || sites[k] == sites[i]; } while (again); }
    std::vector<double> ot(N);
    for (int i = 0; i < N; ++i) ot[i] = t_P + (t_X - t_P) * u01();
    for (int i = 1; i < N; ++i) { double x = ot[i]; int j = i - 1; while (j >= 0 && ot[j] > x) { ot[j + 1] = ot[j]; --j; } ot[j + 1] = x; }   // a stored list is in time order
    const int mode = (int)(next64() % 8);
    for (int i = 0; i < N; ++i) {
      const int from = (int)(next64() % 4), to = (from + 1 + (int)(next64() % 3)) % 4;
      A[i] = (u01() - 0.5) * 4e-3; B[i] = -6.0 - 8.0 * u01();
      old[i] = rec(ot[i], sites[i], from, to, 0);
      double t = t_P + (t_X - t_P) * u01();
      if (mode == 1 && i > 0 && next64() % 2) t = nw[next64() % i].t;                   // equal new times
      if (mode == 2) t = next64() % 3 == 0 ? t_P : (next64() % 2 ? t_X : t);            // a new time at an end of the branch
      if (mode == 3) t = i % 2 ? t_X : t_P;
      if (mode == 4 && i > 0) t = nw[0].t;                                              // all equal: the order is the sites'
      nw[i] = rec(t, sites[i], from, to, i);
    }
    // the general path: the records in memory, sorted there, the sums through `pad`
    std::vector<MutRec> heap(nw, nw + N);
    sort_muts(heap.data(), N);
    const double want = general_delta(A, B, old, N, heap.data(), lam, t_X, t_P);
    // the register path
    emat::ReformMut ro[N], reg[N];
    for (int i = 0; i < N; ++i) { ro[i].m = old[i]; ro[i].A = A[i]; ro[i].B = B[i]; reg[i] = ro[i]; reg[i].m = nw[i]; }
    emat::sort_muts_small<N>(reg);
    const double got = emat::reform_delta_small<N>(ro, reg, lam, t_X, t_P);
    bool same = std::memcmp(&want, &got, 8) == 0;
    for (int i = 0; i < N; ++i) same = same && std::memcmp(&heap[i], &reg[i].m, sizeof(MutRec)) == 0 && std::memcmp(&A[heap[i].pad], &reg[i].A, 8) == 0 && std::memcmp(&B[heap[i].pad], &reg[i].B, 8) == 0;
    if (!same) {
      std::printf("N=%d case %ld: general %a, registers %a\n", N, it, want, got);
      for (int i = 0; i < N; ++i) std::printf("  [%d] general (t %a site %d src %d)  registers (t %a site %d src %d)\n", i, heap[i].t, heap[i].site, heap[i].pad, reg[i].m.t, reg[i].m.site, reg[i].m.pad);
      return 1;
    }
    for (int i = 0; i < N; ++i) { if (i > 0 && reg[i].m.t == reg[i - 1].m.t) ++s_ties; if (reg[i].m.t == t_P || reg[i].m.t == t_X) ++s_at_ends; if (reg[i].m.pad != i) ++s_moved; }
  }
  return 0;
}

int main(int argc, char** argv) {
  const long cases = argc > 1 ? std::atol(argv[1]) : 1000000;
  if (run<1>(cases) || run<2>(cases) || run<3>(cases) || run<4>(cases)) return 1;
  std::printf("N = 1..4, %ld cases each: sorted records and log G differences equal bit for bit (%" PRIu64 " neighbours with equal times, %" PRIu64 " records at an end of the branch, %" PRIu64 " records moved by the sort)\n",
              cases, s_ties, s_at_ends, s_moved);
  return s_ties > 0 && s_at_ends > 0 && s_moved > 0 ? 0 : 2;
}
