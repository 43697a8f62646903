// draw_arith_host.cpp -- the arithmetic between a random word and what a move does with it: shorter spellings that were tried, beside the
// ones the engine uses, for every word the same bits.  Neither is in the engine: each measured inside the run-to-run spread (DESIGN.md
// section 8, "The chain's frame: scalar loop control"); this program is what a later attempt starts from.
//   * to_oo, ((a >> 12) + 0.5) * 2^-52 (delphy_amd/csrc/emat_gamma_pure.hpp, THE spelling for the device and the host), without a
//     conversion: k = a >> 12 under the exponent of 1.0 is the double 1 + k 2^-52, and taking 1 - 2^-53 from it leaves (2 k + 1) 2^-53,
//     a 53-bit integer times a power of two, hence exact: three device instructions for seven.  to_co and to_oc through one fma of the
//     two 32-bit halves (five instructions for six, if the compiler is kept from widening the conversion of the high half).
//   * uniform_int (emat_device_core.hpp), floor(x n / 2^64), with n's 32 bits taken as unsigned -- mul_hi(lo, n) carried into hi * n, two
//     multiplies -- and with n sign-extended to 64 bits as the engine has it (four), both against the 128-bit product.
// The header's own conversions are held to literal copies of themselves as well, so a change of the header shows here first.
//
// Words: random ones, and the edges of the conversions -- 0, all ones, 2^63, 2^11 - 1, 2^12 - 1, a >> 11 == 2^53 - 1, and the low 11 and
// the low 12 bits all set under every pattern of a 16-bit sweep placed at the top of the word, right above the shifted-out bits, and
// across the boundary between the two 32-bit halves.
//
//   c++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I delphy_amd/csrc
//       scripts/micro/draw_arith_host.cpp -o draw_arith_host && ./draw_arith_host [random words, default 100000000] [random n, default 10000000]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "emat_gamma_pure.hpp"

static uint64_t mix(uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

// ---- the engine's spellings, word for word ---------------------------------------------------------------------------------------------
static double old_to_co(uint64_t a) { return (double)(a >> 11) * 0x1.0p-53; }
static double old_to_oo(uint64_t a) { return ((double)(a >> 12) + 0.5) * 0x1.0p-52; }
static double old_to_oc(uint64_t a) { return ((double)(a >> 11) + 1.0) * 0x1.0p-53; }
// __umul64hi(x, (uint64_t)n) with n an int: the conversion sign-extends
static int old_uniform_int(uint64_t x, int n) { return (int)(uint64_t)(((unsigned __int128)x * (unsigned __int128)(uint64_t)n) >> 64); }

// ---- the shorter conversions (-ffp-contract=off: a fused step is an explicit fma) --------------------------------------------------------
static double new_to_oo(uint64_t a) { const uint64_t b = (a >> 12) | 0x3FF0000000000000ull; double d; std::memcpy(&d, &b, 8); return d - 0x1.fffffffffffffp-1; }
static double new_to_co(uint64_t a) { return __builtin_fma((double)(uint32_t)(a >> 32), 0x1.0p-32, (double)((uint32_t)a >> 11) * 0x1.0p-53); }
static double new_to_oc(uint64_t a) { return __builtin_fma((double)(uint32_t)(a >> 32), 0x1.0p-32, __builtin_fma((double)((uint32_t)a | 0x7FFu), 0x1.0p-64, 0x1.0p-64)); }

// ---- the two-multiply pick, in the 32-bit steps the device would take: __umul64hi(x, (uint64_t)(uint32_t)n) ------------------------------
static int new_uniform_int(uint64_t x, int n) {
  const uint32_t m = (uint32_t)n, lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  const uint32_t carry = (uint32_t)(((uint64_t)lo * m) >> 32);                 // v_mul_hi_u32
  return (int)(uint32_t)(((uint64_t)hi * m + (uint64_t)carry) >> 32);          // v_mad_u64_u32, its high word
}

static uint64_t bits_of(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static uint64_t n_words = 0, n_bad = 0;
static void check_word(uint64_t a) {
  ++n_words;
  const uint64_t co = bits_of(old_to_co(a)), oo = bits_of(old_to_oo(a)), oc = bits_of(old_to_oc(a));
  const bool ok = bits_of(emat::to_co(a)) == co && bits_of(emat::to_oo(a)) == oo && bits_of(emat::to_oc(a)) == oc &&
                  bits_of(new_to_co(a)) == co && bits_of(new_to_oo(a)) == oo && bits_of(new_to_oc(a)) == oc;
  if (!ok && n_bad++ < 10)
    std::printf("MISMATCH word %016" PRIx64 ": co %a / %a / %a  oo %a / %a / %a  oc %a / %a / %a (engine / literal copy / shorter)\n", a, emat::to_co(a), old_to_co(a), new_to_co(a),
                emat::to_oo(a), old_to_oo(a), new_to_oo(a), emat::to_oc(a), old_to_oc(a), new_to_oc(a));
}
static uint64_t n_picks = 0, n_bad_picks = 0;
static void check_pick(uint64_t x, int n) {
  ++n_picks;
  const int want = (int)(uint64_t)(((unsigned __int128)x * (unsigned __int128)(uint32_t)n) >> 64);
  const int got = new_uniform_int(x, n), was = old_uniform_int(x, n);
  if ((got != want || was != want || got < 0 || got >= n) && n_bad_picks++ < 10) std::printf("MISMATCH pick x %016" PRIx64 " n %d: new %d old %d exact %d\n", x, n, got, was, want);
}

int main(int argc, char** argv) {
  const uint64_t random_words = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000000ull;
  const uint64_t random_n = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 10000000ull;

  const uint64_t edges[] = {0ull, ~0ull, 1ull << 63, (1ull << 11) - 1, (1ull << 12) - 1, 1ull << 11, 1ull << 12, ((1ull << 53) - 1) << 11, (((1ull << 53) - 1) << 11) | 0x7FFull,
                            ((1ull << 52) - 1) << 12, 0xFFFFFFFFull, 1ull << 32, 0x7FFFFFFFFFFFFFFFull};
  for (uint64_t e : edges) check_word(e);
  uint64_t n_edge = sizeof(edges) / sizeof(edges[0]);
  const uint64_t lows[] = {0x7FFull, 0xFFFull};
  for (uint64_t low : lows) {
    const int at[] = {48, 11, 12, 24};   // the sweep at the top, right above the bits shifted out (11, 12), and across bit 32
    for (int sh : at)
      for (uint64_t h = 0; h < (1ull << 16); ++h) { check_word((h << sh) | low); check_word((~0ull << 44) | (h << sh) | low); n_edge += 2; }
  }
  uint64_t s = 0x243F6A8885A308D3ull;
  for (uint64_t i = 0; i < random_words; ++i) { s = mix(s); check_word(s); }
  std::printf("conversions: %" PRIu64 " words (%" PRIu64 " edge words), %" PRIu64 " mismatches\n", n_words, n_edge, n_bad);

  const int fixed_n[] = {1, 2, 3, 4, 63, 64, 65, 1 << 15, 0x7FFFFFFF};
  for (int n : fixed_n) {
    check_pick(0ull, n); check_pick(~0ull, n);
    for (int i = 0; i < 100000; ++i) { s = mix(s); check_pick(s, n); }
  }
  for (uint64_t i = 0; i < random_n; ++i) {
    s = mix(s);
    const int n = 1 + (int)(s % 0x7FFFFFFFull);   // [1, 2^31)
    s = mix(s);
    check_pick(s, n); check_pick(0ull, n); check_pick(~0ull, n);
  }
  std::printf("uniform_int: %" PRIu64 " picks, %" PRIu64 " mismatches\n", n_picks, n_bad_picks);
  const bool ok = n_bad == 0 && n_bad_picks == 0;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
