// emat_gamma_pure.hpp -- the site-rate moves' random numbers: a stream named by (key, site) and a gamma sampler on it, as plain C++.
//
// A stream is a (key, site) pair over the engine's Philox4x32-10: block j of site l has counter (l << 32) | j and is two 64-bit words,
// word 0 = x | y << 32, word 1 = z | w << 32, taken in order (as rng_next64_computed takes them).  The stream names the SITE, not the
// thread that draws from it: the same (key, site) gives the same numbers on every handle and with every launch shape.  The alpha steps
// of the site-rate moves draw from the pseudo-site 0xFFFFFFFF.  Uniforms and normals come from those words with the conversions below
// -- THE spelling of them: the moves' u01_* and gaussian (emat_device_core.hpp) use these -- and the Box-Muller of `gaussian`.
//
// No context: compiled for the device (emat_device_core.hpp, emat_site_rate_kernels.hpp) and for the host (scripts/micro/gamma_host.cpp,
// which prints the sampler's moments and its longest rejection loop).
#ifndef EMAT_GAMMA_PURE_HPP_
#define EMAT_GAMMA_PURE_HPP_

#include <cmath>
#include <cstdint>

#ifndef EMAT_HD
#if defined(__HIPCC__)
#define EMAT_HD __host__ __device__ inline __attribute__((always_inline))   // (spelled out: also read by host sources that include no HIP header)
#else
#define EMAT_HD inline
#endif
#endif

namespace emat {

// 64 random bits -> a double in [0, 1), (0, 1) and (0, 1]
EMAT_HD double to_co(uint64_t a) { return (double)(a >> 11) * 0x1.0p-53; }
EMAT_HD double to_oo(uint64_t a) { return ((double)(a >> 12) + 0.5) * 0x1.0p-52; }
EMAT_HD double to_oc(uint64_t a) { return ((double)(a >> 11) + 1.0) * 0x1.0p-53; }

// Philox4x32-10 of (counter, key) with the upper counter words zero: the chains' generator (emat_device_core.hpp: philox4x32_10, the
// same rounds on the device's multiply-high).
EMAT_HD void philox4x32_10_pure(uint64_t ctr, uint64_t key, uint32_t out[4]) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0;
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr uint32_t k_site_stream_alpha = 0xFFFFFFFFu;   // the pseudo-site of the alpha steps

struct SiteStream { uint64_t key; uint32_t site; uint32_t word; uint64_t spare; };   // `word`: 64-bit words taken so far
EMAT_HD SiteStream site_stream(uint64_t key, uint32_t site) { SiteStream s; s.key = key; s.site = site; s.word = 0; s.spare = 0; return s; }
EMAT_HD uint64_t site_stream_next64(SiteStream& s) {
  const uint32_t at = s.word++;
  if (at & 1u) return s.spare;
  uint32_t w[4];
  philox4x32_10_pure(((uint64_t)s.site << 32) | (uint64_t)(at >> 1), s.key, w);
  s.spare = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}
// A standard normal: Box-Muller on two words, as the moves' `gaussian` (one of the pair is used).
EMAT_HD double site_stream_normal(SiteStream& s) {
  const uint64_t a = site_stream_next64(s), b = site_stream_next64(s);
  const double u1 = to_oc(a), u2 = to_co(b);
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586476925 * u2);
}

// Gamma(shape, rate) by Marsaglia & Tsang (ACM TOMS 26, 2000): d = shape - 1/3, c = 1 / sqrt(9 d); v = (1 + c x)^3 of a normal x is
// accepted when u < 1 - 0.0331 x^4 (the squeeze) or log u < x^2 / 2 + d (1 - v + log v).  A shape below 1 is drawn at shape + 1 and
// multiplied by u^(1 / shape), u in the open interval.  A round is accepted with probability above 0.95 for every shape, so the loop's
// bound of 64 rounds is reached with probability below 2^-256; a kernel must not be able to spin, and after the bound the draw is the
// mode of the proposal, d / rate.  `rounds` (may be null) receives the rounds taken.  No floor: what a caller does with a draw that
// underflows belongs to the caller (the site-rate move floors at 1e-50, run.cpp:1140).
constexpr int k_gamma_max_rounds = 64;
EMAT_HD double gamma_draw(double shape, double rate, SiteStream& s, int* rounds = nullptr) {
  const bool boost = shape < 1.0;
  const double a = boost ? shape + 1.0 : shape;
  const double d = a - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
  double g = d;
  int round = 0;
  while (round < k_gamma_max_rounds) {
    ++round;
    const double x = site_stream_normal(s);
    double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = to_oo(site_stream_next64(s));
    const double x2 = x * x;
    if (u < 1.0 - 0.0331 * (x2 * x2) || std::log(u) < 0.5 * x2 + d * (1.0 - v + std::log(v))) { g = d * v; break; }
  }
  if (rounds) *rounds = round;
  if (boost) { const double u = to_oo(site_stream_next64(s)); g *= std::exp(std::log(u) / shape); }
  return g / rate;
}

}  // namespace emat
#endif  // EMAT_GAMMA_PURE_HPP_
