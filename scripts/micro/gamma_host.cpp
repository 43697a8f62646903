// gamma_host.cpp -- the site-rate moves' gamma sampler (delphy_amd/csrc/emat_gamma_pure.hpp: site_stream, gamma_draw) compiled for the
// host: per shape, draw i from the stream (key, i) as emat_debug_sample_gamma draws it on the device, and print the sample's mean and
// variance beside shape / rate and shape / rate^2 (in standard errors), the smallest and largest draw, how many draws were zero, not
// finite or below the move's floor of 1e-50, and the longest rejection loop (bounded at k_gamma_max_rounds).  The run fails (exit
// status 1) when a mean or variance is more than six standard errors off, a draw is negative or not finite, or a loop reached its bound.
//
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I delphy_amd/csrc
//       scripts/micro/gamma_host.cpp -o gamma_host && ./gamma_host [draws per shape, default 1000000] [key, default 1]
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "emat_gamma_pure.hpp"

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 1000000;
  const uint64_t key = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  const double shapes[] = {0.02, 0.2, 0.5, 1.0, 1.7, 30.0, 5000.3};
  const double rate = 3.0;
  int bad = 0;
  for (double shape : shapes) {
    double mean = 0.0, m2 = 0.0, m4 = 0.0, lo = INFINITY, hi = 0.0;
    long zeros = 0, not_finite = 0, negative = 0, floored = 0;
    int max_rounds = 0;
    const double want_mean = shape / rate, want_var = shape / (rate * rate);
    for (long i = 0; i < n; ++i) {
      emat::SiteStream s = emat::site_stream(key, (uint32_t)i);
      int rounds = 0;
      const double x = emat::gamma_draw(shape, rate, s, &rounds);
      if (rounds > max_rounds) max_rounds = rounds;
      if (!std::isfinite(x)) { ++not_finite; continue; }
      if (x < 0.0) ++negative;
      if (x == 0.0) ++zeros;
      if (x < 1e-50) ++floored;
      if (x < lo) lo = x;
      if (x > hi) hi = x;
      const double d = x - want_mean;
      mean += x; m2 += d * d; m4 += d * d * d * d;
    }
    mean /= (double)n; m2 /= (double)n; m4 /= (double)n;
    const double se_mean = std::sqrt(want_var / (double)n), se_var = std::sqrt((m4 - m2 * m2) / (double)n);
    const double z_mean = (mean - want_mean) / se_mean, z_var = (m2 - want_var) / se_var;
    printf("shape %-8g rate %g: mean %.6g (want %.6g, z %+.2f) var %.6g (want %.6g, z %+.2f) min %.3g max %.3g zero %ld below 1e-50 %ld (%.5f) max rounds %d\n",
           shape, rate, mean, want_mean, z_mean, m2, want_var, z_var, lo, hi, zeros, floored, (double)floored / (double)n, max_rounds);
    if (std::fabs(z_mean) > 6.0 || std::fabs(z_var) > 6.0 || not_finite || negative || max_rounds >= emat::k_gamma_max_rounds) { printf("  FAILED\n"); bad = 1; }
  }
  return bad;
}
