// Host probe for the negative tail of exp_libm_neg (cice4_amd/csrc/libm_exact_neg.h): glibc's specialcase branch for
// 512 <= |x| < 1024 and the underflow return below it, which ridging reaches with thin ice.  Counts arguments on which
// exp_libm differs from the host libm's exp.  Built and run by tests/test_ridge_libm.py (g++, no GPU).
#include <cstdio>
#include <cstdlib>
#include "../cice4_amd/csrc/libm_exact_neg.h"

static long bad = 0, used = 0;

static void check(double x) {
  ++used;
  const double e = std::exp(x), m = cice::exp_libm_neg(x);
  if (!(e == m) || std::signbit(e) != std::signbit(m)) {
    if (bad < 5) std::printf("mismatch x=%a libm=%a restated=%a\n", x, e, m);
    ++bad;
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 4000000;
  // dense sweep of [-1100, -500]: normal results, the subnormal range (x < -708.4), zero (x < -745.2), the cut at -1024
  for (long i = 0; i <= n; ++i) check(-1100.0 + 600.0 * (double)i / (double)n);
  unsigned long long s = 88172645463325252ull;
  for (long i = 0; i < n; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const double u = (double)(s >> 11) * (1.0 / 9007199254740992.0);
    double x;
    switch (i & 3) {
      case 0: x = -760.0 * u; break;                        // everything with a non-zero result
      case 1: x = -708.0 - 38.0 * u; break;                 // the subnormal results
      case 2: x = -std::exp(14.0 * u); break;               // up to -1.2e6: ridging's thinnest ice
      default: x = -511.0 - 2.0 * u; break;                 // across the seam at -512
    }
    check(x);
  }
  const double pts[] = {-512.0, -511.99999999999994, -512.0000000000001, -708.3964185322641, -745.1332191019411,
                        -745.1332191019412, -745.13321910194122, -1023.9999999999999, -1024.0, -1e5, -4.8e5, -1e300};
  for (double x : pts) check(x);
  std::printf("checked=%ld mismatches=%ld\n", used, bad);
  return 0;
}
