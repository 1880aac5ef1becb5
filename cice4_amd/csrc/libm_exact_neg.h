// exp_libm (libm_exact.h) carried on to EVERY negative argument, for ridging.
//
// ridge_shift calls exp(-(hR - hrmin)/hrexp) with hrexp = mu_rdg sqrt(max(hi, puny)) (source/ice_mechred.F90:1636-1653):
// thin ice drives the argument to -1e5 and further, where the result -- a subnormal number or zero -- becomes the area
// of an empty category.  exp_libm hands |x| >= 512 to the platform exp, which is not the host's on the device.  Here:
// glibc's specialcase() for 512 <= |x| < 1024 (the result is scaled into the subnormal range with one rounding; that
// branch runs WITHOUT fused operations in the host's build, found by probing, pinned by tests/libm_probe_neg.cpp), its
// underflow return 0 below -1024, and exp_libm itself for everything else -- so every argument under 512 in magnitude
// keeps its bits.  A header of its own: libm_exact.h is one of the sources the archived counter passes of the EVP and
// thermo kernels are tied to (bench.py: KERNEL_SOURCES), and those kernels do not change.
#pragma once
#include "libm_exact.h"

namespace cice {

CICE_HD inline double exp_libm_neg(double x) {
  if (!(x <= -512.0)) return exp_libm(x);
  if (x <= -1024.0) return 0.0;             // __math_uflow(0), -inf
  constexpr int N = 128;
  constexpr double InvLn2N = 0x1.71547652b82fep0 * N, Shift = 0x1.8p52;
  constexpr double NegLn2hiN = -0x1.62e42fefa0000p-8, NegLn2loN = -0x1.cf79abc9e3b3ap-47;
  constexpr double C2 = 0x1.ffffffffffdbdp-2, C3 = 0x1.555555555543cp-3, C4 = 0x1.55555cf172b91p-5,
                   C5 = 0x1.1111167a4d017p-7;
  double kd = std::fma(InvLn2N, x, Shift);
  unsigned long long ki;
  std::memcpy(&ki, &kd, 8);
  kd -= Shift;
  const double r = std::fma(kd, NegLn2loN, std::fma(kd, NegLn2hiN, x));
  const unsigned idx = 2u * (unsigned)(ki % N);
  const unsigned long long tbits = libm_exp_table[idx];
  const unsigned long long sbits = libm_exp_table[idx + 1] + (ki << (52 - 7)) + (1022ull << 52);   // k < 0
  double tail, sc;
  std::memcpy(&tail, &tbits, 8);
  std::memcpy(&sc, &sbits, 8);
  const double r2 = r * r;
  const double tmp = std::fma(r2 * r2, std::fma(r, C5, C4), std::fma(r2, std::fma(r, C3, C2), tail + r));
  double y = sc + sc * tmp;
  if (y < 1.0) {                            // round once, at the precision the subnormal result has
    double lo = sc - y + sc * tmp;
    const double hi = 1.0 + y;
    lo = 1.0 - hi + y + lo;
    y = (hi + lo) - 1.0;
    if (y == 0.0) y = 0.0;
  }
  return 0x1p-1022 * y;
}

}  // namespace cice
