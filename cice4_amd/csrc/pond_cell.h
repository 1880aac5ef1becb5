// compute_ponds (source/ice_meltpond.F90:170-227) and increment_age (source/ice_age.F90:117-121) for ONE listed (cell,
// category): nine words in, up to four out.  Host and device: the kernel k_pond_age (pond.hip) and the stand-alone probe
// tests/pond_probe.cpp compile this text, and nothing but libm_exact.h is included, so g++ takes it as it takes
// libm_exact_neg.h.
//
// Arithmetic: the reference's operations in the reference's order, each one correctly rounded fp64 operation (+ * / sqrt,
// and min / max as the compare-and-select the reference's compiler makes of them: `a < b ? a : b`, so that the sign of a
// zero is the reference's), compiled without contraction; exp is the restated glibc exp of libm_exact.h.  Its argument
// (rexp*dTs)/Tp lies in [-0.3, -0.0] for any real surface temperature; dTs = 0 gives exp(-0.0) = 1.
#pragma once
#include "libm_exact.h"

namespace cice {

// what pond_cell asks its caller to store
enum { POND_ST_FRAC = 1,               // apondn and hpondn
       POND_ST_VOL = 2,                // the tracer volpn (not on thin ice: :223 sits in the else branch only)
       POND_ST_AGE = 4 };              // the tracer iage

struct PondIn {
  double aicen, vicen, vsnon, Tsfc;    // the state AFTER thermo_vertical
  double meltt, melts, frain;          // top melt and snow melt of the category (m), rain (kg/m^2/s)
  double volpn, iage;                  // the tracers as they are
};
struct PondOut {
  double apondn, hpondn, volpn, iage;
  int st;                              // the POND_ST_* words that are to be stored; the others are 0
};

namespace pondk {
// drivers/cice4/ice_constants.F90:49-83,176 and the parameters of compute_ponds (:141-147)
constexpr double rhos = 330.0, rhoi = 917.0, rhofresh = 1000.0, Timelt = 0.0, puny = 1.0e-11, c0 = 0.0, c1 = 1.0;
constexpr double hicemin = 0.1, Td = 2.0, rfrac = 0.1, rexp = 0.01, dpthhi = 0.9, dpthfrac = 0.8;
CICE_HD inline double fmin_sel(double a, double b) { return a < b ? a : b; }
CICE_HD inline double fmax_sel(double a, double b) { return a > b ? a : b; }
}  // namespace pondk

// The cell is on the list (aicen > puny on a physical cell: the caller's test).  ponds / age: what runs.
CICE_HD inline PondOut pond_cell(bool ponds, bool age, double dt, const PondIn& in) {
  using namespace pondk;
  PondOut o{};
  if (age) {
    o.iage = in.iage + dt;
    o.st |= POND_ST_AGE;
  }
  if (!ponds) return o;
  const double hi = in.vicen / in.aicen;
  const double hs = in.vsnon / in.aicen;
  if (hi < hicemin) {                  // remove ponds on thin ice; the tracer keeps its old volume
    o.st |= POND_ST_FRAC;             // (apondn = hpondn = 0)
    return o;
  }
  // update pond volume
  double volpn = in.volpn + rfrac * (in.meltt * rhoi / rhofresh + in.melts * rhos / rhofresh + in.frain * dt / rhofresh);
  // shrink pond volume under freezing conditions
  const double Tp = Timelt - Td;
  const double dTs = fmax_sel(Tp - in.Tsfc, c0);
  volpn = volpn * exp_libm(rexp * dTs / Tp);
  volpn = fmax_sel(volpn, c0);
  double apondn = fmin_sel(sqrt(volpn / dpthfrac), c1);
  double hpondn = dpthfrac * apondn;
  // limit pond depth to 90% of ice thickness
  hpondn = fmin_sel(hpondn, dpthhi * hi);
  volpn = hpondn * apondn;
  // if the surface has snow, do not change albedo
  if (hs > puny) apondn = c0;
  o.apondn = apondn;
  o.hpondn = hpondn;
  o.volpn = volpn;                     // reload tracer array
  o.st |= POND_ST_FRAC | POND_ST_VOL;
  return o;
}

}  // namespace cice
