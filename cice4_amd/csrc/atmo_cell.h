// The cell routine of atmo_boundary_layer (source/ice_atmo.F90:56-384) and its two helpers, for the kernels that run it:
// atmo.hip (one lane = one (cell[, category]) of step_therm1) and coupling.hip (the ocean cells of ocean_mixed_layer).  One
// text, included by both: the five stability iterations (:264-305) run in registers.  exp is glibc's (libm_exact.h); log and
// atan are the device library's (<= 1 ulp): the outputs agree with the reference's to ~1e-15 relative, not bit for bit
// (DESIGN.md section 3.6).
#pragma once
#include <cmath>

#include "atmo.h"

namespace cice {

namespace {

struct AtmoOut { double strx, stry, Tref, Qref, delt, delq, lhcoef, shcoef; };

__device__ __forceinline__ double psimhu(double xd, double pih) {   // :165-166
  return log((1.0 + xd * (2.0 + xd)) * (1.0 + xd * xd) / 8.0) - 2.0 * atan(xd) + pih;
}
__device__ __forceinline__ double psixhu(double xd) {               // :169
  return 2.0 * log((1.0 + xd * xd) / 2.0);
}

__device__ __forceinline__ AtmoOut atmo_cell(const AtmoParams& P, int ocn, double Tsf, double potT, double uatm,
                                             double vatm, double wind, double zlvl, double Qa, double rhoa) {
  AtmoOut o;
  const double vmag = fmax(P.umin, wind);                                             // :201 / :214
  const double rdn = ocn ? sqrt(0.0027 / vmag + .000142 + .0000764 * vmag) : P.rdn_ice;  // :202 / :215
  const double TsfK = Tsf + P.Tffresh;                                                // :232
  const double qsat = P.qqq[ocn] * exp_libm(-P.TTT[ocn] / TsfK);
  const double ssq = qsat / rhoa;
  const double thva = potT * (1.0 + P.zvir * Qa);
  const double delt = potT - TsfK, delq = Qa - ssq;
  const double alz = log(zlvl / P.zref);
  const double cp = P.cp_air * (1.0 + P.cpvir * ssq);
  const double rhn = rdn, ren = rdn;                                                  // :248-249
  double ustar = rdn * vmag, tstar = rhn * delt, qstar = ren * delq;
  double hol = 0.0, stable = 0.0, psixh = 0.0, rd = 0.0, rh = 0.0, re = 0.0;
  for (int k = 0; k < 5; ++k) {                                                        // :264
    hol = P.vonkar * P.gravit * zlvl * (tstar / thva + qstar / (1.0 / P.zvir + Qa)) / (ustar * ustar);
    hol = copysign(fmin(fabs(hol), 10.0), hol);
    stable = 0.5 + copysign(0.5, hol);
    double xqq = fmax(sqrt(fabs(1.0 - 16.0 * hol)), 1.0);
    xqq = sqrt(xqq);
    const double psimhs = -(0.7 * hol + 0.75 * (hol - 14.3) * exp_libm(-0.35 * hol) + 10.7);   // Jordan et al 1999
    const double psimh = psimhs * stable + (1.0 - stable) * psimhu(xqq, P.pih);
    psixh = psimhs * stable + (1.0 - stable) * psixhu(xqq);
    rd = rdn / (1.0 + rdn / P.vonkar * (alz - psimh));                                 // :291-293
    rh = rhn / (1.0 + rhn / P.vonkar * (alz - psixh));
    re = ren / (1.0 + ren / P.vonkar * (alz - psixh));
    ustar = rd * vmag; tstar = rh * delt; qstar = re * delq;
  }
  const double tau = rhoa * ustar * rd;                                               // :335
  o.strx = tau * uatm; o.stry = tau * vatm;
  o.shcoef = rhoa * ustar * cp * rh + 1.0;                                            // :359-360
  o.lhcoef = rhoa * ustar * P.Lheat[ocn] * re;
  hol = hol * P.zTrf / zlvl;                                                          // :365
  double xqq = fmax(1.0, sqrt(fabs(1.0 - 16.0 * hol)));
  xqq = sqrt(xqq);
  const double psix2 = -5.0 * hol * stable + (1.0 - stable) * psixhu(xqq);
  double fac = (rh / P.vonkar) * (alz + P.al2 - psixh + psix2);
  o.Tref = potT - delt * fac;
  o.Tref = o.Tref - 0.01 * P.zTrf;
  fac = (re / P.vonkar) * (alz + P.al2 - psixh + psix2);
  o.Qref = Qa - delq * fac;
  o.delt = delt; o.delq = delq;
  return o;
}

}  // namespace

}  // namespace cice
