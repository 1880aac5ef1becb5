// Kernels of the thermodynamic thickness-distribution stage (itd.h): k_linear_itd, k_add_new_ice, k_lateral_melt,
// k_shift_ice and the rain / aggregate_area step in front of them.  Reference: source/ice_therm_itd.F90,
// source/ice_itd.F90:494-548 (aggregate_area), :892-1340 (shift_ice), :1482-1590 (compute_tracers).
//
// The area, volume, snow volume, thickness and tracer products of a cell's five categories live in registers; the
// layer energies and the tracers themselves are addressed in memory (read and written only where ice moves), so that
// no kernel needs scratch.  Every loop over categories, boundaries, layers and tracers is unrolled: all indices into
// the register arrays are constants.
#include "itd.h"

namespace cice {
namespace {

using ull = unsigned long long;
constexpr double puny = K::puny, c0 = 0.0, c1 = 1.0, c2 = 2.0, c3 = 3.0, c6 = 6.0, p5 = 0.5, p001 = K::p001;
constexpr double p333 = c1 / c3, p666 = c2 / c3;            // ice_constants.F90:167-168
constexpr double hfrazilmin = 0.05;                         // ice_therm_itd.F90:45

__device__ __forceinline__ double fmin_(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double fmax_(double a, double b) { return a > b ? a : b; }

struct Cell {
  int b, i, j;       // block (0-based), i, j (1-based)
  size_t q, o2, np;  // cell in its plane, cell in a (nx,ny,nb) field, plane size
  bool ok;
};

__device__ __forceinline__ Cell cell_of(const ItdArgs& A) {
  Cell c;
  c.np = (size_t)A.nx * A.ny;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  c.ok = t < c.np * (size_t)A.nblocks;
  c.b = c.ok ? (int)(t / c.np) : 0;
  c.q = c.ok ? t - (size_t)c.b * c.np : 0;
  c.j = (int)(c.q / A.nx) + 1;
  c.i = (int)(c.q % A.nx) + 1;
  c.o2 = (size_t)c.b * c.np + c.q;
  return c;
}

__device__ __forceinline__ bool physical(const ItdArgs& A, const Cell& c) {
  const int32_t* k = A.blk + 4 * c.b;
  return c.i >= k[0] && c.i <= k[1] && c.j >= k[2] && c.j <= k[3];
}

// aggregate_area (ice_itd.F90:529-546) for one cell
__device__ __forceinline__ void itd_aggregate_area(const double (&a)[NCAT], double& aice, double& aice0) {
  double s = c0;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) s = s + a[n];
  aice = s;
  aice0 = fmax_(c1 - s, c0);
}

// fit_line (ice_therm_itd.F90:777-816) for one cell and category
__device__ __forceinline__ void itd_fit_line(double aicen, double hice, double hbL, double hbR, double& g0, double& g1,
                                             double& hL, double& hR) {
  if (aicen > puny && hbR - hbL > puny) {
    hL = hbL;
    hR = hbR;
    const double h13 = p333 * (c2 * hL + hR);
    const double h23 = p333 * (hL + c2 * hR);
    if (hice < h13) hR = c3 * hice - c2 * hL;
    else if (hice > h23) hL = c3 * hice - c2 * hR;
    const double dhr = c1 / (hR - hL);
    const double wk1 = c6 * aicen * dhr;
    const double wk2 = (hice - hL) * dhr;
    g0 = wk1 * (p666 - wk2);
    g1 = c2 * dhr * wk1 * (wk2 - p5);
  } else {
    g0 = c0; g1 = c0; hL = c0; hR = c0;
  }
}

// shift_ice (ice_itd.F90:1007-1338) for one listed cell.  a, v, s, h: aicen, vicen, vsnon, hicen of the cell's
// categories; da, dv, don: daice, dvice, donor of boundary n (0-based entry n - 1; entry NCAT - 1 unused).
// trc / ei / es: the cell's element of plane 0 of trcrn / eicen / esnon of its block; np: plane stride.
// limit: 0, or the boundary (1-based) in front of whose transfer a limited launch stops.
// Returns 0 done, 1 this cell failed a range check (recorded; nothing more is written), 2 stopped at `limit`.
__device__ __forceinline__ int itd_shift_ice(const ItdParams& p, double (&a)[NCAT], double (&v)[NCAT], double (&s)[NCAT],
                                             double (&h)[NCAT], double (&da)[NCAT], double (&dv)[NCAT], int (&don)[NCAT],
                                             double* trc, double* ei, double* es, size_t np, int limit, ull bkey, ull key,
                                             ull* rec) {
  double atr[NTRCR][NCAT];
  // :1015-1037 aicen*trcrn, vicen*trcrn, vsnon*trcrn
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
#pragma unroll
    for (int it = 0; it < NTRCR; ++it) {
      atr[it][n] = c0;
      if (it < p.ntrcr) {
        const double t = trc[(size_t)(n * NTRCR + it) * np];
        atr[it][n] = p.dep[it] == 0 ? a[n] * t : (p.dep[it] == 1 ? v[n] * t : s[n] * t);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NCAT - 1; ++n) {   // boundary n + 1 between categories n + 1 and n + 2 (1-based)
    const bool up = don[n] == n + 1;     // donor is the category below the boundary
    unsigned fail = 0;
    if (don[n] > 0) {                    // :1055-1094
      const double and_ = up ? a[n] : a[n + 1], vnd = up ? v[n] : v[n + 1];
      if (da[n] < c0) {
        if (da[n] > -puny * and_) { da[n] = c0; dv[n] = c0; }
        else fail |= 1u;
      }
      if (dv[n] < c0) {
        if (dv[n] > -puny * vnd) { da[n] = c0; dv[n] = c0; }
        else fail |= 2u;
      }
      if (da[n] > and_ * (c1 - puny)) {
        if (da[n] < and_ * (c1 + puny)) { da[n] = and_; dv[n] = vnd; }
        else fail |= 4u;
      }
      if (dv[n] > vnd * (c1 - puny)) {
        if (dv[n] < vnd * (c1 + puny)) { da[n] = and_; dv[n] = vnd; }
        else fail |= 8u;
      }
    }
    if (limit == n + 1) {                // the message loops :1101-1187, every kind at once
      if (don[n] > 0) {
        const double and_ = up ? a[n] : a[n + 1], vnd = up ? v[n] : v[n + 1];
        atomicMax(&rec[ITD_REC_LASTDONOR], key << 3 | (ull)don[n]);
        if (da[n] <= -puny * a[n]) atomicMax(&rec[ITD_REC_NEG_DA], key);          // stale nd = n + 1 (1-based n)
        if (da[n] <= -puny * a[n + 1]) atomicMax(&rec[ITD_REC_NEG_DA + 1], key);  // stale nd = n + 2
        if (dv[n] <= -puny * v[n]) atomicMax(&rec[ITD_REC_NEG_DV], key);
        if (dv[n] <= -puny * v[n + 1]) atomicMax(&rec[ITD_REC_NEG_DV + 1], key);
        if (da[n] >= and_ * (c1 + puny)) atomicMax(&rec[ITD_REC_GT_DA], key);
        if (dv[n] >= vnd * (c1 + puny)) atomicMax(&rec[ITD_REC_GT_DV], key);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (fail & (1u << k)) atomicMax(&rec[ITD_REC_FLAG + k], key);
      }
      return 2;
    }
    if (fail) {
      atomicMax(&rec[ITD_REC_SHIFT], (bkey << 8 | (ull)(NCAT - (n + 1))) + 1);
      return 1;
    }
    if (da[n] > c0 && don[n] > 0) {      // :1198-1310
#define ITD_XFER(D, R)                                                                       \
  {                                                                                          \
    const double wa = dv[n] / v[D];                                                          \
    a[D] = a[D] - da[n]; a[R] = a[R] + da[n];                                                \
    v[D] = v[D] - dv[n]; v[R] = v[R] + dv[n];                                                \
    const double dvsnow = s[D] * wa;                                                         \
    s[D] = s[D] - dvsnow; s[R] = s[R] + dvsnow;                                              \
    _Pragma("unroll") for (int it = 0; it < NTRCR; ++it) if (it < p.ntrcr) {                 \
      const double t = trc[(size_t)((D) * NTRCR + it) * np];                                 \
      const double datrcr = p.dep[it] == 0 ? da[n] * t : (p.dep[it] == 1 ? dv[n] * t : dvsnow * t); \
      atr[it][D] = atr[it][D] - datrcr; atr[it][R] = atr[it][R] + datrcr;                    \
    }                                                                                        \
    _Pragma("unroll") for (int k = 0; k < NILYR; ++k) {                                      \
      const double e = ei[(size_t)((D) * NILYR + k) * np];                                   \
      const double deice = e * wa;                                                           \
      ei[(size_t)((D) * NILYR + k) * np] = e - deice;                                        \
      ei[(size_t)((R) * NILYR + k) * np] = ei[(size_t)((R) * NILYR + k) * np] + deice;       \
    }                                                                                        \
    _Pragma("unroll") for (int k = 0; k < NSLYR; ++k) {                                      \
      const double e = es[(size_t)((D) * NSLYR + k) * np];                                   \
      const double desnow = e * wa;                                                          \
      es[(size_t)((D) * NSLYR + k) * np] = e - desnow;                                       \
      es[(size_t)((R) * NSLYR + k) * np] = es[(size_t)((R) * NSLYR + k) * np] + desnow;      \
    }                                                                                        \
  }
      if (up) ITD_XFER(n, n + 1)
      else ITD_XFER(n + 1, n)
#undef ITD_XFER
    }
  }
  // :1318-1338 thickness; compute_tracers :1536-1588
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    h[n] = a[n] > puny ? v[n] / a[n] : c0;
#pragma unroll
    for (int it = 0; it < NTRCR; ++it) {
      if (it < p.ntrcr) {
        double t;
        if (it == p.it_Tsfc) t = a[n] > puny ? atr[it][n] / a[n] : K::Tocnfrz;
        else if (p.dep[it] == 0) t = a[n] > puny ? atr[it][n] / a[n] : c0;
        else if (p.dep[it] == 1) t = v[n] > c0 ? atr[it][n] / v[n] : c0;
        else t = s[n] > c0 ? atr[it][n] / s[n] : c0;
        trc[(size_t)(n * NTRCR + it) * np] = t;
      }
    }
  }
  return 0;
}

// compute_tracers' `trcrn(:,:,:) = c0` (:1536) for a cell outside the list
__device__ __forceinline__ void zero_tracers(const ItdParams& p, double* trc, size_t np) {
#pragma unroll
  for (int n = 0; n < NCAT; ++n)
#pragma unroll
    for (int it = 0; it < NTRCR; ++it)
      if (it < p.ntrcr) trc[(size_t)(n * NTRCR + it) * np] = c0;
}

// ice_step_mod.F90:290-310: rain drains to the ocean (with the area the step came in with), then aggregate_area;
// marks the blocks that hold a cell with aice > puny on the physical domain (`if (icells > 0)`, :327)
__global__ __launch_bounds__(256) void k_itd_rain_aggregate(const ItdArgs A) {
  const Cell c = cell_of(A);
  if (!c.ok || c.b > A.bfail) return;
  if (A.frain) A.fresh[c.o2] = A.fresh[c.o2] + A.frain[c.o2] * A.aice[c.o2];
  if (!A.kitd) return;
  const double* pa = A.aicen + (size_t)c.b * NCAT * c.np + c.q;
  double a[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) a[n] = pa[(size_t)n * c.np];
  double aice, aice0;
  itd_aggregate_area(a, aice, aice0);
  A.aice[c.o2] = aice;
  A.aice0[c.o2] = aice0;
  if (A.blockflag_out && aice > puny && physical(A, c)) A.blockflag_out[c.b] = 1;   // same value from every writer
}

// linear_itd, ice_therm_itd.F90:211-641
__global__ __launch_bounds__(256) void k_linear_itd(const ItdArgs A) {
  const Cell c = cell_of(A);
  if (!c.ok || c.b > A.bfail) return;
  if (A.blockflag && !A.blockflag[c.b]) return;
  const ItdParams& p = A.p;
  const size_t np = c.np;
  const int limit = c.b == A.bfail ? A.nlimit : 0;
  bool listed;
  ull key;
  if (A.listpos) {
    const int lp = A.listpos[c.o2];
    listed = lp > 0;
    key = (ull)lp;
  } else {
    listed = physical(A, c) && A.aice[c.o2] > puny;
    key = (ull)c.q + 1;
  }
  double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
  double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
  double a[NCAT], v[NCAT], s[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) a[n] = pa[(size_t)n * np];
  if (!listed) {
    if (limit) return;                 // the reference left shift_ice in front of compute_tracers and aggregate_area
    zero_tracers(p, trc, np);
    itd_aggregate_area(a, A.aice[c.o2], A.aice0[c.o2]);
    return;
  }
  const double* pai = A.aicen_init + (size_t)c.b * NCAT * np + c.q;
  const double* pvi = A.vicen_init + (size_t)c.b * NCAT * np + c.q;
  double h[NCAT], hinit[NCAT], dh[NCAT], hb[NCAT + 1], hm[NCAT + 1];
#pragma unroll
  for (int n = 0; n <= NCAT; ++n) hm[n] = p.hin_max[n];
  hm[NCAT] = 999.9;                    // :219
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {     // :262-283
    v[n] = pv[(size_t)n * np];
    s[n] = ps[(size_t)n * np];
    const double ai = pai[(size_t)n * np], vi = pvi[(size_t)n * np];
    hinit[n] = ai > puny ? vi / ai : c0;
    if (a[n] > puny) {
      h[n] = v[n] / a[n];
      dh[n] = h[n] - hinit[n];
    } else {
      h[n] = c0;
      dh[n] = c0;
    }
  }
  bool remap = true;
  hb[0] = hm[0];
#pragma unroll
  for (int n = 1; n < NCAT; ++n) {     // :294-383, boundary n between categories n and n + 1 (entries n - 1, n)
    if (hinit[n - 1] > puny && hinit[n] > puny) {
      const double slope = (dh[n] - dh[n - 1]) / (hinit[n] - hinit[n - 1]);
      hb[n] = hm[n] + dh[n - 1] + slope * (hm[n] - hinit[n - 1]);
    } else if (hinit[n - 1] > puny) {
      hb[n] = hm[n] + dh[n - 1];
    } else if (hinit[n] > puny) {
      hb[n] = hm[n] + dh[n];
    } else {
      hb[n] = hm[n];
    }
    if (a[n - 1] > puny && h[n - 1] >= hb[n]) remap = false;
    else if (a[n] > puny && h[n] <= hb[n]) remap = false;
    if (hb[n] > hm[n + 1]) remap = false;
    if (hb[n] < hm[n - 1]) remap = false;
  }
  hb[NCAT] = a[NCAT - 1] > puny ? c3 * h[NCAT - 1] - c2 * hb[NCAT - 1] : hm[NCAT];   // :392-401
  hb[NCAT] = fmax_(hb[NCAT], hm[NCAT - 1]);

  double da[NCAT], dv[NCAT];
  int don[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) { da[n] = c0; dv[n] = c0; don[n] = 0; }
  if (remap) {
    double g0[NCAT], g1[NCAT], hL[NCAT], hR[NCAT];
    itd_fit_line(a[0], hinit[0], hb[0], hm[1], g0[0], g1[0], hL[0], hR[0]);   // :433-441, g(h) of category 1 at the start
    if (a[0] > puny) {                 // :450-490
      double dh0 = dh[0];
      if (dh0 < c0) {
        dh0 = fmin_(-dh0, hm[1]);
        const double etamax = fmin_(dh0, hR[0]) - hL[0];
        if (etamax > c0) {
          const double x1 = etamax;
          const double x2 = p5 * etamax * etamax;
          double da0 = g1[0] * x2 + g0[0] * x1;
          const double damax = a[0] * (c1 - h[0] / hinit[0]);
          da0 = fmin_(da0, damax);
          h[0] = h[0] * a[0] / (a[0] - da0);
          a[0] = a[0] - da0;
        }
      } else {
        hb[0] = fmin_(dh0, hm[1]);
      }
    }
#pragma unroll
    for (int n = 0; n < NCAT; ++n) itd_fit_line(a[n], h[n], hb[n], hb[n + 1], g0[n], g1[n], hL[n], hR[n]);   // :496-507
#pragma unroll
    for (int n = 1; n < NCAT; ++n) {   // :521-591
      double etamin, etamax;
      const bool up = hb[n] > hm[n];   // transfer from n to n + 1
      const double g0d = up ? g0[n - 1] : g0[n], g1d = up ? g1[n - 1] : g1[n], hLd = up ? hL[n - 1] : hL[n],
                   hRd = up ? hR[n - 1] : hR[n];
      if (up) {
        etamin = fmax_(hm[n], hLd) - hLd;
        etamax = fmin_(hb[n], hRd) - hLd;
        don[n - 1] = n;
      } else {
        etamin = c0;
        etamax = fmin_(hm[n], hRd) - hLd;
        don[n - 1] = n + 1;
      }
      if (etamax > etamin) {
        const double x1 = etamax - etamin;
        double wk1 = etamin * etamin;
        double wk2 = etamax * etamax;
        const double x2 = p5 * (wk2 - wk1);
        wk1 = wk1 * etamin;
        wk2 = wk2 * etamax;
        const double x3 = p333 * (wk2 - wk1);
        da[n - 1] = g1d * x2 + g0d * x1;
        dv[n - 1] = g1d * x3 + g0d * x2 + da[n - 1] * hLd;
      }
      const double and_ = up ? a[n - 1] : a[n], vnd = up ? v[n - 1] : v[n];
      if (da[n - 1] < and_ * puny) { da[n - 1] = c0; dv[n - 1] = c0; don[n - 1] = 0; }
      if (dv[n - 1] < vnd * puny) { da[n - 1] = c0; dv[n - 1] = c0; don[n - 1] = 0; }
      if (da[n - 1] > and_ * (c1 - puny)) { da[n - 1] = and_; dv[n - 1] = vnd; }
      if (dv[n - 1] > vnd * (c1 - puny)) { da[n - 1] = and_; dv[n - 1] = vnd; }
    }
  } else {
    atomicAdd(&A.rec[ITD_REC_NOREMAP], 1ull);
  }
  const int st = itd_shift_ice(p, a, v, s, h, da, dv, don, trc, A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q,
                               A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q, np, limit,
                               (ull)(A.nblocks - 1 - c.b), key, A.rec);
  if (st == 1) return;
  if (st == 0 && remap && p.hi_min > c0 && a[0] > puny && h[0] < p.hi_min) {   // :623-632
    a[0] = a[0] * h[0] / p.hi_min;
    h[0] = p.hi_min;
  }
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    pa[(size_t)n * np] = a[n];
    pv[(size_t)n * np] = v[n];
    ps[(size_t)n * np] = s[n];
  }
  if (st == 0) itd_aggregate_area(a, A.aice[c.o2], A.aice0[c.o2]);   // :637
}

// shift_ice with the reference's argument list (hicen, donor, daice, dvice as (icells, ncat) arrays)
__global__ __launch_bounds__(256) void k_shift_ice(const ItdArgs A) {
  const Cell c = cell_of(A);
  if (!c.ok) return;
  const size_t np = c.np;
  const int lp = A.listpos[c.o2];
  double* trc = A.trcrn + c.q;
  if (lp <= 0) {
    if (!A.nlimit) zero_tracers(A.p, trc, np);
    return;
  }
  double* pa = A.aicen + c.q;
  double* pv = A.vicen + c.q;
  double* ps = A.vsnon + c.q;
  double a[NCAT], v[NCAT], s[NCAT], h[NCAT], da[NCAT], dv[NCAT];
  int don[NCAT];
  const size_t m = (size_t)lp - 1, ld = (size_t)A.icells;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    a[n] = pa[(size_t)n * np];
    v[n] = pv[(size_t)n * np];
    s[n] = ps[(size_t)n * np];
    h[n] = c0;                         // shift_ice only writes hicen (:1318-1329), and only where it runs to the end
    da[n] = A.daice[m + ld * n];
    dv[n] = A.dvice[m + ld * n];
    don[n] = A.donor[m + ld * n];
  }
  const int st = itd_shift_ice(A.p, a, v, s, h, da, dv, don, trc, A.eicen + c.q, A.esnon + c.q, np, A.nlimit, 0ull,
                               (ull)lp, A.rec);
  if (st == 1) return;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    pa[(size_t)n * np] = a[n];
    pv[(size_t)n * np] = v[n];
    ps[(size_t)n * np] = s[n];
    if (st == 0) A.hicen[m + ld * n] = h[n];
    A.daice[m + ld * n] = da[n];
    A.dvice[m + ld * n] = dv[n];
  }
}

// add_new_ice, ice_therm_itd.F90:985-1245
__global__ __launch_bounds__(256) void k_add_new_ice(const ItdArgs A) {
  const Cell c = cell_of(A);
  if (!c.ok || c.b >= A.bend) return;
  const ItdParams& p = A.p;
  const size_t np = c.np;
  ull key;
  if (A.listpos) {
    const int lp = A.listpos[c.o2];
    if (lp <= 0) return;
    key = (ull)lp;
  } else {
    if (!A.tmask[c.o2]) return;        // every tmask cell of the whole block, ghost cells included (ice_step_mod.F90:366-376)
    key = (ull)c.q + 1;
  }
  double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
  double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
  double a[NCAT], v[NCAT];
  double vice_init = c0;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    a[n] = pa[(size_t)n * np];
    v[n] = pv[(size_t)n * np];
    vice_init = vice_init + v[n];      // column_sum :999
  }
  const double hi0max = p.hin_max[1] * 0.9;   // :993 (ncat > 1)
  const double rnilyr = (double)NILYR;
  const double qi0 = -K::rhoi * K::Lfresh;    // :1013-1019
  double qi0av = c0;
#pragma unroll
  for (int k = 0; k < NILYR; ++k) qi0av = qi0av + qi0;
  qi0av = qi0av / rnilyr;

  const double dt = A.dt;
  const double aice = A.aice[c.o2];
  double aice0 = A.aice0[c.o2];
  const double fnew = fmax_(A.frzmlt[c.o2], c0);
  double vi0new = -fnew * dt / qi0av;
  vice_init = vice_init + vi0new;
  A.frazil[c.o2] = vi0new;
  if (A.frz_onset) {
    if (vi0new > puny && A.frz_onset[c.o2] < puny) A.frz_onset[c.o2] = A.yday;
  }
  if (p.update_ocn_f) {
    const double dfresh = -K::rhoi * vi0new / dt;
    const double dfsalt = K::ice_ref_salinity * p001 * dfresh;
    A.fresh[c.o2] = A.fresh[c.o2] + dfresh;
    A.fsalt[c.o2] = A.fsalt[c.o2] + dfsalt;
  }
  double hsurp = c0, ai0new = c0;
  if (vi0new > c0) {                   // :1084-1105
    if (aice0 > puny) {
      double hi0new = fmax_(vi0new / aice0, hfrazilmin);
      if (hi0new > hi0max && aice0 + puny < c1) {
        hi0new = hi0max;
        ai0new = aice0;
        const double vsurp = vi0new - ai0new * hi0new;
        hsurp = vsurp / aice;
        vi0new = ai0new * hi0new;
      } else {
        ai0new = vi0new / hi0new;
      }
    } else {
      hsurp = vi0new / aice;
      vi0new = c0;
    }
  }
  if (hsurp > c0) {                    // :1138-1182 surplus over all categories
#pragma unroll
    for (int n = 0; n < NCAT; ++n) {
      const double vsurp = hsurp * a[n];
      const double vtmp = v[n] + vsurp;
      if (p.tr_iage && vtmp > puny) {
        double* t = trc + (size_t)(n * NTRCR + p.it_iage) * np;
        *t = (*t * v[n] + dt * vsurp) / vtmp;
      }
      if (p.tr_lvl && v[n] > puny) {
        double* t = trc + (size_t)(n * NTRCR + p.it_vlvl) * np;
        *t = (*t * v[n] + trc[(size_t)(n * NTRCR + p.it_alvl) * np] * vsurp) / vtmp;
      }
      v[n] = vtmp;
      const double vlyr = vsurp / rnilyr;
#pragma unroll
      for (int k = 0; k < NILYR; ++k) {
        double* e = ei + (size_t)(n * NILYR + k) * np;
        *e = *e + qi0 * vlyr;
      }
    }
  }
  if (vi0new > c0) {                   // :1192-1231 new ice into category 1
    const double area1 = a[0], vice1 = v[0];
    a[0] = a[0] + ai0new;
    aice0 = aice0 - ai0new;
    v[0] = v[0] + vi0new;
    double* t = trc + (size_t)p.it_Tsfc * np;
    *t = (*t * area1 + A.Tf[c.o2] * ai0new) / a[0];
    *t = fmin_(*t, c0);
    if (p.tr_iage && v[0] > puny) {
      double* g = trc + (size_t)p.it_iage * np;
      *g = (*g * vice1 + dt * vi0new) / v[0];
    }
    if (p.tr_lvl && a[0] > puny) {
      double* al = trc + (size_t)p.it_alvl * np;
      double* vl = trc + (size_t)p.it_vlvl * np;
      *al = (*al * area1 + ai0new) / a[0];
      *vl = (*vl * vice1 + vi0new) / v[0];
    }
    const double vlyr = vi0new / rnilyr;
#pragma unroll
    for (int k = 0; k < NILYR; ++k) {
      double* e = ei + (size_t)k * np;
      *e = *e + qi0 * vlyr;
    }
    A.aice0[c.o2] = aice0;
  }
  double vice_final = c0;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    pa[(size_t)n * np] = a[n];
    pv[(size_t)n * np] = v[n];
    vice_final = vice_final + v[n];
  }
  const double d = vice_final - vice_init;
  if ((d < c0 ? -d : d) > puny)        // column_conservation_check, ice_itd.F90:1458-1471: the last failing cell
    atomicMax(&A.rec[ITD_REC_ADD], (ull)(A.nblocks - 1 - c.b) << 32 | key);
}

// lateral_melt, ice_therm_itd.F90:1330-1418.  fhocn accumulates category by category, ice layers before snow layers.
__global__ __launch_bounds__(256) void k_lateral_melt(const ItdArgs A) {
  const Cell c = cell_of(A);
  if (!c.ok || c.b >= A.bend || !physical(A, c)) return;
  const double rside = A.rside[c.o2];
  if (!(rside > c0)) return;
  const size_t np = c.np;
  const double dt = A.dt;
  double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
  double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
  double* es = A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q;
  double fresh = A.fresh[c.o2], fsalt = A.fsalt[c.o2], fhocn = A.fhocn[c.o2], meltl = A.meltl[c.o2];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    const double an = pa[(size_t)n * np], vn = pv[(size_t)n * np], sn = ps[(size_t)n * np];
    const double dfresh = (K::rhos * sn + K::rhoi * vn) * rside / dt;
    const double dfsalt = K::rhoi * vn * K::ice_ref_salinity * p001 * rside / dt;
    fresh = fresh + dfresh;
    fsalt = fsalt + dfsalt;
    meltl = meltl + vn * rside;
    pa[(size_t)n * np] = an * (c1 - rside);
    pv[(size_t)n * np] = vn * (c1 - rside);
    ps[(size_t)n * np] = sn * (c1 - rside);
#pragma unroll
    for (int k = 0; k < NILYR; ++k) {
      double* e = ei + (size_t)(n * NILYR + k) * np;
      const double dfhocn = *e * rside / dt;
      fhocn = fhocn + dfhocn;
      *e = *e * (c1 - rside);
    }
#pragma unroll
    for (int k = 0; k < NSLYR; ++k) {
      double* e = es + (size_t)(n * NSLYR + k) * np;
      const double dfhocn = *e * rside / dt;
      fhocn = fhocn + dfhocn;
      *e = *e * (c1 - rside);
    }
  }
  A.fresh[c.o2] = fresh;
  A.fsalt[c.o2] = fsalt;
  A.fhocn[c.o2] = fhocn;
  A.meltl[c.o2] = meltl;
}

inline unsigned grid_of(const ItdArgs& a) {
  const size_t n = (size_t)a.nx * a.ny * a.nblocks;
  return (unsigned)((n + 255) / 256);
}

}  // namespace

void itd_launch_rain_aggregate(const ItdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_itd_rain_aggregate, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}
void itd_launch_linear(const ItdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_linear_itd, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}
void itd_launch_shift(const ItdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_shift_ice, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}
void itd_launch_add_new_ice(const ItdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_add_new_ice, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}
void itd_launch_lateral_melt(const ItdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_lateral_melt, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
