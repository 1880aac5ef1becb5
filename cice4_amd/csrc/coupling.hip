// k_coupling_prep, k_ocean_mixed_layer (coupling.h).
#include "coupling.h"

#include "atmo_cell.h"

namespace cice {

namespace {

// ice_constants.F90: cprho = cp_ocn*rhow; ice_ocean.F90:87 frzmlt_max
constexpr double cprho = K::cp_ocn * K::rhow, frzmlt_max = 1000.0;

// x**4 as the reference's compiler evaluates it (coupling.h)
__device__ __forceinline__ double pow4(double x) {
  return ((x * x) * x) * x;
}

// Grid (chunks of 256 cells of a plane, 1, blocks); a thread owns a cell with all its categories, as k_prep_radiation: a
// wavefront takes 64 consecutive cells of one (category, block), 512 contiguous bytes per array and access.  Every cell of
// the block, ghost cells included (CICE_RunMod.F90:649-650).
__global__ __launch_bounds__(256) void k_coupling_prep(const CouplingArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int b = (int)blockIdx.z;
  const size_t np = (size_t)a.np, c2 = (size_t)b * np + q;
  const bool lit = a.coszen[c2] > K::puny;                // sun above horizon
  if (a.albcnt) {                                         // for history averaging (:661-665)
    const double cszn = lit ? K::c1 : K::c0;
    for (int n = 0; n < a.nstreams; ++n) {
      double* w = a.albcnt + ((size_t)n * a.nb + b) * np + q;
      *w = *w + cszn;
    }
  }
  double alvdf = K::c0, alidf = K::c0, alvdr = K::c0, alidr = K::c0, albice = K::c0, albsno = K::c0, albpnd = K::c0;
  for (int n = 0; n < a.ncat; ++n) {                      // :668-690
    const size_t c = ((size_t)b * a.ncat + n) * np + q;
    const double aicen = a.aicen[c];
    alvdf = alvdf + a.alvdfn[c] * aicen;
    alidf = alidf + a.alidfn[c] * aicen;
    alvdr = alvdr + a.alvdrn[c] * aicen;
    alidr = alidr + a.alidrn[c] * aicen;
    if (lit) {
      albice = albice + a.albicen[c] * aicen;
      albsno = albsno + a.albsnon[c] * aicen;
      albpnd = albpnd + (a.albpndn ? a.albpndn[c] : K::c0) * aicen;
    }
  }
  a.albice[c2] = albice; a.albsno[c2] = albsno; a.albpnd[c2] = albpnd;
  // grid box mean albedos and fluxes before scaling by aice (:696-705)
  a.alvdf_gbm[c2] = alvdf; a.alidf_gbm[c2] = alidf; a.alvdr_gbm[c2] = alvdr; a.alidr_gbm[c2] = alidr;
  a.fresh_gbm[c2] = a.flux[CPL_FRESH][c2];
  a.fsalt_gbm[c2] = a.flux[CPL_FSALT][c2];
  a.fhocn_gbm[c2] = a.flux[CPL_FHOCN][c2];
  a.fswthru_gbm[c2] = a.flux[CPL_FSWTHRU][c2];
  a.scale_factor[c2] = a.swvdr[c2] * (K::c1 - alvdr) + a.swvdf[c2] * (K::c1 - alvdf) + a.swidr[c2] * (K::c1 - alidr) +
                       a.swidf[c2] * (K::c1 - alidf);    // :710-714
  if (a.scale) {                                          // scale_fluxes (ice_flux.F90:844-886)
    const double aice = a.aice[c2];
    if (a.tmask[c2] != 0 && aice > K::c0) {
      const double ar = K::c1 / aice;
#pragma unroll
      for (int k = 0; k < CPL_FLUXES; ++k) a.flux[k][c2] = a.flux[k][c2] * ar;
      alvdr = alvdr * ar; alidr = alidr * ar; alvdf = alvdf * ar; alidf = alidf * ar;
    } else {                                              // zero out fluxes
#pragma unroll
      for (int k = 0; k < CPL_FLUXES; ++k) a.flux[k][c2] = K::c0;
      // to make upward longwave over ocean reasonable for history file
      a.flux[CPL_FLWOUT][c2] = -K::stefan_boltzmann * pow4(a.Tf[c2] + K::Tffresh);
      a.flux[CPL_TREF][c2] = a.Tair[c2];
      a.flux[CPL_QREF][c2] = a.Qa[c2];
      alvdr = K::c0; alidr = K::c0; alvdf = K::c0; alidf = K::c0;
    }
  }
  a.alvdr[c2] = alvdr; a.alidr[c2] = alidr; a.alvdf[c2] = alvdf; a.alidf[c2] = alidf;
}

// Grid as above, one thread per (cell, block) on every cell of the block
__global__ __launch_bounds__(256) void k_ocean_mixed_layer(const MixedLayerArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const size_t c = (size_t)blockIdx.z * a.np + q;
  const bool ocean = a.tmask[c] != 0;
  // ocean albedo: albocn in each spectral band, the whole block (:178-181)
  a.alvdr_ocn[c] = a.albocn; a.alidr_ocn[c] = a.albocn; a.alvdf_ocn[c] = a.albocn; a.alidf_ocn[c] = a.albocn;
  AtmoOut o{};                                            // atmo_boundary_layer zeroes the block first (ice_atmo.F90:189-194, :314-315)
  if (!ocean) {                                           // :125-130
    a.sst[c] = K::c0; a.frzmlt[c] = K::c0; a.flwout_ocn[c] = K::c0; a.fsens_ocn[c] = K::c0; a.flat_ocn[c] = K::c0;
    a.evap_ocn[c] = K::c0;
  } else {
    double sst = a.sst[c], qdp = a.qdp[c];
    o = atmo_cell(a.p, 1, sst, a.potT[c], a.uatm[c], a.vatm[c], a.wind[c], a.zlvl[c], a.Qa[c], a.rhoa[c]);
    const double Tf = a.Tf[c], hmix = a.hmix[c];
    // shortwave radiative flux (:195-198)
    const double swabs = (K::c1 - a.albocn) * a.swvdr[c] + (K::c1 - a.albocn) * a.swidr[c] + (K::c1 - a.albocn) * a.swvdf[c] +
                         (K::c1 - a.albocn) * a.swidf[c];
    const double TsfK = sst + K::Tffresh;
    const double flwout = -K::stefan_boltzmann * pow4(TsfK);
    const double fsens = o.shcoef * o.delt;
    const double flat = o.lhcoef * o.delq;
    a.flwout_ocn[c] = flwout; a.fsens_ocn[c] = fsens; a.flat_ocn[c] = flat;
    a.evap_ocn[c] = -flat / K::Lvap;
    // sst change due to exchange with atm/ice above (:212-216); fhocn, fswthru are *aice
    sst = sst + a.dt * ((fsens + flat + flwout + a.flw[c] + swabs) * (K::c1 - a.aice[c]) + a.fhocn[c] + a.fswthru[c]) /
                    (cprho * hmix);
    if (sst <= Tf && qdp > K::c0) qdp = K::c0;            // :219
    sst = sst - qdp * a.dt / (cprho * hmix);              // :222
    double frzmlt = (Tf - sst) * cprho * hmix / a.dt;     // :225-226
    frzmlt = fmin(fmax(frzmlt, -frzmlt_max), frzmlt_max);
    if (sst <= Tf) sst = Tf;                              // :229
    a.sst[c] = sst; a.qdp[c] = qdp; a.frzmlt[c] = frzmlt;
  }
  a.strairx_ocn[c] = o.strx; a.strairy_ocn[c] = o.stry; a.Tref_ocn[c] = o.Tref; a.Qref_ocn[c] = o.Qref;
  if (a.delt) a.delt[c] = o.delt;
  if (a.delq) a.delq[c] = o.delq;
  if (a.shcoef) a.shcoef[c] = o.shcoef;
  if (a.lhcoef) a.lhcoef[c] = o.lhcoef;
}

void check_dims(int np, int ncat, int nb, const char* what) {
  CICE_REQUIRE(np >= 1 && ncat >= 1 && nb >= 1, what);
  CICE_REQUIRE((long long)np < (1ll << 31) - 256, what);
  CICE_REQUIRE(nb <= 65535, what);
}

}  // namespace

void coupling_prep_launch(const CouplingArgs& a, hipStream_t s) {
  check_dims(a.np, a.ncat, a.nb, "coupling_prep: bad dimensions");
  CICE_REQUIRE(a.nstreams >= 0 && (!a.albcnt || a.nstreams >= 1), "coupling_prep: bad nstreams");
  CICE_REQUIRE(a.alvdrn && a.alidrn && a.alvdfn && a.alidfn && a.albicen && a.albsnon && a.aicen && a.coszen && a.swvdr &&
                   a.swvdf && a.swidr && a.swidf && a.alvdr && a.alidr && a.alvdf && a.alidf && a.albice && a.albsno &&
                   a.albpnd && a.alvdf_gbm && a.alidf_gbm && a.alvdr_gbm && a.alidr_gbm && a.fresh_gbm && a.fsalt_gbm &&
                   a.fhocn_gbm && a.fswthru_gbm && a.scale_factor, "coupling_prep: NULL buffer");
  bool fluxes = a.flux[CPL_FRESH] && a.flux[CPL_FSALT] && a.flux[CPL_FHOCN] && a.flux[CPL_FSWTHRU];
  for (int k = 0; k < CPL_FLUXES && a.scale; ++k) fluxes = fluxes && a.flux[k];
  CICE_REQUIRE(fluxes && (!a.scale || (a.tmask && a.aice && a.Tf && a.Tair && a.Qa)), "coupling_prep: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), 1u, (unsigned)a.nb);
  hipLaunchKernelGGL(k_coupling_prep, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void ocean_mixed_layer_launch(const MixedLayerArgs& a, hipStream_t s) {
  check_dims(a.np, 1, a.nb, "ocean_mixed_layer: bad dimensions");
  CICE_REQUIRE(a.dt > 0.0, "ocean_mixed_layer: dt must be positive");
  CICE_REQUIRE(a.tmask && a.potT && a.uatm && a.vatm && a.wind && a.zlvl && a.Qa && a.rhoa && a.flw && a.hmix && a.Tf &&
                   a.aice && a.fhocn && a.fswthru && a.swvdr && a.swvdf && a.swidr && a.swidf && a.sst && a.qdp && a.frzmlt &&
                   a.flwout_ocn && a.fsens_ocn && a.flat_ocn && a.evap_ocn && a.strairx_ocn && a.strairy_ocn && a.Tref_ocn &&
                   a.Qref_ocn && a.alvdr_ocn && a.alidr_ocn && a.alvdf_ocn && a.alidf_ocn, "ocean_mixed_layer: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), 1u, (unsigned)a.nb);
  hipLaunchKernelGGL(k_ocean_mixed_layer, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
