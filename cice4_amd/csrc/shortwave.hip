// k_shortwave_ccsm3, k_prep_radiation (shortwave.h).
#include "shortwave.h"

#include <cmath>

namespace cice {

namespace {

// ice_constants.F90: Timelt, kappav; ice_shortwave.F90:637-639 (dalb_mltv, dalb_mlti), :869-872, :1032 (i0vis)
constexpr double Timelt = 0.0, kappav = 1.4, i0vis = 0.70;
constexpr double dalb_mltv = -0.1, dalb_mlti = -0.15;
constexpr double warmice = 0.68, coldice = 0.70, warmsnow = 0.77, coldsnow = 0.81;

__device__ inline bool physical(const int32_t* blk, int b, int q, int nx) {
  const int i = q % nx + 1, j = q / nx + 1;
  const int32_t* w = blk + 4 * b;
  return i >= w[0] && i <= w[1] && j >= w[2] && j <= w[3];
}

// Grid (chunks of 256 cells of a plane, categories, blocks), as k_state_from_transport: a plane of nx * ny cells is
// contiguous, a wavefront takes 64 consecutive cells of one (category, block): 512 contiguous bytes per array and access.
// A cell that is not on the list gets what the reference's whole-block initialisation leaves (:660-695, :883-898,
// :1059-1069): the ocean albedo in the four albedos, zero everywhere else.
__global__ __launch_bounds__(256) void k_shortwave_ccsm3(const ShortwaveArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int n = (int)blockIdx.y, b = (int)blockIdx.z;
  const size_t np = (size_t)a.np;
  const size_t cb = (size_t)b * a.ncat + n;          // (category, block)
  const size_t c = cb * np + q, c2 = (size_t)b * np + q;
  const ShortwaveParams& p = a.p;
  const double aicen = a.aicen[c];
  const double ocn = a.ocn_albedo ? a.ocn_albedo[c2] : p.albocn;
  const bool on = a.listed ? a.listed[q] != 0 : (physical(a.blk, b, q, a.nx) && aicen > K::puny);

  double alvdrn = ocn, alidrn = ocn, alvdfn = ocn, alidfn = ocn, albin = 0.0, albsn = 0.0;
  double fswsfc = 0.0, fswint = 0.0, fswthru = 0.0, Isw[NILYR];
#pragma unroll
  for (int k = 0; k < NILYR; ++k) Isw[k] = 0.0;

  if (on) {
    const double vicen = a.vicen[c], vsnon = a.vsnon[c], Tsfcn = a.Tsfc[cb * a.tsfc_planes * np + q];
    const double swvdr = a.swvdr[c2], swvdf = a.swvdf[c2], swidr = a.swidr[c2], swidf = a.swidf[c2];
    const double hs = vsnon / aicen;
    // ice and snow albedos (direct = diffuse)
    double alvdfni, alidfni, alvdfns, alidfns;
    if (p.albedo_type == 1) {            // constant_albedos (:909-954)
      double v;
      if (hs > K::puny)
        v = (Tsfcn >= -K::c2 * K::puny) ? warmsnow : coldsnow;
      else
        v = (Tsfcn >= -K::c2 * K::puny) ? warmice : coldice;
      alvdfni = alidfni = alvdfns = alidfns = v;
      alvdrn = alidrn = alvdfn = alidfn = v;
    } else {                             // compute_albedos (:705-778)
      const double hi = vicen / aicen;
      const double x = atan(hi * K::c4) / p.fhtan;
      const double fh = x < K::c1 ? x : K::c1;
      const double albo = ocn * (K::c1 - fh);
      alvdfni = p.albicev * fh + albo;
      alidfni = p.albicei * fh + albo;
      const double dTs = Timelt - Tsfcn;
      const double y = dTs / p.dT_mlt - K::c1;
      const double fT = y < K::c0 ? y : K::c0;
      alvdfni = alvdfni - p.dalb_mlt * fT;
      alidfni = alidfni - p.dalb_mlt * fT;
      alvdfni = alvdfni > ocn ? alvdfni : ocn;
      alidfni = alidfni > ocn ? alidfni : ocn;
      alvdfns = ocn;
      alidfns = ocn;
      if (hs > K::puny) {
        alvdfns = p.albsnowv;
        alidfns = p.albsnowi;
        alvdfns = alvdfns - dalb_mltv * fT;
        alidfns = alidfns - dalb_mlti * fT;
      }
    }
    const double alvdrni = alvdfni, alidrni = alidfni, alvdrns = alvdfns, alidrns = alidfns;
    double asnow = K::c0;
    if (hs > K::puny) asnow = hs / (hs + p.snowpatch);
    if (p.albedo_type != 1) {
      alvdfn = alvdfni * (K::c1 - asnow) + alvdfns * asnow;
      alidfn = alidfni * (K::c1 - asnow) + alidfns * asnow;
      alvdrn = alvdrni * (K::c1 - asnow) + alvdrns * asnow;
      alidrn = alidrni * (K::c1 - asnow) + alidrns * asnow;
    }
    albin = p.awtvdr * alvdrni + p.awtidr * alidrni + p.awtvdf * alvdfni + p.awtidf * alidfni;
    albsn = p.awtvdr * alvdrns + p.awtidr * alidrns + p.awtvdf * alvdfns + p.awtidf * alidfns;

    // absorbed_solar (:1071-1158)
    const double swabsv = swvdr * ((K::c1 - alvdrni) * (K::c1 - asnow) + (K::c1 - alvdrns) * asnow) +
                          swvdf * ((K::c1 - alvdfni) * (K::c1 - asnow) + (K::c1 - alvdfns) * asnow);
    const double swabsi = swidr * ((K::c1 - alidrni) * (K::c1 - asnow) + (K::c1 - alidrns) * asnow) +
                          swidf * ((K::c1 - alidfni) * (K::c1 - asnow) + (K::c1 - alidfns) * asnow);
    const double swabs = swabsv + swabsi;
    const double fswpenvdr = swvdr * (K::c1 - alvdrni) * (K::c1 - asnow) * i0vis;
    const double fswpenvdf = swvdf * (K::c1 - alvdfni) * (K::c1 - asnow) * i0vis;
    const double fswpen = fswpenvdr + fswpenvdf;
    fswsfc = swabs - fswpen;
    double trantop = K::c1, tranbot = K::c0;
#pragma unroll
    for (int k = 1; k <= NILYR; ++k) {
      const double hi = vicen / aicen;
      const double hilyr = hi / (double)NILYR;
      tranbot = exp_libm(-kappav * hilyr * (double)k);
      Isw[k - 1] = fswpen * (trantop - tranbot);
      trantop = tranbot;
    }
    fswthru = fswpen * tranbot;
    fswint = fswpen - fswthru;
  }

  a.alvdrn[c] = alvdrn; a.alidrn[c] = alidrn; a.alvdfn[c] = alvdfn; a.alidfn[c] = alidfn;
  a.albicen[c] = albin; a.albsnon[c] = albsn;
  a.fswsfcn[c] = fswsfc; a.fswintn[c] = fswint; a.fswthrun[c] = fswthru;
#pragma unroll
  for (int k = 0; k < NILYR; ++k) a.Iswabsn[(cb * NILYR + k) * np + q] = Isw[k];
  if (a.Sswabsn) {
#pragma unroll
    for (int k = 0; k < NSLYR; ++k) a.Sswabsn[(cb * NSLYR + k) * np + q] = 0.0;
  }
}

// Grid (chunks of 256 cells of a plane, 1, blocks); a thread owns a cell with all its categories
__global__ __launch_bounds__(256) void k_prep_radiation(const PrepRadiationArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int b = (int)blockIdx.z;
  if (!physical(a.blk, b, q, a.nx)) return;
  const size_t np = (size_t)a.np, c2 = (size_t)b * np + q;
  double sf = a.scale_factor[c2];
  if (a.aice[c2] > K::c0 && sf > K::puny) {
    const double netsw = a.swvdr[c2] * (K::c1 - a.alvdr_gbm[c2]) + a.swvdf[c2] * (K::c1 - a.alvdf_gbm[c2]) +
                         a.swidr[c2] * (K::c1 - a.alidr_gbm[c2]) + a.swidf[c2] * (K::c1 - a.alidf_gbm[c2]);
    sf = netsw / sf;
  } else {
    sf = K::c1;
  }
  a.scale_factor[c2] = sf;
  a.fswfac[c2] = sf;
  for (int n = 0; n < a.ncat; ++n) {
    const size_t cb = (size_t)b * a.ncat + n, c = cb * np + q;
    if (!(a.aicen[c] > K::puny)) continue;
    a.fswsfcn[c] = sf * a.fswsfcn[c];
    a.fswintn[c] = sf * a.fswintn[c];
    a.fswthrun[c] = sf * a.fswthrun[c];
#pragma unroll
    for (int k = 0; k < NSLYR; ++k) {
      double* w = a.Sswabsn + (cb * NSLYR + k) * np + q;
      *w = sf * *w;
    }
#pragma unroll
    for (int k = 0; k < NILYR; ++k) {
      double* w = a.Iswabsn + (cb * NILYR + k) * np + q;
      *w = sf * *w;
    }
  }
}

void check_dims(int nx, int np, int ncat, int nb, const char* what) {
  CICE_REQUIRE(nx >= 1 && np >= nx && np % nx == 0 && ncat >= 1 && nb >= 1, what);
  CICE_REQUIRE((long long)np < (1ll << 31) - 256, what);
  CICE_REQUIRE(ncat <= 65535 && nb <= 65535, what);
}

}  // namespace

void shortwave_launch(const ShortwaveArgs& a, hipStream_t s) {
  check_dims(a.nx, a.np, a.ncat, a.nb, "shortwave: bad dimensions");
  CICE_REQUIRE(a.tsfc_planes >= 1 && (a.listed || a.blk), "shortwave: no list");
  CICE_REQUIRE(!a.listed || (a.ncat == 1 && a.nb == 1), "shortwave: a list names the cells of one block and category");
  CICE_REQUIRE(a.aicen && a.vicen && a.vsnon && a.Tsfc && a.swvdr && a.swvdf && a.swidr && a.swidf && a.alvdrn && a.alidrn &&
                   a.alvdfn && a.alidfn && a.albicen && a.albsnon && a.fswsfcn && a.fswintn && a.fswthrun && a.Iswabsn,
               "shortwave: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), (unsigned)a.ncat, (unsigned)a.nb);
  hipLaunchKernelGGL(k_shortwave_ccsm3, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void prep_radiation_launch(const PrepRadiationArgs& a, hipStream_t s) {
  check_dims(a.nx, a.np, a.ncat, a.nb, "prep_radiation: bad dimensions");
  CICE_REQUIRE(a.blk && a.swvdr && a.swvdf && a.swidr && a.swidf && a.alvdr_gbm && a.alvdf_gbm && a.alidr_gbm && a.alidf_gbm &&
                   a.aice && a.aicen && a.scale_factor && a.fswfac && a.fswsfcn && a.fswintn && a.fswthrun && a.Sswabsn &&
                   a.Iswabsn, "prep_radiation: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), 1u, (unsigned)a.nb);
  hipLaunchKernelGGL(k_prep_radiation, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
