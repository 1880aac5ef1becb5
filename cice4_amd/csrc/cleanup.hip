// Kernels of the second half of step_therm2 (cleanup.h): the head of cleanup_itd, the eight passes of rebin, the zap of
// small areas with the flux update, aggregate with the tendencies.  Reference: source/ice_itd.F90:279-485, :557-793,
// :892-1340 (shift_ice with a single boundary), :1482-1590, :1600-2160; source/ice_step_mod.F90:504-509.
//
// A pass keeps donor, daice, dvice as scalars: the boundary and with it the donor and the receiver category are template
// parameters, so area, volume and snow volume of the five categories are registers with constant indices and the tracer
// products are formed where they are used.
#include "cleanup.h"

namespace cice {
namespace {

using ull = unsigned long long;
constexpr double puny = K::puny, c0 = 0.0, c1 = 1.0, p001 = K::p001;

__device__ __forceinline__ double fmax_(double a, double b) { return a > b ? a : b; }

struct CCell {
  int b, i, j;
  size_t q, o2, np;
  bool ok, phys;
};

__device__ __forceinline__ CCell ccell_of(const CleanArgs& A) {
  CCell c;
  c.np = (size_t)A.nx * A.ny;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  c.ok = t < c.np * (size_t)A.nblocks;
  c.b = c.ok ? (int)(t / c.np) : 0;
  c.q = c.ok ? t - (size_t)c.b * c.np : 0;
  c.j = (int)(c.q / A.nx) + 1;
  c.i = (int)(c.q % A.nx) + 1;
  c.o2 = (size_t)c.b * c.np + c.q;
  const int32_t* k = A.blk + 4 * c.b;
  c.phys = c.i >= k[0] && c.i <= k[1] && c.j >= k[2] && c.j <= k[3];
  return c;
}

// boundary (1-based), donor and receiver category (0-based) of pass P: up over boundaries 1..4, down over 4..1
template <int P> struct Pass {
  static constexpr bool up = P <= 4;
  static constexpr int N = up ? P : 9 - P;
  static constexpr int D = up ? N - 1 : N;
  static constexpr int R = up ? N : N - 1;
};

// rebin :663-673: category 1 is at least hin_max(0) thick.  Returns hicen(ij, 1) as rebin holds it in front of pass 1.
__device__ __forceinline__ double cat1_floor(const ItdParams& p, double& a0, double v0) {
  double h = a0 > puny ? v0 / a0 : c0;
  if (a0 > puny && h <= p.hin_max[0] && p.hin_max[0] > c0) {
    a0 = v0 / p.hin_max[0];
    h = p.hin_max[0];
  }
  return h;
}

// :694-695 / :750-751 for the donor category of pass P, thickness h
template <int P> __device__ __forceinline__ bool wants(const ItdParams& p, double ad, double h) {
  return ad > puny && (Pass<P>::up ? h > p.hin_max[Pass<P>::N] : h <= p.hin_max[Pass<P>::N]);
}

// a listed cell's word for pass P: 1 it wants the pass, cell + 2 it wants it and shift_ice would refuse it (vd < 0)
__device__ __forceinline__ void raise(ull* w, bool want, double vd, size_t q) {
  if (!want) return;
  if (vd < c0) atomicMax(w, (ull)q + 2);
  else if (*(volatile ull*)w == 0) atomicMax(w, 1ull);
}

__device__ __forceinline__ bool block_stopped(const ull* bw, int passes) {
  if (bw[CW_STOP_AREA]) return true;
  for (int k = 0; k < passes; ++k)
    if (bw[CW_PASS + k] >= 2) return true;
  return false;
}

// cleanup_itd :1724-1768: aggregate_area on every cell, the bounds check and the list on the physical cells; the need
// of pass 1 on the state as the lift of category 1 will leave it
__global__ __launch_bounds__(256) void k_clean_head(const CleanArgs A) {
  const CCell c = ccell_of(A);
  if (!c.ok) return;
  const size_t np = c.np;
  const double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double s = c0;
  double a0 = c0;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    const double x = pa[(size_t)n * np];
    if (n == 0) a0 = x;
    s = s + x;
  }
  A.aice[c.o2] = s;
  A.aice0[c.o2] = fmax_(c1 - s, c0);
  if (!c.phys) return;
  ull* bw = A.bw + (size_t)c.b * CW_WORDS;
  if (A.limit_aice && (s > c1 + puny || s < -puny)) {
    atomicMax(&bw[CW_STOP_AREA], (ull)c.q + 1);
    return;
  }
  if (!(s > puny)) return;
  const double v0 = A.vicen[(size_t)c.b * NCAT * np + c.q];
  const double h = cat1_floor(A.p, a0, v0);
  raise(&bw[CW_PASS], wants<1>(A.p, a0, h), v0, c.q);
}

// One pass of rebin.  Where the block's word is raised: shift_ice for the single boundary of the pass on every listed
// cell, `trcrn = c0` on the others.  Then the need of the next pass.
template <int P>
__global__ __launch_bounds__(256) void k_rebin_pass(const CleanArgs A) {
  constexpr int D = Pass<P>::D, R = Pass<P>::R;
  const CCell c = ccell_of(A);
  if (!c.ok) return;
  ull* bw = A.bw + (size_t)c.b * CW_WORDS;
  if (bw[CW_STOP_AREA]) return;
  const ItdParams& p = A.p;
  const size_t np = c.np;
  const bool listed = c.phys && A.aice[c.o2] > puny;
  double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
  double h0 = c0;                      // hicen(ij, 1) in front of pass 1
  if (P == 1 && listed) {              // the lift comes before the first shift_ice, which may stop
    double a0 = pa[0];
    const double was = a0;
    h0 = cat1_floor(p, a0, pv[0]);
    if (a0 != was) pa[0] = a0;
  }
  if (block_stopped(bw, P)) return;
  const bool fired = bw[CW_PASS + P - 1] != 0;
  if (!listed) {
    if (fired) {                       // compute_tracers :1536 from shift_ice :1331, every category
#pragma unroll
      for (int n = 0; n < NCAT; ++n)
#pragma unroll
        for (int it = 0; it < NTRCR; ++it)
          if (it < p.ntrcr) trc[(size_t)(n * NTRCR + it) * np] = c0;
    }
    return;
  }
  if (!fired) {
    if constexpr (P < 8) {             // the need of the next pass: two planes
      constexpr int Q = P + 1, D2 = Pass<Q>::D;
      const double ad = pa[(size_t)D2 * np], vd = pv[(size_t)D2 * np];
      raise(&bw[CW_PASS + Q - 1], wants<Q>(p, ad, ad > puny ? vd / ad : c0), vd, c.q);
    }
    return;
  }
  double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
  double a[NCAT], v[NCAT], s[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    a[n] = pa[(size_t)n * np];
    v[n] = pv[(size_t)n * np];
    s[n] = ps[(size_t)n * np];
  }
  const double hd = P == 1 ? h0 : (a[D] > puny ? v[D] / a[D] : c0);
  const bool move = wants<P>(p, a[D], hd);   // (v[D] >= 0: the block would have stopped otherwise)
  // the donor's and the receiver's area, volume, snow volume in front of the transfer: factors of their tracer products
  const double aD = a[D], vD = v[D], sD = s[D], aR = a[R], vR = v[R], sR = s[R];
  double da = c0, dv = c0, dvsnow = c0;
  if (move) {                          // :697-699 with the range checks :1055-1094, which leave daice, dvice as they are
    da = aD;
    dv = vD;
  }
  if (da > c0) {                       // :1198-1310
    double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
    double* es = A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q;
    const double wa = dv / vD;
    a[D] = aD - da; a[R] = aR + da;
    v[D] = vD - dv; v[R] = vR + dv;
    dvsnow = sD * wa;
    s[D] = sD - dvsnow; s[R] = sR + dvsnow;
#pragma unroll
    for (int k = 0; k < NILYR; ++k) {
      const double e = ei[(size_t)(D * NILYR + k) * np];
      const double deice = e * wa;
      ei[(size_t)(D * NILYR + k) * np] = e - deice;
      ei[(size_t)(R * NILYR + k) * np] = ei[(size_t)(R * NILYR + k) * np] + deice;
    }
#pragma unroll
    for (int k = 0; k < NSLYR; ++k) {
      const double e = es[(size_t)(D * NSLYR + k) * np];
      const double desnow = e * wa;
      es[(size_t)(D * NSLYR + k) * np] = e - desnow;
      es[(size_t)(R * NSLYR + k) * np] = es[(size_t)(R * NSLYR + k) * np] + desnow;
    }
    pa[(size_t)D * np] = a[D]; pa[(size_t)R * np] = a[R];
    pv[(size_t)D * np] = v[D]; pv[(size_t)R * np] = v[R];
    ps[(size_t)D * np] = s[D]; ps[(size_t)R * np] = s[R];
  }
  // every tracer of every category through its product and back (:1015-1037, :1235-1262, compute_tracers :1542-1588)
#pragma unroll
  for (int it = 0; it < NTRCR; ++it) {
    if (it < p.ntrcr) {
      const int dep = p.dep[it];
      const double tD = trc[(size_t)(D * NTRCR + it) * np];
      const double datrcr = dep == 0 ? da * tD : (dep == 1 ? dv * tD : dvsnow * tD);
#pragma unroll
      for (int n = 0; n < NCAT; ++n) {
        const double t = n == D ? tD : trc[(size_t)(n * NTRCR + it) * np];
        const double before = n == D ? (dep == 0 ? aD : (dep == 1 ? vD : sD))
                              : n == R ? (dep == 0 ? aR : (dep == 1 ? vR : sR))
                                       : (dep == 0 ? a[n] : (dep == 1 ? v[n] : s[n]));
        double atr = before * t;
        if (da > c0 && n == D) atr = atr - datrcr;
        if (da > c0 && n == R) atr = atr + datrcr;
        double out;
        if (it == p.it_Tsfc) out = a[n] > puny ? atr / a[n] : K::Tocnfrz;
        else if (dep == 0) out = a[n] > puny ? atr / a[n] : c0;
        else if (dep == 1) out = v[n] > c0 ? atr / v[n] : c0;
        else out = s[n] > c0 ? atr / s[n] : c0;
        trc[(size_t)(n * NTRCR + it) * np] = out;
      }
    }
  }
  if constexpr (P < 8) {
    constexpr int Q = P + 1, D2 = Pass<Q>::D;
    raise(&bw[CW_PASS + Q - 1], wants<Q>(p, a[D2], a[D2] > puny ? v[D2] / a[D2] : c0), v[D2], c.q);
  }
}

// zap_small_areas :1943-1968: the first category with a cell aicen < -puny on the physical domain, in it the first cell
__global__ __launch_bounds__(256) void k_clean_scan(const CleanArgs A) {
  const CCell c = ccell_of(A);
  if (!c.ok || !c.phys) return;
  ull* bw = A.bw + (size_t)c.b * CW_WORDS;
  if (block_stopped(bw, 8)) return;
  const double* pa = A.aicen + (size_t)c.b * NCAT * c.np + c.q;
#pragma unroll
  for (int n = 0; n < NCAT; ++n)
    if (pa[(size_t)n * c.np] < -puny) {
      atomicMax(&bw[CW_ZAP], (ull)(NCAT - n) << 32 | (ull)(c.np - c.q));
      return;
    }
}

// zap_small_areas :1943-2158 on the physical cells, then the flux update :1811-1816 on the whole plane
__global__ __launch_bounds__(256) void k_clean_zap(const CleanArgs A) {
  const CCell c = ccell_of(A);
  if (!c.ok) return;
  const ull* bw = A.bw + (size_t)c.b * CW_WORDS;
  if (block_stopped(bw, 8)) return;
  const ItdParams& p = A.p;
  const size_t np = c.np;
  const double dt = A.dt;
  const ull zw = bw[CW_ZAP];
  const int nend = zw ? NCAT - (int)(zw >> 32) : NCAT;   // categories in front of a negative area are zapped
  double dfresh = c0, dfsalt = c0, dfhocn = c0;
  if (c.phys && A.limit_aice) {
    double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
    double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
    double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
    double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
    double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
    double* es = A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q;
    double aice0 = A.aice0[c.o2];
    bool zapped = false;
#pragma unroll
    for (int n = 0; n < NCAT; ++n) {
      if (n < nend) {
        const double an = pa[(size_t)n * np];
        const double mag = an < c0 ? -an : an;
        if (mag != c0 && mag <= puny) {
#pragma unroll
          for (int k = 0; k < NILYR; ++k) {
            dfhocn = dfhocn + ei[(size_t)(n * NILYR + k) * np] / dt;
            ei[(size_t)(n * NILYR + k) * np] = c0;
          }
#pragma unroll
          for (int k = 0; k < NSLYR; ++k) {
            dfhocn = dfhocn + es[(size_t)(n * NSLYR + k) * np] / dt;
            es[(size_t)(n * NSLYR + k) * np] = c0;
          }
          const double vn = pv[(size_t)n * np], sn = ps[(size_t)n * np];
          dfresh = dfresh + (K::rhoi * vn + K::rhos * sn) / dt;
          dfsalt = dfsalt + K::rhoi * vn * K::ice_ref_salinity * p001 / dt;
          aice0 = aice0 + an;
          zapped = true;
          pa[(size_t)n * np] = c0;
          pv[(size_t)n * np] = c0;
          ps[(size_t)n * np] = c0;
          trc[(size_t)(n * NTRCR + p.it_Tsfc) * np] = K::Tocnfrz;
#pragma unroll
          for (int it = 1; it < NTRCR; ++it)   // :2037-2045 "this assumes nt_Tsfc = 1"
            if (it < p.ntrcr) trc[(size_t)(n * NTRCR + it) * np] = c0;
        }
      }
    }
    if (zapped) A.aice0[c.o2] = aice0;
    const double aice = A.aice[c.o2];  // as the head left it: the reference does not refresh it behind the zaps
    if (!zw && aice > c1 && aice < c1 + puny) {   // :2065-2158
#pragma unroll
      for (int n = 0; n < NCAT; ++n) {
#pragma unroll
        for (int k = 0; k < NILYR; ++k) {
          const double e = ei[(size_t)(n * NILYR + k) * np];
          dfhocn = dfhocn + e * (aice - c1) / aice / dt;
          ei[(size_t)(n * NILYR + k) * np] = e * (c1 / aice);
        }
#pragma unroll
        for (int k = 0; k < NSLYR; ++k) {
          const double e = es[(size_t)(n * NSLYR + k) * np];
          dfhocn = dfhocn + e * (aice - c1) / aice / dt;
          es[(size_t)(n * NSLYR + k) * np] = e * (c1 / aice);
        }
        const double an = pa[(size_t)n * np], vn = pv[(size_t)n * np], sn = ps[(size_t)n * np];
        dfresh = dfresh + (K::rhoi * vn + K::rhos * sn) * (aice - c1) / aice / dt;
        dfsalt = dfsalt + K::rhoi * vn * K::ice_ref_salinity * p001 * (aice - c1) / aice / dt;
        pa[(size_t)n * np] = an * (c1 / aice);
        pv[(size_t)n * np] = vn * (c1 / aice);
        ps[(size_t)n * np] = sn * (c1 / aice);
      }
      A.aice[c.o2] = c1;
      A.aice0[c.o2] = c0;
    }
  }
  if (zw) return;                      // a stop: the fluxes stay
  if (A.fresh) A.fresh[c.o2] = A.fresh[c.o2] + dfresh;
  if (A.fsalt) A.fsalt[c.o2] = A.fsalt[c.o2] + dfsalt;
  if (A.fhocn) A.fhocn[c.o2] = A.fhocn[c.o2] + dfhocn;
}

// aggregate :364-481 on every cell of the block, then ice_step_mod.F90:504-509
__global__ __launch_bounds__(256) void k_aggregate_full(const CleanArgs A) {
  const CCell c = ccell_of(A);
  if (!c.ok) return;
  const ItdParams& p = A.p;
  const size_t np = c.np;
  double aice = c0, vice = c0, vsno = c0, eice = c0, esno = c0, aice0 = c1;
  double* trcr = A.trcr + (size_t)c.b * NTRCR * np + c.q;
  if (A.tmask[c.o2]) {
    const double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
    const double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
    const double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
    const double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
    const double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
    const double* es = A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q;
    double atr[NTRCR];
#pragma unroll
    for (int it = 0; it < NTRCR; ++it) atr[it] = c0;
#pragma unroll
    for (int n = 0; n < NCAT; ++n) {
      const double an = pa[(size_t)n * np], vn = pv[(size_t)n * np], sn = ps[(size_t)n * np];
      aice = aice + an;
      vice = vice + vn;
      vsno = vsno + sn;
#pragma unroll
      for (int it = 0; it < NTRCR; ++it)
        if (it < p.ntrcr) {
          const double t = trc[(size_t)(n * NTRCR + it) * np];
          atr[it] = atr[it] + (p.dep[it] == 0 ? t * an : (p.dep[it] == 1 ? t * vn : t * sn));
        }
#pragma unroll
      for (int k = 0; k < NILYR; ++k) eice = eice + ei[(size_t)(n * NILYR + k) * np];
#pragma unroll
      for (int k = 0; k < NSLYR; ++k) esno = esno + es[(size_t)(n * NSLYR + k) * np];
    }
    aice0 = fmax_(c1 - aice, c0);
#pragma unroll
    for (int it = 0; it < NTRCR; ++it)
      if (it < p.ntrcr) {
        double t;
        if (it == p.it_Tsfc) t = aice > puny ? atr[it] / aice : K::Tocnfrz;
        else if (p.dep[it] == 0) t = aice > puny ? atr[it] / aice : c0;
        else if (p.dep[it] == 1) t = vice > c0 ? atr[it] / vice : c0;
        else t = vsno > c0 ? atr[it] / vsno : c0;
        trcr[(size_t)it * np] = t;
      }
  } else {
#pragma unroll
    for (int it = 0; it < NTRCR; ++it)
      if (it < p.ntrcr) trcr[(size_t)it * np] = c0;
  }
  A.aice[c.o2] = aice; A.aice0[c.o2] = aice0;
  A.vice[c.o2] = vice; A.vsno[c.o2] = vsno;
  A.eice[c.o2] = eice; A.esno[c.o2] = esno;
  if (A.daidtt) A.daidtt[c.o2] = (aice - A.daidtt[c.o2]) / A.dt;
  if (A.dvidtt) A.dvidtt[c.o2] = (vice - A.dvidtt[c.o2]) / A.dt;
}

__global__ __launch_bounds__(256) void k_level_transpose(const double* __restrict__ src, double* __restrict__ dst, size_t np,
                                                        int levels, int nb, int to_levels_outer) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= np * (size_t)levels * nb) return;
  const size_t q = t % np, r = t / np;           // t addresses (q, level, block): the batch's order
  const size_t l = r % levels, b = r / levels;
  const size_t u = (l * nb + b) * np + q;        // (q, block, level): the Halo's
  if (to_levels_outer) dst[u] = src[t];
  else dst[t] = src[u];
}

inline unsigned grid_of(const CleanArgs& a) {
  const size_t n = (size_t)a.nx * a.ny * a.nblocks;
  return (unsigned)((n + 255) / 256);
}

template <int P> void launch_pass(const CleanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rebin_pass<P>, dim3(grid_of(a)), dim3(256), 0, s, a);
}

}  // namespace

int clean_decode(const unsigned long long* w, size_t np, size_t* q) {
  if (w[CW_STOP_AREA]) { *q = (size_t)w[CW_STOP_AREA] - 1; return 1; }
  for (int k = 0; k < 8; ++k)
    if (w[CW_PASS + k] >= 2) { *q = (size_t)w[CW_PASS + k] - 2; return 2; }
  if (w[CW_ZAP]) { *q = np - (size_t)(w[CW_ZAP] & 0xffffffffull); return 3; }
  return 0;
}

void clean_launch_head(const CleanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_clean_head, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void clean_launch_pass(const CleanArgs& a, int p, hipStream_t s) {
  switch (p) {
    case 1: launch_pass<1>(a, s); break;
    case 2: launch_pass<2>(a, s); break;
    case 3: launch_pass<3>(a, s); break;
    case 4: launch_pass<4>(a, s); break;
    case 5: launch_pass<5>(a, s); break;
    case 6: launch_pass<6>(a, s); break;
    case 7: launch_pass<7>(a, s); break;
    case 8: launch_pass<8>(a, s); break;
    default: throw Error{CICE_EINVAL, "rebin pass out of range"};
  }
  CICE_HIP(hipGetLastError());
}

void clean_launch_zap(const CleanArgs& a, hipStream_t s) {
  if (a.limit_aice) hipLaunchKernelGGL(k_clean_scan, dim3(grid_of(a)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_clean_zap, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void clean_launch_aggregate(const CleanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_aggregate_full, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void clean_launch_all(const CleanArgs& a, hipStream_t s, hipEvent_t* ev) {
  int e = 0;
  auto mark = [&] { if (ev) CICE_HIP(hipEventRecord(ev[e++], s)); };
  mark();
  clean_launch_head(a, s);
  for (int p = 1; p <= 8; ++p) {
    mark();
    clean_launch_pass(a, p, s);
  }
  mark();
  clean_launch_zap(a, s);
  mark();
}

void clean_launch_transpose(const double* src, double* dst, size_t np, int levels, int nb, bool to_levels_outer,
                            hipStream_t s) {
  const size_t n = np * (size_t)levels * nb;
  hipLaunchKernelGGL(k_level_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, np, levels, nb,
                     to_levels_outer ? 1 : 0);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
