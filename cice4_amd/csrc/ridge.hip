// Kernels of ridge_ice (ridge.h).  Reference: source/ice_mechred.F90:133-552, :573-745, :773-1081, :1099-1773,
// :1788-1842; source/ice_itd.F90:1482-1590.
#include "ridge.h"

#include "libm_exact_neg.h"

namespace cice {
namespace {

using ull = unsigned long long;
constexpr double puny = K::puny, c0 = 0.0, c1 = 1.0, c2 = 2.0;
// ice_mechred.F90:82-100
constexpr double Cs = 0.25, fsnowrdg = 0.5, Gstar = 0.15, astar = 0.05, maxraft = 1.0;
static_assert(NSLYR == 1, "esnow_mlt is summed category by category, layer by layer: one snow layer per pass below");

__device__ __forceinline__ double fmax_(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double fmin_(double a, double b) { return a < b ? a : b; }

struct RCell {
  int b;
  size_t q, o2, np;
  bool ok;
  unsigned pos;     // list position, 0 = not listed
};

__device__ __forceinline__ RCell rcell_of(const RidgeArgs& A) {
  RCell c;
  c.np = (size_t)A.nx * A.ny;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  c.ok = t < c.np * (size_t)A.nblocks;
  c.b = c.ok ? (int)(t / c.np) : 0;
  c.q = c.ok ? t - (size_t)c.b * c.np : 0;
  c.o2 = (size_t)c.b * c.np + c.q;
  c.pos = c.ok ? (unsigned)A.listpos[c.o2] : 0u;
  return c;
}

// A block's word is raised to `value` by ONE lane per wavefront and block, chosen among the lanes that call (a wavefront
// may straddle two blocks; then every lane of the other block goes itself).  Every listed cell raising the word of
// iteration 1 on its own is 1e5 atomics on one address: 0.7 ms at gx1 size.
__device__ __forceinline__ void raise(ull* w, int b, ull value = 1ull) {
  const unsigned long long active = __ballot(1);
  const int leader = __ffsll((long long)active) - 1;
  const int lb = __shfl(b, leader);
  if ((int)(threadIdx.x & 63) == leader || b != lb)
    if (*(volatile ull*)w < value) atomicMax(w, value);
}

// ridge_itd :773-1081 for krdg_redist = 1
struct RItd {
  double aksum, apartic[NCAT + 1], hrmin[NCAT], hrexp[NCAT], krdg[NCAT];
};

__device__ __forceinline__ void ridge_itd(const RidgeParams& r, double aice0, const double* a, const double* v, RItd& o) {
  const double Gstari = c1 / Gstar, astari = c1 / astar;
  double G[NCAT + 2];                  // G[n + 1] = Gsum(n), n = -1..ncat
  G[0] = c0;
  G[1] = aice0 > puny ? aice0 : G[0];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) G[n + 2] = a[n] > puny ? G[n + 1] + a[n] : G[n + 1];
  const double work = c1 / G[NCAT + 1];
#pragma unroll
  for (int n = 0; n <= NCAT; ++n) G[n + 1] = G[n + 1] * work;
  if (r.krdg_partic == 0) {            // Thorndike et al. 1975
#pragma unroll
    for (int n = 0; n <= NCAT; ++n) {
      const double Gm = G[n], Gn = G[n + 1];
      double ap = c0;
      if (Gn < Gstar) ap = Gstari * (Gn - Gm) * (c2 - (Gm + Gn) * Gstari);
      else if (Gm < Gstar) ap = Gstari * (Gstar - Gm) * (c2 - (Gm + Gstar) * Gstari);
      o.apartic[n] = ap;
    }
  } else {                             // exponential dependence on G(h)
    const double xtmp = c1 / (c1 - exp_libm_neg(-astari));
#pragma unroll
    for (int n = 0; n <= NCAT + 1; ++n) G[n] = exp_libm_neg(-G[n] * astari) * xtmp;
#pragma unroll
    for (int n = 0; n <= NCAT; ++n) o.apartic[n] = G[n] - G[n + 1];
  }
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    o.hrmin[n] = c0;
    o.hrexp[n] = c0;
    o.krdg[n] = c1;
    if (a[n] > puny) {
      double hi = v[n] / a[n];
      hi = fmax_(hi, puny);
      o.hrmin[n] = fmin_(c2 * hi, hi + maxraft);
      o.hrexp[n] = r.mu_rdg * sqrt(hi);
      o.krdg[n] = (o.hrmin[n] + o.hrexp[n]) / hi;
    }
  }
  double aksum = o.apartic[0];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) aksum = aksum + o.apartic[n + 1] * (c1 - c1 / o.krdg[n]);
  o.aksum = aksum;
}

__device__ __forceinline__ bool block_dead(const ull* bw) { return bw[RW_STOP_AICE0] != 0 || bw[RW_STOP_ARDG] != 0; }

// Iteration `iter`, first half: [asum_ridging, ridge_prep :283-296,] ridge_itd, ridge_shift :1285-1352 up to the new aice0
template <bool FIRST>
__global__ __launch_bounds__(256) void k_ridge_rates(const RidgeArgs A, const int iter) {
  const RCell c = rcell_of(A);
  if (!c.ok || !c.pos) return;
  ull* bw = A.bw + (size_t)c.b * RW_WORDS;
  if (!FIRST && (!bw[RW_ITER + iter] || block_dead(bw))) return;
  const size_t np = c.np, nall = np * (size_t)A.nblocks;
  double* W = A.work + c.o2;
  const double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  const double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  const double dt = A.dt;
  double a[NCAT], v[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    a[n] = pa[(size_t)n * np];
    v[n] = pv[(size_t)n * np];
  }
  const double aice0 = A.aice0[c.o2];
  double closing_net, opning;
  if (FIRST) {
    double asum = aice0;
#pragma unroll
    for (int n = 0; n < NCAT; ++n) asum = asum + a[n];
    closing_net = Cs * A.rdg_shear[c.o2] + A.rdg_conv[c.o2];
    const double divu_adv = (c1 - asum) / dt;
    if (divu_adv < c0) closing_net = fmax_(closing_net, -divu_adv);
    opning = closing_net + divu_adv;
    W[RG_ARDG1 * nall] = c0; W[RG_ARDG2 * nall] = c0; W[RG_VIRDG * nall] = c0; W[RG_AOPEN * nall] = c0;
    W[RG_MSNOW * nall] = c0; W[RG_ESNOW * nall] = c0;
    raise(&bw[RW_ITER + 1], c.b);
  } else {
    closing_net = W[RG_CLOSING * nall];
    opning = W[RG_OPNING * nall];
  }
  RItd t;
  ridge_itd(A.r, aice0, a, v, t);
  double cg = closing_net / t.aksum;
  if (t.apartic[0] > c0) {             // no more than all of the open water
    const double wk1 = t.apartic[0] * cg * dt;
    if (wk1 > aice0) {
      const double tmpfac = aice0 / wk1;
      cg = cg * tmpfac;
      opning = opning * tmpfac;
    }
  }
#pragma unroll
  for (int n = 0; n < NCAT; ++n)       // no more than all of a category
    if (a[n] > puny && t.apartic[n + 1] > c0) {
      const double wk1 = t.apartic[n + 1] * cg * dt;
      if (wk1 > a[n]) {
        const double tmpfac = a[n] / wk1;
        cg = cg * tmpfac;
        opning = opning * tmpfac;
      }
    }
  const double aice0n = aice0 - t.apartic[0] * cg * dt + opning * dt;
  W[RG_CGROSS * nall] = cg;
  W[RG_OPNING * nall] = opning;
  W[RG_AICE0N * nall] = aice0n;
  if (aice0n < -puny) atomicMax(&bw[RW_STOP_AICE0], (ull)(0xffffffffu - c.pos));
}

// Iteration `iter`, second half: the rest of ridge_shift :1354-1771, asum_ridging, ridge_check
__global__ __launch_bounds__(256) void k_ridge_shift(const RidgeArgs A, const int iter) {
  const RCell c = rcell_of(A);
  if (!c.ok) return;
  ull* bw = A.bw + (size_t)c.b * RW_WORDS;
  if (!bw[RW_ITER + iter] || bw[RW_STOP_ARDG]) return;
  const size_t np = c.np, nall = np * (size_t)A.nblocks;
  double* W = A.work + c.o2;
  const ull stop0 = bw[RW_STOP_AICE0];
  if (stop0) {                         // :1341-1356 ran up to the failing cell, nothing else of this iteration
    const unsigned fail = 0xffffffffu - (unsigned)stop0;
    if (c.pos && c.pos <= fail) {
      const double x = W[RG_AICE0N * nall];
      A.aice0[c.o2] = (x < c0 && !(x < -puny)) ? c0 : x;
    }
    return;
  }
  const ItdParams& p = A.p;
  double* trc = A.trcrn + (size_t)c.b * NCAT * NTRCR * np + c.q;
  if (!c.pos) {                        // compute_tracers :1536, every category
#pragma unroll
    for (int n = 0; n < NCAT; ++n)
#pragma unroll
      for (int it = 0; it < NTRCR; ++it)
        if (it < p.ntrcr) trc[(size_t)(n * NTRCR + it) * np] = c0;
    return;
  }
  double* pa = A.aicen + (size_t)c.b * NCAT * np + c.q;
  double* pv = A.vicen + (size_t)c.b * NCAT * np + c.q;
  double* ps = A.vsnon + (size_t)c.b * NCAT * np + c.q;
  const double dt = A.dt;
  double a[NCAT], v[NCAT], s[NCAT], ai[NCAT], vi[NCAT], si[NCAT];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    a[n] = ai[n] = pa[(size_t)n * np];
    v[n] = vi[n] = pv[(size_t)n * np];
    s[n] = si[n] = ps[(size_t)n * np];
  }
  RItd t;
  ridge_itd(A.r, A.aice0[c.o2], ai, vi, t);
  const double cg = W[RG_CGROSS * nall], opning = W[RG_OPNING * nall];
  double aice0 = W[RG_AICE0N * nall];
  if (aice0 < c0) aice0 = c0;          // roundoff (the block has no cell below -puny)
  A.aice0[c.o2] = aice0;
  W[RG_AOPEN * nall] = opning * dt;

  // what category n gives and where it goes: from the snapshot alone
  bool rdg[NCAT], any = false;
  double afrac[NCAT], ardg1n[NCAT], ardg2n[NCAT], virdgn[NCAT], vsrdgn[NCAT], farea[NCAT][NCAT], fvol[NCAT][NCAT];
  double ardg1 = W[RG_ARDG1 * nall], ardg2 = W[RG_ARDG2 * nall], virdg = W[RG_VIRDG * nall], msnow = W[RG_MSNOW * nall];
#pragma unroll
  for (int n = 0; n < NCAT; ++n) {
    rdg[n] = ai[n] > puny && t.apartic[n + 1] > c0 && cg > c0;
    afrac[n] = ardg1n[n] = ardg2n[n] = virdgn[n] = vsrdgn[n] = c0;
#pragma unroll
    for (int nr = 0; nr < NCAT; ++nr) farea[n][nr] = fvol[n][nr] = c0;
    if (!rdg[n]) continue;
    any = true;
    double x = t.apartic[n + 1] * cg * dt;
    if (x > ai[n] + puny) {            // :1432, unreachable (ridge.h)
      atomicMax(&bw[RW_STOP_ARDG], (ull)(NCAT - n) << 32 | (ull)(0xffffffffu - c.pos));
      return;
    }
    x = fmin_(ai[n], x);
    ardg1n[n] = x;
    ardg2n[n] = x / t.krdg[n];
    afrac[n] = x / ai[n];
    virdgn[n] = vi[n] * afrac[n];
    vsrdgn[n] = si[n] * afrac[n];
    ardg1 = ardg1 + ardg1n[n];
    ardg2 = ardg2 + ardg2n[n];
    virdg = virdg + virdgn[n];
    msnow = msnow + K::rhos * vsrdgn[n] * (c1 - fsnowrdg);
    const double hi1 = t.hrmin[n], hexp = t.hrexp[n];
#pragma unroll
    for (int nr = 0; nr < NCAT; ++nr) {   // :1622-1659; hin_max(nr - 1) = p.hin_max[nr]
      if (nr < NCAT - 1) {
        if (!(hi1 >= p.hin_max[nr + 1])) {
          const double hL = fmax_(hi1, p.hin_max[nr]), hR = p.hin_max[nr + 1];
          const double expL = exp_libm_neg(-(hL - hi1) / hexp), expR = exp_libm_neg(-(hR - hi1) / hexp);
          farea[n][nr] = expL - expR;
          fvol[n][nr] = ((hL + hexp) * expL - (hR + hexp) * expR) / (hi1 + hexp);
        }
      } else {
        const double hL = fmax_(hi1, p.hin_max[nr]);
        const double expL = exp_libm_neg(-(hL - hi1) / hexp);
        farea[n][nr] = expL;
        fvol[n][nr] = (hL + hexp) * expL / (hi1 + hexp);
      }
    }
  }
  if (any) {
    W[RG_ARDG1 * nall] = ardg1; W[RG_ARDG2 * nall] = ardg2; W[RG_VIRDG * nall] = virdg; W[RG_MSNOW * nall] = msnow;
    // area, ice volume, snow volume :1458-1460, :1673-1676
#pragma unroll
    for (int n = 0; n < NCAT; ++n)
      if (rdg[n]) {
        a[n] = a[n] - ardg1n[n];
        v[n] = v[n] - virdgn[n];
        s[n] = s[n] - vsrdgn[n];
#pragma unroll
        for (int nr = 0; nr < NCAT; ++nr) {
          a[nr] = a[nr] + farea[n][nr] * ardg2n[n];
          v[nr] = v[nr] + fvol[n][nr] * virdgn[n];
          s[nr] = s[nr] + fvol[n][nr] * vsrdgn[n] * fsnowrdg;
        }
      }
#pragma unroll
    for (int n = 0; n < NCAT; ++n) {
      pa[(size_t)n * np] = a[n];
      pv[(size_t)n * np] = v[n];
      ps[(size_t)n * np] = s[n];
    }
    // ice energy, layer by layer :1513-1515, :1689-1690
    double* ei = A.eicen + (size_t)c.b * NCAT * NILYR * np + c.q;
#pragma unroll
    for (int k = 0; k < NILYR; ++k) {
      double e[NCAT], e0[NCAT];
#pragma unroll
      for (int n = 0; n < NCAT; ++n) e[n] = e0[n] = ei[(size_t)(n * NILYR + k) * np];
#pragma unroll
      for (int n = 0; n < NCAT; ++n)
        if (rdg[n]) {
          const double d = e0[n] * afrac[n];
          e[n] = e[n] - d;
#pragma unroll
          for (int nr = 0; nr < NCAT; ++nr) e[nr] = e[nr] + fvol[n][nr] * d;
        }
#pragma unroll
      for (int n = 0; n < NCAT; ++n) ei[(size_t)(n * NILYR + k) * np] = e[n];
    }
    // snow energy :1534-1538, :1704-1705
    double* es = A.esnon + (size_t)c.b * NCAT * NSLYR * np + c.q;
    double esnow = W[RG_ESNOW * nall];
    {
      double e[NCAT], e0[NCAT];
#pragma unroll
      for (int n = 0; n < NCAT; ++n) e[n] = e0[n] = es[(size_t)n * np];
#pragma unroll
      for (int n = 0; n < NCAT; ++n)
        if (rdg[n]) {
          const double d = e0[n] * afrac[n];
          e[n] = e[n] - d;
          esnow = esnow + d * (c1 - fsnowrdg);
#pragma unroll
          for (int nr = 0; nr < NCAT; ++nr) e[nr] = e[nr] + fvol[n][nr] * d * fsnowrdg;
        }
#pragma unroll
      for (int n = 0; n < NCAT; ++n) es[(size_t)n * np] = e[n];
    }
    W[RG_ESNOW * nall] = esnow;
  }
  // every tracer of every category through its product and back :1252-1274, :1479-1480, :1555-1580, :1726-1751,
  // compute_tracers -- also where nothing ridged
#pragma unroll
  for (int it = 0; it < NTRCR; ++it) {
    if (it < p.ntrcr) {
      const int dep = p.dep[it];
      const bool lvl = p.tr_lvl && (it == p.it_alvl || it == p.it_vlvl);
      double tr[NCAT], at[NCAT];
#pragma unroll
      for (int n = 0; n < NCAT; ++n) {
        tr[n] = trc[(size_t)(n * NTRCR + it) * np];
        at[n] = (dep == 0 ? ai[n] : (dep == 1 ? vi[n] : si[n])) * tr[n];
      }
#pragma unroll
      for (int n = 0; n < NCAT; ++n)
        if (rdg[n]) {
          if (lvl) at[n] = at[n] * (c1 - afrac[n]);
          at[n] = at[n] - (dep == 0 ? ardg1n[n] : (dep == 1 ? virdgn[n] : vsrdgn[n])) * tr[n];
#pragma unroll
          for (int nr = 0; nr < NCAT; ++nr) {
            const double w = dep == 0 ? farea[n][nr] * ardg2n[n]
                                      : (dep == 1 ? fvol[n][nr] * virdgn[n] : fvol[n][nr] * vsrdgn[n] * fsnowrdg);
            at[nr] = at[nr] + w * tr[n];
          }
        }
#pragma unroll
      for (int n = 0; n < NCAT; ++n) {
        double out;
        if (it == p.it_Tsfc) out = a[n] > puny ? at[n] / a[n] : K::Tocnfrz;
        else if (dep == 0) out = a[n] > puny ? at[n] / a[n] : c0;
        else if (dep == 1) out = v[n] > c0 ? at[n] / v[n] : c0;
        else out = s[n] > c0 ? at[n] / s[n] : c0;
        trc[(size_t)(n * NTRCR + it) * np] = out;
      }
    }
  }
  // asum_ridging :370-373, ridge_check :1828-1840
  double asum = aice0;
#pragma unroll
  for (int n = 0; n < NCAT; ++n) asum = asum + a[n];
  const double off = asum - c1;
  if ((off < c0 ? -off : off) < puny) {
    W[RG_CLOSING * nall] = c0;
    W[RG_OPNING * nall] = c0;
  } else {
    raise(&bw[RW_ITER + iter + 1], c.b);
    const double divu_adv = (c1 - asum) / dt;
    W[RG_CLOSING * nall] = fmax_(c0, -divu_adv);
    W[RG_OPNING * nall] = fmax_(c0, divu_adv);
  }
  raise(&bw[RW_NITER], c.b, (ull)iter);
}

// :478-526 where the loop came to its `exit`
__global__ __launch_bounds__(256) void k_ridge_finish(const RidgeArgs A) {
  const RCell c = rcell_of(A);
  if (!c.ok || !c.pos) return;
  const ull* bw = A.bw + (size_t)c.b * RW_WORDS;
  if (block_dead(bw) || bw[RW_ITER + RIDGE_NITERMAX + 1]) return;
  const size_t nall = c.np * (size_t)A.nblocks;
  const double* W = A.work + c.o2;
  const double dti = c1 / A.dt;
  if (A.dardg1dt) A.dardg1dt[c.o2] = W[RG_ARDG1 * nall] * dti;
  if (A.dardg2dt) A.dardg2dt[c.o2] = W[RG_ARDG2 * nall] * dti;
  if (A.dvirdgdt) A.dvirdgdt[c.o2] = W[RG_VIRDG * nall] * dti;
  if (A.opening) A.opening[c.o2] = W[RG_AOPEN * nall] * dti;
  if (A.fresh) A.fresh[c.o2] = A.fresh[c.o2] + W[RG_MSNOW * nall] * dti;
  if (A.fhocn) A.fhocn[c.o2] = A.fhocn[c.o2] + W[RG_ESNOW * nall] * dti;
}

__global__ __launch_bounds__(256) void k_ridge_list(int32_t* listpos, const int32_t* __restrict__ tmask,
                                                    const int32_t* __restrict__ blk, int nx, int ny, int nblocks) {
  const size_t np = (size_t)nx * ny, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= np * (size_t)nblocks) return;
  const int b = (int)(t / np);
  const size_t q = t - (size_t)b * np;
  const int i = (int)(q % nx) + 1, j = (int)(q / nx) + 1;
  const int32_t* k = blk + 4 * b;
  const bool phys = i >= k[0] && i <= k[1] && j >= k[2] && j <= k[3];
  // list order of ice_step_mod.F90:621-631 (j outer, i inner) over the physical cells: the position in the plane orders alike
  listpos[t] = phys && tmask[t] ? (int32_t)q + 1 : 0;
}

inline unsigned grid_of(const RidgeArgs& a) {
  const size_t n = (size_t)a.nx * a.ny * a.nblocks;
  return (unsigned)((n + 255) / 256);
}

}  // namespace

int ridge_decode(const unsigned long long* w, unsigned* listpos, int* niter) {
  *listpos = 0;
  *niter = (int)w[RW_NITER];
  if (w[RW_STOP_AICE0]) {
    *listpos = 0xffffffffu - (unsigned)w[RW_STOP_AICE0];
    *niter += 1;                       // the iteration that stopped has not counted itself
    return RIDGE_STOP_AICE0;
  }
  if (w[RW_STOP_ARDG]) {
    *listpos = 0xffffffffu - (unsigned)(w[RW_STOP_ARDG] & 0xffffffffull);
    return RIDGE_STOP_ARDG;
  }
  if (w[RW_ITER + RIDGE_NITERMAX + 1]) return RIDGE_STOP_NITER;
  return RIDGE_OK;
}

bool ridge_wants_more(const unsigned long long* w, int done) {
  return done < RIDGE_NITERMAX && !w[RW_STOP_AICE0] && !w[RW_STOP_ARDG] && w[RW_ITER + done + 1] != 0;
}

void ridge_launch_iterations(const RidgeArgs& a, int first, int count, hipStream_t s, hipEvent_t* ev) {
  if (first < 1 || count < 0 || first + count - 1 > RIDGE_NITERMAX) throw Error{CICE_EINVAL, "ridging iteration out of range"};
  int e = 0;
  auto mark = [&] { if (ev) CICE_HIP(hipEventRecord(ev[e++], s)); };
  for (int k = first; k < first + count; ++k) {
    mark();
    if (k == 1) hipLaunchKernelGGL(k_ridge_rates<true>, dim3(grid_of(a)), dim3(256), 0, s, a, k);
    else hipLaunchKernelGGL(k_ridge_rates<false>, dim3(grid_of(a)), dim3(256), 0, s, a, k);
    mark();
    hipLaunchKernelGGL(k_ridge_shift, dim3(grid_of(a)), dim3(256), 0, s, a, k);
  }
  mark();
  CICE_HIP(hipGetLastError());
}

void ridge_launch_finish(const RidgeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_ridge_finish, dim3(grid_of(a)), dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

void ridge_launch_list(int32_t* listpos, const int32_t* tmask, const int32_t* blk, int nx, int ny, int nblocks,
                       hipStream_t s) {
  const size_t n = (size_t)nx * ny * nblocks;
  hipLaunchKernelGGL(k_ridge_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, listpos, tmask, blk, nx, ny, nblocks);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
