// atmo_boundary_layer (source/ice_atmo.F90:56-384) for gfx950.  One lane = one (cell[, category]); the cell routine
// is atmo_cell.h's: the five stability iterations (:264-305) run in registers.  exp is glibc's (libm_exact.h); log
// and atan are the device library's (<= 1 ulp): the outputs agree with the reference's to ~1e-15 relative, not bit
// for bit -- which is why the bit-exact whole-driver configuration keeps the reference's host routine (DESIGN.md
// section 3.6).
#include <cmath>

#include "atmo.h"
#include "atmo_cell.h"

namespace cice {

void AtmoParams::init() {
  vonkar = 0.4; gravit = 9.80616; zvir = 0.606; cp_air = 1005.0; cpvir = 1.81e3 / 1005.0 - 1.0;
  Tffresh = 273.15; pih = 0.5 * 3.14159265358979323846; zTrf = 2.0; umin = 1.0; zref = 10.0;
  qqq[0] = 11637800.0; TTT[0] = 5897.8; Lheat[0] = 2.835e6;
  qqq[1] = 627572.4; TTT[1] = 5107.4; Lheat[1] = 2.501e6;
  rdn_ice = vonkar / std::log(zref / 0.0005);
  al2 = std::log(zref / zTrf);
}

namespace {

// one block, the reference's list: everything is zeroed first (:179-188, :313-318), then the listed cells
__global__ __launch_bounds__(256) void k_atmo_zero(AtmoArgs a) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)a.nx * a.ny) return;
  a.Tref[q] = 0.0; a.Qref[q] = 0.0; a.delt[q] = 0.0; a.delq[q] = 0.0; a.shcoef[q] = 0.0; a.lhcoef[q] = 0.0;
  if (a.calc_strair) { a.strx[q] = 0.0; a.stry[q] = 0.0; }
}
__global__ __launch_bounds__(256) void k_atmo_list(AtmoArgs a) {
  const int ij = blockIdx.x * 256 + threadIdx.x;
  if (ij >= a.icells) return;
  const size_t q = (size_t)(a.indxj[ij] - 1) * a.nx + (a.indxi[ij] - 1);
  const AtmoOut o = atmo_cell(a.p, a.ocn, a.Tsf[q], a.potT[q], a.uatm[q], a.vatm[q], a.wind[q], a.zlvl[q], a.Qa[q],
                              a.rhoa[q]);
  if (a.calc_strair) { a.strx[q] = o.strx; a.stry[q] = o.stry; }
  a.Tref[q] = o.Tref; a.Qref[q] = o.Qref; a.delt[q] = o.delt; a.delq[q] = o.delq;
  a.lhcoef[q] = o.lhcoef; a.shcoef[q] = o.shcoef;
}

// every category of every block; blockIdx.y = b * ncat + n
__global__ __launch_bounds__(256) void k_atmo_dense(AtmoArgs a) {
  const size_t np = (size_t)a.nx * a.ny;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= np) return;
  const int bn = blockIdx.y, b = bn / a.ncat;
  const int i = (int)(q % a.nx) + 1, j = (int)(q / a.nx) + 1;
  const int32_t* bl = a.blk + 4 * b;
  const size_t c = (size_t)bn * np + q, f = (size_t)b * np + q;
  const bool in = i >= bl[0] && i <= bl[1] && j >= bl[2] && j <= bl[3] && a.aicen[c] > K::puny;
  AtmoOut o{};
  if (in)
    o = atmo_cell(a.p, 0, a.Tsf[((size_t)bn * NTRCR + a.it_Tsfc) * np + q], a.potT[f], a.uatm[f], a.vatm[f],
                  a.wind[f], a.zlvl[f], a.Qa[f], a.rhoa[f]);
  if (a.calc_strair) { a.strx[c] = o.strx; a.stry[c] = o.stry; }
  else { a.strx[c] = a.strax[f]; a.stry[c] = a.stray[f]; }
  a.Tref[c] = o.Tref; a.Qref[c] = o.Qref; a.lhcoef[c] = o.lhcoef; a.shcoef[c] = o.shcoef;
  if (a.delt) a.delt[c] = o.delt;
  if (a.delq) a.delq[c] = o.delq;
}

}  // namespace

void atmo_launch_list(const AtmoArgs& a, hipStream_t s) {
  const size_t np = (size_t)a.nx * a.ny;
  k_atmo_zero<<<dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s>>>(a);
  if (a.icells > 0) k_atmo_list<<<dim3((unsigned)((a.icells + 255) / 256)), dim3(256), 0, s>>>(a);
  CICE_HIP(hipGetLastError());
}

void atmo_launch_dense(const AtmoArgs& a, hipStream_t s) {
  const size_t np = (size_t)a.nx * a.ny;
  k_atmo_dense<<<dim3((unsigned)((np + 255) / 256), (unsigned)(a.ncat * a.nblocks)), dim3(256), 0, s>>>(a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
