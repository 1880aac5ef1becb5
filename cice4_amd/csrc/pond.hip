// k_pond_age (pond.h).
#include "pond.h"

#include "pond_cell.h"

namespace cice {

namespace {

__device__ inline bool physical(const int32_t* blk, int b, int q, int nx) {
  const int i = q % nx + 1, j = q / nx + 1;
  const int32_t* w = blk + 4 * b;
  return i >= w[0] && i <= w[1] && j >= w[2] && j <= w[3];
}

// Grid (chunks of 256 cells of a plane, categories, blocks), as k_shortwave_ccsm3: a wavefront takes 64 consecutive cells
// of one (category, block), 512 contiguous bytes per array and access.  Nine words in and four out per listed column at the
// most; a thread off the list returns without a store.
__global__ __launch_bounds__(256) void k_pond_age(const PondArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int n = (int)blockIdx.y, b = (int)blockIdx.z;
  const size_t np = (size_t)a.np;
  const size_t cb = (size_t)b * a.ncat + n;          // (category, block)
  const size_t c = cb * np + q;
  PondIn in{};
  if (a.listed) {                                    // increment_age on the caller's list
    if (a.listed[q] == 0) return;
  } else {
    if (!physical(a.blk, b, q, a.nx)) return;
    in.aicen = a.aicen[c];
    if (!(in.aicen > pondk::puny)) return;
  }
  const size_t cv = cb * a.volpn_planes * np + q, ca = cb * a.iage_planes * np + q;
  if (a.ponds) {
    in.vicen = a.vicen[c]; in.vsnon = a.vsnon[c];
    in.Tsfc = a.Tsfc[cb * a.tsfc_planes * np + q];
    in.meltt = a.meltt[c]; in.melts = a.melts[c];
    in.frain = a.frain[(size_t)b * np + q];
    in.volpn = a.volpn[cv];
  }
  if (a.age) in.iage = a.iage[ca];
  const PondOut o = pond_cell(a.ponds != 0, a.age != 0, a.dt, in);
  const int st = o.st;
  if (st & POND_ST_FRAC) {
    a.apondn[c] = o.apondn;
    a.hpondn[c] = o.hpondn;
  }
  if (st & POND_ST_VOL) a.volpn[cv] = o.volpn;
  if (st & POND_ST_AGE) a.iage[ca] = o.iage;
}

}  // namespace

void pond_launch(const PondArgs& a, hipStream_t s) {
  CICE_REQUIRE(a.nx >= 1 && a.np >= a.nx && a.np % a.nx == 0 && a.ncat >= 1 && a.nb >= 1, "pond: bad dimensions");
  CICE_REQUIRE((long long)a.np < (1ll << 31) - 256 && a.ncat <= 65535 && a.nb <= 65535, "pond: bad dimensions");
  CICE_REQUIRE(a.ponds || a.age, "pond: nothing to run");
  CICE_REQUIRE(a.listed || (a.blk && a.aicen), "pond: no list");
  CICE_REQUIRE(!a.listed || (a.ncat == 1 && a.nb == 1 && !a.ponds), "pond: a list names the cells of one block and category of increment_age");
  CICE_REQUIRE(!a.ponds || (a.vicen && a.vsnon && a.Tsfc && a.meltt && a.melts && a.frain && a.volpn && a.apondn && a.hpondn &&
                            a.tsfc_planes >= 1 && a.volpn_planes >= 1), "pond: NULL buffer");
  CICE_REQUIRE(!a.age || (a.iage && a.iage_planes >= 1), "pond: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), (unsigned)a.ncat, (unsigned)a.nb);
  hipLaunchKernelGGL(k_pond_age, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
