// k_state_from_transport: the transport's device state (level-major) into the column batch (a block's levels together).
#include "handover.h"

namespace cice {

namespace {

// Grid (chunks of 256 cells of a plane, moved planes, blocks).  A plane of nx * ny cells is contiguous in both layouts, so
// a wavefront takes 64 consecutive cells of one plane of one (array, level, block): 512 contiguous bytes in, 512 out, one
// 8-byte load and store per lane.  Which array a plane belongs to is the same for the whole workgroup (scalar work).
__global__ __launch_bounds__(256) void k_state_from_transport(const HandoverArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int p = (int)blockIdx.y, b = (int)blockIdx.z;
  int k = 0;
#pragma unroll
  for (int m = 1; m < HO_ARRAYS; ++m)
    if (p >= a.first[m]) k = m;
  const int l = p - a.first[k];
  const int level = l / a.use[k] * a.stride[k] + l % a.use[k];
  const size_t np = (size_t)a.np;
  const double v = a.src[k][((size_t)level * a.nb + b) * np + q];
  a.dst[k][((size_t)b * a.levels[k] + level) * np + q] = v;
}

}  // namespace

HandoverArgs handover_args(int nx, int ny, int nb, int ntrcr, const double* const src[HO_ARRAYS], double* const dst[HO_ARRAYS]) {
  CICE_REQUIRE(nx >= 1 && ny >= 1 && nb >= 1 && ntrcr >= 1 && ntrcr <= NTRCR, "state hand-over: bad dimensions");
  CICE_REQUIRE((long long)nx * ny < (1ll << 31) - 256, "state hand-over: block too large");
  HandoverArgs a{};
  a.np = nx * ny; a.nb = nb;
  const int levels[HO_ARRAYS] = {1, NCAT, NCAT, NCAT, NCAT * NILYR, NCAT * NSLYR, NCAT * NTRCR};
  for (int k = 0; k < HO_ARRAYS; ++k) {
    CICE_REQUIRE(src[k] && dst[k], "state hand-over: NULL buffer");
    const bool tracers = k == HO_ARRAYS - 1;
    a.levels[k] = levels[k];
    a.use[k] = tracers ? ntrcr : levels[k];
    a.stride[k] = tracers ? NTRCR : levels[k];
    a.first[k + 1] = a.first[k] + (tracers ? NCAT * ntrcr : levels[k]);
    a.src[k] = src[k]; a.dst[k] = dst[k];
  }
  return a;
}

void handover_launch(const HandoverArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.np + 255) / 256), (unsigned)a.first[HO_ARRAYS], (unsigned)a.nb);
  CICE_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "state hand-over: too many planes or blocks for one launch");
  hipLaunchKernelGGL(k_state_from_transport, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
