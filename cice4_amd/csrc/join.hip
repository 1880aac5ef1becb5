// Sweeps on a joined image of a task's blocks: geometry, cell maps, and the kernels that move planes between the block
// arrays and the image (join.h).
#include "join.h"

#include <algorithm>

namespace cice {

// ---- geometry (host, no device) ----------------------------------------------------------------------------------------
bool join_geometry(const Domain& d, JoinGeom& g, bool allow_fold) {
  g = JoinGeom{};
  const int nb = d.nblocks();
  if (d.nranks != 1 || d.overlap != 0 || d.self_comm || !d.rsrc.empty() || !d.hfill.empty()) return false;
  if ((d.tripole() && !allow_fold) || d.ns == BND_CYCLIC) return false;   // (a fold over several blocks: only where asked for)
  if (d.tripole() && d.ew != BND_CYCLIC) return false;
  if (d.ew != BND_OPEN && d.ew != BND_CYCLIC && d.ew != BND_CLOSED) return false;
  if (nb < 2 || nb != d.nbx * d.nby || (int)d.all.size() != nb) return false;   // one block: nothing to join
  for (const Block& b : d.all)
    if (b.owner != d.rank) return false;                   // an eliminated land block
  const long long inx = (long long)d.nxg + 2, iny = (long long)d.nyg + 2;
  const size_t np = (size_t)d.nx_block * d.ny_block;
  if (inx * iny > 0x7fffffffLL || (long long)np * nb > 0x7fffffffLL) return false;
  g.nx = (int)inx;
  g.ny = (int)iny;
  g.n = (size_t)inx * iny;
  g.nblk = np * nb;
  g.map.assign(g.nblk, -1);
  g.tnat.assign(g.nblk, -1);
  g.usrc.assign(g.nblk, -1);
  g.inv.assign(g.n, -1);
  auto addr = [&](const Block& b, int i, int j) { return (size_t)b.local_id * np + (size_t)(j - 1) * d.nx_block + (size_t)(i - 1); };
  // the place of block cell (i, j) in the image, 0-based linear: column i - ilo + i0 + 1, row j - jlo + j0 + 1 (the image's
  // physical cells start at column / row 1, 0-based)
  auto nat = [&](const Block& b, int i, int j) {
    return (int32_t)((size_t)(j - b.jlo + b.j0 + 1) * g.nx + (size_t)(i - b.ilo + b.i0 + 1));
  };
  for (const Block& b : d.all) {
    for (int j = b.jlo - 1; j <= b.jhi + 1; ++j)
      for (int i = b.ilo - 1; i <= b.ihi + 1; ++i) {
        const size_t c = addr(b, i, j);
        const bool phys = i >= b.ilo && i <= b.ihi && j >= b.jlo && j <= b.jhi;
        g.map[c] = nat(b, i, j);             // (ghost cells with a source: below)
        if (phys) {
          g.usrc[c] = (int32_t)c;
          g.inv[(size_t)g.map[c]] = (int32_t)c;
        }
        if (i >= b.ilo && j >= b.jlo) g.tnat[c] = nat(b, i, j);
      }
  }
  // Under a fold the top ghost row of the top block row is written by the fold, from no copy source: its cells keep the
  // place on the image's top ring they were given above.  A copy into one of them would alias it to a physical cell.
  std::vector<char> fold_row;
  if (d.tripole()) {
    fold_row.assign(g.nblk, 0);
    const Block& t0 = d.all[(size_t)(d.nby - 1) * d.nbx];
    for (int ib = 0; ib < d.nbx; ++ib) {
      const Block& b = d.all[(size_t)(d.nby - 1) * d.nbx + ib];
      if (b.jlo != t0.jlo || b.jhi != t0.jhi || b.local_id != t0.local_id + ib) return false;
      for (int i = 1; i <= d.nx_block; ++i) fold_row[addr(b, i, b.jhi + 1)] = 1;
    }
    g.fold = true;
    g.nxb = d.nx_block;
    g.nyb = d.ny_block;
    g.top_nb = d.nbx;
    g.top_jhi = t0.jhi;
    g.top_first = (size_t)t0.local_id * np;
  }
  for (size_t e = 0; e < d.hsrc.size(); ++e) {
    const size_t s = (size_t)d.hsrc[e], c = (size_t)d.hdst[e];
    if (s >= g.nblk || c >= g.nblk || g.usrc[s] != (int32_t)s) return false;   // (sources are physical cells)
    if (g.fold && fold_row[c]) return false;
    g.map[c] = g.map[s];
    g.usrc[c] = (int32_t)s;
  }
  // the ring of the image: the ghost cells of the edge blocks as they lie
  for (int J = 0; J < g.ny; ++J)
    for (int I = 0; I < g.nx; ++I) {
      if (I >= 1 && I <= g.nx - 2 && J >= 1 && J <= g.ny - 2) continue;
      const int gi = std::min(std::max(I - 1, 0), d.nxg - 1), gj = std::min(std::max(J - 1, 0), d.nyg - 1);
      const Block& b = d.all[(size_t)(gj / d.bsy) * d.nbx + (size_t)(gi / d.bsx)];
      g.inv[(size_t)J * g.nx + I] = (int32_t)addr(b, b.ilo + (I - 1 - b.i0), b.jlo + (J - 1 - b.j0));
    }
  for (size_t q = 0; q < g.n; ++q)
    if (g.inv[q] < 0 || (size_t)g.inv[q] >= g.nblk) return false;               // (every cell of the image has a source)
  for (size_t c = 0; c < g.nblk; ++c)
    if (g.map[c] >= (int32_t)g.n || g.tnat[c] >= (int32_t)g.n) return false;
  g.ok = true;
  return true;
}

long long join_map_debug(int nxg, int nyg, int bsx, int bsy, int ew, int ns, int32_t* map, long long cap, int fold) {
  if (nxg < 1 || nyg < 1 || bsx < 1 || bsy < 1 || cap < 0 || (cap > 0 && !map)) return -2;
  Domain d;
  const char* msg = d.create(nxg, nyg, bsx, bsy, ew, ns, 0, 1, 1);
  if (msg && msg[0]) return -2;
  JoinGeom g;
  if (!join_geometry(d, g, fold != 0)) return 0;
  for (long long c = 0; c < std::min<long long>(cap, (long long)g.nblk); ++c) map[c] = g.map[(size_t)c];
  return (long long)g.nblk;
}

// ---- kernels: one thread per cell, lanes along i ------------------------------------------------------------------------
namespace {

struct alignas(16) jdbl2 { double x, y; };

// the 14 planes of the blocks' state gathered into both copies of the image; PAIRS: as 7 planes of pairs (k_subcycle_skew's
// own layout, 16-byte stores), so that no second pass converts them
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_join_state(size_t ni, size_t nb, const int32_t* __restrict__ inv,
                                                    const double* __restrict__ in, double* __restrict__ out0,
                                                    double* __restrict__ out1) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ni) return;
  const size_t s = (size_t)inv[q];
#pragma unroll
  for (int p = 0; p < 7; ++p) {
    jdbl2 t;
    t.x = in[(size_t)(2 * p) * nb + s];
    t.y = in[(size_t)(2 * p + 1) * nb + s];
    if (PAIRS) {
      *(jdbl2*)(out0 + 2 * ((size_t)p * ni + q)) = t;
      *(jdbl2*)(out1 + 2 * ((size_t)p * ni + q)) = t;
    } else {
      out0[(size_t)(2 * p) * ni + q] = t.x;
      out0[(size_t)(2 * p + 1) * ni + q] = t.y;
      out1[(size_t)(2 * p) * ni + q] = t.x;
      out1[(size_t)(2 * p + 1) * ni + q] = t.y;
    }
  }
}

// what k_skew_pack produces, in image geometry, and the strength
__global__ __launch_bounds__(256) void k_join_inputs(size_t ni, size_t nb, const int32_t* __restrict__ inv,
                                                     const double* __restrict__ uar, const int32_t* __restrict__ tmk,
                                                     const int32_t* __restrict__ umk, const double* __restrict__ strength,
                                                     double* __restrict__ uar4, int32_t* __restrict__ msk,
                                                     double* __restrict__ strength_i) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ni) return;
  const size_t s = (size_t)inv[q];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    jdbl2 t;
    t.x = uar[(size_t)(2 * p) * nb + s];
    t.y = uar[(size_t)(2 * p + 1) * nb + s];
    *(jdbl2*)(uar4 + 2 * ((size_t)p * ni + q)) = t;
  }
  msk[q] = (tmk[s] == 1 ? 1 : 0) | (umk[s] != 0 ? 2 : 0);
  strength_i[q] = strength[s];
}

// ... and what k_skew_pack_grid produces, with the planes the sweep reads singly
__global__ __launch_bounds__(256) void k_join_grid(size_t ni, const int32_t* __restrict__ inv, const double* __restrict__ HTN,
                                                   const double* __restrict__ HTE, const double* __restrict__ tarear,
                                                   double* __restrict__ hnhe, double* __restrict__ HTN_i,
                                                   double* __restrict__ HTE_i, double* __restrict__ tarear_i) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ni) return;
  const size_t s = (size_t)inv[q];
  jdbl2 t;
  t.x = HTN[s];
  t.y = HTE[s];
  *(jdbl2*)(hnhe + 2 * q) = t;
  HTN_i[q] = t.x;
  HTE_i[q] = t.y;
  tarear_i[q] = tarear[s];
}

// The image back into the blocks: exactly the cells one launch per subcycle on the blocks would have written -- the
// stresses of the T-cells a block computes (its own and the ghost column / row east and north of them) where there is
// ice, u and v of the U-cells with ice and of the ghost cells that mirror them on this rank.  Everything else keeps what
// it holds (no subcycle kernel ever writes it, so either copy of the blocks' state holds the same value there).
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_split_state(size_t nb, size_t ni, const int32_t* __restrict__ tnat,
                                                     const int32_t* __restrict__ umap, const int32_t* __restrict__ usrc,
                                                     const int32_t* __restrict__ tmk, const int32_t* __restrict__ umk,
                                                     const double* __restrict__ in, double* __restrict__ out) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb) return;
  const int32_t s = usrc[c];
  if (s >= 0 && umk[s] != 0) {
    const size_t q = (size_t)umap[c];
    if (PAIRS) {
      const jdbl2 t = *(const jdbl2*)(in + 2 * q);
      out[c] = t.x;
      out[nb + c] = t.y;
    } else {
      out[c] = in[q];
      out[nb + c] = in[ni + q];
    }
  }
  const int32_t t0 = tnat[c];
  if (t0 >= 0 && tmk[c] == 1) {
    const size_t q = (size_t)t0;
#pragma unroll
    for (int p = 1; p < 7; ++p) {
      jdbl2 t;
      if (PAIRS) {
        t = *(const jdbl2*)(in + 2 * ((size_t)p * ni + q));
      } else {
        t.x = in[(size_t)(2 * p) * ni + q];
        t.y = in[(size_t)(2 * p + 1) * ni + q];
      }
      out[(size_t)(2 * p) * nb + c] = t.x;
      out[(size_t)(2 * p + 1) * nb + c] = t.y;
    }
  }
}

struct OutPtrs { double* p[9]; };

// what the sweep that ends evp(dt) leaves beside the state: five T-cell diagnostics, four U-cell stresses (physical U-cells)
__global__ __launch_bounds__(256) void k_split_out(size_t nb, size_t ni, const int32_t* __restrict__ tnat,
                                                   const int32_t* __restrict__ umap, const int32_t* __restrict__ usrc,
                                                   const int32_t* __restrict__ tmk, const int32_t* __restrict__ umk,
                                                   const double* __restrict__ in, const OutPtrs o, int32_t q_end) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb) return;
  const int32_t t0 = tnat[c];
  if (t0 >= 0 && t0 < q_end && tmk[c] == 1) {
#pragma unroll
    for (int p = 0; p < 5; ++p) o.p[p][c] = in[(size_t)p * ni + (size_t)t0];
  }
  if (usrc[c] == (int32_t)c && umk[c] != 0 && umap[c] < q_end) {
    const size_t q = (size_t)umap[c];
#pragma unroll
    for (int p = 5; p < 9; ++p) o.p[p][c] = in[(size_t)p * ni + q];
  }
}

// ---- the band of top rows under a fold: block geometry <-> image ----
// The rows of the top block row's blocks from local row j0 (0-based) on, `rows` of them, every column: from the image
// (through map: a ghost cell reads its source's image cell, the top ghost row its place on the ring) into both band copies.
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_band_from_image(size_t cells, int nxb, int rows, int j0, size_t first, size_t np, size_t nb,
                                                         size_t ni, const int32_t* __restrict__ map,
                                                         const double* __restrict__ in, double* __restrict__ out0,
                                                         double* __restrict__ out1) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const size_t per = (size_t)rows * nxb, b = t / per, rem = t - b * per;
  const size_t c = first + b * np + (size_t)j0 * nxb + rem;
  const int32_t m = map[c];
  if (m < 0) return;                     // padding of a last block
  const size_t q = (size_t)m;
#pragma unroll
  for (int p = 0; p < 7; ++p) {
    jdbl2 v;
    if (PAIRS) {
      v = *(const jdbl2*)(in + 2 * ((size_t)p * ni + q));
    } else {
      v.x = in[(size_t)(2 * p) * ni + q];
      v.y = in[(size_t)(2 * p + 1) * ni + q];
    }
    out0[(size_t)(2 * p) * nb + c] = v.x;
    out0[(size_t)(2 * p + 1) * nb + c] = v.y;
    out1[(size_t)(2 * p) * nb + c] = v.x;
    out1[(size_t)(2 * p + 1) * nb + c] = v.y;
  }
}

// `cells` cells of the image from cell q0 on (whole rows, ring included) take the band's values
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_band_to_image(size_t cells, size_t q0, size_t nb, size_t ni, const int32_t* __restrict__ inv,
                                                       const double* __restrict__ in, double* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const size_t q = q0 + t, s = (size_t)inv[q];
#pragma unroll
  for (int p = 0; p < 7; ++p) {
    jdbl2 v;
    v.x = in[(size_t)(2 * p) * nb + s];
    v.y = in[(size_t)(2 * p + 1) * nb + s];
    if (PAIRS) {
      *(jdbl2*)(out + 2 * ((size_t)p * ni + q)) = v;
    } else {
      out[(size_t)(2 * p) * ni + q] = v.x;
      out[(size_t)(2 * p + 1) * ni + q] = v.y;
    }
  }
}

// u | v of two rows of the top block row's blocks (the top physical row and the ghost row above it), every mapped column
__global__ __launch_bounds__(256) void k_band_top_rows(size_t cells, int nxb, int j0, size_t first, size_t np, size_t nb,
                                                       const int32_t* __restrict__ map, const double* __restrict__ in,
                                                       double* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const size_t per = (size_t)2 * nxb, b = t / per, rem = t - b * per;
  const size_t c = first + b * np + (size_t)j0 * nxb + rem;
  if (map[c] < 0) return;
  out[c] = in[c];
  out[nb + c] = in[nb + c];
}

inline dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

// ---- device side --------------------------------------------------------------------------------------------------------
void JoinImage::init(const Domain& d, hipStream_t s) {
  grid_done = false;
  if (!join_geometry(d, g, /*allow_fold=*/true)) return;   // (whether a fold is swept on the image: Evp::can_join)
  inv.alloc(g.n);
  inv.upload(g.inv.data(), s);
  tnat.alloc(g.nblk);
  tnat.upload(g.tnat.data(), s);
  umap.alloc(g.nblk);
  umap.upload(g.map.data(), s);
  usrc.alloc(g.nblk);
  usrc.upload(g.usrc.data(), s);
  const int32_t hb[6] = {2, g.nx - 1, 2, g.ny - 1, 2, g.ny - 1};   // the image as one block: ilo, ihi, jlo, jhi, own_jlo, own_jhi
  blk.alloc(6);
  CICE_HIP(hipMemcpyAsync(blk.p, hb, sizeof(hb), hipMemcpyHostToDevice, s));
  CICE_HIP(hipStreamSynchronize(s));       // (hb and the vectors are read by the copies)
}

void JoinImage::alloc() {
  if (allocated()) return;
  for (int k = 0; k < 2; ++k) st[k].alloc(14 * g.n);
  uar4.alloc(8 * g.n);
  hnhe.alloc(2 * g.n);
  HTN.alloc(g.n);
  HTE.alloc(g.n);
  tarear.alloc(g.n);
  strength.alloc(g.n);
  msk.alloc(g.n);
  out.alloc(9 * g.n);
  grid_done = false;
}

void JoinImage::pack_grid(hipStream_t s, const double* HTN_b, const double* HTE_b, const double* tarear_b) {
  hipLaunchKernelGGL(k_join_grid, grid_of(g.n), dim3(256), 0, s, g.n, (const int32_t*)inv.p, HTN_b, HTE_b, tarear_b, hnhe.p,
                     HTN.p, HTE.p, tarear.p);
  grid_done = true;
}

void JoinImage::pack_inputs(hipStream_t s, const double* uarena_b, const int32_t* tmk_b, const int32_t* umk_b,
                            const double* strength_b) {
  hipLaunchKernelGGL(k_join_inputs, grid_of(g.n), dim3(256), 0, s, g.n, g.nblk, (const int32_t*)inv.p, uarena_b, tmk_b, umk_b,
                     strength_b, uar4.p, msk.p, strength.p);
}

void JoinImage::join_state(hipStream_t s, const double* st_b, int cur, bool pairs) {
  if (pairs)
    hipLaunchKernelGGL(k_join_state<true>, grid_of(g.n), dim3(256), 0, s, g.n, g.nblk, (const int32_t*)inv.p, st_b, st[cur].p,
                       st[1 - cur].p);
  else
    hipLaunchKernelGGL(k_join_state<false>, grid_of(g.n), dim3(256), 0, s, g.n, g.nblk, (const int32_t*)inv.p, st_b, st[cur].p,
                       st[1 - cur].p);
}

void JoinImage::split_state(hipStream_t s, double* st_b, int cur, bool pairs, const int32_t* tmk_b, const int32_t* umk_b) {
  if (pairs)
    hipLaunchKernelGGL(k_split_state<true>, grid_of(g.nblk), dim3(256), 0, s, g.nblk, g.n, (const int32_t*)tnat.p,
                       (const int32_t*)umap.p, (const int32_t*)usrc.p, tmk_b, umk_b, (const double*)st[cur].p, st_b);
  else
    hipLaunchKernelGGL(k_split_state<false>, grid_of(g.nblk), dim3(256), 0, s, g.nblk, g.n, (const int32_t*)tnat.p,
                       (const int32_t*)umap.p, (const int32_t*)usrc.p, tmk_b, umk_b, (const double*)st[cur].p, st_b);
}

void JoinImage::split_out(hipStream_t s, double* const out_b[9], const int32_t* tmk_b, const int32_t* umk_b, int row_end) {
  const int32_t q_end = row_end < 0 || row_end > g.ny ? (int32_t)g.n : (int32_t)((size_t)row_end * g.nx);
  OutPtrs o;
  for (int p = 0; p < 9; ++p) o.p[p] = out_b[p];
  hipLaunchKernelGGL(k_split_out, grid_of(g.nblk), dim3(256), 0, s, g.nblk, g.n, (const int32_t*)tnat.p, (const int32_t*)umap.p,
                     (const int32_t*)usrc.p, tmk_b, umk_b, (const double*)out.p, o, q_end);
}

// (the image's row of global row r, 1-based, is r; a block's 0-based row of its local row j is j - 1)
void JoinImage::band_gather(hipStream_t s, int K, int cur, bool pairs, double* band0, double* band1) {
  const int rows = 2 * K + 3, j0 = g.top_jhi - 2 * K - 2;   // local rows jhi-2K-1 .. jhi+1
  const size_t cells = (size_t)g.top_nb * rows * g.nxb, np = (size_t)g.nxb * g.nyb;
  if (pairs)
    hipLaunchKernelGGL(k_band_from_image<true>, grid_of(cells), dim3(256), 0, s, cells, g.nxb, rows, j0, g.top_first, np, g.nblk, g.n,
                       (const int32_t*)umap.p, (const double*)st[cur].p, band0, band1);
  else
    hipLaunchKernelGGL(k_band_from_image<false>, grid_of(cells), dim3(256), 0, s, cells, g.nxb, rows, j0, g.top_first, np, g.nblk, g.n,
                       (const int32_t*)umap.p, (const double*)st[cur].p, band0, band1);
}

void JoinImage::band_scatter(hipStream_t s, int K, int cur, bool pairs, const double* band) {
  const size_t cells = (size_t)(K + 1) * g.nx, q0 = (size_t)(g.ny - 1 - K) * g.nx;   // image rows nyg-K+1 .. nyg+1
  if (pairs)
    hipLaunchKernelGGL(k_band_to_image<true>, grid_of(cells), dim3(256), 0, s, cells, q0, g.nblk, g.n, (const int32_t*)inv.p, band,
                       st[cur].p);
  else
    hipLaunchKernelGGL(k_band_to_image<false>, grid_of(cells), dim3(256), 0, s, cells, q0, g.nblk, g.n, (const int32_t*)inv.p, band,
                       st[cur].p);
}

void JoinImage::band_top_rows(hipStream_t s, const double* band, double* st_b) {
  const size_t cells = (size_t)g.top_nb * 2 * g.nxb, np = (size_t)g.nxb * g.nyb;
  hipLaunchKernelGGL(k_band_top_rows, grid_of(cells), dim3(256), 0, s, cells, g.nxb, g.top_jhi - 1, g.top_first, np, g.nblk,
                     (const int32_t*)umap.p, band, st_b);
}

}  // namespace cice
