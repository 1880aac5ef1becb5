// The blocks of a one-task domain joined into ONE full-width image for the K-subcycle sweep (Evp: can_join, in_image).
//
// The sweep kernel (k_subcycle_skew) wants one full-width block per task.  Where the blocks of a task tile the whole grid,
// the subcycle loop runs it on an image of (nxg + 2) x (nyg + 2) cells -- one pseudo-block, ilo = jlo = 2 -- and the
// blocks get the result back.  Physical cells map one to one; the image's outer ring is taken from the ghost cells of the
// edge blocks as they lie (beyond an open or closed edge: what the caller uploaded; along a cyclic east-west edge: the
// wrap, which prepare() and every subcycle keep current), so the image holds what a one-block domain of the same grid
// would hold.  Padded last blocks contribute their physical cells only.
//
// Under a tripole fold (join_geometry(.., allow_fold); Evp option "skew_join_fold") the image is the same, but the top ghost
// row of the top block row -- written by the fold, with a sign, from no copy source -- keeps its own place on the image's
// top ring, as beyond an open edge.  The fold itself is carried by a band of top rows that runs on the BLOCKS beside each
// sweep (evp.hip: launch_subcycle_join_fold); k_band_from_image / k_band_to_image move those rows between the two.
//
// Geometry and the cell maps are host code without a device (join_geometry; cice_debug_join_map for the CPU tests); the
// kernels are gathers / scatters of whole planes, one thread per cell, lanes along i.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"
#include "domain.h"

namespace cice {

struct JoinGeom {
  bool ok = false;
  int nx = 0, ny = 0;          // the image: nxg + 2, nyg + 2
  size_t n = 0, nblk = 0;      // cells of the image / of the block arrays (nblocks * ny_block * nx_block)
  // per cell of the block arrays:
  std::vector<int32_t> map;    // image cell that holds this cell's value: physical cells their own; a ghost cell with an on-rank
                               // source that of its source; a ghost cell beyond an open / closed edge its place on the ring; -1: padding
  std::vector<int32_t> tnat;   // T-cells a subcycle kernel of the block computes (ilo .. ihi+1, jlo .. jhi+1): their place in the image, else -1
  std::vector<int32_t> usrc;   // U-cells a subcycle leaves a velocity in: the block cell that owns it (itself; a ghost cell's source), else -1
  // per cell of the image: the block cell it is gathered from
  std::vector<int32_t> inv;
  // a tripole fold on top: the blocks of the top block row, which hold the band (they share jlo / jhi and lie one after
  // another in the block arrays)
  bool fold = false;
  int nxb = 0, nyb = 0;        // cells of a block's rows / columns (nx_block, ny_block)
  int top_nb = 0, top_jhi = 0; // blocks of the top block row; their jhi (1-based, local)
  size_t top_first = 0;        // first cell of the first of them in the block arrays
};

// Does the domain qualify (one rank that owns every block of the grid, more than one block, no overlap rows, north-south
// open or closed -- or, with allow_fold, a tripole fold), and if so, its image and maps.
bool join_geometry(const Domain& d, JoinGeom& g, bool allow_fold = false);

// host-only test aid (cice_debug_join_map): cells of the block arrays (0: the layout does not qualify, -2: bad arguments)
// fold != 0: the geometry that admits a tripole fold (cice_debug_join_map_fold)
long long join_map_debug(int nxg, int nyg, int bsx, int bsy, int ew, int ns, int32_t* map, long long cap, int fold = 0);

// Device side: maps, the image's copies of what the sweep reads and writes, and the launches.
struct JoinImage {
  JoinGeom g;
  DevBuf<int32_t> inv, tnat, umap, usrc, blk, msk;
  DevBuf<double> st[2];        // the state, 14 planes each: pairs {u, v} {s1, s2} .. or planes, as the sweeps of the range want it
  DevBuf<double> uar4, hnhe, HTN, HTE, tarear, strength;
  DevBuf<double> out;          // what the sweep that ends evp(dt) leaves: divu, rdg_conv, rdg_shear, shear, prs_sig, strintx, strinty, strocnx, strocny
  bool grid_done = false;
  void init(const Domain& d, hipStream_t s);                       // geometry; uploads the maps if the domain qualifies
  bool allocated() const { return st[0].p != nullptr; }
  void alloc();                                                    // (outside any capture)
  void pack_grid(hipStream_t s, const double* HTN_b, const double* HTE_b, const double* tarear_b);
  void pack_inputs(hipStream_t s, const double* uarena_b, const int32_t* tmk_b, const int32_t* umk_b, const double* strength_b);
  void join_state(hipStream_t s, const double* st_b, int cur, bool pairs);
  // the image's copy `cur` back into the blocks' (st_b: 14 planes of g.nblk): stresses where the block's kernels would have
  // written them (icetmask == 1), u and v where a U-cell with ice owns them, ghost copies included
  void split_state(hipStream_t s, double* st_b, int cur, bool pairs, const int32_t* tmk_b, const int32_t* umk_b);
  // row_end: cells of image rows from row_end up keep what they hold (a band on the blocks has written them); -1: every row
  void split_out(hipStream_t s, double* const out_b[9], const int32_t* tmk_b, const int32_t* umk_b, int row_end = -1);
  // ---- the band of top rows under a fold (g.fold): block geometry, the top block row only ----
  bool band_fits(int K) const { return g.fold && g.top_jhi - 1 >= 2 * K + 1 && g.ny - 2 >= 4 * K + 4; }   // rows nyg-2K .. nyg lie in the top block row
  // global rows nyg-2K-1 .. nyg+1 of the image's copy `cur` into both band copies (14 planes of g.nblk), ghost cells included
  void band_gather(hipStream_t s, int K, int cur, bool pairs, double* band0, double* band1);
  // global rows nyg-K+1 .. nyg+1 of a band copy into the image's copy `cur`
  void band_scatter(hipStream_t s, int K, int cur, bool pairs, const double* band);
  // u, v of the top physical row and the ghost row above it -- what the fold writes, with or without ice -- into the blocks' state
  void band_top_rows(hipStream_t s, const double* band, double* st_b);
};

}  // namespace cice
