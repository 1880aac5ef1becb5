// The state's way from the transport into the column batch on the device (cice_ridge_chain): Transport keeps every array
// level-major, (nx, ny, nblocks) per level, the layout the halo lists address; the batch keeps a block's levels together,
// (nx, ny, levels, nblocks), the host layout.  One launch copies the seven state arrays from the one into the other.
#pragma once
#include "common.h"

namespace cice {

enum { HO_ARRAYS = 7 };   // aice0, aicen, vicen, vsnon, eicen, esnon, trcrn

// The array table of k_state_from_transport.  Array k owns the planes first[k] .. first[k + 1] - 1 of the launch; of every
// `stride` consecutive levels of a block the first `use` move (trcrn: ntrcr of max_ntrcr per category; the others: all).
struct HandoverArgs {
  int np, nb;                      // cells of a block's plane (nx * ny), blocks
  int first[HO_ARRAYS + 1];
  int use[HO_ARRAYS], stride[HO_ARRAYS], levels[HO_ARRAYS];   // levels: of a block in the destination
  const double* src[HO_ARRAYS];    // (np, nb) per level
  double* dst[HO_ARRAYS];          // (np, levels, nb)
};

// the table for a transport of `ntrcr` tracers; src / dst in the order aice0, aicen, vicen, vsnon, eicen, esnon, trcrn
HandoverArgs handover_args(int nx, int ny, int nb, int ntrcr, const double* const src[HO_ARRAYS], double* const dst[HO_ARRAYS]);
void handover_launch(const HandoverArgs& a, hipStream_t s);

}  // namespace cice
