// compute_ponds (source/ice_meltpond.F90:88-229) and increment_age (source/ice_age.F90:87-123) on the device: the two calls
// of step_therm1's category loop (drivers/cice4/CICE_RunMod.F90:449-454, :550-559) as ONE kernel, k_pond_age, run as a
// stage of its own behind the column update.  That is legal: thermo_vertical neither reads nor writes the age tracer, and
// aicen is intent(in) there, so the list aicen > puny on ilo..ihi, jlo..jhi is the same before and after.
//
// The cell arithmetic is pond_cell.h; every output word is meant to carry the compiled reference's bits.
#pragma once
#include "common.h"

namespace cice {

// One launch over (cells of a plane, categories, blocks).  np = nx * ny.  Per-category arrays (np, ncat, nb); frain (np, nb).
// Tsfc, volpn, iage are planes of tracer arrays: the plane of (category, block) cb starts at cb * <name>_planes * np.
// The list of compute_ponds: aicen > puny on the physical cells of blk.  The list of increment_age: the same, or -- the
// block-wise entry, ncat = nb = 1 -- the cells where `listed` is not 0, whatever their aicen.
// A thread off its lists stores nothing: ghost cells and cells without ice keep what they held.
struct PondArgs {
  int nx, np, ncat, nb;
  int ponds, age;                      // what runs
  int tsfc_planes, volpn_planes, iage_planes;
  double dt;
  const int32_t* blk;
  const int32_t* listed;               // increment_age's explicit list, or NULL
  const double *aicen, *vicen, *vsnon, *Tsfc, *meltt, *melts, *frain;   // read with ponds only (aicen: also for age on blk)
  double *volpn, *apondn, *hpondn;     // ponds
  double* iage;                        // age
};
void pond_launch(const PondArgs& a, hipStream_t s);

}  // namespace cice
