// Thermodynamic changes of the thickness distribution on the device: module ice_therm_itd (source/ice_therm_itd.F90:
// linear_itd :58, add_new_ice :843, lateral_melt :1266) with aggregate_area and shift_ice of source/ice_itd.F90
// (:494, :892).  The first half of step_therm2 (source/ice_step_mod.F90:286-422).
//
// One thread per cell, the category loop inside the thread; every field is addressed as the reference's planes
// (consecutive lanes = consecutive i).  The reference's cell lists are predicates per thread: either evaluated from
// the fields (the one-call stage) or given as a plane of 1-based list positions (the block-wise entries, whose
// callers hand in indxi / indxj).  Arithmetic: the reference's operations in its order, fp64, no contraction.
//
// STOPS.  Nothing in a kernel waits for another thread, but shift_ice stops ALL cells at the first boundary at which
// ANY cell fails its range check (ice_itd.F90:1043-1187).  So a launch runs as if no cell failed; a thread that does
// fail records (block, boundary) with one atomicMax and gives up.  Only then -- the model is about to abort -- the host
// restores the inputs and launches again with that block and boundary as a limit: the failing block stops in front of
// the boundary's transfer, as the reference does, and every thread of it evaluates the reference's four message
// conditions there (one atomicMax per matching kind), from which the host takes the cell: first kind in the order
// negative daice, negative dvice, daice > aicen, dvice > vicen; the LAST cell in list order (istop, jstop are
// overwritten).  Blocks in front of the failing one complete, blocks behind it are not touched.
//
// UNPINNED: the two "negative" message loops (:1101-1141) test against aicen / vicen of category `nd`, which is stale
// there: left over from the last cell of the list with donor > 0 in the preceding loop.  The rule is reproduced as
// written (the record holds the matches for both possible values of that category and the donor of the last such
// cell), but no fixture pins it; only the daice > aicen kind is pinned (tests/golden/therm_itd.npz, stop_shift).
// Where the stale category makes NO cell match a kind whose flag was raised, the reference would carry on; the
// library stops and names the last cell that raised the flag.
#pragma once
#include "common.h"

namespace cice {

struct ItdParams {   // cice_itd_config; tracer slots 0-based here, -1 = absent
  int ntrcr;
  int dep[NTRCR];
  int it_Tsfc, it_iage, it_alvl, it_vlvl;
  int tr_iage, tr_lvl, update_ocn_f;
  double hin_max[NCAT + 1];   // hin_max(ncat) as init_itd left it; linear_itd uses 999.9 (ice_therm_itd.F90:219)
  double hi_min;
};

// record words of a launch (unsigned long long each)
enum {
  ITD_REC_SHIFT = 0,     // atomicMax of ((nblocks-1-b) << 8 | (ncat - n)) + 1: first block, in it first boundary
  ITD_REC_NOREMAP = 1,   // cells of linear_itd whose remap_flag went false
  ITD_REC_NEG_DA = 2,    // [2], [3]: limited launch: last cell matching "negative daice" with stale nd = n, n + 1
  ITD_REC_NEG_DV = 4,    // [4], [5]: the same for dvice
  ITD_REC_GT_DA = 6,     // last cell with daice >= aicen(nd) (1 + puny)
  ITD_REC_GT_DV = 7,
  ITD_REC_LASTDONOR = 8, // last cell with donor > 0 at the boundary: key << 3 | donor
  ITD_REC_FLAG = 9,      // [9..12]: last cell that raised the flag of kind 0..3
  ITD_REC_ADD = 13,      // add_new_ice conservation: atomicMax of (nblocks-1-b) << 32 | key
  ITD_REC_WORDS = 16
};

struct ItdArgs {
  ItdParams p;
  int nx, ny, nblocks;
  const int32_t* blk;        // ilo, ihi, jlo, jhi per block (1-based)
  const int32_t* listpos;    // 1-based list position per cell, 0 = not listed; nullptr: the predicate of the stage
  const int32_t* blockflag;  // stage: != 0 where a block has a cell with aice > puny (`if (icells > 0)`); may be nullptr
  int32_t* blockflag_out;    // k_itd_rain_aggregate writes it
  int icells;                // block-wise shift_ice: leading dimension of hicen / donor / daice / dvice
  int kitd;
  int bfail, nlimit;         // limited launch: blocks > bfail are skipped, block bfail stops at boundary nlimit (1-based;
                             // 0: no limit).  bfail = nblocks: an ordinary launch
  int bend;                  // add_new_ice / lateral_melt: blocks >= bend are skipped
  double dt, yday;
  double *aicen, *trcrn, *vicen, *vsnon, *eicen, *esnon;
  const double *aicen_init, *vicen_init;
  double *aice, *aice0;
  const double *frain, *frzmlt, *Tf, *rside;
  const int32_t* tmask;
  double *frazil, *frz_onset, *fresh, *fsalt, *fhocn, *meltl;
  double *hicen, *daice, *dvice;   // block-wise shift_ice, (icells, ncat)
  const int32_t* donor;
  unsigned long long* rec;
};

void itd_launch_rain_aggregate(const ItdArgs& a, hipStream_t s);   // ice_step_mod.F90:290-310
void itd_launch_linear(const ItdArgs& a, hipStream_t s);
void itd_launch_shift(const ItdArgs& a, hipStream_t s);
void itd_launch_add_new_ice(const ItdArgs& a, hipStream_t s);
void itd_launch_lateral_melt(const ItdArgs& a, hipStream_t s);

}  // namespace cice
