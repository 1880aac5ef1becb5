// The second half of step_therm2 on the device (source/ice_step_mod.F90:445-511): cleanup_itd (source/ice_itd.F90:1600
// with rebin :557 and zap_small_areas :1844), aggregate (:279) and the tendencies daidtt / dvidtt.  bound_state between
// them is the context's Halo (batch.hip).
//
// One thread per cell, the category loop inside, the reference's planes, fp64, no contraction -- as in itd.h.
//
// THE BLOCK-WIDE FLAG.  rebin makes eight passes over category boundaries (up over 1..4, down over 4..1).  Its
// `shiftflag` is one flag per block and pass: when ANY listed cell of a block moves a category at a pass, shift_ice runs
// over ALL listed cells of that block (every tracer goes through trcrn*aicen and back: not the identity in the last
// bit) and compute_tracers zeroes the tracers of every cell that is NOT listed.  No thread waits for another: what a
// pass has to know about its block crosses a kernel boundary as a word in device memory.  Each pass is one launch; the
// launch in front of it (the head, or the pass before) evaluates "does this cell want pass p" on the state it leaves and
// raises the block's word CW_PASS + p - 1.  A block whose word is not raised only evaluates the next pass.
//
// STOPS are block-wide too and travel the same way (no second launch):
//   - area out of bounds (:1729-1753): the head raises CW_STOP_AREA with atomicMax of the cell: the LAST failing cell;
//     nothing but aice, aice0 has been written, every later launch leaves the block alone.
//   - shift_ice's range checks out of rebin: the donor gives exactly what it has, so the only check that can fail is
//     "negative dvice" (vicen(nd) < 0 under aicen(nd) > puny).  Whoever evaluates the need for pass p sees it on the same
//     state and raises the pass word to cell + 2 (atomicMax: the LAST such cell, as the message loop :1121-1141 names
//     it); the pass and everything behind it leave the block alone.  UNPINNED: no fixture.
//   - zap_small_areas, negative area (:1952-1959): a scan behind the last pass raises CW_ZAP with the FIRST category and
//     in it the FIRST cell; the zap kernel then zaps the categories in front of it only and adds no fluxes.
//   - zap_small_areas, excess area (:2057-2064): dead with limit_aice (the head has stopped at the same condition on the
//     same aice), and zap_small_areas does not run without it.
#pragma once
#include "itd.h"

namespace cice {

enum { CW_STOP_AREA = 0, CW_ZAP = 1, CW_PASS = 2, CW_WORDS = 10 };   // words of a block; CW_PASS + p - 1, p = 1..8

struct CleanArgs {
  ItdParams p;
  int nx, ny, nblocks;
  const int32_t* blk;        // ilo, ihi, jlo, jhi per block (1-based)
  int limit_aice;
  double dt;
  double *aicen, *trcrn, *vicen, *vsnon, *eicen, *esnon;
  double *aice, *aice0;
  double *fresh, *fsalt, *fhocn;            // each may be nullptr (an absent optional)
  unsigned long long* bw;                   // CW_WORDS per block, zero before the head
  // aggregate and the tendencies
  const int32_t* tmask;
  double *vice, *vsno, *eice, *esno, *trcr; // trcr: (nx, ny, max_ntrcr[, nblocks])
  double *daidtt, *dvidtt;                  // nullptr: no tendencies (the block-wise entry)
};

// what a block's words say: 0 no stop, else the stage-1 stop of cleanup_itd and its cell (0-based in the plane)
int clean_decode(const unsigned long long* w, size_t np, size_t* q);

void clean_launch_head(const CleanArgs& a, hipStream_t s);     // aggregate_area, bounds check, need of pass 1
void clean_launch_pass(const CleanArgs& a, int p, hipStream_t s);   // p = 1..8; pass 1 lifts category 1 to hin_max(0) first
void clean_launch_zap(const CleanArgs& a, hipStream_t s);      // the negative-area scan, zap_small_areas, the fluxes
void clean_launch_aggregate(const CleanArgs& a, hipStream_t s);
// the whole of cleanup_itd: head, eight passes, zap; `ev` (11 events or nullptr) is recorded in front of each and behind
void clean_launch_all(const CleanArgs& a, hipStream_t s, hipEvent_t* ev = nullptr);

// (nx*ny, levels, nb) <-> (nx*ny, nb, levels): the batch keeps a block's levels together, the Halo addresses a level's
// blocks together
void clean_launch_transpose(const double* src, double* dst, size_t np, int levels, int nb, bool to_levels_outer,
                            hipStream_t s);

}  // namespace cice
