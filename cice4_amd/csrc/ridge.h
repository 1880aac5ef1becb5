// Mechanical redistribution on the device: ridge_ice of source/ice_mechred.F90 (:133-552) with asum_ridging :573,
// ridge_prep :647, ridge_itd :773, ridge_shift :1099, ridge_check :1788 and compute_tracers of source/ice_itd.F90 :1482.
// The column half of step_dynamics (source/ice_step_mod.F90:586-745) is this routine and then what cleanup.h holds.
//
// One thread per cell, the category loop inside, the reference's planes, fp64, no contraction -- as in itd.h, cleanup.h.
//
// THE REPEAT FLAG IS BLOCK-WIDE.  ridge_ice repeats ridge_itd + ridge_shift up to nitermax = 20 times; ridge_check sets
// ONE iterate_ridging per block: while any listed cell of a block has abs(asum - 1) >= puny, EVERY listed cell of that
// block goes round again.  A converged cell has closing_net = opning = 0 and ridges nothing, but its tracers still go
// through atrcrn = aicen*trcrn and back (not the identity in the last bit), and compute_tracers' `trcrn(:,:,:) = c0`
// zeroes the tracers of every cell of the block that is NOT listed, in every iteration.  A block without a listed cell
// is never called and keeps its tracers.  No thread waits for another: an iteration is two launches, and what it has to
// know about its block is a word in device memory, RW_ITER + k, raised by the launch in front of it (iteration 1: by the
// rate kernel of that iteration, from the listed cells themselves).  A block whose word is down leaves at once.  The host
// queues RIDGE_QUEUE iterations, reads the block words once (they carry the stops too) and queues more only while a block
// still asks (DESIGN.md 8.4 for the number).
//
// TWO LAUNCHES PER ITERATION, because of the stop `aice0 < -puny` (:1344-1352): it names the FIRST failing cell in list
// order; the cells in front of it hold their new aice0, the failing cell its negative value, and nothing else of the
// iteration has happened.  So k_ridge_rates computes ridge_itd, closing_gross with its cuts and the new aice0 into work
// planes and raises RW_STOP_AICE0 with atomicMax of (2^32 - 1 - list position); k_ridge_shift either commits aice0 up to
// that position and leaves, or commits it everywhere and shifts.  k_ridge_shift evaluates ridge_itd again from the same
// aicen, vicen, aice0 (the same operations give the same bits) instead of carrying 21 planes across the boundary.
//
// SNAPSHOTS.  ridge_shift takes aicen_init ... esnon_init once per iteration; category n gives init(n)*afrac while
// aicen(n) may already hold what the categories below ridged into it.  Everything a transfer is made of -- afrac(n),
// ardg1n, ardg2n, virdgn, vsrdgn, farea(n, nr), fvol(n, nr) -- depends on the snapshot and on ridge_itd only, so the
// thread forms them once and then walks each array element on its own (areas and volumes, each energy layer, each
// tracer) in the reference's order: for n = 1..ncat the subtraction at n, then the additions for nr = 1..ncat.
//
// OTHER STOPS.
//   - `ardg > aicen` (:1432).  Unreachable: closing_gross has just been cut by tmpfac = aicen(n)/wk1 with
//     wk1 = apartic(n)*closing_gross*dt, so afterwards apartic(n)*closing_gross*dt equals aicen(n) up to three
//     roundings, a relative 4e-16; later cuts only lower closing_gross.  The stop asks for an excess of puny = 1e-11
//     ABSOLUTE, i.e. an area of 1e4 or more in one category.  Built as a rule all the same: the thread raises
//     RW_STOP_ARDG with the first category and in it the first list position, and gives up; the block runs no further
//     iteration and writes no diagnostics.  UNPINNED, and what the other cells of the block hold then is the finished
//     iteration, not the reference's half-finished one.
//   - niter == nitermax (:392-398): l_stop with istop = jstop = 0, the state holds 20 iterations, no diagnostics.  It is
//     the word RW_ITER + 21, raised behind iteration 20.  UNPINNED (a seeded search found no input past 14 iterations).
//   - "total area > 1" (:532-550) is dead: the loop is left only by `exit` when no cell has abs(asum - 1) >= puny, and
//     the final check asks for abs(asum - 1) > puny of the same asum.
//
// krdg_redist = 0 IS NOT BUILT (CICE_EUNSUPPORTED).  In the reference's ridge_shift, hrmax is indexed by the compressed
// counter of ridging cells instead of the cell (`hrmax(ij,n)` :1495-1496, :1601-1607 with ij over iridge): a cell reads
// another cell's hrmax.  Reproducing that needs a per-block, per-category rank of ridging cells, and no ice_in of the
// reference's input_templates uses it.  krdg_partic 0 and 1, tr_lvl and trcr_depend 0, 1, 2 are built.
#pragma once
#include "itd.h"

namespace cice {

constexpr int RIDGE_NITERMAX = 20;   // :245
constexpr int RIDGE_QUEUE = 3;       // iterations queued before the block words are read

struct RidgeParams {   // cice_ridge_init
  int krdg_partic, krdg_redist;
  double mu_rdg;
};

// words of a block; RW_ITER + k, k = 1..21: iteration k is wanted (k = 21: nitermax exceeded)
enum { RW_STOP_AICE0 = 0, RW_STOP_ARDG = 1, RW_NITER = 2, RW_ITER = 3, RW_WORDS = RW_ITER + RIDGE_NITERMAX + 2 };
// work planes, (nx, ny[, nblocks]) each: what ridge_ice keeps per listed cell between its routines
enum { RG_CLOSING = 0, RG_OPNING, RG_CGROSS, RG_AICE0N, RG_ARDG1, RG_ARDG2, RG_VIRDG, RG_AOPEN, RG_MSNOW, RG_ESNOW,
       RG_PLANES };

struct RidgeArgs {
  ItdParams p;
  RidgeParams r;
  int nx, ny, nblocks;
  const int32_t* listpos;    // per cell: 0 = not listed, else its 1-based position in the block's list order
  double dt;
  const double *rdg_conv, *rdg_shear;
  double *aicen, *trcrn, *vicen, *vsnon, *eicen, *esnon, *aice0;
  double *dardg1dt, *dardg2dt, *dvirdgdt, *opening, *fresh, *fhocn;   // each may be nullptr (an absent optional)
  double* work;              // RG_PLANES planes
  unsigned long long* bw;    // RW_WORDS per block, zero before iteration 1
};

enum { RIDGE_OK = 0, RIDGE_STOP_AICE0 = 1, RIDGE_STOP_ARDG = 2, RIDGE_STOP_NITER = 3 };
// what a block's words say: the stop, the list position it names (0: none) and the iterations the block ran
int ridge_decode(const unsigned long long* w, unsigned* listpos, int* niter);
// after `done` iterations: does the block ask for another one
bool ridge_wants_more(const unsigned long long* w, int done);

// iterations first .. first + count - 1 (1-based): the rate kernel and the shift kernel of each; `ev`: 2*count + 1 events
void ridge_launch_iterations(const RidgeArgs& a, int first, int count, hipStream_t s, hipEvent_t* ev = nullptr);
// the diagnostics and the two fluxes (:478-526) of every block that came to an end without a stop
void ridge_launch_finish(const RidgeArgs& a, hipStream_t s);
// the one-call stage's list: listpos = cell + 1 on the physical tmask cells of blk (ilo, ihi, jlo, jhi per block)
void ridge_launch_list(int32_t* listpos, const int32_t* tmask, const int32_t* blk, int nx, int ny, int nblocks,
                       hipStream_t s);

}  // namespace cice
