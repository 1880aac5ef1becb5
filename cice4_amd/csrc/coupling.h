// coupling_prep (drivers/cice4/CICE_RunMod.F90:588-767) on the device: the mixed layer (ocean_mixed_layer,
// source/ice_ocean.F90:64-234, atmbndy = 'default') as one kernel, and the area-weighted merge of the per-category albedos,
// the *_gbm copies, scale_factor and scale_fluxes (source/ice_flux.F90:776-888) as another.
//
// Arithmetic: the reference's operations in the reference's order, uncontracted (the Makefile's -ffp-contract=off); every
// step of k_coupling_prep and of the mixed layer's tail (:190-231) is one correctly rounded operation, so those agree with
// the reference bit for bit.  x**4 is ((x*x)*x)*x, the form the reference's compiler gives both (Tf + Tffresh)**4 of
// scale_fluxes and TsfK**4 of the mixed layer, as it does in therm.hip: (x*x)*(x*x) differs from the compiled reference in
// the last bit of some cells (tests/golden/make_golden_coupling.py holds the restatement that uses this form
// to the compiled reference's bits).  The boundary layer is atmo_cell of atmo_cell.h: its log and atan are the device
// library's, so delt, delq are bit for bit and the six other outputs agree to ~1e-15.
//
// atmbndy = 'constant' is not built: in that branch the reference never sets its local arrays delt and delq
// (ice_ocean.F90:139-150) and then multiplies by them (:207-208).  sfcflux_to_ocn (CICE_RunMod.F90:747) is empty unless
// the reference is compiled -DCICE_IN_NEMO: nothing is built for it.
#pragma once
#include "atmo.h"
#include "common.h"

namespace cice {

// what cice_coupling_init was given
struct CouplingParams {
  int scale, mixed;                    // scale_fluxes is called; oceanmixed_ice
  double albocn;
};

// The 13 in / out fields of scale_fluxes in the order of its argument list; behind them it has the four merged albedos.
enum { CPL_STRAIRX = 0, CPL_STRAIRY, CPL_FSENS, CPL_FLAT, CPL_FSWABS, CPL_FLWOUT, CPL_EVAP, CPL_TREF, CPL_QREF, CPL_FRESH,
       CPL_FSALT, CPL_FHOCN, CPL_FSWTHRU, CPL_FLUXES };

// One launch over (cells of a plane, 1, blocks), EVERY cell of a block (the reference loops 1..nx_block, 1..ny_block).
// np = nx * ny cells per plane; per-category arrays (np, ncat, nb), 2-d fields (np, nb), albcnt (np, nb, nstreams).
struct CouplingArgs {
  int np, ncat, nb, nstreams, scale;   // scale = 0: scale_fluxes is skipped (a reference compiled -DAusCOM)
  const int32_t* tmask;
  const double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon, *albpndn;   // albpndn NULL: zeros
  const double* aicen;
  const double *coszen, *aice, *Tf, *Tair, *Qa, *swvdr, *swvdf, *swidr, *swidf;
  double* flux[CPL_FLUXES];            // scale = 0: only fresh, fsalt, fhocn, fswthru, and they are read only
  double *alvdr, *alidr, *alvdf, *alidf, *albice, *albsno, *albpnd;
  double *alvdf_gbm, *alidf_gbm, *alvdr_gbm, *alidr_gbm, *fresh_gbm, *fsalt_gbm, *fhocn_gbm, *fswthru_gbm;
  double* scale_factor;
  double* albcnt;                      // NULL: no history count
};
void coupling_prep_launch(const CouplingArgs& a, hipStream_t s);

// One launch over (cells of a plane, 1, blocks), every cell of a block.  All fields (np, nb).
struct MixedLayerArgs {
  AtmoParams p;
  int np, nb;
  double dt, albocn;
  const int32_t* tmask;
  const double *potT, *uatm, *vatm, *wind, *zlvl, *Qa, *rhoa, *flw, *hmix, *Tf, *aice, *fhocn, *fswthru;
  const double *swvdr, *swvdf, *swidr, *swidf;
  double *sst, *qdp;                   // in / out
  double *frzmlt, *flwout_ocn, *fsens_ocn, *flat_ocn, *evap_ocn, *strairx_ocn, *strairy_ocn, *Tref_ocn, *Qref_ocn;
  double *alvdr_ocn, *alidr_ocn, *alvdf_ocn, *alidf_ocn;
  double *delt, *delq, *shcoef, *lhcoef;   // the reference's local arrays: each may be NULL
};
void ocean_mixed_layer_launch(const MixedLayerArgs& a, hipStream_t s);

}  // namespace cice
