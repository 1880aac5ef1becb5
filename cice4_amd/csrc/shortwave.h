// Shortwave radiation, shortwave = 'default' (ccsm3), on the device: shortwave_ccsm3 with compute_albedos, constant_albedos
// and absorbed_solar (source/ice_shortwave.F90:364-1185) as one kernel, and the scaling of prep_radiation
// (source/ice_step_mod.F90:84-218) as another.  Delta-Eddington: dedd.h.
//
// Arithmetic: the reference's operations in the reference's order, uncontracted (the Makefile's -ffp-contract=off).  exp is
// the restated glibc exp of libm_exact.h, one call per ice layer with the reference's argument expression
// (exp_libm(-0.0) = 1: its tiny-argument path returns 1 + x).  atan(hi*c4) is the device library's (<= 1 ulp; DESIGN.md
// 3.6), so the bare-ice albedos of ice thinner than ahmax, and what absorbed_solar makes of them, agree with the reference
// to ~1e-15, not bit for bit; fhtan = atan(ahmax*c4) comes from the host libm.  Everything else is bit for bit.
#pragma once
#include "common.h"

namespace cice {

// module variables of ice_shortwave (namelist) and what the stand-alone build has as parameters (dT_mlt, dalb_mlt,
// snowpatch, albocn: namelist values under -DAusCOM), as cice_shortwave_init was given them
struct ShortwaveParams {
  int albedo_type;                     // 0 'default', 1 'constant'
  double albicev, albicei, albsnowv, albsnowi, ahmax;
  double fhtan;                        // atan(ahmax*c4), host libm
  double albocn, dT_mlt, dalb_mlt, snowpatch;
  double awtvdr, awtidr, awtvdf, awtidf;
};

// One launch over (cells of a plane, categories, blocks).  np = nx * ny cells per plane.  Per-category arrays are
// (np, ncat, nb); Tsfc is plane 0 of every tsfc_planes consecutive planes (the tracer array seen from its nt_Tsfc plane, or
// a plain (np, ncat, nb) array with tsfc_planes = 1); sw* and ocn_albedo are (np, nb); Iswabs (np, nilyr, ncat, nb),
// Sswabs (np, nslyr, ncat, nb) or NULL (the block-wise entry: the caller's array).
// The list: `listed` (np int32 per block, non-zero = on the list; the block-wise entry) or, where it is NULL, the reference
// driver's predicate aicen > puny on the physical cells blk[4b .. 4b+3] = ilo, ihi, jlo, jhi (1-based).
struct ShortwaveArgs {
  ShortwaveParams p;
  int nx, np, ncat, nb, tsfc_planes;
  const int32_t* blk;
  const int32_t* listed;
  const double *aicen, *vicen, *vsnon, *Tsfc;
  const double *swvdr, *swvdf, *swidr, *swidf;
  const double* ocn_albedo;            // NULL: the scalar p.albocn
  double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon;
  double *fswsfcn, *fswintn, *fswthrun, *Iswabsn, *Sswabsn;
};
void shortwave_launch(const ShortwaveArgs& a, hipStream_t s);

// prep_radiation on (cells of a plane, blocks), the category loop inside a thread: scale_factor is read and written in
// place, so the thread that writes a cell's new value is the only one that reads it.  All 2-d fields (np, nb); the five
// per-category arrays and aicen as above.
struct PrepRadiationArgs {
  int nx, np, ncat, nb;
  const int32_t* blk;
  const double *swvdr, *swvdf, *swidr, *swidf, *alvdr_gbm, *alvdf_gbm, *alidr_gbm, *alidf_gbm, *aice, *aicen;
  double *scale_factor, *fswfac;
  double *fswsfcn, *fswintn, *fswthrun, *Sswabsn, *Iswabsn;
};
void prep_radiation_launch(const PrepRadiationArgs& a, hipStream_t s);

}  // namespace cice
