// Shortwave radiation, shortwave = 'dEdd' (delta-Eddington), on the device: what step_radiation does for one (cell,
// category) in its dEdd branch (source/ice_step_mod.F90:872-916) -- shortwave_dEdd_set_snow, shortwave_dEdd_set_pond,
// shortwave_dEdd with its three compute_dEdd passes (bare ice, snow, pond), each over three spectral bands with
// solution_dEdd inside (source/ice_shortwave.F90:1372-3681) -- as ONE kernel, k_shortwave_dedd.
//
// Arithmetic: the reference's operations in the reference's order, uncontracted (the Makefile's -ffp-contract=off); the
// statement functions alpha, gamma, n, u, el, taus, omgs, asys with their parentheses as written.  The scheme's only
// transcendental functions are exp and sqrt: exp is the restated glibc exp of libm_exact.h, called with the reference's
// argument expression and clamped by max(exp_min, .) as there; sqrt and division are correctly rounded on the device.  So
// every output word is meant to carry the compiled reference's bits.
#pragma once
#include "common.h"

namespace cice {

// What cice_shortwave_dedd_init was given, and what it derives once on the host: the tuned optical properties of bare and
// ponded ice (compute_dEdd :2357-2423 from R_ice, R_pnd) and exp_min = exp(-10) of the host libm (init_dEdd :1267).
struct DeddParams {
  int tr_pond;                         // 1: fp, hp from the caller's apondn, hpondn; 0: shortwave_dEdd_set_pond
  double R_snw;
  double awtvdr, awtidr, awtvdf, awtidf;
  double exp_min;
  double ki_ssl[3], wi_ssl[3], gi_ssl[3], ki_dl[3], wi_dl[3], gi_dl[3], ki_int[3], wi_int[3], gi_int[3];
  double ki_p_ssl[3], wi_p_ssl[3], gi_p_ssl[3], ki_p_int[3], wi_p_int[3], gi_p_int[3];
};
// the tuning of :2357-2423 in plain C++, the reference's operation order, compiled without contraction
void dedd_tune(DeddParams& p, double R_ice, double R_pnd);

// One launch over (cells of a plane, categories, blocks), laid out as ShortwaveArgs (shortwave.h).  np = nx * ny.
// Per-category arrays (np, ncat, nb); coszen and sw* (np, nb); Iswabs (np, nilyr, ncat, nb), Sswabs (np, nslyr, ncat, nb).
// The list: `listed` (the block-wise entry) or aicen > puny on the physical cells of blk.
// snow_given (the block-wise entry, a drop-in for shortwave_dEdd alone): fs, fp, hp (np) and rhosnw, rsnw (np, nslyr) are
// inputs and Tsfc is not read.  Otherwise set_snow runs in the thread, and set_pond unless p.tr_pond, where fp, hp are the
// (np, ncat, nb) arrays apondn, hpondn.
// Every output is written on every cell: zero off the list and where coszen <= puny, the four albedos included.
struct DeddArgs {
  DeddParams p;
  int nx, np, ncat, nb, tsfc_planes, snow_given;
  const int32_t* blk;
  const int32_t* listed;
  const double *aicen, *vicen, *vsnon, *Tsfc, *coszen;
  const double *swvdr, *swvdf, *swidr, *swidf;
  const double *fs, *rhosnw, *rsnw, *fp, *hp;
  double *alvdrn, *alvdfn, *alidrn, *alidfn, *fswsfcn, *fswintn, *fswthrun, *Sswabsn, *Iswabsn;
  double *albicen, *albsnon, *albpndn;
};
void dedd_launch(const DeddArgs& a, hipStream_t s);

}  // namespace cice
