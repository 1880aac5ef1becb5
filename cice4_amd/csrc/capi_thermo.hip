// C-ABI of libcice4_amd.so: the column thermodynamics, block-wise and on the batch of all local blocks.
#include "capi.h"

extern "C" {

// ---- thermodynamics --------------------------------------------------------------------------
int cice_thermo_init(cice_ctx* ctx, const cice_thermo_config* cfg, double* salin, double* Tmlt) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "NULL argument");
  CICE_REQUIRE(cfg->conduct == 0 || cfg->conduct == 1, "conduct must be 0 (MU71) or 1 (bubbly)");
  CICE_REQUIRE(cfg->nt_Tsfc >= 1 && cfg->nt_Tsfc <= NTRCR, "nt_Tsfc out of range");
  if (!cfg->heat_capacity)
    throw Error{CICE_EUNSUPPORTED, "zero-layer thermodynamics (heat_capacity = F) is not implemented on the device"};
  c_->tp.init(*cfg);
  c_->have_thermo = true;
  if (salin) std::memcpy(salin, c_->tp.salin, sizeof(c_->tp.salin));
  if (Tmlt) std::memcpy(Tmlt, c_->tp.Tmlt, sizeof(c_->tp.Tmlt));
  CICE_CATCH
}

int cice_thermo_vertical(cice_ctx* ctx, int nx, int ny, double dt, int icells, const int32_t* indxi,
                         const int32_t* indxj, double* aicen, double* trcrn, double* vicen,
                         double* vsnon, double* eicen, double* esnon, const double* flw,
                         const double* potT, const double* Qa, const double* rhoa,
                         const double* fsnow, const double* fbot, const double* Tbot,
                         const double* lhcoef, const double* shcoef, double* fswsfc, double* fswint,
                         double* fswthrun, double* Sswabs, double* Iswabs, double* fsurfn,
                         double* fcondtopn, double* fsensn, double* flatn, double* fswabsn,
                         double* flwoutn, double* evapn, double* freshn, double* fsaltn,
                         double* fhocnn, double* meltt, double* melts, double* meltb, double* congel,
                         double* snoice, double* mlt_onset, double* frz_onset, double yday,
                         int32_t* l_stop, int32_t* istop, int32_t* jstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(c_->have_thermo, "cice_thermo_init has not been called");
  CICE_REQUIRE(l_stop && istop && jstop, "NULL status pointer");
  CICE_REQUIRE(nx >= 1 && ny >= 1, "bad dimensions");
  const size_t np = (size_t)nx * ny;
  CICE_REQUIRE(icells >= 0 && (size_t)icells <= np, "icells out of range");
  CICE_REQUIRE(icells == 0 || (indxi && indxj), "thermo_vertical: NULL index list");
  // Every array of the call, once: its first plane in the staging buffer, its planes, its host address and which way it
  // travels.  Both paths below walk this table, in this order, for what they take to the device and what they bring back.
  // Of the tracers only Tsfc is read and written by the column physics (:137-142, :508-513).  With calc_Tsfc = F fsurfn,
  // fcondtopn and flatn are intent(in) (ice_therm_vertical.F90:213-217): they travel in, last, and are not zeroed.
  enum { TV_IN = 1, TV_OUT = 2, TV_IO = 3, TV_ZERO = 4 };
  struct TvArray { int plane, planes; const double* h; int dir; };
  const int it_T = c_->tp.nt_Tsfc - 1;
  const int O = TV_OUT | TV_ZERO, F = c_->tp.calc_Tsfc ? O : TV_OUT, F_IN = c_->tp.calc_Tsfc ? 0 : TV_IN;
  const TvArray tv[] = {
      {A_AICEN, 1, aicen, TV_IO}, {A_TRCRN + it_T, 1, trcrn ? trcrn + (size_t)it_T * np : nullptr, TV_IO},
      {A_VICEN, 1, vicen, TV_IO}, {A_VSNON, 1, vsnon, TV_IO}, {A_EICEN, NILYR, eicen, TV_IO}, {A_ESNON, NSLYR, esnon, TV_IO},
      {A_FLW, 1, flw, TV_IN}, {A_POTT, 1, potT, TV_IN}, {A_QA, 1, Qa, TV_IN}, {A_RHOA, 1, rhoa, TV_IN},
      {A_FSNOW, 1, fsnow, TV_IN}, {A_FBOT, 1, fbot, TV_IN}, {A_TBOT, 1, Tbot, TV_IN}, {A_LH, 1, lhcoef, TV_IN},
      {A_SH, 1, shcoef, TV_IN}, {A_FSWSFC, 1, fswsfc, TV_IO}, {A_FSWINT, 1, fswint, TV_IO}, {A_FSWTHRU, 1, fswthrun, TV_IN},
      {A_SSW, NSLYR, Sswabs, TV_IO}, {A_ISW, NILYR, Iswabs, TV_IO},
      {A_OUT + 0, 1, fsurfn, F}, {A_OUT + 1, 1, fcondtopn, F}, {A_OUT + 2, 1, fsensn, O}, {A_OUT + 3, 1, flatn, F},
      {A_OUT + 4, 1, fswabsn, O}, {A_OUT + 5, 1, flwoutn, O}, {A_OUT + 6, 1, evapn, O}, {A_OUT + 7, 1, freshn, O},
      {A_OUT + 8, 1, fsaltn, O}, {A_OUT + 9, 1, fhocnn, O}, {A_OUT + 10, 1, meltt, O}, {A_OUT + 11, 1, melts, O},
      {A_OUT + 12, 1, meltb, O}, {A_OUT + 13, 1, congel, O}, {A_OUT + 14, 1, snoice, O},
      {A_MLT, 1, mlt_onset, TV_IO}, {A_FRZ, 1, frz_onset, TV_IO},
      {A_OUT + 0, 1, fsurfn, F_IN}, {A_OUT + 1, 1, fcondtopn, F_IN}, {A_OUT + 3, 1, flatn, F_IN}};
  auto host = [](const TvArray& x) { return const_cast<double*>(x.h); };   // written rows are non-const arguments
  for (const TvArray& x : tv) CICE_REQUIRE(x.h != nullptr, "thermo_vertical: NULL array");   // before anything is queued
  for (int e = 0; e < icells; ++e)
    CICE_REQUIRE(indxi[e] >= 1 && indxi[e] <= nx && indxj[e] >= 1 && indxj[e] <= ny,
                 "thermo_vertical: index outside block");
  c_->need_device();
  hipStream_t s = c_->stream;
  DevBuf<double>& d = c_->tv_stage;
  DevBuf<int32_t>& li = c_->tv_list;
  const bool compact = (size_t)icells * 2 <= np;
  const size_t m = compact ? (size_t)icells : np;   // cells of a staged plane
  double* hp = nullptr;
  std::vector<size_t>& cq = c_->tv_cells;
  if (compact) {
    // Few of the block's cells carry ice of this category (the rule on a real grid: the reference compresses to a
    // list for that reason): only the listed cells travel.  The host gathers them plane by plane into a page-locked
    // buffer, ONE copy takes all planes to the device, the list kernel runs on that compact "1 x icells block", ONE
    // copy brings everything back, the host zeroes the output planes (:299-329) and scatters the listed cells.
    // 54 copies of whole planes become 2 of icells elements per plane.
    if (m == 0) {
      for (const TvArray& x : tv)
        if (x.dir & TV_ZERO) std::memset(host(x), 0, np * 8);
      clear_stop(l_stop, istop, jstop);
      return CICE_OK;
    }
    hp = static_cast<double*>(c_->tv_host.need(((size_t)A_END * m) * 8 + 2 * m * 4));
    if (d.n < (size_t)A_END * m) d.alloc((size_t)A_END * std::max(m, np / 8));
    if (li.n < 2 * m) li.alloc(2 * std::max(m, np / 8));
    int32_t* hl = reinterpret_cast<int32_t*>(hp + (size_t)A_END * m);
    cq.resize(m);
    for (size_t e = 0; e < m; ++e) {
      cq[e] = (size_t)(indxj[e] - 1) * nx + (indxi[e] - 1);
      hl[e] = (int32_t)e + 1;      // the compact block is one row of m cells
      hl[m + e] = 1;
    }
    for (const TvArray& x : tv)
      for (int k = 0; k < x.planes && (x.dir & TV_IN); ++k) {
        double* o = hp + (size_t)(x.plane + k) * m;
        const double* src = x.h + (size_t)k * np;
        for (size_t e = 0; e < m; ++e) o[e] = src[cq[e]];
      }
    CICE_HIP(hipMemcpyAsync(d.p, hp, (size_t)A_END * m * 8, hipMemcpyHostToDevice, s));
    CICE_HIP(hipMemcpyAsync(li.p, hl, 2 * m * 4, hipMemcpyHostToDevice, s));
  } else {
    if (d.n < (size_t)A_END * np) d.alloc((size_t)A_END * np);
    if (li.n < 2 * np) li.alloc(2 * np);
    c_->fan.fork(s);   // 22 separate host arrays in, 27 out: spread over the side streams
    for (const TvArray& x : tv)
      if (x.dir & TV_IN)
        CICE_HIP(hipMemcpyAsync(d.p + (size_t)x.plane * np, x.h, (size_t)x.planes * np * 8, hipMemcpyHostToDevice, c_->cs()));
    CICE_HIP(hipMemcpyAsync(li.p, indxi, (size_t)icells * 4, hipMemcpyHostToDevice, c_->cs()));
    CICE_HIP(hipMemcpyAsync(li.p + np, indxj, (size_t)icells * 4, hipMemcpyHostToDevice, c_->cs()));
    c_->fan.join();
  }
  c_->tkey.alloc(THERMO_STATUS_WORDS);
  thermo_status_reset(c_->tkey.p, s);
  // the staged block: one row of the m listed cells, or the caller's block
  ThermoArgs a = thermo_args(c_->tp, c_->tkey.p, compact ? (int)m : nx, compact ? 1 : ny, 1, 1, dt, yday,
                             [&](int plane) { return d.p + (size_t)plane * m; });
  a.icells = icells; a.indxi = li.p; a.indxj = li.p + m;
  thermo_launch_list(a, s);
  if (compact) {
    CICE_HIP(hipMemcpyAsync(hp, d.p, (size_t)A_END * m * 8, hipMemcpyDeviceToHost, s));
  } else {
    c_->fan.fork(s);
    for (const TvArray& x : tv)
      if (x.dir & TV_OUT)
        CICE_HIP(hipMemcpyAsync(host(x), d.p + (size_t)x.plane * np, (size_t)x.planes * np * 8, hipMemcpyDeviceToHost, c_->cs()));
    c_->fan.join();
  }
  unsigned long long key = 0;
  CICE_HIP(hipMemcpyAsync(&key, c_->tkey.p, 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));
  if (compact) {
    for (const TvArray& x : tv)
      if (x.dir & TV_ZERO) std::memset(host(x), 0, np * 8);
    for (const TvArray& x : tv)
      for (int k = 0; k < x.planes && (x.dir & TV_OUT); ++k) {
        const double* in = hp + (size_t)(x.plane + k) * m;
        double* dst = host(x) + (size_t)k * np;
        for (size_t e = 0; e < m; ++e) dst[cq[e]] = in[e];
      }
  }
  decode_err(key, nx, 1, indxi, indxj, l_stop, istop, jstop, nullptr, nullptr);
  CICE_CATCH
}

// ---- the column batch (batch.h) ---------------------------------------------------------------
int cice_thermo_batch_alloc(cice_ctx* ctx, int nx, int ny, int nb) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nx >= 3 && ny >= 3 && nb >= 1, "bad dimensions");
  c_->need_device();
  c_->batch.alloc(c_->stream, c_->fan, nx, ny, nb, c_->have_domain ? &c_->dom : nullptr);
  CICE_CATCH
}

int cice_thermo_batch_upload(cice_ctx* ctx, const cice_thermo_fields* h) {
  CICE_TRY(ctx) c_->chain_ready = false; NEED_BATCH(h); c_->batch.upload(c_->thermo(), h); CICE_CATCH
}

int cice_thermo_set_chio(cice_ctx* ctx, double chio) {
  CICE_TRY(ctx)
#ifdef CICE4_AMD_AUSCOM
  c_->chio = chio;   // a kernel argument of frzmlt_bottom_lateral: later launches see it
#else
  (void)chio;
  throw Error{CICE_EINVAL, "cice_thermo_set_chio: this is the stand-alone build of the library (chio is the constant "
                           "0.006 there, ice_therm_vertical.F90:680); the coupled one is libcice4_amd_auscom.so"};
#endif
  CICE_CATCH
}

int cice_thermo_set_option(cice_ctx* ctx, const char* key, int value) {
  CICE_TRY(ctx) CICE_REQUIRE(key, "NULL key"); c_->batch.set_option(key, value); CICE_CATCH
}

int cice_thermo_batch_step(cice_ctx* ctx, double dt, double yday, long long* n_updates,
                           int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop,
                           int32_t* bstop, float* elapsed_ms) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(l_stop && istop && jstop, "NULL status pointer");
  NEED_BATCH(true);
  c_->batch.step(c_->thermo(), dt, yday, n_updates, l_stop, istop, jstop, nstop, bstop, elapsed_ms);
  CICE_CATCH
}

int cice_thermo_batch_download(cice_ctx* ctx, cice_thermo_fields* h) {
  CICE_TRY(ctx) c_->chain_ready = false; NEED_BATCH(h); c_->batch.download(c_->thermo(), h); CICE_CATCH
}

int cice_thermo_batch_merge(cice_ctx* ctx, const cice_merge_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false; NEED_BATCH(f); c_->batch.merge(f); CICE_CATCH
}

// The thermodynamic half of a time step in one call (ColumnBatch::step_therm1) ...
int cice_step_therm1(cice_ctx* ctx, double dt, double yday, cice_thermo_fields* st,
                     const cice_frzmlt_fields* fz, const cice_merge_fields* mg, long long* n_updates,
                     int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  NEED_BATCH(true);
  c_->batch.step_therm1(c_->thermo(), c_->chio, dt, yday, st, fz, mg, nullptr, n_updates, l_stop, istop, jstop, nstop, bstop);
  CICE_CATCH
}

// ... with atmo_boundary_layer on the device as well: lhcoef / shcoef of `st` and the four atmosphere fields of `mg`
// are not read; what the routine produced comes back through `atm` where asked for.
int cice_step_therm1_abl(cice_ctx* ctx, double dt, double yday, cice_thermo_fields* st,
                         const cice_frzmlt_fields* fz, const cice_merge_fields* mg, const cice_atmo_fields* atm,
                         long long* n_updates, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop,
                         int32_t* bstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(atm != nullptr, "NULL argument");
  NEED_BATCH(true);
  c_->batch.step_therm1(c_->thermo(), c_->chio, dt, yday, st, fz, mg, atm, n_updates, l_stop, istop, jstop, nstop, bstop);
  CICE_CATCH
}

// atmo_boundary_layer (source/ice_atmo.F90:56-384), one block, host pointers, the reference's argument list
// (sfctype: 0 'ice', 1 'ocn'; calc_strair is the module variable of ice_atmo).
int cice_atmo_boundary_layer(cice_ctx* ctx, int nx, int ny, int sfctype, int icells, const int32_t* indxi,
                             const int32_t* indxj, const double* Tsf, const double* potT, const double* uatm,
                             const double* vatm, const double* wind, const double* zlvl, const double* Qa,
                             const double* rhoa, int calc_strair, double* strx, double* stry, double* Tref,
                             double* Qref, double* delt, double* delq, double* lhcoef, double* shcoef) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nx >= 1 && ny >= 1 && icells >= 0 && (size_t)icells <= (size_t)nx * ny, "bad dimensions");
  CICE_REQUIRE(sfctype == 0 || sfctype == 1, "sfctype: 0 'ice' or 1 'ocn'");
  CICE_REQUIRE(Tsf && potT && uatm && vatm && wind && zlvl && Qa && rhoa && strx && stry && Tref && Qref && delt &&
                   delq && lhcoef && shcoef && (icells == 0 || (indxi && indxj)), "atmo_boundary_layer: NULL array");
  c_->need_device();
  hipStream_t s = c_->stream;
  const size_t np = (size_t)nx * ny;
  DevBuf<double>& d = c_->fz_stage;
  if (d.n < 16 * np) d.alloc(16 * np);
  DevBuf<int32_t>& li = c_->tv_list;
  if (li.n < 2 * np) li.alloc(2 * np);
  const double* in[8] = {Tsf, potT, uatm, vatm, wind, zlvl, Qa, rhoa};
  for (int k = 0; k < 8; ++k) CICE_HIP(hipMemcpyAsync(d.p + (size_t)k * np, in[k], np * 8, hipMemcpyHostToDevice, s));
  if (!calc_strair) {   // strx, stry are left as they are (:309)
    CICE_HIP(hipMemcpyAsync(d.p + 8 * np, strx, np * 8, hipMemcpyHostToDevice, s));
    CICE_HIP(hipMemcpyAsync(d.p + 9 * np, stry, np * 8, hipMemcpyHostToDevice, s));
  }
  if (icells > 0) {
    CICE_HIP(hipMemcpyAsync(li.p, indxi, (size_t)icells * 4, hipMemcpyHostToDevice, s));
    CICE_HIP(hipMemcpyAsync(li.p + np, indxj, (size_t)icells * 4, hipMemcpyHostToDevice, s));
  }
  AtmoArgs a{};
  a.p.init();
  a.nx = nx; a.ny = ny; a.ncat = 1; a.nblocks = 1; a.ocn = sfctype; a.calc_strair = calc_strair != 0;
  a.icells = icells; a.indxi = li.p; a.indxj = li.p + np;
  a.Tsf = d.p; a.potT = d.p + np; a.uatm = d.p + 2 * np; a.vatm = d.p + 3 * np; a.wind = d.p + 4 * np;
  a.zlvl = d.p + 5 * np; a.Qa = d.p + 6 * np; a.rhoa = d.p + 7 * np;
  double* out[8] = {strx, stry, Tref, Qref, delt, delq, lhcoef, shcoef};
  double** dev[8] = {&a.strx, &a.stry, &a.Tref, &a.Qref, &a.delt, &a.delq, &a.lhcoef, &a.shcoef};
  for (int k = 0; k < 8; ++k) *dev[k] = d.p + (size_t)(8 + k) * np;
  atmo_launch_list(a, s);
  for (int k = 0; k < 8; ++k) CICE_HIP(hipMemcpyAsync(out[k], *dev[k], np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));
  CICE_CATCH
}

int cice_frzmlt_bottom_lateral(cice_ctx* ctx, int nx, int ny, int ilo, int ihi, int jlo, int jhi,
                               double dt, const double* aice, const double* frzmlt,
                               const double* eicen, const double* esnon, const double* sst,
                               const double* Tf, const double* strocnxT, const double* strocnyT,
                               double* Tbot, double* fbot, double* rside) {
  CICE_TRY(ctx)
  CICE_REQUIRE(c_->have_thermo, "cice_thermo_init has not been called");
  CICE_REQUIRE(nx >= 1 && ny >= 1 && ilo >= 1 && ihi <= nx && jlo >= 1 && jhi <= ny, "bad dimensions");
  CICE_REQUIRE(aice && frzmlt && eicen && esnon && sst && Tf && strocnxT && strocnyT && Tbot && fbot && rside,
               "frzmlt_bottom_lateral: NULL array");     // before anything is queued on the stream
  c_->need_device();
  hipStream_t s = c_->stream;
  const size_t np = (size_t)nx * ny;
  const int NE = NCAT * NILYR, NSN = NCAT * NSLYR;
  DevBuf<double>& d = c_->fz_stage;
  if (d.n < (size_t)(9 + NE + NSN) * np) d.alloc((size_t)(9 + NE + NSN) * np);
  auto up = [&](size_t plane, const double* h, size_t planes = 1) {
    CICE_REQUIRE(h != nullptr, "frzmlt_bottom_lateral: NULL array");
    CICE_HIP(hipMemcpyAsync(d.p + plane * np, h, planes * np * 8, hipMemcpyHostToDevice, s));
  };
  up(0, aice); up(1, frzmlt); up(2, sst); up(3, Tf); up(4, strocnxT); up(5, strocnyT);
  up(9, eicen, NE); up(9 + NE, esnon, NSN);
  FrzmltArgs a{};
  a.nx = nx; a.ny = ny; a.ilo = ilo; a.ihi = ihi; a.jlo = jlo; a.jhi = jhi; a.dt = dt;
  a.ustar_min = c_->tp.ustar_min; a.chio = c_->chio;
  a.aice = d.p; a.frzmlt = d.p + np; a.sst = d.p + 2 * np; a.Tf = d.p + 3 * np;
  a.strocnxT = d.p + 4 * np; a.strocnyT = d.p + 5 * np;
  a.Tbot = d.p + 6 * np; a.fbot = d.p + 7 * np; a.rside = d.p + 8 * np;
  a.eicen = d.p + 9 * np; a.esnon = d.p + (size_t)(9 + NE) * np;
  frzmlt_launch(a, s);
  CICE_HIP(hipMemcpyAsync(Tbot, a.Tbot, np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(fbot, a.fbot, np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(rside, a.rside, np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));
  CICE_CATCH
}

}  // extern "C"
