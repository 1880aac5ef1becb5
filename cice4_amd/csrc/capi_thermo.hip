// C-ABI of libcice4_amd.so: the column thermodynamics, block-wise and on the batch of all local blocks.
#include "capi.h"

// The device arrays of a ThermoArgs by name.  The values are the planes of cice_thermo_vertical's staging buffer (a field of
// several planes is named by its first); A_OUT + k: the 15 per-category outputs, fsurfn ... snoice in ThermoArgs' order.
enum { A_AICEN = 0, A_TRCRN = 1, A_VICEN = A_TRCRN + NTRCR, A_VSNON, A_EICEN, A_ESNON = A_EICEN + NILYR,
       A_FLW = A_ESNON + NSLYR, A_POTT, A_QA, A_RHOA, A_FSNOW, A_FBOT, A_TBOT, A_LH, A_SH, A_FSWSFC,
       A_FSWINT, A_FSWTHRU, A_SSW, A_ISW = A_SSW + NSLYR, A_OUT = A_ISW + NILYR, A_MLT = A_OUT + 15,
       A_FRZ, A_END };

// the status words before a launch: no error key, no column counted
static void thermo_status_reset(cice_ctx* c) {
  CICE_HIP(hipMemsetAsync(c->tkey.p, 0xff, 8, c->stream));
  CICE_HIP(hipMemsetAsync(c->tkey.p + 1, 0, (THERMO_STATUS_WORDS - 1) * 8, c->stream));
}

// The arguments of a launch on (nx, ny, ncat, nblocks): plane_of(A_...) is the device array of that name.  What is left at
// zero is the caller's: the list (icells, indxi, indxj) or the dense mode's blk and niter.
template <class PlaneOf>
static ThermoArgs thermo_args(cice_ctx* c, int nx, int ny, int ncat, int nblocks, double dt, double yday, PlaneOf plane_of) {
  ThermoArgs a{};
  a.p = c->tp; a.nx = nx; a.ny = ny; a.ncat = ncat; a.nblocks = nblocks; a.dt = dt; a.yday = yday;
  a.aicen = plane_of(A_AICEN); a.trcrn = plane_of(A_TRCRN); a.vicen = plane_of(A_VICEN); a.vsnon = plane_of(A_VSNON);
  a.eicen = plane_of(A_EICEN); a.esnon = plane_of(A_ESNON); a.flw = plane_of(A_FLW); a.potT = plane_of(A_POTT);
  a.Qa = plane_of(A_QA); a.rhoa = plane_of(A_RHOA); a.fsnow = plane_of(A_FSNOW); a.fbot = plane_of(A_FBOT);
  a.Tbot = plane_of(A_TBOT); a.lhcoef = plane_of(A_LH); a.shcoef = plane_of(A_SH); a.fswsfc = plane_of(A_FSWSFC);
  a.fswint = plane_of(A_FSWINT); a.fswthrun = plane_of(A_FSWTHRU); a.Sswabs = plane_of(A_SSW); a.Iswabs = plane_of(A_ISW);
  double** outs[15] = {&a.fsurfn, &a.fcondtopn, &a.fsensn, &a.flatn, &a.fswabsn, &a.flwoutn, &a.evapn,
                       &a.freshn, &a.fsaltn, &a.fhocnn, &a.meltt, &a.melts, &a.meltb, &a.congel,
                       &a.snoice};
  for (int k = 0; k < 15; ++k) *outs[k] = plane_of(A_OUT + k);
  a.mlt_onset = plane_of(A_MLT); a.frz_onset = plane_of(A_FRZ);
  a.errkey = c->tkey.p; a.nupdates = c->tkey.p + THERMO_COUNT_STRIDE;
  return a;
}

void batch_tracer_copy(cice_ctx* c, int it, const double* from, double* to, hipMemcpyKind kind) {
  const auto& t = c->tb;
  const size_t np = (size_t)t.nx * t.ny, o = (size_t)it * np, pitch = (size_t)NTRCR * np * 8;
  CICE_HIP(hipMemcpy2DAsync(to + o, pitch, from + o, pitch, np * 8, (size_t)NCAT * t.nb, kind, c->cs()));
}

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

static void decode_err(unsigned long long key, int nx, int ncat, const int32_t* indxi,
                       const int32_t* indxj, int32_t* l_stop, int32_t* istop, int32_t* jstop,
                       int32_t* nstop, int32_t* bstop) {
  clear_stop(l_stop, istop, jstop);
  if (nstop) *nstop = 0;
  if (bstop) *bstop = 0;
  if (key == ~0ull) return;
  *l_stop = 1;
  const unsigned long long order = key & ((1ull << 40) - 1);
  const unsigned long long cb = key >> 44;
  if (indxi) {
    *istop = indxi[order];
    *jstop = indxj[order];
  } else {
    *jstop = (int32_t)(order / nx) + 1;
    *istop = (int32_t)(order % nx) + 1;
  }
  if (nstop) *nstop = (int32_t)(cb % ncat) + 1;
  if (bstop) *bstop = (int32_t)(cb / ncat) + 1;
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
  thermo_status_reset(c_);
  // the staged block: one row of the m listed cells, or the caller's block
  ThermoArgs a = thermo_args(c_, compact ? (int)m : nx, compact ? 1 : ny, 1, 1, dt, yday,
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

int cice_thermo_batch_alloc(cice_ctx* ctx, int nx, int ny, int nb) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nx >= 3 && ny >= 3 && nb >= 1, "bad dimensions");
  c_->need_device();
  auto& t = c_->tb;
  t.nx = nx; t.ny = ny; t.nb = nb;
  t.kept_aicen_init = false;
  const size_t np = (size_t)nx * ny, n2 = np * nb, nc = n2 * NCAT;
  std::vector<int32_t> hb;
  if (c_->have_domain && c_->dom.nblocks() == nb && c_->dom.nx_block == nx && c_->dom.ny_block == ny) {
    for (int gid : c_->dom.local) {
      const Block& b = c_->dom.all[gid];
      hb.insert(hb.end(), {b.ilo, b.ihi, b.own_jlo, b.own_jhi});  // owned rows only
    }
  } else {
    for (int b = 0; b < nb; ++b) hb.insert(hb.end(), {2, nx - 1, 2, ny - 1});
  }
  t.blk.alloc(hb.size());
  t.blk.upload(hb.data(), c_->stream);
  t.hblk = hb;
  t.mrg_in.alloc(5 * nc); t.mrg_acc.alloc(20 * n2); t.fz_in.alloc(7 * n2);
  t.aicen.alloc(nc); t.trcrn.alloc(nc * NTRCR); t.vicen.alloc(nc); t.vsnon.alloc(nc);
  t.eicen.alloc(nc * NILYR); t.esnon.alloc(nc * NSLYR);
  for (DevBuf<double>* d : {&t.flw, &t.potT, &t.Qa, &t.rhoa, &t.fsnow, &t.fbot, &t.Tbot, &t.mlt_onset,
                            &t.frz_onset})
    d->alloc(n2);
  for (DevBuf<double>* d : {&t.lhcoef, &t.shcoef, &t.fswsfc, &t.fswint, &t.fswthrun}) d->alloc(nc);
  t.Sswabs.alloc(nc * NSLYR); t.Iswabs.alloc(nc * NILYR);
  t.out15.alloc(nc * 15);
  t.out15.zero(c_->stream);
  c_->tkey.alloc(THERMO_STATUS_WORDS);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

static void batch_upload(cice_ctx* c_, const cice_thermo_fields* h, bool with_fbot_tbot, bool with_coef = true) {
  auto& t = c_->tb;
  CICE_REQUIRE(t.nb > 0 && h, "cice_thermo_batch_alloc has not been called");
  struct U { DevBuf<double>* d; const double* h; };
  U us[] = {{&t.aicen, h->aicen}, {&t.trcrn, h->trcrn}, {&t.vicen, h->vicen}, {&t.vsnon, h->vsnon},
            {&t.eicen, h->eicen}, {&t.esnon, h->esnon}, {&t.flw, h->flw}, {&t.potT, h->potT},
            {&t.Qa, h->Qa}, {&t.rhoa, h->rhoa}, {&t.fsnow, h->fsnow}, {&t.fbot, h->fbot},
            {&t.Tbot, h->Tbot}, {&t.lhcoef, h->lhcoef}, {&t.shcoef, h->shcoef}, {&t.fswsfc, h->fswsfc},
            {&t.fswint, h->fswint}, {&t.fswthrun, h->fswthrun}, {&t.Sswabs, h->Sswabs},
            {&t.Iswabs, h->Iswabs}, {&t.mlt_onset, h->mlt_onset}, {&t.frz_onset, h->frz_onset}};
  for (U& x : us) {
    if (!with_fbot_tbot && (x.d == &t.fbot || x.d == &t.Tbot)) continue;   // produced on the device
    if (!with_coef && (x.d == &t.lhcoef || x.d == &t.shcoef)) continue;    // likewise (atmo_boundary_layer)
    CICE_REQUIRE(x.h != nullptr, "cice_thermo_batch_upload: NULL field");
    if (x.d == &t.trcrn && c_->have_thermo) {
      // of trcrn(nx, ny, max_ntrcr, ncat, nblocks) the column physics reads and writes the surface temperature only:
      // that plane of every (category, block), one strided copy (5 planes at ncat = 5 instead of 25)
      batch_tracer_copy(c_, c_->tp.nt_Tsfc - 1, x.h, t.trcrn.p, hipMemcpyHostToDevice);
      continue;
    }
    x.d->upload(x.h, c_->cs());
  }
  if (c_->have_thermo && !c_->tp.calc_Tsfc) {  // surface fluxes are inputs (ice_therm_vertical.F90:213-217)
    const size_t nc = (size_t)t.nx * t.ny * t.nb * NCAT;
    const double* in3[3] = {h->fsurfn, h->fcondtopn, h->flatn};
    const int plane[3] = {0, 1, 3};
    for (int k = 0; k < 3; ++k) {
      CICE_REQUIRE(in3[k] != nullptr, "cice_thermo_batch_upload: calc_Tsfc = F needs fsurfn, fcondtopn, flatn");
      CICE_HIP(hipMemcpyAsync(t.out15.p + (size_t)plane[k] * nc, in3[k], nc * 8, hipMemcpyHostToDevice, c_->cs()));
    }
  }
}

int cice_thermo_batch_upload(cice_ctx* ctx, const cice_thermo_fields* h) {
  CICE_TRY(ctx) c_->chain_ready = false;
  c_->tb.kept_aicen_init = false;
  batch_upload(c_, h, true);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

// number of columns updated: the sum of the kernel's counters (therm.h)
static long long status_count(const unsigned long long* h) {
  long long n = 0;
  for (int k = 0; k < THERMO_COUNT_SLOTS; ++k) n += (long long)h[THERMO_COUNT_STRIDE * (1 + k)];
  return n;
}

// launches the dense kernel; the status words (error key, update counters) land in `status` once the
// stream has been synchronised
static void batch_step(cice_ctx* c_, double dt, double yday, unsigned long long status[THERMO_STATUS_WORDS], float* elapsed_ms,
                       hipEvent_t* ev) {
  auto& t = c_->tb;
  CICE_REQUIRE(t.nb > 0, "cice_thermo_batch_alloc has not been called");
  CICE_REQUIRE(c_->have_thermo, "cice_thermo_init has not been called");
  hipStream_t s = c_->stream;
  const size_t nc = (size_t)t.nx * t.ny * t.nb * NCAT;
  thermo_status_reset(c_);
  ThermoArgs a = thermo_args(c_, t.nx, t.ny, NCAT, t.nb, dt, yday, [&](int name) -> double* {
    switch (name) {
      case A_AICEN: return t.aicen.p;   case A_TRCRN: return t.trcrn.p;     case A_VICEN: return t.vicen.p;
      case A_VSNON: return t.vsnon.p;   case A_EICEN: return t.eicen.p;     case A_ESNON: return t.esnon.p;
      case A_FLW: return t.flw.p;       case A_POTT: return t.potT.p;       case A_QA: return t.Qa.p;
      case A_RHOA: return t.rhoa.p;     case A_FSNOW: return t.fsnow.p;     case A_FBOT: return t.fbot.p;
      case A_TBOT: return t.Tbot.p;     case A_LH: return t.lhcoef.p;       case A_SH: return t.shcoef.p;
      case A_FSWSFC: return t.fswsfc.p; case A_FSWINT: return t.fswint.p;   case A_FSWTHRU: return t.fswthrun.p;
      case A_SSW: return t.Sswabs.p;    case A_ISW: return t.Iswabs.p;      case A_MLT: return t.mlt_onset.p;
      case A_FRZ: return t.frz_onset.p;
      default: return t.out15.p + (size_t)(name - A_OUT) * nc;   // A_OUT + k
    }
  });
  a.blk = t.blk.p;
  if (t.niter.n != nc) {
    t.niter.alloc(nc);
    t.niter.zero(s);
  }
  a.niter = t.niter.p;
  if (elapsed_ms) {
    CICE_HIP(hipEventCreate(&ev[0]));
    CICE_HIP(hipEventCreate(&ev[1]));
    CICE_HIP(hipEventRecord(ev[0], s));
  }
  static const int env_chunk = [] { const char* e = std::getenv("CICE4_AMD_THERMO_SORT"); return e ? std::atoi(e) : -1; }();
  const int chunk = env_chunk >= 0 ? env_chunk : t.sort_chunk;
  static const int env_group = [] { const char* e = std::getenv("CICE4_AMD_THERMO_GROUP"); return e ? std::atoi(e) : -1; }();
  const int group = env_group > 0 ? env_group : t.sort_group;
  if (chunk >= 256 && chunk <= 2048 && chunk % 256 == 0 && (group == 1 || group == 2 || group == 4 || group == 8 ||
                                                            group == 16 || group == 32)) {
    const size_t np = (size_t)t.nx * t.ny;
    const size_t want = thermo_sorted_plane(np, chunk) * t.nb * NCAT;
    if (t.perm.n != want) t.perm.alloc(want);
    // the Tsfc tracer plane of (category, block) cb: trcrn is (nx, ny, max_ntrcr, ncat, nb)
    thermo_launch_sorted(a, chunk, group, t.perm.p, t.trcrn.p + (size_t)(c_->tp.nt_Tsfc - 1) * np, (size_t)NTRCR * np, s);
  } else {
    thermo_launch_dense(a, s);
  }
  if (elapsed_ms) CICE_HIP(hipEventRecord(ev[1], s));
  CICE_HIP(hipMemcpyAsync(status, c_->tkey.p, THERMO_STATUS_WORDS * 8, hipMemcpyDeviceToHost, s));
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
  CICE_TRY(ctx)
  CICE_REQUIRE(key, "NULL key");
  if (!std::strcmp(key, "sort_chunk")) {
    CICE_REQUIRE(value == 0 || (value >= 256 && value <= 2048 && value % 256 == 0), "sort_chunk must be 0 or 256 .. 2048 in steps of 256");
    c_->tb.sort_chunk = value;
  } else if (!std::strcmp(key, "sort_group")) {
    CICE_REQUIRE(value == 1 || value == 2 || value == 4 || value == 8 || value == 16 || value == 32, "sort_group must be 1, 2, 4, 8, 16 or 32");
    c_->tb.sort_group = value;
  } else {
    throw Error{CICE_EINVAL, std::string("unknown option ") + key};
  }
  CICE_CATCH
}

int cice_thermo_batch_step(cice_ctx* ctx, double dt, double yday, long long* n_updates,
                           int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop,
                           int32_t* bstop, float* elapsed_ms) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(l_stop && istop && jstop, "NULL status pointer");
  unsigned long long h[THERMO_STATUS_WORDS];
  hipEvent_t ev[2] = {nullptr, nullptr};
  batch_step(c_, dt, yday, h, elapsed_ms, ev);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  if (elapsed_ms) {
    CICE_HIP(hipEventElapsedTime(elapsed_ms, ev[0], ev[1]));
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
  }
  if (n_updates) *n_updates = status_count(h);
  decode_err(h[0], c_->tb.nx, NCAT, nullptr, nullptr, l_stop, istop, jstop, nstop, bstop);
  CICE_CATCH
}

static void batch_download(cice_ctx* c_, cice_thermo_fields* h) {
  auto& t = c_->tb;
  CICE_REQUIRE(t.nb > 0 && h, "cice_thermo_batch_alloc has not been called");
  const size_t nc = (size_t)t.nx * t.ny * t.nb * NCAT;
  struct D { const DevBuf<double>* d; double* h; };
  D ds[] = {{&t.aicen, h->aicen}, {&t.trcrn, h->trcrn}, {&t.vicen, h->vicen}, {&t.vsnon, h->vsnon},
            {&t.eicen, h->eicen}, {&t.esnon, h->esnon}, {&t.fswsfc, h->fswsfc}, {&t.fswint, h->fswint},
            {&t.Sswabs, h->Sswabs}, {&t.Iswabs, h->Iswabs}, {&t.mlt_onset, h->mlt_onset},
            {&t.frz_onset, h->frz_onset}};
  for (D& x : ds) {
    if (!x.h) continue;
    if (x.d == &t.trcrn && c_->have_thermo) {   // the surface-temperature plane, as it was uploaded
      batch_tracer_copy(c_, c_->tp.nt_Tsfc - 1, t.trcrn.p, x.h, hipMemcpyDeviceToHost);
      continue;
    }
    x.d->download(x.h, c_->cs());
  }
  double* houts[15] = {h->fsurfn, h->fcondtopn, h->fsensn, h->flatn, h->fswabsn, h->flwoutn, h->evapn,
                       h->freshn, h->fsaltn, h->fhocnn, h->meltt, h->melts, h->meltb, h->congel,
                       h->snoice};
  for (int k = 0; k < 15; ++k)
    if (houts[k])
      CICE_HIP(hipMemcpyAsync(houts[k], t.out15.p + (size_t)k * nc, nc * 8, hipMemcpyDeviceToHost, c_->cs()));
}

int cice_thermo_batch_download(cice_ctx* ctx, cice_thermo_fields* h) {
  CICE_TRY(ctx) c_->chain_ready = false;
  batch_download(c_, h);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

// aicen_init_dev: device copy of the initial concentrations (cice_step_therm1 keeps one); otherwise
// f->aicen_init is uploaded
// phases: the uploads, the kernel and the downloads can be asked for separately (cice_step_therm1 puts its copies on
// side streams and the uploads in front of every kernel)
enum { MRG_UP = 1, MRG_RUN = 2, MRG_DOWN = 4, MRG_ALL = 7 };
static void batch_merge(cice_ctx* c_, const cice_merge_fields* f, const double* aicen_init_dev,
                        bool atmo_on_device = false, int phases = MRG_ALL) {
  auto& t = c_->tb;
  CICE_REQUIRE(t.nb > 0 && f, "cice_thermo_batch_alloc has not been called");
  hipStream_t s = c_->stream;
  const size_t n2 = (size_t)t.nx * t.ny * t.nb, nc = n2 * NCAT;
  DevBuf<double>&up = t.mrg_in, &acc = t.mrg_acc;
  const double* hin[5] = {f->aicen_init, f->strairxn, f->strairyn, f->Trefn, f->Qrefn};
  for (int k = 0; k < 5 && (phases & MRG_UP); ++k) {
    if (k == 0 && aicen_init_dev) continue;
    if (k > 0 && atmo_on_device) continue;    // strairxn, strairyn, Trefn, Qrefn were produced in place
    CICE_REQUIRE(hin[k] != nullptr, "cice_thermo_batch_merge: NULL input");
    CICE_HIP(hipMemcpyAsync(up.p + (size_t)k * nc, hin[k], nc * 8, hipMemcpyHostToDevice, c_->cs()));
  }
  for (int k = 0; k < 20 && (phases & MRG_UP); ++k) {
    CICE_REQUIRE(f->acc[k] != nullptr, "cice_thermo_batch_merge: NULL accumulator");
    CICE_HIP(hipMemcpyAsync(acc.p + (size_t)k * n2, f->acc[k], n2 * 8, hipMemcpyHostToDevice, c_->cs()));
  }
  MergeArgs a{};
  a.nx = t.nx; a.ny = t.ny; a.ncat = NCAT; a.nblocks = t.nb; a.blk = t.blk.p;
  a.aicen_init = aicen_init_dev ? aicen_init_dev : up.p; a.flw = t.flw.p;
  auto out = [&](int k) { return (const double*)(t.out15.p + (size_t)k * nc); };
  // out15 order: fsurfn fcondtopn fsensn flatn fswabsn flwoutn evapn freshn fsaltn fhocnn meltt melts
  //              meltb congel snoice
  const double* src[20] = {up.p + nc, up.p + 2 * nc, out(0), out(1), out(2), out(3), out(4), out(5),
                           out(6), up.p + 3 * nc, up.p + 4 * nc, out(7), out(8), out(9), t.fswthrun.p,
                           out(10), out(12), out(11), out(13), out(14)};
  for (int k = 0; k < 20; ++k) {
    a.src[k] = src[k];
    a.acc[k] = acc.p + (size_t)k * n2;
  }
  if (phases & MRG_RUN) merge_launch(a, s);
  for (int k = 0; k < 20 && (phases & MRG_DOWN); ++k)
    CICE_HIP(hipMemcpyAsync(f->acc[k], acc.p + (size_t)k * n2, n2 * 8, hipMemcpyDeviceToHost, c_->cs()));
}

int cice_thermo_batch_merge(cice_ctx* ctx, const cice_merge_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  batch_merge(c_, f, nullptr);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

// One call for the thermodynamic half of a time step on all local blocks (the work of step_therm1,
// drivers/cice4/CICE_RunMod.F90:260-598, minus atmo_boundary_layer, whose per-category outputs are inputs
// here): ONE upload, frzmlt_bottom_lateral (:363) -> thermo_vertical for every category (:502) ->
// merge_fluxes (:565) on the device, ONE download, one synchronisation.
static void step_therm1(cice_ctx* c_, double dt, double yday, cice_thermo_fields* st, const cice_frzmlt_fields* fz,
                        const cice_merge_fields* mg, const cice_atmo_fields* atm, long long* n_updates,
                        int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop) {
  auto& t = c_->tb;
  CICE_REQUIRE(t.nb > 0, "cice_thermo_batch_alloc has not been called");
  CICE_REQUIRE(c_->have_thermo, "cice_thermo_init has not been called");
  CICE_REQUIRE(st && fz && mg && l_stop && istop && jstop, "NULL argument");
  CICE_REQUIRE(fz->aice && fz->frzmlt && fz->sst && fz->Tf && fz->strocnxT && fz->strocnyT, "NULL frzmlt input");
  hipStream_t s = c_->stream;
  const size_t np = (size_t)t.nx * t.ny, n2 = np * t.nb, nc = n2 * NCAT;
  // every upload first, spread over the side streams (about 150 separate host arrays), then the kernels
  c_->fan.fork(s);
  batch_upload(c_, st, false, atm == nullptr);
  if (atm) {
    CICE_REQUIRE(atm->uatm && atm->vatm && atm->wind && atm->zlvl, "NULL atmosphere input");
    CICE_REQUIRE(atm->calc_strair || (atm->strax && atm->stray), "calc_strair = F needs strax, stray");
    if (t.atm_in.n < 6 * n2) t.atm_in.alloc(6 * n2);
    const double* ain[6] = {atm->uatm, atm->vatm, atm->wind, atm->zlvl, atm->strax, atm->stray};
    for (int k = 0; k < (atm->calc_strair ? 4 : 6); ++k)
      CICE_HIP(hipMemcpyAsync(t.atm_in.p + (size_t)k * n2, ain[k], n2 * 8, hipMemcpyHostToDevice, c_->cs()));
  }
  {
    const double* fin[6] = {fz->aice, fz->frzmlt, fz->sst, fz->Tf, fz->strocnxT, fz->strocnyT};
    for (int k = 0; k < 6; ++k)
      CICE_HIP(hipMemcpyAsync(t.fz_in.p + (size_t)k * n2, fin[k], n2 * 8, hipMemcpyHostToDevice, c_->cs()));
  }
  batch_merge(c_, mg, t.mrg_in.p, atm != nullptr, MRG_UP);
  c_->fan.join();
  if (atm) {   // atmo_boundary_layer for every category (CICE_RunMod.F90:402-425), on the state before the update
    AtmoArgs a{};
    a.p.init();
    a.nx = t.nx; a.ny = t.ny; a.ncat = NCAT; a.nblocks = t.nb; a.ocn = 0; a.calc_strair = atm->calc_strair != 0;
    a.blk = t.blk.p; a.aicen = t.aicen.p; a.Tsf = t.trcrn.p; a.it_Tsfc = c_->tp.nt_Tsfc - 1;
    a.potT = t.potT.p; a.Qa = t.Qa.p; a.rhoa = t.rhoa.p;
    a.uatm = t.atm_in.p; a.vatm = t.atm_in.p + n2; a.wind = t.atm_in.p + 2 * n2; a.zlvl = t.atm_in.p + 3 * n2;
    a.strax = t.atm_in.p + 4 * n2; a.stray = t.atm_in.p + 5 * n2;
    a.strx = t.mrg_in.p + nc; a.stry = t.mrg_in.p + 2 * nc; a.Tref = t.mrg_in.p + 3 * nc; a.Qref = t.mrg_in.p + 4 * nc;
    a.lhcoef = t.lhcoef.p; a.shcoef = t.shcoef.p;
    atmo_launch_dense(a, s);
  }
  for (int b = 0; b < t.nb; ++b) {   // frzmlt_bottom_lateral per block, on the uploaded enthalpies
    FrzmltArgs a{};
    a.nx = t.nx; a.ny = t.ny; a.dt = dt; a.ustar_min = c_->tp.ustar_min; a.chio = c_->chio;
    a.ilo = t.hblk[4 * b]; a.ihi = t.hblk[4 * b + 1]; a.jlo = t.hblk[4 * b + 2]; a.jhi = t.hblk[4 * b + 3];
    const size_t o = (size_t)b * np;
    a.aice = t.fz_in.p + o; a.frzmlt = t.fz_in.p + n2 + o; a.sst = t.fz_in.p + 2 * n2 + o;
    a.Tf = t.fz_in.p + 3 * n2 + o; a.strocnxT = t.fz_in.p + 4 * n2 + o; a.strocnyT = t.fz_in.p + 5 * n2 + o;
    a.Tbot = t.Tbot.p + o; a.fbot = t.fbot.p + o; a.rside = t.fz_in.p + 6 * n2 + o;
    a.eicen = t.eicen.p + (size_t)b * NCAT * NILYR * np; a.esnon = t.esnon.p + (size_t)b * NCAT * NSLYR * np;
    frzmlt_launch(a, s);
  }
  // aicen_init of merge_fluxes = the concentrations before the column update (CICE_RunMod.F90:342-355)
  CICE_HIP(hipMemcpyAsync(t.mrg_in.p, t.aicen.p, nc * 8, hipMemcpyDeviceToDevice, s));
  t.kept_aicen_init = true;
  unsigned long long h[THERMO_STATUS_WORDS];
  batch_step(c_, dt, yday, h, nullptr, nullptr);
  batch_merge(c_, mg, t.mrg_in.p, atm != nullptr, MRG_RUN);
  c_->fan.fork(s);   // ... and every download after the last kernel
  batch_merge(c_, mg, t.mrg_in.p, atm != nullptr, MRG_DOWN);
  batch_download(c_, st);
  if (atm) {
    double* aout[6] = {atm->strairxn, atm->strairyn, atm->Trefn, atm->Qrefn, atm->lhcoef, atm->shcoef};
    const double* asrc[6] = {t.mrg_in.p + nc, t.mrg_in.p + 2 * nc, t.mrg_in.p + 3 * nc, t.mrg_in.p + 4 * nc,
                             t.lhcoef.p, t.shcoef.p};
    for (int k = 0; k < 6; ++k)
      if (aout[k]) CICE_HIP(hipMemcpyAsync(aout[k], asrc[k], nc * 8, hipMemcpyDeviceToHost, c_->cs()));
  }
  if (fz->Tbot) t.Tbot.download(fz->Tbot, c_->cs());
  if (fz->fbot) t.fbot.download(fz->fbot, c_->cs());
  if (fz->rside) CICE_HIP(hipMemcpyAsync(fz->rside, t.fz_in.p + 6 * n2, n2 * 8, hipMemcpyDeviceToHost, c_->cs()));
  c_->fan.join();
  CICE_HIP(hipStreamSynchronize(s));
  if (n_updates) *n_updates = status_count(h);
  decode_err(h[0], t.nx, NCAT, nullptr, nullptr, l_stop, istop, jstop, nstop, bstop);
}

int cice_step_therm1(cice_ctx* ctx, double dt, double yday, cice_thermo_fields* st,
                     const cice_frzmlt_fields* fz, const cice_merge_fields* mg, long long* n_updates,
                     int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  step_therm1(c_, dt, yday, st, fz, mg, nullptr, n_updates, l_stop, istop, jstop, nstop, bstop);
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
  step_therm1(c_, dt, yday, st, fz, mg, atm, n_updates, l_stop, istop, jstop, nstop, bstop);
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
