// cice::ColumnBatch (batch.h) and the two decoders it shares with the block-wise entries.
#include "batch.h"

namespace cice {

void decode_err(unsigned long long key, int nx, int ncat, const int32_t* indxi, const int32_t* indxj, int32_t* l_stop,
                int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop) {
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

unsigned long long itd_shift_key(const unsigned long long* r, int N) {
  const int stale = (int)(r[ITD_REC_LASTDONOR] & 7) - N;   // 0 / 1: the donor of the last cell with donor > 0 is N / N + 1
  for (int k = 0; k < 4; ++k) {
    if (!r[ITD_REC_FLAG + k]) continue;
    unsigned long long key = 0;
    if (k < 2 && (stale == 0 || stale == 1)) key = r[(k == 0 ? ITD_REC_NEG_DA : ITD_REC_NEG_DV) + stale];
    if (k == 2) key = r[ITD_REC_GT_DA];
    if (k == 3) key = r[ITD_REC_GT_DV];
    if (key) return key;
  }
  for (int k = 0; k < 4; ++k)
    if (r[ITD_REC_FLAG + k]) return r[ITD_REC_FLAG + k];
  return 0;
}

ColumnBatch::~ColumnBatch() {
  for (hipEvent_t e : clean_ev_)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ridge_ev_)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ho_ev_)
    if (e) (void)hipEventDestroy(e);
}

// Every field of cice_thermo_fields, once, in the order the fields travel: what alloc sizes, upload and download move
// and launch_step hands to the kernel.  The exceptions are the callers': of trcrn only the surface-temperature plane
// travels, fbot / Tbot and lhcoef / shcoef stay behind when they are produced on the device, and the three surface
// fluxes travel in (F_FLUX_UP, behind everything else) with calc_Tsfc = F only.
std::vector<ColumnBatch::Field> ColumnBatch::fields(const cice_thermo_fields* h) {
  static const cice_thermo_fields none{};
  const cice_thermo_fields& f = h ? *h : none;
  const size_t C = NCAT;
  std::vector<Field> v = {
      {A_AICEN, &aicen_, 0, f.aicen, C, F_IO}, {A_TRCRN, &trcrn_, 0, f.trcrn, C * NTRCR, F_IO},
      {A_VICEN, &vicen_, 0, f.vicen, C, F_IO}, {A_VSNON, &vsnon_, 0, f.vsnon, C, F_IO},
      {A_EICEN, &eicen_, 0, f.eicen, C * NILYR, F_IO}, {A_ESNON, &esnon_, 0, f.esnon, C * NSLYR, F_IO},
      {A_FLW, &flw_, 0, f.flw, 1, F_UP}, {A_POTT, &potT_, 0, f.potT, 1, F_UP}, {A_QA, &Qa_, 0, f.Qa, 1, F_UP},
      {A_RHOA, &rhoa_, 0, f.rhoa, 1, F_UP}, {A_FSNOW, &fsnow_, 0, f.fsnow, 1, F_UP}, {A_FBOT, &fbot_, 0, f.fbot, 1, F_UP},
      {A_TBOT, &Tbot_, 0, f.Tbot, 1, F_UP}, {A_LH, &lhcoef_, 0, f.lhcoef, C, F_UP}, {A_SH, &shcoef_, 0, f.shcoef, C, F_UP},
      {A_FSWSFC, &fswsfc_, 0, f.fswsfc, C, F_IO}, {A_FSWINT, &fswint_, 0, f.fswint, C, F_IO},
      {A_FSWTHRU, &fswthrun_, 0, f.fswthrun, C, F_UP}, {A_SSW, &Sswabs_, 0, f.Sswabs, C * NSLYR, F_IO},
      {A_ISW, &Iswabs_, 0, f.Iswabs, C * NILYR, F_IO}, {A_MLT, &mlt_onset_, 0, f.mlt_onset, 1, F_IO},
      {A_FRZ, &frz_onset_, 0, f.frz_onset, 1, F_IO}};
  const double* outs[15] = {f.fsurfn, f.fcondtopn, f.fsensn, f.flatn, f.fswabsn, f.flwoutn, f.evapn, f.freshn,
                            f.fsaltn, f.fhocnn, f.meltt, f.melts, f.meltb, f.congel, f.snoice};
  for (int k = 0; k < 15; ++k) v.push_back({A_OUT + k, &out15_, k, outs[k], C, F_DOWN | (k < 2 || k == 3 ? F_FLUX_UP : 0)});
  return v;
}

void ColumnBatch::alloc(hipStream_t stream, CopyFan& fan, int nx, int ny, int nb, const Domain* dom) {
  stream_ = stream; fan_ = &fan;
  nx_ = nx; ny_ = ny; nb_ = nb;
  kept_aicen_init_ = false;
  therm2_state_ = false;
  therm1_state_ = false;
  pond_armed_ = false;
  forget_sw();
  alb_scheme_ = ALB_NONE;
  const size_t np = (size_t)nx * ny, n2 = np * nb, nc = n2 * NCAT;
  std::vector<int32_t> hb;
  if (dom && same_layout(*dom)) {
    for (int gid : dom->local) {
      const Block& b = dom->all[gid];
      hb.insert(hb.end(), {b.ilo, b.ihi, b.own_jlo, b.own_jhi});  // owned rows only
    }
  } else {
    for (int b = 0; b < nb; ++b) hb.insert(hb.end(), {2, nx - 1, 2, ny - 1});
  }
  blk_.alloc(hb.size());
  blk_.upload(hb.data(), stream_);
  hblk_ = hb;
  mrg_in_.alloc(5 * nc); mrg_acc_.alloc(20 * n2); fz_in_.alloc(7 * n2);
  // (the order of the allocations as it has always been: the state, the fields per cell, the fields per category)
  for (int group = 0; group < 3; ++group)
    for (const Field& x : fields(nullptr))
      if (x.d != &out15_ && group == (x.name < A_FLW ? 0 : x.per == 1 ? 1 : 2)) x.d->alloc(n2 * x.per);
  out15_.alloc(nc * 15);
  out15_.zero(stream_);
  key_.alloc(THERMO_STATUS_WORDS);
  CICE_HIP(hipStreamSynchronize(stream_));
}

// Plane `it` of trcrn(nx, ny, max_ntrcr, ncat, nblocks) for every (category, block), one strided copy between the caller's
// array and the batch's; `from` and `to` are the two arrays' first elements
void ColumnBatch::tracer_copy(int it, const double* from, double* to, hipMemcpyKind kind) {
  const size_t np = (size_t)nx_ * ny_, o = (size_t)it * np, pitch = (size_t)NTRCR * np * 8;
  CICE_HIP(hipMemcpy2DAsync(to + o, pitch, from + o, pitch, np * 8, (size_t)NCAT * nb_, kind, cs()));
}

void ColumnBatch::move_state(const HostState& h, int members, int t0, int t1, hipMemcpyKind kind) {
  const bool up = kind == hipMemcpyHostToDevice;
  const size_t bytes = (size_t)nx_ * ny_ * nb_ * 8;
  const struct { int member; const double* h; double* d; size_t per; } arr[5] = {
      {ST_AICEN, h.aicen, aicen_.p, NCAT}, {ST_VICEN, h.vicen, vicen_.p, NCAT}, {ST_VSNON, h.vsnon, vsnon_.p, NCAT},
      {ST_EICEN, h.eicen, eicen_.p, NCAT * NILYR}, {ST_ESNON, h.esnon, esnon_.p, NCAT * NSLYR}};
  for (const auto& x : arr)
    if (members & x.member)
      CICE_HIP(hipMemcpyAsync(up ? x.d : const_cast<double*>(x.h), up ? x.h : x.d, bytes * x.per, kind, cs()));
  for (int it = t0; it < t1; ++it)
    tracer_copy(it, up ? h.trcrn : trcrn_.p, up ? trcrn_.p : const_cast<double*>(h.trcrn), kind);
}

void ColumnBatch::move_sw(const SwArrays& h, hipMemcpyKind kind) {
  DevBuf<double>* const d[5] = {&fswsfc_, &fswint_, &fswthrun_, &Sswabs_, &Iswabs_};
  for (int k = 0; k < 5; ++k)
    if (kind == hipMemcpyHostToDevice) d[k]->upload(h.h[k], cs());
    else d[k]->download(h.h[k], cs());
}

void ColumnBatch::zero_sw(hipStream_t s) {
  fswsfc_.zero(s); fswint_.zero(s); fswthrun_.zero(s); Sswabs_.zero(s); Iswabs_.zero(s);
}

void ColumnBatch::upload_fields(const ThermoParams* tp, const cice_thermo_fields* h, bool with_fbot_tbot, bool with_coef,
                                bool with_sw) {
  const size_t n2 = (size_t)nx_ * ny_ * nb_;
  const std::vector<Field> fs = fields(h);
  for (const Field& x : fs) {
    if (!(x.dir & F_UP)) continue;
    if (!with_fbot_tbot && (x.name == A_FBOT || x.name == A_TBOT)) continue;   // produced on the device
    if (!with_coef && (x.name == A_LH || x.name == A_SH)) continue;            // likewise (atmo_boundary_layer)
    if (!with_sw && (x.name == A_FSWSFC || x.name == A_FSWINT || x.name == A_FSWTHRU || x.name == A_SSW || x.name == A_ISW))
      continue;                                                                // left there by the radiation stage
    CICE_REQUIRE(x.h != nullptr, "cice_thermo_batch_upload: NULL field");
    if (x.name == A_TRCRN && tp) {
      // of trcrn(nx, ny, max_ntrcr, ncat, nblocks) the column physics reads and writes the surface temperature only:
      // that plane of every (category, block), one strided copy (5 planes at ncat = 5 instead of 25)
      tracer_copy(tp->nt_Tsfc - 1, x.h, trcrn_.p, hipMemcpyHostToDevice);
      continue;
    }
    x.d->upload(x.h, cs());
  }
  for (const Field& x : fs) {
    if (!(x.dir & F_FLUX_UP) || !tp || tp->calc_Tsfc) continue;  // surface fluxes are inputs (ice_therm_vertical.F90:213-217)
    CICE_REQUIRE(x.h != nullptr, "cice_thermo_batch_upload: calc_Tsfc = F needs fsurfn, fcondtopn, flatn");
    CICE_HIP(hipMemcpyAsync(x.d->p + x.k * n2 * x.per, x.h, n2 * x.per * 8, hipMemcpyHostToDevice, cs()));
  }
}

void ColumnBatch::upload(const ThermoParams* tp, const cice_thermo_fields* h) {
  kept_aicen_init_ = false;
  therm2_state_ = false;
  therm1_state_ = false;
  forget_sw();
  upload_fields(tp, h, true, true);
  CICE_HIP(hipStreamSynchronize(stream_));
}

// launches the dense kernel; the status words (error key, update counters) land in `status` once the
// stream has been synchronised, and the clock holds the kernel's events
void ColumnBatch::launch_step(const ThermoParams& tp, double dt, double yday, unsigned long long status[THERMO_STATUS_WORDS],
                              StageClock<1>& clock) {
  hipStream_t s = stream_;
  const size_t n2 = (size_t)nx_ * ny_ * nb_, nc = n2 * NCAT;
  thermo_status_reset(key_.p, s);
  const std::vector<Field> fs = fields(nullptr);
  ThermoArgs a = thermo_args(tp, key_.p, nx_, ny_, NCAT, nb_, dt, yday, [&](int name) -> double* {
    for (const Field& x : fs)
      if (x.name == name) return x.d->p + x.k * n2 * x.per;
    return nullptr;
  });
  a.blk = blk_.p;
  if (niter_.n != nc) {
    niter_.alloc(nc);
    niter_.zero(s);
  }
  a.niter = niter_.p;
  clock.mark(0, s);
  static const int env_chunk = [] { const char* e = std::getenv("CICE4_AMD_THERMO_SORT"); return e ? std::atoi(e) : -1; }();
  const int chunk = env_chunk >= 0 ? env_chunk : sort_chunk_;
  static const int env_group = [] { const char* e = std::getenv("CICE4_AMD_THERMO_GROUP"); return e ? std::atoi(e) : -1; }();
  const int group = env_group > 0 ? env_group : sort_group_;
  if (chunk >= 256 && chunk <= 2048 && chunk % 256 == 0 && (group == 1 || group == 2 || group == 4 || group == 8 ||
                                                            group == 16 || group == 32)) {
    const size_t np = (size_t)nx_ * ny_;
    const size_t want = thermo_sorted_plane(np, chunk) * nb_ * NCAT;
    if (perm_.n != want) perm_.alloc(want);
    // the Tsfc tracer plane of (category, block) cb: trcrn is (nx, ny, max_ntrcr, ncat, nb)
    thermo_launch_sorted(a, chunk, group, perm_.p, trcrn_.p + (size_t)(tp.nt_Tsfc - 1) * np, (size_t)NTRCR * np, s);
  } else {
    thermo_launch_dense(a, s);
  }
  clock.mark(1, s);
  CICE_HIP(hipMemcpyAsync(status, key_.p, THERMO_STATUS_WORDS * 8, hipMemcpyDeviceToHost, s));
}

void ColumnBatch::set_option(const char* key, int value) {
  if (!std::strcmp(key, "sort_chunk")) {
    CICE_REQUIRE(value == 0 || (value >= 256 && value <= 2048 && value % 256 == 0), "sort_chunk must be 0 or 256 .. 2048 in steps of 256");
    sort_chunk_ = value;
  } else if (!std::strcmp(key, "sort_group")) {
    CICE_REQUIRE(value == 1 || value == 2 || value == 4 || value == 8 || value == 16 || value == 32, "sort_group must be 1, 2, 4, 8, 16 or 32");
    sort_group_ = value;
  } else {
    throw Error{CICE_EINVAL, std::string("unknown option ") + key};
  }
}

void ColumnBatch::step(const ThermoParams* tp, double dt, double yday, long long* n_updates, int32_t* l_stop, int32_t* istop,
                       int32_t* jstop, int32_t* nstop, int32_t* bstop, float* elapsed_ms) {
  CICE_REQUIRE(tp, "cice_thermo_init has not been called");
  therm2_state_ = false;
  therm1_state_ = false;
  forget_sw();                         // the column update writes the shortwave buffers
  unsigned long long h[THERMO_STATUS_WORDS];
  StageClock<1> clock;                 // of this call: no events without elapsed_ms
  clock.on = elapsed_ms != nullptr;
  launch_step(*tp, dt, yday, h, clock);
  CICE_HIP(hipStreamSynchronize(stream_));
  clock.read(0, 1);
  if (elapsed_ms) *elapsed_ms = clock.ms[0];
  if (n_updates) *n_updates = status_count(h);
  decode_err(h[0], nx_, NCAT, nullptr, nullptr, l_stop, istop, jstop, nstop, bstop);
}

void ColumnBatch::download_fields(const ThermoParams* tp, cice_thermo_fields* h) {
  const size_t n2 = (size_t)nx_ * ny_ * nb_;
  for (const Field& x : fields(h)) {
    if (!(x.dir & F_DOWN) || !x.h) continue;
    double* to = const_cast<double*>(x.h);   // (the fields that travel back are the struct's non-const members)
    if (x.name == A_TRCRN && tp)             // the surface-temperature plane, as it was uploaded
      tracer_copy(tp->nt_Tsfc - 1, trcrn_.p, to, hipMemcpyDeviceToHost);
    else
      CICE_HIP(hipMemcpyAsync(to, x.d->p + x.k * n2 * x.per, n2 * x.per * 8, hipMemcpyDeviceToHost, cs()));
  }
}

void ColumnBatch::download(const ThermoParams* tp, cice_thermo_fields* h) {
  download_fields(tp, h);
  CICE_HIP(hipStreamSynchronize(stream_));
}

// aicen_init_dev: device copy of the initial concentrations (step_therm1 keeps one); otherwise f->aicen_init is uploaded
// phases: the uploads, the kernel and the downloads can be asked for separately (step_therm1 puts its copies on
// side streams and the uploads in front of every kernel)
void ColumnBatch::merge_phases(const cice_merge_fields* f, const double* aicen_init_dev, bool atmo_on_device, int phases) {
  hipStream_t s = stream_;
  const size_t n2 = (size_t)nx_ * ny_ * nb_, nc = n2 * NCAT;
  DevBuf<double>&up = mrg_in_, &acc = mrg_acc_;
  const double* hin[5] = {f->aicen_init, f->strairxn, f->strairyn, f->Trefn, f->Qrefn};
  for (int k = 0; k < 5 && (phases & MRG_UP); ++k) {
    if (k == 0 && aicen_init_dev) continue;
    if (k > 0 && atmo_on_device) continue;    // strairxn, strairyn, Trefn, Qrefn were produced in place
    CICE_REQUIRE(hin[k] != nullptr, "cice_thermo_batch_merge: NULL input");
    CICE_HIP(hipMemcpyAsync(up.p + (size_t)k * nc, hin[k], nc * 8, hipMemcpyHostToDevice, cs()));
  }
  for (int k = 0; k < 20 && (phases & MRG_UP); ++k) {
    CICE_REQUIRE(f->acc[k] != nullptr, "cice_thermo_batch_merge: NULL accumulator");
    CICE_HIP(hipMemcpyAsync(acc.p + (size_t)k * n2, f->acc[k], n2 * 8, hipMemcpyHostToDevice, cs()));
  }
  MergeArgs a{};
  a.nx = nx_; a.ny = ny_; a.ncat = NCAT; a.nblocks = nb_; a.blk = blk_.p;
  a.aicen_init = aicen_init_dev ? aicen_init_dev : up.p; a.flw = flw_.p;
  auto out = [&](int k) { return (const double*)(out15_.p + (size_t)k * nc); };
  // out15 order: fsurfn fcondtopn fsensn flatn fswabsn flwoutn evapn freshn fsaltn fhocnn meltt melts
  //              meltb congel snoice
  const double* src[20] = {up.p + nc, up.p + 2 * nc, out(0), out(1), out(2), out(3), out(4), out(5),
                           out(6), up.p + 3 * nc, up.p + 4 * nc, out(7), out(8), out(9), fswthrun_.p,
                           out(10), out(12), out(11), out(13), out(14)};
  for (int k = 0; k < 20; ++k) {
    a.src[k] = src[k];
    a.acc[k] = acc.p + (size_t)k * n2;
  }
  if (phases & MRG_RUN) merge_launch(a, s);
  for (int k = 0; k < 20 && (phases & MRG_DOWN); ++k)
    CICE_HIP(hipMemcpyAsync(f->acc[k], acc.p + (size_t)k * n2, n2 * 8, hipMemcpyDeviceToHost, cs()));
}

void ColumnBatch::merge(const cice_merge_fields* f) {
  merge_phases(f, nullptr, false, MRG_ALL);
  CICE_HIP(hipStreamSynchronize(stream_));
}

// One call for the thermodynamic half of a time step on all local blocks (the work of step_therm1,
// drivers/cice4/CICE_RunMod.F90:260-598; atmo_boundary_layer too where `atm` is given, else its per-category outputs
// are inputs here): ONE upload, frzmlt_bottom_lateral (:363) -> thermo_vertical for every category (:502) ->
// merge_fluxes (:565) on the device, ONE download, one synchronisation.
void ColumnBatch::step_therm1(const ThermoParams* tp, double chio, double dt, double yday, cice_thermo_fields* st,
                              const cice_frzmlt_fields* fz, const cice_merge_fields* mg, const cice_atmo_fields* atm,
                              long long* n_updates, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop,
                              int32_t* bstop) {
  CICE_REQUIRE(tp, "cice_thermo_init has not been called");
  CICE_REQUIRE(st && fz && mg && l_stop && istop && jstop, "NULL argument");
  CICE_REQUIRE(fz->aice && fz->frzmlt && fz->sst && fz->Tf && fz->strocnxT && fz->strocnyT, "NULL frzmlt input");
  hipStream_t s = stream_;
  therm2_state_ = false;
  therm1_state_ = false;
  // cice_radiation_chain: the five shortwave arrays are on the device already if they are the host arrays the radiation
  // stage downloaded to; consumed or not, the record ends here (the column update writes those buffers)
  const bool sw_kept = sw_armed_ && st->fswsfc == sw_host_[0] && st->fswint == sw_host_[1] && st->fswthrun == sw_host_[2] &&
                       st->Sswabs == sw_host_[3] && st->Iswabs == sw_host_[4];
  forget_sw();
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  // every upload first, spread over the side streams (about 150 separate host arrays), then the kernels
  fan_->fork(s);
  upload_fields(tp, st, false, atm == nullptr, !sw_kept);
  if (atm) {
    CICE_REQUIRE(atm->uatm && atm->vatm && atm->wind && atm->zlvl, "NULL atmosphere input");
    CICE_REQUIRE(atm->calc_strair || (atm->strax && atm->stray), "calc_strair = F needs strax, stray");
    if (atm_in_.n < 6 * n2) atm_in_.alloc(6 * n2);
    const double* ain[6] = {atm->uatm, atm->vatm, atm->wind, atm->zlvl, atm->strax, atm->stray};
    for (int k = 0; k < (atm->calc_strair ? 4 : 6); ++k)
      CICE_HIP(hipMemcpyAsync(atm_in_.p + (size_t)k * n2, ain[k], n2 * 8, hipMemcpyHostToDevice, cs()));
  }
  {
    const double* fin[6] = {fz->aice, fz->frzmlt, fz->sst, fz->Tf, fz->strocnxT, fz->strocnyT};
    for (int k = 0; k < 6; ++k)
      CICE_HIP(hipMemcpyAsync(fz_in_.p + (size_t)k * n2, fin[k], n2 * 8, hipMemcpyHostToDevice, cs()));
  }
  merge_phases(mg, mrg_in_.p, atm != nullptr, MRG_UP);
  fan_->join();
  if (atm) {   // atmo_boundary_layer for every category (CICE_RunMod.F90:402-425), on the state before the update
    AtmoArgs a{};
    a.p.init();
    a.nx = nx_; a.ny = ny_; a.ncat = NCAT; a.nblocks = nb_; a.ocn = 0; a.calc_strair = atm->calc_strair != 0;
    a.blk = blk_.p; a.aicen = aicen_.p; a.Tsf = trcrn_.p; a.it_Tsfc = tp->nt_Tsfc - 1;
    a.potT = potT_.p; a.Qa = Qa_.p; a.rhoa = rhoa_.p;
    a.uatm = atm_in_.p; a.vatm = atm_in_.p + n2; a.wind = atm_in_.p + 2 * n2; a.zlvl = atm_in_.p + 3 * n2;
    a.strax = atm_in_.p + 4 * n2; a.stray = atm_in_.p + 5 * n2;
    a.strx = mrg_in_.p + nc; a.stry = mrg_in_.p + 2 * nc; a.Tref = mrg_in_.p + 3 * nc; a.Qref = mrg_in_.p + 4 * nc;
    a.lhcoef = lhcoef_.p; a.shcoef = shcoef_.p;
    atmo_launch_dense(a, s);
  }
  for (int b = 0; b < nb_; ++b) {   // frzmlt_bottom_lateral per block, on the uploaded enthalpies
    FrzmltArgs a{};
    a.nx = nx_; a.ny = ny_; a.dt = dt; a.ustar_min = tp->ustar_min; a.chio = chio;
    a.ilo = hblk_[4 * b]; a.ihi = hblk_[4 * b + 1]; a.jlo = hblk_[4 * b + 2]; a.jhi = hblk_[4 * b + 3];
    const size_t o = (size_t)b * np;
    a.aice = fz_in_.p + o; a.frzmlt = fz_in_.p + n2 + o; a.sst = fz_in_.p + 2 * n2 + o;
    a.Tf = fz_in_.p + 3 * n2 + o; a.strocnxT = fz_in_.p + 4 * n2 + o; a.strocnyT = fz_in_.p + 5 * n2 + o;
    a.Tbot = Tbot_.p + o; a.fbot = fbot_.p + o; a.rside = fz_in_.p + 6 * n2 + o;
    a.eicen = eicen_.p + (size_t)b * NCAT * NILYR * np; a.esnon = esnon_.p + (size_t)b * NCAT * NSLYR * np;
    frzmlt_launch(a, s);
  }
  // aicen_init of merge_fluxes = the concentrations before the column update (CICE_RunMod.F90:342-355)
  CICE_HIP(hipMemcpyAsync(mrg_in_.p, aicen_.p, nc * 8, hipMemcpyDeviceToDevice, s));
  kept_aicen_init_ = true;
  unsigned long long h[THERMO_STATUS_WORDS];
  StageClock<1> untimed;
  launch_step(*tp, dt, yday, h, untimed);
  merge_phases(mg, mrg_in_.p, atm != nullptr, MRG_RUN);
  fan_->fork(s);   // ... and every download after the last kernel
  merge_phases(mg, mrg_in_.p, atm != nullptr, MRG_DOWN);
  download_fields(tp, st);
  if (atm) {
    double* aout[6] = {atm->strairxn, atm->strairyn, atm->Trefn, atm->Qrefn, atm->lhcoef, atm->shcoef};
    const double* asrc[6] = {mrg_in_.p + nc, mrg_in_.p + 2 * nc, mrg_in_.p + 3 * nc, mrg_in_.p + 4 * nc,
                             lhcoef_.p, shcoef_.p};
    for (int k = 0; k < 6; ++k)
      if (aout[k]) CICE_HIP(hipMemcpyAsync(aout[k], asrc[k], nc * 8, hipMemcpyDeviceToHost, cs()));
  }
  if (fz->Tbot) Tbot_.download(fz->Tbot, cs());
  if (fz->fbot) fbot_.download(fz->fbot, cs());
  if (fz->rside) CICE_HIP(hipMemcpyAsync(fz->rside, fz_in_.p + 6 * n2, n2 * 8, hipMemcpyDeviceToHost, cs()));
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  if (n_updates) *n_updates = status_count(h);
  decode_err(h[0], nx_, NCAT, nullptr, nullptr, l_stop, istop, jstop, nstop, bstop);
  therm1_state_ = !*l_stop;            // the updated state and the per-category melt are on the device (step_ponds)
}

// the record words once the stream has run dry
void ColumnBatch::read_rec(unsigned long long h[ITD_REC_WORDS]) {
  CICE_HIP(hipMemcpyAsync(h, rec_.p, ITD_REC_WORDS * 8, hipMemcpyDeviceToHost, stream_));
  CICE_HIP(hipStreamSynchronize(stream_));
}

// The thickness-distribution stage on the batch (ice_step_mod.F90:286-422): see include/cice4_amd.h
void ColumnBatch::step_therm2_itd(const ThermoParams* tp, const ItdParams* ip, double dt, double yday,
                                  const cice_therm2_fields* f, int32_t* l_stop, int32_t* istop, int32_t* jstop,
                                  int32_t* bstop, int32_t* stage) {
  CICE_REQUIRE(ip, "cice_itd_init has not been called");
  CICE_REQUIRE(dt > 0.0, "dt");
  CICE_REQUIRE(f->aicen && f->trcrn && f->vicen && f->vsnon && f->eicen && f->esnon && f->vicen_init && f->frain &&
                   f->frzmlt && f->Tf && f->rside && f->tmask && f->aice && f->aice0 && f->fresh && f->fsalt && f->fhocn &&
                   f->frazil && f->meltl && f->frz_onset, "cice_step_therm2_itd: NULL field");
  const bool resident = f->state_resident != 0;
  CICE_REQUIRE(resident || f->aicen_init, "cice_step_therm2_itd: aicen_init is needed without a resident state");
  CICE_REQUIRE(!resident || (tp && tp->nt_Tsfc - 1 == ip->it_Tsfc),
               "cice_step_therm2_itd: state_resident needs cice_thermo_init with the same nt_Tsfc");
  CICE_REQUIRE(f->aicen_init || kept_aicen_init_,
               "cice_step_therm2_itd: aicen_init = NULL needs a cice_step_therm1 call on this batch in front");
  hipStream_t s = stream_;
  therm2_state_ = false;
  therm1_state_ = false;
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  if (itd_b_.n < 2 * nc + 12 * n2) itd_b_.alloc(2 * nc + 12 * n2);
  if (itd_bi_.n < n2 + (size_t)nb_) itd_bi_.alloc(n2 + (size_t)nb_);
  rec_.alloc(ITD_REC_WORDS);
  double* ainit = itd_b_.p;
  double* vinit = itd_b_.p + nc;
  double* d2 = itd_b_.p + 2 * nc;
  int32_t* flag = itd_bi_.p + n2;
  const int ntr = ip->ntrcr, it_T = ip->it_Tsfc;
  const HostState hs{f->aicen, f->vicen, f->vsnon, f->eicen, f->esnon, f->trcrn};
  auto upload = [&](bool state) {      // (a resident state: the tracer planes but the surface temperature's)
    fan_->fork(s);
    move_state(hs, state ? ST_ALL : 0, 0, state ? ntr : it_T, hipMemcpyHostToDevice);
    if (!state) move_state(hs, 0, it_T + 1, ntr, hipMemcpyHostToDevice);
    if (f->aicen_init) CICE_HIP(hipMemcpyAsync(ainit, f->aicen_init, nc * 8, hipMemcpyHostToDevice, cs()));
    CICE_HIP(hipMemcpyAsync(vinit, f->vicen_init, nc * 8, hipMemcpyHostToDevice, cs()));
    const double* in2[12] = {f->aice, f->aice0, f->frain, f->frzmlt, f->Tf, f->rside, f->fresh, f->fsalt, f->fhocn,
                             nullptr, f->meltl, f->frz_onset};
    for (int k = 0; k < 12; ++k)
      if (in2[k]) CICE_HIP(hipMemcpyAsync(d2 + (size_t)k * n2, in2[k], n2 * 8, hipMemcpyHostToDevice, cs()));
    CICE_HIP(hipMemcpyAsync(itd_bi_.p, f->tmask, n2 * 4, hipMemcpyHostToDevice, cs()));
    fan_->join();
    CICE_HIP(hipMemsetAsync(d2 + (size_t)I2_FRAZIL * n2, 0, n2 * 8, s));
    CICE_HIP(hipMemsetAsync(rec_.p, 0, ITD_REC_WORDS * 8, s));
    CICE_HIP(hipMemsetAsync(flag, 0, (size_t)nb_ * 4, s));
  };
  ItdArgs a{};
  a.p = *ip;
  a.nx = nx_; a.ny = ny_; a.nblocks = nb_; a.blk = blk_.p; a.kitd = f->kitd != 0; a.dt = dt; a.yday = yday;
  a.blockflag = flag; a.blockflag_out = flag; a.tmask = itd_bi_.p;
  a.aicen = aicen_.p; a.trcrn = trcrn_.p; a.vicen = vicen_.p; a.vsnon = vsnon_.p; a.eicen = eicen_.p;
  a.esnon = esnon_.p; a.vicen_init = vinit;
  a.aicen_init = f->aicen_init ? ainit : mrg_in_.p;   // NULL: the concentrations step_therm1 kept for merge_fluxes
  a.aice = d2 + I2_AICE * n2; a.aice0 = d2 + I2_AICE0 * n2; a.frain = d2 + I2_FRAIN * n2; a.frzmlt = d2 + I2_FRZMLT * n2;
  a.Tf = d2 + I2_TF * n2; a.rside = d2 + I2_RSIDE * n2; a.fresh = d2 + I2_FRESH * n2; a.fsalt = d2 + I2_FSALT * n2;
  a.fhocn = d2 + I2_FHOCN * n2; a.frazil = d2 + I2_FRAZIL * n2; a.meltl = d2 + I2_MELTL * n2;
  a.frz_onset = d2 + I2_FRZ_ONSET * n2;
  a.rec = rec_.p;
  auto run = [&](int bfail, int nlimit, int bend_add, int bend_melt) {
    ItdArgs k = a;
    k.bfail = bfail; k.nlimit = nlimit;
    itd_clock_.mark(0, s);
    itd_launch_rain_aggregate(k, s);
    itd_clock_.mark(1, s);
    if (k.kitd) itd_launch_linear(k, s);
    itd_clock_.mark(2, s);
    k.bend = bend_add;
    itd_launch_add_new_ice(k, s);
    itd_clock_.mark(3, s);
    k.bend = bend_melt;
    itd_launch_lateral_melt(k, s);
    itd_clock_.mark(4, s);
  };
  unsigned long long r[ITD_REC_WORDS];
  upload(!resident);
  run(nb_, 0, nb_, nb_);
  read_rec(r);
  itd_clock_.read(0, 4);
  clear_stop(l_stop, istop, jstop);
  *bstop = 0; *stage = 0;
  int bl = -1, N = 0, ba = -1;
  if (r[ITD_REC_SHIFT]) {
    const unsigned long long v = r[ITD_REC_SHIFT] - 1;
    bl = nb_ - 1 - (int)(v >> 8);
    N = NCAT - (int)(v & 0xff);
  }
  if (r[ITD_REC_ADD]) ba = nb_ - 1 - (int)(r[ITD_REC_ADD] >> 32);
  if (bl >= 0 || ba >= 0) {            // a stop: again from the caller's arrays, up to where the reference stops (itd.h)
    const bool in_shift = bl >= 0 && (ba < 0 || bl <= ba);
    const int bf = in_shift ? bl : ba;
    upload(true);
    run(bf, in_shift ? N : 0, in_shift ? bf : bf + 1, bf);
    read_rec(r);
    unsigned long long key = in_shift ? itd_shift_key(r, N) : (r[ITD_REC_ADD] & 0xffffffffull);
    *l_stop = 1; *bstop = bf + 1; *stage = in_shift ? 1 : 2;
    if (key) { *istop = (int32_t)((key - 1) % nx_) + 1; *jstop = (int32_t)((key - 1) / nx_) + 1; }
  }
  fan_->fork(s);
  move_state(hs, ST_ALL, 0, ntr, hipMemcpyDeviceToHost);
  double* out2[12] = {f->aice, f->aice0, nullptr, nullptr, nullptr, nullptr, f->fresh, f->fsalt, f->fhocn, f->frazil,
                      f->meltl, f->frz_onset};
  for (int k = 0; k < 12; ++k)
    if (out2[k]) CICE_HIP(hipMemcpyAsync(out2[k], d2 + (size_t)k * n2, n2 * 8, hipMemcpyDeviceToHost, cs()));
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  therm2_state_ = !*l_stop;            // the state with all its tracer planes is on the device (step_therm2_cleanup)
}

// The second half of step_therm2 on the batch (ice_step_mod.F90:445-511): see include/cice4_amd.h and cleanup.h
void ColumnBatch::step_therm2_cleanup(const ItdParams* ip, double dt, const cice_therm2_cleanup_fields* f, Halo* halo,
                                      int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage) {
  column_stages(ip, dt, f, nullptr, halo, l_stop, istop, jstop, bstop, stage);
}

// The column half of step_dynamics on the batch (ice_step_mod.F90:586-745): ridge_ice in front of the same three stages
void ColumnBatch::step_ridge(const ItdParams* ip, const RidgeParams* rp, double dt, const cice_ridge_fields* f,
                             Transport* from, Halo* halo, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop,
                             int32_t* stage) {
  CICE_REQUIRE(rp, "cice_ridge_init has not been called");
  CICE_REQUIRE(f->rdg_conv && f->rdg_shear && f->dardg1dt && f->dardg2dt && f->dvirdgdt && f->opening,
               "cice_step_ridge: NULL field");
  cice_therm2_cleanup_fields c{};
  c.ncat = f->ncat; c.state_resident = 0; c.bound = f->bound;
  c.aicen = f->aicen; c.trcrn = f->trcrn; c.vicen = f->vicen; c.vsnon = f->vsnon; c.eicen = f->eicen; c.esnon = f->esnon;
  c.tmask = f->tmask;
  c.aice = f->aice; c.aice0 = f->aice0; c.vice = f->vice; c.vsno = f->vsno; c.eice = f->eice; c.esno = f->esno;
  c.trcr = f->trcr;
  c.fresh = f->fresh; c.fsalt = f->fsalt; c.fhocn = f->fhocn; c.daidtt = f->daidtd; c.dvidtt = f->dvidtd;
  const RidgeStage rs{rp, f->rdg_conv, f->rdg_shear, f->dardg1dt, f->dardg2dt, f->dvirdgdt, f->opening, from};
  column_stages(ip, dt, &c, &rs, halo, l_stop, istop, jstop, bstop, stage);
}

// cleanup_itd, bound_state, aggregate and the tendencies on the batch; with `rs`, ridge_ice (ridge.h) in front of them as
// stage 1 on the physical tmask cells of every block that has one, and the numbers of the other stages one up
void ColumnBatch::column_stages(const ItdParams* ip, double dt, const cice_therm2_cleanup_fields* f, const RidgeStage* rs,
                                Halo* halo, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop,
                                int32_t* stage) {
  CICE_REQUIRE(ip, "cice_itd_init has not been called");
  CICE_REQUIRE(dt > 0.0, "dt");
  CICE_REQUIRE(f->aicen && f->trcrn && f->vicen && f->vsnon && f->eicen && f->esnon && f->tmask && f->aice && f->aice0 &&
                   f->vice && f->vsno && f->eice && f->esno && f->trcr && f->fresh && f->fsalt && f->fhocn && f->daidtt &&
                   f->dvidtt, "cice_step_therm2_cleanup: NULL field");
  const bool resident = f->state_resident != 0;
  CICE_REQUIRE(!resident || therm2_state_,
               "cice_step_therm2_cleanup: state_resident needs a cice_step_therm2_itd call on this batch in front");
  hipStream_t s = stream_;
  therm2_state_ = false;
  therm1_state_ = false;
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_;
  const int ntr = ip->ntrcr;
  enum { C_AICE = 0, C_AICE0, C_VICE, C_VSNO, C_EICE, C_ESNO, C_FRESH, C_FSALT, C_FHOCN, C_DAIDTT, C_DVIDTT, C_TRCR,
         C_PLANES = C_TRCR + NTRCR };
  if (clean_b_.n < C_PLANES * n2) clean_b_.alloc(C_PLANES * n2);
  if (clean_bi_.n < n2) clean_bi_.alloc(n2);
  clean_w_.alloc((size_t)nb_ * CW_WORDS);
  const bool timed = clean_timed_;
  for (hipEvent_t& e : clean_ev_)
    if (timed && !e) CICE_HIP(hipEventCreate(&e));
  auto d2 = [&](int k) { return clean_b_.p + (size_t)k * n2; };
  // the state: resident from step_therm2_itd, handed over by the transport on the device (below), or uploaded
  Transport* const from = rs ? rs->from : nullptr;
  const bool late = from && from->download_deferred();   // the host arrays have not seen the transport's result
  fan_->fork(s);
  if (!resident && !from) {
    aicen_.upload(f->aicen, cs()); vicen_.upload(f->vicen, cs()); vsnon_.upload(f->vsnon, cs());
    eicen_.upload(f->eicen, cs()); esnon_.upload(f->esnon, cs());
    for (int it = 0; it < ntr; ++it) tracer_copy(it, f->trcrn, trcrn_.p, hipMemcpyHostToDevice);
  }
  {
    const double* in2[5] = {f->fresh, f->fsalt, f->fhocn, f->daidtt, f->dvidtt};
    for (int k = 0; k < 5; ++k) CICE_HIP(hipMemcpyAsync(d2(C_FRESH + k), in2[k], n2 * 8, hipMemcpyHostToDevice, cs()));
    CICE_HIP(hipMemcpyAsync(clean_bi_.p, f->tmask, n2 * 4, hipMemcpyHostToDevice, cs()));
  }
  enum { R_CONV = RG_PLANES, R_SHEAR, R_D1, R_D2, R_DV, R_OPEN, R_PLANES };
  auto dr = [&](int k) { return ridge_b_.p + (size_t)k * n2; };
  if (rs) {                            // ridge_ice reads aice0; its diagnostics keep what they held off the list
    if (ridge_b_.n < R_PLANES * n2) ridge_b_.alloc(R_PLANES * n2);
    if (ridge_bi_.n < n2) ridge_bi_.alloc(n2);
    ridge_w_.alloc((size_t)nb_ * RW_WORDS);
    const double* in[7] = {rs->rdg_conv, rs->rdg_shear, rs->dardg1dt, rs->dardg2dt, rs->dvirdgdt, rs->opening, f->aice0};
    for (int k = 0; k < 6; ++k) CICE_HIP(hipMemcpyAsync(dr(R_CONV + k), in[k], n2 * 8, hipMemcpyHostToDevice, cs()));
    if (!from) CICE_HIP(hipMemcpyAsync(d2(C_AICE0), in[6], n2 * 8, hipMemcpyHostToDevice, cs()));
  }
  fan_->join();
  if (from) {                          // one launch instead of the uploads of the seven arrays (handover.h)
    const double* src[HO_ARRAYS];
    from->state_buffers(src);
    double* dst[HO_ARRAYS] = {d2(C_AICE0), aicen_.p, vicen_.p, vsnon_.p, eicen_.p, esnon_.p, trcrn_.p};
    for (hipEvent_t& e : ho_ev_)
      if (ho_timed_ && !e) CICE_HIP(hipEventCreate(&e));
    if (ho_timed_) CICE_HIP(hipEventRecord(ho_ev_[0], s));
    handover_launch(handover_args(nx_, ny_, nb_, ntr, src, dst), s);
    if (ho_timed_) CICE_HIP(hipEventRecord(ho_ev_[1], s));
    ho_pending_ = ho_timed_;
  }
  clear_stop(l_stop, istop, jstop);
  *bstop = 0; *stage = 0;
  const int s0 = rs ? 1 : 0;           // what the stage numbers of the cleanup are shifted by
  // the blocks 0 .. b of the state and of the named planes: what a stop in block b hands back
  // (late: the blocks behind b "come back as they went in" from the transport's buffers -- everything it holds goes to the
  // host arrays first, all blocks, aice0 included, and the blocks 0 .. b of this call's result on top of that)
  auto part_state = [&](int b) {
    const size_t m = (size_t)b + 1;
    auto part = [&](double* h, const double* d, size_t per) {
      CICE_HIP(hipMemcpyAsync(h, d, m * per * np * 8, hipMemcpyDeviceToHost, cs()));
    };
    part(f->aicen, aicen_.p, NCAT); part(f->vicen, vicen_.p, NCAT); part(f->vsnon, vsnon_.p, NCAT);
    part(f->eicen, eicen_.p, NCAT * NILYR); part(f->esnon, esnon_.p, NCAT * NSLYR);
    for (int it = 0; it < ntr; ++it)
      CICE_HIP(hipMemcpy2DAsync(f->trcrn + (size_t)it * np, (size_t)NTRCR * np * 8, trcrn_.p + (size_t)it * np,
                                (size_t)NTRCR * np * 8, np * 8, (size_t)NCAT * m, hipMemcpyDeviceToHost, cs()));
  };
  auto late_state = [&] {
    if (!late) return;
    const cice_transport_fields t{f->aice0, f->aicen, f->trcrn, f->vicen, f->vsnon, f->eicen, f->esnon, nullptr, nullptr};
    from->download_state(t);
  };
  if (rs) {
    CICE_HIP(hipMemsetAsync(ridge_w_.p, 0, ridge_w_.n * 8, s));
    ridge_launch_list(ridge_bi_.p, clean_bi_.p, blk_.p, nx_, ny_, nb_, s);
    RidgeArgs r{};
    r.p = *ip; r.r = *rs->rp;
    r.nx = nx_; r.ny = ny_; r.nblocks = nb_; r.listpos = ridge_bi_.p; r.dt = dt;
    r.rdg_conv = dr(R_CONV); r.rdg_shear = dr(R_SHEAR);
    r.aicen = aicen_.p; r.trcrn = trcrn_.p; r.vicen = vicen_.p; r.vsnon = vsnon_.p; r.eicen = eicen_.p; r.esnon = esnon_.p;
    r.aice0 = d2(C_AICE0);
    r.dardg1dt = dr(R_D1); r.dardg2dt = dr(R_D2); r.dvirdgdt = dr(R_DV); r.opening = dr(R_OPEN);
    r.fresh = d2(C_FRESH); r.fhocn = d2(C_FHOCN);
    r.work = dr(0); r.bw = ridge_w_.p;
    const bool rtimed = ridge_timed_;
    for (hipEvent_t& e : ridge_ev_)
      if (rtimed && !e) CICE_HIP(hipEventCreate(&e));
    for (float& x : ridge_ms_) x = 0.0f;
    std::vector<unsigned long long> rw((size_t)nb_ * RW_WORDS);
    for (int done = 0;;) {
      const int count = std::min<int>(RIDGE_QUEUE, RIDGE_NITERMAX - done);
      ridge_launch_iterations(r, done + 1, count, s, rtimed ? ridge_ev_ : nullptr);
      CICE_HIP(hipMemcpyAsync(rw.data(), ridge_w_.p, rw.size() * 8, hipMemcpyDeviceToHost, s));
      CICE_HIP(hipStreamSynchronize(s));
      for (int k = 0; k < 2 * count && rtimed; ++k)
        CICE_HIP(hipEventElapsedTime(&ridge_ms_[2 * done + k], ridge_ev_[k], ridge_ev_[k + 1]));
      done += count;
      bool more = false;
      for (int b = 0; b < nb_; ++b) more = more || ridge_wants_more(rw.data() + (size_t)b * RW_WORDS, done);
      if (!more) break;
    }
    if (rtimed) CICE_HIP(hipEventRecord(ridge_ev_[0], s));
    ridge_launch_finish(r, s);         // (leaves a stopped block alone)
    if (rtimed) {
      CICE_HIP(hipEventRecord(ridge_ev_[1], s));
      CICE_HIP(hipStreamSynchronize(s));
      CICE_HIP(hipEventElapsedTime(&ridge_ms_[RIDGE_TIMES - 1], ridge_ev_[0], ridge_ev_[1]));
    }
    for (int b = 0; b < nb_; ++b) {
      unsigned pos = 0;
      int n_it = 0;
      if (!ridge_decode(rw.data() + (size_t)b * RW_WORDS, &pos, &n_it)) continue;
      // the failing block as ridge_ice leaves it, the blocks in front of it ridged, the blocks behind it as they went in
      *l_stop = 1; *stage = 1; *bstop = b + 1;
      if (pos) { *istop = (int32_t)((pos - 1) % nx_) + 1; *jstop = (int32_t)((pos - 1) / nx_) + 1; }
      const size_t m = (size_t)b + 1;
      late_state();
      fan_->fork(s);
      part_state(b);
      double* h[7] = {rs->dardg1dt, rs->dardg2dt, rs->dvirdgdt, rs->opening, f->aice0, f->fresh, f->fhocn};
      const double* d[7] = {dr(R_D1), dr(R_D2), dr(R_DV), dr(R_OPEN), d2(C_AICE0), d2(C_FRESH), d2(C_FHOCN)};
      for (int k = 0; k < 7; ++k) CICE_HIP(hipMemcpyAsync(h[k], d[k], m * np * 8, hipMemcpyDeviceToHost, cs()));
      fan_->join();
      CICE_HIP(hipStreamSynchronize(s));
      return;
    }
  }
  CICE_HIP(hipMemsetAsync(clean_w_.p, 0, clean_w_.n * 8, s));
  CleanArgs a{};
  a.p = *ip;
  a.nx = nx_; a.ny = ny_; a.nblocks = nb_; a.blk = blk_.p; a.limit_aice = 1; a.dt = dt;
  a.aicen = aicen_.p; a.trcrn = trcrn_.p; a.vicen = vicen_.p; a.vsnon = vsnon_.p; a.eicen = eicen_.p; a.esnon = esnon_.p;
  a.aice = d2(C_AICE); a.aice0 = d2(C_AICE0); a.fresh = d2(C_FRESH); a.fsalt = d2(C_FSALT); a.fhocn = d2(C_FHOCN);
  a.bw = clean_w_.p; a.tmask = clean_bi_.p;
  a.vice = d2(C_VICE); a.vsno = d2(C_VSNO); a.eice = d2(C_EICE); a.esno = d2(C_ESNO); a.trcr = d2(C_TRCR);
  a.daidtt = d2(C_DAIDTT); a.dvidtt = d2(C_DVIDTT);
  // stage 1: cleanup_itd on every block
  clean_launch_all(a, s, timed ? clean_ev_ : nullptr);
  std::vector<unsigned long long> w((size_t)nb_ * CW_WORDS);
  CICE_HIP(hipMemcpyAsync(w.data(), clean_w_.p, w.size() * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));
  for (int b = 0; b < nb_; ++b) {
    size_t q = 0;
    if (!clean_decode(w.data() + (size_t)b * CW_WORDS, np, &q)) continue;
    // the failing block as cleanup_itd leaves it, the blocks in front of it cleaned, the blocks behind it as they went in
    *l_stop = 1; *stage = 1 + s0; *bstop = b + 1;
    *istop = (int32_t)(q % nx_) + 1; *jstop = (int32_t)(q / nx_) + 1;
    const size_t m = (size_t)b + 1;
    late_state();
    fan_->fork(s);
    part_state(b);
    double* h[3] = {f->fresh, f->fsalt, f->fhocn};
    for (int k = 0; k < 3; ++k) CICE_HIP(hipMemcpyAsync(h[k], d2(C_FRESH + k), m * np * 8, hipMemcpyDeviceToHost, cs()));
    fan_->join();
    CICE_HIP(hipStreamSynchronize(s));
    return;
  }
  // stage 2: bound_state (ice_state.F90:162-217), the six updates of the transport on the batch's arrays.  The Halo
  // addresses a level's blocks together, the batch keeps a block's levels together: with more than one block an array
  // is turned over into clean_t_ and back.
  if (halo) {
    struct { DevBuf<double>* d; int levels; } arr[6] = {{&aicen_, NCAT}, {&trcrn_, NCAT * NTRCR}, {&vicen_, NCAT},
                                                        {&vsnon_, NCAT}, {&eicen_, NCAT * NILYR}, {&esnon_, NCAT * NSLYR}};
    if (nb_ > 1 && clean_t_.n < (size_t)NCAT * NTRCR * n2) clean_t_.alloc((size_t)NCAT * NTRCR * n2);
    for (const auto& x : arr) {
      double* base = x.d->p;
      if (nb_ > 1) {
        clean_launch_transpose(x.d->p, clean_t_.p, np, x.levels, nb_, true, s);
        base = clean_t_.p;
      }
      if (x.d == &trcrn_) {
        for (int c = 0; c < NCAT; ++c)   // trcrn(:,:,1:ntrcr,:,:) only (:206)
          halo->update_r8(base + (size_t)c * NTRCR * n2, ntr, n2, true, LOC_CENTER, KIND_SCALAR);
      } else {
        halo->update_r8(base, x.levels, n2, true, LOC_CENTER, KIND_SCALAR);
      }
      if (nb_ > 1) clean_launch_transpose(clean_t_.p, x.d->p, np, x.levels, nb_, false, s);
    }
  }
  if (timed) CICE_HIP(hipEventRecord(clean_ev_[CLEAN_TIMES - 1], s));
  // stage 3: aggregate and the tendencies
  clean_launch_aggregate(a, s);
  if (timed) CICE_HIP(hipEventRecord(clean_ev_[CLEAN_TIMES], s));
  fan_->fork(s);
  aicen_.download(f->aicen, cs()); vicen_.download(f->vicen, cs()); vsnon_.download(f->vsnon, cs());
  eicen_.download(f->eicen, cs()); esnon_.download(f->esnon, cs());
  for (int it = 0; it < ntr; ++it) {
    tracer_copy(it, trcrn_.p, f->trcrn, hipMemcpyDeviceToHost);
    CICE_HIP(hipMemcpy2DAsync(f->trcr + (size_t)it * np, (size_t)NTRCR * np * 8, d2(C_TRCR) + (size_t)it * np,
                              (size_t)NTRCR * np * 8, np * 8, (size_t)nb_, hipMemcpyDeviceToHost, cs()));
  }
  double* out2[11] = {f->aice, f->aice0, f->vice, f->vsno, f->eice, f->esno, f->fresh, f->fsalt, f->fhocn, f->daidtt,
                      f->dvidtt};
  for (int k = 0; k < 11; ++k) CICE_HIP(hipMemcpyAsync(out2[k], d2(k), n2 * 8, hipMemcpyDeviceToHost, cs()));
  if (rs) {
    double* h[4] = {rs->dardg1dt, rs->dardg2dt, rs->dvirdgdt, rs->opening};
    for (int k = 0; k < 4; ++k) CICE_HIP(hipMemcpyAsync(h[k], dr(R_D1 + k), n2 * 8, hipMemcpyDeviceToHost, cs()));
  }
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < CLEAN_TIMES && timed; ++k) CICE_HIP(hipEventElapsedTime(&clean_ms_[k], clean_ev_[k], clean_ev_[k + 1]));
  therm2_state_ = true;
}

void ColumnBatch::keep_sw(const SwArrays& h) {
  sw_resident_ = true;
  sw_armed_ = rad_mode_ == 1;
  for (int k = 0; k < 5; ++k) sw_host_[k] = h.h[k];
}

// step_radiation (ice_step_mod.F90:764-973) on the batch with the scheme `r` describes: see include/cice4_amd.h
template <class Launch>
void ColumnBatch::radiation_stage(const ThermoParams& tp, const RadScheme& r, Launch launch) {
  auto text = [&](const char* what) { return std::string(r.entry) + ": " + what; };
  CICE_REQUIRE(r.state_resident == 0 || r.state_resident == 1, text("state_resident must be 0 or 1"));
  const bool resident = r.state_resident == 1;
  CICE_REQUIRE(!resident || therm2_state_,
               text("state_resident needs a cice_step_ridge or cice_step_therm2_cleanup on this batch in front"));
  CICE_REQUIRE(resident || (r.state.aicen && r.state.trcrn && r.state.vicen && r.state.vsnon), text("NULL state"));
  bool outputs = true, forcing = true;
  for (int k = 0; k < r.nout; ++k) outputs = outputs && r.out[k];
  for (double* h : r.sw.h) outputs = outputs && h;
  CICE_REQUIRE(outputs, text("NULL output"));
  hipStream_t s = stream_;
  if (r.forget_first) forget_sw();
  alb_scheme_ = ALB_NONE;              // (a call that fails, or zero-fills, leaves no set of albedos to merge)
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  if (r.buf->n != r.planes2 * n2 + r.planesc * nc) r.buf->alloc(r.planes2 * n2 + r.planesc * nc);
  double* const p2 = r.buf->p;
  double* const pc = p2 + r.planes2 * n2;
  if (!tp.calc_Tsfc) {                 // "initialize for safety" (:946-967): the four albedos and the five; nothing else is touched
    forget_sw();
    CICE_HIP(hipMemsetAsync(pc, 0, 4 * nc * 8, s));
    zero_sw(s);
    fan_->fork(s);
    for (int k = 0; k < 4; ++k) CICE_HIP(hipMemcpyAsync(r.out[k], pc + k * nc, nc * 8, hipMemcpyDeviceToHost, cs()));
    move_sw(r.sw, hipMemcpyDeviceToHost);
    fan_->join();
    CICE_HIP(hipStreamSynchronize(s));
    keep_sw(r.sw);
    return;
  }
  for (const auto& x : r.in2) forcing = forcing && (x.h || x.may_be_null);
  CICE_REQUIRE(forcing, text("NULL forcing"));
  CICE_REQUIRE(!r.pond || (r.pondn[0] && r.pondn[1]), text("tr_pond needs apondn and hpondn"));
  forget_sw();
  fan_->fork(s);
  if (!resident) {                     // of the state the scheme reads these four; the rest of the batch's state is stale now
    therm2_state_ = false;
    therm1_state_ = false;
    move_state(r.state, ST_AICEN | ST_VICEN | ST_VSNON, tp.nt_Tsfc - 1, tp.nt_Tsfc, hipMemcpyHostToDevice);
  }
  for (int k = 0; k < 5; ++k)
    if (r.in2[k].h) CICE_HIP(hipMemcpyAsync(p2 + k * n2, r.in2[k].h, n2 * 8, hipMemcpyHostToDevice, cs()));
  for (int k = 0; k < 2 && r.pond; ++k)
    if (r.pond_dev[k])                 // cice_pond_chain: the pond stage's device copy is the host array's
      CICE_HIP(hipMemcpyAsync(pc + (r.nout + k) * nc, r.pond_dev[k], nc * 8, hipMemcpyDeviceToDevice, cs()));
    else
      CICE_HIP(hipMemcpyAsync(pc + (r.nout + k) * nc, r.pondn[k], nc * 8, hipMemcpyHostToDevice, cs()));
  fan_->join();
  r.clock->mark(0, s);
  launch(p2, pc);
  r.clock->mark(1, s);
  fan_->fork(s);
  for (int k = 0; k < r.nout; ++k) CICE_HIP(hipMemcpyAsync(r.out[k], pc + k * nc, nc * 8, hipMemcpyDeviceToHost, cs()));
  move_sw(r.sw, hipMemcpyDeviceToHost);
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  r.clock->read(0, 1);
  for (size_t q = 0; q < n2 && r.coszen_out; ++q) r.coszen_out[q] = K::p5;   // "sun above the horizon" (:843), every cell
  keep_sw(r.sw);
  alb_scheme_ = r.buf == &rad_b_ ? ALB_CCSM3 : ALB_DEDD;
}

// what ShortwaveArgs and DeddArgs have in common: the batch's state and shortwave buffers, the four shortwave fields from
// plane `sw` of p2 on, the six albedo outputs they share at the head of pc
template <class Args>
void ColumnBatch::radiation_args(Args& a, const ThermoParams& tp, double* p2, int sw, double* pc) {
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  a.nx = nx_; a.np = (int)np; a.ncat = NCAT; a.nb = nb_; a.tsfc_planes = NTRCR;
  a.blk = blk_.p;
  a.aicen = aicen_.p; a.vicen = vicen_.p; a.vsnon = vsnon_.p; a.Tsfc = trcrn_.p + (size_t)(tp.nt_Tsfc - 1) * np;
  a.swvdr = p2 + sw * n2; a.swvdf = p2 + (sw + 1) * n2; a.swidr = p2 + (sw + 2) * n2; a.swidf = p2 + (sw + 3) * n2;
  a.alvdrn = pc; a.alidrn = pc + nc; a.alvdfn = pc + 2 * nc; a.alidfn = pc + 3 * nc; a.albicen = pc + 4 * nc; a.albsnon = pc + 5 * nc;
  a.fswsfcn = fswsfc_.p; a.fswintn = fswint_.p; a.fswthrun = fswthrun_.p; a.Iswabsn = Iswabs_.p; a.Sswabsn = Sswabs_.p;
}

// planes of rad_b_: the 2-d fields (nx, ny, nb each), then six (nx, ny, ncat, nb) arrays -- step_radiation's albedo outputs;
// prep_radiation keeps its copy of aicen in the first of them
enum { R_SWVDR = 0, R_SWVDF, R_SWIDR, R_SWIDF, R_OCN, R_GBM, R_AICE = R_GBM + 4, R_SF, R_FAC, R_2D };

// shortwave = 'default': coszen is an output, 0.5 everywhere
void ColumnBatch::step_radiation(const ThermoParams* tp, const ShortwaveParams* sp, const cice_radiation_fields* f) {
  CICE_REQUIRE(tp, "cice_thermo_init has not been called");
  CICE_REQUIRE(sp, "cice_shortwave_init has not been called");
  const RadScheme r{"cice_step_radiation", f->state_resident, {f->aicen, f->vicen, f->vsnon, nullptr, nullptr, f->trcrn},
                    &rad_b_, R_2D, 6, {{f->swvdr}, {f->swvdf}, {f->swidr}, {f->swidf}, {f->ocn_albedo, true}}, false, {}, {}, 6,
                    {f->alvdrn, f->alidrn, f->alvdfn, f->alidfn, f->albicen, f->albsnon},
                    {{f->fswsfcn, f->fswintn, f->fswthrun, f->Sswabsn, f->Iswabsn}}, &sw_clock_, true, f->coszen};
  radiation_stage(*tp, r, [&](double* p2, double* pc) {
    ShortwaveArgs a{};
    a.p = *sp;
    radiation_args(a, *tp, p2, R_SWVDR, pc);
    a.ocn_albedo = f->ocn_albedo ? p2 + R_OCN * ((size_t)nx_ * ny_ * nb_) : nullptr;
    shortwave_launch(a, stream_);
  });
}

// prep_radiation (ice_step_mod.F90:84-218) on the batch: see include/cice4_amd.h
void ColumnBatch::prep_radiation(const ThermoParams* tp, const cice_prep_radiation_fields* f) {
  CICE_REQUIRE(tp, "cice_thermo_init has not been called");
  CICE_REQUIRE(f->sw_resident == 0 || f->sw_resident == 1, "cice_prep_radiation: sw_resident must be 0 or 1");
  const bool resident = f->sw_resident == 1;
  CICE_REQUIRE(!resident || sw_resident_,
               "cice_prep_radiation: sw_resident needs a cice_step_radiation on this batch in front");
  CICE_REQUIRE(f->fswsfcn && f->fswintn && f->fswthrun && f->Sswabsn && f->Iswabsn, "cice_prep_radiation: NULL field");
  hipStream_t s = stream_;
  forget_sw();
  if (alb_scheme_ == ALB_CCSM3) alb_scheme_ = ALB_NONE;   // (aicen is staged in the first albedo plane)
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  if (rad_b_.n != R_2D * n2 + 6 * nc) rad_b_.alloc(R_2D * n2 + 6 * nc);
  auto d2 = [&](int k) { return rad_b_.p + (size_t)k * n2; };
  double* const daicen = rad_b_.p + R_2D * n2;
  const SwArrays sw{{f->fswsfcn, f->fswintn, f->fswthrun, f->Sswabsn, f->Iswabsn}};
  if (!tp->calc_Tsfc) {                // "initialize for safety" (:195-212)
    zero_sw(s);
    fan_->fork(s);
    move_sw(sw, hipMemcpyDeviceToHost);
    fan_->join();
    CICE_HIP(hipStreamSynchronize(s));
    keep_sw(sw);
    return;
  }
  CICE_REQUIRE(f->swvdr && f->swvdf && f->swidr && f->swidf && f->alvdr_gbm && f->alvdf_gbm && f->alidr_gbm &&
                   f->alidf_gbm && f->aice && f->scale_factor && f->fswfac && f->aicen, "cice_prep_radiation: NULL field");
  fan_->fork(s);
  const double* in2[10] = {f->swvdr, f->swvdf, f->swidr, f->swidf, nullptr, f->alvdr_gbm, f->alvdf_gbm, f->alidr_gbm,
                           f->alidf_gbm, f->aice};
  static_assert(R_AICE == 9 && R_SF == 10 && R_FAC == 11, "order of in2");
  for (int k = 0; k < 10; ++k)
    if (in2[k]) CICE_HIP(hipMemcpyAsync(d2(k), in2[k], n2 * 8, hipMemcpyHostToDevice, cs()));
  CICE_HIP(hipMemcpyAsync(d2(R_SF), f->scale_factor, n2 * 8, hipMemcpyHostToDevice, cs()));
  CICE_HIP(hipMemcpyAsync(d2(R_FAC), f->fswfac, n2 * 8, hipMemcpyHostToDevice, cs()));   // (kept off the physical cells)
  CICE_HIP(hipMemcpyAsync(daicen, f->aicen, nc * 8, hipMemcpyHostToDevice, cs()));
  if (!resident) move_sw(sw, hipMemcpyHostToDevice);
  fan_->join();
  PrepRadiationArgs a{};
  a.nx = nx_; a.np = (int)np; a.ncat = NCAT; a.nb = nb_; a.blk = blk_.p;
  a.swvdr = d2(R_SWVDR); a.swvdf = d2(R_SWVDF); a.swidr = d2(R_SWIDR); a.swidf = d2(R_SWIDF);
  a.alvdr_gbm = d2(R_GBM); a.alvdf_gbm = d2(R_GBM + 1); a.alidr_gbm = d2(R_GBM + 2); a.alidf_gbm = d2(R_GBM + 3);
  a.aice = d2(R_AICE); a.aicen = daicen; a.scale_factor = d2(R_SF); a.fswfac = d2(R_FAC);
  a.fswsfcn = fswsfc_.p; a.fswintn = fswint_.p; a.fswthrun = fswthrun_.p; a.Sswabsn = Sswabs_.p; a.Iswabsn = Iswabs_.p;
  prep_clock_.mark(0, s);
  prep_radiation_launch(a, s);
  prep_clock_.mark(1, s);
  fan_->fork(s);
  CICE_HIP(hipMemcpyAsync(f->scale_factor, d2(R_SF), n2 * 8, hipMemcpyDeviceToHost, cs()));
  CICE_HIP(hipMemcpyAsync(f->fswfac, d2(R_FAC), n2 * 8, hipMemcpyDeviceToHost, cs()));
  move_sw(sw, hipMemcpyDeviceToHost);
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  prep_clock_.read(0, 1);
  keep_sw(sw);
}

// planes of pond_b_ ((nx, ny, ncat, nb) each; behind them frain, (nx, ny, nb)): the two tracers, the pond fraction and depth,
// and what state_resident = 0 uploads
enum { P_VOLPN = 0, P_IAGE, P_APOND, P_HPOND, P_AICEN, P_VICEN, P_VSNON, P_TSFC, P_MELTT, P_MELTS, P_PLANES };

// planes of dedd_b_: coszen and the four sw fields (nx, ny, nb each), then nine (nx, ny, ncat, nb) arrays -- the four
// albedos, albicen, albsnon, albpndn, and the inputs apondn, hpondn
enum { D_COSZEN = 0, D_SWVDR, D_SWVDF, D_SWIDR, D_SWIDF, D_2D };

// shortwave = 'dEdd': coszen is an input; a call refused for its forcing or its pond arrays leaves the record of the
// shortwave buffers standing
void ColumnBatch::step_radiation_dedd(const ThermoParams* tp, const DeddParams* dp, const cice_radiation_dedd_fields* f) {
  CICE_REQUIRE(tp, "cice_thermo_init has not been called");
  CICE_REQUIRE(dp, "cice_shortwave_dedd_init has not been called");
  // cice_pond_chain: apondn and hpondn are on the device already if they are the host arrays the pond stage downloaded to
  const bool chained = pond_armed_ && dp->tr_pond && f->apondn == pond_host_[0] && f->hpondn == pond_host_[1];
  const size_t ncp = (size_t)nx_ * ny_ * nb_ * NCAT;
  const RadScheme r{"cice_step_radiation_dedd", f->state_resident, {f->aicen, f->vicen, f->vsnon, nullptr, nullptr, f->trcrn},
                    &dedd_b_, D_2D, 9, {{f->coszen}, {f->swvdr}, {f->swvdf}, {f->swidr}, {f->swidf}}, dp->tr_pond != 0,
                    {f->apondn, f->hpondn},
                    {chained ? pond_b_.p + P_APOND * ncp : nullptr, chained ? pond_b_.p + P_HPOND * ncp : nullptr}, 7, {f->alvdrn, f->alidrn, f->alvdfn, f->alidfn, f->albicen, f->albsnon, f->albpndn},
                    {{f->fswsfcn, f->fswintn, f->fswthrun, f->Sswabsn, f->Iswabsn}}, &dedd_clock_, false, nullptr};
  radiation_stage(*tp, r, [&](double* p2, double* pc) {
    const size_t nc = (size_t)nx_ * ny_ * nb_ * NCAT;
    DeddArgs a{};
    a.p = *dp;
    radiation_args(a, *tp, p2, D_SWVDR, pc);
    a.snow_given = 0;
    a.coszen = p2;
    a.albpndn = pc + 6 * nc;
    if (dp->tr_pond) { a.fp = pc + 7 * nc; a.hp = pc + 8 * nc; }
    dedd_launch(a, stream_);
  });
}

void ColumnBatch::radiation_chain(int mode) {
  CICE_REQUIRE(mode == 0 || mode == 1, "cice_radiation_chain: mode must be 0 or 1");
  rad_mode_ = mode;
  sw_armed_ = false;
}

// planes of cpl_b_ (nx, ny, nb each): the nine inputs, the 13 in / out fields of scale_fluxes, the seven merged albedos, the
// eight *_gbm, scale_factor; the mixed layer's eight inputs, sst, qdp, its 13 outputs and the four optional ones.  Behind
// them albcnt (nstreams planes) and, where they are uploaded, the seven per-category albedos and aicen.
enum { C_COSZEN = 0, C_AICE, C_TF, C_TAIR, C_QA, C_SWVDR, C_SWVDF, C_SWIDR, C_SWIDF, C_FLUX, C_ALB = C_FLUX + CPL_FLUXES,
       C_GBM = C_ALB + 7, C_SF = C_GBM + 8, C_MIX_IN, C_SST = C_MIX_IN + 8, C_QDP, C_MIX_OUT, C_MIX_OPT = C_MIX_OUT + 13,
       C_2D = C_MIX_OPT + 4 };

// coupling_prep (drivers/cice4/CICE_RunMod.F90:588-767) on the batch: see include/cice4_amd.h
void ColumnBatch::coupling_prep(const CouplingParams* cp, double dt, const cice_coupling_fields* f, Halo* halo) {
  CICE_REQUIRE(cp, "cice_coupling_prep: cice_coupling_init has not been called");
  CICE_REQUIRE(f->state_resident == 0 || f->state_resident == 1, "cice_coupling_prep: state_resident must be 0 or 1");
  CICE_REQUIRE(f->alb_resident == 0 || f->alb_resident == 1, "cice_coupling_prep: alb_resident must be 0 or 1");
  CICE_REQUIRE(f->nstreams >= 0, "cice_coupling_prep: nstreams must not be negative");
  CICE_REQUIRE(!f->albcnt || f->nstreams >= 1, "cice_coupling_prep: albcnt is given with nstreams = 0");
  const bool st_res = f->state_resident == 1, alb_res = f->alb_resident == 1, scale = cp->scale != 0, mixed = cp->mixed != 0;
  CICE_REQUIRE(!st_res || therm2_state_,
               "cice_coupling_prep: state_resident needs a cice_step_ridge or cice_step_therm2_cleanup on this batch in front");
  CICE_REQUIRE(!alb_res || alb_scheme_ != ALB_NONE,
               "cice_coupling_prep: alb_resident needs a cice_step_radiation or cice_step_radiation_dedd on this batch in front");
  CICE_REQUIRE(!mixed || dt > 0.0, "cice_coupling_prep: dt must be positive");
  // the host arrays by plane of cpl_b_
  const double* in2[C_2D] = {};
  double* out2[C_2D] = {};
  const double* head[9] = {f->coszen, f->aice, f->Tf, f->Tair, f->Qa, f->swvdr, f->swvdf, f->swidr, f->swidf};
  double* const flux[CPL_FLUXES] = {f->strairxT, f->strairyT, f->fsens, f->flat, f->fswabs, f->flwout, f->evap, f->Tref,
                                    f->Qref, f->fresh, f->fsalt, f->fhocn, f->fswthru};
  double* const res[16] = {f->alvdr, f->alidr, f->alvdf, f->alidf, f->albice, f->albsno, f->albpnd, f->alvdf_gbm,
                           f->alidf_gbm, f->alvdr_gbm, f->alidr_gbm, f->fresh_gbm, f->fsalt_gbm, f->fhocn_gbm,
                           f->fswthru_gbm, f->scale_factor};
  static_assert(C_SF == C_ALB + 15 && C_MIX_IN == C_SF + 1, "order of res");
  const double* mix_in[8] = {f->potT, f->uatm, f->vatm, f->wind, f->zlvl, f->rhoa, f->flw, f->hmix};
  double* const mix_out[17] = {f->frzmlt, f->flwout_ocn, f->fsens_ocn, f->flat_ocn, f->evap_ocn, f->strairx_ocn, f->strairy_ocn,
                               f->Tref_ocn, f->Qref_ocn, f->alvdr_ocn, f->alidr_ocn, f->alvdf_ocn, f->alidf_ocn, f->delt,
                               f->delq, f->shcoef, f->lhcoef};
  bool ok = true;
  for (int k = 0; k < 9; ++k) {
    const bool used = k == C_COSZEN || k >= C_SWVDR || scale || (mixed && k != C_TAIR);   // aice, Tf, Tair, Qa otherwise
    ok = ok && (!used || head[k]);
    if (used) in2[k] = head[k];
  }
  for (int k = 0; k < CPL_FLUXES; ++k) {
    const bool used = scale || k >= CPL_FRESH;
    ok = ok && (!used || flux[k]);
    if (used) in2[C_FLUX + k] = flux[k];
    if (scale) out2[C_FLUX + k] = flux[k];
  }
  for (int k = 0; k < 16; ++k) {
    ok = ok && res[k];
    out2[C_ALB + k] = res[k];
  }
  for (int k = 0; k < 8 && mixed; ++k) {
    ok = ok && mix_in[k];
    in2[C_MIX_IN + k] = mix_in[k];
  }
  for (int k = 0; k < 17 && mixed; ++k) {
    ok = ok && (k >= 13 || mix_out[k]);
    out2[C_MIX_OUT + k] = mix_out[k];
  }
  if (mixed) {
    ok = ok && f->sst && f->qdp;
    in2[C_SST] = out2[C_SST] = f->sst;
    in2[C_QDP] = out2[C_QDP] = f->qdp;
  }
  ok = ok && (f->tmask || !(scale || mixed)) && (st_res || f->aicen);
  ok = ok && (alb_res || (f->alvdrn && f->alidrn && f->alvdfn && f->alidfn && f->albicen && f->albsnon));
  CICE_REQUIRE(ok, "cice_coupling_prep: NULL field");

  hipStream_t s = stream_;
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  const size_t want = (C_2D + (size_t)f->nstreams) * n2 + 8 * nc;
  if (cpl_b_.n != want) cpl_b_.alloc(want);
  if (cpl_bi_.n != n2) cpl_bi_.alloc(n2);
  auto d2 = [&](int k) { return cpl_b_.p + (size_t)k * n2; };
  double* const dcnt = d2(C_2D);
  double* const dc = dcnt + (size_t)f->nstreams * n2;      // alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, albpndn, aicen
  fan_->fork(s);
  if (f->tmask) CICE_HIP(hipMemcpyAsync(cpl_bi_.p, f->tmask, n2 * 4, hipMemcpyHostToDevice, cs()));
  for (int k = 0; k < C_2D; ++k)
    if (in2[k]) CICE_HIP(hipMemcpyAsync(d2(k), in2[k], n2 * 8, hipMemcpyHostToDevice, cs()));
  if (f->albcnt) CICE_HIP(hipMemcpyAsync(dcnt, f->albcnt, (size_t)f->nstreams * n2 * 8, hipMemcpyHostToDevice, cs()));
  const double* albn[7] = {f->alvdrn, f->alidrn, f->alvdfn, f->alidfn, f->albicen, f->albsnon, f->albpndn};
  for (int k = 0; k < 7 && !alb_res; ++k)
    if (albn[k]) CICE_HIP(hipMemcpyAsync(dc + k * nc, albn[k], nc * 8, hipMemcpyHostToDevice, cs()));
  if (!st_res) CICE_HIP(hipMemcpyAsync(dc + 7 * nc, f->aicen, nc * 8, hipMemcpyHostToDevice, cs()));
  fan_->join();

  cpl_clock_.mark(0, s);
  if (mixed) {                         // first: it reads fhocn, fswthru and aice before they are scaled
    MixedLayerArgs m{};
    m.p.init();
    m.np = (int)np; m.nb = nb_; m.dt = dt; m.albocn = cp->albocn;
    m.tmask = cpl_bi_.p;
    m.potT = d2(C_MIX_IN); m.uatm = d2(C_MIX_IN + 1); m.vatm = d2(C_MIX_IN + 2); m.wind = d2(C_MIX_IN + 3);
    m.zlvl = d2(C_MIX_IN + 4); m.rhoa = d2(C_MIX_IN + 5); m.flw = d2(C_MIX_IN + 6); m.hmix = d2(C_MIX_IN + 7);
    m.Qa = d2(C_QA); m.Tf = d2(C_TF); m.aice = d2(C_AICE);
    m.fhocn = d2(C_FLUX + CPL_FHOCN); m.fswthru = d2(C_FLUX + CPL_FSWTHRU);
    m.swvdr = d2(C_SWVDR); m.swvdf = d2(C_SWVDF); m.swidr = d2(C_SWIDR); m.swidf = d2(C_SWIDF);
    m.sst = d2(C_SST); m.qdp = d2(C_QDP);
    double** const o[17] = {&m.frzmlt, &m.flwout_ocn, &m.fsens_ocn, &m.flat_ocn, &m.evap_ocn, &m.strairx_ocn, &m.strairy_ocn,
                            &m.Tref_ocn, &m.Qref_ocn, &m.alvdr_ocn, &m.alidr_ocn, &m.alvdf_ocn, &m.alidf_ocn, &m.delt, &m.delq,
                            &m.shcoef, &m.lhcoef};
    for (int k = 0; k < 17; ++k) *o[k] = k < 13 || mix_out[k] ? d2(C_MIX_OUT + k) : nullptr;
    ocean_mixed_layer_launch(m, s);
  }
  cpl_clock_.mark(1, s);
  CouplingArgs a{};
  a.np = (int)np; a.ncat = NCAT; a.nb = nb_; a.nstreams = f->nstreams; a.scale = scale;
  a.tmask = f->tmask ? cpl_bi_.p : nullptr;
  if (alb_res) {                       // the scheme's per-category outputs (radiation_args): albpndn is delta-Eddington's
    const bool dedd = alb_scheme_ == ALB_DEDD;
    const double* pc = dedd ? dedd_b_.p + D_2D * n2 : rad_b_.p + R_2D * n2;
    a.alvdrn = pc; a.alidrn = pc + nc; a.alvdfn = pc + 2 * nc; a.alidfn = pc + 3 * nc; a.albicen = pc + 4 * nc;
    a.albsnon = pc + 5 * nc; a.albpndn = dedd ? pc + 6 * nc : nullptr;
  } else {
    a.alvdrn = dc; a.alidrn = dc + nc; a.alvdfn = dc + 2 * nc; a.alidfn = dc + 3 * nc; a.albicen = dc + 4 * nc;
    a.albsnon = dc + 5 * nc; a.albpndn = f->albpndn ? dc + 6 * nc : nullptr;
  }
  a.aicen = st_res ? aicen_.p : dc + 7 * nc;
  a.coszen = d2(C_COSZEN); a.aice = d2(C_AICE); a.Tf = d2(C_TF); a.Tair = d2(C_TAIR); a.Qa = d2(C_QA);
  a.swvdr = d2(C_SWVDR); a.swvdf = d2(C_SWVDF); a.swidr = d2(C_SWIDR); a.swidf = d2(C_SWIDF);
  for (int k = 0; k < CPL_FLUXES; ++k) a.flux[k] = in2[C_FLUX + k] ? d2(C_FLUX + k) : nullptr;
  double** const o[16] = {&a.alvdr, &a.alidr, &a.alvdf, &a.alidf, &a.albice, &a.albsno, &a.albpnd, &a.alvdf_gbm, &a.alidf_gbm,
                          &a.alvdr_gbm, &a.alidr_gbm, &a.fresh_gbm, &a.fsalt_gbm, &a.fhocn_gbm, &a.fswthru_gbm, &a.scale_factor};
  for (int k = 0; k < 16; ++k) *o[k] = d2(C_ALB + k);
  a.albcnt = f->albcnt ? dcnt : nullptr;
  coupling_prep_launch(a, s);
  cpl_clock_.mark(2, s);
  // ice_HaloUpdate (scale_factor, halo_info, field_loc_center, field_type_scalar) (:758-759)
  if (halo) halo->update_r8(d2(C_SF), 1, n2, true, LOC_CENTER, KIND_SCALAR);

  fan_->fork(s);
  for (int k = 0; k < C_2D; ++k)
    if (out2[k]) CICE_HIP(hipMemcpyAsync(out2[k], d2(k), n2 * 8, hipMemcpyDeviceToHost, cs()));
  if (f->albcnt) CICE_HIP(hipMemcpyAsync(f->albcnt, dcnt, (size_t)f->nstreams * n2 * 8, hipMemcpyDeviceToHost, cs()));
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  cpl_clock_.read(0, 2);
}

// compute_ponds and increment_age behind step_therm1 (CICE_RunMod.F90:449-454, :550-559): see include/cice4_amd.h.  The
// capi has checked the flags against the tracers and the arrays they require.
void ColumnBatch::step_ponds(const ThermoParams* tp, int nt_volpn, double dt, const cice_pond_fields* f) {
  CICE_REQUIRE(tp, "cice_step_ponds: cice_thermo_init has not been called");
  const bool resident = f->state_resident == 1, ponds = f->ponds != 0, age = f->age != 0;
  CICE_REQUIRE(!resident || therm1_state_,
               "cice_step_ponds: state_resident needs a cice_step_therm1 call without a stop on this batch in front");
  hipStream_t s = stream_;
  pond_armed_ = false;
  const size_t np = (size_t)nx_ * ny_, n2 = np * nb_, nc = n2 * NCAT;
  if (pond_b_.n != P_PLANES * nc + n2) pond_b_.alloc(P_PLANES * nc + n2);
  auto pl = [&](int k) { return pond_b_.p + (size_t)k * nc; };
  double* const dfrain = pl(P_PLANES);
  // plane `it` of the caller's trcrn(nx, ny, max_ntrcr, ncat, nb) and plane `k` of pond_b_, one strided copy
  auto tracer_plane = [&](int it, int k, hipMemcpyKind kind) {
    double* h = f->trcrn + (size_t)it * np;
    const size_t hp = (size_t)NTRCR * np * 8, dp = np * 8;
    if (kind == hipMemcpyHostToDevice) CICE_HIP(hipMemcpy2DAsync(pl(k), dp, h, hp, np * 8, (size_t)NCAT * nb_, kind, cs()));
    else CICE_HIP(hipMemcpy2DAsync(h, hp, pl(k), dp, np * 8, (size_t)NCAT * nb_, kind, cs()));
  };
  auto up = [&](int k, const double* h) { CICE_HIP(hipMemcpyAsync(pl(k), h, nc * 8, hipMemcpyHostToDevice, cs())); };
  fan_->fork(s);
  if (ponds) {
    CICE_HIP(hipMemcpyAsync(dfrain, f->frain, n2 * 8, hipMemcpyHostToDevice, cs()));
    tracer_plane(nt_volpn - 1, P_VOLPN, hipMemcpyHostToDevice);
    up(P_APOND, f->apondn); up(P_HPOND, f->hpondn);
  }
  if (age) tracer_plane(tp->nt_iage - 1, P_IAGE, hipMemcpyHostToDevice);
  if (!resident) {
    up(P_AICEN, f->aicen);
    if (ponds) {
      up(P_VICEN, f->vicen); up(P_VSNON, f->vsnon); up(P_MELTT, f->melttn); up(P_MELTS, f->meltsn);
      tracer_plane(tp->nt_Tsfc - 1, P_TSFC, hipMemcpyHostToDevice);
    }
  }
  fan_->join();
  PondArgs a{};
  a.nx = nx_; a.np = (int)np; a.ncat = NCAT; a.nb = nb_; a.ponds = ponds; a.age = age; a.dt = dt;
  a.blk = blk_.p;
  a.volpn_planes = 1; a.iage_planes = 1;
  a.volpn = pl(P_VOLPN); a.iage = pl(P_IAGE); a.apondn = pl(P_APOND); a.hpondn = pl(P_HPOND); a.frain = dfrain;
  if (resident) {                      // out15_: fsurfn ... fhocnn, meltt, melts, ... (ThermoArgs' order)
    a.aicen = aicen_.p; a.vicen = vicen_.p; a.vsnon = vsnon_.p;
    a.Tsfc = trcrn_.p + (size_t)(tp->nt_Tsfc - 1) * np; a.tsfc_planes = NTRCR;
    a.meltt = out15_.p + 10 * nc; a.melts = out15_.p + 11 * nc;
  } else {
    a.aicen = pl(P_AICEN); a.vicen = pl(P_VICEN); a.vsnon = pl(P_VSNON); a.Tsfc = pl(P_TSFC); a.tsfc_planes = 1;
    a.meltt = pl(P_MELTT); a.melts = pl(P_MELTS);
  }
  pond_clock_.mark(0, s);
  pond_launch(a, s);
  pond_clock_.mark(1, s);
  fan_->fork(s);
  if (ponds) {
    CICE_HIP(hipMemcpyAsync(f->apondn, pl(P_APOND), nc * 8, hipMemcpyDeviceToHost, cs()));
    CICE_HIP(hipMemcpyAsync(f->hpondn, pl(P_HPOND), nc * 8, hipMemcpyDeviceToHost, cs()));
    tracer_plane(nt_volpn - 1, P_VOLPN, hipMemcpyDeviceToHost);
  }
  if (age) tracer_plane(tp->nt_iage - 1, P_IAGE, hipMemcpyDeviceToHost);
  fan_->join();
  CICE_HIP(hipStreamSynchronize(s));
  pond_clock_.read(0, 1);
  if (ponds) {
    pond_host_[0] = f->apondn; pond_host_[1] = f->hpondn;
    pond_armed_ = pond_mode_ == 1;
  }
}

void ColumnBatch::pond_chain(int mode) {
  CICE_REQUIRE(mode == 0 || mode == 1, "cice_pond_chain: mode must be 0 or 1");
  pond_mode_ = mode;
  pond_armed_ = false;
}

void ColumnBatch::handover_time(bool enable, float* ms) {
  if (ho_pending_) {                   // (every path of column_stages has waited for the stream since)
    CICE_HIP(hipEventElapsedTime(&ho_ms_, ho_ev_[0], ho_ev_[1]));
    ho_pending_ = false;
  }
  if (ms) *ms = ho_ms_;
  if (enable != ho_timed_) ho_ms_ = 0.0f;
  ho_timed_ = enable;
}

void ColumnBatch::ridge_times(bool enable, float ms[RIDGE_TIMES]) {
  ridge_timed_ = enable;
  for (int k = 0; k < RIDGE_TIMES && ms; ++k) ms[k] = ridge_ms_[k];
}

void ColumnBatch::cleanup_times(bool enable, float ms[CLEAN_TIMES]) {
  clean_timed_ = enable;
  for (int k = 0; k < CLEAN_TIMES && ms; ++k) ms[k] = clean_ms_[k];
}

long long ColumnBatch::debug_read(const char* what, long long* out, long long cap) const {
  const bool niter = !std::strcmp(what, "thermo_niter");
  if (!niter && std::strcmp(what, "thermo_perm")) return -1;
  const void* src = niter ? (const void*)niter_.p : (const void*)perm_.p;
  const long long nbytes = niter ? (long long)niter_.n : (long long)perm_.n * 4, nw = (nbytes + 7) / 8;
  if (out && nbytes) {
    CICE_REQUIRE(cap >= nw, "cice_evp_debug: buffer too small");
    CICE_HIP(hipStreamSynchronize(stream_));
    CICE_HIP(hipMemcpy(out, src, (size_t)nbytes, hipMemcpyDeviceToHost));
  }
  return nw;
}

}  // namespace cice
