// C-ABI of libcice4_amd.so: thermodynamic changes of the thickness distribution, block-wise and on the batch.
#include "capi.h"

namespace {
// plane offsets of the block-wise staging buffer (units of nx*ny doubles)
enum { IB_AICEN = 0, IB_VICEN = 5, IB_VSNON = 10, IB_TRCRN = 15, IB_EICEN = 40, IB_ESNON = 60, IB_AINIT = 65,
       IB_VINIT = 70, IB_2D = 75, IB_SHIFT = 87, IB_PLANES = 102 };
static_assert(NCAT == 5 && NILYR == 4 && NSLYR == 1 && NTRCR == 5, "plane offsets above");

// the record words once the stream has run dry
void itd_read_rec(cice_ctx* c, unsigned long long h[ITD_REC_WORDS]) {
  CICE_HIP(hipMemcpyAsync(h, c->itd_rec.p, ITD_REC_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
  CICE_HIP(hipStreamSynchronize(c->stream));
}

// the state arrays of the block-wise entries in the order they travel; an entry moves the members it names
enum { ST_AICEN = 1, ST_VICEN = 2, ST_VSNON = 4, ST_TRCRN = 8, ST_EICEN = 16, ST_ESNON = 32, ST_ALL = 63 };
struct ItdState { double *aicen, *vicen, *vsnon, *trcrn, *eicen, *esnon; };

struct ItdBlock {   // one (nx, ny) block staged on the device
  cice_ctx* c;
  size_t np;
  ItdArgs a{};
  std::vector<int32_t> lp;
  const int32_t *indxi, *indxj;
  double* pl(int plane) const { return c->itd_d.p + (size_t)plane * np; }
  ItdBlock(cice_ctx* c_, int nx, int ny, int icells, const int32_t* indxi_, const int32_t* indxj_)
      : c(c_), np((size_t)nx * ny), indxi(indxi_), indxj(indxj_) {
    CICE_REQUIRE(c->have_itd, "cice_itd_init has not been called");
    lp = list_mask(nx, ny, icells, indxi, indxj, true);
    c->need_device();
    if (c->itd_d.n < IB_PLANES * np) c->itd_d.alloc(IB_PLANES * np);
    if (c->itd_i.n < 7 * np + 4) c->itd_i.alloc(7 * np + 4);
    c->itd_rec.alloc(ITD_REC_WORDS);
    const int32_t blk[4] = {1, nx, 1, ny};
    hipStream_t s = c->stream;
    CICE_HIP(hipMemcpyAsync(c->itd_i.p, lp.data(), np * 4, hipMemcpyHostToDevice, s));
    CICE_HIP(hipMemcpyAsync(c->itd_i.p + 7 * np, blk, 16, hipMemcpyHostToDevice, s));
    CICE_HIP(hipStreamSynchronize(s));   // blk is a local
    a.p = c->ip;
    a.nx = nx; a.ny = ny; a.nblocks = 1; a.icells = icells; a.kitd = 1; a.bfail = 1; a.nlimit = 0; a.bend = 1;
    a.listpos = c->itd_i.p; a.blk = c->itd_i.p + 7 * np;
    a.aicen = pl(IB_AICEN); a.vicen = pl(IB_VICEN); a.vsnon = pl(IB_VSNON); a.trcrn = pl(IB_TRCRN);
    a.eicen = pl(IB_EICEN); a.esnon = pl(IB_ESNON); a.aicen_init = pl(IB_AINIT); a.vicen_init = pl(IB_VINIT);
    a.aice = pl(IB_2D + I2_AICE); a.aice0 = pl(IB_2D + I2_AICE0); a.frzmlt = pl(IB_2D + I2_FRZMLT);
    a.Tf = pl(IB_2D + I2_TF); a.rside = pl(IB_2D + I2_RSIDE); a.fresh = pl(IB_2D + I2_FRESH);
    a.fsalt = pl(IB_2D + I2_FSALT); a.fhocn = pl(IB_2D + I2_FHOCN); a.frazil = pl(IB_2D + I2_FRAZIL);
    a.meltl = pl(IB_2D + I2_MELTL); a.frz_onset = pl(IB_2D + I2_FRZ_ONSET);
    a.rec = c->itd_rec.p;
  }
  void set_tracers(int ntrcr, const int32_t* dep) {   // the reference passes ntrcr, trcr_depend with every call
    CICE_REQUIRE(ntrcr >= 1 && ntrcr <= NTRCR && a.p.it_Tsfc < ntrcr, "ntrcr out of range");
    a.p.ntrcr = ntrcr;
    for (int k = 0; k < ntrcr && dep; ++k) {
      CICE_REQUIRE(dep[k] >= 0 && dep[k] <= 2, "trcr_depend must be 0, 1 or 2");
      a.p.dep[k] = dep[k];
    }
  }
  void up(int plane, const double* h, int planes = 1) const {
    CICE_HIP(hipMemcpyAsync(pl(plane), h, (size_t)planes * np * 8, hipMemcpyHostToDevice, c->stream));
  }
  void down(double* h, int plane, int planes = 1) const {
    CICE_HIP(hipMemcpyAsync(h, pl(plane), (size_t)planes * np * 8, hipMemcpyDeviceToHost, c->stream));
  }
  void state(const ItdState& h, int members, bool to_device) const {
    const struct { int member, plane, planes; double* h; } list[] = {
        {ST_AICEN, IB_AICEN, NCAT, h.aicen}, {ST_VICEN, IB_VICEN, NCAT, h.vicen}, {ST_VSNON, IB_VSNON, NCAT, h.vsnon},
        {ST_TRCRN, IB_TRCRN, NCAT * NTRCR, h.trcrn}, {ST_EICEN, IB_EICEN, NCAT * NILYR, h.eicen},
        {ST_ESNON, IB_ESNON, NCAT * NSLYR, h.esnon}};
    for (const auto& x : list)
      if (members & x.member) to_device ? up(x.plane, x.h, x.planes) : down(x.h, x.plane, x.planes);
  }
  void clear_rec() const { CICE_HIP(hipMemsetAsync(c->itd_rec.p, 0, ITD_REC_WORDS * 8, c->stream)); }
  // shift_ice stopped (r[ITD_REC_SHIFT]): again from the inputs, up to the failing boundary (itd.h), for the cell to name
  template <class Upload, class Launch>
  void rerun_to_stop(unsigned long long r[ITD_REC_WORDS], Upload upload, Launch launch, int32_t* l_stop, int32_t* istop,
                     int32_t* jstop) {
    const int N = NCAT - (int)((r[ITD_REC_SHIFT] - 1) & 0xff);
    upload();
    clear_rec();
    a.bfail = 0; a.nlimit = N;         // (bfail: linear_itd's kernel; shift_ice's own does not read it)
    launch();
    itd_read_rec(c, r);
    const unsigned long long key = itd_shift_key(r, N);
    *l_stop = 1;
    if (key) { *istop = indxi[key - 1]; *jstop = indxj[key - 1]; }
  }
};
}  // namespace

extern "C" {

int cice_itd_init(cice_ctx* ctx, const cice_itd_config* cfg) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "NULL argument");
  CICE_REQUIRE(cfg->ntrcr >= 1 && cfg->ntrcr <= NTRCR, "cice_itd_init: ntrcr out of range");
  ItdParams p{};
  p.ntrcr = cfg->ntrcr;
  for (int k = 0; k < cfg->ntrcr; ++k) {
    CICE_REQUIRE(cfg->trcr_depend[k] >= 0 && cfg->trcr_depend[k] <= 2, "cice_itd_init: trcr_depend must be 0, 1 or 2");
    p.dep[k] = cfg->trcr_depend[k];
  }
  auto slot = [&](int nt, bool needed, const char* what) {
    CICE_REQUIRE(!needed || (nt >= 1 && nt <= cfg->ntrcr), what);
    return nt - 1;
  };
  p.it_Tsfc = slot(cfg->nt_Tsfc, true, "cice_itd_init: nt_Tsfc is not a tracer in use");
  p.it_iage = slot(cfg->nt_iage, cfg->tr_iage != 0, "cice_itd_init: tr_iage without nt_iage");
  p.it_alvl = slot(cfg->nt_alvl, cfg->tr_lvl != 0, "cice_itd_init: tr_lvl without nt_alvl");
  p.it_vlvl = slot(cfg->nt_vlvl, cfg->tr_lvl != 0, "cice_itd_init: tr_lvl without nt_vlvl");
  p.tr_iage = cfg->tr_iage != 0; p.tr_lvl = cfg->tr_lvl != 0; p.update_ocn_f = cfg->update_ocn_f != 0;
  for (int n = 0; n <= NCAT; ++n) p.hin_max[n] = cfg->hin_max[n];
  p.hi_min = cfg->hi_min;
  c_->ip = p;
  c_->have_itd = true;
  CICE_CATCH
}

int cice_linear_itd(cice_ctx* ctx, int nx, int ny, int icells, const int32_t* indxi, const int32_t* indxj, int ntrcr,
                    const int32_t* trcr_depend, const double* aicen_init, const double* vicen_init, double* aicen,
                    double* trcrn, double* vicen, double* vsnon, double* eicen, double* esnon, double* aice,
                    double* aice0, int32_t* l_stop, int32_t* istop, int32_t* jstop, long long* n_not_remapped) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(aicen_init && vicen_init && aicen && trcrn && vicen && vsnon && eicen && esnon && aice && aice0 && l_stop &&
                   istop && jstop, "linear_itd: NULL argument");
  ItdBlock B(c_, nx, ny, icells, indxi, indxj);
  B.set_tracers(ntrcr, trcr_depend);
  const ItdState st{aicen, vicen, vsnon, trcrn, eicen, esnon};
  auto up_state = [&] {
    B.state(st, ST_ALL, true);
    B.up(IB_2D + I2_AICE, aice); B.up(IB_2D + I2_AICE0, aice0);
  };
  auto launch = [&] { itd_launch_linear(B.a, c_->stream); };
  up_state();
  B.up(IB_AINIT, aicen_init, NCAT); B.up(IB_VINIT, vicen_init, NCAT);
  B.clear_rec();
  launch();
  unsigned long long r[ITD_REC_WORDS];
  itd_read_rec(c_, r);
  clear_stop(l_stop, istop, jstop);
  if (n_not_remapped) *n_not_remapped = (long long)r[ITD_REC_NOREMAP];
  if (r[ITD_REC_SHIFT]) B.rerun_to_stop(r, up_state, launch, l_stop, istop, jstop);
  B.state(st, ST_ALL, false);
  B.down(aice, IB_2D + I2_AICE); B.down(aice0, IB_2D + I2_AICE0);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

int cice_shift_ice(cice_ctx* ctx, int nx, int ny, const int32_t* indxi, const int32_t* indxj, int icells, int ntrcr,
                   const int32_t* trcr_depend, double* aicen, double* trcrn, double* vicen, double* vsnon, double* eicen,
                   double* esnon, double* hicen, const int32_t* donor, double* daice, double* dvice, int32_t* l_stop,
                   int32_t* istop, int32_t* jstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(aicen && trcrn && vicen && vsnon && eicen && esnon && hicen && donor && daice && dvice && l_stop && istop &&
                   jstop, "shift_ice: NULL argument");
  for (int n = 1; n < NCAT; ++n)
    for (int ij = 0; ij < icells; ++ij) {
      const int d = donor[(size_t)(n - 1) * icells + ij];
      CICE_REQUIRE(d == 0 || d == n || d == n + 1, "shift_ice: donor(ij, n) must be 0, n or n + 1");
      CICE_REQUIRE(d != 0 || !(daice[(size_t)(n - 1) * icells + ij] > 0.0), "shift_ice: daice > 0 without a donor");
    }
  ItdBlock B(c_, nx, ny, icells, indxi, indxj);
  B.set_tracers(ntrcr, trcr_depend);
  const size_t np = B.np, ne = (size_t)icells * NCAT;
  double* dsh = B.pl(IB_SHIFT);        // hicen, daice, dvice: 3 x icells x ncat <= 15 planes
  int32_t* ddon = c_->itd_i.p + np;    // donor: icells x ncat <= 5 planes
  B.a.hicen = dsh; B.a.daice = dsh + ne; B.a.dvice = dsh + 2 * ne; B.a.donor = ddon;
  hipStream_t s = c_->stream;
  const ItdState st{aicen, vicen, vsnon, trcrn, eicen, esnon};
  auto up_state = [&] {
    B.state(st, ST_ALL, true);
    if (ne) {
      CICE_HIP(hipMemcpyAsync(dsh, hicen, ne * 8, hipMemcpyHostToDevice, s));
      CICE_HIP(hipMemcpyAsync(dsh + ne, daice, ne * 8, hipMemcpyHostToDevice, s));
      CICE_HIP(hipMemcpyAsync(dsh + 2 * ne, dvice, ne * 8, hipMemcpyHostToDevice, s));
      CICE_HIP(hipMemcpyAsync(ddon, donor, ne * 4, hipMemcpyHostToDevice, s));
    }
  };
  auto launch = [&] { itd_launch_shift(B.a, s); };
  up_state();
  B.clear_rec();
  launch();
  unsigned long long r[ITD_REC_WORDS];
  itd_read_rec(c_, r);
  clear_stop(l_stop, istop, jstop);
  if (r[ITD_REC_SHIFT]) B.rerun_to_stop(r, up_state, launch, l_stop, istop, jstop);
  B.state(st, ST_ALL, false);
  if (ne) {
    CICE_HIP(hipMemcpyAsync(hicen, dsh, ne * 8, hipMemcpyDeviceToHost, s));
    CICE_HIP(hipMemcpyAsync(daice, dsh + ne, ne * 8, hipMemcpyDeviceToHost, s));
    CICE_HIP(hipMemcpyAsync(dvice, dsh + 2 * ne, ne * 8, hipMemcpyDeviceToHost, s));
  }
  CICE_HIP(hipStreamSynchronize(s));
  CICE_CATCH
}

int cice_add_new_ice(cice_ctx* ctx, int nx, int ny, int ntrcr, int icells, const int32_t* indxi, const int32_t* indxj,
                     const int32_t* tmask, double dt, double* aicen, double* trcrn, double* vicen, double* eicen,
                     double* aice0, const double* aice, const double* frzmlt, double* frazil, double* frz_onset,
                     double yday, double* fresh, double* fsalt, const double* Tf, int32_t* l_stop, int32_t* istop,
                     int32_t* jstop) {
  CICE_TRY(ctx) c_->chain_ready = false;
  (void)tmask;                         // the reference does not read it either
  CICE_REQUIRE(aicen && trcrn && vicen && eicen && aice0 && aice && frzmlt && frazil && fresh && fsalt && Tf && l_stop &&
                   istop && jstop, "add_new_ice: NULL argument");
  CICE_REQUIRE(dt > 0.0, "add_new_ice: dt");
  ItdBlock B(c_, nx, ny, icells, indxi, indxj);
  B.set_tracers(ntrcr, nullptr);
  B.a.dt = dt; B.a.yday = yday;
  if (!frz_onset) B.a.frz_onset = nullptr;   // `present(frz_onset)`, :1041
  const ItdState st{aicen, vicen, nullptr, trcrn, eicen, nullptr};
  const int members = ST_AICEN | ST_VICEN | ST_TRCRN | ST_EICEN;
  B.state(st, members, true);
  B.up(IB_2D + I2_AICE, aice); B.up(IB_2D + I2_AICE0, aice0); B.up(IB_2D + I2_FRZMLT, frzmlt);
  B.up(IB_2D + I2_TF, Tf); B.up(IB_2D + I2_FRAZIL, frazil); B.up(IB_2D + I2_FRESH, fresh); B.up(IB_2D + I2_FSALT, fsalt);
  if (frz_onset) B.up(IB_2D + I2_FRZ_ONSET, frz_onset);
  B.clear_rec();
  itd_launch_add_new_ice(B.a, c_->stream);
  B.state(st, members, false);
  B.down(aice0, IB_2D + I2_AICE0); B.down(frazil, IB_2D + I2_FRAZIL); B.down(fresh, IB_2D + I2_FRESH);
  B.down(fsalt, IB_2D + I2_FSALT);
  if (frz_onset) B.down(frz_onset, IB_2D + I2_FRZ_ONSET);
  unsigned long long r[ITD_REC_WORDS];
  itd_read_rec(c_, r);
  clear_stop(l_stop, istop, jstop);
  if (r[ITD_REC_ADD]) {
    const unsigned long long key = r[ITD_REC_ADD] & 0xffffffffull;
    *l_stop = 1; *istop = indxi[key - 1]; *jstop = indxj[key - 1];
  }
  CICE_CATCH
}

int cice_lateral_melt(cice_ctx* ctx, int nx, int ny, int ilo, int ihi, int jlo, int jhi, double dt, double* fresh,
                      double* fsalt, double* fhocn, const double* rside, double* meltl, double* aicen, double* vicen,
                      double* vsnon, double* eicen, double* esnon) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(fresh && fsalt && fhocn && rside && meltl && aicen && vicen && vsnon && eicen && esnon,
               "lateral_melt: NULL argument");
  CICE_REQUIRE(nx >= 1 && ny >= 1 && ilo >= 1 && ihi <= nx && jlo >= 1 && jhi <= ny && dt > 0.0, "bad dimensions");
  ItdBlock B(c_, nx, ny, 0, nullptr, nullptr);
  B.a.dt = dt;
  const int32_t blk[4] = {ilo, ihi, jlo, jhi};
  CICE_HIP(hipMemcpyAsync(c_->itd_i.p + 7 * B.np, blk, 16, hipMemcpyHostToDevice, c_->stream));
  CICE_HIP(hipStreamSynchronize(c_->stream));
  const ItdState st{aicen, vicen, vsnon, nullptr, eicen, esnon};
  B.state(st, ST_ALL & ~ST_TRCRN, true);
  B.up(IB_2D + I2_RSIDE, rside); B.up(IB_2D + I2_FRESH, fresh); B.up(IB_2D + I2_FSALT, fsalt);
  B.up(IB_2D + I2_FHOCN, fhocn); B.up(IB_2D + I2_MELTL, meltl);
  itd_launch_lateral_melt(B.a, c_->stream);
  B.state(st, ST_ALL & ~ST_TRCRN, false);
  B.down(fresh, IB_2D + I2_FRESH); B.down(fsalt, IB_2D + I2_FSALT); B.down(fhocn, IB_2D + I2_FHOCN);
  B.down(meltl, IB_2D + I2_MELTL);
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

// The stage on the batch (ice_step_mod.F90:286-422): see include/cice4_amd.h
int cice_step_therm2_itd(cice_ctx* ctx, double dt, double yday, const cice_therm2_fields* f, int32_t* l_stop,
                         int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f && l_stop && istop && jstop && bstop && stage, "NULL argument");
  if (f->ncat == 1) throw Error{CICE_EUNSUPPORTED, "cice_step_therm2_itd: ncat = 1 (reduce_area) is not built"};
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_therm2_itd: ncat is not the library's");
  NEED_BATCH(true);
  c_->batch.step_therm2_itd(c_->thermo(), c_->itd(), dt, yday, f, l_stop, istop, jstop, bstop, stage);
  CICE_CATCH
}

// cleanup_itd (ice_itd.F90:1600-1835) on one block: see include/cice4_amd.h and cleanup.h
int cice_cleanup_itd(cice_ctx* ctx, int nx, int ny, int ilo, int ihi, int jlo, int jhi, double dt, int ntrcr, double* aicen,
                     double* trcrn, double* vicen, double* vsnon, double* eicen, double* esnon, double* aice0, double* aice,
                     const int32_t* trcr_depend, double* fresh, double* fsalt, double* fhocn, int heat_capacity,
                     int32_t* l_stop, int32_t* istop, int32_t* jstop, int limit_aice) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(aicen && trcrn && vicen && vsnon && eicen && esnon && aice0 && aice && trcr_depend && l_stop && istop && jstop,
               "cleanup_itd: NULL argument");
  CICE_REQUIRE(nx >= 1 && ny >= 1 && ilo >= 1 && ihi <= nx && jlo >= 1 && jhi <= ny && dt > 0.0, "bad dimensions");
  if (!heat_capacity) throw Error{CICE_EUNSUPPORTED, "cleanup_itd: heat_capacity = F (zerolayer_check) is not built"};
  ItdBlock B(c_, nx, ny, 0, nullptr, nullptr);
  B.set_tracers(ntrcr, trcr_depend);
  hipStream_t s = c_->stream;
  const int32_t blk[4] = {ilo, ihi, jlo, jhi};
  CICE_HIP(hipMemcpyAsync(c_->itd_i.p + 7 * B.np, blk, 16, hipMemcpyHostToDevice, s));
  CICE_HIP(hipStreamSynchronize(s));
  const ItdState st{aicen, vicen, vsnon, trcrn, eicen, esnon};
  B.state(st, ST_ALL, true);
  B.up(IB_2D + I2_AICE, aice); B.up(IB_2D + I2_AICE0, aice0);
  if (fresh) B.up(IB_2D + I2_FRESH, fresh);
  if (fsalt) B.up(IB_2D + I2_FSALT, fsalt);
  if (fhocn) B.up(IB_2D + I2_FHOCN, fhocn);
  static_assert(ITD_REC_WORDS >= CW_WORDS, "the record words hold a block's words");
  B.clear_rec();
  CleanArgs a{};
  a.p = B.a.p;
  a.nx = nx; a.ny = ny; a.nblocks = 1; a.blk = B.a.blk; a.limit_aice = limit_aice != 0; a.dt = dt;
  a.aicen = B.a.aicen; a.trcrn = B.a.trcrn; a.vicen = B.a.vicen; a.vsnon = B.a.vsnon; a.eicen = B.a.eicen;
  a.esnon = B.a.esnon; a.aice = B.a.aice; a.aice0 = B.a.aice0;
  a.fresh = fresh ? B.a.fresh : nullptr; a.fsalt = fsalt ? B.a.fsalt : nullptr; a.fhocn = fhocn ? B.a.fhocn : nullptr;
  a.bw = c_->itd_rec.p;
  clean_launch_all(a, s);
  B.state(st, ST_ALL, false);
  B.down(aice, IB_2D + I2_AICE); B.down(aice0, IB_2D + I2_AICE0);
  if (fresh) B.down(fresh, IB_2D + I2_FRESH);
  if (fsalt) B.down(fsalt, IB_2D + I2_FSALT);
  if (fhocn) B.down(fhocn, IB_2D + I2_FHOCN);
  unsigned long long r[ITD_REC_WORDS];
  itd_read_rec(c_, r);
  clear_stop(l_stop, istop, jstop);
  size_t q = 0;
  if (clean_decode(r, B.np, &q)) {
    *l_stop = 1; *istop = (int32_t)(q % nx) + 1; *jstop = (int32_t)(q / nx) + 1;
  }
  CICE_CATCH
}

// aggregate (ice_itd.F90:279-485) on one block
int cice_aggregate(cice_ctx* ctx, int nx, int ny, const double* aicen, const double* trcrn, const double* vicen,
                   const double* vsnon, const double* eicen, const double* esnon, double* aice, double* trcr, double* vice,
                   double* vsno, double* eice, double* esno, double* aice0, const int32_t* tmask, int ntrcr,
                   const int32_t* trcr_depend) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(aicen && trcrn && vicen && vsnon && eicen && esnon && aice && trcr && vice && vsno && eice && esno && aice0 &&
                   tmask && trcr_depend, "aggregate: NULL argument");
  ItdBlock B(c_, nx, ny, 0, nullptr, nullptr);
  B.set_tracers(ntrcr, trcr_depend);
  hipStream_t s = c_->stream;
  auto in = [](const double* p) { return const_cast<double*>(p); };   // (uploaded only)
  const ItdState st{in(aicen), in(vicen), in(vsnon), in(trcrn), in(eicen), in(esnon)};
  B.state(st, ST_ALL, true);
  int32_t* dmask = c_->itd_i.p + B.np;
  CICE_HIP(hipMemcpyAsync(dmask, tmask, B.np * 4, hipMemcpyHostToDevice, s));
  CICE_HIP(hipMemcpyAsync(B.pl(IB_SHIFT + 4), trcr, (size_t)NTRCR * B.np * 8, hipMemcpyHostToDevice, s));   // planes >= ntrcr stay
  CleanArgs a{};
  a.p = B.a.p;
  a.nx = nx; a.ny = ny; a.nblocks = 1; a.blk = B.a.blk; a.dt = 1.0;
  a.aicen = B.a.aicen; a.trcrn = B.a.trcrn; a.vicen = B.a.vicen; a.vsnon = B.a.vsnon; a.eicen = B.a.eicen;
  a.esnon = B.a.esnon; a.aice = B.a.aice; a.aice0 = B.a.aice0; a.tmask = dmask;
  a.vice = B.pl(IB_SHIFT); a.vsno = B.pl(IB_SHIFT + 1); a.eice = B.pl(IB_SHIFT + 2); a.esno = B.pl(IB_SHIFT + 3);
  a.trcr = B.pl(IB_SHIFT + 4);
  clean_launch_aggregate(a, s);
  B.down(aice, IB_2D + I2_AICE); B.down(aice0, IB_2D + I2_AICE0);
  B.down(vice, IB_SHIFT); B.down(vsno, IB_SHIFT + 1); B.down(eice, IB_SHIFT + 2); B.down(esno, IB_SHIFT + 3);
  B.down(trcr, IB_SHIFT + 4, NTRCR);
  CICE_HIP(hipStreamSynchronize(s));
  CICE_CATCH
}

// The second half of step_therm2 on the batch (ice_step_mod.F90:445-511): see include/cice4_amd.h
int cice_step_therm2_cleanup(cice_ctx* ctx, double dt, const cice_therm2_cleanup_fields* f, int32_t* l_stop, int32_t* istop,
                             int32_t* jstop, int32_t* bstop, int32_t* stage) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f && l_stop && istop && jstop && bstop && stage, "NULL argument");
  if (f->ncat == 1) throw Error{CICE_EUNSUPPORTED, "cice_step_therm2_cleanup: ncat = 1 is not built"};
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_therm2_cleanup: ncat is not the library's");
  NEED_BATCH(true);
  Halo* halo = nullptr;
  if (f->bound) {
    CICE_REQUIRE(c_->have_domain, "cice_step_therm2_cleanup: bound = 1 needs cice_domain_create");
    CICE_REQUIRE(c_->batch.same_layout(c_->dom), "cice_step_therm2_cleanup: the batch does not have the domain's layout");
    c_->need_halo();
    halo = c_->halo.get();
  }
  c_->batch.step_therm2_cleanup(c_->itd(), dt, f, halo, l_stop, istop, jstop, bstop, stage);
  CICE_CATCH
}

int cice_ridge_init(cice_ctx* ctx, int krdg_partic, int krdg_redist, double mu_rdg) {
  CICE_TRY(ctx)
  CICE_REQUIRE(krdg_partic == 0 || krdg_partic == 1, "cice_ridge_init: krdg_partic must be 0 or 1");
  CICE_REQUIRE(krdg_redist == 0 || krdg_redist == 1, "cice_ridge_init: krdg_redist must be 0 or 1");
  if (krdg_redist == 0)
    throw Error{CICE_EUNSUPPORTED, "cice_ridge_init: krdg_redist = 0 is not built (the reference indexes hrmax by the "
                                   "compressed counter of ridging cells; see ridge.h)"};
  CICE_REQUIRE(mu_rdg > 0.0, "cice_ridge_init: mu_rdg must be positive");
  c_->rp = RidgeParams{krdg_partic, krdg_redist, mu_rdg};
  c_->have_ridge = true;
  CICE_CATCH
}

// ridge_ice (ice_mechred.F90:133-552) on one block: see include/cice4_amd.h and ridge.h
int cice_ridge_ice(cice_ctx* ctx, int nx, int ny, double dt, int ntrcr, int icells, const int32_t* indxi,
                   const int32_t* indxj, const double* rdg_conv, const double* rdg_shear, double* aicen, double* trcrn,
                   double* vicen, double* vsnon, double* eicen, double* esnon, double* aice0, const int32_t* trcr_depend,
                   int32_t* l_stop, int32_t* istop, int32_t* jstop, double* dardg1dt, double* dardg2dt, double* dvirdgdt,
                   double* opening, double* fresh, double* fhocn, int32_t* niter) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(rdg_conv && rdg_shear && aicen && trcrn && vicen && vsnon && eicen && esnon && aice0 && trcr_depend &&
                   l_stop && istop && jstop, "ridge_ice: NULL argument");
  CICE_REQUIRE(c_->have_ridge, "cice_ridge_init has not been called");
  CICE_REQUIRE(dt > 0.0, "ridge_ice: dt");
  ItdBlock B(c_, nx, ny, icells, indxi, indxj);
  B.set_tracers(ntrcr, trcr_depend);
  clear_stop(l_stop, istop, jstop);
  if (niter) *niter = 0;
  if (icells == 0) return CICE_OK;     // (the caller's `if (icells > 0)`: nothing is read or written)
  hipStream_t s = c_->stream;
  // planes of the staging buffer that the thickness-distribution entries use for other things
  enum { P_CONV = IB_AINIT, P_SHEAR, P_D1, P_D2, P_DV, P_OPEN, P_WORK = IB_SHIFT };
  static_assert(P_OPEN < IB_2D && P_WORK + RG_PLANES <= IB_PLANES, "planes of the staging buffer");
  const ItdState st{aicen, vicen, vsnon, trcrn, eicen, esnon};
  B.state(st, ST_ALL, true);
  B.up(IB_2D + I2_AICE0, aice0); B.up(P_CONV, rdg_conv); B.up(P_SHEAR, rdg_shear);
  const struct { double* h; int plane; } opt[6] = {{dardg1dt, P_D1}, {dardg2dt, P_D2}, {dvirdgdt, P_DV}, {opening, P_OPEN},
                                                   {fresh, IB_2D + I2_FRESH}, {fhocn, IB_2D + I2_FHOCN}};
  for (const auto& o : opt)
    if (o.h) B.up(o.plane, o.h);
  c_->ridge_w.alloc(RW_WORDS);
  c_->ridge_w.zero(s);
  RidgeArgs a{};
  a.p = B.a.p; a.r = c_->rp;
  a.nx = nx; a.ny = ny; a.nblocks = 1; a.listpos = B.a.listpos; a.dt = dt;
  a.rdg_conv = B.pl(P_CONV); a.rdg_shear = B.pl(P_SHEAR);
  a.aicen = B.a.aicen; a.trcrn = B.a.trcrn; a.vicen = B.a.vicen; a.vsnon = B.a.vsnon; a.eicen = B.a.eicen;
  a.esnon = B.a.esnon; a.aice0 = B.a.aice0;
  a.dardg1dt = dardg1dt ? B.pl(P_D1) : nullptr; a.dardg2dt = dardg2dt ? B.pl(P_D2) : nullptr;
  a.dvirdgdt = dvirdgdt ? B.pl(P_DV) : nullptr; a.opening = opening ? B.pl(P_OPEN) : nullptr;
  a.fresh = fresh ? B.a.fresh : nullptr; a.fhocn = fhocn ? B.a.fhocn : nullptr;
  a.work = B.pl(P_WORK); a.bw = c_->ridge_w.p;
  unsigned long long w[RW_WORDS];
  for (int done = 0;;) {
    const int count = std::min<int>(RIDGE_QUEUE, RIDGE_NITERMAX - done);
    ridge_launch_iterations(a, done + 1, count, s);
    done += count;
    CICE_HIP(hipMemcpyAsync(w, a.bw, sizeof w, hipMemcpyDeviceToHost, s));
    CICE_HIP(hipStreamSynchronize(s));
    if (!ridge_wants_more(w, done)) break;
  }
  unsigned pos = 0;
  int n_it = 0;
  const int stop = ridge_decode(w, &pos, &n_it);
  if (stop == RIDGE_OK) ridge_launch_finish(a, s);
  B.state(st, ST_ALL, false);
  B.down(aice0, IB_2D + I2_AICE0);
  for (const auto& o : opt)
    if (o.h) B.down(o.h, o.plane);
  CICE_HIP(hipStreamSynchronize(s));
  if (niter) *niter = n_it;
  if (stop != RIDGE_OK) {
    *l_stop = 1;
    if (pos) { *istop = indxi[pos - 1]; *jstop = indxj[pos - 1]; }
  }
  CICE_CATCH
}

// The column half of step_dynamics on the batch (ice_step_mod.F90:586-745): see include/cice4_amd.h
int cice_step_ridge(cice_ctx* ctx, double dt, const cice_ridge_fields* f, int32_t* l_stop, int32_t* istop, int32_t* jstop,
                    int32_t* bstop, int32_t* stage) {
  CICE_TRY_HANDOVER(ctx) c_->chain_ready = false;
  // the consumer of the transport -> ridging hand-over: given the arrays the armed transport call was given, it takes the
  // state from the transport's device buffers; anything else ends the hand-over as every other entry does
  const cice_transport_fields& t = c_->ridge_f;
  const bool handed = c_->ridge_armed && f && f->aice0 == t.aice0 && f->aicen == t.aicen && f->trcrn == t.trcrn &&
                      f->vicen == t.vicen && f->vsnon == t.vsnon && f->eicen == t.eicen && f->esnon == t.esnon;
  if (!handed) c_->end_handover();
  // (handed: from here on a throw leaves the hand-over armed, and the next entry's frame makes a deferred download good)
  CICE_REQUIRE(f && l_stop && istop && jstop && bstop && stage, "NULL argument");
  if (f->ncat == 1) throw Error{CICE_EUNSUPPORTED, "cice_step_ridge: ncat = 1 is not built"};
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_ridge: ncat is not the library's");
  NEED_BATCH(true);
  Halo* halo = nullptr;
  if (f->bound) {
    CICE_REQUIRE(c_->have_domain, "cice_step_ridge: bound = 1 needs cice_domain_create");
    CICE_REQUIRE(c_->batch.same_layout(c_->dom), "cice_step_ridge: the batch does not have the domain's layout");
    c_->need_halo();
    halo = c_->halo.get();
  }
  c_->batch.step_ridge(c_->itd(), c_->have_ridge ? &c_->rp : nullptr, dt, f, handed ? c_->transport.get() : nullptr, halo,
                       l_stop, istop, jstop, bstop, stage);
  if (handed) {                        // consumed: the host arrays hold what this call downloaded
    c_->ridge_armed = false;
    c_->transport->forget_state();
  }
  CICE_CATCH
}

int cice_ridge_times(cice_ctx* ctx, int enable, float ms[41]) {
  static_assert(RIDGE_TIMES == 41, "include/cice4_amd.h");
  CICE_TRY(ctx) c_->batch.ridge_times(enable != 0, ms); CICE_CATCH
}

int cice_ridge_chain_time(cice_ctx* ctx, int enable, float* ms) {
  CICE_TRY(ctx) c_->batch.handover_time(enable != 0, ms); CICE_CATCH
}

int cice_therm2_cleanup_times(cice_ctx* ctx, int enable, float ms[12]) {
  CICE_TRY(ctx) c_->batch.cleanup_times(enable != 0, ms); CICE_CATCH
}

int cice_therm2_itd_times(cice_ctx* ctx, int enable, float ms[4]) {
  CICE_TRY(ctx) c_->batch.itd_times(enable != 0, ms); CICE_CATCH
}

}  // extern "C"
