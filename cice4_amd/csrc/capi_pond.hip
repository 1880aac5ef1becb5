// C-ABI of libcice4_amd.so: melt ponds and ice age (compute_ponds, increment_age), block-wise and on the batch.
#include "capi.h"

namespace {

// nt_volpn against what cice_thermo_init holds now (that call may have been repeated since cice_pond_init)
void check_slot(const cice_ctx* c, int nt_volpn, const char* entry) {
  const std::string e(entry);
  CICE_REQUIRE(nt_volpn >= 0 && nt_volpn <= NTRCR, e + ": nt_volpn out of range");
  CICE_REQUIRE(nt_volpn == 0 || nt_volpn != c->tp.nt_Tsfc, e + ": nt_volpn is nt_Tsfc");
  CICE_REQUIRE(nt_volpn == 0 || !c->tp.tr_iage || nt_volpn != c->tp.nt_iage, e + ": nt_volpn is nt_iage");
}

}  // namespace

extern "C" {

int cice_pond_init(cice_ctx* ctx, int nt_volpn) {
  CICE_TRY(ctx)
  CICE_REQUIRE(c_->have_thermo, "cice_pond_init: cice_thermo_init has not been called");
  check_slot(c_, nt_volpn, "cice_pond_init");
  CICE_REQUIRE(!c_->tp.tr_iage || (c_->tp.nt_iage >= 1 && c_->tp.nt_iage <= NTRCR && c_->tp.nt_iage != c_->tp.nt_Tsfc),
               "cice_pond_init: tr_iage with an nt_iage that is out of range or nt_Tsfc");
  c_->nt_volpn = nt_volpn;
  c_->have_pond = true;
  CICE_CATCH
}

// compute_ponds (ice_meltpond.F90:88-229) on one block and category: see include/cice4_amd.h
int cice_compute_ponds(cice_ctx* ctx, int nx, int ny, int ilo, int ihi, int jlo, int jhi, double dt, const double* meltt,
                       const double* melts, const double* frain, const double* aicen, const double* vicen,
                       const double* vsnon, double* trcrn, double* apondn, double* hpondn) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(c_->have_pond, "cice_compute_ponds: cice_pond_init has not been called");
  check_slot(c_, c_->nt_volpn, "cice_compute_ponds");
  CICE_REQUIRE(c_->nt_volpn >= 1, "cice_compute_ponds: cice_pond_init was given no pond tracer");
  CICE_REQUIRE(nx >= 1 && ny >= 1 && ilo >= 1 && ihi <= nx && jlo >= 1 && jhi <= ny, "cice_compute_ponds: bad dimensions");
  CICE_REQUIRE(meltt && melts && frain && aicen && vicen && vsnon && trcrn && apondn && hpondn,
               "cice_compute_ponds: NULL argument");
  c_->need_device();
  const size_t np = (size_t)nx * ny;
  // planes of the staging buffer: the inputs in argument order, the two tracer planes, apondn, hpondn
  enum { P_MELTT = 0, P_MELTS, P_FRAIN, P_AICEN, P_VICEN, P_VSNON, P_TSFC, P_VOLPN, P_APOND, P_HPOND, P_PLANES };
  if (c_->pond_d.n < P_PLANES * np) c_->pond_d.alloc(P_PLANES * np);
  if (c_->pond_i.n < np + 4) c_->pond_i.alloc(np + 4);
  hipStream_t s = c_->stream;
  auto pl = [&](int k) { return c_->pond_d.p + (size_t)k * np; };
  const int32_t blk[4] = {ilo, ihi, jlo, jhi};
  CICE_HIP(hipMemcpyAsync(c_->pond_i.p, blk, sizeof(blk), hipMemcpyHostToDevice, s));
  double* const volpn = trcrn + (size_t)(c_->nt_volpn - 1) * np;
  const double* in[P_PLANES] = {meltt, melts, frain, aicen, vicen, vsnon, trcrn + (size_t)(c_->tp.nt_Tsfc - 1) * np, volpn,
                                apondn, hpondn};
  for (int k = 0; k < P_PLANES; ++k) CICE_HIP(hipMemcpyAsync(pl(k), in[k], np * 8, hipMemcpyHostToDevice, s));
  PondArgs a{};
  a.nx = nx; a.np = (int)np; a.ncat = 1; a.nb = 1; a.ponds = 1; a.age = 0; a.dt = dt;
  a.tsfc_planes = 1; a.volpn_planes = 1; a.iage_planes = 1;
  a.blk = c_->pond_i.p;
  a.aicen = pl(P_AICEN); a.vicen = pl(P_VICEN); a.vsnon = pl(P_VSNON); a.Tsfc = pl(P_TSFC);
  a.meltt = pl(P_MELTT); a.melts = pl(P_MELTS); a.frain = pl(P_FRAIN);
  a.volpn = pl(P_VOLPN); a.apondn = pl(P_APOND); a.hpondn = pl(P_HPOND);
  pond_launch(a, s);
  CICE_HIP(hipMemcpyAsync(volpn, pl(P_VOLPN), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(apondn, pl(P_APOND), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(hpondn, pl(P_HPOND), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));     // (`blk` is a local)
  CICE_CATCH
}

// increment_age (ice_age.F90:87-123) on one block and category, on the caller's list
int cice_increment_age(cice_ctx* ctx, int nx, int ny, double dt, int icells, const int32_t* indxi, const int32_t* indxj,
                       double* iage) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(iage, "cice_increment_age: NULL argument");
  const std::vector<int32_t> on = list_mask(nx, ny, icells, indxi, indxj, true);
  const size_t np = on.size();
  c_->need_device();
  if (c_->pond_d.n < np) c_->pond_d.alloc(np);
  if (c_->pond_i.n < np + 4) c_->pond_i.alloc(np + 4);
  hipStream_t s = c_->stream;
  CICE_HIP(hipMemcpyAsync(c_->pond_i.p + 4, on.data(), np * 4, hipMemcpyHostToDevice, s));
  CICE_HIP(hipMemcpyAsync(c_->pond_d.p, iage, np * 8, hipMemcpyHostToDevice, s));
  PondArgs a{};
  a.nx = nx; a.np = (int)np; a.ncat = 1; a.nb = 1; a.ponds = 0; a.age = 1; a.dt = dt;
  a.tsfc_planes = 1; a.volpn_planes = 1; a.iage_planes = 1;
  a.listed = c_->pond_i.p + 4;
  a.iage = c_->pond_d.p;
  pond_launch(a, s);
  CICE_HIP(hipMemcpyAsync(iage, c_->pond_d.p, np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));     // (`on` is a local)
  CICE_CATCH
}

int cice_step_ponds(cice_ctx* ctx, double dt, const cice_pond_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f, "cice_step_ponds: NULL argument");
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_ponds: ncat is not the library's");
  CICE_REQUIRE(c_->have_pond && c_->have_thermo, "cice_step_ponds: cice_pond_init has not been called");
  check_slot(c_, c_->nt_volpn, "cice_step_ponds");
  CICE_REQUIRE(f->state_resident == 0 || f->state_resident == 1, "cice_step_ponds: state_resident must be 0 or 1");
  CICE_REQUIRE((f->ponds == 0 || f->ponds == 1) && (f->age == 0 || f->age == 1) && (f->ponds || f->age),
               "cice_step_ponds: ponds and age must be 0 or 1, and not both 0");
  CICE_REQUIRE(!f->ponds || c_->nt_volpn >= 1, "cice_step_ponds: ponds = 1, but cice_pond_init was given no pond tracer");
  CICE_REQUIRE(!f->age || c_->tp.tr_iage, "cice_step_ponds: age = 1, but cice_thermo_init was given tr_iage = 0");
  CICE_REQUIRE(!f->age || (c_->tp.nt_iage >= 1 && c_->tp.nt_iage <= NTRCR), "cice_step_ponds: nt_iage out of range");
  bool ok = f->trcrn != nullptr;
  if (f->ponds) ok = ok && f->frain && f->apondn && f->hpondn;
  if (!f->state_resident) ok = ok && f->aicen && (!f->ponds || (f->vicen && f->vsnon && f->melttn && f->meltsn));
  CICE_REQUIRE(ok, "cice_step_ponds: NULL field");
  CICE_REQUIRE(c_->batch.allocated(), "cice_step_ponds: cice_thermo_batch_alloc has not been called");
  c_->batch.step_ponds(c_->thermo(), c_->nt_volpn, dt, f);
  CICE_CATCH
}

int cice_pond_times(cice_ctx* ctx, int enable, float ms[1]) {
  CICE_TRY(ctx) c_->batch.pond_times(enable != 0, ms); CICE_CATCH
}

int cice_pond_chain(cice_ctx* ctx, int mode) {
  CICE_TRY(ctx) c_->batch.pond_chain(mode); CICE_CATCH
}

}  // extern "C"
