// C-ABI of libcice4_amd.so: shortwave radiation (shortwave = 'default'), block-wise and on the batch.
#include "capi.h"

extern "C" {

int cice_shortwave_init(cice_ctx* ctx, const cice_shortwave_config* cfg) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "NULL argument");
  CICE_REQUIRE(c_->have_thermo, "cice_shortwave_init: cice_thermo_init has not been called");
  CICE_REQUIRE(cfg->shortwave == 0 || cfg->shortwave == 1, "cice_shortwave_init: shortwave must be 0 (default) or 1 (dEdd)");
  if (cfg->shortwave == 1)
    throw Error{CICE_EUNSUPPORTED, "cice_shortwave_init: shortwave = 'dEdd' (delta-Eddington) has an entry of its own, "
                                   "cice_shortwave_dedd_init"};
  if (!c_->tp.heat_capacity)
    throw Error{CICE_EUNSUPPORTED, "cice_shortwave_init: heat_capacity = F (absorbed_solar's nilyr = 1 branch) is not built"};
  CICE_REQUIRE(cfg->albedo_type == 0 || cfg->albedo_type == 1, "cice_shortwave_init: albedo_type must be 0 (default) or 1 (constant)");
  CICE_REQUIRE(cfg->ahmax > 0.0, "cice_shortwave_init: ahmax must be positive");
  CICE_REQUIRE(cfg->dT_mlt != 0.0, "cice_shortwave_init: dT_mlt must not be zero");
  ShortwaveParams p{};
  p.albedo_type = cfg->albedo_type;
  p.albicev = cfg->albicev; p.albicei = cfg->albicei; p.albsnowv = cfg->albsnowv; p.albsnowi = cfg->albsnowi;
  p.ahmax = cfg->ahmax;
  p.fhtan = std::atan(cfg->ahmax * K::c4);   // the host libm, as the reference's `fhtan = atan(ahmax*c4)` (:658)
  p.albocn = cfg->albocn; p.dT_mlt = cfg->dT_mlt; p.dalb_mlt = cfg->dalb_mlt; p.snowpatch = cfg->snowpatch;
  p.awtvdr = cfg->awtvdr; p.awtidr = cfg->awtidr; p.awtvdf = cfg->awtvdf; p.awtidf = cfg->awtidf;
  c_->sp = p;
  c_->have_sw = true;
  CICE_CATCH
}

// shortwave_ccsm3 (ice_shortwave.F90:364-541) on one block and category: see include/cice4_amd.h
int cice_shortwave_ccsm3(cice_ctx* ctx, int nx, int ny, int icells, const int32_t* indxi, const int32_t* indxj,
                         const double* aicen, const double* vicen, const double* vsnon, const double* Tsfcn,
                         const double* swvdr, const double* swvdf, const double* swidr, const double* swidf, double* alvdrn,
                         double* alidrn, double* alvdfn, double* alidfn, double* fswsfc, double* fswint, double* fswthru,
                         double* Iswabs, double* albin, double* albsn, const double* ocn_albedo) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(c_->have_sw, "cice_shortwave_init has not been called");
  CICE_REQUIRE(aicen && vicen && vsnon && Tsfcn && swvdr && swvdf && swidr && swidf && alvdrn && alidrn && alvdfn && alidfn &&
                   fswsfc && fswint && fswthru && Iswabs && albin && albsn, "shortwave_ccsm3: NULL argument");
  const std::vector<int32_t> on = list_mask(nx, ny, icells, indxi, indxj);
  const size_t np = on.size();
  c_->need_device();
  // planes of the staging buffer: the nine inputs, the nine outputs, Iswabs
  enum { P_IN = 0, P_OCN = 8, P_OUT = 9, P_ISW = 18, P_PLANES = P_ISW + NILYR };
  if (c_->sw_d.n < P_PLANES * np) c_->sw_d.alloc(P_PLANES * np);
  if (c_->sw_i.n < np) c_->sw_i.alloc(np);
  hipStream_t s = c_->stream;
  auto pl = [&](int k) { return c_->sw_d.p + (size_t)k * np; };
  CICE_HIP(hipMemcpyAsync(c_->sw_i.p, on.data(), np * 4, hipMemcpyHostToDevice, s));
  const double* in[9] = {aicen, vicen, vsnon, Tsfcn, swvdr, swvdf, swidr, swidf, ocn_albedo};
  for (int k = 0; k < 9; ++k)
    if (in[k]) CICE_HIP(hipMemcpyAsync(pl(P_IN + k), in[k], np * 8, hipMemcpyHostToDevice, s));
  ShortwaveArgs a{};
  a.p = c_->sp;
  a.nx = nx; a.np = (int)np; a.ncat = 1; a.nb = 1; a.tsfc_planes = 1;
  a.listed = c_->sw_i.p;
  a.aicen = pl(0); a.vicen = pl(1); a.vsnon = pl(2); a.Tsfc = pl(3);
  a.swvdr = pl(4); a.swvdf = pl(5); a.swidr = pl(6); a.swidf = pl(7);
  a.ocn_albedo = ocn_albedo ? pl(P_OCN) : nullptr;
  double* out[9] = {alvdrn, alidrn, alvdfn, alidfn, fswsfc, fswint, fswthru, albin, albsn};
  a.alvdrn = pl(P_OUT); a.alidrn = pl(P_OUT + 1); a.alvdfn = pl(P_OUT + 2); a.alidfn = pl(P_OUT + 3);
  a.fswsfcn = pl(P_OUT + 4); a.fswintn = pl(P_OUT + 5); a.fswthrun = pl(P_OUT + 6);
  a.albicen = pl(P_OUT + 7); a.albsnon = pl(P_OUT + 8);
  a.Iswabsn = pl(P_ISW); a.Sswabsn = nullptr;   // (Sswabsn is the caller's: `Sswabsn(:,:,sl1:sl2,iblk) = c0` in front of the call)
  shortwave_launch(a, s);
  for (int k = 0; k < 9; ++k) CICE_HIP(hipMemcpyAsync(out[k], pl(P_OUT + k), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(Iswabs, pl(P_ISW), (size_t)NILYR * np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));     // (`on` is a local)
  CICE_CATCH
}

int cice_step_radiation(cice_ctx* ctx, const cice_radiation_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f, "NULL argument");
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_radiation: ncat is not the library's");
  NEED_BATCH(true);
  c_->batch.step_radiation(c_->thermo(), c_->have_sw ? &c_->sp : nullptr, f);
  CICE_CATCH
}

int cice_prep_radiation(cice_ctx* ctx, const cice_prep_radiation_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f, "NULL argument");
  CICE_REQUIRE(f->ncat == NCAT, "cice_prep_radiation: ncat is not the library's");
  NEED_BATCH(true);
  c_->batch.prep_radiation(c_->thermo(), f);
  CICE_CATCH
}

int cice_radiation_chain(cice_ctx* ctx, int mode) {
  CICE_TRY(ctx) c_->batch.radiation_chain(mode); CICE_CATCH
}

int cice_radiation_times(cice_ctx* ctx, int enable, float ms[2]) {
  CICE_TRY(ctx) c_->batch.radiation_times(enable != 0, ms); CICE_CATCH
}

}  // extern "C"
