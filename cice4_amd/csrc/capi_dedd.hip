// C-ABI of libcice4_amd.so: shortwave radiation, shortwave = 'dEdd' (delta-Eddington), block-wise and on the batch.
#include "capi.h"

extern "C" {

int cice_shortwave_dedd_init(cice_ctx* ctx, const cice_dedd_config* cfg) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "NULL argument");
  CICE_REQUIRE(c_->have_thermo, "cice_shortwave_dedd_init: cice_thermo_init has not been called");
  if (!c_->tp.heat_capacity)
    throw Error{CICE_EUNSUPPORTED, "cice_shortwave_dedd_init: heat_capacity = F (compute_dEdd's nilyr = 1 branch) is not built"};
  CICE_REQUIRE(cfg->tr_pond == 0 || cfg->tr_pond == 1, "cice_shortwave_dedd_init: tr_pond must be 0 or 1");
  CICE_REQUIRE(std::isfinite(cfg->R_ice) && std::isfinite(cfg->R_pnd) && std::isfinite(cfg->R_snw),
               "cice_shortwave_dedd_init: R_ice, R_pnd, R_snw must be finite");
  DeddParams p{};
  p.tr_pond = cfg->tr_pond;
  p.R_snw = cfg->R_snw;
  p.awtvdr = cfg->awtvdr; p.awtidr = cfg->awtidr; p.awtvdf = cfg->awtvdf; p.awtidf = cfg->awtidf;
  p.exp_min = std::exp(-10.0);             // the host libm, as the reference's `exp_min = exp(-argmax)` (:1267)
  dedd_tune(p, cfg->R_ice, cfg->R_pnd);
  c_->dp = p;
  c_->have_dedd = true;
  CICE_CATCH
}

// shortwave_dEdd (ice_shortwave.F90:1372-1787) on one block and category: see include/cice4_amd.h
int cice_shortwave_dEdd(cice_ctx* ctx, int nx, int ny, int icells, const int32_t* indxi, const int32_t* indxj,
                        const double* coszen, const double* aice, const double* vice, const double* vsno, const double* fs,
                        const double* rhosnw, const double* rsnw, const double* fp, const double* hp, const double* swvdr,
                        const double* swvdf, const double* swidr, const double* swidf, double* alvdr, double* alvdf,
                        double* alidr, double* alidf, double* fswsfc, double* fswint, double* fswthru, double* Sswabs,
                        double* Iswabs, double* albice, double* albsno, double* albpnd) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(c_->have_dedd, "cice_shortwave_dedd_init has not been called");
  CICE_REQUIRE(coszen && aice && vice && vsno && fs && rhosnw && rsnw && fp && hp && swvdr && swvdf && swidr && swidf && alvdr &&
                   alvdf && alidr && alidf && fswsfc && fswint && fswthru && Sswabs && Iswabs && albice && albsno && albpnd,
               "shortwave_dEdd: NULL argument");
  const std::vector<int32_t> on = list_mask(nx, ny, icells, indxi, indxj);
  const size_t np = on.size();
  c_->need_device();
  // planes of the staging buffer: the inputs in argument order (rhosnw, rsnw nslyr planes each), then the outputs
  enum { P_COSZEN = 0, P_AICE, P_VICE, P_VSNO, P_FS, P_RHOSNW, P_RSNW = P_RHOSNW + NSLYR, P_FP = P_RSNW + NSLYR, P_HP, P_SW,
         P_OUT = P_SW + 4, P_SSW = P_OUT + 7, P_ISW = P_SSW + NSLYR, P_HIST = P_ISW + NILYR, P_PLANES = P_HIST + 3 };
  if (c_->dedd_d.n < P_PLANES * np) c_->dedd_d.alloc(P_PLANES * np);
  if (c_->dedd_i.n < np) c_->dedd_i.alloc(np);
  hipStream_t s = c_->stream;
  auto pl = [&](int k) { return c_->dedd_d.p + (size_t)k * np; };
  CICE_HIP(hipMemcpyAsync(c_->dedd_i.p, on.data(), np * 4, hipMemcpyHostToDevice, s));
  const struct { const double* h; int plane, planes; } in[] = {
      {coszen, P_COSZEN, 1}, {aice, P_AICE, 1}, {vice, P_VICE, 1}, {vsno, P_VSNO, 1}, {fs, P_FS, 1},
      {rhosnw, P_RHOSNW, NSLYR}, {rsnw, P_RSNW, NSLYR}, {fp, P_FP, 1}, {hp, P_HP, 1},
      {swvdr, P_SW, 1}, {swvdf, P_SW + 1, 1}, {swidr, P_SW + 2, 1}, {swidf, P_SW + 3, 1}};
  for (const auto& e : in) CICE_HIP(hipMemcpyAsync(pl(e.plane), e.h, (size_t)e.planes * np * 8, hipMemcpyHostToDevice, s));
  DeddArgs a{};
  a.p = c_->dp;
  a.nx = nx; a.np = (int)np; a.ncat = 1; a.nb = 1; a.tsfc_planes = 1; a.snow_given = 1;
  a.listed = c_->dedd_i.p;
  a.coszen = pl(P_COSZEN); a.aicen = pl(P_AICE); a.vicen = pl(P_VICE); a.vsnon = pl(P_VSNO);
  a.fs = pl(P_FS); a.rhosnw = pl(P_RHOSNW); a.rsnw = pl(P_RSNW); a.fp = pl(P_FP); a.hp = pl(P_HP);
  a.swvdr = pl(P_SW); a.swvdf = pl(P_SW + 1); a.swidr = pl(P_SW + 2); a.swidf = pl(P_SW + 3);
  a.alvdrn = pl(P_OUT); a.alvdfn = pl(P_OUT + 1); a.alidrn = pl(P_OUT + 2); a.alidfn = pl(P_OUT + 3);
  a.fswsfcn = pl(P_OUT + 4); a.fswintn = pl(P_OUT + 5); a.fswthrun = pl(P_OUT + 6);
  a.Sswabsn = pl(P_SSW); a.Iswabsn = pl(P_ISW);
  a.albicen = pl(P_HIST); a.albsnon = pl(P_HIST + 1); a.albpndn = pl(P_HIST + 2);
  dedd_launch(a, s);
  double* out[7] = {alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru};
  for (int k = 0; k < 7; ++k) CICE_HIP(hipMemcpyAsync(out[k], pl(P_OUT + k), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(Sswabs, pl(P_SSW), (size_t)NSLYR * np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipMemcpyAsync(Iswabs, pl(P_ISW), (size_t)NILYR * np * 8, hipMemcpyDeviceToHost, s));
  double* hist[3] = {albice, albsno, albpnd};
  for (int k = 0; k < 3; ++k) CICE_HIP(hipMemcpyAsync(hist[k], pl(P_HIST + k), np * 8, hipMemcpyDeviceToHost, s));
  CICE_HIP(hipStreamSynchronize(s));     // (`on` is a local)
  CICE_CATCH
}

int cice_step_radiation_dedd(cice_ctx* ctx, const cice_radiation_dedd_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f, "NULL argument");
  CICE_REQUIRE(f->ncat == NCAT, "cice_step_radiation_dedd: ncat is not the library's");
  NEED_BATCH(true);
  c_->batch.step_radiation_dedd(c_->thermo(), c_->have_dedd ? &c_->dp : nullptr, f);
  CICE_CATCH
}

int cice_dedd_times(cice_ctx* ctx, int enable, float ms[1]) {
  CICE_TRY(ctx) c_->batch.dedd_times(enable != 0, ms); CICE_CATCH
}

}  // extern "C"
