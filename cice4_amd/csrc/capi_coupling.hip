// C-ABI of libcice4_amd.so: coupling_prep (the mixed layer, the albedo merge, scale_fluxes) on the batch.
#include "capi.h"

extern "C" {

int cice_coupling_init(cice_ctx* ctx, const cice_coupling_config* cfg) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "cice_coupling_init: NULL argument");
  CICE_REQUIRE(c_->have_thermo, "cice_coupling_init: cice_thermo_init has not been called");
  CICE_REQUIRE(cfg->scale_fluxes == 0 || cfg->scale_fluxes == 1, "cice_coupling_init: scale_fluxes must be 0 or 1");
  CICE_REQUIRE(cfg->oceanmixed_ice == 0 || cfg->oceanmixed_ice == 1, "cice_coupling_init: oceanmixed_ice must be 0 or 1");
  CICE_REQUIRE(cfg->atmbndy == 0 || cfg->atmbndy == 1, "cice_coupling_init: atmbndy must be 0 (default) or 1 (constant)");
  if (cfg->atmbndy == 1)
    throw Error{CICE_EUNSUPPORTED, "cice_coupling_init: atmbndy = 'constant' is not built: in that branch ocean_mixed_layer never "
                                   "sets its local arrays delt and delq (ice_ocean.F90:139-150) and then multiplies by them "
                                   "(:207-208)"};
  c_->cp = CouplingParams{cfg->scale_fluxes, cfg->oceanmixed_ice, cfg->albocn};
  c_->have_cpl = true;
  CICE_CATCH
}

int cice_coupling_prep(cice_ctx* ctx, double dt, const cice_coupling_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(f, "cice_coupling_prep: NULL argument");
  CICE_REQUIRE(f->ncat == NCAT, "cice_coupling_prep: ncat is not the library's");
  CICE_REQUIRE(c_->have_cpl, "cice_coupling_prep: cice_coupling_init has not been called");
  CICE_REQUIRE(c_->batch.allocated(), "cice_coupling_prep: cice_thermo_batch_alloc has not been called");
  Halo* halo = nullptr;
  CICE_REQUIRE(f->bound == 0 || f->bound == 1, "cice_coupling_prep: bound must be 0 or 1");
  if (f->bound) {
    CICE_REQUIRE(c_->have_domain, "cice_coupling_prep: bound = 1 needs cice_domain_create");
    CICE_REQUIRE(c_->batch.same_layout(c_->dom), "cice_coupling_prep: the batch does not have the domain's layout");
    c_->need_halo();
    halo = c_->halo.get();
  }
  c_->batch.coupling_prep(&c_->cp, dt, f, halo);
  CICE_CATCH
}

int cice_coupling_times(cice_ctx* ctx, int enable, float ms[2]) {
  CICE_TRY(ctx) c_->batch.coupling_times(enable != 0, ms); CICE_CATCH
}

}  // extern "C"
