// C-ABI of libcice4_amd.so: horizontal transport (remap, upwind) and the evp -> transport chain.
#include "capi.h"

extern "C" {

// ---- horizontal transport ---------------------------------------------------------------------
int cice_transport_init(cice_ctx* ctx, const cice_transport_config* cfg, const cice_transport_grid* grid) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg && grid, "NULL argument");
  c_->need_halo();
  c_->transport.reset(new Transport(c_->dom, *c_->halo, c_->stream, c_->fan));
  c_->transport->init(*cfg, *grid);
  CICE_CATCH
}

int cice_transport_remap(cice_ctx* ctx, double dt, const cice_transport_fields* f, int32_t* l_stop,
                         int32_t* istop, int32_t* jstop) {
  CICE_TRY(ctx)
  CICE_REQUIRE(c_->transport != nullptr, "cice_transport_init has not been called");
  CICE_REQUIRE(f, "NULL argument");
  if (c_->chain_on && c_->chain_ready && c_->evp && f->aice0 == c_->chain.aice0 && f->trcrn == c_->chain.trcrn &&
      f->vsnon == c_->chain.vsnon && f->eicen == c_->chain.eicen && f->esnon == c_->chain.esnon &&
      f->aicen == c_->chain_aicen && f->vicen == c_->chain_vicen && f->uvel == c_->chain_u && f->vvel == c_->chain_v)
    c_->transport->adopt(c_->evp->d_uv(), c_->evp->d_aicen(), c_->evp->d_vicen());
  c_->chain_ready = false;
  // transport -> ridging hand-over: what cice_step_ridge will need to take this call's result from the device
  const bool can_arm = c_->ridge_mode != 0 && c_->have_itd && c_->have_ridge && c_->batch.allocated() &&
                       c_->batch.same_layout(c_->dom) && c_->transport->same_tracers(c_->ip.ntrcr, c_->ip.dep);
  c_->transport->defer_download = can_arm && c_->ridge_mode == 2;
  int32_t stop = 0;
  c_->transport->remap(dt, *f, &stop, istop, jstop);
  if (l_stop) *l_stop = stop;
  if (can_arm && stop == 0 && c_->transport->state_ready()) {
    c_->ridge_f = *f;
    c_->ridge_armed = true;
  }
  CICE_CATCH
}

int cice_ridge_chain(cice_ctx* ctx, int mode) {
  CICE_TRY(ctx)
  CICE_REQUIRE(mode >= 0 && mode <= 2, "cice_ridge_chain: mode must be 0, 1 or 2");
  c_->ridge_mode = mode;
  CICE_CATCH
}

int cice_transport_download_state(cice_ctx* ctx) {
  CICE_TRY(ctx)   // (the frame has done it)
  CICE_CATCH
}

int cice_transport_chain(cice_ctx* ctx, const cice_transport_fields* f) {
  CICE_TRY(ctx)
  c_->chain_ready = false;
  c_->chain_on = false;
  if (f) {
    CICE_REQUIRE(c_->transport != nullptr, "cice_transport_chain: cice_transport_init has not been called");
    CICE_REQUIRE(f->aice0 && f->aicen && f->trcrn && f->vicen && f->vsnon && f->eicen && f->esnon && f->uvel && f->vvel,
                 "cice_transport_chain: NULL field");
    c_->chain = *f;
    c_->chain_on = true;
  }
  CICE_CATCH
}

int cice_transport_upwind_init(cice_ctx* ctx, const cice_transport_config* cfg, int nt_Tsfc, const double* HTE,
                               const double* HTN, const double* tarea) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg, "NULL argument");
  c_->need_halo();
  c_->upwind.reset(new Upwind(c_->dom, *c_->halo, c_->stream, c_->fan));
  c_->upwind->init(*cfg, nt_Tsfc, HTE, HTN, tarea);
  CICE_CATCH
}

int cice_transport_upwind(cice_ctx* ctx, double dt, const cice_transport_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false;
  CICE_REQUIRE(c_->upwind != nullptr, "cice_transport_upwind_init has not been called");
  CICE_REQUIRE(f, "NULL argument");
  c_->upwind->step(dt, *f);
  CICE_CATCH
}

// test aid (not part of the drop-in surface): see Transport::debug_stop / debug_fetch
int cice_transport_debug(cice_ctx* ctx, int stop_stage, int which, double* out, long long* count) {
  CICE_TRY(ctx)
  CICE_REQUIRE(c_->transport != nullptr, "cice_transport_init has not been called");
  c_->transport->debug_stop(stop_stage);
  const size_t n = which >= 0 ? c_->transport->debug_fetch(which, out) : 0;
  if (count) *count = (long long)n;
  CICE_CATCH
}

}  // extern "C"
