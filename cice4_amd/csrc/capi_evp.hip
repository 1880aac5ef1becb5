// C-ABI of libcice4_amd.so: the EVP dynamics, the peer connections of its one-launch loop, and its host-only test aids.
#include "capi.h"

extern "C" {

// ---- EVP -------------------------------------------------------------------------------------
int cice_evp_init(cice_ctx* ctx, const cice_evp_config* cfg, const cice_evp_grid* grid) {
  CICE_TRY(ctx)
  CICE_REQUIRE(cfg && grid, "NULL argument");
  c_->need_halo();
  c_->evp.reset(new Evp(c_->dom, *c_->halo, c_->stream, c_->fan));
  c_->evp->init(*cfg, *grid);
  CICE_CATCH
}

int cice_evp_upload(cice_ctx* ctx, const cice_evp_fields* f) {
  CICE_TRY(ctx) c_->chain_ready = false; NEED_EVP; CICE_REQUIRE(f, "NULL argument"); c_->evp->upload(*f); CICE_CATCH
}
int cice_evp_download(cice_ctx* ctx, cice_evp_fields* f) {
  CICE_TRY(ctx) NEED_EVP; CICE_REQUIRE(f, "NULL argument"); c_->evp->download(*f); CICE_CATCH
}
int cice_evp_step(cice_ctx* ctx, double dt) { CICE_TRY(ctx) c_->chain_ready = false; NEED_EVP; c_->evp->forget_host_state(); c_->evp->step(dt); CICE_CATCH }
int cice_evp(cice_ctx* ctx, double dt, cice_evp_fields* f) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(f, "NULL argument");
  c_->chain_ready = false;
  const bool chain = c_->chain_on && c_->transport;
  c_->evp->run(dt, *f, [&]() {
    if (!chain) return;
    // the rest of the transport's state travels while the subcycle loop runs (the link idles then); see cice_transport_chain
    c_->transport->prefetch(c_->chain);
    c_->chain_aicen = f->aicen; c_->chain_vicen = f->vicen; c_->chain_u = f->uvel; c_->chain_v = f->vvel;
  });
  c_->chain_ready = chain;   // only a call that got this far leaves device copies the transport may take over
  CICE_CATCH
}
// f1 hand-off: the state the batched thermodynamic step left on the device becomes the dynamics' input without crossing
// PCIe (valid when nothing on the host has changed aicen / vicen / vsnon since: the caller's statement).
int cice_evp_adopt_thermo_state(cice_ctx* ctx) {
  CICE_TRY(ctx) c_->chain_ready = false;
  NEED_EVP;
  NEED_BATCH(true);
  CICE_REQUIRE(c_->batch.same_layout(c_->dom),
               "cice_evp_adopt_thermo_state: the thermodynamic batch has another block layout than the dynamics");
  c_->evp->adopt_state(c_->batch.aicen(), c_->batch.vicen(), c_->batch.vsnon());
  CICE_CATCH
}
int cice_evp_pin_fields(cice_ctx* ctx, const cice_evp_fields* f) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(f, "NULL argument");
  const size_t n = (size_t)c_->dom.nblocks() * c_->dom.nx_block * c_->dom.ny_block;
  auto pin = [&](const void* h, size_t bytes) { c_->pin_range(h, bytes); };
  const double* r8[] = {f->aice, f->vice, f->vsno, f->aice0, f->strairxT, f->strairyT, f->uocn, f->vocn,
                        f->ss_tltx, f->ss_tlty, f->uvel, f->vvel, f->stressp_1, f->stressp_2, f->stressp_3,
                        f->stressp_4, f->stressm_1, f->stressm_2, f->stressm_3, f->stressm_4, f->stress12_1,
                        f->stress12_2, f->stress12_3, f->stress12_4, f->fm, f->strtltx, f->strtlty, f->strocnx,
                        f->strocny, f->strintx, f->strinty, f->strairx, f->strairy, f->strength, f->divu,
                        f->shear, f->rdg_conv, f->rdg_shear, f->prs_sig, f->strocnxT, f->strocnyT};
  for (const double* h : r8) pin(h, n * 8);
  pin(f->aicen, n * NCAT * 8);
  pin(f->vicen, n * NCAT * 8);
  pin(f->iceumask, n * 4);
  CICE_CATCH
}
int cice_evp_prepare(cice_ctx* ctx, double dt) { CICE_TRY(ctx) c_->chain_ready = false; NEED_EVP; c_->evp->forget_host_state(); c_->evp->prepare(dt); CICE_CATCH }
int cice_evp_subcycles(cice_ctx* ctx, int ksub0, int nsub, float* ms) {
  CICE_TRY_QUEUED(ctx) c_->chain_ready = false; NEED_EVP; c_->evp->forget_host_state(); c_->evp->subcycles(ksub0, nsub, ms); CICE_CATCH
}
int cice_evp_finish(cice_ctx* ctx) { CICE_TRY(ctx) c_->chain_ready = false; NEED_EVP; c_->evp->forget_host_state(); c_->evp->finish(); CICE_CATCH }
int cice_evp_download_stresses(cice_ctx* ctx, cice_evp_fields* f) {
  CICE_TRY(ctx) NEED_EVP; CICE_REQUIRE(f, "NULL argument"); c_->evp->download_stresses(*f); CICE_CATCH
}
int cice_evp_set_option(cice_ctx* ctx, const char* key, int value) {
  CICE_TRY(ctx) NEED_EVP; CICE_REQUIRE(key, "NULL key"); c_->evp->set_option(key, value); CICE_CATCH
}
int cice_evp_get_info(cice_ctx* ctx, const char* key, int* value) {
  CICE_TRY_QUEUED(ctx)
  NEED_EVP;
  CICE_REQUIRE(key && value, "NULL argument");
  if (!std::strcmp(key, "resident_pending")) {   // one-launch loops queued whose outcome nobody has looked at yet
    *value = c_->evp->resident_pending();
    return CICE_OK;
  }
  c_->evp->retire_resident();   // (every other key describes the object as a wait behind every loop would have left it)
  if (!std::strcmp(key, "derive_metrics")) *value = c_->evp->derives_metrics() ? 1 : 0;
  else if (!std::strcmp(key, "waves")) *value = c_->evp->tile_waves();
  else if (!std::strcmp(key, "rows_per_wave")) *value = c_->evp->tile_rows();
  else if (!std::strcmp(key, "fused")) *value = c_->evp->can_fuse() ? 1 : 0;
  else if (!std::strcmp(key, "fused_waves")) *value = c_->evp->fused_waves();
  else if (!std::strcmp(key, "skew")) *value = c_->evp->can_skew() || c_->evp->can_skew_fold() ? 1 : 0;
  else if (!std::strcmp(key, "skew_fold")) *value = (!c_->evp->can_skew() && c_->evp->can_skew_fold()) || c_->evp->skew_joined_fold() ? 1 : 0;
  else if (!std::strcmp(key, "skew_joined")) *value = c_->evp->skew_joined() ? 1 : 0;
  else if (!std::strcmp(key, "skew_join_fold")) *value = c_->evp->join_fold_option() ? 1 : 0;
  else if (!std::strcmp(key, "skew_levels")) *value = c_->evp->skew_levels();
  else if (!std::strcmp(key, "skew_subs")) *value = c_->evp->skew_subs(c_->evp->skew_levels());
  else if (!std::strcmp(key, "skew_pairs")) *value = c_->evp->pairs_ok() ? 1 : 0;
  else if (!std::strcmp(key, "skew_fill")) *value = c_->evp->skew_rows_on() ? c_->evp->skew_fill_pct() : 0;
  else if (!std::strcmp(key, "resident_map")) *value = c_->evp->resident_map();
  else if (!std::strcmp(key, "skew_rowact")) *value = c_->evp->rowact_on() ? 1 : 0;
  else if (!std::strcmp(key, "skew_balance")) *value = c_->evp->skew_rows_on() && c_->evp->balance_on() ? 1 : 0;
  else if (!std::strcmp(key, "skew_balanced")) *value = (int)std::min<long long>(c_->evp->balanced_sweeps(), 2000000000LL);
  else if (!std::strcmp(key, "skew_trim_ext")) *value = (c_->evp->can_skew() && c_->evp->can_trim()) ? 1 : 0;
  else if (!std::strcmp(key, "skew_split")) *value = (c_->evp->can_skew() && c_->evp->can_split()) ? 1 : 0;
  else if (!std::strcmp(key, "skew_strips")) *value = c_->evp->skew_strips(c_->evp->skew_levels(), nullptr);
  else if (!std::strcmp(key, "skew_seg_rows")) *value = c_->evp->skew_seg_rows(c_->evp->skew_levels());
  else if (!std::strcmp(key, "resident")) *value = (c_->evp->can_reside() || c_->evp->can_reside_peer()) ? 1 : 0;
  else if (!std::strcmp(key, "resident_peer")) *value = c_->evp->can_reside_peer() ? 1 : 0;
  else if (!std::strcmp(key, "last_launches")) *value = c_->evp->last_launches;
  else if (!std::strcmp(key, "resident_peer_fine")) *value = c_->evp->peer_buffers_fine() ? 1 : 0;
#ifdef CICE4_AMD_EXPERIMENTS
  else if (!std::strcmp(key, "experiments")) *value = 1;
#else
  else if (!std::strcmp(key, "experiments")) *value = 0;     // (the variants measured slower are not in this build: evp.hip)
#endif
  else if (!std::strcmp(key, "resident_granules")) *value = c_->evp->granules_in_use() ? 1 : 0;
  else if (!std::strcmp(key, "resident_waves")) *value = c_->evp->resident_waves();
  else if (!std::strcmp(key, "resident_dense")) *value = c_->evp->can_reside() && c_->evp->resident_dense() ? 1 : 0;
  else throw Error{CICE_EINVAL, std::string("unknown info key ") + key};
  CICE_CATCH
}
int cice_evp_peer_export(cice_ctx* ctx, void* bufs[3], long long* plane) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(bufs && plane, "NULL argument");
  c_->evp->peer_export(bufs);
  *plane = (long long)c_->dom.nblocks() * c_->dom.nx_block * c_->dom.ny_block;
  CICE_CATCH
}
int cice_evp_peer_connect(cice_ctx* ctx, int side, void* xu0, void* xu1, void* rprog, long long plane) {
  CICE_TRY(ctx) NEED_EVP; c_->evp->peer_connect(side, xu0, xu1, rprog, plane); CICE_CATCH
}
// Any cartesian layout with one block per rank (round 5): the ranks this rank's block exchanges ghost cells with, and the
// connection of one of them by its rank.
int cice_evp_peer_ranks(cice_ctx* ctx, int* n, int32_t ranks[8]) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(n && ranks, "NULL argument");
  const std::vector<int> v = c_->evp->peer_ranks();
  CICE_REQUIRE(v.size() <= 8, "cice_evp_peer_ranks: more than eight neighbouring ranks");
  *n = (int)v.size();
  for (size_t k = 0; k < v.size(); ++k) ranks[k] = v[k];
  CICE_CATCH
}
int cice_evp_peer_connect_rank(cice_ctx* ctx, int rank, void* xu0, void* xu1, void* rprog, long long plane) {
  CICE_TRY(ctx) NEED_EVP; c_->evp->peer_connect_rank(rank, xu0, xu1, rprog, plane); CICE_CATCH
}
static void ipc_open(const char handles[3][64], void* p[3]) {
  for (int k = 0; k < 3; ++k) {
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles[k], 64);
    CICE_HIP(hipIpcOpenMemHandle(&p[k], h, hipIpcMemLazyEnablePeerAccess));
  }
}
int cice_evp_peer_connect_rank_ipc(cice_ctx* ctx, int rank, const char handles[3][64], long long plane) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(handles, "NULL argument");
  void* p[3];
  ipc_open(handles, p);
  c_->evp->peer_connect_rank(rank, p[0], p[1], p[2], plane);
  CICE_CATCH
}
// The same buffers as IPC handles (3 x 64 bytes) for a neighbour in ANOTHER process, and their opening on the other
// side.  (Across processes / GPUs; not exercised on the one-GPU test boxes, where two contexts of one process exchange
// plain pointers.)
int cice_evp_peer_export_ipc(cice_ctx* ctx, char handles[3][64], long long* plane) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(handles && plane, "NULL argument");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
  void* bufs[3];
  c_->evp->peer_export(bufs);
  for (int k = 0; k < 3; ++k) CICE_HIP(hipIpcGetMemHandle((hipIpcMemHandle_t*)handles[k], bufs[k]));
  *plane = (long long)c_->dom.nblocks() * c_->dom.nx_block * c_->dom.ny_block;
  CICE_CATCH
}
int cice_evp_peer_connect_ipc(cice_ctx* ctx, int side, const char handles[3][64], long long plane) {
  CICE_TRY(ctx)
  NEED_EVP;
  CICE_REQUIRE(handles, "NULL argument");
  void* p[3];
  ipc_open(handles, p);
  c_->evp->peer_connect(side, p[0], p[1], p[2], plane);
  CICE_CATCH
}
int cice_evp_debug(cice_ctx* ctx, const char* what, long long* out, long long* count) {
  CICE_TRY(ctx)
  CICE_REQUIRE(what && count, "NULL argument");
  const long long nw = c_->batch.debug_read(what, out, *count);   // "thermo_niter", "thermo_perm": the column batch's
  if (nw >= 0) {
    *count = nw;
    return CICE_OK;
  }
  NEED_EVP;
  *count = c_->evp->debug_read(what, out, *count);
  CICE_CATCH
}
int cice_evp_active_cells(cice_ctx* ctx, long long* nt, long long* nu) {
  CICE_TRY(ctx) NEED_EVP; c_->evp->active_cells(nt, nu); CICE_CATCH
}

int cice_evp_stress(cice_ctx* ctx, double dt, int ndte, int damping, int nx, int ny, int ksub,
                    int icellt, const int32_t* ti, const int32_t* tj, const double* uvel,
                    const double* vvel, const double* dxt, const double* dyt, const double* dxhy,
                    const double* dyhx, const double* cxp, const double* cyp, const double* cxm,
                    const double* cym, const double* tarear, const double* tinyarea,
                    const double* strength, double* sp1, double* sp2, double* sp3, double* sp4,
                    double* sm1, double* sm2, double* sm3, double* sm4, double* s121, double* s122,
                    double* s123, double* s124, double* shear, double* divu, double* prs_sig,
                    double* rdg_conv, double* rdg_shear, double* str) {
  CICE_TRY(ctx)
  c_->need_device();
  const double* g10[10] = {dxt, dyt, dxhy, dyhx, cxp, cyp, cxm, cym, tarear, tinyarea};
  double* sg[12] = {sp1, sp2, sp3, sp4, sm1, sm2, sm3, sm4, s121, s122, s123, s124};
  double* dg[5] = {shear, divu, prs_sig, rdg_conv, rdg_shear};
  CICE_REQUIRE(nx >= 3 && ny >= 3 && ndte >= 1, "bad dimensions");
  Evp::stress_host(c_->stream, dt, ndte, damping, nx, ny, ksub, icellt, ti, tj, uvel, vvel, g10,
                   strength, sg, dg, str);
  CICE_CATCH
}

int cice_evp_stepu(cice_ctx* ctx, int nx, int ny, int icellu, const int32_t* ui, const int32_t* uj,
                   const double* aiu, const double* str, const double* uocn, const double* vocn,
                   const double* waterx, const double* watery, const double* forcex,
                   const double* forcey, const double* umassdtei, const double* fm,
                   const double* uarear, double* strocnx, double* strocny, double* strintx,
                   double* strinty, double* uvel, double* vvel) {
  CICE_TRY(ctx)
  c_->need_device();
  const double* in10[10] = {aiu, uocn, vocn, waterx, watery, forcex, forcey, umassdtei, fm, uarear};
  double* io6[6] = {strocnx, strocny, strintx, strinty, uvel, vvel};
  CICE_REQUIRE(nx >= 3 && ny >= 3, "bad dimensions");
  Evp::stepu_host(c_->stream, nx, ny, icellu, ui, uj, in10, str, io6);
  CICE_CATCH
}

int cice_set_auscom(cice_ctx* ctx, double cosw, double sinw, double dragio, int use_ocnslope) {
  CICE_TRY(ctx)
#ifdef CICE4_AMD_AUSCOM
  const double want[4] = {cosw, sinw, dragio, use_ocnslope ? 1.0 : 0.0};
  if (c_->nml_set && !std::memcmp(want, c_->nml, sizeof(want))) return CICE_OK;   // called before every evp(dt)
  CICE_HIP(hipStreamSynchronize(c_->stream));   // nothing in flight reads the old values
  evp_set_namelist(cosw, sinw, dragio, use_ocnslope);
  std::memcpy(c_->nml, want, sizeof(want));
  c_->nml_set = true;
#else
  (void)cosw; (void)sinw; (void)dragio; (void)use_ocnslope;
  throw Error{CICE_EINVAL, "cice_set_auscom: this is the stand-alone build of the library (libcice4_amd.so); the coupled "
                           "one, with the access-om constants and the hemisphere-dependent turning angle, is "
                           "libcice4_amd_auscom.so"};
#endif
  CICE_CATCH
}

// host only (tests): what the retire of n pending one-launch loops does -- see evp_resident_plan
int cice_debug_resident_plan(int n, const uint32_t* word0, const int32_t* cur, const int32_t* flips, const int32_t* ident,
                             int cur_now, int flips_now, int ident_now, int32_t out[5]) {
  if (n < 0 || !out || (n > 0 && (!word0 || !cur || !flips || !ident))) return CICE_EINVAL;
  int o[5];
  evp_resident_plan(n, word0, cur, flips, ident, cur_now, flips_now, ident_now, o);
  for (int k = 0; k < 5; ++k) out[k] = o[k];
  return CICE_OK;
}

// test aid, no device needed: smallest shift of the sweep kernel's strip layout that is right for a block of ncol columns
// (K levels, S wavefronts per level), -1 if none; *strips = column strips of the block with it
int cice_debug_skew_layout(int K, int S, int ncol, int cyclic, int* strips) {
  if (K < 2 || K > 8 || (S != 1 && S != 3) || ncol < 1) return -2;
  for (int shift = 0; shift < 2 * K + 4; ++shift)
    if (evp_skew_layout_ok(K, S, ncol, shift, cyclic != 0)) {
      const int ownw = 62 * S + 2 - 2 * K, f = ownw - 1 - shift, npos = ncol + 1;
      if (strips) *strips = npos <= f ? 1 : 1 + (npos - f + ownw - 1) / ownw;
      return shift;
    }
  return -1;
}

// test aid, no device needed: the cell map of the image a one-task domain of several blocks is joined into for the sweeps
long long cice_debug_join_map(int nxg, int nyg, int bsx, int bsy, int ew, int ns, int32_t* map, long long cap) {
  try {
    return cice::join_map_debug(nxg, nyg, bsx, bsy, ew, ns, map, cap);
  } catch (...) {
    return -2;
  }
}

// ... the geometry that admits a tripole fold (option "skew_join_fold"); without a fold the same map
long long cice_debug_join_map_fold(int nxg, int nyg, int bsx, int bsy, int ew, int ns, int32_t* map, long long cap) {
  try {
    return cice::join_map_debug(nxg, nyg, bsx, bsy, ew, ns, map, cap, 1);
  } catch (...) {
    return -2;
  }
}

// test aid, no device needed: one strip's step of the measured balancing of the sweep's segments (cice::balance_strip)
int cice_debug_balance_strip(int rows, int n, const int32_t* ends, const double* durations, const double* weights,
                             const unsigned char* rows_with_ice, int32_t* new_ends, double* total) {
  if (rows < 1 || n < 1 || !ends || !durations || !weights || !new_ends) return -2;
  for (int i = 0; i < n; ++i)
    if (ends[i] < (i ? ends[i - 1] : 0) || ends[i] > rows) return -2;
  std::vector<double> cost((size_t)rows);
  std::vector<int> e(ends, ends + n), ne((size_t)n);
  const double t = cice::balance_strip(rows, n, e.data(), durations, weights, rows_with_ice, cost.data(), ne.data());
  if (total) *total = t;
  for (int i = 0; i < n; ++i) new_ends[i] = t > 0 ? ne[(size_t)i] : ends[i];
  return 0;
}

}  // extern "C"
