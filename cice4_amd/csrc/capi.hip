// C-ABI of libcice4_amd.so (include/cice4_amd.h).  Exceptions never cross the
// boundary: every entry returns a status code and records the message.
// Here: the context (life cycle, page locks, device memory), the domain, the communicator; the components: capi_*.hip.
#include "capi.h"

void cice_ctx::pin_range(const void* p, size_t bytes) {
  if (!p || !bytes) return;
  static const bool off = [] { const char* e = std::getenv("CICE4_AMD_PIN"); return e && e[0] == '0'; }();
  if (off) return;
  uintptr_t lo = (uintptr_t)p, hi = (uintptr_t)p + bytes;
  for (const auto& r : pin_ranges)
    if (lo >= r.first && hi <= r.second) return;            // already inside a registered range
  for (const auto& r : pin_refused)
    if (lo >= r.first && hi <= r.second) return;
  const uintptr_t lo0 = lo, hi0 = hi;
  std::vector<std::pair<uintptr_t, uintptr_t>> released;   // registered ranges the new one touches
  for (size_t k = 0; k < pin_ranges.size();) {
    if (pin_ranges[k].first <= hi0 && lo0 <= pin_ranges[k].second) {
      lo = std::min(lo, pin_ranges[k].first);
      hi = std::max(hi, pin_ranges[k].second);
      if (released.empty()) (void)hipDeviceSynchronize();    // no copy may be in flight on a range being released
      if (hipHostUnregister((void*)pin_ranges[k].first) != hipSuccess) (void)hipGetLastError();
      released.push_back(pin_ranges[k]);
      pin_ranges.erase(pin_ranges.begin() + k);
    } else {
      ++k;
    }
  }
  if (hipHostRegister((void*)lo, hi - lo, hipHostRegisterDefault) == hipSuccess) {
    pin_ranges.push_back({lo, hi});
    return;
  }
  // registered by somebody else, or not registrable: what was page-locked before stays page-locked (the union is
  // all or nothing for the runtime, not for us), only the request itself stays pageable and is not asked for again
  (void)hipGetLastError();
  for (const auto& r : released) {
    if (hipHostRegister((void*)r.first, r.second - r.first, hipHostRegisterDefault) == hipSuccess) pin_ranges.push_back(r);
    else (void)hipGetLastError();
  }
  pin_refused.push_back({lo0, hi0});
}

void cice_ctx::unpin_all() {
  for (const auto& r : pin_ranges)
    if (hipHostUnregister((void*)r.first) != hipSuccess) (void)hipGetLastError();
  pin_ranges.clear();
  pin_refused.clear();
}

void cice_ctx::need_device() {
  if (stream) {
    CICE_HIP(hipSetDevice(device));
    return;
  }
  int cnt = 0;
  CICE_HIP(hipGetDeviceCount(&cnt));
  if (cnt < 1) throw Error{CICE_EDEVICE, "no HIP device visible"};
  if (device >= 0) CICE_HIP(hipSetDevice(device));
  else CICE_HIP(hipGetDevice(&device));
  CICE_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  // one operation at once: the runtime binds a stream to a hardware queue when it first has work, and contexts that share a
  // device (ranks of a rehearsal on one GPU, whose one-launch loops wait for each other) need their MAIN streams on queues
  // of their own -- created, and bound, one after the other (tests/ranks_case.py)
  void* p = nullptr;
  CICE_HIP(hipMalloc(&p, 64));
  CICE_HIP(hipMemsetAsync(p, 0, 64, stream));
  CICE_HIP(hipStreamSynchronize(stream));
  CICE_HIP(hipFree(p));
}

void cice_ctx::need_halo() {
  need_device();
  if (!halo) {
    CICE_REQUIRE(have_domain, "cice_domain_create has not been called");
    halo.reset(new Halo());
    frame_halo.reset();
    halo->init(dom, stream);
    connect(*halo);
  }
}

void cice_ctx::connect(Halo& h) {
  if (comm) h.set_comm((ncclComm*)comm, comm_rank, comm_nranks);
  if (link) h.set_link(link, comm_rank, comm_nranks);
}

static std::string g_create_err;

// Calibration stream for the HBM counters: one 8-byte load and one 8-byte store per lane,
// the access width of the hot kernels (MI355X_MICROARCH.md: FETCH_SIZE is calibrated for
// 16-B lanes only, other widths must be calibrated on a known byte count).
__global__ __launch_bounds__(256) void k_diag_copy8(const double* __restrict__ src,
                                                    double* __restrict__ dst, size_t n) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = src[t] + 1.0;
}

__global__ __launch_bounds__(256) void k_diag_copy16(const double2* __restrict__ src,
                                                     double2* __restrict__ dst, size_t n2) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n2) {
    double2 v = src[t];
    v.x += 1.0;
    dst[t] = v;
  }
}

// what every cice_domain_create* does around its Domain::create*; a new decomposition: whatever was built on the one
// before goes
template <class Create>
static void domain_create(cice_ctx* c, const char* entry, int ew, int ns, Create create) {
  CICE_REQUIRE(ew >= 0 && ew <= 2 && ns >= 0 && ns <= 4,
               "boundary type must be 0 (open), 1 (cyclic), 2 (closed) or, north-south only, 3 (tripole) or 4 (tripoleT)");
  c->dom.self_comm = std::getenv("CICE4_AMD_SELF_COMM") != nullptr;  // test aid, see domain.h
  const char* msg = create();
  if (msg[0]) throw Error{CICE_EINVAL, std::string(entry) + ": " + msg};
  c->have_domain = true;
  c->evp.reset();
  c->transport.reset();
  c->chain_on = c->chain_ready = false;
  c->upwind.reset();
  c->halo.reset();
  c->frame_halo.reset();
}

extern "C" {

int cice_create(cice_ctx** ctx, int device) {
  if (!ctx) return CICE_EINVAL;
  try {
    *ctx = new cice_ctx();
    (*ctx)->device = device;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return CICE_EINVAL;
  }
  return CICE_OK;
}

int cice_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int cice_host_register(cice_ctx* ctx, void* host, size_t bytes) {
  CICE_TRY(ctx)
  CICE_REQUIRE(host && bytes, "NULL array");
  c_->need_device();
  c_->pin_range(host, bytes);
  CICE_CATCH
}

// Undo every cice_host_register / cice_evp_pin_fields of this context.  Page-locked host ranges MUST be
// released before the host frees that memory: the runtime keeps treating the range as DMA-able, and a later
// allocation that lands there is read through a stale mapping (GPU memory access fault).
int cice_host_unregister_all(cice_ctx* ctx) {
  CICE_TRY(ctx)
  if (c_->stream) CICE_HIP(hipStreamSynchronize(c_->stream));
  c_->unpin_all();
  CICE_CATCH
}

int cice_destroy(cice_ctx* ctx) {
  if (!ctx) return CICE_EINVAL;
  ctx->frame_host.release();
  ctx->tv_host.release();
  ctx->unpin_all();
  ctx->evp.reset();
  ctx->transport.reset();
  ctx->chain_on = ctx->chain_ready = false;
  ctx->upwind.reset();
  ctx->frame_halo.reset();
  ctx->halo.reset();
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  if (ctx->link && ctx->link_owned) link_close(ctx->link);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return CICE_OK;
}

// The library is compiled for one set of ice_domain_size parameters (CICE_NCAT, ...): every stride of the
// category / layer / tracer dimensions of the caller's module arrays is derived from them.  A host model built
// with other sizes must not get past its init calls.
int cice_check_sizes(cice_ctx* ctx, int ncat, int nilyr, int nslyr, int max_ntrcr) {
  CICE_TRY(ctx)
  if (ncat != NCAT || nilyr != NILYR || nslyr != NSLYR || max_ntrcr != NTRCR)
    throw Error{CICE_EINVAL, "libcice4_amd is built for ncat=" + std::to_string(NCAT) + " nilyr=" + std::to_string(NILYR) +
                                 " nslyr=" + std::to_string(NSLYR) + " max_ntrcr=" + std::to_string(NTRCR) +
                                 "; the host model has ncat=" + std::to_string(ncat) + " nilyr=" + std::to_string(nilyr) +
                                 " nslyr=" + std::to_string(nslyr) + " max_ntrcr=" + std::to_string(max_ntrcr) +
                                 " (rebuild the library with matching CICE_NCAT / CICE_NILYR / CICE_NSLYR / CICE_MAX_NTRCR)"};
  CICE_CATCH
}

const char* cice_last_error(const cice_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int cice_diag_stream_copy(cice_ctx* ctx, long long n_doubles, float* elapsed_ms) {
  CICE_TRY(ctx)
  CICE_REQUIRE(n_doubles > 0, "bad size");
  c_->need_device();
  DevBuf<double> a, b;
  a.alloc((size_t)n_doubles);
  b.alloc((size_t)n_doubles);
  a.zero(c_->stream);
  hipEvent_t e0, e1;
  CICE_HIP(hipEventCreate(&e0));
  CICE_HIP(hipEventCreate(&e1));
  const dim3 g((unsigned)(((size_t)n_doubles + 255) / 256));
  hipLaunchKernelGGL(k_diag_copy8, g, dim3(256), 0, c_->stream, (const double*)a.p, b.p, (size_t)n_doubles);
  CICE_HIP(hipEventRecord(e0, c_->stream));
  hipLaunchKernelGGL(k_diag_copy8, g, dim3(256), 0, c_->stream, (const double*)a.p, b.p, (size_t)n_doubles);
  CICE_HIP(hipEventRecord(e1, c_->stream));
  {  // same bytes with 16-byte lanes, for comparison in the kernel trace only
    const size_t n2 = (size_t)n_doubles / 2;
    const dim3 g2((unsigned)((n2 + 255) / 256));
    for (int r = 0; r < 2; ++r)
      hipLaunchKernelGGL(k_diag_copy16, g2, dim3(256), 0, c_->stream, (const double2*)a.p, (double2*)b.p, n2);
  }
  CICE_HIP(hipEventSynchronize(e1));
  if (elapsed_ms) CICE_HIP(hipEventElapsedTime(elapsed_ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  CICE_CATCH
}

int cice_device_sync(cice_ctx* ctx) {
  CICE_TRY(ctx)
  c_->need_device();
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

// device memory for callers that keep fields resident (cice_halo_update_dev_*): plain hipMalloc/hipFree on
// the context's device plus explicit copies ordered on the library's stream
int cice_device_alloc(cice_ctx* ctx, size_t bytes, void** dev) {
  CICE_TRY(ctx)
  CICE_REQUIRE(dev != nullptr, "NULL argument");
  c_->need_device();
  CICE_HIP(hipMalloc(dev, bytes));
  CICE_CATCH
}
int cice_device_free(cice_ctx* ctx, void* dev) {
  CICE_TRY(ctx)
  c_->need_device();
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_HIP(hipFree(dev));
  CICE_CATCH
}
int cice_device_copy(cice_ctx* ctx, void* dst, const void* src, size_t bytes, int to_device) {
  CICE_TRY(ctx)
  CICE_REQUIRE(dst && src, "NULL argument");
  c_->need_device();
  CICE_HIP(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c_->stream));
  CICE_HIP(hipStreamSynchronize(c_->stream));
  CICE_CATCH
}

const char* cice_build_flavour(void) {
#ifdef CICE4_AMD_AUSCOM
  return "auscom";
#else
  return "standalone";
#endif
}

// ---- domain ---------------------------------------------------------------------------------
int cice_domain_create(cice_ctx* ctx, int nxg, int nyg, int bsx, int bsy, int ew, int ns, int rank,
                       int npx, int npy) {
  CICE_TRY(ctx)
  domain_create(c_, "cice_domain_create", ew, ns, [&] { return c_->dom.create(nxg, nyg, bsx, bsy, ew, ns, rank, npx, npy); });
  CICE_CATCH
}

int cice_domain_create_map(cice_ctx* ctx, int nxg, int nyg, int bsx, int bsy, int ew, int ns, int rank,
                           int nranks, const int* owner, const int* local_id) {
  CICE_TRY(ctx)
  domain_create(c_, "cice_domain_create_map", ew, ns,
                [&] { return c_->dom.create_map(nxg, nyg, bsx, bsy, ew, ns, rank, nranks, owner, local_id); });
  CICE_CATCH
}

// host copies of the index lists of the current domain (tests, external tools): *n entries; out may be NULL
int cice_domain_list(const cice_ctx* ctx, const char* name, int loc, int* n, int32_t* out) {
  if (!ctx || !ctx->have_domain || !name || !n) return CICE_EINVAL;
  const Domain& d = ctx->dom;
  const std::vector<int32_t>* v = nullptr;
  const std::string k(name);
  const int l = loc - 1;
  const bool lok = l >= 0 && l < 4;
  if (k == "hfill") v = &d.hfill;
  else if (k == "fold_lsrc") v = &d.fold_lsrc;
  else if (k == "fold_bidx") v = &d.fold_bidx;
  else if (k == "fold_dst" && lok) v = &d.fold_out[l].dst;
  else if (k == "fold_src" && lok) v = &d.fold_out[l].src;
  else if (k == "fold_lo" && lok) v = &d.fold_lo[l];
  else if (k == "fold_hi" && lok) v = &d.fold_hi[l];
  if (!v) return CICE_EINVAL;
  *n = (int)v->size();
  if (out && !v->empty()) std::memcpy(out, v->data(), v->size() * 4);
  return CICE_OK;
}

int cice_domain_create_slabs(cice_ctx* ctx, int nxg, int nyg, int nblocks_y, int ew, int ns, int rank,
                             int nranks, int overlap) {
  CICE_TRY(ctx)
  domain_create(c_, "cice_domain_create_slabs", ew, ns,
                [&] { return c_->dom.create_slabs(nxg, nyg, nblocks_y, ew, ns, rank, nranks, overlap); });
  CICE_CATCH
}

int cice_domain_halo_refresh(const cice_ctx* ctx, int* n, int32_t* src, int32_t* dst) {
  if (!ctx || !ctx->have_domain || !n) return CICE_EINVAL;
  const Domain& d = ctx->dom;
  *n = (int)d.rsrc.size();
  if (src && dst && !d.rsrc.empty()) {
    std::memcpy(src, d.rsrc.data(), d.rsrc.size() * 4);
    std::memcpy(dst, d.rdst.data(), d.rdst.size() * 4);
  }
  return CICE_OK;
}

int cice_domain_info(const cice_ctx* ctx, int info[9]) {
  if (!ctx || !info || !ctx->have_domain) return CICE_EINVAL;
  const Domain& d = ctx->dom;
  int ns = 0, nr = 0;
  for (const HaloMsg& m : d.send) ns += (int)m.addr.size();
  for (const HaloMsg& m : d.recv) nr += (int)m.addr.size();
  const int v[9] = {d.nx_block, d.ny_block, d.nblocks(), (int)d.all.size(), (int)d.hsrc.size(),
                    (int)d.send.size(), (int)d.recv.size(), ns, nr};
  std::memcpy(info, v, sizeof(v));
  return CICE_OK;
}

int cice_domain_block(const cice_ctx* ctx, int lb, int info[10]) {
  if (!ctx || !info || !ctx->have_domain || lb < 0 || lb >= ctx->dom.nblocks()) return CICE_EINVAL;
  const Block& b = ctx->dom.all[ctx->dom.local[lb]];
  const int v[10] = {b.ilo, b.ihi, b.jlo, b.jhi, b.i0, b.j0, b.gid, b.owner, b.own_jlo, b.own_jhi};
  std::memcpy(info, v, sizeof(v));
  return CICE_OK;
}

int cice_domain_halo_local(const cice_ctx* ctx, int32_t* src, int32_t* dst) {
  if (!ctx || !ctx->have_domain || !src || !dst) return CICE_EINVAL;
  const Domain& d = ctx->dom;
  if (!d.hsrc.empty()) {
    std::memcpy(src, d.hsrc.data(), d.hsrc.size() * 4);
    std::memcpy(dst, d.hdst.data(), d.hdst.size() * 4);
  }
  return CICE_OK;
}

int cice_domain_halo_msg(const cice_ctx* ctx, int dir, int msg, int* peer, int* count, int32_t* addr) {
  if (!ctx || !ctx->have_domain) return CICE_EINVAL;
  // dir 0 / 1: ghost-cell messages (send / receive); 2 / 3: tripole top rows into the global buffer
  // (send: local addresses, receive: buffer indices)
  if (dir < 0 || dir > 3) return CICE_EINVAL;
  const std::vector<HaloMsg>& v = dir == 0 ? ctx->dom.send : dir == 1 ? ctx->dom.recv
                                  : dir == 2 ? ctx->dom.fold_send : ctx->dom.fold_recv;
  if (msg < 0 || msg >= (int)v.size()) return CICE_EINVAL;
  if (peer) *peer = v[msg].peer;
  if (count) *count = (int)v[msg].addr.size();
  if (addr) std::memcpy(addr, v[msg].addr.data(), v[msg].addr.size() * 4);
  return CICE_OK;
}

// ---- communication ---------------------------------------------------------------------------
// CICE4_AMD_SKIP_COMM (test aid): no RCCL communicator is created -- for checks of the block topology
// of a multi-rank run on hosts without one GPU per rank; any later exchange then fails loudly.
static bool skip_comm() { return std::getenv("CICE4_AMD_SKIP_COMM") != nullptr; }

int cice_comm_unique_id(char uid[128]) {
  if (!uid) return CICE_EINVAL;
  if (skip_comm()) {
    std::memset(uid, 0, 128);
    return CICE_OK;
  }
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return CICE_ECOMM;
  std::memcpy(uid, &id, 128);
  return CICE_OK;
}

int cice_comm_init(cice_ctx* ctx, const char uid[128], int rank, int nranks) {
  CICE_TRY(ctx)
  if (skip_comm()) return CICE_OK;
  CICE_REQUIRE(uid != nullptr && nranks >= 1 && rank >= 0 && rank < nranks, "cice_comm_init: bad arguments");
  c_->need_halo();
  if (!c_->comm) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    const ncclResult_t r = ncclCommInitRank(&c_->comm, nranks, id, rank);
    if (r != ncclSuccess) {
      c_->comm = nullptr;
      throw Error{CICE_ECOMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)};
    }
    c_->comm_rank = rank;
    c_->comm_nranks = nranks;
  } else {
    CICE_REQUIRE(rank == c_->comm_rank && nranks == c_->comm_nranks,
                 "cice_comm_init: this context already has a communicator with another rank / size");
  }
  c_->halo->set_comm((ncclComm*)c_->comm, c_->comm_rank, c_->comm_nranks);
  if (c_->frame_halo) c_->frame_halo->set_comm((ncclComm*)c_->comm, c_->comm_rank, c_->comm_nranks);
  CICE_CATCH
}

// a link in place of an RCCL communicator (halo.h), for the Halos this context has; owned: closed by cice_destroy
static void use_link(cice_ctx* c, LocalLink* l, bool owned, int rank, int nranks) {
  c->link = l;
  c->link_owned |= owned;
  c->comm_rank = rank;
  c->comm_nranks = nranks;
  c->halo->set_link(l, rank, nranks);
  if (c->frame_halo) c->frame_halo->set_link(l, rank, nranks);
}

// In-process link (halo.h): the ranks are contexts of this process, one host thread each.
int cice_comm_init_local(cice_ctx* ctx, int link_id, int rank, int nranks) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "cice_comm_init_local: bad arguments");
  CICE_REQUIRE(!c_->comm, "cice_comm_init_local: this context already has an RCCL communicator");
  c_->need_halo();
  use_link(c_, local_link_get(link_id, nranks), false, rank, nranks);
  CICE_CATCH
}

// The same between processes of one host (a file under /dev/shm; box_bytes = the largest message).
int cice_comm_init_shm(cice_ctx* ctx, const char* name, int rank, int nranks, long long box_bytes) {
  CICE_TRY(ctx)
  CICE_REQUIRE(name && name[0] == '/' && nranks >= 1 && rank >= 0 && rank < nranks && box_bytes > 0,
               "cice_comm_init_shm: bad arguments (the name must start with '/')");
  CICE_REQUIRE(!c_->comm && !c_->link, "cice_comm_init_shm: this context already has a communicator");
  c_->need_halo();
  use_link(c_, shm_link_open(name, rank, nranks, (size_t)box_bytes), true, rank, nranks);
  CICE_CATCH
}

// TIMING AID (halo.hip: MirrorLink): this context is rank `rank` of `nranks`, alone; its messages come back to it.
int cice_comm_init_mirror(cice_ctx* ctx, int rank, int nranks) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "cice_comm_init_mirror: bad arguments");
  CICE_REQUIRE(!c_->comm && !c_->link, "cice_comm_init_mirror: this context already has a communicator");
  c_->need_halo();
  use_link(c_, mirror_link_new(nranks), true, rank, nranks);
  CICE_CATCH
}

// Ranks of this context's communicator as RCCL itself counts them (ncclCommCount); 0 before cice_comm_init.
int cice_comm_count(cice_ctx* ctx, int* nranks) {
  CICE_TRY(ctx)
  CICE_REQUIRE(nranks != nullptr, "NULL argument");
  *nranks = 0;
  if (c_->link) *nranks = c_->comm_nranks;
  if (c_->comm) {
    const ncclResult_t r = ncclCommCount(c_->comm, nranks);
    if (r != ncclSuccess) throw Error{CICE_ECOMM, std::string("ncclCommCount: ") + ncclGetErrorString(r)};
  }
  CICE_CATCH
}

}  // extern "C"
