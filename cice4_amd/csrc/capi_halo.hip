// C-ABI of libcice4_amd.so: ice_HaloUpdate on host arrays and on device-resident fields.
#include "capi.h"

// one update of nlev levels of n elements on the device, by the element type
template <class T>
static void halo_apply_on(Halo& h, T* d, int nlev, size_t n, int loc, int kind, double fill) {
  if (std::is_same<T, double>::value) h.update_r8(reinterpret_cast<double*>(d), nlev, n, true, loc, kind, fill);
  else if (std::is_same<T, float>::value) h.update_r4(reinterpret_cast<float*>(d), nlev, n, loc, kind, (float)fill);
  else h.update_i4(reinterpret_cast<int32_t*>(d), nlev, n, loc, kind, (int32_t)fill);
}

// Host-pointer form of ice_HaloUpdate (what rccl/ice_boundary.F90 calls with a module array): the field is
// staged through a persistent device buffer (grown only when a larger field comes along) and ALL its levels
// travel in one update = one message per neighbour (bound_state's 65 levels included, ice_state.F90:162-217).
template <class T>
static void halo_host(cice_ctx* c, T* field, int nlev, int loc = LOC_CENTER, int kind = KIND_SCALAR, double fill = 0.0) {
  c->need_halo();
  CICE_REQUIRE(field && nlev >= 1, "bad argument");
  const size_t n = (size_t)c->dom.nblocks() * c->dom.nx_block * c->dom.ny_block;
  const size_t words = (n * nlev * sizeof(T) + 7) / 8;
  if (c->halo_stage.n < words) c->halo_stage.alloc(words);
  T* d = reinterpret_cast<T*>(c->halo_stage.p);
  CICE_HIP(hipMemcpyAsync(d, field, n * nlev * sizeof(T), hipMemcpyHostToDevice, c->stream));
  halo_apply_on<T>(*c->halo, d, nlev, n, loc, kind, fill);
  CICE_HIP(hipMemcpyAsync(field, d, n * nlev * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  CICE_HIP(hipStreamSynchronize(c->stream));
}

// The same for a field in the reference's own array layout (nx_block, ny_block, nz, nblocks) -- block outermost,
// what ice_HaloUpdate3D/4D receive: strided copies to and from the level-major device layout replace the
// repacking on the host.
//
// Only the cells a halo update can read or write travel: the FRAME of the rank's blocks (physical edge cells and ghost
// cells: every address that occurs in a copy, fill, message or fold list of the domain; ~4 (nx + ny) of the nx * ny
// cells of a block).  The host gathers the frame into a page-locked buffer (a few thousand elements per level), one
// copy takes it to the device, the update runs ON THE GATHERED BUFFER (a second Halo whose lists address positions
// in the frame instead of cells of the field), one copy brings it back and the host scatters it.  At gx1 a 2-D update moves 22 KB each way instead of 1 MB, a 25-level
// one 0.6 MB instead of 25 -- the reference's own timer of ice_HaloUpdate (timer_bound) in the whole model fell
// accordingly.
template <class D, class F>
static void each_halo_list(D& dm, F f) {   // every list of the domain that holds addresses of field cells
  f(dm.hsrc); f(dm.hdst); f(dm.hfill); f(dm.rsrc); f(dm.rdst); f(dm.fold_lsrc);
  for (auto& m : dm.send) f(m.addr);
  for (auto& m : dm.recv) f(m.addr);
  for (auto& m : dm.fold_send) f(m.addr);
  for (int l = 0; l < 4; ++l) f(dm.fold_out[l].dst);
}

static void frame_build(cice_ctx* c) {
  const Domain& dm = c->dom;
  const size_t n = (size_t)dm.nblocks() * dm.nx_block * dm.ny_block;
  std::vector<char> mark(n, 0);
  each_halo_list(dm, [&](const std::vector<int32_t>& v) {
    for (int32_t a : v)
      if (a >= 0 && (size_t)a < n) mark[a] = 1;
  });
  c->frame.clear();
  std::vector<int32_t> pos(n, -1);
  for (size_t a = 0; a < n; ++a)
    if (mark[a]) {
      pos[a] = (int32_t)c->frame.size();
      c->frame.push_back((int32_t)a);
    }
  // the same lists with every field address replaced by its position in the gathered frame: the update then runs on
  // the gathered buffer itself (level stride = frame size), copies, fills, messages and folds alike
  Domain fd = dm;
  each_halo_list(fd, [&](std::vector<int32_t>& v) {
    for (int32_t& a : v)
      if (a >= 0 && (size_t)a < n) a = pos[a];
  });
  c->frame_halo.reset(new Halo());
  c->frame_halo->init(fd, c->stream);
  c->connect(*c->frame_halo);
  CICE_HIP(hipStreamSynchronize(c->stream));
}

// A HOST array on a domain without messages (one rank: every ghost cell mirrors a cell of the same array, takes the
// fill value or comes out of the tripole fold): the update is a few thousand element copies inside the caller's own
// array, done right here on the host from the domain's lists -- what serial/ice_boundary.F90:591-873 does, in the
// order Halo::update works (copy list, fill list, refresh list, fold).  No device round trip: the whole model's Bound
// timer is back at the reference's.  Device-resident fields (cice_halo_update_dev_*) and
// domains with off-rank neighbours keep the device path.
template <class T>
static T fold_avg_host(T x1, T x2, int sgn) {
  if (std::is_same<T, int32_t>::value) return (T)std::round(0.5 * (double)(x1 + sgn * x2));   // nint()
  return (T)0.5 * (x1 + (T)sgn * x2);
}

// strides (in elements) of the caller's array: level (z1, z2) of block b starts at b * sb + z2 * s2 + z1 * s1; the
// contiguous (nx, ny, nz, nblocks) array is nz1 = nz, s1 = np, nz2 = 1, sb = nz * np
struct LevelStrides { int nz1, nz2; size_t s1, s2, sb; };

template <class T>
static void halo_host_lists(const Domain& dm, T* field, const LevelStrides& ls, int loc, int kind, T fill) {
  const size_t np = (size_t)dm.nx_block * dm.ny_block;
  // list address (level-major numbering: block * np + cell) -> element of level 0 in the caller's layout
  auto at = [&](int32_t a) { const size_t b = (size_t)a / np; return b * ls.sb + ((size_t)a - b * np); };
  const int nz = ls.nz1 * ls.nz2;
  const bool fold = dm.fold;
  if (fold) {
    CICE_REQUIRE(loc >= LOC_CENTER && loc <= LOC_EFACE, "halo: field location unknown on a tripole grid");
    CICE_REQUIRE(kind >= KIND_SCALAR && kind <= KIND_ANGLE, "halo: field kind unknown on a tripole grid");
  }
  const int sgn = kind == KIND_SCALAR ? 1 : -1;
  std::vector<T> buf(fold ? (size_t)dm.fold_rows() * dm.nxg : 0);
  for (int z = 0; z < nz; ++z) {
    T* f = field + (size_t)(z % ls.nz1) * ls.s1 + (size_t)(z / ls.nz1) * ls.s2;
    for (size_t e = 0; e < dm.hsrc.size(); ++e) f[at(dm.hdst[e])] = f[at(dm.hsrc[e])];
    for (int32_t a : dm.hfill) f[at(a)] = fill;
    for (size_t e = 0; e < dm.rsrc.size(); ++e) f[at(dm.rdst[e])] = f[at(dm.rsrc[e])];
    if (fold) {
      const int l = loc - 1;
      std::fill(buf.begin(), buf.end(), fill);
      for (size_t e = 0; e < dm.fold_lsrc.size(); ++e) buf[dm.fold_bidx[e]] = f[at(dm.fold_lsrc[e])];
      for (size_t e = 0; e < dm.fold_lo[l].size(); ++e) {
        const int32_t lo = dm.fold_lo[l][e], hi = dm.fold_hi[l][e];
        const T x = fold_avg_host<T>(buf[lo], buf[hi], sgn);
        buf[lo] = x;
        buf[hi] = (T)sgn * x;
      }
      const Domain::FoldOut& fo = dm.fold_out[l];
      for (size_t e = 0; e < fo.dst.size(); ++e) f[at(fo.dst[e])] = (T)sgn * buf[fo.src[e]];
    }
  }
}

static bool domain_has_messages(const Domain& dm) {
  return !dm.send.empty() || !dm.recv.empty() || !dm.fold_send.empty() || !dm.fold_recv.empty();
}

template <class T>
static void halo_host_blocked(cice_ctx* c, T* field, int nz, int loc, int kind, double fill) {
  CICE_REQUIRE(field && nz >= 1, "bad argument");
  CICE_REQUIRE(c->have_domain, "cice_domain_create has not been called");
  static const bool force_dev = std::getenv("CICE4_AMD_HALO_HOST_ON_DEVICE") != nullptr;   // test aid: the frame path
  if (!domain_has_messages(c->dom) && !force_dev) {
    const size_t np_ = (size_t)c->dom.nx_block * c->dom.ny_block;
    halo_host_lists<T>(c->dom, field, LevelStrides{nz, 1, np_, 0, (size_t)nz * np_}, loc, kind, (T)fill);
    return;
  }
  c->need_halo();
  const int nb = c->dom.nblocks();
  const size_t np = (size_t)c->dom.nx_block * c->dom.ny_block, n = np * nb;
  if (!c->frame_halo) frame_build(c);   // the frame belongs to the domain: dropped by cice_domain_create*
  const size_t nc = c->frame.size();
  if (nc > 0 && nc * 2 <= n) {   // the frame is the smaller part of the field: move only the frame
    const size_t cnt = nc * nz, bytes = cnt * sizeof(T);
    T* hp = static_cast<T*>(c->frame_host.need(bytes));
    if (c->frame_pack.n < (bytes + 7) / 8) c->frame_pack.alloc((bytes + 7) / 8);
    T* dp = reinterpret_cast<T*>(c->frame_pack.p);
    const int32_t* cell = c->frame.data();
    std::vector<size_t>& at = c->frame_at;     // element (level 0) of every frame cell in the caller's layout
    at.resize(nc);
    for (size_t k = 0; k < nc; ++k) {
      const size_t b = (size_t)cell[k] / np, q = (size_t)cell[k] - b * np;
      at[k] = b * nz * np + q;
    }
    for (int z = 0; z < nz; ++z) {
      T* out = hp + (size_t)z * nc;
      const T* src = field + (size_t)z * np;
      for (size_t k = 0; k < nc; ++k) out[k] = src[at[k]];
    }
    CICE_HIP(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, c->stream));
    halo_apply_on<T>(*c->frame_halo, dp, nz, nc, loc, kind, fill);
    CICE_HIP(hipGetLastError());
    CICE_HIP(hipMemcpyAsync(hp, dp, bytes, hipMemcpyDeviceToHost, c->stream));
    CICE_HIP(hipStreamSynchronize(c->stream));
    for (int z = 0; z < nz; ++z) {
      const T* in = hp + (size_t)z * nc;
      T* dst = field + (size_t)z * np;
      for (size_t k = 0; k < nc; ++k) dst[at[k]] = in[k];
    }
    return;
  }
  const size_t words = (n * nz * sizeof(T) + 7) / 8;
  if (c->halo_stage.n < words) c->halo_stage.alloc(words);
  T* d = reinterpret_cast<T*>(c->halo_stage.p);
  if (nz == 1 || nb == 1) {
    CICE_HIP(hipMemcpyAsync(d, field, n * nz * sizeof(T), hipMemcpyHostToDevice, c->stream));
  } else {
    for (int b = 0; b < nb; ++b)
      CICE_HIP(hipMemcpy2DAsync(d + (size_t)b * np, n * sizeof(T), field + (size_t)b * nz * np, np * sizeof(T),
                                np * sizeof(T), nz, hipMemcpyHostToDevice, c->stream));
  }
  halo_apply_on<T>(*c->halo, d, nz, n, loc, kind, fill);
  if (nz == 1 || nb == 1) {
    CICE_HIP(hipMemcpyAsync(field, d, n * nz * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  } else {
    for (int b = 0; b < nb; ++b)
      CICE_HIP(hipMemcpy2DAsync(field + (size_t)b * nz * np, np * sizeof(T), d + (size_t)b * np, n * sizeof(T),
                                np * sizeof(T), nz, hipMemcpyDeviceToHost, c->stream));
  }
  CICE_HIP(hipStreamSynchronize(c->stream));
}

// The same for a SECTION of a 4-d module array, e.g. trcrn(:,:,1:ntrcr,:,:) in bound_state (source/ice_state.F90:206): the
// horizontal planes are whole, the levels (z1, z2) and the blocks are strided.  On a one-rank domain the lists are
// applied in place (no copy of the section: that copy was most of the model's Bound timer); otherwise the section is
// gathered into a contiguous array, updated by the general path and scattered back.
template <class T>
static void halo_host_strided(cice_ctx* c, T* field, const LevelStrides& ls, int loc, int kind, double fill) {
  CICE_REQUIRE(field && ls.nz1 >= 1 && ls.nz2 >= 1, "bad argument");
  CICE_REQUIRE(c->have_domain, "cice_domain_create has not been called");
  const size_t np = (size_t)c->dom.nx_block * c->dom.ny_block;
  const int nb = c->dom.nblocks(), nz = ls.nz1 * ls.nz2;
  static const bool force_dev = std::getenv("CICE4_AMD_HALO_HOST_ON_DEVICE") != nullptr;
  if (!domain_has_messages(c->dom) && !force_dev) {
    halo_host_lists<T>(c->dom, field, ls, loc, kind, (T)fill);
    return;
  }
  std::vector<T> tmp((size_t)nb * nz * np);
  auto level = [&](int b, int z) {
    return field + (size_t)b * ls.sb + (size_t)(z / ls.nz1) * ls.s2 + (size_t)(z % ls.nz1) * ls.s1;
  };
  for (int b = 0; b < nb; ++b)
    for (int z = 0; z < nz; ++z) std::memcpy(tmp.data() + ((size_t)b * nz + z) * np, level(b, z), np * sizeof(T));
  halo_host_blocked<T>(c, tmp.data(), nz, loc, kind, fill);
  for (int b = 0; b < nb; ++b)
    for (int z = 0; z < nz; ++z) std::memcpy(level(b, z), tmp.data() + ((size_t)b * nz + z) * np, np * sizeof(T));
}

// Device-resident form: the field already lives in device memory (nlev levels of nblocks*ny_block*nx_block
// elements, level stride = one such plane set); nothing crosses PCIe, no allocation, asynchronous on the
// library's stream.
template <class T>
static void halo_dev(cice_ctx* c, T* dev_field, int nlev, int loc = LOC_CENTER, int kind = KIND_SCALAR, double fill = 0.0) {
  c->need_halo();
  CICE_REQUIRE(dev_field && nlev >= 1, "bad argument");
  hipPointerAttribute_t at{};
  CICE_REQUIRE(hipPointerGetAttributes(&at, dev_field) == hipSuccess && at.type == hipMemoryTypeDevice,
               "cice_halo_update_dev: not a device pointer");
  const size_t n = (size_t)c->dom.nblocks() * c->dom.nx_block * c->dom.ny_block;
  halo_apply_on<T>(*c->halo, dev_field, nlev, n, loc, kind, fill);
}

extern "C" {

int cice_halo_update_r8(cice_ctx* ctx, double* field, int nlev) {
  CICE_TRY(ctx) halo_host<double>(c_, field, nlev); CICE_CATCH
}
int cice_halo_update_i4(cice_ctx* ctx, int32_t* field, int nlev) {
  CICE_TRY(ctx) halo_host<int32_t>(c_, field, nlev); CICE_CATCH
}
// the same with the field location / kind (FieldLoc, FieldKind codes of ice_constants.F90:185-205: they decide
// offsets and sign at a tripole fold) and the fill value for ghost cells facing eliminated land blocks
int cice_halo_update_ex_r8(cice_ctx* ctx, double* field, int nlev, int loc, int kind, double fill) {
  CICE_TRY(ctx) halo_host<double>(c_, field, nlev, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_ex_r4(cice_ctx* ctx, float* field, int nlev, int loc, int kind, float fill) {
  CICE_TRY(ctx) halo_host<float>(c_, field, nlev, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_ex_i4(cice_ctx* ctx, int32_t* field, int nlev, int loc, int kind, int32_t fill) {
  CICE_TRY(ctx) halo_host<int32_t>(c_, field, nlev, loc, kind, fill); CICE_CATCH
}
// host field in the reference's (nx_block, ny_block, nz, nblocks) layout (nz = product of the level dimensions)
int cice_halo_update_blocked_r8(cice_ctx* ctx, double* field, int nz, int loc, int kind, double fill) {
  CICE_TRY(ctx) halo_host_blocked<double>(c_, field, nz, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_blocked_r4(cice_ctx* ctx, float* field, int nz, int loc, int kind, float fill) {
  CICE_TRY(ctx) halo_host_blocked<float>(c_, field, nz, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_blocked_i4(cice_ctx* ctx, int32_t* field, int nz, int loc, int kind, int32_t fill) {
  CICE_TRY(ctx) halo_host_blocked<int32_t>(c_, field, nz, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_strided_r8(cice_ctx* ctx, double* field, int nz1, long long stride1, int nz2, long long stride2,
                                long long stride_block, int loc, int kind, double fill) {
  CICE_TRY(ctx)
  CICE_REQUIRE(stride1 >= 0 && stride2 >= 0 && stride_block >= 0, "negative stride");
  halo_host_strided<double>(c_, field, LevelStrides{nz1, nz2, (size_t)stride1, (size_t)stride2, (size_t)stride_block}, loc,
                            kind, fill);
  CICE_CATCH
}
int cice_halo_update_dev_ex_r8(cice_ctx* ctx, double* dev_field, int nlev, int loc, int kind, double fill) {
  CICE_TRY(ctx) halo_dev<double>(c_, dev_field, nlev, loc, kind, fill); CICE_CATCH
}
int cice_halo_update_dev_r8(cice_ctx* ctx, double* dev_field, int nlev) {
  CICE_TRY(ctx) halo_dev<double>(c_, dev_field, nlev); CICE_CATCH
}
int cice_halo_update_dev_i4(cice_ctx* ctx, int32_t* dev_field, int nlev) {
  CICE_TRY(ctx) halo_dev<int32_t>(c_, dev_field, nlev); CICE_CATCH
}

}  // extern "C"
