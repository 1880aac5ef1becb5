// Private to the C-ABI glue (capi*.hip): the context behind the opaque cice_ctx of include/cice4_amd.h, the frame every
// entry is wrapped in, and the few helpers more than one of those units needs.
#pragma once
#include <rccl/rccl.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "domain.h"
#include "evp.h"
#include "halo.h"
#include "atmo.h"
#include "therm.h"
#include "itd.h"
#include "ridge.h"
#include "shortwave.h"
#include "dedd.h"
#include "coupling.h"
#include "pond.h"
#include "transport.h"
#include "batch.h"

using namespace cice;

// Page-locked host buffer of an entry that is called again and again with the same size: grown only when a larger
// request comes along, then by half as much again; freed by cice_destroy.
struct HostBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void* need(size_t want) {
    if (bytes < want) {
      release();
      CICE_HIP(hipHostMalloc(&p, want + want / 2, hipHostMallocDefault));
      bytes = want + want / 2;
    }
    return p;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct cice_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  std::string err;
  Domain dom;
  bool have_domain = false;
  std::unique_ptr<Halo> halo;
  std::unique_ptr<Evp> evp;
  std::unique_ptr<Transport> transport;
  std::unique_ptr<Upwind> upwind;
  // RCCL communicator of this rank (cice_comm_init): created once, handed to every Halo built afterwards --
  // the block decomposition may change (cice_domain_create*), the set of ranks does not
  ncclComm_t comm = nullptr;
  int comm_rank = -1, comm_nranks = 0;
  CopyFan fan;                 // side streams for the entries that move many separate host arrays: ONE set per context,
                               // shared by the dynamics, the thermodynamic half-step and the transport
  hipStream_t cs() { return fan.forked ? fan.next() : stream; }   // the stream for the next host <-> device copy
  // evp -> transport chain (cice_transport_chain): the host arrays the transport calls will be given; chain_ready: a
  // cice_evp call has prefetched them and no transport call has consumed that yet
  cice_transport_fields chain{};
  bool chain_on = false, chain_ready = false;
  const double *chain_aicen = nullptr, *chain_vicen = nullptr, *chain_u = nullptr, *chain_v = nullptr;   // what cice_evp was given
  // transport -> ridging hand-over (cice_ridge_chain).  ridge_armed: the last entry was a cice_transport_remap that ended
  // without a stop, its result is in the transport's device buffers and ridge_f names the host arrays it was given;
  // Transport::download_deferred(): ... and those arrays have not received it (mode 2).  Every entry but the consuming
  // cice_step_ridge ends this in its frame (end_handover): a deferred download is made good first.
  int ridge_mode = 0;
  bool ridge_armed = false;
  cice_transport_fields ridge_f{};
  void end_handover() {
    if (!ridge_armed) return;
    ridge_armed = false;       // (first: a flush that throws must not be tried again with arrays that may be gone)
    if (transport && transport->download_deferred()) transport->download_state(ridge_f);
  }
  double chio = 0.006;         // coupled flavour: the namelist's chio (cice_thermo_set_chio)
  double nml[4] = {1.0, 0.0, 0.00536, 0.0};   // coupled flavour: cosw, sinw, dragio, use_ocnslope last sent to the device
  bool nml_set = false;
  LocalLink* link = nullptr;   // stand-in for the communicator without RCCL (cice_comm_init_local / _shm; tests)
  bool link_owned = false;     // the shared-memory form belongs to this context
  // Page-locked host ranges of this context: [start, end) in bytes, disjoint.  One manager for the explicit
  // registrations (cice_host_register, cice_evp_pin_fields): a new range that touches registered ones is registered
  // as their union (a whole array after some of its slices), because a copy whose host range is partly registered
  // is refused by the runtime.  CICE4_AMD_PIN=0 in the environment leaves everything pageable (diagnostic).
  // Exact byte ranges, not page-rounded, for the same reason (a neighbouring variable sharing the last page).
  std::vector<std::pair<uintptr_t, uintptr_t>> pin_ranges;
  std::vector<std::pair<uintptr_t, uintptr_t>> pin_refused;  // ranges hipHostRegister turned down (not retried)
  void pin_range(const void* p, size_t bytes);
  void unpin_all();
  // staging of the host-pointer entries (thermo_vertical is called ncat x nblocks times per step with
  // the same block size: allocated once, grown only when a larger block comes along)
  DevBuf<double> tv_stage, fz_stage, halo_stage;
  // page-locked gather buffer and cell offsets of the compact thermo_vertical path
  HostBuf tv_host;
  std::vector<size_t> tv_cells;
  // frame of the rank's blocks (cells a halo update can read or write), for host-array halo updates
  std::vector<int32_t> frame;
  std::vector<size_t> frame_at;
  std::unique_ptr<Halo> frame_halo;   // the domain's lists re-addressed to positions in the gathered frame
  DevBuf<double> frame_pack;
  HostBuf frame_host;
  DevBuf<int32_t> tv_list;
  // thermo
  ThermoParams tp{};
  bool have_thermo = false;
  DevBuf<unsigned long long> tkey;  // THERMO_STATUS_WORDS of the block-wise entries: [0] error key, then the update counters
  ColumnBatch batch;           // the device-resident state of all local blocks and its stages (batch.h)
  const ThermoParams* thermo() const { return have_thermo ? &tp : nullptr; }   // what the batch's methods are handed:
  const ItdParams* itd() const { return have_itd ? &ip : nullptr; }            // nullptr before the init call
  // thickness-distribution stage (itd.h): module variables given to cice_itd_init, staging and record words of the
  // block-wise entries (grown on demand)
  ItdParams ip{};
  bool have_itd = false;
  DevBuf<double> itd_d;
  DevBuf<int32_t> itd_i;
  DevBuf<unsigned long long> itd_rec;
  // ridging (ridge.h): the namelist values given to cice_ridge_init, the block words of the block-wise entry
  RidgeParams rp{};
  bool have_ridge = false;
  DevBuf<unsigned long long> ridge_w;
  // shortwave (shortwave.h): the namelist values given to cice_shortwave_init; staging and list of the block-wise entry
  ShortwaveParams sp{};
  bool have_sw = false;
  DevBuf<double> sw_d;
  DevBuf<int32_t> sw_i;
  // delta-Eddington shortwave (dedd.h): what cice_shortwave_dedd_init was given and derived; staging and list of the
  // block-wise entry.  Independent of sp / have_sw: a context may hold both schemes
  DeddParams dp{};
  bool have_dedd = false;
  DevBuf<double> dedd_d;
  DevBuf<int32_t> dedd_i;
  // coupling_prep (coupling.h): what cice_coupling_init was given
  CouplingParams cp{};
  bool have_cpl = false;
  // melt ponds and ice age (pond.h): the slot given to cice_pond_init (0: no pond tracer); staging of the block-wise entries
  int nt_volpn = 0;
  bool have_pond = false;
  DevBuf<double> pond_d;
  DevBuf<int32_t> pond_i;
  // device is required lazily: domain queries work on a CPU-only host
  // Every C-ABI entry binds the calling thread to this context's device first (CICE_TRY): the host
  // process may have changed the current device since the last call (another context on another GPU,
  // torch.cuda.set_device, another thread).
  void bind_device() {
    if (stream) CICE_HIP(hipSetDevice(device));
  }
  void need_device();
  void need_halo();
  void connect(Halo& h);       // hands this rank's communicator or link, if any, to a Halo built on the domain
};

#define CICE_TRY_BARE(ctx_) \
  cice_ctx* c_ = (ctx_); \
  if (!c_) return CICE_EINVAL; \
  try {                        \
    c_->bind_device();         \
    c_->fan.forked = false;   /* an entry that failed between fork and join leaves nothing behind for the next */
// Every entry but the consumer of the transport -> ridging hand-over (cice_step_ridge, which reads ridge_armed first and ends
// the hand-over itself) ends it here: a state whose download was deferred reaches the host arrays before the entry runs.
#define CICE_TRY_QUEUED(ctx_) \
  CICE_TRY_BARE(ctx_)         \
    c_->end_handover();
// Every entry but the two that may leave one-launch EVP loops pending (cice_evp_subcycles, and cice_evp_get_info asked for
// "resident_pending") first looks at the records of the pending ones (Evp::retire_resident): whatever it reads, launches or
// changes then finds the state a wait behind every loop would have left.
#define CICE_TRY_HANDOVER(ctx_) \
  CICE_TRY_BARE(ctx_)           \
    if (c_->evp) c_->evp->retire_resident();
#define CICE_TRY(ctx_)      \
  CICE_TRY_HANDOVER(ctx_)   \
    c_->end_handover();
#define CICE_CATCH                                            \
  }                                                           \
  catch (const Error& e) {                                    \
    c_->err = e.msg;                                          \
    return e.code;                                            \
  }                                                           \
  catch (const std::exception& e) {                           \
    c_->err = e.what();                                       \
    return CICE_EINVAL;                                       \
  }                                                           \
  return CICE_OK;

// The list (icells, indxi, indxj) of a block-wise entry on its (nx, ny) block as one int32 per cell: 1 on the listed cells,
// 0 elsewhere -- or, with `positions`, the cell's place in the list counted from 1, where no cell may be named twice.
inline std::vector<int32_t> list_mask(int nx, int ny, int icells, const int32_t* indxi, const int32_t* indxj,
                                      bool positions = false) {
  CICE_REQUIRE(nx >= 1 && ny >= 1 && icells >= 0 && (size_t)icells <= (size_t)nx * ny && (icells == 0 || (indxi && indxj)),
               "bad dimensions or NULL index list");
  std::vector<int32_t> m((size_t)nx * ny, 0);
  for (int ij = 0; ij < icells; ++ij) {
    CICE_REQUIRE(indxi[ij] >= 1 && indxi[ij] <= nx && indxj[ij] >= 1 && indxj[ij] <= ny, "index list outside the block");
    int32_t& w = m[(size_t)(indxj[ij] - 1) * nx + indxi[ij] - 1];
    CICE_REQUIRE(!positions || w == 0, "index list names a cell twice");
    w = positions ? ij + 1 : 1;
  }
  return m;
}

#define NEED_EVP CICE_REQUIRE(c_->evp != nullptr, "cice_evp_init has not been called")
// (`also`: a pointer the entry has always checked in the same breath)
#define NEED_BATCH(also) CICE_REQUIRE(c_->batch.allocated() && (also), "cice_thermo_batch_alloc has not been called")
