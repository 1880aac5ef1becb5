// The column batch: the state of every category of every local block, resident on the device, and the stages that run on
// it (the thermodynamic half-step, the thermodynamic changes of the thickness distribution).  Also what those stages share
// with the block-wise entries of the C-ABI: the names of a ThermoArgs' arrays, the status words, the decoding of a stop.
#pragma once
#include <cstring>
#include <vector>

#include "atmo.h"
#include "cleanup.h"
#include "coupling.h"
#include "dedd.h"
#include "common.h"
#include "domain.h"
#include "halo.h"
#include "handover.h"
#include "itd.h"
#include "pond.h"
#include "ridge.h"
#include "shortwave.h"
#include "therm.h"
#include "transport.h"

namespace cice {

// The device arrays of a ThermoArgs by name.  The values are the planes of cice_thermo_vertical's staging buffer (a field of
// several planes is named by its first); A_OUT + k: the 15 per-category outputs, fsurfn ... snoice in ThermoArgs' order.
enum { A_AICEN = 0, A_TRCRN = 1, A_VICEN = A_TRCRN + NTRCR, A_VSNON, A_EICEN, A_ESNON = A_EICEN + NILYR,
       A_FLW = A_ESNON + NSLYR, A_POTT, A_QA, A_RHOA, A_FSNOW, A_FBOT, A_TBOT, A_LH, A_SH, A_FSWSFC,
       A_FSWINT, A_FSWTHRU, A_SSW, A_ISW = A_SSW + NSLYR, A_OUT = A_ISW + NILYR, A_MLT = A_OUT + 15,
       A_FRZ, A_END };
// the (nx, ny[, nblocks]) fields of the thickness-distribution stage in the order they are staged
// device times of cice_therm2_cleanup_times: head, the eight passes, zap, bound_state, aggregate
enum { CLEAN_TIMES = 12 };
// device times of cice_ridge_times: rate kernel and shift kernel of each of the 20 possible iterations, the finish
enum { RIDGE_TIMES = 2 * RIDGE_NITERMAX + 1 };
enum { I2_AICE = 0, I2_AICE0, I2_FRAIN, I2_FRZMLT, I2_TF, I2_RSIDE, I2_FRESH, I2_FSALT, I2_FHOCN, I2_FRAZIL, I2_MELTL,
       I2_FRZ_ONSET };

// the status words (THERMO_STATUS_WORDS at `key`) before a launch: no error key, no column counted
inline void thermo_status_reset(unsigned long long* key, hipStream_t s) {
  CICE_HIP(hipMemsetAsync(key, 0xff, 8, s));
  CICE_HIP(hipMemsetAsync(key + 1, 0, (THERMO_STATUS_WORDS - 1) * 8, s));
}

// The arguments of a launch on (nx, ny, ncat, nblocks): plane_of(A_...) is the device array of that name.  What is left at
// zero is the caller's: the list (icells, indxi, indxj) or the dense mode's blk and niter.
template <class PlaneOf>
ThermoArgs thermo_args(const ThermoParams& tp, unsigned long long* key, int nx, int ny, int ncat, int nblocks, double dt,
                       double yday, PlaneOf plane_of) {
  ThermoArgs a{};
  a.p = tp; a.nx = nx; a.ny = ny; a.ncat = ncat; a.nblocks = nblocks; a.dt = dt; a.yday = yday;
  a.aicen = plane_of(A_AICEN); a.trcrn = plane_of(A_TRCRN); a.vicen = plane_of(A_VICEN); a.vsnon = plane_of(A_VSNON);
  a.eicen = plane_of(A_EICEN); a.esnon = plane_of(A_ESNON); a.flw = plane_of(A_FLW); a.potT = plane_of(A_POTT);
  a.Qa = plane_of(A_QA); a.rhoa = plane_of(A_RHOA); a.fsnow = plane_of(A_FSNOW); a.fbot = plane_of(A_FBOT);
  a.Tbot = plane_of(A_TBOT); a.lhcoef = plane_of(A_LH); a.shcoef = plane_of(A_SH); a.fswsfc = plane_of(A_FSWSFC);
  a.fswint = plane_of(A_FSWINT); a.fswthrun = plane_of(A_FSWTHRU); a.Sswabs = plane_of(A_SSW); a.Iswabs = plane_of(A_ISW);
  double** outs[15] = {&a.fsurfn, &a.fcondtopn, &a.fsensn, &a.flatn, &a.fswabsn, &a.flwoutn, &a.evapn,
                       &a.freshn, &a.fsaltn, &a.fhocnn, &a.meltt, &a.melts, &a.meltb, &a.congel,
                       &a.snoice};
  for (int k = 0; k < 15; ++k) *outs[k] = plane_of(A_OUT + k);
  a.mlt_onset = plane_of(A_MLT); a.frz_onset = plane_of(A_FRZ);
  a.errkey = key; a.nupdates = key + THERMO_COUNT_STRIDE;
  return a;
}

// number of columns updated: the sum of the kernel's counters (therm.h)
inline long long status_count(const unsigned long long* h) {
  long long n = 0;
  for (int k = 0; k < THERMO_COUNT_SLOTS; ++k) n += (long long)h[THERMO_COUNT_STRIDE * (1 + k)];
  return n;
}

// "no stop": what every entry with the reference's l_stop / istop / jstop reports first
inline void clear_stop(int32_t* l_stop, int32_t* istop, int32_t* jstop) { *l_stop = 0; *istop = 0; *jstop = 0; }

// The device times of a stage: N intervals between N + 1 events on one stream.  While it is off nothing is created and
// nothing recorded; the events are made at the first timed use and go with the clock.
template <int N>
struct StageClock {
  hipEvent_t ev[N + 1] = {};
  bool on = false;
  float ms[N] = {};
  StageClock() = default;
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void mark(int k, hipStream_t s) {    // event k on the stream, if on
    if (on && !ev[k]) CICE_HIP(hipEventCreate(&ev[k]));
    if (on) CICE_HIP(hipEventRecord(ev[k], s));
  }
  void read(int a, int b) {            // the intervals [a, b), once the stream has passed their events
    for (int k = a; k < b && on; ++k) CICE_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
  }
  void query(bool enable, float* out) {   // a *_times entry: the flag, and the times of the last timed call
    on = enable;
    for (int k = 0; k < N && out; ++k) out[k] = ms[k];
  }
};

// the error key of a thermo launch as the reference's stop: the cell (of the list, or of the dense plane), category, block
void decode_err(unsigned long long key, int nx, int ncat, const int32_t* indxi, const int32_t* indxj, int32_t* l_stop,
                int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop);
// the list key of the cell shift_ice names after a limited launch at boundary N (itd.h: STOPS)
unsigned long long itd_shift_key(const unsigned long long* r, int N);

class ColumnBatch {
 public:
  ColumnBatch() = default;
  ~ColumnBatch();
  // cice_thermo_batch_alloc.  dom: the context's domain or nullptr; its owned rows become the block table if its shape is
  // this one, and nothing of it is kept.  A call with the shape of the last one keeps every buffer (niter, perm included).
  void alloc(hipStream_t stream, CopyFan& fan, int nx, int ny, int nb, const Domain* dom);
  bool allocated() const { return nb_ > 0; }
  bool same_layout(const Domain& d) const { return nx_ == d.nx_block && ny_ == d.ny_block && nb_ == d.nblocks(); }
  const double* aicen() const { return aicen_.p; }
  const double* vicen() const { return vicen_.p; }
  const double* vsnon() const { return vsnon_.p; }
  // The entries of include/cice4_amd.h of the same names, behind their argument checks.  tp / ip: the parameters of
  // cice_thermo_init / cice_itd_init, nullptr before that call.
  void upload(const ThermoParams* tp, const cice_thermo_fields* h);
  void step(const ThermoParams* tp, double dt, double yday, long long* n_updates, int32_t* l_stop, int32_t* istop,
            int32_t* jstop, int32_t* nstop, int32_t* bstop, float* elapsed_ms);
  void download(const ThermoParams* tp, cice_thermo_fields* h);
  void merge(const cice_merge_fields* f);
  void step_therm1(const ThermoParams* tp, double chio, double dt, double yday, cice_thermo_fields* st,
                   const cice_frzmlt_fields* fz, const cice_merge_fields* mg, const cice_atmo_fields* atm,
                   long long* n_updates, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* nstop, int32_t* bstop);
  void step_therm2_itd(const ThermoParams* tp, const ItdParams* ip, double dt, double yday, const cice_therm2_fields* f,
                       int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage);
  // halo: the context's ghost-cell update (bound = 1) or nullptr
  void step_therm2_cleanup(const ItdParams* ip, double dt, const cice_therm2_cleanup_fields* f, Halo* halo, int32_t* l_stop,
                           int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage);
  // from: the transport whose device buffers hold the state (cice_ridge_chain), or nullptr: the state is uploaded
  void step_ridge(const ItdParams* ip, const RidgeParams* rp, double dt, const cice_ridge_fields* f, Transport* from,
                  Halo* halo, int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage);
  void ridge_times(bool enable, float ms[RIDGE_TIMES]);
  // step_radiation / prep_radiation for shortwave = 'default' (shortwave.h); sp: the parameters of cice_shortwave_init
  void step_radiation(const ThermoParams* tp, const ShortwaveParams* sp, const cice_radiation_fields* f);
  void prep_radiation(const ThermoParams* tp, const cice_prep_radiation_fields* f);
  // step_radiation for shortwave = 'dEdd' (dedd.h); dp: the parameters of cice_shortwave_dedd_init
  void step_radiation_dedd(const ThermoParams* tp, const DeddParams* dp, const cice_radiation_dedd_fields* f);
  void dedd_times(bool enable, float ms[1]) { dedd_clock_.query(enable, ms); }   // the last timed k_shortwave_dedd
  // coupling_prep (coupling.h); cp: the parameters of cice_coupling_init; halo: the context's ghost-cell update (bound = 1)
  // or nullptr
  void coupling_prep(const CouplingParams* cp, double dt, const cice_coupling_fields* f, Halo* halo);
  void coupling_times(bool enable, float ms[2]) { cpl_clock_.query(enable, ms); }   // k_ocean_mixed_layer, k_coupling_prep
  // compute_ponds and increment_age behind step_therm1 (pond.h); nt_volpn: the slot given to cice_pond_init, 0 none
  void step_ponds(const ThermoParams* tp, int nt_volpn, double dt, const cice_pond_fields* f);
  void pond_times(bool enable, float ms[1]) { pond_clock_.query(enable, ms); }      // the last timed k_pond_age
  void pond_chain(int mode);                        // cice_pond_chain
  void radiation_chain(int mode);                   // cice_radiation_chain
  void radiation_times(bool enable, float ms[2]) {  // the last timed k_shortwave_ccsm3, k_prep_radiation
    sw_clock_.query(enable, ms);
    prep_clock_.query(enable, ms ? ms + 1 : nullptr);
  }
  void handover_time(bool enable, float* ms);       // the last timed k_state_from_transport (0: none since enabled)
  void set_option(const char* key, int value);      // before or after alloc; kept across re-allocations
  void itd_times(bool enable, float ms[4]) { itd_clock_.query(enable, ms); }     // likewise
  void cleanup_times(bool enable, float ms[CLEAN_TIMES]);
  // "thermo_niter", one byte per (cell, category); "thermo_perm", the permutation of the last sorted step as int32 -- either
  // packed in 8-byte words.  Returns their number, -1 for another name.
  long long debug_read(const char* what, long long* out, long long cap) const;

 private:
  // One field of cice_thermo_fields: its name, where it lives on the device (plane `k` of `d` in units of the field's own
  // size), its host array, doubles per cell and block, and which way it travels.
  enum { F_UP = 1, F_DOWN = 2, F_IO = 3, F_FLUX_UP = 4 };
  struct Field { int name; DevBuf<double>* d; int k; const double* h; size_t per; int dir; };
  std::vector<Field> fields(const cice_thermo_fields* h);
  hipStream_t cs() { return fan_->forked ? fan_->next() : stream_; }   // the stream for the next host <-> device copy
  void tracer_copy(int it, const double* from, double* to, hipMemcpyKind kind);
  // The caller's state arrays, and their copies to (hipMemcpyHostToDevice) or from the batch in the order they travel: the
  // named members, then the tracer planes t0 .. t1 - 1.  A download writes through the pointers (the state of every entry
  // that downloads is its non-const members).
  enum { ST_AICEN = 1, ST_VICEN = 2, ST_VSNON = 4, ST_EICEN = 8, ST_ESNON = 16, ST_ALL = 31 };
  struct HostState { const double *aicen, *vicen, *vsnon, *eicen, *esnon, *trcrn; };
  void move_state(const HostState& h, int members, int t0, int t1, hipMemcpyKind kind);
  // the caller's fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn, and their copies to or from the five shortwave buffers
  struct SwArrays { double* h[5]; };
  void move_sw(const SwArrays& h, hipMemcpyKind kind);
  void zero_sw(hipStream_t s);
  // with_sw = false: the five shortwave arrays stay behind (cice_radiation_chain: the device copies are the host's)
  void upload_fields(const ThermoParams* tp, const cice_thermo_fields* h, bool with_fbot_tbot, bool with_coef,
                     bool with_sw = true);
  void download_fields(const ThermoParams* tp, cice_thermo_fields* h);
  void launch_step(const ThermoParams& tp, double dt, double yday, unsigned long long status[THERMO_STATUS_WORDS],
                   StageClock<1>& clock);
  enum { MRG_UP = 1, MRG_RUN = 2, MRG_DOWN = 4, MRG_ALL = 7 };
  void merge_phases(const cice_merge_fields* f, const double* aicen_init_dev, bool atmo_on_device, int phases);
  void read_rec(unsigned long long h[ITD_REC_WORDS]);
  // what cice_step_ridge has beyond the cleanup's fields
  struct RidgeStage {
    const RidgeParams* rp;
    const double *rdg_conv, *rdg_shear;
    double *dardg1dt, *dardg2dt, *dvirdgdt, *opening;
    Transport* from;
  };
  void column_stages(const ItdParams* ip, double dt, const cice_therm2_cleanup_fields* f, const RidgeStage* rs, Halo* halo,
                     int32_t* l_stop, int32_t* istop, int32_t* jstop, int32_t* bstop, int32_t* stage);

  hipStream_t stream_ = nullptr;
  CopyFan* fan_ = nullptr;
  int nx_ = 0, ny_ = 0, nb_ = 0;
  DevBuf<int32_t> blk_;
  std::vector<int32_t> hblk_;                // ilo, ihi, jlo, jhi per block (host copy of blk_)
  DevBuf<double> aicen_, trcrn_, vicen_, vsnon_, eicen_, esnon_, flw_, potT_, Qa_, rhoa_, fsnow_, fbot_, Tbot_, lhcoef_,
      shcoef_, fswsfc_, fswint_, fswthrun_, Sswabs_, Iswabs_, out15_, mlt_onset_, frz_onset_;
  DevBuf<double> mrg_in_, mrg_acc_, fz_in_;  // merge_fluxes inputs / accumulators, frzmlt inputs + rside
  DevBuf<double> atm_in_;                    // uatm, vatm, wind, zlvl, strax, stray (cice_step_therm1_abl)
  DevBuf<unsigned long long> key_;           // THERMO_STATUS_WORDS: [0] error key, then the update counters (therm.h)
  DevBuf<int32_t> perm_;                     // columns of every chunk sorted by expected work (k_thermo_sort)
  int sort_chunk_ = 0, sort_group_ = 8;      // chunk 0: no sorting (k_thermo_dense) -- the default: DESIGN.md 3.3
  DevBuf<unsigned char> niter_;              // solver iterations of every (cell, category) in the last step
  bool kept_aicen_init_ = false;             // mrg_in_ holds the concentrations step_therm1 found (step_therm2_itd)
  // thickness-distribution stage: its extra fields, record words, the clock of itd_times
  DevBuf<double> itd_b_;
  DevBuf<int32_t> itd_bi_;
  DevBuf<unsigned long long> rec_;
  StageClock<4> itd_clock_;
  // cleanup stage: the state is what step_therm2_itd left (all ntrcr tracer planes); its 2-d fields, tmask, block words
  bool therm2_state_ = false;
  DevBuf<double> clean_b_, clean_t_;
  DevBuf<int32_t> clean_bi_;
  DevBuf<unsigned long long> clean_w_;
  hipEvent_t clean_ev_[CLEAN_TIMES + 1] = {};
  bool clean_timed_ = false;
  float clean_ms_[CLEAN_TIMES] = {};
  // ridging stage: work planes, rdg_conv / rdg_shear and the four diagnostics; the list; block words (ridge.h)
  DevBuf<double> ridge_b_;
  DevBuf<int32_t> ridge_bi_;
  DevBuf<unsigned long long> ridge_w_;
  hipEvent_t ridge_ev_[2 * RIDGE_QUEUE + 1] = {};
  bool ridge_timed_ = false;
  float ridge_ms_[RIDGE_TIMES] = {};
  // radiation stage: its 2-d fields, the six albedo outputs, prep_radiation's copy of aicen.  sw_resident_: fswsfc_,
  // fswint_, fswthrun_, Sswabs_, Iswabs_ hold what the last step_radiation / prep_radiation left (and downloaded);
  // sw_armed_: ... to the host arrays sw_host_ (cice_radiation_chain mode 1).  Whatever else writes those five buffers
  // ends both (forget_sw).
  DevBuf<double> rad_b_;
  bool sw_resident_ = false, sw_armed_ = false;
  int rad_mode_ = 0;
  const double* sw_host_[5] = {};
  void forget_sw() { sw_resident_ = false; sw_armed_ = false; }
  void keep_sw(const SwArrays& h);
  // What the two schemes of step_radiation differ in.  buf: the scheme's buffer, planes2 (nx, ny, nb) planes -- the 2-d
  // inputs in2[k] in plane k -- then planesc (nx, ny, ncat, nb) planes: the nout per-category outputs, behind them apondn
  // and hpondn where `pond` says they are read.
  struct RadScheme {
    const char* entry;                       // the C entry, in front of every error text
    int state_resident;
    HostState state;
    DevBuf<double>* buf;
    int planes2, planesc;
    struct { const double* h; bool may_be_null; } in2[5];
    bool pond;
    const double* pondn[2];
    const double* pond_dev[2];               // cice_pond_chain: the device copies of pondn, or NULL: pondn is uploaded
    int nout;
    double* out[7];
    SwArrays sw;
    StageClock<1>* clock;
    bool forget_first;                       // the record of the shortwave buffers ends before the forcing is looked at
    double* coszen_out;                      // filled with 0.5 on the host afterwards, or nullptr
  };
  // launch(p2, pc): the scheme's kernel on the buffer's 2-d planes p2 and per-category planes pc
  template <class Launch> void radiation_stage(const ThermoParams& tp, const RadScheme& r, Launch launch);
  template <class Args> void radiation_args(Args& a, const ThermoParams& tp, double* p2, int sw, double* pc);
  StageClock<1> sw_clock_, prep_clock_;      // k_shortwave_ccsm3, k_prep_radiation: the two times of radiation_times
  // delta-Eddington: coszen and the four sw fields, the seven albedo outputs, apondn and hpondn
  DevBuf<double> dedd_b_;
  StageClock<1> dedd_clock_;
  // coupling stage.  alb_scheme_: whose buffer holds the per-category albedos of the last successful step_radiation --
  // ALB_CCSM3 rad_b_, ALB_DEDD dedd_b_, ALB_NONE neither: whatever rewrites or re-allocates those planes ends the record
  enum { ALB_NONE = 0, ALB_CCSM3, ALB_DEDD };
  int alb_scheme_ = ALB_NONE;
  DevBuf<double> cpl_b_;                     // the 2-d fields, albcnt, and the uploaded per-category arrays
  DevBuf<int32_t> cpl_bi_;                   // tmask
  StageClock<2> cpl_clock_;
  // pond stage.  therm1_state_: aicen_, vicen_, vsnon_, the surface temperature plane of trcrn_ and the meltt / melts
  // planes of out15_ hold what the last successful step_therm1 left -- whatever rewrites one of them ends the record.
  // pond_armed_: pond_b_ holds the apondn, hpondn the last step_ponds downloaded to the host arrays pond_host_
  // (cice_pond_chain mode 1).
  bool therm1_state_ = false;
  DevBuf<double> pond_b_;                    // volpn, iage, apondn, hpondn, six planes of uploaded state; frain
  StageClock<1> pond_clock_;
  int pond_mode_ = 0;
  bool pond_armed_ = false;
  const double* pond_host_[2] = {};
  hipEvent_t ho_ev_[2] = {};                 // around k_state_from_transport (handover_time)
  bool ho_timed_ = false, ho_pending_ = false;
  float ho_ms_ = 0.0f;
};

}  // namespace cice
