// uwspr_internal.h -- shared declarations of the HIP implementation
// (context, device-side records, kernel launchers).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <vector>

#include "../../include/uwspr_hip.h"
#include "stream_ring.h"

// Options of a context, by index (names and defaults: uwspr_api.hip: kOptions; ABI: uwspr_set_option).
enum {
  UWSPR_OPT_SCHED = 0,          // 1 fused kernel (default), 0 staged launches
  UWSPR_OPT_STAGE_KERNELS,      // staged form: 1 packed / ring kernels (default), 0 flat kernel everywhere
  UWSPR_OPT_REUSE,              // 1 (default): the hypothesis that repeats the previous stage's winner is not correlated again
  UWSPR_OPT_PHASOR_TABLES,      // 1 (default)
  UWSPR_OPT_FAST_SEARCH,        // 0 (default)
  UWSPR_OPT_K4_T,               // flat kernel: tones per lane (0 = by size)
  UWSPR_OPT_K5_LANES,           // fold form: -1 by size (default), 0 wave form, 1 lanes form
  UWSPR_OPT_K1_ROWS,            // spectrogram rows per wavefront walk (0 = default)
  UWSPR_OPT_K3_TILE,            // coarse-search tile form (-1 = by size)
  UWSPR_OPT_SCHED_STAMPS,       // diagnostics: phase times of the fused kernel
  UWSPR_OPT_DIST_FORCE_COMM,    // tests: a one-rank communicator is really created
  UWSPR_OPT_FRONTEND,           // K0 taps: 0 the flowgraph's three-stage GNU Radio chain (default), 1 the compact single stage
  UWSPR_OPT_K4_FORMS,           // staged form: 1 (default) S5 through the register-ring kernel k4_jig, 0 through k4_ring<6,8>
  UWSPR_OPT_AUDIO_RATE,         // rate of the audio uwspr_stream_push_audio takes (default 12000: no resampler; else K11 ahead of K0)
  UWSPR_OPT_BLANK,              // uwspr_stream_push_audio: K12's threshold in quarters of the block median (default 0: no blanker)
  UWSPR_OPT_BLANK_GUARD,        // K12's guard G: samples zeroed either side of a flagged one (default 2)
  UWSPR_OPT_CARRIER,            // K0's centre in Hz (default 1500), the flowgraph's Center_Frequency
  UWSPR_OPT_FRONTEND_HBW,       // K0's half-bandwidth in Hz (default 10; grc mode), the flowgraph's Half_Bandwidth
  UWSPR_OPT_TX_CUTOFF,          // K7: cut-off of the transmit chain's second low-pass in Hz (default 2500)
  UWSPR_OPT_TX_FORM,            // K7: 0 (default) the carrier form only where a carrier or the cut-off asks for it, 1 always
  UWSPR_NOPT
};

// Launch forms of the sweep kernels, counted on the host where the launchers choose (uwspr_ctx::launch_forms, read by
// uwspr_debug_launch_forms: the slot layout of its `out`).  A test that forces a form reads here that it really ran.
enum {
  UWSPR_FORM_FLAT_T1 = 0,       // k4_tonecorr<1>
  UWSPR_FORM_FLAT_T2,           // k4_tonecorr<2>
  UWSPR_FORM_FLAT_T4,           // k4_tonecorr<4>
  UWSPR_FORM_FLAT_FAST,         // k4_tonecorr<1, true> (fast_search)
  UWSPR_FORM_FOLD_WAVE,         // k5_fold_wave, with or without soft symbols
  UWSPR_FORM_FOLD_LANES,        // k5_fold
  UWSPR_FORM_GRID_NL1,          // k4_grid<NL>: NL = 1, 2, 4, 5, 6, 8 in the next six slots
  UWSPR_FORM_GRID_NL2,
  UWSPR_FORM_GRID_NL4,
  UWSPR_FORM_GRID_NL5,
  UWSPR_FORM_GRID_NL6,
  UWSPR_FORM_GRID_NL8,
  UWSPR_FORM_GRID_WPW1,         // k4_grid with 1, 2, 4 wavefronts per workgroup
  UWSPR_FORM_GRID_WPW2,
  UWSPR_FORM_GRID_WPW4,
  UWSPR_FORM_GRID_FALLBACK,     // uwspr_sync_grid: a lag block did not fit LDS, the whole call went through the flat kernel
  UWSPR_FORM_FOLD_WAVE_SOFT,    // of the fold launches above: those that wrote soft symbols ...
  UWSPR_FORM_FOLD_LANES_SOFT,
  UWSPR_FORM_FOLD_WAVE_PWIN,    // ... and those that were given the stage winner's magnitudes (stage 5 of the schedule)
  UWSPR_FORM_FOLD_LANES_PWIN,
  UWSPR_NFORMS
};

namespace uwspr {

// 162 WSPR sync bits (lib/pr3.h:5-13), LSB-first packed; a protocol constant.
#define UWSPR_PR3_WORDS                                                        \
  { 0x07a47103u, 0x58b340a4u, 0x56349558u, 0xe2cdc904u, 0x63580ca0u, 0x00000000u }
__host__ __device__ constexpr uint32_t pr3_word(int w) {
  constexpr uint32_t t[6] = UWSPR_PR3_WORDS;
  return t[w];
}
__host__ __device__ constexpr int pr3_bit(int k) { return (pr3_word(k >> 5) >> (k & 31)) & 1; }

// IEEE-754 correctly rounded binary32 sqrt and divide.  NOTE: HIP's __fsqrt_rn /
// __fdiv_rn are NOT that (they lower to the 1-ulp native forms unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined); plain sqrtf() and `/` are, under
// -fhip-fp32-correctly-rounded-divide-sqrt (set explicitly in the build flags).
__device__ __forceinline__ float ieee_sqrtf(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float ieee_divf(float x, float y) { return x / y; }

// Workgroups are dealt to the 8 XCDs round-robin by blockIdx, each XCD with a private
// 4 MB L2.  This bijective remap hands every XCD a CONTIGUOUS range of logical blocks,
// so the blocks that re-read the same symbol windows (the hypotheses of one candidate)
// share one L2 instead of each missing in its own.  Pure placement: results unchanged.
__device__ __forceinline__ unsigned xcd_swizzle(unsigned bid, unsigned nwg) {
  const unsigned q = nwg >> 3, r = nwg & 7u, x = bid & 7u;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// Instruction-issue priority of the short kernels' wavefronts (s_setprio, 0..3).  Under several streams the kernels
// of different lanes share the SIMDs and the arbiter serves higher priority first, then age: a fold or a schedule
// transition that takes 6 us alone took 40-65 us beside the other lanes' correlation launches, and every lane's chain
// waits on five of them per step.  With priority 3 in the K5 family (folds, schedule init / transitions / finish,
// slab packing) `value` rises 2 % (profiles/r03_ab_experiments.txt); raising K1..K3 or the S0..S4 correlation
// launches above the jiggered-shift ring as well adds nothing.
constexpr int kSmallPrio = 3;
#define UWSPR_SET_PRIO(level) do { if ((level) > 0) __builtin_amdgcn_s_setprio(level); } while (0)

// fine-grid hypothesis as the kernels consume it (24 B)
struct dev_hyp {
  int32_t frame;   // <0: skip
  int32_t lag;
  float f0;
  float drift;     // linear: *drift1
  float slmc;      // nonlinear: slmFrequencyDrift(m_nl, cf, t=0)
  int32_t m_type;
};

// A lag group: up to 8 hypotheses that differ only in their time lag (same
// frame, frequency, drift model).  They share the per-symbol tone phasors, so
// K4 advances the phasor recurrence once and correlates all lags against it.
struct dev_grp {
  int32_t frame;     // <0: skip
  int32_t m_type;
  float f0, drift, slmc;
  int32_t nvalid;    // lags in use (the kernel is instantiated for NL >= nvalid)
  int32_t hyp_base;  // lag slot l is hypothesis hyp_base + ((hmap >> 4l) & 15)
  int32_t lag[8];
  uint32_t hmap;     // 0x76543210 when the slots are in hypothesis order
};
static_assert(sizeof(dev_grp) == 64, "dev_grp is one 64-byte record");

// per-candidate refinement state kept in HBM between schedule stages
struct cand_state {
  int32_t frame;       // <0: empty slot
  int32_t m_type;
  float slmc;
  float f1, drift1, sync1;
  int32_t shift1;
  int32_t worth;
  float driftp, driftm;
  // The middle hypothesis of S1, S3 and S4 is the hypothesis that won the stage before it
  // (same f0, lag, drift): its metric is already known and K4 / the fold skip it.
  float csync;         // metric of (f1, shift1, drift1) when cknown
  int32_t cknown;
  // staged form: phasor tables of the lag stages (k5: ptab_build): the centre frequency each set was built
  // around and whether it was built (the frequency did not depend on the symbol at that point)
  float tabA_f, tabB_f;
  int32_t tabA_ok, tabB_ok;
};
// phasor tables of the staged schedule, per slot: tables 0..4 = set A (candidate frequency + {-2..2} 0.25 Hz: S0 uses
// the middle one, S1 all five), tables 5..9 = set B (f1 + {-2..2} 0.05 Hz after S2: S3 the middle one, S4 all five,
// S5 the stage-4 winner's); each [4 tones][256 steps] (c, s) -- the sequence of cc:186-199
constexpr int kPtabPerSlot = 10;
constexpr int kPtabSetB = 5;           // first table of set B
constexpr int kPtabFloat2 = 4 * 256;   // float2 per table

struct fdr_consts {
  int fl, n, size, m, hpbm, finpb, noiseidx, maxfreqs, maxdrift;
  int band_lo, band_w;
  int cell_hyps, nlin, ntot;      // hyps per (ifr,k0) cell; linear ones; 130*cell_hyps
  int off_min, off_max, nc;       // ifd-ifr range; tile centres per row = 5 + off_max-off_min
  int tp;                         // K3 tile row pitch, in float4 (tile form 0) or floats (forms 1, 2)
  int k3_mode;                    // K3 tile form (k3_coarse.hip: K3_TILE_*)
  int ifr_lo, n_ifr;              // rows of the offset table
  int umax;                       // distinct offset sequences per cell (max over rows)
  int cand_slots;                 // max candidates a frame can yield
  float df, min_snr, min_snr_floor, threshold;
};

struct ev_pair { hipEvent_t a, b; int kind; int64_t units; };
struct tx_state;
void tx_release(uwspr_ctx *c);   // k7_transmit.hip: frees what the uwspr_tx_* calls made
struct sub_state;
void sub_release(uwspr_ctx *c);  // k8_subtract.hip: frees what uwspr_subtract_batch / the pipe's second pass made
struct osd_state;
void osd_release(uwspr_ctx *c);  // k9_osd.hip: frees what uwspr_osd_batch / the pipe's option "osd" made
struct blk_state;
void blk_release(uwspr_ctx *c);  // k10_blockdemod.hip: frees what uwspr_blockdemod_batch / the pipe's option "block" made
struct rs_state;
void rs_release(uwspr_ctx *c);   // k11_resample.hip: frees what uwspr_resample_batch made
struct bk_state;
void bk_release(uwspr_ctx *c);   // k12_blank.hip: frees what uwspr_blank_batch made
struct deep_state;
void deep_release(uwspr_ctx *c); // k13_deep.hip: frees what uwspr_deep_set_list / uwspr_deep_batch made
struct calls_state;
struct calls_set;
void calls_release(uwspr_ctx *c); // k14_calls.hip: frees what uwspr_calls_set / uwspr_calls_batch made
struct trk_state;
struct trk_set;
void trk_release(uwspr_ctx *c);  // k15_track.hip: frees what uwspr_track_set / uwspr_track_batch made
struct fol_state;
struct fol_set;
void fol_release(uwspr_ctx *c);  // k16_follow.hip: frees what uwspr_follow_set / uwspr_follow_batch made

}  // namespace uwspr

struct uwspr_ctx {
  uwspr_params p;
  uwspr::fdr_consts fc;
  int device;
  int num_cus;
  char device_name[64];
  hipStream_t own_stream, stream;
  char err[512];

  // constant tables in HBM
  float *d_window;     // [512]
  float *d_twiddle;    // [256][2]
  float *d_k3_tile;    // [num_cus][n][tp] sqrt rows when the coarse tile does not fit LDS (K3_TILE_F1_HBM), else null
  uint32_t *d_off;     // [n_ifr][umax][84]: distinct offset sequences, 2 x u16 tile byte offsets per word (k3_coarse.hip)
  uint16_t *d_umap;    // [n_ifr][cell_hyps]: hypothesis -> distinct sequence
  float *d_fe_taps;    // [32][fe_J][2] complex front-end taps by phase (K0), built on first use for mode fe_mode
  int fe_mode, fe_J, fe_dcols;
  int fe_fc, fe_hb;    // the centre and half-bandwidth d_fe_taps was designed for
                       // (away from 1500 Hz, 10 Hz: frontend_carrier_tables' block, the rotator table behind the taps)
  // uwspr_debug_frontend_carrier_launch's tables, kept between calls with the same carriers: [NC][32][J] taps, rotator, fc mod 375
  std::vector<int> dbg_car;
  int dbg_mode = -1, dbg_hb = 0, dbg_J = 0, dbg_dcols = 0;
  float *d_dbg_taps = nullptr;
  size_t cap_audio; float *d_audio;   // staging when the audio is host memory

  // batch scratch (grown on demand, never shrunk)
  size_t cap_frames_bytes; float *d_frames;       // staging when frames are host memory
  int cap_B;
  float *d_ps;          // [B][n][band_w]
  float *d_psavg;       // [B][band_w]
  float *d_smraw;       // [B][finpb]
  float *d_smspec;      // [B][finpb]
  float *d_noise;       // [B]
  uwspr_candidate *d_cands;  // [B][maxfreqs]
  int32_t *d_npk;       // [B]
  int32_t *d_work;      // [1 + B*cand_slots]: count, then frame*cand_slots + j items
  int last_B;
  int grid_cap; size_t cap_grid_bytes; float *d_syncgrid;  // [B][grid_cap][ntot]

  size_t cap_hyps; uwspr::dev_hyp *d_hyps;
  size_t cap_grps; uwspr::dev_grp *d_grps;
  size_t cap_cent; uwspr_candidate *d_cent; int32_t *d_cent_frame;   // per-slot grid centres (S1/S2/S4)
  size_t cap_abi_hyps; uwspr_hyp *d_abi_hyps;
  size_t cap_p; float4 *d_p;                      // [H][162] tone magnitudes
  size_t cap_sync; float *d_sync;                 // [H]
  size_t cap_sym; uint8_t *d_sym;                 // [H][162]
  size_t cap_state; uwspr::cand_state *d_state;
  size_t cap_dout; uwspr_demod_out *d_dout;
  // buffers the current call writes (the context's own, or the caller's device memory)
  uwspr_candidate *cur_cands; int32_t *cur_npk; uwspr_demod_out *cur_dout;
  int last_per_frame;
  // Options (uwspr_set_option; defaults in uwspr_api.hip: kOptions).  The ones the launch sequences branch on:
  int opt[UWSPR_NOPT];
  bool opt_set[UWSPR_NOPT];   // set by the caller (environment or uwspr_set_option), not the default
  long long launch_forms[UWSPR_NFORMS] = {};   // launches per form since the context was created (UWSPR_FORM_*)
  bool use_fused;        // "sched" = 1: one workgroup per candidate runs S0..S5 (k6_sched); 0: staged launches
  bool use_stage_kernels;   // "stage_kernels" >= 1: the staged form's packed / ring / rows kernels; 0: the flat kernel for every stage
  bool reuse_centre;     // "reuse": skip the stage-winner hypothesis in S1/S3/S4 and try 0 of S5 (0: recompute it)
  bool use_ptab;         // "phasor_tables": the lag stages read their phasors from per-slot tables (0: every lane runs the recurrence)
  // "fast_search" = 1: stages S0..S4 of the schedule with fused multiply-adds and shuffle-tree sums (not
  // the reference's arithmetic; S5 and every other entry point stay exact).  fast_now: set around those launches.
  bool fast_search, fast_now;
  bool cands_from_fdr;   // the schedule call's candidates are this context's own FDR output (drift within +-maxdrift)
  uint8_t *next_slab = nullptr; int next_slab_K = 0; bool next_slab_done = false;   // uwspr_pipeline_slabs (one shot)
  int sched_per_frame = 1;   // candidate slots per frame of the schedule being launched
  // fused schedule (k6_sched)
  size_t cap_tabs; float *d_tabs;     // [num_cus][2][5][4][256](c, s) phasor tables
  int *d_counter;                     // candidate queue head of the running launch
  size_t cap_tmpc; uwspr_candidate *d_tmpc; size_t cap_tmpn; int32_t *d_tmpn;   // uwspr_demod_batch: host records staged
  // pinned staging for host -> device copies (two halves, ping-pong)
  void *h_pin; hipEvent_t pin_ev[2]; bool pin_busy[2];
  // overlap-aware stream ingest (uwspr_stream_*): the stream tail lives on the device (stream_ring.h)
  uwspr::stream_ring ring; float *d_stream_frames; size_t cap_stream_frames;
  hipEvent_t ring_ev;                 // recorded on `stream` at every take: the readers of earlier views are behind it
  // Frame pitch of the current calls (uwspr_set_frame_stride; default fl = contiguous frames) and the
  // sample bound of the fine search: npoints = 45000 whatever fl is (sync_and_demodulate_impl.cc:92,
  // passed at cc:413-465), capped at fl where the reference would read past its arrays.
  int fstride, np;
  int ntries;                         // mode-2 tries per candidate a schedule call produces (uwspr_set_tries)
  size_t cap_ptab; float2 *d_ptab;    // [nslots][kPtabPerSlot][4][256] phasor tables of the lag stages (staged form)
  size_t cap_pwin; float *d_pwin;     // [nslots][162][4] magnitudes of the stage winner (f1, shift1, drift1): try 0 of stage 5, and what uwspr_demod_resume starts from
  size_t cap_need; uint8_t *d_need;   // staging of the resume mask
  int last_slots, last_sched_B, last_sched_per_frame;
  bool last_sched_lazy; uwspr_demod_out *last_sched_out;   // what uwspr_demod_resume may continue (run_schedule)
  unsigned long long *d_sched_stamps; size_t cap_sched_stamps;   // option "sched_stamps": phase times of the last launch
  size_t cap_slab; uint8_t *d_slab;
  // multi-GPU gather (dist.hip): RCCL communicator of this rank, or null (single rank / not initialised)
  void *dist_comm; int dist_rank, dist_world;
  // transmitter (k7_transmit.hip): composite taps and call scratch, made by the first uwspr_tx_* call
  uwspr::tx_state *tx;
  // subtraction (k8_subtract.hip): window tables and call scratch, made by the first use
  uwspr::sub_state *sub;
  // ordered-statistics decoding (k9_osd.hip): the generator / de-interleave table and call scratch, made by the first use
  uwspr::osd_state *osd;
  // block demodulation (k10_blockdemod.hip): call scratch, made by the first use
  uwspr::blk_state *blk;
  // resampler (k11_resample.hip): the batch call's taps and staging, made by the first use
  uwspr::rs_state *rs;
  // blanker (k12_blank.hip): the batch call's staging and tables, made by the first use
  uwspr::bk_state *bk;
  // list search (k13_deep.hip): the list's table and call scratch, made by uwspr_deep_set_list / the first use
  uwspr::deep_state *deep;
  // call search (k14_calls.hip): the call set and call scratch, made by uwspr_calls_set / the first use
  uwspr::calls_state *calls;
  // trajectory fit (k15_track.hip): the set's tables and call scratch, made by uwspr_track_set
  uwspr::trk_state *trk;
  // blind demodulation along passes (k16_follow.hip): the set and call scratch, made by uwspr_follow_set
  uwspr::fol_state *fol;

  int prof_mask;
  std::vector<uwspr::ev_pair> prof_events;
  std::vector<hipEvent_t> ev_pool;
};

namespace uwspr {

// frames of a batch call -> device pointer (host frames are staged in the context; uwspr_api.hip)
int api_frames_on_device(uwspr_ctx *c, const float *frames, int B, int where, const float **dev);
// K8 (k8_subtract.hip): slot s of dst [nslots][fl] = input frame slot_frame[s] (null: s) with the items whose `frame` is s
// taken out, in list order; items are host records that passed subtract_check (sorted by frame, frames in [0, nframes),
// symbols 0..3, finite f / drift, bounded shift: UWSPR_ERR_ARG with a message otherwise)
int subtract_check(uwspr_ctx *c, const uwspr_sub_item *items, int nitems, int nframes);
int subtract_run(uwspr_ctx *c, const float *src, size_t stride, int nslots, const int *slot_frame, const uwspr_sub_item *items,
                 int nitems, int refine, float *dst);

// K9 (k9_osd.hip): n items on the context's stream, item i = the 162 interleaved soft symbols at base + off[i] (off: host
// array, null = 162 i; base: device memory); results to res (device memory), or with res null to a buffer of the context
// handed back through *res_out.  order 0..2 (the caller checks it).
int osd_run(uwspr_ctx *c, const uint8_t *base, const unsigned long long *off, int n, int order, uwspr_osd_result *res,
            uwspr_osd_result **res_out);

// K13 (k13_deep.hip): n > 0 items on the context's stream against a table of M messages in the kernel's operand layout
// (d_tab: device memory made from deep_build_table; null = the list of uwspr_deep_set_list), item i = the 162 interleaved
// soft symbols at base + off[i] (off: host array, null = 162 i; base: device memory); results to res (device memory), or
// with res null to a buffer of the context handed back through *res_out.  deep_check_list: null when the list keeps the
// rules at uwspr_deep_set_list, else what is wrong (written into msg).
int deep_run(uwspr_ctx *c, const int8_t *d_tab, int M, const uint8_t *base, const unsigned long long *off, int n,
             uwspr_deep_result *res, uwspr_deep_result **res_out);
const char *deep_check_list(const int8_t *messages7, int M, char *msg, size_t cap);
int deep_build_table(const int8_t *messages7, int M, std::vector<int8_t> &tab);

// K14 (k14_calls.hip): a call set is checked (calls_check: null when it keeps the rules at uwspr_calls_set, else what is
// wrong, no device asked) and built into memory of the current device (calls_build: null with *status and msg on failure;
// read-only from then on, freed by calls_free_set).  calls_run: n > 0 items on the context's stream against a set (null =
// the set of uwspr_calls_set), items and results as at deep_run.  calls_message: message(h) of a set; calls_count: its
// number of allowed hypotheses.
const char *calls_check(const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask, int32_t *n1_out,
                        char *msg, size_t cap);
calls_set *calls_build(const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask, int *status, char *msg, size_t cap);
void calls_free_set(calls_set *s);
int calls_run(uwspr_ctx *c, const calls_set *set, const uint8_t *base, const unsigned long long *off, int n,
              uwspr_call_result *res, uwspr_call_result **res_out);
void calls_message(const calls_set *s, int h, int8_t *message7);
long long calls_count(const calls_set *s);

// K10 (k10_blockdemod.hip): nitems > 0 items (host records that passed blockdemod_check against the frames of src: sorted by
// frame, frames in [0, nframes), finite f / drift, bounded shift) on the context's stream; src: device frames, frame b at
// src + 2 stride b floats; the [nitems][3][162] bytes go to out (device memory), or with out null to a buffer of the
// context handed back through *out_dev
int blockdemod_check(uwspr_ctx *c, const uwspr_block_item *items, int nitems, int nframes);
int blockdemod_run(uwspr_ctx *c, const float *src, size_t stride, const uwspr_block_item *items, int nitems, uint8_t *out,
                   uint8_t **out_dev);

// K15 (k15_track.hip): a trajectory set is checked (track_check: null when it keeps the rules at uwspr_track_set, else what
// is wrong, no device asked) and built into memory of the current device (track_build: null with *status and msg on
// failure; read-only from then on, freed by track_free_set).  track_run: nitems > 0 items (host records that passed
// subtract_check) on the context's stream against a set (null = the set of uwspr_track_set); src: device frames, frame b at
// src + 2 stride b floats; results to res and the surface to surface (device memory), or with either null to a buffer of
// the context (the results' handed back through *res_out).
// A trajectory set on the current device: read-only once built (track_build), so one set serves every lane of a pipe.
// K16's sets are the same object (the tables are exactly uwspr_track_design's).
struct trk_set {
  int n = 0, qf = 0, model = 0;
  double *d_dfreq = nullptr; int32_t *d_tau = nullptr;   // [162][n]
};
const char *track_check(const uwspr_track_traj *traj, int n, int nmax, int qf, int model, char *msg, size_t cap);
trk_set *track_build(const uwspr_track_traj *traj, int n, int qf, int model, double cf, int *status, char *msg, size_t cap);
void track_free_set(trk_set *s);
int track_run(uwspr_ctx *c, const trk_set *set, const float *src, size_t stride, const uwspr_sub_item *items, int nitems,
              uwspr_track_result *res, float *surface, uwspr_track_result **res_out);

// K16 (k16_follow.hip): a follow set is a trajectory set (track_check / track_build, qf the reach in steps of df / 8) and a
// lag reach nl (follow_check: null, or what is wrong).  follow_run: nitems > 0 items (host records that passed
// blockdemod_check) on the context's stream against a set (null = the set of uwspr_follow_set); results, the [nitems][162]
// bytes and the surface go to res / symbols / surface (device memory), or with any of them null to buffers of the context
// (results and bytes handed back through *res_out / *sym_out).
struct fol_set {
  trk_set *t = nullptr;
  int nl = 0;
  float2 *d_W = nullptr;   // the 2048 roots of unity e^{-j 2 pi m / 2048}, made on the device by k16_roots
};
const char *follow_check(const uwspr_track_traj *traj, int n, int qf, int nl, int model, char *msg, size_t cap);
fol_set *follow_build(const uwspr_track_traj *traj, int n, int qf, int nl, int model, double cf, int *status, char *msg, size_t cap);
void follow_free_set(fol_set *s);
int follow_run(uwspr_ctx *c, const fol_set *set, const float *src, size_t stride, const uwspr_block_item *items, int nitems,
               uwspr_follow_result *res, uint8_t *symbols, float *surface, uwspr_follow_result **res_out, uint8_t **sym_out);

// ---- launchers (each enqueues on ctx->stream) ------------------------------
int frontend_design(int mode, int stage, std::vector<double> &out, int *delay);
int frontend_tap_image(int mode, std::vector<float> &img, int *J, int *dcols);
// the same at centre fc and half-bandwidth hb (integer Hz; frontend_carrier_ok says which are allowed)
int frontend_design_at(int mode, int fc, int hb, int stage, std::vector<double> &out, int *delay);
// firdes::low_pass(1, fs, cutoff, tw, WIN_HAMMING) as GNU Radio 3.7 designs it (binary32 taps; k0_frontend.hip)
std::vector<float> lowpass_hamming(double fs, double cutoff, double tw);
int frontend_prepare();
double gr_izero(double x);   // I0 as K0's Kaiser windows compute it (k0_frontend.hip)
// K11 (k11_resample.hip): the batch call and the one-launch door behind uwspr_resample_batch / uwspr_debug_resample_launch
// (arguments checked by the callers); launches of the kernel per input format since the process started
int rs_batch(uwspr_ctx *c, const void *audio, long long nin, int nch, int s16, int rate, int where, float *out, long long nout);
int rs_debug_launch(uwspr_ctx *c, const void *audio_dev, int s16, long long nin, long long in0, int nch, int rate, float *out_dev,
                    long long nout, long long j_first);
long long resample_launch_count(int s16);
// K12 (k12_blank.hip): the batch call and the one-launch door behind uwspr_blank_batch / uwspr_debug_blank_launch
// (arguments checked by the callers); launches per kernel and input format (0, 1: k12_level float, int16; 2, 3: k12_apply)
int bk_batch(uwspr_ctx *c, const void *audio, long long nin, int nch, int s16, int where, int blank, int guard, float *out,
             float *med, int *nzero);
int bk_debug_launch(uwspr_ctx *c, const void *audio_dev, int s16, long long nin, long long in0, int nch, float *lev_dev,
                    long long nlev, long long blk0, long long level_first, long long level_n, int blank, int guard, float *out_dev,
                    long long nout, long long y_first, int *nz_dev);
long long blank_launch_count(int which);
int ring_blank_stats(stream_ring &r, long long *samples, long long *zeroed, int cap);   // uwspr_api.hip
const char *chain_refusal(chain_part part, const audio_chain_cfg &want, const audio_chain_cfg &have, char (&buf)[160]);   // uwspr_api.hip
const char *chain_part_name(chain_part part);
void launch_frontend(uwspr_ctx *c, const float *audio, int B, int nin, float2 *out, int nout);
void launch_spectrogram(uwspr_ctx *c, const float *frames, int B);
void launch_spectrum(uwspr_ctx *c, int B);
void launch_coarse(uwspr_ctx *c, int B);
void launch_prep_hyps(uwspr_ctx *c, const uwspr_hyp *abi, dev_hyp *out, int H);
// flat form; taken != null: hypotheses of groups that have their phasor table are left alone (see k4_tonecorr);
// skip_pairs: stage S2 -- the mirrored drift tries launch_tonecorr_dpair computes are left alone
void launch_tonecorr(uwspr_ctx *c, const float *frames, int B, const dev_hyp *hyps, int H,
                     float4 *p, const dev_grp *taken = nullptr, int hyps_per_grp = 1, bool skip_pairs = false);
// stage S2 (hyps 2 s, 2 s + 1 = the two drift tries of slot s): the slots whose tries mirror each other (k4_pair.hip)
void launch_tonecorr_dpair(uwspr_ctx *c, const float *frames, int B, const dev_hyp *hyps, int nslots, float4 *p);
void launch_tonecorr_lag0(uwspr_ctx *c, const float *frames, int B, const dev_grp *grps, int nslots,
                          int64_t nhyps, float4 *p);
void launch_tonecorr_fstage(uwspr_ctx *c, const float *frames, int B, const dev_hyp *hyps, int nslots,
                            int64_t nhyps, float4 *p);
void launch_tonecorr_ring(uwspr_ctx *c, const float *frames, int B, const dev_grp *grps, int G,
                          int NL, int step, int64_t nhyps, float4 *p, int groups_per_slot = 1);
// S5's jiggered shifts with the sample pairs in a register ring (k4_jig.hip)
void launch_tonecorr_jig(uwspr_ctx *c, const float *frames, int B, const dev_grp *grps, int G, int64_t nhyps, float4 *p,
                         int groups_per_slot);
// grid form (one centre per frame, shared sample windows); false = does not fit, use the flat path
bool launch_tonecorr_grid(uwspr_ctx *c, const float *frames, int B, const uwspr_candidate *centres,
                          int nf, const float *df, int ndrift, const float *ddrift, int nlag,
                          const int *dlag_host, const int *dlag_dev, dev_hyp *hyps, float4 *p);
void launch_fold(uwspr_ctx *c, const dev_hyp *hyps, const float4 *p, int H, float *sync,
                 uint8_t *symbols, const float4 *pwin = nullptr, int per_slot = 1);
void launch_keep_try0(uwspr_ctx *c, int nslots, int njig);
// schedule stages; see k5_schedule.hip
void launch_sched_init(uwspr_ctx *c, const uwspr_candidate *cands, const int32_t *npk,
                       int cand_stride, int B, int per_frame);
void launch_fold_step(uwspr_ctx *c, int stage, int ncand, int njig = UWSPR_NJIG);
void launch_pack_slabs(uwspr_ctx *c, const uwspr_candidate *cands, const int32_t *npk,
                       const uwspr_demod_out *dout, int per_frame, int K, uint8_t *slab, int B);
void launch_sched_finish(uwspr_ctx *c, int ncand, int njig = UWSPR_NJIG);
// the whole schedule in one launch (k6_sched.hip); njig = mode-2 tries to produce (17 = all)
void launch_sched_fused(uwspr_ctx *c, const float *frames, int B, const uwspr_candidate *cands,
                        const int32_t *npk, int cand_stride, int per_frame, uwspr_demod_out *out,
                        int njig, const uint8_t *resume = nullptr);
constexpr int kSchedTabFloats = 2 * 5 * 4 * 512;   // per resident workgroup

// profiling brackets
struct prof_scope {
  uwspr_ctx *c; int idx; bool ext;
  // ext = false: events recorded on the stream before / after the bracketed launches (one
  // marker packet each).  ext = true: the ONE launch inside the scope goes through
  // launch_timed(), which hands the pair to hipExtLaunchKernelGGL -- the kernel's own dispatch
  // packet carries the time stamps and no extra packet (and no ~5 us bubble) enters the queue.
  prof_scope(uwspr_ctx *c, int kind, int64_t units, bool ext = false);
  ~prof_scope();
};

template <typename K, typename... A>
inline void launch_timed(uwspr_ctx *c, prof_scope &ps, K kernel, dim3 grid, dim3 block, size_t shmem,
                         A... args) {
  if (ps.idx >= 0 && ps.ext)
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shmem, c->stream, c->prof_events[ps.idx].a,
                          c->prof_events[ps.idx].b, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, shmem, c->stream, args...);
}

}  // namespace uwspr
