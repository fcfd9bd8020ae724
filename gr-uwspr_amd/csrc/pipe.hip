// pipe.hip -- the pipelined end-to-end decoder of include/uwspr_hip.h (uwspr_pipe_*): host code only,
// built on the C ABI's own entry points, so what it produces is by construction what the sequential
// calls produce -- only the ORDER IN TIME of the stages of consecutive batches differs:
//
//   producer thread (the caller)      copy stream          lane k's HIP stream           coordinator + pool
//   acquire / fill / commit  ------>  H2D of new samples
//   batch complete: view in place --------------------->   K1 K2 K3, schedule (try 0),
//                                                          D2H of records, event  ---->  wait event
//   (next batch: lane k+1 ...)                                                           Fano on try 0 (pool; one
//                                                                                        coordinator per lane)
//                                                          resume (tries 1..16) <------  for what did not decode
//                                                          D2H, event            ---->   Fano on tries 1..16
//                                                                                        results in frame order
//
// Reference: the flowgraph chain sliding_window_stream_to_pdu -> FDR -> sync_and_demodulate
// (lib/sliding_window_stream_to_pdu_impl.cc:97-138, lib/FDR_impl.cc:214-456,
// lib/sync_and_demodulate_impl.cc:315-534; the lazy tries are cc:457-490's early exit).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "host_pool.h"
#include "pipe_rules.h"
#include "uwspr_internal.h"

using namespace uwspr;

namespace {

constexpr int kPipeStreams = 3;   // HIP streams the lanes share (see uwspr_pipe_open)

struct pipe_lane {
  uwspr_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  uwspr_candidate *d_cands = nullptr; int32_t *d_npk = nullptr; uwspr_demod_out *d_out = nullptr; uint8_t *d_need = nullptr;
  uwspr_candidate *h_cands = nullptr; int32_t *h_npk = nullptr; uwspr_demod_out *h_out = nullptr; uint8_t *h_need = nullptr;
  hipEvent_t ev_done = nullptr;
  // the batch in flight
  bool busy = false;       // taken by the producer, until its records have been emitted
  bool launched = false;   // its GPU work is enqueued: a coordinator may pick it up
  bool claimed = false;    // a coordinator has
  double host_since = 0.0; // > 0: its first GPU pass is complete and it has been in its host tail since then (now_s())
  int64_t seq = 0;         // batch number (emission order)
  std::vector<uwspr_decode> recs;   // the batch's records, built by the coordinator, emitted in batch order
  int B = 0, stride = 0, channel = 0;
  const float *frames = nullptr;
  int64_t frame0 = 0, pos0 = -1;
  std::vector<uint8_t> dec;          // [B*per] decoded flags
  std::vector<int32_t> idt;          // [B*per]
  std::vector<int8_t> msg;           // [B*per][7]
  std::vector<int> first;            // records whose first pass goes to the pool
  std::vector<int> redo;             // records resumed
  std::vector<int> tasks;            // (record << 5) | try: the resumed tries, decoded in parallel
  std::vector<uint8_t> task_ok;
  std::vector<int8_t> task_msg;
  // second pass (option "passes" = 2): the frames that decoded, with their decoded signals taken out, [slots][fl]
  float *d_res2 = nullptr; size_t cap_res2 = 0;
  std::vector<int> slot_frame;           // slot -> frame of the batch
  std::vector<uwspr_sub_item> items;     // the decoded records as subtraction items (frame = slot)
  std::vector<uwspr_decode> extra;       // the second pass's records, frame = index in the batch until they are merged
  // The fallbacks (option "block", the list search, the call search, option "osd"): the records Fano gave up on, one item
  // each.  They run one after the other on a lane, so they share one set of item vectors.
  std::vector<uint8_t> osdf;                 // [B*per] 1, 2, 3: decoded by K9, K13, K14
  std::vector<uint8_t> blkf;                 // [B*per] 2, 3: decoded from the soft symbols of that block length
  std::vector<int> fb_rec, fb_idt;           // item -> record, try (collect_items)
  std::vector<unsigned long long> fb_off;    // item -> byte offset of its symbols in d_out
  std::vector<uint8_t> fb_res;               // the running fallback's results as the kernel wrote them: [items] of its result
                                             // record (scored_tail), or K10's [items][3][162] soft symbols (block_tail)
  std::vector<uwspr_block_item> blk_items;
  std::vector<uint8_t> blk_n;                // item -> the block length that decoded (0: none)
  std::vector<int8_t> blk_msg;               // [items][7]
  // trajectory fit (uwspr_pipe_set_tracks): the decoded records of the running search as K15 items
  std::vector<uwspr_sub_item> trk_items;
  std::vector<int> trk_rec;                      // item -> record
  std::vector<uwspr_track_result> trk_fetch;     // [items] as the kernel wrote them
  std::vector<uwspr_track_result> trk_by_rec;    // [B*per]: the fit of record i of the running search, where it decoded
  std::vector<uwspr_track_result> rec_trk;       // beside recs: the fit of each decoded record
  std::vector<uwspr_track_record> trecs;         // the batch's track records, emitted with recs
  // blind demodulation along passes (uwspr_pipe_set_follow): what Fano gave up on as K16 items
  std::vector<uwspr_block_item> fol_items;
  std::vector<uwspr_follow_result> fol_fetch;    // [items] as the kernel wrote them
  std::vector<uint8_t> fol_ok;                   // item -> the bytes decoded
  std::vector<int8_t> fol_msg;                   // [items][7]
  std::vector<uwspr_follow_result> fol_by_rec;   // [B*per]: the fit of record i of the running search, where K16 decoded it
  std::vector<uwspr_follow_result> rec_fol;      // beside recs: the fit of each record K16 decoded
  std::vector<uwspr_follow_record> frecs;        // the batch's follow records, emitted with recs
};

// what the host tails of a batch add to the pipe's statistics
struct tail_acc {
  long long calls = 0, fails = 0, resumed = 0;
  double gpu_wait_s = 0.0, fano_s = 0.0, resume_s = 0.0;
};

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct uwspr_pipe {
  uwspr_params p;
  uwspr_pipe_opts o;
  int device = 0, fl = 0, maxfreqs = 0, per = 1;
  int passes = 1;   // uwspr_pipe_set_option("passes"): 2 = subtract what decoded and search the residual again
  int osd = 0, osd_gap = UWSPR_OSD_GAP_DEFAULT;   // uwspr_pipe_set_option("osd" / "osd_gap"): K9 on what Fano timed out on
  // uwspr_pipe_set_list / uwspr_pipe_set_option("deep_min" / "deep_gap"): K13 on those records against the list; one device
  // table for all lanes (made and freed by set_list, read-only in between), the list's bytes on the host
  int deep_M = 0, deep_min = UWSPR_DEEP_MIN_DEFAULT, deep_gap = UWSPR_DEEP_GAP_DEFAULT;
  int8_t *d_deep_tab = nullptr;
  std::vector<int8_t> deep_msgs;
  // uwspr_pipe_set_calls / uwspr_pipe_set_option("call_min" / "call_gap"): K14 on those records against the call set; one
  // device set for all lanes (made and freed by set_calls, read-only in between)
  calls_set *call_set = nullptr;
  int call_min = UWSPR_CALL_MIN_DEFAULT, call_gap = UWSPR_CALL_GAP_DEFAULT;
  // uwspr_pipe_set_tracks: K15 on every decoded record against the trajectory set; one device set for all lanes (made and
  // freed by set_tracks, read-only in between)
  trk_set *track_set = nullptr;
  // uwspr_pipe_set_follow: K16 on what Fano gave up on, against the follow set; one device set for all lanes (made and freed
  // by set_follow, read-only in between)
  fol_set *follow_set = nullptr;
  int block = 0;    // uwspr_pipe_set_option("block"): 2, 3 = K10's soft symbols of block lengths 2 .. block for those records
  int audio_rate = 12000;   // uwspr_pipe_set_option("audio_rate"): the rate of the pushed audio (12000: no resampler, else K11 ahead of K0)
  int blank = 0, blank_guard = 2;   // uwspr_pipe_set_option("blank" / "blank_guard"): K12 ahead of K11 / K0 (blank 0: off)
  std::vector<int> carriers = std::vector<int>(1, UWSPR_CARRIER_DEFAULT);   // uwspr_pipe_set_carriers: K0's centres in Hz, in plane order
  int frontend_hbw = UWSPR_FRONTEND_HBW_DEFAULT;                            // uwspr_pipe_set_option("frontend_hbw")
  char err[512];
  // Sticky status of the first RUNTIME failure (HIP, a lane's context), written by coordinators and the producer, read
  // by both without the lock.  Argument errors are not sticky: the call that made them returns UWSPR_ERR_ARG (with
  // its message), nothing in flight is harmed and the pipe goes on.
  std::atomic<int> failed{0};
  std::atomic<int64_t> inject_seq{-1}; std::atomic<int> inject_where{0};   // uwspr_pipe_inject_failure (tests): read by the coordinators and the producer without q->m

  std::vector<pipe_lane> lanes;
  double spare_after = 2.5e-3;   // seconds of host tail after which a spare lane may open (take_lane)
  int next_lane = 0;
  int64_t next_frame[UWSPR_PIPE_MAX_CHANNELS] = {};   // per channel (submitted frames and (I,Q) streams: channel 0)

  stream_ring ring;
  static constexpr int NSTAGE = 4;
  float *h_stage[NSTAGE] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_ev[NSTAGE] = {nullptr, nullptr, nullptr, nullptr};
  bool stage_busy[NSTAGE] = {false, false, false, false};
  int stage_next = 0, stage_cur = -1;
  size_t stage_samples = 0;

  std::mutex m;
  std::condition_variable cv_lane, cv_work, cv_done, cv_turn;
  std::deque<uwspr_decode> done;
  std::deque<uwspr_track_record> done_trk;   // uwspr_pipe_collect_tracks: pushed with the decode records they belong to
  std::deque<uwspr_follow_record> done_fol;  // uwspr_pipe_collect_follows: likewise
  bool stop = false;
  int64_t next_seq = 0, emit_seq = 0;     // batches launched / emitted (records leave in batch order)
  std::vector<std::thread> coords;         // one coordinator per lane: the host tails of consecutive batches overlap
  host_pool *pool = nullptr;
  bool own_pool = false;
  uwspr_pipe_stats st;
};

static int pfail(uwspr_pipe *q, int status, const char *fmt, ...) {
  if (q) {
    std::lock_guard<std::mutex> lk(q->m);
    if (!q->failed.load()) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(q->err, sizeof(q->err), fmt, ap);
      va_end(ap);
      q->failed.store(status);
    }
  }
  if (q) q->cv_done.notify_all();   // (a collector waiting for records learns of the failure)
  return status;
}
// an argument error of the calling thread: message, status, nothing sticky
static int parg(uwspr_pipe *q, const char *fmt, ...) {
  if (q) {
    std::lock_guard<std::mutex> lk(q->m);
    if (!q->failed.load()) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(q->err, sizeof(q->err), fmt, ap);
      va_end(ap);
    }
  }
  return UWSPR_ERR_ARG;
}

#define PHIP(q, call)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) return pfail((q), UWSPR_ERR_HIP, "%s failed: %s (%s:%d)", #call,          \
                                       hipGetErrorString(e_), __FILE__, __LINE__);                  \
  } while (0)

// ---- coordinator: finishes the batches in launch order ------------------------------------------
// record i of the lane's search (frame i / per, slot i % per) holds a candidate
static bool lane_valid(const uwspr_pipe *q, const pipe_lane &L, int i) {
  const int b = i / q->per, j = i - b * q->per;
  return j < L.h_npk[b] && j < q->maxfreqs;
}

// device -> host on the lane's stream, waited for on the lane's event (the coordinator sleeps on it)
static int lane_fetch(uwspr_pipe *q, pipe_lane &L, void *dst, const void *src, size_t bytes) {
  PHIP(q, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, L.stream));
  PHIP(q, hipEventRecord(L.ev_done, L.stream));
  PHIP(q, hipEventSynchronize(L.ev_done));
  return UWSPR_OK;
}

// what a search of n frames left in the lane's device buffers -> its host records; the lane's event is behind the copies
static int fetch_first_pass(uwspr_pipe *q, pipe_lane &L, int n) {
  const int per = q->per;
  PHIP(q, hipMemcpyAsync(L.h_npk, L.d_npk, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  PHIP(q, hipMemcpy2DAsync(L.h_cands, (size_t)per * sizeof(uwspr_candidate), L.d_cands,
                           (size_t)q->maxfreqs * sizeof(uwspr_candidate), (size_t)per * sizeof(uwspr_candidate), n,
                           hipMemcpyDeviceToHost, L.stream));
  PHIP(q, hipMemcpyAsync(L.h_out, L.d_out, (size_t)n * per * sizeof(uwspr_demod_out), hipMemcpyDeviceToHost, L.stream));
  PHIP(q, hipEventRecord(L.ev_done, L.stream));
  return UWSPR_OK;
}

// ---- the fallback path: what runs on the records Fano gave up on.  A fallback supplies a kernel call on the lane's
// context, a failure prefix, an acceptance rule (pipe_rules.h) and where the 7 message bytes come from (scored_fallback); one
// whose results need host work of their own is written out like block_tail, on the same collection and fetch.
// The item rule of all of them: record i is an item when it was worth a try, no try decoded and at least one try passed the
// gates of cc:470; its try is rules::fallback_pick's (-1: no item).  All 17 tries are in L.d_out by now (the resume, or the
// eager first pass).
static int fallback_try(const uwspr_pipe *q, const pipe_lane &L, int i) {
  if (!lane_valid(q, L, i) || !L.h_out[i].worth_a_try || L.dec[i]) return -1;
  return rules::fallback_pick(L.h_out[i]);
}

// the items of the fallback that runs next, into L.fb_rec / L.fb_idt: collected afresh by each one, so that a record the
// fallback before decoded is no item any more
static int collect_items(const uwspr_pipe *q, pipe_lane &L, int nrec) {
  L.fb_rec.clear(); L.fb_idt.clear();
  for (int i = 0; i < nrec; i++) {
    const int pick = fallback_try(q, L, i);
    if (pick < 0) continue;
    L.fb_rec.push_back(i); L.fb_idt.push_back(pick);
  }
  return (int)L.fb_rec.size();
}

// where the symbols of try `pick` of record i lie in the lane's device records: they are read in place
static unsigned long long symbols_offset(const pipe_lane &L, int i, int pick) {
  return (unsigned long long)((const char *)&L.d_out[i].symbols[pick][0] - (const char *)L.d_out);
}

// A fallback that scores an item's 162 soft symbols and answers with one result record per item.
struct scored_fallback {
  const char *what;     // prefix of a failure's message
  uint8_t osdf;         // uwspr_decode::osd of a record it decodes
  size_t res_size;      // bytes of its result record
  int (*run)(uwspr_pipe *q, pipe_lane &L, int n, const void **d_res);           // n items at L.fb_off -> device results
  bool (*accept)(const uwspr_pipe *q, const void *res);                         // the result makes its record a decoded one
  void (*message)(const uwspr_pipe *q, const void *res, int8_t *message7);      // ... with these bytes
};

// Option "osd": K9.  An item whose runner-up is at least osd_gap behind and whose bytes unpack.
static const scored_fallback kOsdFallback = {
    "ordered-statistics decoding", 1, sizeof(uwspr_osd_result),
    [](uwspr_pipe *q, pipe_lane &L, int n, const void **d_res) {
      return osd_run(L.ctx, (const uint8_t *)L.d_out, L.fb_off.data(), n, q->osd, nullptr, (uwspr_osd_result **)d_res);
    },
    [](const uwspr_pipe *q, const void *res) {
      const uwspr_osd_result &r = *(const uwspr_osd_result *)res;
      char text[32];
      return rules::osd_accepts(r, q->osd_gap) && uwspr_unpack_message(r.message, text, sizeof(text)) == 0;
    },
    [](const uwspr_pipe *, const void *res, int8_t *message7) { memcpy(message7, ((const uwspr_osd_result *)res)->message, 7); }};

// The list search (uwspr_pipe_set_list): K13 against the pipe's table.  An item with sbest >= deep_min and (M == 1 or
// sbest - snext >= deep_gap), with the list's bytes (no unpacking: the list is the user's word).
static const scored_fallback kListFallback = {
    "list search", 2, sizeof(uwspr_deep_result),
    [](uwspr_pipe *q, pipe_lane &L, int n, const void **d_res) {
      return deep_run(L.ctx, q->d_deep_tab, q->deep_M, (const uint8_t *)L.d_out, L.fb_off.data(), n, nullptr, (uwspr_deep_result **)d_res);
    },
    [](const uwspr_pipe *q, const void *res) { return rules::list_accepts(*(const uwspr_deep_result *)res, q->deep_M, q->deep_min, q->deep_gap); },
    [](const uwspr_pipe *q, const void *res, int8_t *message7) {
      memcpy(message7, &q->deep_msgs[7 * (size_t)((const uwspr_deep_result *)res)->best], 7);
    }};

// The call search (uwspr_pipe_set_calls): K14 against the pipe's call set.  An item with sbest >= call_min and (one allowed
// hypothesis or sbest - snext >= call_gap), with message(best) (no unpacking: the message is valid by construction).
static const scored_fallback kCallFallback = {
    "call search", 3, sizeof(uwspr_call_result),
    [](uwspr_pipe *q, pipe_lane &L, int n, const void **d_res) {
      return calls_run(L.ctx, q->call_set, (const uint8_t *)L.d_out, L.fb_off.data(), n, nullptr, (uwspr_call_result **)d_res);
    },
    [](const uwspr_pipe *q, const void *res) {
      return rules::calls_accepts(*(const uwspr_call_result *)res, calls_count(q->call_set), q->call_min, q->call_gap);
    },
    [](const uwspr_pipe *q, const void *res, int8_t *message7) { calls_message(q->call_set, ((const uwspr_call_result *)res)->best, message7); }};

// One scored fallback over the batch's records.  Its time counts as resume time; without items it touches no stream.
static int scored_tail(uwspr_pipe *q, pipe_lane &L, int nrec, const scored_fallback &f, tail_acc &ta) {
  const int n = collect_items(q, L, nrec);
  if (n == 0) return UWSPR_OK;
  const double t0 = now_s();
  L.fb_off.clear();
  for (int k = 0; k < n; k++) L.fb_off.push_back(symbols_offset(L, L.fb_rec[k], L.fb_idt[k]));
  const void *d_res = nullptr;
  int rc = f.run(q, L, n, &d_res);
  if (rc) return pfail(q, rc, "%s: %s", f.what, uwspr_last_error(L.ctx));
  L.fb_res.resize((size_t)n * f.res_size);
  if ((rc = lane_fetch(q, L, L.fb_res.data(), d_res, L.fb_res.size()))) return rc;
  for (int k = 0; k < n; k++) {
    const void *r = &L.fb_res[(size_t)k * f.res_size];
    if (!f.accept(q, r)) continue;
    const int i = L.fb_rec[k];
    L.dec[i] = 1; L.idt[i] = L.fb_idt[k]; L.osdf[i] = f.osdf;
    f.message(q, r, &L.msg[7 * (size_t)i]);
  }
  ta.resume_s += now_s() - t0;
  return UWSPR_OK;
}

// Option "block".  K10 makes each item's soft symbols for the block lengths 1, 2, 3 from the frames the search itself read,
// at the try's jig_shift and the frequency model the fine search correlated with (rules::fine_model).  On the host pool, per
// item: for n = 2 .. block, a vector above the rms gate of cc:470 goes through Fano; the first that decodes to bytes that
// unpack makes the record a decoded one.  Its time counts as resume time, its Fano calls as the batch's.
static int block_tail(uwspr_pipe *q, pipe_lane &L, const float *frames, int nrec, tail_acc &ta) {
  const int per = q->per;
  const int n = collect_items(q, L, nrec);
  if (n == 0) return UWSPR_OK;
  L.blk_items.clear();
  for (int k = 0; k < n; k++) {
    const int i = L.fb_rec[k];
    uwspr_block_item it;
    it.frame = i / per;
    it.shift = L.h_out[i].jig_shift[L.fb_idt[k]];
    rules::fine_model(L.h_cands[i], L.h_out[i], (float)q->p.cf, &it.f_hz, &it.drift_hz);   // (h_cands is [B][per], as h_out)
    L.blk_items.push_back(it);
  }
  const double t0 = now_s();
  uint8_t *d_sym = nullptr;
  int rc = blockdemod_check(L.ctx, L.blk_items.data(), n, (nrec + per - 1) / per);
  if (!rc) rc = blockdemod_run(L.ctx, frames, (size_t)L.ctx->fstride, L.blk_items.data(), n, nullptr, &d_sym);
  if (rc) return pfail(q, rc, "block demodulation: %s", uwspr_last_error(L.ctx));
  std::vector<uint8_t> &blk_sym = L.fb_res;   // [items][3][162]
  blk_sym.resize((size_t)n * 3 * UWSPR_NSYM);
  if ((rc = lane_fetch(q, L, blk_sym.data(), d_sym, blk_sym.size()))) return rc;
  L.blk_n.assign((size_t)n, 0);
  L.blk_msg.assign((size_t)n * 7, 0);
  std::atomic<long long> calls(0), fails(0);
  const int nmax = q->block;
  auto one = [&](int k) {
    for (int nb = 2; nb <= nmax; nb++) {
      uint8_t sym[UWSPR_NSYM], data[11];
      memcpy(sym, &blk_sym[((size_t)k * 3 + (nb - 1)) * UWSPR_NSYM], UWSPR_NSYM);
      float sq = 0.0f;   // cc:469-474
      for (int i = 0; i < UWSPR_NSYM; i++) { const float y = (float)((double)(float)sym[i] - 128.0); sq += y * y; }
      if (!((float)sqrt((double)sq / 162.0) > rules::kMinRms)) continue;
      uwspr_deinterleave(sym);
      memset(data, 0, sizeof(data));
      uint32_t metric, cycles, maxnp;
      calls.fetch_add(1, std::memory_order_relaxed);
      if (uwspr_fano_decode(sym, data, &metric, &cycles, &maxnp, 60, 10000) != 0) { fails.fetch_add(1, std::memory_order_relaxed); continue; }
      int8_t msg[7];
      char text[32];
      for (int i = 0; i < 7; i++) msg[i] = (int8_t)data[i];
      if (uwspr_unpack_message(msg, text, sizeof(text)) != 0) continue;
      L.blk_n[k] = (uint8_t)nb;
      memcpy(&L.blk_msg[7 * (size_t)k], msg, 7);
      return;
    }
  };
  if (n <= 2) for (int k = 0; k < n; k++) one(k);
  else q->pool->run(n, q->o.host_threads, one);
  for (int k = 0; k < n; k++) {
    if (!L.blk_n[k]) continue;
    const int i = L.fb_rec[k];
    L.dec[i] = 1; L.idt[i] = L.fb_idt[k]; L.blkf[i] = L.blk_n[k];
    memcpy(&L.msg[7 * (size_t)i], &L.blk_msg[7 * (size_t)k], 7);
  }
  ta.calls += calls.load(); ta.fails += fails.load();
  ta.resume_s += now_s() - t0;
  return UWSPR_OK;
}

// uwspr_pipe_set_follow.  K16 demodulates each item -- the common rule's: collect_items -- along the set's passes from the
// frames the search itself read, at the try's jig_shift and the frequency model the fine search correlated with
// (rules::fine_model), as "block" does.  An item whose result and bytes pass rules::follow_gates goes through de-interleave
// and Fano on the host pool; bytes that unpack make the record a decoded one with osd = 4, and its fit goes to
// L.fol_by_rec.  Its time counts as resume time, its Fano calls as the batch's.
static int follow_tail(uwspr_pipe *q, pipe_lane &L, const float *frames, int nrec, tail_acc &ta) {
  const int per = q->per;
  const int n = collect_items(q, L, nrec);
  if (n == 0) return UWSPR_OK;
  L.fol_items.clear();
  for (int k = 0; k < n; k++) {
    const int i = L.fb_rec[k];
    uwspr_block_item it;
    it.frame = i / per;
    it.shift = L.h_out[i].jig_shift[L.fb_idt[k]];
    rules::fine_model(L.h_cands[i], L.h_out[i], (float)q->p.cf, &it.f_hz, &it.drift_hz);
    L.fol_items.push_back(it);
  }
  const double t0 = now_s();
  uwspr_follow_result *d_res = nullptr;
  uint8_t *d_sym = nullptr;
  int rc = blockdemod_check(L.ctx, L.fol_items.data(), n, (nrec + per - 1) / per);
  if (!rc) rc = follow_run(L.ctx, q->follow_set, frames, (size_t)L.ctx->fstride, L.fol_items.data(), n, nullptr, nullptr, nullptr, &d_res, &d_sym);
  if (rc) return pfail(q, rc, "follow: %s", uwspr_last_error(L.ctx));
  L.fol_fetch.resize((size_t)n);
  if ((rc = lane_fetch(q, L, L.fol_fetch.data(), d_res, (size_t)n * sizeof(uwspr_follow_result)))) return rc;
  std::vector<uint8_t> &fol_sym = L.fb_res;   // [items][162]
  fol_sym.resize((size_t)n * UWSPR_NSYM);
  if ((rc = lane_fetch(q, L, fol_sym.data(), d_sym, fol_sym.size()))) return rc;
  L.fol_ok.assign((size_t)n, 0);
  L.fol_msg.assign((size_t)n * 7, 0);
  std::atomic<long long> calls(0), fails(0);
  auto one = [&](int k) {
    uint8_t sym[UWSPR_NSYM], data[11];
    memcpy(sym, &fol_sym[(size_t)k * UWSPR_NSYM], UWSPR_NSYM);
    if (!rules::follow_gates(L.fol_fetch[k], sym)) return;
    uwspr_deinterleave(sym);
    memset(data, 0, sizeof(data));
    uint32_t metric, cycles, maxnp;
    calls.fetch_add(1, std::memory_order_relaxed);
    if (uwspr_fano_decode(sym, data, &metric, &cycles, &maxnp, 60, 10000) != 0) { fails.fetch_add(1, std::memory_order_relaxed); return; }
    int8_t msg[7];
    char text[32];
    for (int i = 0; i < 7; i++) msg[i] = (int8_t)data[i];
    if (uwspr_unpack_message(msg, text, sizeof(text)) != 0) return;
    L.fol_ok[k] = 1;
    memcpy(&L.fol_msg[7 * (size_t)k], msg, 7);
  };
  if (n <= 2) for (int k = 0; k < n; k++) one(k);
  else q->pool->run(n, q->o.host_threads, one);
  for (int k = 0; k < n; k++) {
    if (!L.fol_ok[k]) continue;
    const int i = L.fb_rec[k];
    L.dec[i] = 1; L.idt[i] = L.fb_idt[k]; L.osdf[i] = 4;
    memcpy(&L.msg[7 * (size_t)i], &L.fol_msg[7 * (size_t)k], 7);
    L.fol_by_rec[i] = L.fol_fetch[k];
  }
  ta.calls += calls.load(); ta.fails += fails.load();
  ta.resume_s += now_s() - t0;
  return UWSPR_OK;
}

// uwspr_pipe_set_tracks.  Behind the fallbacks every decoded record of the search -- Fano's, "block"'s, the list's, the call
// search's and OSD's alike -- becomes one K15 item: the symbols of its message, the jig_shift of the try that decoded and
// the frequency model the fine search correlated with (rules::fine_model: what the second pass subtracts with), over the
// frames the search itself read.  The fits go to L.trk_by_rec; no decode record changes.  Its time counts as resume time.
static int track_tail(uwspr_pipe *q, pipe_lane &L, const float *frames, int nrec, tail_acc &ta) {
  const int per = q->per;
  L.trk_items.clear(); L.trk_rec.clear();
  for (int i = 0; i < nrec; i++) {
    if (!lane_valid(q, L, i) || !L.dec[i]) continue;
    const uwspr_demod_out &o = L.h_out[i];
    uwspr_sub_item it;
    memset(&it, 0, sizeof(it));
    it.frame = i / per;
    it.shift = o.jig_shift[L.idt[i] >= 0 && L.idt[i] < UWSPR_NJIG ? L.idt[i] : 0];
    rules::fine_model(L.h_cands[i], o, (float)q->p.cf, &it.f_hz, &it.drift_hz);
    if (L.osdf[i] == 4) {   // K16 decoded it: at the follower's lag and frequency, without drift
      const fol_set *fs = q->follow_set;
      it.shift += 32 * (L.fol_by_rec[i].best % (2 * fs->nl + 1) - fs->nl);
      it.f_hz = L.fol_by_rec[i].f_hz; it.drift_hz = 0.0f;
    }
    if (uwspr_wspr_symbols(&L.msg[7 * (size_t)i], it.symbols)) return pfail(q, UWSPR_ERR_ARG, "trajectory fit: symbols of a decoded message");
    L.trk_items.push_back(it); L.trk_rec.push_back(i);
  }
  const int n = (int)L.trk_items.size();
  if (n == 0) return UWSPR_OK;
  const double t0 = now_s();
  uwspr_track_result *d_res = nullptr;
  int rc = subtract_check(L.ctx, L.trk_items.data(), n, (nrec + per - 1) / per);
  if (!rc) rc = track_run(L.ctx, q->track_set, frames, (size_t)L.ctx->fstride, L.trk_items.data(), n, nullptr, nullptr, &d_res);
  if (rc) return pfail(q, rc, "trajectory fit: %s", uwspr_last_error(L.ctx));
  L.trk_fetch.resize((size_t)n);
  if ((rc = lane_fetch(q, L, L.trk_fetch.data(), d_res, (size_t)n * sizeof(uwspr_track_result)))) return rc;
  for (int k = 0; k < n; k++) L.trk_by_rec[L.trk_rec[k]] = L.trk_fetch[k];
  ta.resume_s += now_s() - t0;
  return UWSPR_OK;
}

// The host tail of one search of B frames (the batch itself, first = true; or its second pass over the residual frames):
// waits for the lane's event, runs Fano on what the GPU produced, resumes what try 0 did not decode, then the fallbacks.
// Leaves L.dec / L.idt / L.msg / L.osdf / L.blkf for the B * per records of L.h_out.
static int host_tail(uwspr_pipe *q, pipe_lane &L, const float *frames, int B, bool first, tail_acc &ta) {
  const int per = q->per, nrec = B * per;
  double t0 = now_s();
  PHIP(q, hipEventSynchronize(L.ev_done));
  if (first && q->inject_where.load() == 1 && L.seq == q->inject_seq.load()) return pfail(q, UWSPR_ERR_HIP, "injected failure in the host tail of batch %lld", (long long)L.seq);
  double t1 = now_s();
  if (first) {
    std::lock_guard<std::mutex> lk(q->m);
    L.host_since = t1;   // the host tail of this batch starts: the producer may open a spare lane if it lasts (take_lane)
  }
  // cc:457-490 on what the first pass produced (try 0 alone in the lazy flow)
  std::atomic<long long> calls(0), fails(0);
  // only the records that are worth a try go to the pool (a quiet stream has almost none: no wake-ups for it)
  L.first.clear();
  for (int i = 0; i < nrec; i++) {
    L.dec[i] = 0; L.idt[i] = -1;
    memset(&L.msg[7 * (size_t)i], 0, 7);
    if (lane_valid(q, L, i) && L.h_out[i].worth_a_try) L.first.push_back(i);
  }
  auto first_pass = [&](int k) {
    const int i = L.first[k];
    int32_t idt = -1;
    int nc = 0;
    const int r = decode_candidate_from(&L.h_out[i], 0, &L.msg[7 * (size_t)i], &idt, &nc);
    if (nc) { calls.fetch_add(nc, std::memory_order_relaxed); fails.fetch_add(nc - r, std::memory_order_relaxed); }
    if (!r) memset(&L.msg[7 * (size_t)i], 0, 7);
    L.dec[i] = (uint8_t)r;
    L.idt[i] = idt;
  };
  if (L.first.size() <= 2) for (size_t k = 0; k < L.first.size(); k++) first_pass((int)k);
  else q->pool->run((int)L.first.size(), q->o.host_threads, first_pass);
  double t2 = now_s(), t3 = t2;
  L.redo.clear();
  if (!q->o.eager) {
    for (int i = 0; i < nrec; i++) {
      const bool need = lane_valid(q, L, i) && L.h_out[i].worth_a_try && !L.dec[i];
      L.h_need[i] = need ? 1 : 0;
      if (need) L.redo.push_back(i);
    }
  }
  if (!L.redo.empty()) {
    // the other 16 tries of those candidates, then Fano from try 1 on
    PHIP(q, hipMemcpyAsync(L.d_need, L.h_need, (size_t)nrec, hipMemcpyHostToDevice, L.stream));
    int rc = uwspr_demod_resume(L.ctx, frames, B, UWSPR_DEVICE, L.d_need, per, L.d_out);
    if (rc) return pfail(q, rc, "uwspr_demod_resume: %s", uwspr_last_error(L.ctx));
    if (L.redo.size() * 4 > (size_t)nrec) {
      PHIP(q, hipMemcpyAsync(L.h_out, L.d_out, (size_t)nrec * sizeof(uwspr_demod_out), hipMemcpyDeviceToHost, L.stream));
    } else {
      for (int i : L.redo)
        PHIP(q, hipMemcpyAsync(&L.h_out[i], &L.d_out[i], sizeof(uwspr_demod_out), hipMemcpyDeviceToHost, L.stream));
    }
    PHIP(q, hipEventRecord(L.ev_done, L.stream));
    PHIP(q, hipEventSynchronize(L.ev_done));
    t3 = now_s();
    // The reference walks a candidate's tries one after the other and stops at the first that decodes
    // (cc:457-490).  A try that does not decode runs Fano to its 10000-cycles-per-bit time-out (~4 ms of one
    // core), so a candidate nothing decodes would hold ONE thread for 16 time-outs while the pool idles.
    // The tries are independent decodes: all (candidate, try) pairs go to the pool at once and the first
    // try in the reference's order that decoded is the answer -- the same message and idt; the tries after
    // a decoding one are work the reference would not have done.
    L.tasks.clear();
    for (int i : L.redo)
      for (int idt = 1; idt < UWSPR_NJIG; idt++) L.tasks.push_back((i << 5) | idt);
    L.task_ok.assign(L.tasks.size(), 0);
    L.task_msg.resize(L.tasks.size() * 7);
    q->pool->run((int)L.tasks.size(), q->o.host_threads, [&](int t) {
      const int i = L.tasks[t] >> 5, idt = L.tasks[t] & 31;
      const int r = decode_try(&L.h_out[i], idt, &L.task_msg[7 * (size_t)t]);
      if (r >= 0) calls.fetch_add(1, std::memory_order_relaxed);
      if (r == 0) fails.fetch_add(1, std::memory_order_relaxed);
      L.task_ok[t] = (uint8_t)(r > 0);
    });
    for (size_t t = 0; t < L.tasks.size(); t++) {   // tasks are in (candidate, try) order
      const int i = L.tasks[t] >> 5, idt = L.tasks[t] & 31;
      if (L.task_ok[t] && !L.dec[i]) {
        L.dec[i] = 1; L.idt[i] = idt;
        memcpy(&L.msg[7 * (size_t)i], &L.task_msg[7 * t], 7);
      }
    }
  }
  double t4 = now_s();
  ta.calls += calls.load(); ta.fails += fails.load();   // (tries run after a decoding one count as calls)
  ta.resumed += (long long)L.redo.size();
  ta.gpu_wait_s += (t1 - t0);
  ta.fano_s += (t2 - t1) + (t4 - t3);
  ta.resume_s += (t3 - t2);
  // block -> follow -> list -> calls -> OSD (the blind methods first); a record one of them decoded is no item of the next
  memset(L.osdf.data(), 0, (size_t)nrec);
  memset(L.blkf.data(), 0, (size_t)nrec);
  if (q->block > 0)
    if (const int rc = block_tail(q, L, frames, nrec, ta)) return rc;
  if (q->follow_set)
    if (const int rc = follow_tail(q, L, frames, nrec, ta)) return rc;
  if (q->deep_M > 0)
    if (const int rc = scored_tail(q, L, nrec, kListFallback, ta)) return rc;
  if (q->call_set)
    if (const int rc = scored_tail(q, L, nrec, kCallFallback, ta)) return rc;
  if (q->osd > 0)
    if (const int rc = scored_tail(q, L, nrec, kOsdFallback, ta)) return rc;
  if (q->track_set) return track_tail(q, L, frames, nrec, ta);
  return UWSPR_OK;
}

// Record i of the lane's search as the pipe emits it: frame b of the batch, candidate number cand of that frame's npk.
static uwspr_decode make_record(const pipe_lane &L, int b, int i, int cand, int32_t npk, int pass) {
  uwspr_decode d;
  memset(&d, 0, sizeof(d));
  d.frame = L.frame0 + b;
  d.channel = (int16_t)L.channel;
  d.stream_pos = L.pos0 >= 0 ? L.pos0 + (int64_t)b * L.stride : -1;
  d.cand = cand; d.npk = npk;
  d.coarse = L.h_cands[i];   // [B][per], as h_out
  const uwspr_demod_out &o = L.h_out[i];
  d.f1 = o.f1; d.drift1 = o.drift1; d.sync1 = o.sync1; d.shift1 = o.shift1; d.worth_a_try = o.worth_a_try;
  d.decoded = L.dec[i]; d.idt = L.idt[i];
  memcpy(d.message, &L.msg[7 * (size_t)i], 7);
  d.pass = (uint8_t)pass;
  d.osd = L.osdf[i];
  d.block = L.blkf[i];
  return d;
}

static int second_pass(uwspr_pipe *q, pipe_lane &L, tail_acc &ta, int *ncand, int *ndec);

static int finish_batch(uwspr_pipe *q, pipe_lane &L) {
  const int per = q->per, B = L.B;
  L.recs.clear();   // (a failure below emits nothing for this batch)
  L.rec_trk.clear(); L.trecs.clear();
  L.rec_fol.clear(); L.frecs.clear();
  const bool tracks = q->track_set != nullptr, follows = q->follow_set != nullptr;
  tail_acc ta;
  if (const int rc = host_tail(q, L, L.frames, B, true, ta)) return rc;
  int ncand = 0, ndec = 0;
  for (int b = 0; b < B; b++)
    for (int j = 0; j < per; j++) {
      const int i = b * per + j;
      if (!lane_valid(q, L, i)) continue;
      L.recs.push_back(make_record(L, b, i, j, L.h_npk[b], 0));
      if (tracks) L.rec_trk.push_back(L.trk_by_rec[i]);
      if (follows) L.rec_fol.push_back(L.fol_by_rec[i]);
      ncand++; ndec += L.dec[i];
    }
  if (q->passes == 2 && ndec > 0) {
    const int rc = second_pass(q, L, ta, &ncand, &ndec);
    if (rc) { L.recs.clear(); L.rec_trk.clear(); L.rec_fol.clear(); return rc; }
  }
  if (follows)   // one follow record per record K16 decoded, in their order
    for (size_t r = 0; r < L.recs.size(); r++) {
      const uwspr_decode &d = L.recs[r];
      if (!d.decoded || d.osd != 4) continue;
      uwspr_follow_record fr;
      memset(&fr, 0, sizeof(fr));
      fr.frame = d.frame; fr.cand = d.cand; fr.channel = d.channel; fr.pass = d.pass; fr.result = L.rec_fol[r];
      L.frecs.push_back(fr);
    }
  if (tracks)   // one track record per decoded record, in their order
    for (size_t r = 0; r < L.recs.size(); r++) {
      const uwspr_decode &d = L.recs[r];
      if (!d.decoded) continue;
      uwspr_track_record tr;
      memset(&tr, 0, sizeof(tr));
      tr.frame = d.frame; tr.cand = d.cand; tr.channel = d.channel; tr.pass = d.pass; tr.result = L.rec_trk[r];
      L.trecs.push_back(tr);
    }
  {
    std::lock_guard<std::mutex> lk(q->m);
    q->st.frames += B; q->st.batches += 1; q->st.candidates += ncand; q->st.decoded += ndec;
    q->st.resumed += (int64_t)ta.resumed;
    q->st.fano_calls += ta.calls; q->st.fano_timeouts += ta.fails;
    q->st.gpu_wait_s += ta.gpu_wait_s;
    q->st.fano_s += ta.fano_s;
    q->st.resume_s += ta.resume_s;
  }
  return UWSPR_OK;
}

// Option "passes" = 2.  L.recs holds the batch's records; the frames with a decoded one go through K8 -- every decoded
// record an item: the symbols of its message, its f1, the shift of the try that decoded, its drift1, refined against
// the samples -- into the lane's own buffer (the ring is only read), and that buffer through FDR + schedule + Fano as the
// batch itself went.  What decodes there and is not one of its frame's first-pass messages becomes a record with
// pass = 1 behind the frame's first-pass records.
static int second_pass(uwspr_pipe *q, pipe_lane &L, tail_acc &ta, int *ncand, int *ndec) {
  const int per = q->per, B = L.B;
  L.slot_frame.clear(); L.items.clear(); L.extra.clear();
  for (int b = 0; b < B; b++)
    for (int j = 0; j < per; j++) {
      const int i = b * per + j;
      if (!lane_valid(q, L, i) || !L.dec[i]) continue;
      if (L.slot_frame.empty() || L.slot_frame.back() != b) L.slot_frame.push_back(b);
      const uwspr_demod_out &o = L.h_out[i];
      uwspr_sub_item it;
      memset(&it, 0, sizeof(it));
      it.frame = (int32_t)L.slot_frame.size() - 1;
      it.shift = o.jig_shift[L.idt[i] >= 0 && L.idt[i] < UWSPR_NJIG ? L.idt[i] : 0];
      rules::fine_model(L.h_cands[i], o, (float)q->p.cf, &it.f_hz, &it.drift_hz);
      if (uwspr_wspr_symbols(&L.msg[7 * (size_t)i], it.symbols)) return pfail(q, UWSPR_ERR_ARG, "second pass: symbols of a decoded message");
      L.items.push_back(it);
    }
  const int ns = (int)L.slot_frame.size();
  if (ns == 0) return UWSPR_OK;
  std::vector<int32_t> npk1(ns);
  for (int s = 0; s < ns; s++) npk1[s] = L.h_npk[L.slot_frame[s]];
  const size_t need = (size_t)ns * q->fl * 2;
  if (need > L.cap_res2) {
    PHIP(q, hipStreamSynchronize(L.stream));
    if (L.d_res2) { PHIP(q, hipFree(L.d_res2)); L.d_res2 = nullptr; L.cap_res2 = 0; }
    if (hipMalloc((void **)&L.d_res2, need * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return pfail(q, UWSPR_ERR_NOMEM, "second pass: %zu bytes for %d residual frames", need * sizeof(float), ns); }
    L.cap_res2 = need;
  }
  int rc = subtract_check(L.ctx, L.items.data(), (int)L.items.size(), ns);
  if (!rc) rc = subtract_run(L.ctx, L.frames, (size_t)L.stride, ns, L.slot_frame.data(), L.items.data(), (int)L.items.size(), 1, L.d_res2);
  if (rc) return pfail(q, rc, "second pass, subtraction: %s", uwspr_last_error(L.ctx));
  rc = uwspr_set_frame_stride(L.ctx, 0);
  if (!rc) rc = uwspr_set_tries(L.ctx, q->o.eager ? UWSPR_NJIG : 1);
  if (!rc) rc = uwspr_pipeline_batch(L.ctx, L.d_res2, ns, UWSPR_DEVICE, per, L.d_cands, L.d_npk, L.d_out);
  if (rc) return pfail(q, rc, "second pass, uwspr_pipeline_batch: %s", uwspr_last_error(L.ctx));
  if ((rc = fetch_first_pass(q, L, ns))) return rc;
  if ((rc = host_tail(q, L, L.d_res2, ns, false, ta))) return rc;
  // merge: the records of frame b, then what the second pass adds to it
  std::vector<uwspr_decode> merged;
  merged.reserve(L.recs.size() + (size_t)ns * per);
  const bool tracks = q->track_set != nullptr;   // then L.rec_trk goes through the same merge, beside the records
  const bool follows = q->follow_set != nullptr;   // and L.rec_fol likewise
  std::vector<uwspr_track_result> mtrk;
  std::vector<uwspr_follow_result> mfol;
  auto keep = [&](size_t r) {
    merged.push_back(L.recs[r]);
    if (tracks) mtrk.push_back(L.rec_trk[r]);
    if (follows) mfol.push_back(L.rec_fol[r]);
  };
  size_t r0 = 0;
  for (int s = 0; s < ns; s++) {
    const int64_t fr = L.frame0 + L.slot_frame[s];
    while (r0 < L.recs.size() && L.recs[r0].frame < fr) keep(r0++);
    const size_t first = r0, mfirst = merged.size();   // the frame's first record in L.recs / in merged
    while (r0 < L.recs.size() && L.recs[r0].frame == fr) keep(r0++);
    int cand = (int)(r0 - first);
    for (int j = 0; j < per; j++) {
      const int i = s * per + j;
      if (!lane_valid(q, L, i) || !L.dec[i]) continue;
      bool known = false;   // one of the frame's first-pass messages, or of the second-pass records already made for it
      for (size_t r = mfirst; r < merged.size() && !known; r++) known = merged[r].decoded && !memcmp(merged[r].message, &L.msg[7 * (size_t)i], 7);
      if (known) continue;
      merged.push_back(make_record(L, L.slot_frame[s], i, cand++, npk1[s], 1));
      if (tracks) mtrk.push_back(L.trk_by_rec[i]);
      if (follows) mfol.push_back(L.fol_by_rec[i]);
      (*ncand)++; (*ndec)++;
    }
  }
  while (r0 < L.recs.size()) keep(r0++);
  L.recs.swap(merged);
  if (tracks) L.rec_trk.swap(mtrk);
  if (follows) L.rec_fol.swap(mfol);
  return UWSPR_OK;
}

// A coordinator takes the oldest launched batch nobody has taken yet, finishes it and emits its records when the
// batches before it have been emitted.  ncoords threads run this loop (default: one per lane, so that the host
// tails of consecutive batches overlap).
static void coordinator(uwspr_pipe *q) {
  (void)hipSetDevice(q->device);
  for (;;) {
    pipe_lane *Lp = nullptr;
    {
      std::unique_lock<std::mutex> lk(q->m);
      q->cv_work.wait(lk, [&]() {
        Lp = nullptr;
        for (auto &L : q->lanes)
          if (L.launched && !L.claimed && (!Lp || L.seq < Lp->seq)) Lp = &L;
        return q->stop || Lp != nullptr;
      });
      if (!Lp) return;   // stop, nothing left to take
      Lp->claimed = true;
    }
    pipe_lane &L = *Lp;
    if (finish_batch(q, L)) { L.trecs.clear(); L.frecs.clear(); }   // a failure is sticky in q->failed; the lane is released either way
    {
      std::unique_lock<std::mutex> lk(q->m);
      q->cv_turn.wait(lk, [&]() { return q->emit_seq == L.seq; });
      for (const uwspr_track_record &t : L.trecs) q->done_trk.push_back(t);   // (no later than the decode records they belong to)
      for (const uwspr_follow_record &t : L.frecs) q->done_fol.push_back(t);
      for (const uwspr_decode &d : L.recs) q->done.push_back(d);
      q->emit_seq++;
      L.launched = false; L.claimed = false; L.host_since = 0.0;
      L.busy = false;
    }
    q->cv_turn.notify_all();
    q->cv_lane.notify_all();
    q->cv_done.notify_all();
  }
}

// ---- producer side --------------------------------------------------------------------------------
// The first kPipeStreams lanes (one per HIP stream) take the batches in turn: that is what a GPU-bound stream wants
// (more batches in flight only cost it cache and 6 % of its rate).  The lanes beyond them are SPARES for a stream whose
// host tail is the bottleneck -- Fano time-outs, 4 ms of a core each: a spare is opened only while every base lane is busy
// and one of them has been in its host tail (first GPU pass complete) for longer than kSpareAfter (2.5 ms).
constexpr double kSpareAfter = 2.5e-3;   // seconds (a Fano time-out is ~4 ms; the host tail of a batch that decodes at once ~0.3 ms)
// (uwspr_pipe_opts::spare_after_us: tests open the spares at once with 1)
static pipe_lane *take_lane(uwspr_pipe *q) {
  std::unique_lock<std::mutex> lk(q->m);
  const int n = (int)q->lanes.size(), base = n < kPipeStreams ? n : kPipeStreams;
  pipe_lane *pick = nullptr;
  for (;;) {
    for (int k = 0; k < base && !pick; k++) {
      const int idx = (q->next_lane + k) % base;
      if (!q->lanes[idx].busy) { pick = &q->lanes[idx]; q->next_lane = (idx + 1) % base; }
    }
    if (pick) break;
    if (n > base) {
      const double now = now_s();
      bool slow_tail = false;
      for (int k = 0; k < base; k++) slow_tail |= q->lanes[k].host_since > 0.0 && now - q->lanes[k].host_since > q->spare_after;
      if (slow_tail)
        for (int k = base; k < n && !pick; k++) if (!q->lanes[k].busy) pick = &q->lanes[k];
      if (pick) break;
      q->cv_lane.wait_for(lk, std::chrono::microseconds(500));   // (a host tail grows old without anybody notifying)
    } else {
      q->cv_lane.wait(lk);
    }
  }
  pick->busy = true;
  return pick;
}

static int launch(uwspr_pipe *q, pipe_lane &L, const float *frames, int B, int stride, int64_t pos0, int ringbuf,
                  int channel = 0) {
  const int per = q->per;
  L.B = B; L.stride = stride; L.frames = frames; L.pos0 = pos0; L.channel = channel; L.frame0 = q->next_frame[channel];
  q->next_frame[channel] += B;
  if (q->inject_where.load() == 0 && q->next_seq == q->inject_seq.load())
    return pfail(q, UWSPR_ERR_HIP, "injected failure at the launch of batch %lld", (long long)q->next_seq);
  int rc = uwspr_set_frame_stride(L.ctx, stride);
  if (!rc) rc = uwspr_set_tries(L.ctx, q->o.eager ? UWSPR_NJIG : 1);
  if (!rc) rc = uwspr_pipeline_batch(L.ctx, frames, B, UWSPR_DEVICE, per, L.d_cands, L.d_npk, L.d_out);
  if (rc) return pfail(q, rc, "uwspr_pipeline_batch: %s", uwspr_last_error(L.ctx));
  if ((rc = fetch_first_pass(q, L, B))) return rc;
  if (ringbuf >= 0) q->ring.reader_done(ringbuf, L.ev_done);
  {
    std::lock_guard<std::mutex> lk(q->m);
    L.seq = q->next_seq++;
    L.launched = true;
  }
  q->cv_work.notify_all();
  return UWSPR_OK;
}

static void release_lane(uwspr_pipe *q, pipe_lane &L) {   // a launch that failed before it was queued
  {
    std::lock_guard<std::mutex> lk(q->m);
    L.busy = false;
  }
  q->cv_lane.notify_all();
}

// k frames of every plane (channel c, carrier k: plane c * ncar + k; one carrier: the channels): one batch per plane, in
// plane order, each in place in its plane; the batch's `channel` is the plane index.  The view consumes
// the frames of all planes; the lanes of channels 1.. wait for the same uploads (nothing is appended in between: the
// producer thread is the only writer) and each lane's event joins the buffer's readers.
static int launch_from_ring(uwspr_pipe *q, int k) {
  stream_ring &r = q->ring;
  const float *frames = nullptr;
  long long pos = 0;
  int buf = 0;
  for (int c = 0; c < r.npl; c++) {
    pipe_lane *L = take_lane(q);
    if (c == 0 && !r.view(k, L->stream, &frames, &pos, &buf)) {
      release_lane(q, *L);
      return pfail(q, UWSPR_ERR_HIP, "stream view: %s", hipGetErrorString(r.err));
    }
    if (c > 0 && (r.err = hipStreamWaitEvent(L->stream, r.ev_up, 0)) != hipSuccess) {
      release_lane(q, *L);
      return pfail(q, UWSPR_ERR_HIP, "stream view: %s", hipGetErrorString(r.err));
    }
    const int rc = launch(q, *L, frames + 2 * (size_t)c * r.plane, k, r.hop, pos, buf, c);
    if (rc) { release_lane(q, *L); return rc; }
  }
  return UWSPR_OK;
}

extern "C" const char *uwspr_pipe_last_error(const uwspr_pipe *q) { return q ? q->err : "null pipe"; }

extern "C" void uwspr_pipe_close(uwspr_pipe *q) {
  if (!q) return;
  {
    std::lock_guard<std::mutex> lk(q->m);
    q->stop = true;
  }
  q->cv_work.notify_all();
  for (auto &t : q->coords) if (t.joinable()) t.join();
  (void)hipSetDevice(q->device);
  for (auto &L : q->lanes) if (L.stream) (void)hipStreamSynchronize(L.stream);
  for (auto &L : q->lanes)   // lanes beyond the stream count ran on another lane's stream: back to their own before any is destroyed
    if (L.ctx && L.stream != L.ctx->own_stream) { (void)uwspr_set_stream(L.ctx, nullptr); L.stream = L.ctx->own_stream; }
  for (auto &L : q->lanes) {
    void *dev[] = {L.d_cands, L.d_npk, L.d_out, L.d_need, L.d_res2};
    for (void *b : dev) if (b) (void)hipFree(b);
    void *host[] = {L.h_cands, L.h_npk, L.h_out, L.h_need};
    for (void *b : host) if (b) (void)hipHostFree(b);
    if (L.ev_done) (void)hipEventDestroy(L.ev_done);
    if (L.ctx) uwspr_ctx_destroy(L.ctx);
  }
  if (q->d_deep_tab) (void)hipFree(q->d_deep_tab);
  calls_free_set(q->call_set);
  track_free_set(q->track_set);
  follow_free_set(q->follow_set);
  q->ring.close();
  for (int k = 0; k < uwspr_pipe::NSTAGE; k++) {
    if (q->h_stage[k]) (void)hipHostFree(q->h_stage[k]);
    if (q->stage_ev[k]) (void)hipEventDestroy(q->stage_ev[k]);
  }
  if (q->own_pool) delete q->pool;
  delete q;
}

extern "C" int uwspr_pipe_open(const uwspr_params *p, int device, const uwspr_pipe_opts *o, uwspr_pipe **out) {
  if (!p || !o || !out) return UWSPR_ERR_ARG;
  *out = nullptr;
  uwspr_pipe *q = new (std::nothrow) uwspr_pipe();
  if (!q) return UWSPR_ERR_NOMEM;
  memset(q->err, 0, sizeof(q->err));
  memset(&q->st, 0, sizeof(q->st));
  q->p = *p; q->o = *o; q->device = device; q->fl = p->fl; q->maxfreqs = p->maxfreqs;
  *out = q;   // handed back even on failure so uwspr_pipe_last_error() can be read
  if (q->o.batch_frames <= 0) q->o.batch_frames = 256;
  if (q->o.max_per_frame <= 0) q->o.max_per_frame = 1;
  if (q->o.lanes <= 0) q->o.lanes = 9;   // three streams + six spares (take_lane)
  if (q->o.lanes > 12) q->o.lanes = 12;
  q->spare_after = q->o.spare_after_us > 0 ? 1e-6 * (double)q->o.spare_after_us : kSpareAfter;
  if (q->o.hop <= 0) q->o.hop = p->fl;
  if (q->o.hop > p->fl) return pfail(q, UWSPR_ERR_ARG, "hop=%d > fl=%d", q->o.hop, p->fl);
  q->per = q->o.max_per_frame < p->maxfreqs ? q->o.max_per_frame : p->maxfreqs;
  const int Bm = q->o.batch_frames, per = q->per;
  q->lanes.resize(q->o.lanes);
  for (auto &L : q->lanes) {
    const int rc = uwspr_ctx_create(p, device, &L.ctx);
    if (rc) return pfail(q, rc, "uwspr_ctx_create: %s", L.ctx ? uwspr_last_error(L.ctx) : uwspr_status_string(rc));
    L.stream = L.ctx->own_stream;
    // At most kPipeStreams HIP streams: lane k >= kPipeStreams launches on the stream of lane k % kPipeStreams (a
    // fourth stream shares a hardware queue with another and the GPU-bound rate drops: 4 / 6 lanes 734 / 833 k
    // against 861 k for 3, round-3 probe).  The extra lanes are batches in flight on the HOST side -- their own
    // buffers and coordinator -- which is what a stream with many Fano time-outs needs (busy stream: 39 k frames/s
    // with 3 lanes, 49 k with 6 on 3 streams).
    const int lane_idx = (int)(&L - &q->lanes[0]);
    if (lane_idx >= kPipeStreams) {
      const int rcs = uwspr_set_stream(L.ctx, q->lanes[lane_idx % kPipeStreams].ctx->own_stream);
      if (rcs) return pfail(q, rcs, "uwspr_set_stream: %s", uwspr_last_error(L.ctx));
      L.stream = q->lanes[lane_idx % kPipeStreams].ctx->own_stream;
    }
    // schedule form: with three or more batches in flight the staged launches leave room for the other
    // lanes' kernels and win (861 k against 773 k decoded frames/s at 3 lanes); alone or in pairs the fused
    // kernel does (tools/pipe_lanes_probe.py).  A "sched" option in UWSPR_OPTIONS still decides when set.
    if (q->o.sched_form == 1) (void)uwspr_set_option(L.ctx, "sched", 1);
    else if (q->o.sched_form == 2) (void)uwspr_set_option(L.ctx, "sched", 0);
    else if (!L.ctx->opt_set[UWSPR_OPT_SCHED]) (void)uwspr_set_option(L.ctx, "sched", q->o.lanes < kPipeStreams ? 1 : 0);
    PHIP(q, hipMalloc((void **)&L.d_cands, (size_t)Bm * p->maxfreqs * sizeof(uwspr_candidate)));
    PHIP(q, hipMalloc((void **)&L.d_npk, (size_t)Bm * sizeof(int32_t)));
    PHIP(q, hipMalloc((void **)&L.d_out, (size_t)Bm * per * sizeof(uwspr_demod_out)));
    PHIP(q, hipMalloc((void **)&L.d_need, (size_t)Bm * per));
    PHIP(q, hipHostMalloc((void **)&L.h_cands, (size_t)Bm * per * sizeof(uwspr_candidate), hipHostMallocDefault));
    PHIP(q, hipHostMalloc((void **)&L.h_npk, (size_t)Bm * sizeof(int32_t), hipHostMallocDefault));
    PHIP(q, hipHostMalloc((void **)&L.h_out, (size_t)Bm * per * sizeof(uwspr_demod_out), hipHostMallocDefault));
    PHIP(q, hipHostMalloc((void **)&L.h_need, (size_t)Bm * per, hipHostMallocDefault));
    // the coordinator sleeps on this event (it does not spin: the cores belong to the Fano pool)
    PHIP(q, hipEventCreateWithFlags(&L.ev_done, hipEventDisableTiming | hipEventBlockingSync));
    L.dec.resize((size_t)Bm * per); L.idt.resize((size_t)Bm * per); L.msg.resize((size_t)Bm * per * 7);
    L.osdf.resize((size_t)Bm * per);
    L.trk_by_rec.resize((size_t)Bm * per);
    L.blkf.resize((size_t)Bm * per);
  }
  // pushed streams: the device ring and the page-locked staging buffers are made by the first acquire (open_ingest):
  // a pipe that only takes device frames (uwspr_pipe_submit_device) never pays their 2 x 83 MB of HBM + 4 x 6.9 MB page-locked (hop 3375; 2.2 GB + 0.37 GB at hop 0 = the frame length)
  q->stage_samples = (size_t)Bm * q->o.hop;
  if (q->o.host_threads <= 0) q->o.host_threads = host_cpu_share() > 3 ? host_cpu_share() - 2 : 1;
  q->pool = &host_pool::shared();   // the process-wide pool; this pipe's jobs use host_threads of it
  const int ncoords = (int)q->lanes.size();
  for (int k = 0; k < ncoords; k++) q->coords.emplace_back(coordinator, q);
  return UWSPR_OK;
}

// the device ring and the page-locked staging buffers.  Per channel plane: ceil(lanes / nch) + 3 takes of slack (at
// most `lanes` batches are in flight, nch per take) + fl.  A ring nothing was pushed into yet takes the channel count
// of the first push (a pipe's stream kind and channel count are latched by its first push).
// With ncar carriers (audio pushes only) the planes are nch * ncar, and that product takes nch's place in the formula.
static int open_ingest(uwspr_pipe *q, int nch, int ncar = 1) {
  stream_ring &r = q->ring;
  if (r.is_open() && ((r.nch == nch && r.ncar == ncar) || r.kind != RING_EMPTY)) return UWSPR_OK;
  const bool staged = r.is_open();
  const int npl = nch * ncar;
  const int takes = (q->o.lanes + npl - 1) / npl + 3;
  if (!r.open(q->fl, q->o.hop, q->o.batch_frames, takes, nch, ncar))
    return pfail(q, UWSPR_ERR_NOMEM, "stream ring (%d channel planes of %lld pairs, 2 buffers): %s", npl,
                 (long long)takes * q->o.batch_frames * q->o.hop + q->fl, hipGetErrorString(r.err));
  if (staged) return UWSPR_OK;
  for (int k = 0; k < uwspr_pipe::NSTAGE; k++) {
    PHIP(q, hipHostMalloc((void **)&q->h_stage[k], q->stage_samples * 2 * sizeof(float), hipHostMallocDefault));
    PHIP(q, hipEventCreateWithFlags(&q->stage_ev[k], hipEventDisableTiming));
  }
  return UWSPR_OK;
}

extern "C" int uwspr_pipe_inject_failure(uwspr_pipe *q, long long batch, int where) {
  if (!q || where < 0 || where > 1) return UWSPR_ERR_ARG;
  q->inject_where.store(where); q->inject_seq.store(batch);
  return UWSPR_OK;
}

extern "C" int uwspr_pipe_acquire(uwspr_pipe *q, int nsamples, float **iq) {
  if (!q || !iq) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (nsamples <= 0 || (size_t)nsamples > q->stage_samples)
    return parg(q, "uwspr_pipe_acquire(%d): at most %zu samples per piece", nsamples, q->stage_samples);
  (void)hipSetDevice(q->device);
  if (const int rc = open_ingest(q, 1)) return rc;
  const int s = q->stage_next;
  if (q->stage_busy[s]) { PHIP(q, hipEventSynchronize(q->stage_ev[s])); q->stage_busy[s] = false; }
  q->stage_cur = s;
  *iq = q->h_stage[s];
  return UWSPR_OK;
}

extern "C" int uwspr_pipe_commit(uwspr_pipe *q, int nsamples) {
  if (!q) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (q->stage_cur < 0 || nsamples < 0 || (size_t)nsamples > q->stage_samples)
    return parg(q, "uwspr_pipe_commit(%d) without a matching uwspr_pipe_acquire", nsamples);
  (void)hipSetDevice(q->device);
  const int s = q->stage_cur;
  q->stage_cur = -1;
  if (nsamples > 0 && q->ring.kind == RING_AUDIO) return parg(q, "uwspr_pipe_commit: the pipe's stream is audio");
  if (nsamples > 0) {
    q->ring.kind = RING_IQ;
    // room behind the unconsumed samples: launch what is complete first if the ring is full
    while (q->ring.have + (size_t)nsamples > q->ring.cap && q->ring.ready() > 0) {
      const int rc = launch_from_ring(q, q->ring.ready() < q->o.batch_frames ? q->ring.ready() : q->o.batch_frames);
      if (rc) return rc;
    }
    if (!q->ring.append(q->h_stage[s], (size_t)nsamples, false))
      return pfail(q, UWSPR_ERR_HIP, "stream upload: %s", hipGetErrorString(q->ring.err));
    PHIP(q, hipEventRecord(q->stage_ev[s], q->ring.copy));
    q->stage_busy[s] = true;
    q->stage_next = (s + 1) % uwspr_pipe::NSTAGE;
  }
  while (q->ring.ready() >= q->o.batch_frames) {
    const int rc = launch_from_ring(q, q->o.batch_frames);
    if (rc) return rc;
  }
  return UWSPR_OK;
}

extern "C" int uwspr_pipe_push(uwspr_pipe *q, const float *iq, int nsamples) {
  if (!q || (nsamples > 0 && !iq) || nsamples < 0) return UWSPR_ERR_ARG;
  size_t off = 0;
  while (off < (size_t)nsamples) {
    const size_t n = (size_t)nsamples - off < q->stage_samples ? (size_t)nsamples - off : q->stage_samples;
    float *dst = nullptr;
    int rc = uwspr_pipe_acquire(q, (int)n, &dst);
    if (rc) return rc;
    memcpy(dst, iq + 2 * off, n * 2 * sizeof(float));
    if ((rc = uwspr_pipe_commit(q, (int)n))) return rc;
    off += n;
  }
  return UWSPR_OK;
}

// Audio through the same page-locked staging (its bytes: batch_frames * hop (I,Q) pairs per buffer), then K0 on the
// copy stream into the ring (stream_ring::chain_push); batches are launched from the ring as uwspr_pipe_commit does,
// one per channel.  One channel is the same call with nchannels = 1.
extern "C" int uwspr_pipe_push_audio_channels(uwspr_pipe *q, const void *audio, int nframes, int nchannels, int format) {
  if (!q || (nframes > 0 && !audio) || nframes < 0) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (nchannels < 1 || nchannels > UWSPR_PIPE_MAX_CHANNELS)
    return parg(q, "uwspr_pipe_push_audio_channels: nchannels %d (1..%d)", nchannels, UWSPR_PIPE_MAX_CHANNELS);
  if (format != UWSPR_AUDIO_F32 && format != UWSPR_AUDIO_S16) return parg(q, "uwspr_pipe_push_audio: format %d", format);
  if (q->p.fs != 375) return parg(q, "uwspr_pipe_push_audio: the front-end is 12000 -> 375 S/s (fs=%d)", q->p.fs);
  if (nframes == 0) return UWSPR_OK;
  stream_ring &r = q->ring;
  if (r.kind == RING_IQ) return parg(q, "uwspr_pipe_push_audio: the pipe's stream is (I,Q)");
  if (r.kind == RING_AUDIO && nchannels != r.nch)
    return parg(q, "uwspr_pipe_push_audio_channels: %d channels into a stream of %d", nchannels, r.nch);
  const bool s16 = format == UWSPR_AUDIO_S16;
  // the front-end mode, the carriers and "frontend_hbw" (nchannels * carriers planes in all), "audio_rate", "blank" /
  // "blank_guard": latched by the stream's first push
  const audio_chain_cfg cfg = {q->lanes[0].ctx->opt[UWSPR_OPT_FRONTEND], q->carriers, q->frontend_hbw, q->audio_rate, q->blank, q->blank_guard};
  const chain_part changed = r.chain_mismatch(cfg);
  char why[160];
  if (changed == CHAIN_FRONTEND) return parg(q, "uwspr_pipe_push_audio: %s", chain_refusal(changed, cfg, r.chain_latched(), why));
  const int ncar = (int)cfg.carriers.size();
  if ((long long)nchannels * ncar > UWSPR_PIPE_MAX_CHANNELS)
    return parg(q, "uwspr_pipe_push_audio_channels: %d channels x %d carriers (at most %d planes)", nchannels, ncar, UWSPR_PIPE_MAX_CHANNELS);
  for (int fc : cfg.carriers)
    if (!frontend_carrier_ok(cfg.mode, fc, cfg.hbw))
      return parg(q, "uwspr_pipe_push_audio: carrier %d Hz with half-bandwidth %d Hz (hb + 20 <= carrier <= 6000 - hb - 20)", fc, cfg.hbw);
  if (changed) return parg(q, "uwspr_pipe_push_audio: %s", chain_refusal(changed, cfg, r.chain_latched(), why));
  (void)hipSetDevice(q->device);
  if (const int rc = open_ingest(q, nchannels, ncar)) return rc;
  if (const chain_part f = r.chain_latch(cfg, s16))
    return pfail(q, r.err == hipErrorOutOfMemory ? UWSPR_ERR_NOMEM : UWSPR_ERR_HIP, "%s set-up (%d S/s, %d channels): %s", chain_part_name(f),
                 cfg.rate, nchannels, hipGetErrorString(r.err));
  const size_t es = (s16 ? 2 : 4) * (size_t)nchannels;   // bytes per frame
  size_t piece = q->stage_samples * 2 * sizeof(float) / es;
  // several channels straight into K0: whole K0 workgroups per piece (32 * 512 frames), so a launch has no ragged last
  // output block
  constexpr size_t kBlockFrames = 32 * 512;
  if (cfg.rate == 12000 && !cfg.blank && nchannels > 1 && piece >= kBlockFrames) piece = piece / kBlockFrames * kBlockFrames;
  // a rate below 12000 makes more 12 kS/s samples than it is given: a piece yields no more of them than a 12 kS/s piece
  int L = 1, M = 1;
  r.chain_ratio(&L, &M);
  if (L > M) piece = piece * (size_t)M / (size_t)L;
  if (piece < 1) piece = 1;
  for (size_t off = 0; off < (size_t)nframes;) {
    const size_t n = (size_t)nframes - off < piece ? (size_t)nframes - off : piece;
    const int s = q->stage_next;
    if (q->stage_busy[s]) { PHIP(q, hipEventSynchronize(q->stage_ev[s])); q->stage_busy[s] = false; }
    memcpy(q->h_stage[s], (const char *)audio + off * es, n * es);
    const size_t nout = (size_t)r.chain_outputs(n, cfg);
    while (r.have + nout > r.cap && r.ready() > 0) {
      const int rc = launch_from_ring(q, r.ready() < q->o.batch_frames ? r.ready() : q->o.batch_frames);
      if (rc) return rc;
    }
    if (!r.chain_push(q->h_stage[s], n, s16, false)) return pfail(q, UWSPR_ERR_HIP, "audio stream: %s", hipGetErrorString(r.err));
    PHIP(q, hipEventRecord(q->stage_ev[s], r.copy));
    q->stage_busy[s] = true;
    q->stage_next = (s + 1) % uwspr_pipe::NSTAGE;
    while (r.ready() >= q->o.batch_frames) {
      const int rc = launch_from_ring(q, q->o.batch_frames);
      if (rc) return rc;
    }
    off += n;
  }
  return UWSPR_OK;
}

extern "C" int uwspr_pipe_push_audio(uwspr_pipe *q, const void *audio, int nsamples, int format) {
  return uwspr_pipe_push_audio_channels(q, audio, nsamples, 1, format);
}

extern "C" int uwspr_pipe_submit_device(uwspr_pipe *q, const float *dev_frames, int B, int stride) {
  if (!q || !dev_frames) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (B <= 0 || B > q->o.batch_frames || stride < 0)
    return parg(q, "uwspr_pipe_submit_device: B=%d (1..%d) stride=%d", B, q->o.batch_frames, stride);
  (void)hipSetDevice(q->device);
  pipe_lane *L = take_lane(q);
  const int rc = launch(q, *L, dev_frames, B, stride > 0 ? stride : q->fl, -1, -1);
  if (rc) release_lane(q, *L);
  return rc;
}

// K0's carriers: n distinct centres in Hz, in plane order (plane = channel * n + k).  Only before the first audio push;
// nchannels * n <= UWSPR_PIPE_MAX_CHANNELS and the range against "frontend_hbw" are checked by the push that latches them.
extern "C" int uwspr_pipe_set_carriers(uwspr_pipe *q, const int *hz, int n) {
  if (!q) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (!hz || n < 1 || n > UWSPR_PIPE_MAX_CHANNELS) return parg(q, "uwspr_pipe_set_carriers: hz / n %d (1..%d)", n, UWSPR_PIPE_MAX_CHANNELS);
  for (int i = 0; i < n; i++) {
    if (hz[i] < 21 || hz[i] > 5979) return parg(q, "uwspr_pipe_set_carriers: carrier %d Hz (21 .. 5979)", hz[i]);
    for (int j = 0; j < i; j++)
      if (hz[j] == hz[i]) return parg(q, "uwspr_pipe_set_carriers: carrier %d Hz twice", hz[i]);
  }
  if (q->ring.kind == RING_AUDIO) return parg(q, "uwspr_pipe_set_carriers: the audio stream runs (carriers are latched by its first push)");
  q->carriers.assign(hz, hz + n);
  return UWSPR_OK;
}

// What the pipe's lanes read may change only while no batch is in flight.  Called with q->m held -- a lane is marked busy
// under the same lock when a batch is launched on it, so none starts between this check and the change that follows it (the
// producer is single-threaded by contract, the coordinators are not).  false: the refusal is in q->err, in the name of
// what = the call, or call(option).
static bool lanes_idle_locked(uwspr_pipe *q, const char *call, const char *option = nullptr) {
  for (auto &L : q->lanes)
    if (L.busy) {
      snprintf(q->err, sizeof(q->err), option ? "%s(%s): batches in flight (flush first)" : "%s%s: batches in flight (flush first)", call, option ? option : "");
      return false;
    }
  return true;
}

// The pipe's own integer options that its host tails read: allowed values, how the refusal says so, where the value goes.
struct pipe_int_option { const char *name; bool (*ok)(int); const char *rule; int uwspr_pipe::*target; };
static const pipe_int_option kPipeIntOptions[] = {
    {"passes", [](int v) { return v == 1 || v == 2; }, "is 1 or 2", &uwspr_pipe::passes},   // 2 = subtract what decoded and search the residual
    {"osd", [](int v) { return v >= 0 && v <= 2; }, "is 0, 1 or 2", &uwspr_pipe::osd},      // K9 on the records Fano gave up on
    {"osd_gap", [](int v) { return v >= 0; }, "is >= 0", &uwspr_pipe::osd_gap},
    {"deep_min", [](int v) { return v >= 0; }, "is >= 0", &uwspr_pipe::deep_min},           // the list search's acceptance thresholds
    {"deep_gap", [](int v) { return v >= 0; }, "is >= 0", &uwspr_pipe::deep_gap},
    {"call_min", [](int v) { return v >= 0; }, "is >= 0", &uwspr_pipe::call_min},           // the call search's acceptance thresholds
    {"call_gap", [](int v) { return v >= 0; }, "is >= 0", &uwspr_pipe::call_gap},
    {"block", [](int v) { return v == 0 || v == 2 || v == 3; }, "is 0, 2 or 3", &uwspr_pipe::block},   // K10's block soft symbols for those records
};

// An option of the pipe (the table above; the audio chain's, latched by the first push) or of every lane's context
// (uwspr_set_option).  The latter and the table's only while nothing is in flight -- the lanes read their options when they
// launch -- and not "sched": the pipe picks the schedule form by its lane count (opts.sched_form).
extern "C" int uwspr_pipe_set_option(uwspr_pipe *q, const char *name, int value) {
  if (!q || !name) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  if (!strcmp(name, "sched")) return parg(q, "uwspr_pipe_set_option: \"sched\" belongs to uwspr_pipe_opts.sched_form");
  for (const pipe_int_option &po : kPipeIntOptions) {
    if (strcmp(name, po.name)) continue;
    if (!po.ok(value)) return parg(q, "uwspr_pipe_set_option: \"%s\" %s, not %d", name, po.rule, value);
    std::lock_guard<std::mutex> lk(q->m);
    if (!lanes_idle_locked(q, "uwspr_pipe_set_option", name)) return UWSPR_ERR_ARG;
    q->*po.target = value;
    return UWSPR_OK;
  }
  if (!strcmp(name, "audio_rate")) {   // the pipe's own: the rate of the audio its pushes carry, latched by the first push
    resample_plan pl;
    if (resample_design(value, pl)) return parg(q, "uwspr_pipe_set_option: \"audio_rate\" = %d is not a supported rate", value);
    if (const int running = q->ring.chain_running_rate(); running && value != running)
      return parg(q, "uwspr_pipe_set_option: \"audio_rate\" = %d while the audio stream runs at %d S/s", value, running);
    q->audio_rate = value;
    return UWSPR_OK;
  }
  if (!strcmp(name, "carrier")) return uwspr_pipe_set_carriers(q, &value, 1);
  if (!strcmp(name, "frontend_hbw")) {   // the pipe's own: K0's half-bandwidth, latched by the first audio push
    if (value < 1 || value > 150) return parg(q, "uwspr_pipe_set_option: \"frontend_hbw\" is 1 .. 150 Hz, not %d", value);
    if (const audio_chain_cfg has = q->ring.chain_latched(); has.rate && value != has.hbw)
      return parg(q, "uwspr_pipe_set_option: \"frontend_hbw\" = %d while the audio stream runs with %d Hz", value, has.hbw);
    q->frontend_hbw = value;
    return UWSPR_OK;
  }
  if (!strcmp(name, "blank") || !strcmp(name, "blank_guard")) {   // the pipe's own: K12 ahead of K11 / K0, latched by the first push
    const bool g = name[5] != 0;
    if (g ? (value < 0 || value > 64) : (value != 0 && (value < 4 || value > 1024)))
      return parg(q, g ? "uwspr_pipe_set_option: \"blank_guard\" is 0 .. 64, not %d" : "uwspr_pipe_set_option: \"blank\" is 0 or 4 .. 1024, not %d", value);
    audio_chain_cfg has = q->ring.chain_latched(), now = has;   // (what the running stream has, but for this option)
    (g ? now.guard : now.blank) = value;
    if (q->ring.chain_mismatch(now))
      return parg(q, "uwspr_pipe_set_option: \"%s\" = %d while the audio stream runs with blank %d, guard %d", name, value,
                  has.blank, has.guard);
    (g ? q->blank_guard : q->blank) = value;
    return UWSPR_OK;
  }
  // checked AND applied under q->m (lanes_idle_locked)
  std::lock_guard<std::mutex> lk(q->m);
  if (!lanes_idle_locked(q, "uwspr_pipe_set_option", name)) return UWSPR_ERR_ARG;
  for (auto &L : q->lanes) {
    const int rc = uwspr_set_option(L.ctx, name, value);
    if (rc) {
      if (!q->failed.load()) snprintf(q->err, sizeof(q->err), "uwspr_pipe_set_option(%s, %d): %s", name, value, uwspr_last_error(L.ctx));
      return UWSPR_ERR_ARG;
    }
  }
  return UWSPR_OK;
}

// The list of expected messages: checked, its table built on the host and uploaded before anything of the pipe changes;
// one table for all lanes (the lanes' contexts live on the pipe's device and only read it).
extern "C" int uwspr_pipe_set_list(uwspr_pipe *q, const int8_t *messages7, int M) {
  if (!q) return UWSPR_ERR_ARG;
  if (M != 0) {
    char why[160];
    if (deep_check_list(messages7, M, why, sizeof(why))) return parg(q, "uwspr_pipe_set_list: %s", why);
  }
  if (const int f = q->failed.load()) return f;
  int8_t *d_new = nullptr;
  if (M > 0) {
    std::vector<int8_t> tab;
    if (deep_build_table(messages7, M, tab)) return parg(q, "uwspr_pipe_set_list: symbols of a message");
    (void)hipSetDevice(q->device);
    if (hipMalloc((void **)&d_new, tab.size()) != hipSuccess) { (void)hipGetLastError(); return pfail(q, UWSPR_ERR_NOMEM, "uwspr_pipe_set_list: %zu bytes for the table", tab.size()); }
    const hipError_t e = hipMemcpy(d_new, tab.data(), tab.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_new); return pfail(q, UWSPR_ERR_HIP, "uwspr_pipe_set_list: upload of the table: %s", hipGetErrorString(e)); }
  }
  std::lock_guard<std::mutex> lk(q->m);
  if (!lanes_idle_locked(q, "uwspr_pipe_set_list")) {
    if (d_new) (void)hipFree(d_new);
    return UWSPR_ERR_ARG;
  }
  if (q->d_deep_tab) (void)hipFree(q->d_deep_tab);   // (nothing in flight: no lane reads it)
  q->d_deep_tab = d_new;
  q->deep_M = M;
  if (M > 0) q->deep_msgs.assign(messages7, messages7 + 7 * (size_t)M);
  else std::vector<int8_t>().swap(q->deep_msgs);
  return UWSPR_OK;
}

// The call set: checked, built on the host and uploaded before anything of the pipe changes; one set for all lanes (the
// lanes' contexts live on the pipe's device and only read it).
extern "C" int uwspr_pipe_set_calls(uwspr_pipe *q, const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask) {
  if (!q) return UWSPR_ERR_ARG;
  char why[200];
  if (A != 0 && calls_check(calls, A, grid_bitmap, power_mask, nullptr, why, sizeof(why))) return parg(q, "uwspr_pipe_set_calls: %s", why);
  if (const int f = q->failed.load()) return f;
  calls_set *fresh = nullptr;
  if (A > 0) {
    (void)hipSetDevice(q->device);
    int rc = UWSPR_OK;
    fresh = calls_build(calls, A, grid_bitmap, power_mask, &rc, why, sizeof(why));
    if (!fresh) return rc == UWSPR_ERR_ARG ? parg(q, "uwspr_pipe_set_calls: %s", why) : pfail(q, rc, "uwspr_pipe_set_calls: %s", why);
  }
  std::lock_guard<std::mutex> lk(q->m);
  if (!lanes_idle_locked(q, "uwspr_pipe_set_calls")) {
    calls_free_set(fresh);
    return UWSPR_ERR_ARG;
  }
  calls_free_set(q->call_set);   // (nothing in flight: no lane reads it)
  q->call_set = fresh;
  return UWSPR_OK;
}

// The trajectory set: checked, designed on the host and uploaded before anything of the pipe changes; one set for all lanes
// (the lanes' contexts live on the pipe's device and only read it).  n = 0 clears it.
extern "C" int uwspr_pipe_set_tracks(uwspr_pipe *q, const uwspr_track_traj *traj, int n, int qf, int model) {
  if (!q) return UWSPR_ERR_ARG;
  char why[256];
  if (n != 0 && track_check(traj, n, UWSPR_TRACK_MAX, qf, model, why, sizeof(why))) return parg(q, "uwspr_pipe_set_tracks: %s", why);
  if (const int f = q->failed.load()) return f;
  trk_set *fresh = nullptr;
  if (n > 0) {
    (void)hipSetDevice(q->device);
    int rc = UWSPR_OK;
    fresh = track_build(traj, n, qf, model, (double)q->p.cf, &rc, why, sizeof(why));
    if (!fresh) return rc == UWSPR_ERR_ARG ? parg(q, "uwspr_pipe_set_tracks: %s", why) : pfail(q, rc, "uwspr_pipe_set_tracks: %s", why);
  }
  std::lock_guard<std::mutex> lk(q->m);
  if (!lanes_idle_locked(q, "uwspr_pipe_set_tracks")) {
    track_free_set(fresh);
    return UWSPR_ERR_ARG;
  }
  track_free_set(q->track_set);   // (nothing in flight: no lane reads it)
  q->track_set = fresh;
  return UWSPR_OK;
}

// The follow set: K15's rules (checked, designed on the host and uploaded before anything of the pipe changes; one set for
// all lanes).  n = 0 clears it.
extern "C" int uwspr_pipe_set_follow(uwspr_pipe *q, const uwspr_track_traj *traj, int n, int qf, int nl, int model) {
  if (!q) return UWSPR_ERR_ARG;
  char why[256];
  if (n != 0 && follow_check(traj, n, qf, nl, model, why, sizeof(why))) return parg(q, "uwspr_pipe_set_follow: %s", why);
  if (n == 0 && (qf < 0 || qf > UWSPR_FOLLOW_QF_MAX || nl < 0 || nl > UWSPR_FOLLOW_NL_MAX || (model != UWSPR_TX_DOPPLER && model != UWSPR_TX_DELAY)))
    return parg(q, "uwspr_pipe_set_follow: n 0 clears the set, but qf %d (0..%d), nl %d (0..%d), model %d are no set's", qf, UWSPR_FOLLOW_QF_MAX, nl,
                UWSPR_FOLLOW_NL_MAX, model);
  if (const int f = q->failed.load()) return f;
  fol_set *fresh = nullptr;
  if (n > 0) {
    (void)hipSetDevice(q->device);
    int rc = UWSPR_OK;
    fresh = follow_build(traj, n, qf, nl, model, (double)q->p.cf, &rc, why, sizeof(why));
    if (!fresh) return rc == UWSPR_ERR_ARG ? parg(q, "uwspr_pipe_set_follow: %s", why) : pfail(q, rc, "uwspr_pipe_set_follow: %s", why);
  }
  std::lock_guard<std::mutex> lk(q->m);
  if (!lanes_idle_locked(q, "uwspr_pipe_set_follow")) {
    follow_free_set(fresh);
    return UWSPR_ERR_ARG;
  }
  if (fresh)   // (the per-record fits exist only in a pipe that follows)
    for (pipe_lane &L : q->lanes) L.fol_by_rec.resize(L.dec.size());
  follow_free_set(q->follow_set);   // (nothing in flight: no lane reads it)
  q->follow_set = fresh;
  return UWSPR_OK;
}

// the follow records emitted so far, at most cap of them; never waits
extern "C" int uwspr_pipe_collect_follows(uwspr_pipe *q, uwspr_follow_record *out, int cap) {
  if (!q || (cap > 0 && !out) || cap < 0) return UWSPR_ERR_ARG;
  std::lock_guard<std::mutex> lk(q->m);
  if (q->failed.load() && q->done_fol.empty()) return q->failed.load();
  int n = 0;
  while (n < cap && !q->done_fol.empty()) { out[n++] = q->done_fol.front(); q->done_fol.pop_front(); }
  return n;
}

// the track records emitted so far, at most cap of them; never waits
extern "C" int uwspr_pipe_collect_tracks(uwspr_pipe *q, uwspr_track_record *out, int cap) {
  if (!q || (cap > 0 && !out) || cap < 0) return UWSPR_ERR_ARG;
  std::lock_guard<std::mutex> lk(q->m);
  if (q->failed.load() && q->done_trk.empty()) return q->failed.load();
  int n = 0;
  while (n < cap && !q->done_trk.empty()) { out[n++] = q->done_trk.front(); q->done_trk.pop_front(); }
  return n;
}

extern "C" int uwspr_pipe_flush(uwspr_pipe *q) {
  if (!q) return UWSPR_ERR_ARG;
  (void)hipSetDevice(q->device);
  while (!q->failed.load() && q->ring.is_open() && q->ring.ready() > 0) {
    const int k = q->ring.ready() < q->o.batch_frames ? q->ring.ready() : q->o.batch_frames;
    const int rc = launch_from_ring(q, k);
    if (rc) return rc;
  }
  std::unique_lock<std::mutex> lk(q->m);
  q->cv_done.wait(lk, [&]() {
    for (auto &L : q->lanes) if (L.busy) return false;
    return true;
  });
  return q->failed.load();
}

extern "C" int uwspr_pipe_collect(uwspr_pipe *q, uwspr_decode *out, int cap, int wait) {
  if (!q || (cap > 0 && !out) || cap < 0) return UWSPR_ERR_ARG;
  std::unique_lock<std::mutex> lk(q->m);
  if (wait)
    q->cv_done.wait(lk, [&]() {
      if (!q->done.empty() || q->failed.load()) return true;
      for (auto &L : q->lanes) if (L.busy) return false;
      return true;
    });
  if (q->failed.load() && q->done.empty()) return q->failed.load();
  int n = 0;
  while (n < cap && !q->done.empty()) { out[n++] = q->done.front(); q->done.pop_front(); }
  return n;
}

extern "C" int uwspr_pipe_blank_stats(uwspr_pipe *q, long long *samples, long long *zeroed, int cap) {
  if (!q) return UWSPR_ERR_ARG;
  if (const int f = q->failed.load()) return f;
  (void)hipSetDevice(q->device);
  const int rc = ring_blank_stats(q->ring, samples, zeroed, cap);
  if (rc == UWSPR_ERR_ARG) return parg(q, "uwspr_pipe_blank_stats: samples/zeroed/cap %d", cap);
  if (rc < 0) return pfail(q, rc, "uwspr_pipe_blank_stats: %s", hipGetErrorString(q->ring.err));
  return rc;
}

extern "C" int uwspr_pipe_get_stats(uwspr_pipe *q, uwspr_pipe_stats *st) {
  if (!q || !st) return UWSPR_ERR_ARG;
  std::lock_guard<std::mutex> lk(q->m);
  *st = q->st;
  return UWSPR_OK;
}
