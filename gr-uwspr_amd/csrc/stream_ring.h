// stream_ring.h -- the tail of a 375 S/s (I,Q) stream kept in device memory so that the overlapping
// frames sliding_window_stream_to_pdu cuts from it (lib/sliding_window_stream_to_pdu_impl.cc:113-135:
// frame k = samples [k hop, k hop + fl)) can be read IN PLACE: frame k of a take starts at
// view + 2 * hop * k floats, nothing is cut or copied per frame, and a take's unique samples
// ((B-1) hop + fl of them) are what the kernels' working set is.
//
// Uploads run on the ring's own copy stream, so they overlap the search kernels of the batches before:
//   producer:  append()  H2D on the copy stream (page-locked source: one DMA; pageable: staged through
//                        two page-locked halves), ev_up recorded behind it
//   consumer:  view()    makes its stream wait for ev_up, returns the in-place pointer, consumes k hop
//                        samples; reader_done() tells the ring when the kernels reading a view have
//                        been enqueued (an event on the consumer's stream)
// Memory: two linear buffers of `cap` samples.  Appends go behind the unconsumed samples; when the
// current buffer is full the unconsumed tail (< fl + a take) moves to the front of the other buffer
// (rare: cap is several takes) after every reader of THAT buffer has finished.
//
// Channel planes (uwspr_pipe_push_audio_channels): a buffer holds nch planes of `plane` pairs each, one stream per
// channel.  The channels advance in lockstep, so the bookkeeping (base, have, pos, cur, the events) is shared:
// reserve / view return plane 0 and channel c is at + 2 * c * plane floats; the tail move is one 2-D copy of all
// planes.  The audio history is one interleaved [time][nch] buffer.
//
// Carriers (uwspr_pipe_set_carriers, option "carrier"): NC carriers listen to every audio channel, so the ring holds
// npl = nch * ncar planes, plane c * ncar + k for channel c and carrier k.  nch stays the AUDIO channel count (the
// interleave stride of the histories; what K11 and K12 see); npl is what the ring, reserve / view, the tail move and the
// batches see.  With one carrier npl == nch.
//
// Audio (chain_push): real samples go through a chain of stages on the copy stream into the ring -- K12, the blanker
// (option "blank" != 0), K11, the resampler (option "audio_rate" != 12000), and K0, the front-end, always.  What the
// chain is made of is latched by the first audio push after open / reset (chain_latch) and a stage hands its outputs
// to the next as a device source.  Every stage keeps its input in a staged_input: two device buffers, the current one
// holding [history | new frames], the history being the inputs the stage's next output still reads.  Which output a
// piece completes, from where the history is kept and how large the buffers are is stream_stage.h's arithmetic.
// Formats: a staged input stays int16 while every push is; a float push widens its history once (s / 32768, exact) and
// from then on int16 pushes are widened on arrival, so formats may mix and every output sees the same sample values.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "stream_stage.h"

namespace uwspr {

// K0's stream form (k0_frontend.hip)
int frontend_tap_image(int mode, std::vector<float> &img, int *J, int *dcols);
int frontend_prepare();
int frontend_read_ahead(int mode);
void launch_frontend_stream(hipStream_t s, const void *audio, bool s16, int nin, long long in0, const float *taps,
                            int J, int dcols, float *out, int nout, long long m_first, int nch, long long plane);
// K0 at a centre fc and half-bandwidth hb, and its carrier form (the definition: include/uwspr_hip.h)
bool frontend_carrier_ok(int mode, int fc, int hb);
int frontend_tap_image_at(int mode, int fc, int hb, std::vector<float> &img, int *J, int *dcols);
void frontend_rotator(float *out750);
int frontend_carrier_tables(int mode, const std::vector<int> &carriers, int hb, std::vector<float> &blk, int *J, int *dcols);
void launch_frontend_carrier(hipStream_t s, const void *audio, bool s16, int nin, long long in0, const float *tables, int J,
                             int dcols, float *out, int nout, long long m_first, int nch, int NC, long long plane);
long long frontend_carrier_launch_count(int s16);
void launch_widen_s16(hipStream_t s, const int16_t *in, float *out, size_t n);

// K11, the rational resampler ahead of K0 (k11_resample.hip; the definition: include/uwspr_hip.h)
struct resample_plan {
  int rate = 0, L = 0, M = 0, T = 0, N = 0, D = 0;
  std::vector<double> h;               // T * L taps in binary64 (zero from N on)
};
int resample_design(int rate, resample_plan &out);
void resample_tap_image(const resample_plan &pl, std::vector<float> &img, int *TP);
hipError_t launch_resample(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, const float *taps,
                           const resample_plan &pl, int TP, float *out, long long nout, long long j_first);

// K12, the noise blanker ahead of K11 and K0 (k12_blank.hip; the definition: include/uwspr_hip.h)
hipError_t launch_blank_level(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, float *lev,
                              long long nblk, long long blk_first);
hipError_t launch_blank_apply(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, const float *lev,
                              long long nlev, long long blk0, int blank, int guard, float *out, long long nout, long long y_first,
                              int *nz);
static_assert(stage::BLANK_N == UWSPR_BLANK_BLOCK, "stream_stage.h restates the block length");

enum { RING_EMPTY = 0, RING_IQ = 1, RING_AUDIO = 2 };   // what the stream is, decided by its first push

// What an audio stream's chain is made of: the options its first push latches.
struct audio_chain_cfg {
  int mode;                            // K0's tap mode (option "frontend")
  std::vector<int> carriers;           // K0's centres in Hz, in plane order
  int hbw;                             // K0's half-bandwidth
  int rate;                            // of the pushed audio; any other than 12000 puts K11 ahead of K0
  int blank, guard;                    // blank != 0 puts K12 ahead of both
};
// the part of a chain a refused change or a failed set-up belongs to
enum chain_part { CHAIN_OK = 0, CHAIN_FRONTEND, CHAIN_CARRIERS, CHAIN_RATE, CHAIN_BLANK };

// n elements a stage owns, on the device or page-locked on the host.  alloc() frees what was held first and holds
// nothing after a failure.
template <typename T, bool HOST = false>
struct owned {
  T *p = nullptr;
  size_t n = 0;
  void release() { if (p) (void)(HOST ? hipHostFree(p) : hipFree(p)); p = nullptr; n = 0; }
  hipError_t alloc(size_t count) {
    release();
    const hipError_t e = HOST ? hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, count * sizeof(T));
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
};

struct stream_ring {
  int fl = 0, hop = 0, maxf = 0;
  float *buf[2] = {nullptr, nullptr};
  size_t cap = 0;                      // samples per buffer (per plane)
  int nch = 1;                         // audio channels
  int ncar = 1, npl = 1;               // carriers per channel; planes per buffer (nch * ncar)
  size_t plane = 0;                    // pairs from one plane to the next (>= cap)
  int cur = 0;
  size_t base = 0, have = 0;           // unconsumed samples: buf[cur][base, base + have)
  long long pos = 0;                   // stream index of buf[cur][base]
  hipStream_t copy = nullptr;
  hipEvent_t ev_up = nullptr;          // behind the last append / compaction
  bool up_pending = false;
  std::vector<hipEvent_t> readers[2];  // events after which buf[k] is no longer read
  // page-locked staging for pageable sources
  static constexpr size_t PIECE = 4u << 20;
  char *pin = nullptr;
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  int pin_next = 0;
  bool last_direct = false;            // the last append / push DMAs straight from the caller's (page-locked) buffer
  hipError_t err = hipSuccess;
  int kind = RING_EMPTY;

  // A stage's input: frames of nch samples, int16 while every push so far was (s16), else float.  d[cur] holds
  // [history | new frames] from input h.i_base on; the other buffer takes int16 arrivals on their way to a float
  // history, and the tail when the history's origin moves.  Everything runs on the ring's copy stream.
  struct staged_input {
    owned<char> d[2];
    int cur = 0, s16 = 0;
    stage::history h;
    size_t frame_bytes(const stream_ring &r) const { return (s16 ? 2 : 4) * (size_t)r.nch; }
    bool ensure(stream_ring &r, size_t bytes) { return r.ensure(d[0], bytes) && r.ensure(d[1], bytes); }
    void release() { d[0].release(); d[1].release(); }
    // a stream's first frames: format and history (the caller fills or zeroes it)
    void start(bool s16_, long long i_base, size_t hist) { s16 = s16_; h.i_base = i_base; h.hist = hist; }
    // before the first float frames: an int16 history becomes float
    bool widen_history(stream_ring &r) {
      if (!s16) return true;
      launch_widen_s16(r.copy, (const int16_t *)d[cur].p, (float *)d[cur ^ 1].p, h.hist * (size_t)r.nch);
      cur ^= 1; s16 = 0;
      return (r.err = hipGetLastError()) == hipSuccess;
    }
    // k frames from src (see upload) behind the history; returns the buffer the stage's kernels read (h.hist + k frames
    // from input h.i_base on), null on failure
    char *take(stream_ring &r, const void *src, size_t k, bool s16_in, bool on_device, hipEvent_t src_ready) {
      const size_t C = (size_t)r.nch;
      char *b = d[cur].p, *at = b + h.hist * frame_bytes(r);
      if (s16_in && !s16) {   // (the other buffer is free until keep(), which comes after on the same stream)
        if (!r.upload(d[cur ^ 1].p, src, k * 2 * C, on_device, src_ready)) return nullptr;
        launch_widen_s16(r.copy, (const int16_t *)d[cur ^ 1].p, (float *)at, k * C);
        if ((r.err = hipGetLastError()) != hipSuccess) return nullptr;
      } else if (!r.upload(at, src, k * frame_bytes(r), on_device, src_ready)) {
        return nullptr;
      }
      return b;
    }
    // after the launches on the k frames take() brought: inputs from `from` on are the new history
    bool keep(stream_ring &r, size_t k, long long from) {
      const size_t es = frame_bytes(r);
      const stage::history::tail t = h.advance(k, from);
      if (!t.moves) return true;
      if (t.len && (r.err = hipMemcpyAsync(d[cur ^ 1].p, d[cur].p + t.off * es, t.len * es, hipMemcpyDeviceToDevice, r.copy)) != hipSuccess)
        return false;
      cur ^= 1;
      return true;
    }
  };

  // K0: 12 kS/s frames into the ring, one plane per channel and carrier
  struct audio_state {
    int mode = -1;                     // latched by the first push after open / reset
    int J = 0, dcols = 0, taps_mode = -1;
    // [32][J] float2, the stream's own copy (a batch call may swap the context's).  Anything but {1500 Hz}, 10 Hz runs
    // the carrier form: then frontend_carrier_tables' block -- [ncar][32][J] taps, the rotator table, the carriers mod 375
    owned<float> taps;
    std::vector<int> car, taps_car;    // K0's centre(s) and half-bandwidth, latched with the mode
    int hbw = 0, taps_hbw = 0;
    bool carrier_form = false;
    staged_input in;                   // audio indices; zero before the stream's first sample
    long long m_next = 0;              // stream index of the next output
  } au;
  // K11: frames at another rate into 12 kS/s float frames for K0.  Counters restart at 0 with every open / reset: K0 sees
  // output j as 12 kS/s sample 32 pos + j.
  struct resample_state {
    int rate = 0;                      // latched by the first audio push after open / reset (0: no resampler)
    int taps_rate = 0, TP = 0;
    resample_plan pl;                  // of taps_rate
    owned<float> taps;                 // [L][TP]
    staged_input in;
    long long n_in = 0, j_next = 0;    // inputs pushed, next output
    owned<float> out;                  // [audio_piece_frames()][nch]
  } rs;
  // K12: frames with their impulses zeroed, as float frames at the same rate for K11 or K0.  The level table holds the
  // last three complete blocks ahead of the ones a push completes; the per-block zero counts go to the host through a
  // page-locked queue and are summed there (blank_drain).
  struct blank_state {
    int blank = 0, guard = 0;          // latched by the first audio push after open / reset (blank 0: no blanker)
    staged_input in;
    long long n_in = 0, y_next = 0;    // inputs pushed, next output
    owned<float> out;                  // [audio_piece_frames()][nch]
    owned<float> lev[2];               // [blank_lev_rows][nch]: the levels of blocks lev0 .. blk_done - 1
    int lcur = 0;
    long long lev0 = 0, blk_done = 0;  // first block of the table, complete blocks so far
    owned<int> nz;                     // zero counts [..][nch] of the launches since the last drain
    owned<int, true> h_nz;             // their page-locked copy
    size_t nz_used = 0;                // in ints (multiples of nch)
    std::vector<long long> zeroed;     // per channel, drained so far
    bool stale = false;                // a reset left counts in flight: drained and dropped by the next latch
  } bk;
  // most new samples per K0 launch: AUDIO_PIECE / nch frames (one channel: 131072 outputs, 256 workgroups), so the
  // history buffers hold at most (32 J + 32) nch + AUDIO_PIECE samples whatever the channel count
  static constexpr size_t AUDIO_PIECE = 4u << 20;
  size_t audio_piece_frames() const { return AUDIO_PIECE / (size_t)nch; }

  bool is_open() const { return buf[0] != nullptr; }

  void close() {
    if (copy) (void)hipStreamSynchronize(copy);
    for (int k = 0; k < 2; k++) { if (buf[k]) (void)hipFree(buf[k]); buf[k] = nullptr; readers[k].clear(); }
    if (pin) { (void)hipHostFree(pin); pin = nullptr; }
    for (int k = 0; k < 2; k++) if (pin_ev[k]) { (void)hipEventDestroy(pin_ev[k]); pin_ev[k] = nullptr; }
    if (ev_up) { (void)hipEventDestroy(ev_up); ev_up = nullptr; }
    au.in.release(); au.taps.release();
    au = audio_state();
    rs.in.release(); rs.taps.release(); rs.out.release();
    rs = resample_state();
    bk.in.release(); bk.out.release(); bk.lev[0].release(); bk.lev[1].release(); bk.nz.release(); bk.h_nz.release();
    bk = blank_state();
    if (copy) { (void)hipStreamDestroy(copy); copy = nullptr; }
    cap = 0; plane = 0; nch = 1; ncar = 1; npl = 1; have = 0; base = 0; up_pending = false;
  }

  // takes_of_slack: how many full takes fit behind one another before the tail has to move; nchannels audio channels
  // with ncarriers carriers each: nchannels * ncarriers planes
  bool open(int fl_, int hop_, int max_frames, int takes_of_slack = 6, int nchannels = 1, int ncarriers = 1) {
    close();
    fl = fl_; hop = hop_; maxf = max_frames;
    cap = (size_t)takes_of_slack * max_frames * hop + fl;
    nch = nchannels; ncar = ncarriers; npl = nchannels * ncarriers;
    plane = npl == 1 ? cap : (cap + 63) / 64 * 64;   // (planes start 512-byte aligned)
    for (int k = 0; k < 2; k++)
      if ((err = hipMalloc((void **)&buf[k], plane * npl * 2 * sizeof(float))) != hipSuccess) { close(); return false; }
    if ((err = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking)) != hipSuccess) { close(); return false; }
    if ((err = hipEventCreateWithFlags(&ev_up, hipEventDisableTiming)) != hipSuccess) { close(); return false; }
    cur = 0; base = 0; have = 0; pos = 0; up_pending = false; pin_next = 0;
    kind = RING_EMPTY;
    pin_busy[0] = pin_busy[1] = false;
    return true;
  }

  int ready() const {
    if (have < (size_t)fl) return 0;
    const size_t n = (have - fl) / hop + 1;
    return (int)(n < (size_t)maxf ? n : (size_t)maxf);
  }
  size_t room() const { return 2 * cap > 0 ? cap - have : 0; }   // samples an append can take (after moving the tail)

  // drop what is buffered.  Kernels may still be reading views of the current buffer, so the next append
  // goes through make_room() (base = cap: nothing fits) to the OTHER buffer, behind its readers.
  // An audio stream starts again at audio index 32 p with a zero history.
  void reset(long long p) { have = 0; base = cap; pos = p; kind = RING_EMPTY; au.mode = -1; au.m_next = p; rs.rate = 0;
    if (bk.blank) { bk.blank = 0; bk.stale = true; }
  }

  // make space for n more samples behind the unconsumed ones
  bool make_room(size_t n) {
    if (base + have + n <= cap) return true;
    if (have + n > cap) return false;
    const int other = cur ^ 1;
    for (hipEvent_t e : readers[other])
      if ((err = hipStreamWaitEvent(copy, e, 0)) != hipSuccess) return false;
    readers[other].clear();
    if (have && npl == 1 && (err = hipMemcpyAsync(buf[other], buf[cur] + 2 * base, have * 2 * sizeof(float),
                                                  hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
    if (have && npl > 1 && (err = hipMemcpy2DAsync(buf[other], plane * 2 * sizeof(float), buf[cur] + 2 * base,
                                                   plane * 2 * sizeof(float), have * 2 * sizeof(float), (size_t)npl,
                                                   hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
    cur = other; base = 0;
    return true;
  }

  // n samples of space behind the unconsumed ones (in every plane) for a producer on the copy stream (a kernel), then
  // commit(n).  Returns plane 0.
  float *reserve(size_t n) {
    if (!make_room(n)) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
    return buf[cur] + 2 * (base + have);
  }
  bool commit(size_t n) {
    have += n;
    if ((err = hipEventRecord(ev_up, copy)) != hipSuccess) return false;
    up_pending = true;
    return true;
  }

  // bytes from src to device memory dst on the copy stream.  src: host (page-locked or pageable) when !on_device,
  // else device memory that `src_ready` (may be null: already complete) orders.  A page-locked source is read by
  // the DMA itself (last_direct) and must stay unmodified until wait_uploads().
  bool upload(void *dst, const void *src, size_t bytes, bool on_device, hipEvent_t src_ready) {
    if (on_device) {
      if (src_ready && (err = hipStreamWaitEvent(copy, src_ready, 0)) != hipSuccess) return false;
      return (err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, copy)) == hipSuccess;
    }
    hipPointerAttribute_t at;
    const bool locked = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost;
    if (!locked) (void)hipGetLastError();   // an ordinary pointer is "invalid value" to the query: not an error here
    if (locked) {
      last_direct = true;
      return (err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, copy)) == hipSuccess;
    }
    if (!pin) {
      if ((err = hipHostMalloc((void **)&pin, 2 * PIECE, hipHostMallocDefault)) != hipSuccess) { pin = nullptr; return false; }
      for (int k = 0; k < 2; k++)
        if ((err = hipEventCreateWithFlags(&pin_ev[k], hipEventDisableTiming)) != hipSuccess) return false;
    }
    size_t off = 0;
    while (off < bytes) {
      const size_t m = bytes - off < PIECE ? bytes - off : PIECE;
      const int h = pin_next;
      pin_next ^= 1;
      if (pin_busy[h] && (err = hipEventSynchronize(pin_ev[h])) != hipSuccess) return false;
      memcpy(pin + (size_t)h * PIECE, (const char *)src + off, m);
      if ((err = hipMemcpyAsync((char *)dst + off, pin + (size_t)h * PIECE, m, hipMemcpyHostToDevice, copy)) != hipSuccess) return false;
      if ((err = hipEventRecord(pin_ev[h], copy)) != hipSuccess) return false;
      pin_busy[h] = true;
      off += m;
    }
    return true;
  }

  // n (I,Q) pairs (see upload) of a one-plane ring.  Returns with the transfer enqueued on the copy stream.
  bool append(const float *src, size_t n, bool on_device, hipEvent_t src_ready = nullptr) {
    if (n == 0) return true;
    last_direct = false;
    float *dst = reserve(n);
    if (!dst) return false;
    if (!upload(dst, src, n * 2 * sizeof(float), on_device, src_ready)) return false;
    return commit(n);
  }

  // ---- the audio chain's memory
  // a stage's buffer of `count` elements in place of the one it holds (launches on the copy stream may still read that)
  template <typename O>
  bool renew(O &o, size_t count) {
    if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
    return (err = o.alloc(count)) == hipSuccess;
  }
  template <typename O>
  bool ensure(O &o, size_t count) { return o.n >= count || renew(o, count); }

  // ---- K0
  // outputs a push of n 12 kS/s samples would add, for a stream in front-end mode `mode`
  long long audio_outputs(size_t n, int mode) const {
    const int dcols = frontend_read_ahead(mode) / 32;
    const long long a_end = au.mode >= 0 ? au.in.h.i_base + (long long)au.in.h.hist : 32LL * au.m_next;
    return stage::added(stage::audio_complete(a_end + (long long)n, dcols), au.m_next);
  }

  static bool default_carriers(const std::vector<int> &car, int hbw) {
    return car.size() == 1 && car[0] == UWSPR_CARRIER_DEFAULT && hbw == UWSPR_FRONTEND_HBW_DEFAULT;
  }

  // The first audio push after open / reset: taps of `mode` at the centres cs (ncar carriers, Hz) and half-bandwidth hbw
  // -- the default set {1500}, 10 as one tap image, anything else as the carrier form's tables --, buffers, a zero history.
  bool audio_latch(int mode, bool s16, const std::vector<int> &cs, int hbw) {
    if ((int)cs.size() != ncar) { err = hipErrorInvalidValue; return false; }
    const bool form = !default_carriers(cs, hbw);
    if (au.taps_mode != mode || au.taps_car != cs || au.taps_hbw != hbw) {
      std::vector<float> img;
      int J = 0, dcols = 0;
      if ((form ? frontend_carrier_tables(mode, cs, hbw, img, &J, &dcols) : frontend_tap_image(mode, img, &J, &dcols)) ||
          frontend_prepare()) { err = hipErrorInvalidValue; return false; }
      au.taps_mode = -1;   // (no taps are resident until the new ones have arrived)
      if (!renew(au.taps, img.size())) return false;
      if ((err = hipMemcpy(au.taps.p, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return false;
      au.taps_mode = mode; au.J = J; au.dcols = dcols; au.taps_car = cs; au.taps_hbw = hbw;
    }
    au.carrier_form = form; au.car = cs; au.hbw = hbw;
    if (!au.in.ensure(*this, stage::audio_need(au.J, audio_piece_frames(), (size_t)nch) * sizeof(float))) return false;
    au.mode = mode;
    const long long a0 = stage::audio_keep(au.m_next, au.J, au.dcols);
    au.in.start(s16, a0, (size_t)(32LL * au.m_next - a0));
    if ((err = hipMemsetAsync(au.in.d[au.in.cur].p, 0, au.in.h.hist * au.in.frame_bytes(*this), copy)) != hipSuccess) return false;
    kind = RING_AUDIO;
    return true;
  }

  // A push through one stage: n frames of nch samples (int16 when s16_in, else float) from src (see upload), cut into
  // pieces of at most `piece` frames.  Each piece goes behind the stage's history; stage(b, k, &from) launches on the
  // buffer b for the outputs the k new frames complete, hands them on, and says from which input on the history stays.
  template <typename F>
  bool staged_push(staged_input &in, size_t piece, const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready,
                   F stage) {
    if (n && !s16_in && !in.widen_history(*this)) return false;
    const size_t es_in = (s16_in ? 2 : 4) * (size_t)nch;   // bytes per frame
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      char *b = in.take(*this, (const char *)src + off * es_in, k, s16_in, on_device, src_ready);
      long long from = 0;
      if (!b || !stage(b, k, &from) || !in.keep(*this, k, from)) return false;
      off += k;
    }
    return true;
  }

  // 12 kS/s frames: K0 for the outputs that became complete, straight into the ring.  (The caller has checked room()
  // against chain_outputs().)
  bool push_audio(const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready) {
    return staged_push(au.in, audio_piece_frames(), src, n, s16_in, on_device, src_ready, [this](char *b, size_t k, long long *from) {
      const int held = (int)(au.in.h.hist + k);
      const long long a0 = au.in.h.i_base, m_end = stage::audio_complete(a0 + held, au.dcols);
      if (m_end > au.m_next) {
        const int nout = (int)(m_end - au.m_next);
        float *dst = reserve((size_t)nout);
        if (!dst) return false;
        if (au.carrier_form)
          launch_frontend_carrier(copy, b, au.in.s16, held, a0, au.taps.p, au.J, au.dcols, dst, nout, au.m_next, nch, ncar,
                                  (long long)plane);
        else
          launch_frontend_stream(copy, b, au.in.s16, held, a0, au.taps.p, au.J, au.dcols, dst, nout, au.m_next, nch, (long long)plane);
        if ((err = hipGetLastError()) != hipSuccess) return false;
        if (!commit((size_t)nout)) return false;
        au.m_next = m_end;
      }
      *from = stage::audio_keep(au.m_next, au.J, au.dcols);
      return true;
    });
  }

  // ---- K11
  // 12 kS/s samples a push of n frames at `rate` would add (rate: the latched one, or the one the push would latch);
  // -1: the rate is not supported
  long long resample_outputs(size_t n, int rate) const {
    if (rate == 12000) return (long long)n;
    resample_plan tmp;
    const resample_plan *pl = &rs.pl;
    if (rs.taps_rate != rate) { if (resample_design(rate, tmp)) return -1; pl = &tmp; }
    const bool running = rs.rate == rate;
    return stage::added(stage::resample_complete((running ? rs.n_in : 0) + (long long)n, pl->L, pl->M, pl->D), running ? rs.j_next : 0);
  }
  size_t resample_piece_frames() const { return stage::resample_piece_frames(audio_piece_frames(), rs.pl.L, rs.pl.M); }

  // The first audio push after open / reset at a rate other than 12000: taps and buffers of `rate`, an empty history
  // (inputs before 0 read as zero in the kernel), counters at 0.
  bool resample_latch(int rate, bool s16) {
    if (rs.taps_rate != rate) {
      resample_plan pl;
      std::vector<float> img;
      int TP = 0;
      if (resample_design(rate, pl)) { err = hipErrorInvalidValue; return false; }
      resample_tap_image(pl, img, &TP);
      rs.taps_rate = 0;
      if (!renew(rs.taps, img.size())) return false;
      if ((err = hipMemcpy(rs.taps.p, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return false;
      rs.taps_rate = rate; rs.pl = pl; rs.TP = TP;
    }
    const size_t C = (size_t)nch;
    if (!rs.in.ensure(*this, stage::resample_in_need(rs.pl.T, resample_piece_frames(), C) * sizeof(float)) ||
        !ensure(rs.out, stage::resample_out_need(audio_piece_frames(), C))) return false;
    rs.rate = rate; rs.n_in = 0; rs.j_next = 0;
    rs.in.start(s16, 0, 0);
    return true;
  }

  // frames at the latched rate: K11 for the outputs that became complete, those on to K0
  bool push_resampled(const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready) {
    return staged_push(rs.in, resample_piece_frames(), src, n, s16_in, on_device, src_ready, [this](char *b, size_t k, long long *from) {
      const resample_plan &pl = rs.pl;
      rs.n_in += (long long)k;
      const long long j_end = stage::resample_complete(rs.n_in, pl.L, pl.M, pl.D);
      if (j_end > rs.j_next) {
        const long long nout = j_end - rs.j_next;
        if ((size_t)nout * (size_t)nch > rs.out.n) { err = hipErrorInvalidValue; return false; }
        if ((err = launch_resample(copy, b, rs.in.s16 != 0, (long long)(rs.in.h.hist + k), rs.in.h.i_base, nch, rs.taps.p, pl, rs.TP,
                                   rs.out.p, nout, rs.j_next)) != hipSuccess) return false;
        rs.j_next = j_end;
        if (!push_audio(rs.out.p, (size_t)nout, false, true, nullptr)) return false;
      }
      *from = stage::resample_keep(rs.j_next, pl.L, pl.M, pl.T, pl.D);
      return true;
    });
  }

  // ---- K12
  // samples a push of n frames would complete, for the blanker that runs or the one the push would latch (blank 0: n)
  long long blank_outputs(size_t n, int blank, int guard) const {
    if (!blank) return (long long)n;
    const bool running = bk.blank != 0;
    return stage::added(stage::blank_complete((running ? bk.n_in : 0) + (long long)n, guard), running ? bk.y_next : 0);
  }

  // The first audio push after open / reset with "blank" != 0: buffers, an empty history, counters at 0.
  bool blank_latch(int blank, int guard, bool s16) {
    const size_t C = (size_t)nch, piece = audio_piece_frames();
    if (bk.stale && (err = hipStreamSynchronize(copy)) != hipSuccess) return false;   // (counts of the stream before the reset)
    bk.stale = false;
    if (!bk.in.ensure(*this, stage::blank_in_need(piece, C) * sizeof(float)) || !ensure(bk.out, piece * C) ||
        !ensure(bk.lev[0], stage::blank_lev_rows(piece) * C) || !ensure(bk.lev[1], stage::blank_lev_rows(piece) * C) ||
        !ensure(bk.nz, stage::blank_nz_cap(piece, C)) || !ensure(bk.h_nz, stage::blank_nz_cap(piece, C))) return false;
    bk.blank = blank; bk.guard = guard;
    bk.n_in = 0; bk.y_next = 0; bk.lev0 = 0; bk.blk_done = 0; bk.nz_used = 0;
    bk.in.start(s16, 0, 0);
    bk.zeroed.assign(C, 0);
    return true;
  }

  // the zero counts the launches so far have written: wait for the copy stream, add them up per channel
  bool blank_drain() {
    if (!bk.nz_used) return true;
    if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
    for (size_t i = 0; i < bk.nz_used; i++) bk.zeroed[i % (size_t)nch] += bk.h_nz.p[i];
    bk.nz_used = 0;
    return true;
  }
  // per-channel totals since open / reset: outputs made and outputs zeroed (both 0 without a blanker)
  bool blank_stats(long long *samples, long long *zeroed, int cap) {
    if (bk.blank && !blank_drain()) return false;
    for (int k = 0; k < nch && k < cap; k++) {
      samples[k] = bk.blank ? bk.y_next : 0;
      zeroed[k] = bk.blank ? bk.zeroed[(size_t)k] : 0;
    }
    return true;
  }

  // frames at the pushed rate: k12_level for the blocks that became complete, k12_apply for the outputs, those on to
  // K11 or K0
  bool push_blanked(const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready) {
    return staged_push(bk.in, audio_piece_frames(), src, n, s16_in, on_device, src_ready, [this](char *b, size_t k, long long *from) {
      const size_t C = (size_t)nch;
      const long long held = (long long)(bk.in.h.hist + k), in0 = bk.in.h.i_base;
      bk.n_in += (long long)k;
      const long long done = stage::blank_blocks_done(bk.n_in);
      if (done > bk.blk_done) {
        if ((size_t)(done - bk.lev0) * C > bk.lev[bk.lcur].n) { err = hipErrorInvalidValue; return false; }
        if ((err = launch_blank_level(copy, b, bk.in.s16 != 0, held, in0, nch, bk.lev[bk.lcur].p + (size_t)(bk.blk_done - bk.lev0) * C,
                                      done - bk.blk_done, bk.blk_done)) != hipSuccess) return false;
        bk.blk_done = done;
      }
      const long long y_end = stage::blank_complete(bk.n_in, bk.guard);
      if (y_end > bk.y_next) {
        const long long nout = y_end - bk.y_next;
        const size_t nzn = (size_t)stage::blank_blocks_of(bk.y_next, nout) * C;
        if ((size_t)nout * C > bk.out.n || nzn > bk.nz.n) { err = hipErrorInvalidValue; return false; }
        if (bk.nz_used + nzn > bk.nz.n && !blank_drain()) return false;
        if ((err = launch_blank_apply(copy, b, bk.in.s16 != 0, held, in0, nch, bk.lev[bk.lcur].p, bk.blk_done - bk.lev0, bk.lev0, bk.blank,
                                      bk.guard, bk.out.p, nout, bk.y_next, bk.nz.p + bk.nz_used)) != hipSuccess) return false;
        if ((err = hipMemcpyAsync(bk.h_nz.p + bk.nz_used, bk.nz.p + bk.nz_used, nzn * sizeof(int), hipMemcpyDeviceToHost, copy)) != hipSuccess)
          return false;
        bk.nz_used += nzn;
        bk.y_next = y_end;
        if (!(rs.rate ? push_resampled(bk.out.p, (size_t)nout, false, true, nullptr) : push_audio(bk.out.p, (size_t)nout, false, true, nullptr)))
          return false;
      }
      const long long lev0n = stage::blank_lev_first(bk.blk_done);
      if (lev0n != bk.lev0) {
        if ((err = hipMemcpyAsync(bk.lev[bk.lcur ^ 1].p, bk.lev[bk.lcur].p + (size_t)(lev0n - bk.lev0) * C,
                                  (size_t)(bk.blk_done - lev0n) * C * sizeof(float), hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
        bk.lcur ^= 1; bk.lev0 = lev0n;
      }
      *from = stage::blank_keep(bk.y_next, bk.guard, bk.blk_done);
      return true;
    });
  }

  // ---- the chain: what the two doors (uwspr_stream_push_audio, uwspr_pipe_push_audio_channels) see of all this
  // the rate an audio stream runs at (0: no audio stream runs)
  int chain_running_rate() const { return kind != RING_AUDIO ? 0 : rs.rate ? rs.rate : 12000; }
  // what the running audio stream has latched (rate 0: none runs)
  audio_chain_cfg chain_latched() const { return {au.mode, au.car, au.hbw, chain_running_rate(), bk.blank, bk.guard}; }
  // the first setting of c that differs from what the running audio stream has latched ("blank_guard" counts with a
  // blanker only); CHAIN_OK: none, or no audio stream runs
  chain_part chain_mismatch(const audio_chain_cfg &c) const {
    if (kind != RING_AUDIO) return CHAIN_OK;
    if (c.mode != au.mode) return CHAIN_FRONTEND;
    if (c.carriers != au.car || c.hbw != au.hbw) return CHAIN_CARRIERS;
    if (c.rate != chain_running_rate()) return CHAIN_RATE;
    if (c.blank != bk.blank || (c.blank && c.guard != bk.guard)) return CHAIN_BLANK;
    return CHAIN_OK;
  }
  // the resampler's ratio L / M = 12000 / rate (1 / 1 without one)
  void chain_ratio(int *L, int *M) const { *L = rs.rate ? rs.pl.L : 1; *M = rs.rate ? rs.pl.M : 1; }
  // ring samples a push of n frames would add, for the running chain or the one c would latch; -1: c.rate is not supported
  long long chain_outputs(size_t n, const audio_chain_cfg &c) const {
    const long long n12 = resample_outputs((size_t)blank_outputs(n, c.blank, c.guard), c.rate);
    return n12 < 0 ? -1 : audio_outputs((size_t)n12, c.mode);
  }
  // Before the first audio push after open / reset (nothing to do while a stream runs): every stage of c, the first
  // taking the pushed format and the ones behind it float frames.  Returns the stage that failed (err says why).
  chain_part chain_latch(const audio_chain_cfg &c, bool s16) {
    if (kind == RING_AUDIO) return CHAIN_OK;
    const bool bk_on = c.blank != 0, rs_on = c.rate != 12000;
    if (bk_on && !blank_latch(c.blank, c.guard, s16)) return CHAIN_BLANK;
    if (rs_on && !resample_latch(c.rate, s16 && !bk_on)) return CHAIN_RATE;
    if (!audio_latch(c.mode, s16 && !rs_on && !bk_on, c.carriers, c.hbw)) return CHAIN_FRONTEND;
    return CHAIN_OK;
  }
  // n frames of nch samples into the latched chain's first stage.  The caller has checked room() against chain_outputs(n).
  bool chain_push(const void *src, size_t n, bool s16, bool on_device, hipEvent_t src_ready = nullptr) {
    last_direct = false;
    if (!(bk.blank ? push_blanked(src, n, s16, on_device, src_ready)
          : rs.rate ? push_resampled(src, n, s16, on_device, src_ready)
                    : push_audio(src, n, s16, on_device, src_ready))) return false;
    if (n && (err = hipEventRecord(ev_up, copy)) != hipSuccess) return false;
    if (n) up_pending = true;
    return true;
  }

  bool wait_uploads() {
    if (up_pending && (err = hipEventSynchronize(ev_up)) != hipSuccess) return false;
    up_pending = false;
    return true;
  }

  // The next k frames in place (plane 0; channel c at + 2 * c * plane floats); `consumer` is the stream whose kernels
  // will read them.
  // *bufidx = which buffer they live in (for reader_done).
  bool view(int k, hipStream_t consumer, const float **frames, long long *first_pos, int *bufidx) {
    if (k <= 0 || k > ready()) { err = hipErrorInvalidValue; return false; }
    if ((err = hipStreamWaitEvent(consumer, ev_up, 0)) != hipSuccess) return false;
    *frames = buf[cur] + 2 * base;
    if (first_pos) *first_pos = pos;
    if (bufidx) *bufidx = cur;
    const size_t used = (size_t)k * hop;
    base += used; have -= used; pos += (long long)used;
    return true;
  }
  void reader_done(int bufidx, hipEvent_t e) {
    for (hipEvent_t q : readers[bufidx]) if (q == e) return;   // re-recorded: a wait sees its newest record
    readers[bufidx].push_back(e);
  }
};

}  // namespace uwspr
