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
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

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
long long blank_blocks_of(long long y_first, long long nout);

enum { RING_EMPTY = 0, RING_IQ = 1, RING_AUDIO = 2 };   // what the stream is, decided by its first push

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
  bool last_direct = false;            // the last append DMAs straight from the caller's (page-locked) buffer
  hipError_t err = hipSuccess;
  int kind = RING_EMPTY;
  // Audio streams (push_audio): 12 kS/s real samples (frames of nch interleaved samples) go through K0 into the
  // ring.  Output m of the stream is y[m] = sum_k g[k] x[32 m + D - k] (audio index 32 m = stream index m) and is
  // produced as soon as x[32 m + D] has been pushed.  The device buffer holds [history | new frames]: the history is
  // the audio from index 32 (m_next + dcols - J) on, at most 32 J frames, zero before the stream's first sample.
  struct audio_state {
    int mode = -1;                     // latched by the first push after open / reset
    int s16 = 0;                       // the buffer holds int16 samples (every push so far was int16), else float
    int J = 0, dcols = 0, taps_mode = -1;
    float *d_taps = nullptr;           // [32][J] float2, the stream's own copy (a batch call may swap the context's)
    // K0's centre(s) and half-bandwidth, latched with the mode.  Anything but {1500 Hz}, 10 Hz runs the carrier form:
    // d_taps is then frontend_carrier_tables' block: [ncar][32][J] taps, the rotator table, the carriers mod 375
    std::vector<int> car, taps_car;
    int hbw = 0, taps_hbw = 0;
    bool carrier_form = false;
    char *d_buf[2] = {nullptr, nullptr};
    size_t buf_bytes = 0;
    int cur = 0;
    long long a0 = 0;                  // audio index of d_buf[cur][0]
    size_t hist = 0;                   // frames held in d_buf[cur]: audio [a0, a0 + hist)
    long long m_next = 0;              // stream index of the next output
  } au;
  // Audio at another rate (option "audio_rate" != 12000): the pushed frames go through K11 into a device buffer of
  // 12 kS/s float frames, which push_audio takes as a device source on the same stream.  Output j of the resampler is
  // complete as soon as input floor((j M + D) / L) has been pushed; the device buffer holds [history | new frames], the
  // history being the inputs from floor((j_next M + D) / L) - (T - 1) on (at most T - 1 frames, zero before the first).
  // Counters restart at 0 with every open / reset: K0 sees output j as 12 kS/s sample 32 pos + j.
  struct resample_state {
    int rate = 0;                      // latched by the first audio push after open / reset (0: none yet; 12000: no resampler)
    int taps_rate = 0, TP = 0;
    resample_plan pl;                  // of taps_rate
    float *d_taps = nullptr;           // [L][TP]
    int s16 = 0;                       // the input buffer holds int16 frames (every push so far was int16)
    char *d_in[2] = {nullptr, nullptr};
    size_t in_bytes = 0;
    int cur = 0;
    long long i_base = 0;              // input index of d_in[cur][0]
    size_t hist = 0;                   // frames held: inputs [i_base, i_base + hist)
    long long n_in = 0, j_next = 0;    // inputs pushed, next output
    float *d_out = nullptr;            // [out_frames][nch]
    size_t out_frames = 0;
  } rs;
  // Impulsive noise (option "blank" != 0): the pushed frames go through K12 into a device buffer of float frames at the
  // same rate, which push_resampled or push_audio takes as a device source on the same stream.  Output i is complete as
  // soon as input i + G has been pushed.  The device buffer holds [history | new frames]: the history is whatever is
  // not yet output plus its guard (inputs from y_next - G on) and the incomplete block (from (n_in div N) N on), at
  // most N + 2 G frames.  The level table holds the last three complete blocks ahead of the ones a push completes.
  // The per-block zero counts go to the host through a page-locked queue and are summed there (blank_drain).
  struct blank_state {
    int blank = 0, guard = 0;          // latched by the first audio push after open / reset (blank 0: no blanker)
    int s16 = 0;                       // the input buffer holds int16 frames (every push so far was int16)
    char *d_in[2] = {nullptr, nullptr};
    size_t in_bytes = 0;
    int cur = 0;
    long long i_base = 0;              // input index of d_in[cur][0]
    size_t hist = 0;                   // frames held: inputs [i_base, i_base + hist)
    long long n_in = 0, y_next = 0;    // inputs pushed, next output
    float *d_out = nullptr;            // [out_frames][nch]
    size_t out_frames = 0;
    float *d_lev[2] = {nullptr, nullptr};   // [lev_rows][nch]: the levels of blocks lev0 .. blk_done - 1
    size_t lev_rows = 0;
    int lcur = 0;
    long long lev0 = 0, blk_done = 0;  // first block of the table, complete blocks so far
    int *d_nz = nullptr, *h_nz = nullptr;   // zero counts [..][nch] of the launches since the last drain, device and page-locked host
    size_t nz_cap = 0, nz_used = 0;    // in ints (multiples of nch)
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
    for (int k = 0; k < 2; k++) if (au.d_buf[k]) { (void)hipFree(au.d_buf[k]); au.d_buf[k] = nullptr; }
    if (au.d_taps) { (void)hipFree(au.d_taps); au.d_taps = nullptr; }
    au = audio_state();
    for (int k = 0; k < 2; k++) if (rs.d_in[k]) (void)hipFree(rs.d_in[k]);
    if (rs.d_out) (void)hipFree(rs.d_out);
    if (rs.d_taps) (void)hipFree(rs.d_taps);
    rs = resample_state();
    for (int k = 0; k < 2; k++) { if (bk.d_in[k]) (void)hipFree(bk.d_in[k]); if (bk.d_lev[k]) (void)hipFree(bk.d_lev[k]); }
    if (bk.d_out) (void)hipFree(bk.d_out);
    if (bk.d_nz) (void)hipFree(bk.d_nz);
    if (bk.h_nz) (void)hipHostFree(bk.h_nz);
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

  // ---- audio streams
  // stream index one past the last output that audio [.., a_end) completes (floor division: a_end may be < D)
  static long long audio_complete(long long a_end, int dcols) {
    const long long t = a_end - 1 - 32LL * dcols;
    return (t >= 0 ? t / 32 : -((-t + 31) / 32)) + 1;
  }
  // outputs a push of n samples would add, for a stream in front-end mode `mode`
  long long audio_outputs(size_t n, int mode) const {
    const int dcols = frontend_read_ahead(mode) / 32;
    const long long a_end = au.mode >= 0 ? au.a0 + (long long)au.hist : 32LL * au.m_next;
    const long long m = audio_complete(a_end + (long long)n, dcols);
    return m > au.m_next ? m - au.m_next : 0;
  }

  static bool default_carriers(const std::vector<int> &car, int hbw) {
    return car.size() == 1 && car[0] == UWSPR_CARRIER_DEFAULT && hbw == UWSPR_FRONTEND_HBW_DEFAULT;
  }

  // The first audio push after open / reset: taps of `mode`, buffers, a zero history.  car (ncar carriers, Hz) and hbw:
  // K0's centres and half-bandwidth; null: the default set {1500}, 10.
  bool audio_latch(int mode, bool s16, const std::vector<int> *car = nullptr, int hbw = UWSPR_FRONTEND_HBW_DEFAULT) {
    const std::vector<int> dflt(1, UWSPR_CARRIER_DEFAULT);
    const std::vector<int> &cs = car ? *car : dflt;
    if ((int)cs.size() != ncar) { err = hipErrorInvalidValue; return false; }
    if (!default_carriers(cs, hbw)) return carrier_latch(mode, s16, cs, hbw);
    au.carrier_form = false; au.car = cs; au.hbw = hbw;
    if (au.taps_mode != mode || !default_carriers(au.taps_car, au.taps_hbw)) {
      std::vector<float> img;
      int J = 0, dcols = 0;
      if (frontend_tap_image(mode, img, &J, &dcols) || frontend_prepare()) { err = hipErrorInvalidValue; return false; }
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;   // (launches with the old taps)
      if (au.d_taps) { (void)hipFree(au.d_taps); au.d_taps = nullptr; }
      if ((err = hipMalloc((void **)&au.d_taps, img.size() * sizeof(float))) != hipSuccess) { au.d_taps = nullptr; return false; }
      if ((err = hipMemcpy(au.d_taps, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return false;
      au.taps_mode = mode; au.J = J; au.dcols = dcols; au.taps_car = cs; au.taps_hbw = hbw;
    }
    return audio_latch_buffers(mode, s16);
  }

  // the carrier form's tables: one tap image per carrier, the rotator table, the carriers mod 375
  bool carrier_latch(int mode, bool s16, const std::vector<int> &cs, int hbw) {
    if (au.taps_mode != mode || au.taps_car != cs || au.taps_hbw != hbw) {
      std::vector<float> all;
      int J = 0, dcols = 0;
      if (frontend_carrier_tables(mode, cs, hbw, all, &J, &dcols) || frontend_prepare()) { err = hipErrorInvalidValue; return false; }
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;   // (launches with the old taps)
      if (au.d_taps) { (void)hipFree(au.d_taps); au.d_taps = nullptr; }
      au.taps_mode = -1;
      if ((err = hipMalloc((void **)&au.d_taps, all.size() * sizeof(float))) != hipSuccess) { au.d_taps = nullptr; return false; }
      if ((err = hipMemcpy(au.d_taps, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return false;
      au.taps_mode = mode; au.J = J; au.dcols = dcols; au.taps_car = cs; au.taps_hbw = hbw;
    }
    au.carrier_form = true; au.car = cs; au.hbw = hbw;
    return audio_latch_buffers(mode, s16);
  }

  bool audio_latch_buffers(int mode, bool s16) {
    const size_t need = ((32 * (size_t)au.J + 32) * nch + audio_piece_frames() * nch) * sizeof(float);
    if (au.buf_bytes < need) {
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
      for (int k = 0; k < 2; k++) {
        if (au.d_buf[k]) { (void)hipFree(au.d_buf[k]); au.d_buf[k] = nullptr; }
        if ((err = hipMalloc((void **)&au.d_buf[k], need)) != hipSuccess) { au.d_buf[k] = nullptr; au.buf_bytes = 0; return false; }
      }
      au.buf_bytes = need;
    }
    au.mode = mode; au.s16 = s16;
    au.a0 = 32 * (au.m_next + au.dcols - au.J);
    au.hist = (size_t)(32LL * au.m_next - au.a0);
    if ((err = hipMemsetAsync(au.d_buf[au.cur], 0, au.hist * nch * (s16 ? 2 : 4), copy)) != hipSuccess) return false;
    kind = RING_AUDIO;
    return true;
  }

  // n audio frames of nch samples (int16 when s16, else float) from src (see upload): upload behind the history, K0
  // for the outputs that became complete straight into the ring (one plane per channel), keep the new tail as
  // history.  The caller has latched the stream and checked room() against audio_outputs(n).  An int16 stream stays int16 while every push is; a float push
  // widens its history once (s / 32768, exact) and from then on int16 pushes are widened on arrival, so formats may
  // mix and every output sees the same sample values.
  bool push_audio(const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready = nullptr) {
    last_direct = false;
    const size_t C = (size_t)nch;
    if (n && au.s16 && !s16_in) {
      launch_widen_s16(copy, (const int16_t *)au.d_buf[au.cur], (float *)au.d_buf[au.cur ^ 1], au.hist * C);
      if ((err = hipGetLastError()) != hipSuccess) return false;
      au.cur ^= 1; au.s16 = 0;
    }
    const bool widen = s16_in && !au.s16;   // int16 samples into a float buffer
    const size_t es = (au.s16 ? 2 : 4) * C, es_in = (s16_in ? 2 : 4) * C;   // bytes per frame
    const size_t piece = audio_piece_frames();
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      char *b = au.d_buf[au.cur];
      if (widen) {   // (the other buffer is free until the tail copy below, which comes after on the same stream)
        char *tmp = au.d_buf[au.cur ^ 1];
        if (!upload(tmp, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) return false;
        launch_widen_s16(copy, (const int16_t *)tmp, (float *)(b + au.hist * es), k * C);
        if ((err = hipGetLastError()) != hipSuccess) return false;
      } else if (!upload(b + au.hist * es, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) {
        return false;
      }
      const long long a_end = au.a0 + (long long)(au.hist + k);
      const long long m_end = audio_complete(a_end, au.dcols);
      if (m_end > au.m_next) {
        const int nout = (int)(m_end - au.m_next);
        float *dst = reserve((size_t)nout);
        if (!dst) return false;
        if (au.carrier_form)
          launch_frontend_carrier(copy, b, au.s16, (int)(au.hist + k), au.a0, au.d_taps, au.J, au.dcols, dst, nout, au.m_next,
                                  nch, ncar, (long long)plane);
        else
          launch_frontend_stream(copy, b, au.s16, (int)(au.hist + k), au.a0, au.d_taps, au.J, au.dcols, dst, nout, au.m_next,
                                 nch, (long long)plane);
        if ((err = hipGetLastError()) != hipSuccess) return false;
        if (!commit((size_t)nout)) return false;
        au.m_next = m_end;
      }
      const long long a0n = 32 * (au.m_next + au.dcols - au.J);
      au.hist = (size_t)(a_end - a0n);
      if (a0n != au.a0) {   // the tail to the front of the other buffer
        if ((err = hipMemcpyAsync(au.d_buf[au.cur ^ 1], b + (size_t)(a0n - au.a0) * es, au.hist * es,
                                  hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
        au.cur ^= 1; au.a0 = a0n;
      }
      off += k;
    }
    if (n && (err = hipEventRecord(ev_up, copy)) != hipSuccess) return false;
    if (n) up_pending = true;
    return true;
  }

  // ---- audio at another rate (K11 ahead of K0)
  // one past the last resampler output that n_in pushed inputs complete
  static long long resample_complete(long long n_in, const resample_plan &pl) {
    const long long t = n_in * pl.L - 1 - pl.D;
    return t >= 0 ? t / pl.M + 1 : 0;
  }
  // 12 kS/s samples a push of n frames at `rate` would add (rate: the latched one, or the one the push would latch);
  // -1: the rate is not supported
  long long resample_outputs(size_t n, int rate) const {
    if (rate == 12000) return (long long)n;
    resample_plan tmp;
    const resample_plan *pl = &rs.pl;
    if (rs.taps_rate != rate) { if (resample_design(rate, tmp)) return -1; pl = &tmp; }
    const bool running = rs.rate == rate;
    const long long j = resample_complete((running ? rs.n_in : 0) + (long long)n, *pl);
    const long long jn = running ? rs.j_next : 0;
    return j > jn ? j - jn : 0;
  }
  // most input frames per K11 launch: its outputs fit d_out (audio_piece_frames() frames, one K0 piece) whatever L / M is
  size_t resample_piece_frames() const {
    const size_t outp = audio_piece_frames();
    const size_t by_out = (size_t)((long long)(outp - 2) * rs.pl.M / rs.pl.L);
    return by_out < outp ? by_out : outp;
  }

  // The first audio push after open / reset at a rate other than 12000: taps and buffers of `rate`, zero history,
  // counters at 0.  (The caller latches K0's side with audio_latch(mode, false): the resampler delivers float frames.)
  bool resample_latch(int rate, bool s16) {
    if (rs.taps_rate != rate) {
      resample_plan pl;
      std::vector<float> img;
      int TP = 0;
      if (resample_design(rate, pl)) { err = hipErrorInvalidValue; return false; }
      resample_tap_image(pl, img, &TP);
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;   // (launches with the old taps)
      if (rs.d_taps) { (void)hipFree(rs.d_taps); rs.d_taps = nullptr; rs.taps_rate = 0; }
      if ((err = hipMalloc((void **)&rs.d_taps, img.size() * sizeof(float))) != hipSuccess) { rs.d_taps = nullptr; return false; }
      if ((err = hipMemcpy(rs.d_taps, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return false;
      rs.taps_rate = rate; rs.pl = pl; rs.TP = TP;
    }
    const size_t C = (size_t)nch, outp = audio_piece_frames();
    const size_t need = ((size_t)rs.pl.T + resample_piece_frames()) * C * sizeof(float);
    if (rs.in_bytes < need || rs.out_frames < outp) {
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
      for (int k = 0; k < 2; k++) {
        if (rs.d_in[k]) { (void)hipFree(rs.d_in[k]); rs.d_in[k] = nullptr; }
        rs.in_bytes = 0;
        if ((err = hipMalloc((void **)&rs.d_in[k], need)) != hipSuccess) { rs.d_in[k] = nullptr; return false; }
      }
      rs.in_bytes = need;
      if (rs.d_out) { (void)hipFree(rs.d_out); rs.d_out = nullptr; }
      rs.out_frames = 0;
      if ((err = hipMalloc((void **)&rs.d_out, outp * C * sizeof(float))) != hipSuccess) { rs.d_out = nullptr; return false; }
      rs.out_frames = outp;
    }
    rs.rate = rate; rs.s16 = s16;
    rs.i_base = 0; rs.hist = 0; rs.n_in = 0; rs.j_next = 0;   // (inputs before 0 read as zero in the kernel)
    return true;
  }

  // n frames of nch samples at the latched rate: behind the resampler's history, K11 for the outputs that became
  // complete, those into push_audio as a device source on the copy stream.  Formats mix as in push_audio.  The caller
  // has latched both sides and checked room() against audio_outputs(resample_outputs(n)).
  bool push_resampled(const void *src, size_t n, bool s16_in, bool on_device, hipEvent_t src_ready = nullptr) {
    const size_t C = (size_t)nch;
    bool direct = false;
    if (n && rs.s16 && !s16_in) {
      launch_widen_s16(copy, (const int16_t *)rs.d_in[rs.cur], (float *)rs.d_in[rs.cur ^ 1], rs.hist * C);
      if ((err = hipGetLastError()) != hipSuccess) return false;
      rs.cur ^= 1; rs.s16 = 0;
    }
    const bool widen = s16_in && !rs.s16;
    const size_t es = (rs.s16 ? 2 : 4) * C, es_in = (s16_in ? 2 : 4) * C;
    const size_t piece = resample_piece_frames();
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      char *b = rs.d_in[rs.cur];
      last_direct = false;
      if (widen) {
        char *tmp = rs.d_in[rs.cur ^ 1];
        if (!upload(tmp, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) return false;
        launch_widen_s16(copy, (const int16_t *)tmp, (float *)(b + rs.hist * es), k * C);
        if ((err = hipGetLastError()) != hipSuccess) return false;
      } else if (!upload(b + rs.hist * es, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) {
        return false;
      }
      direct = direct || last_direct;
      rs.n_in += (long long)k;
      const long long j_end = resample_complete(rs.n_in, rs.pl);
      if (j_end > rs.j_next) {
        const long long nout = j_end - rs.j_next;
        if ((size_t)nout > rs.out_frames) { err = hipErrorInvalidValue; return false; }
        if ((err = launch_resample(copy, b, rs.s16 != 0, (long long)(rs.hist + k), rs.i_base, nch, rs.d_taps, rs.pl, rs.TP,
                                   rs.d_out, nout, rs.j_next)) != hipSuccess) return false;
        rs.j_next = j_end;
        if (!push_audio(rs.d_out, (size_t)nout, false, true, nullptr)) return false;
      }
      // keep the inputs the next output's window starts at
      long long keep = (rs.j_next * rs.pl.M + rs.pl.D) / rs.pl.L - (rs.pl.T - 1);
      if (keep > rs.n_in) keep = rs.n_in;
      if (keep < rs.i_base) keep = rs.i_base;
      const size_t nh = (size_t)(rs.n_in - keep);
      if (keep != rs.i_base) {   // the tail to the front of the other buffer
        if (nh && (err = hipMemcpyAsync(rs.d_in[rs.cur ^ 1], b + (size_t)(keep - rs.i_base) * es, nh * es,
                                        hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
        rs.cur ^= 1; rs.i_base = keep;
      }
      rs.hist = nh;
      off += k;
    }
    last_direct = direct;
    if (n && (err = hipEventRecord(ev_up, copy)) != hipSuccess) return false;
    if (n) up_pending = true;
    return true;
  }

  // ---- impulsive noise (K12 ahead of K11 and K0)
  static constexpr long long BLANK_N = UWSPR_BLANK_BLOCK;
  // samples a push of n frames would complete, for the blanker that runs or the one the push would latch (blank 0: n)
  long long blank_outputs(size_t n, int blank, int guard) const {
    if (!blank) return (long long)n;
    const bool running = bk.blank != 0;
    const long long y = (running ? bk.n_in : 0) + (long long)n - guard, yn = running ? bk.y_next : 0;
    return y > yn ? y - yn : 0;
  }
  size_t blank_piece_frames() const { return audio_piece_frames(); }

  // The first audio push after open / reset with "blank" != 0: buffers, an empty history, counters at 0.  (The caller
  // latches the stages behind with float input: the blanker delivers float frames.)
  bool blank_latch(int blank, int guard, bool s16) {
    const size_t C = (size_t)nch, piece = blank_piece_frames();
    const size_t need = ((size_t)BLANK_N + 2 * 64 + piece) * C * sizeof(float);
    const size_t rows = piece / (size_t)BLANK_N + 6, nzc = (piece / (size_t)BLANK_N + 2) * C * 64;
    if (bk.stale && (err = hipStreamSynchronize(copy)) != hipSuccess) return false;   // (counts of the stream before the reset)
    bk.stale = false;
    if (bk.in_bytes < need || bk.out_frames < piece || bk.lev_rows < rows || bk.nz_cap < nzc) {
      if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
      for (int k = 0; k < 2; k++) {
        if (bk.d_in[k]) { (void)hipFree(bk.d_in[k]); bk.d_in[k] = nullptr; }
        if (bk.d_lev[k]) { (void)hipFree(bk.d_lev[k]); bk.d_lev[k] = nullptr; }
      }
      if (bk.d_out) { (void)hipFree(bk.d_out); bk.d_out = nullptr; }
      if (bk.d_nz) { (void)hipFree(bk.d_nz); bk.d_nz = nullptr; }
      if (bk.h_nz) { (void)hipHostFree(bk.h_nz); bk.h_nz = nullptr; }
      bk.in_bytes = 0; bk.out_frames = 0; bk.lev_rows = 0; bk.nz_cap = 0;
      for (int k = 0; k < 2; k++) {
        if ((err = hipMalloc((void **)&bk.d_in[k], need)) != hipSuccess) { bk.d_in[k] = nullptr; return false; }
        if ((err = hipMalloc((void **)&bk.d_lev[k], rows * C * sizeof(float))) != hipSuccess) { bk.d_lev[k] = nullptr; return false; }
      }
      if ((err = hipMalloc((void **)&bk.d_out, piece * C * sizeof(float))) != hipSuccess) { bk.d_out = nullptr; return false; }
      if ((err = hipMalloc((void **)&bk.d_nz, nzc * sizeof(int))) != hipSuccess) { bk.d_nz = nullptr; return false; }
      if ((err = hipHostMalloc((void **)&bk.h_nz, nzc * sizeof(int), hipHostMallocDefault)) != hipSuccess) { bk.h_nz = nullptr; return false; }
      bk.in_bytes = need; bk.out_frames = piece; bk.lev_rows = rows; bk.nz_cap = nzc;
    }
    bk.blank = blank; bk.guard = guard; bk.s16 = s16;
    bk.i_base = 0; bk.hist = 0; bk.n_in = 0; bk.y_next = 0; bk.lev0 = 0; bk.blk_done = 0; bk.nz_used = 0;
    bk.zeroed.assign(C, 0);
    return true;
  }

  // the zero counts the launches so far have written: wait for the copy stream, add them up per channel
  bool blank_drain() {
    if (!bk.nz_used) return true;
    if ((err = hipStreamSynchronize(copy)) != hipSuccess) return false;
    for (size_t i = 0; i < bk.nz_used; i++) bk.zeroed[i % (size_t)nch] += bk.h_nz[i];
    bk.nz_used = 0;
    return true;
  }

  // n frames of nch samples: behind the blanker's history, k12_level for the blocks the push completes, k12_apply for
  // the outputs it completes, those into push_resampled (rs_on) or push_audio as a device source on the copy stream.
  // Formats mix as in push_audio.  The caller has latched every stage and checked room() against what the outputs make.
  bool push_blanked(const void *src, size_t n, bool s16_in, bool on_device, bool rs_on, hipEvent_t src_ready = nullptr) {
    const size_t C = (size_t)nch;
    const long long G = bk.guard;
    bool direct = false;
    if (n && bk.s16 && !s16_in) {
      launch_widen_s16(copy, (const int16_t *)bk.d_in[bk.cur], (float *)bk.d_in[bk.cur ^ 1], bk.hist * C);
      if ((err = hipGetLastError()) != hipSuccess) return false;
      bk.cur ^= 1; bk.s16 = 0;
    }
    const bool widen = s16_in && !bk.s16;
    const size_t es = (bk.s16 ? 2 : 4) * C, es_in = (s16_in ? 2 : 4) * C;
    const size_t piece = blank_piece_frames();
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      char *b = bk.d_in[bk.cur];
      last_direct = false;
      if (widen) {
        char *tmp = bk.d_in[bk.cur ^ 1];
        if (!upload(tmp, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) return false;
        launch_widen_s16(copy, (const int16_t *)tmp, (float *)(b + bk.hist * es), k * C);
        if ((err = hipGetLastError()) != hipSuccess) return false;
      } else if (!upload(b + bk.hist * es, (const char *)src + off * es_in, k * es_in, on_device, src_ready)) {
        return false;
      }
      direct = direct || last_direct;
      bk.n_in += (long long)k;
      const long long held = (long long)(bk.hist + k);
      // the blocks this piece completes
      const long long done = bk.n_in / BLANK_N;
      if (done > bk.blk_done) {
        if ((size_t)(done - bk.lev0) > bk.lev_rows) { err = hipErrorInvalidValue; return false; }
        if ((err = launch_blank_level(copy, b, bk.s16 != 0, held, bk.i_base, nch, bk.d_lev[bk.lcur] + (size_t)(bk.blk_done - bk.lev0) * C,
                                      done - bk.blk_done, bk.blk_done)) != hipSuccess) return false;
        bk.blk_done = done;
      }
      // the outputs it completes
      const long long y_end = bk.n_in - G;
      if (y_end > bk.y_next) {
        const long long nout = y_end - bk.y_next;
        const size_t nzn = (size_t)blank_blocks_of(bk.y_next, nout) * C;
        if ((size_t)nout > bk.out_frames || nzn > bk.nz_cap) { err = hipErrorInvalidValue; return false; }
        if (bk.nz_used + nzn > bk.nz_cap && !blank_drain()) return false;
        if ((err = launch_blank_apply(copy, b, bk.s16 != 0, held, bk.i_base, nch, bk.d_lev[bk.lcur], bk.blk_done - bk.lev0, bk.lev0,
                                      bk.blank, bk.guard, bk.d_out, nout, bk.y_next, bk.d_nz + bk.nz_used)) != hipSuccess) return false;
        if ((err = hipMemcpyAsync(bk.h_nz + bk.nz_used, bk.d_nz + bk.nz_used, nzn * sizeof(int), hipMemcpyDeviceToHost, copy)) != hipSuccess)
          return false;
        bk.nz_used += nzn;
        bk.y_next = y_end;
        if (!(rs_on ? push_resampled(bk.d_out, (size_t)nout, false, true, nullptr) : push_audio(bk.d_out, (size_t)nout, false, true, nullptr)))
          return false;
      }
      // the level table keeps the last three complete blocks
      const long long lev0n = bk.blk_done > 3 ? bk.blk_done - 3 : 0;
      if (lev0n != bk.lev0) {
        if ((err = hipMemcpyAsync(bk.d_lev[bk.lcur ^ 1], bk.d_lev[bk.lcur] + (size_t)(lev0n - bk.lev0) * C,
                                  (size_t)(bk.blk_done - lev0n) * C * sizeof(float), hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
        bk.lcur ^= 1; bk.lev0 = lev0n;
      }
      // keep what is not yet output with its guard, and the incomplete block
      long long keep = bk.y_next - G < bk.blk_done * BLANK_N ? bk.y_next - G : bk.blk_done * BLANK_N;
      if (keep < bk.i_base) keep = bk.i_base;
      const size_t nh = (size_t)(bk.n_in - keep);
      if (keep != bk.i_base) {   // the tail to the front of the other buffer
        if (nh && (err = hipMemcpyAsync(bk.d_in[bk.cur ^ 1], b + (size_t)(keep - bk.i_base) * es, nh * es,
                                        hipMemcpyDeviceToDevice, copy)) != hipSuccess) return false;
        bk.cur ^= 1; bk.i_base = keep;
      }
      bk.hist = nh;
      off += k;
    }
    last_direct = direct;
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
