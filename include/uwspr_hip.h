/*
 * uwspr_hip.h -- C ABI of the MI355X (gfx950) implementation of gr-uwspr's
 * coarse (FDR) + fine (sync_and_demodulate) search path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * A GNU Radio block shim (gr-uwspr_amd/host/) or any FFI (ctypes, cgo, JNI)
 * binds exactly these symbols.  Each entry point cites the reference interface
 * it replaces (paths relative to the upstream gr-uwspr tree).
 *
 * Conventions
 *   - every function returns 0 (UWSPR_OK) or a negative uwspr_status; nothing
 *     here calls exit() or throws (the reference does: lib/FDR_impl.cc:85-90).
 *   - `where` says whether the bulk pointers of that call are host
 *     (UWSPR_HOST) or device (UWSPR_DEVICE) memory; a call never mixes them.
 *   - frames are interleaved (I,Q) binary32 pairs, `fl` pairs per frame,
 *     frame b at frames + 2*fl*b (or 2*stride*b, uwspr_set_frame_stride): the payload of the PDU that
 *     sliding_window_stream_to_pdu emits (lib/sliding_window_stream_to_pdu_impl.cc:113-135)
 *     narrowed from complex<double> to the gr_complex it was built from (cc:109).
 *   - a context is thread-compatible: one context per host thread; no globals.
 */
#ifndef UWSPR_HIP_H
#define UWSPR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UWSPR_ABI_VERSION 6   /* 2: frame stride, in-place stream views, uwspr_pipe_*, uwspr_dist_*, uwspr_host_threads;
                                 3: uwspr_set_option / uwspr_get_option, uwspr_pipe_set_option, uwspr_pipe_inject_failure,
                                    uwspr_pipe_opts.spare_after_us (was reserved);
                                 4: option "frontend" (the flowgraph's GNU Radio chain is the default front-end),
                                    uwspr_frontend_design replaces uwspr_frontend_taps;
                                 5: uwspr_host_set_ranks (the host's CPU share divided between the ranks of a node);
                                 6: audio streams: uwspr_stream_push_audio, uwspr_pipe_push_audio; multichannel
                                    audio into one pipe: uwspr_pipe_push_audio_channels, uwspr_decode.channel (carved
                                    out of the padding: the record stays 112 bytes); the transmit side: uwspr_wspr_pack,
                                    uwspr_nhash, uwspr_wspr_symbols, uwspr_c2_write, uwspr_tx_baseband, uwspr_tx_render;
                                    moving sources: uwspr_tx_motion, uwspr_tx_baseband_moving, uwspr_tx_render_moving;
                                    known-symbol subtraction: uwspr_sub_item, uwspr_sub_result, uwspr_subtract_batch, the pipe
                                    option "passes", uwspr_decode.pass (carved out of the padding as well);
                                    ordered-statistics decoding: uwspr_osd_result, uwspr_osd_batch, the pipe options "osd" and
                                    "osd_gap", uwspr_decode.osd (the last byte of the padding);
                                    block demodulation: uwspr_block_item, uwspr_blockdemod_batch, the pipe option "block",
                                    uwspr_decode.block (the byte that was _pad0);
                                    audio at other rates: uwspr_resample_design, uwspr_resample_batch, the option
                                    "audio_rate" of contexts and pipes;
                                    impulsive noise: uwspr_blank_batch, uwspr_stream_blank_stats, uwspr_pipe_blank_stats,
                                    the options "blank" and "blank_guard" of contexts and pipes;
                                    transmit at any carrier: uwspr_tx_render_at, uwspr_tx_baseband_at, uwspr_tx_design_at,
                                    the options "tx_cutoff" and "tx_form";
                                    list search: uwspr_deep_result, uwspr_deep_set_list, uwspr_deep_batch,
                                    uwspr_pipe_set_list, the pipe options "deep_min" and "deep_gap", uwspr_decode.osd = 2;
                                    call search (only entry points and a value of uwspr_decode.osd are added, so the
                                    version stays what it is): uwspr_call_result, uwspr_calls_set, uwspr_calls_batch, uwspr_call_message,
                                    uwspr_pipe_set_calls, the pipe options "call_min" and "call_gap", uwspr_decode.osd = 3;
                                    transmit through a medium (entry points and records only, so the version stays):
                                    uwspr_tx_fade, uwspr_tx_impulse, uwspr_tx_render_medium, uwspr_tx_baseband_medium,
                                    uwspr_tx_fade_design;
                                    trajectory fit of a decoded source (entry points and records only, so the version stays):
                                    uwspr_track_traj, uwspr_track_result, uwspr_track_design, uwspr_track_from_slm,
                                    uwspr_track_set, uwspr_track_batch, uwspr_track_record, uwspr_pipe_set_tracks,
                                    uwspr_pipe_collect_tracks;
                                    blind demodulation along straight-line passes (entry points and records only, so the
                                    version stays): uwspr_follow_result, uwspr_follow_set, uwspr_follow_batch,
                                    uwspr_follow_record, uwspr_pipe_set_follow, uwspr_pipe_collect_follows,
                                    uwspr_decode.osd = 4 */

typedef enum {
  UWSPR_OK = 0,
  UWSPR_ERR_PARAM = -1,       /* halfbandwidth > fs/2 (reference exit(-1)s: FDR_impl.cc:85-90) */
  UWSPR_ERR_RANGE = -2,       /* pass band + search reach leaves [0,size) (reference reads OOB) */
  UWSPR_ERR_UNSUPPORTED = -3, /* geometry this build does not implement (spb != 256, ...) */
  UWSPR_ERR_HIP = -4,         /* HIP runtime error, see uwspr_last_error() */
  UWSPR_ERR_NOMEM = -5,
  UWSPR_ERR_ARG = -6,         /* bad pointer / size / ordering in a call */
  UWSPR_ERR_NODEVICE = -7     /* no usable gfx950 device: there is NO CPU fallback */
} uwspr_status;

/* UWSPR_DEVICE_FRAMES (uwspr_fdr_batch, uwspr_demod_batch, uwspr_pipeline_batch, uwspr_demod_resume): the frames are device
 * memory (e.g. what uwspr_stream_take returned), every other pointer of the call is host memory. */
enum { UWSPR_HOST = 0, UWSPR_DEVICE = 1, UWSPR_DEVICE_FRAMES = 2,
       UWSPR_HOST_ASYNC = 3 /* uwspr_stream_push, uwspr_stream_push_audio only: see there */ };
enum { UWSPR_LINEAR = 0, UWSPR_NONLINEAR = 1 };   /* enum Modes, lib/candidate_t.h:36 */

#define UWSPR_NSYM 162      /* symbols per frame */
#define UWSPR_NSLM 125      /* straight-line-model instances, lib/slm.cc:79-87 */
#define UWSPR_NK0 26        /* half-symbol start offsets, FDR_impl.cc:346 */
#define UWSPR_NIFR 5        /* tuned bins if0-2..if0+2, FDR_impl.cc:344 */
#define UWSPR_NJIG 17       /* jiggered shifts, sync_and_demodulate_impl.cc:460 */

/* Constructor arguments of the two blocks:
 * gr::uwspr::FDR::make(fs,fl,spb,maxdrift,maxfreqs,halfbandwidth,cf,threshold)
 *   include/uwspr/FDR.h:49-50
 * gr::uwspr::sync_and_demodulate::make(fs,fl,spb,maxdrift,maxfreqs,cf)
 *   include/uwspr/sync_and_demodulate.h:49  (a subset of the above) */
typedef struct uwspr_params {
  int32_t fs;             /* 375 */
  int32_t fl;             /* 45000 */
  int32_t spb;            /* 256 */
  int32_t maxdrift;       /* 0 */
  int32_t maxfreqs;       /* 200 */
  int32_t halfbandwidth;  /* 10 in the flowgraphs (the GRC default 187 is rejected: UWSPR_ERR_RANGE) */
  int32_t cf;             /* 1500 */
  int32_t threshold;      /* 10 */
} uwspr_params;

/* candidate_t, lib/candidate_t.h:27-50: same 48-byte layout, so a slab of
 * these can be handed to code compiled against the reference header. */
typedef struct uwspr_candidate {
  float freq;
  float snr;
  float drift;     /* unused by the reference as well */
  float sync;
  int32_t shift;
  int32_t m_type;  /* UWSPR_LINEAR / UWSPR_NONLINEAR */
  union {
    struct { float drift; } m_linear;
    struct { double V1, V2; int32_t p1, p2; } m_nonlinear;
  };
} uwspr_candidate;

/* One point of the fine (freq, time-lag, drift) grid: one pass of the
 * ifreq/lag loop body of sync_and_demodulate_impl.cc:163-232. */
typedef struct uwspr_hyp {
  int32_t frame;   /* index into the frames of the call; <0 = skip */
  int32_t m_type;
  float f0;        /* Hz, the f0 of cc:164 */
  int32_t lag;     /* samples, the lag of cc:165 */
  float drift;     /* linear: *drift1 of cc:173 */
  int32_t p1, p2;  /* nonlinear: candidate.m_nonlinear */
  int32_t _pad;
  double V1, V2;
} uwspr_hyp;

/* Result of the per-candidate refinement schedule
 * (sync_and_demodulate_impl.cc:403-482) up to, not including, Fano: every
 * one of the 17 jiggered mode-2 soft-symbol vectors is produced, in the order
 * the reference tries them, with the sync and rms it gates Fano on. */
typedef struct uwspr_demod_out {
  float f1;
  float drift1;
  float sync1;
  int32_t shift1;
  int32_t worth_a_try;
  float jig_sync[UWSPR_NJIG];
  float jig_rms[UWSPR_NJIG];
  int32_t jig_shift[UWSPR_NJIG];
  uint8_t symbols[UWSPR_NJIG][UWSPR_NSYM];
  uint8_t _pad[2];
} uwspr_demod_out;

/* Derived constants (FDR_impl.cc:81-141) and buffer geometry. */
typedef struct uwspr_info {
  int32_t abi_version;
  int32_t size, m, hpbm, n, finpb, noiseidx;
  float df, min_snr;
  int32_t band_lo, band_w;     /* spectrogram columns kept: [band_lo, band_lo+band_w) */
  int32_t cell_hyps;           /* (2*maxdrift+1) + 125 */
  int32_t off_min, off_max;    /* range of ifd-ifr over the whole search */
  int32_t device;
  char device_name[64];
} uwspr_info;

typedef struct uwspr_ctx uwspr_ctx;

/* ---- lifetime ---------------------------------------------------------- */
/* Replaces FDR_impl::FDR_impl / sync_and_demodulate_impl ctor set-up
 * (FDR_impl.cc:48-151, sync_and_demodulate_impl.cc:62-111). */
int uwspr_ctx_create(const uwspr_params *p, int device, uwspr_ctx **out);
void uwspr_ctx_destroy(uwspr_ctx *ctx);
const char *uwspr_last_error(const uwspr_ctx *ctx);
const char *uwspr_status_string(int status);
int uwspr_get_info(const uwspr_ctx *ctx, uwspr_info *info);
/* Run on a caller-owned hipStream_t (NULL = the context's own, non-blocking
 * stream).  All calls are asynchronous on that stream when where==UWSPR_DEVICE
 * and complete before returning when where==UWSPR_HOST.  Device inputs written
 * by work on ANOTHER stream must be complete (or ordered by the caller, e.g. by
 * passing that stream here) before the call: the library adds no cross-stream
 * dependency of its own. */
int uwspr_set_stream(uwspr_ctx *ctx, void *hip_stream);
int uwspr_synchronize(uwspr_ctx *ctx);

/* ---- front-end -------------------------------------- */
/* 12 kS/s real audio -> fl complex samples at 375 S/s.  In the reference this is the flowgraph's chain of GNU Radio
 * blocks (examples/WaveFilePlusNoiseDecode.grc): float_to_complex (:527) -> freq_xlating_fft_filter_ccc with
 * firdes.band_pass(1, 12000, 1490, 1510, 10, WIN_HAMMING) real taps at centre 0 (:303-352, 840-893) ->
 * freq_xlating_fft_filter_ccc with firdes.low_pass(1, 12000, 1510, 10, WIN_HAMMING) at centre 1500 Hz (:358-400,
 * 903-956) -> rational_resampler_ccc(1, 32) with its own Kaiser design (:1767-1808).
 *   option "frontend" = 0 (UWSPR_FRONTEND_GRC, default): that chain, its taps designed from GNU Radio 3.7's published
 *     formulas and folded into ONE 6831-tap complex polyphase decimator (every stage is linear, the mixer's period
 *     divides the decimation): y[m] = sum_k g[k] x[32 m - k];
 *   option "frontend" = 1 (UWSPR_FRONTEND_COMPACT): mix by -1500 Hz, 1025-tap Hamming low-pass (100 Hz), decimate:
 *     y[m] = sum_k g[k] x[32 m + 512 - k] -- a sixth of the arithmetic, not the reference's pass band.
 * GNU Radio is third-party, unpinned and absent here: **parity unpinned**; oracle/frontend_grc.py restates the chain
 * stage by stage in binary64.  audio [B][nin] (zero outside the record), frames_out [B][fl] (I,Q) pairs.
 * uwspr_frontend_design: stage 0 = the composite complex taps g (cap counts (re, im) pairs) and *delay = D of
 * y[m] = sum_k g[k] x[32 m + D - k]; stages 1, 2, 3 (grc mode) = the band-pass, low-pass and resampler designs
 * (real taps).  Returns the tap count (taps may be NULL), < 0 on a bad mode / stage.
 *
 * Another carrier.  The flowgraph's two variables are options of the context: "carrier" (Center_Frequency, integer Hz,
 * default 1500) and "frontend_hbw" (Half_Bandwidth, Hz, default 10).  The grc mode designs
 *   h1 = band_pass(1, 12000, fc - hb, fc + hb, 10, HAMMING),
 *   h2 = low_pass(1, 12000, fc + hb, 10, HAMMING) rotated by e^{+j 2 pi fc k / 12000} and rounded to binary32 pairs,
 *   h3 = the resampler's Kaiser design rotated in exact arithmetic,      g = h1 * rot(h2) * rot(h3)
 * (6831 taps whatever fc and hb are: the tap counts follow the 10 Hz transition width); the compact mode mixes the same
 * 1025-tap low-pass by -fc and has no hb.  fc k is reduced mod 12000 in integers before any cos / sin, and a multiple of
 * pi/4 takes the exact octant values, so (1500, 10) gives the taps it always gave, byte for byte.
 * Allowed: 1 <= hb <= 150 (the / 32 resampler passes 0.4 x 375 Hz) and hb + 20 <= fc <= 6000 - hb - 20 (the compact
 * mode: 20 <= fc <= 5980); anything else is UWSPR_ERR_ARG.
 * The rotator.  At the decimated instants the chain's mixer is e^{-j 2 pi fc m / 375}: the identity exactly when 375
 * divides fc (1500 needs none), otherwise one of 375 values.  uwspr_frontend_rotator returns the table K0 uses,
 *   rot[i] = ((float)cos(2 pi i / 375), (float)(-sin(2 pi i / 375))),  i = 0 .. 374, computed in binary64,
 * and output m of a stream (m its 64-bit stream index) is, with s the sum K0 forms at any carrier (16 chains of fused
 * multiply-adds, added in wavefront order) and (c, d) = rot[((fc mod 375) (m mod 375)) mod 375],
 *   y.re = fmaf(s.re, c, -(s.im d)),   y.im = fmaf(s.re, d, s.im c)      -- this one order;
 * when fc mod 375 == 0 no product is made and y is s's bytes, NaN and inf included.
 * Both options are latched by a stream's first audio push like "frontend" (a change while it runs is UWSPR_ERR_ARG and
 * leaves the stream as it was); uwspr_frontend_batch reads them at every call.  With (1500, 10) nothing new runs or is
 * allocated.  The transmitter follows ("Transmit at another carrier" below).  Not built: carriers are integer Hz, and uwspr_params.cf (the SLM Doppler
 * scale) stays the caller's: one per context or pipe, to be set to the carrier when there is one carrier.
 * uwspr_frontend_design_at: uwspr_frontend_design at (centre_hz, half_bw_hz). */
enum { UWSPR_FRONTEND_GRC = 0, UWSPR_FRONTEND_COMPACT = 1 };
#define UWSPR_CARRIER_DEFAULT 1500
#define UWSPR_FRONTEND_HBW_DEFAULT 10
int uwspr_frontend_design_at(int mode, int centre_hz, int half_bw_hz, int stage, double *taps, int cap, int *delay);
int uwspr_frontend_rotator(float *out750);
int uwspr_frontend_batch(uwspr_ctx *ctx, const float *audio, int B, int nin, int where,
                         float *frames_out);
int uwspr_frontend_design(int mode, int stage, double *taps, int cap, int *delay);

/* ---- overlap-aware stream ingest ----------------------- */
/* sliding_window_stream_to_pdu::work (lib/sliding_window_stream_to_pdu_impl.cc:97-138) cuts the
 * 375 S/s stream into frames of fl samples that start every hop = shift*fs = 3375 samples: 41625 of
 * a frame's 45000 samples are its predecessor's.  Handing whole frames to the calls below uploads
 * every sample 13 times; through this interface every sample crosses PCIe ONCE, on a copy stream of
 * its own (uploads overlap the search kernels of the batches before), and the frames are read where
 * they lie:
 *   uwspr_stream_open(ctx, hop, max_frames)        hop in samples; at most max_frames per take
 *   uwspr_stream_push(ctx, iq, n, where, &nready)  append n (I,Q) pairs; nready = complete frames waiting.
 *       where = UWSPR_HOST: on return iq may be reused (pageable memory is staged; a page-locked buffer
 *       is read by the DMA itself and the call waits for that transfer -- not for any kernel);
 *       UWSPR_HOST_ASYNC: page-locked iq is only enqueued and must stay unmodified until
 *       uwspr_stream_wait_uploads returns; UWSPR_DEVICE: iq is device memory written by work on the
 *       context's stream.
 *   uwspr_stream_take_view(ctx, k, &frames, &stride, &pos)   the next k frames IN PLACE: frame j starts
 *       at frames + 2*stride*j floats (stride = hop; the frames overlap in memory as they do in the
 *       stream), valid until the next take; pos = stream index of the first one's first sample;
 *       consumes k*hop samples.  Use with uwspr_set_frame_stride(ctx, stride) and where = UWSPR_DEVICE
 *       or UWSPR_DEVICE_FRAMES; the kernels reading them must be enqueued before the next take.
 *   uwspr_stream_take(ctx, k, dev_dst, &frames, &pos)        the same frames COPIED out as contiguous
 *       [k][fl] pairs (dev_dst, or NULL = a buffer of the context, valid until the next take) for
 *       consumers that keep frames beyond the next take (the block mirror's FDR -> sync hand-over).
 *   uwspr_stream_reset(ctx, pos)                   drop what is buffered; the next sample pushed has index pos
 * Frame k of the stream is bit for bit the frame the reference's PDU k carries.
 *
 * uwspr_set_frame_stride(ctx, s): the calls that follow read frame b of their `frames` argument at
 * frames + 2*s*b floats instead of 2*fl*b (s = 0 restores fl).  With where = UWSPR_HOST the span
 * (B-1)*s + fl is uploaded once, so a host buffer holding a stretch of the stream (s = hop) is also
 * ingested without repeats.  Applies to every entry point that takes frames. */
int uwspr_set_frame_stride(uwspr_ctx *ctx, int stride_samples);
int uwspr_stream_open(uwspr_ctx *ctx, int hop, int max_frames);
int uwspr_stream_push(uwspr_ctx *ctx, const float *iq, int nsamples, int where, int *nready);
int uwspr_stream_wait_uploads(uwspr_ctx *ctx);
int uwspr_stream_take_view(uwspr_ctx *ctx, int nframes, const float **frames, int *stride, long long *first_pos);
int uwspr_stream_take(uwspr_ctx *ctx, int nframes, float *dev_dst, const float **frames, long long *first_pos);
int uwspr_stream_reset(uwspr_ctx *ctx, long long pos);
/* Audio streams: the receiver flowgraph's whole front half (examples/AudioSourceDecode.grc: audio_source at 12 kS/s
 * (:376) -> float_to_complex -> band-pass -> low-pass -> rational_resampler /32 (:1804) ->
 * sliding_window_stream_to_pdu (:1973)) on a pushed stream of real 12 kS/s samples.  Each push uploads the new samples
 * behind the front-end's history on the stream's copy stream and runs the front-end (option "frontend", as
 * uwspr_frontend_batch) there for the outputs that just became complete, straight into the stream buffer:
 *     stream sample m = y[m] = sum_k g[k] x[32 m + D - k]     (audio index 32 m <-> stream index m; D = 0 or 512)
 * x being the pushed audio (x[0] = the first sample after uwspr_stream_open; zero before it).  y[m] is produced as soon
 * as x[32 m + D] has been pushed: no flush, no padding at the live end.  Frames, takes and first_pos keep their
 * meaning: frame k's audio time is first_pos / 375 s.  uwspr_stream_reset(ctx, pos) zeroes the history and makes the
 * next pushed sample x[32 pos].  The first push after open / reset makes the stream an audio or an (I,Q) stream; a
 * push of the other kind or a change of option "frontend" while it runs fail that call with UWSPR_ERR_ARG (the
 * stream is unharmed).  where: as for uwspr_stream_push.  int16 samples count as s / 32768 (GNU Radio's
 * wavfile_source), exactly, so pushes of either format may follow each other: the outputs are the same bytes. */
enum { UWSPR_AUDIO_F32 = 0, UWSPR_AUDIO_S16 = 1 };
int uwspr_stream_push_audio(uwspr_ctx *ctx, const void *audio, int nsamples, int format, int where, int *nready);
/* ---- audio at other rates: a rational resampler ahead of the front-end (K11) ------------------------------------
 * Sound cards and recorders deliver 44.1, 48, 96 or 192 kS/s (loggers 8, 16, 32 kS/s), the front-end takes 12 kS/s.
 * A rate R (S/s) is supported when 8000 <= R <= 192000 and, with g = gcd(R, 12000), L = 12000 / g, M = R / g, L <= 160:
 * 8000, 9600, 10000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400 and 192000 among
 * them.  R = 12000 means "no resampler" (the design call reports the identity: one tap 1, L = M = T = 1, D = 0).
 * The reference has no such stage; this is the project's own definition, and it is exact:
 *   Prototype low-pass, designed on the host in binary64 at the rate F = L R: pass edge fp = 2400 Hz, stop edge
 *   fs = min(R, 12000) - 2400 Hz, cut-off fc = (fp + fs) / 2; Kaiser window with A = 100 dB, beta = 0.1102 (A - 8.7);
 *   dw = 2 pi (fs - fp) / F, N0 = ceil((A - 8) / (2.285 dw)) + 1, N = N0 rounded up to odd, T = ceil(N / L) taps per
 *   phase (taps N .. T L - 1 are zero);
 *     h[k] = (2 fc / F) sinc((2 fc / F) (k - (N - 1) / 2)) w[k],  sinc(x) = sin(pi x) / (pi x),
 *     w[k] = I0(beta sqrt(1 - (2 k / (N - 1) - 1)^2)) / I0(beta),
 *   scaled so that sum h = L; delay D = (N - 1) / 2.  The taps are rounded to binary32 once: hp[p][t] = (float) h[p + t L].
 *   Output j (12 kS/s index; audio time j / 12000 s exactly, the delay being compensated):
 *     q = j M + D (64-bit integer), i0 = floor(q / L), p = q mod L,
 *     acc = 0; for t = T - 1 .. 0: acc = fmaf(hp[p][t], x[i0 - t], acc)      (binary32; y[j] = acc)
 *   x being zero before the first sample (and, in the batch call, behind the last), int16 samples counting as s / 32768
 *   exactly.  y[j] is complete as soon as x[i0] has been pushed.  One owner and one order per output: its bytes do
 *   not depend on the batch, the launch, the channel count or the cuts of a stream.
 * Pass band: 0 - 2400 Hz within 2.2e-5 of unity, stop band from fs on at -97.6 dB or below, for every rate above
 * (T = 12 at 11025 S/s .. 173 at 192000 S/s, L T <= 1920).  0 - 2400 Hz is what every "frontend" mode reads (1490 -
 * 1510 Hz, or +- 100 Hz around 1500 Hz in the compact mode): this is NOT a general-purpose 6 kHz audio resampler.
 *   uwspr_resample_design    the design: returns the tap count N (taps may be NULL; at most cap are written) and
 *                            L, M, T, D through the pointers that are not NULL; < 0 for an unsupported rate.
 *   uwspr_resample_batch     a whole record: audio [nin][nchannels] interleaved (format UWSPR_AUDIO_F32 / _S16,
 *                            1..UWSPR_PIPE_MAX_CHANNELS channels), zero outside it -> out [nout][nchannels] float,
 *                            outputs 0 .. nout - 1.  where = UWSPR_HOST (complete on return) or UWSPR_DEVICE
 *                            (asynchronous on the context's stream).
 * Streams: option "audio_rate" (uwspr_set_option; default 12000) is the rate of what uwspr_stream_push_audio is given.
 * It is latched by the first audio push after open / reset, as "frontend" is; a change while the stream runs fails that
 * push with UWSPR_ERR_ARG (the stream is unharmed: set the old rate again and go on), an unsupported value fails
 * uwspr_set_option with UWSPR_ERR_ARG.  At another rate than 12000 a push uploads the new frames behind the resampler's
 * own history (at most T - 1 frames in the pushed format, widened once when the formats mix), runs K11 on the copy
 * stream for the outputs that became complete and hands those 12 kS/s float frames to the front-end on the same
 * stream, exactly as a device push of them would.  After open or uwspr_stream_reset(ctx, pos) the next pushed sample
 * sits at audio time pos / 375 s, the resampler's counters restart at 0 with a zero history, and its output j is 12 kS/s
 * sample 32 pos + j of the front-end; first_pos / 375 stays audio time in seconds.  The buffer-full check counts the
 * 12 kS/s samples a push will produce.  With "audio_rate" = 12000 K11 never runs, none of its buffers exists, an int16
 * stream stays int16, and every byte is what it was before this option existed.
 * Device memory the resampler adds to a stream, made by the first push at another rate: the taps (L (T | 1) floats),
 * two input buffers of (T + P) * nchannels samples (4 bytes) with P = min(Q, (Q - 2) M / L) frames and Q = 4 Mi /
 * nchannels, and one output buffer of Q * nchannels floats: at most 3 x 16 MB. */
int uwspr_resample_design(int rate, double *taps, int cap, int *L, int *M, int *T, int *delay);
int uwspr_resample_batch(uwspr_ctx *ctx, const void *audio, long long nin, int nchannels, int format, int rate, int where,
                         float *out, long long nout);
/* ---- impulsive noise: a median-gated blanker ahead of the resampler and the front-end (K12) ------------------------
 * The underwater channel is impulsive (snapping shrimp, clicks, mooring and electrical spikes).  K0 reads +-10 Hz, so
 * its impulse response is about half a second long: a click of 0.1 ms that reaches it is smeared over that half second
 * and its whole energy lands in the band, while zeroing the click ahead of K0 costs 0.1 ms of signal.  The reference
 * has no such stage; this is the project's own definition, and it is exact.  It is OFF by default; with it off nothing
 * of it runs or is allocated and every byte is what it was before the option existed.
 *   Audio is taken at the rate it is pushed at, ahead of K11 and K0, each channel on its own, int16 samples counting
 *   as s / 32768 exactly; the output is always float32.  Let N = UWSPR_BLANK_BLOCK = 4096.  Block b holds audio indices
 *   b N .. b N + N - 1, counted from the stream's first sample after open / reset, or from the start of the record in
 *   the batch call.
 *   Level of a COMPLETE block: with u(i) the bit pattern of x[i] with the sign cleared, as an unsigned 32-bit integer,
 *     med(b) = the value of rank N / 2 - 1 (0-based, ascending) among the N patterns of block b
 *   (a selection: exact, ties need no rule).
 *   Threshold: the samples of block b >= 1 use
 *     thr(b) = fl32(fl32((float) blank * med(b - 1)) * 0.25f)      (two binary32 multiplies, subnormals kept).
 *   Block 0 has no threshold, nor has a block whose med(b - 1) has pattern 0 or >= 0x7f800000 (infinity, NaN).
 *   Causal: a sample never waits for audio behind it, except for the guard.
 *   Flag: sample i is flagged iff its block has a threshold and u(i) > bits(thr(block(i))) as unsigned integers (so a
 *   NaN sample in a block with a threshold is flagged; in a block without one, nothing is).
 *   Output: y[i] = +0.0f if any j with |j - i| <= G is flagged, else x[i] unchanged (the float value of an int16
 *   sample).  G is the guard; j is limited to samples that exist (j >= 0; in the batch call j < nin); the guard crosses
 *   block edges and each j is judged by its OWN block's threshold.
 *   Completeness: in a stream y[i] is complete as soon as x[i + G] has been pushed.  Like K0 there is no flush and no
 *   padding: the last G samples of a stream that ends are never produced.  A stream's bytes do not depend on how the
 *   audio was cut, on the sample format of a piece or on the channel count, and on every index both produce they are
 *   the batch call's.
 * What the design costs: a level step of more than blank / 4 between neighbouring blocks is blanked for up to one
 * block (0.34 s at 12 kS/s) -- a signal that switches on is judged by the silence before it -- and block 0 passes
 * untouched (the first 0.34 s of a stream are not protected).
 * Options: "blank" is the threshold in quarters of the median: 0 = off (default), 4 .. 1024 = on (24 means 6 x the
 * median of |x|, about 4.05 sigma of Gaussian noise); "blank_guard" is G, 0 .. 64, default 2.  Anything else is
 * UWSPR_ERR_ARG.  Both are options of the context (uwspr_set_option) for uwspr_stream_push_audio, and the pipe's own
 * in uwspr_pipe_set_option, as "audio_rate" is.  Both are latched by the first audio push after open / reset; a change
 * while the stream runs fails that push with UWSPR_ERR_ARG (the stream is unharmed: set the old values again and go on).
 * With "blank" != 0 a push uploads the new frames behind the blanker's own history (what is not yet output, its guard
 * and the incomplete block: at most N + 2 G frames), runs the level kernel for the blocks the push completes and the
 * apply kernel for the outputs it completes on the copy stream, and hands those float frames to the resampler or the
 * front-end on the same stream, exactly as a device push of them would; the buffer-full check counts the samples a push
 * will complete.  Device memory it adds to a stream, made by the first such push: two input buffers of (N + 2 G + Q) *
 * nchannels samples (4 bytes), one output buffer of Q * nchannels floats (Q = 4 Mi / nchannels frames), and tables of a
 * few KB: 3 x 16 MB and at most 2 x 1.1 MB of history.
 *   uwspr_blank_batch         a whole record: audio [nin][nchannels] interleaved (format UWSPR_AUDIO_F32 / _S16,
 *                             1..UWSPR_PIPE_MAX_CHANNELS channels), blank 4 .. 1024, guard 0 .. 64 -> out [nin][nchannels]
 *                             float; med [nblocks][nchannels] float (nblocks = ceil(nin / N)): the level of every
 *                             COMPLETE block, 0 for a trailing partial one; nzero [nblocks][nchannels] int32: the
 *                             outputs of that block set to zero.  med and nzero may be NULL.  where = UWSPR_HOST
 *                             (complete on return) or UWSPR_DEVICE (asynchronous on the context's stream), as in
 *                             uwspr_resample_batch.
 *   uwspr_stream_blank_stats  per channel (at most cap of them): the samples output and the samples set to zero since
 *                             open / reset, summed on the host from the per-block counts (waits for the copy
 *                             stream); zeros when no blanker runs.  Returns the channel count. */
#define UWSPR_BLANK_BLOCK 4096
int uwspr_blank_batch(uwspr_ctx *ctx, const void *audio, long long nin, int nchannels, int format, int where, int blank,
                      int guard, float *out, float *med, int *nzero);
int uwspr_stream_blank_stats(uwspr_ctx *ctx, long long *samples, long long *zeroed, int cap);
/* device memory for callers without a HIP runtime of their own (the block mirror's frame hand-over) */
int uwspr_device_alloc(size_t bytes, void **ptr);
void uwspr_device_free(void *ptr);
/* Page-locked host memory for frames handed over as host pointers: the upload is then one DMA at the
 * link's rate instead of the runtime's staged copy of pageable memory (any page-locked buffer is
 * recognised, whoever allocated it). */
int uwspr_host_alloc(size_t bytes, void **ptr);
void uwspr_host_free(void *ptr);

/* ---- coarse search: FDR_impl::transform, FDR_impl.cc:214-456 ------------ */
/* cands: [B][maxfreqs] records; npk: [B].  Same candidate order, fields and
 * selection rule (running-best, FDR_impl.cc:360,392) as the reference. */
int uwspr_fdr_batch(uwspr_ctx *ctx, const float *frames, int B, int where,
                    uwspr_candidate *cands, int32_t *npk);

/* Inspection of the intermediates of the LAST uwspr_fdr_batch call (host
 * pointers; any may be NULL):
 *   ps_band [B][n][band_w]   FDR_impl.cc:246-253 (columns band_lo..)
 *   psavg   [B][band_w]      cc:257-263
 *   smraw   [B][finpb]       cc:268-275
 *   smspec  [B][finpb]       cc:287-291
 *   noise   [B]              cc:285 */
int uwspr_fdr_read_spectrum(uwspr_ctx *ctx, int B, float *ps_band, float *psavg,
                            float *smraw, float *smspec, float *noise);
/* When enabled, the next uwspr_fdr_batch also keeps every hypothesis metric:
 * grid [B][ncand_cap][5][26][cell_hyps] (cc:357,390), read back with
 * uwspr_fdr_read_syncgrid.  Off by default: it is 65 KB per candidate, and the coarse search then has to
 * evaluate every hypothesis instead of only those that can still be accepted (same candidates either way). */
int uwspr_fdr_keep_syncgrid(uwspr_ctx *ctx, int ncand_cap);
int uwspr_fdr_read_syncgrid(uwspr_ctx *ctx, int B, float *grid);

/* ---- fine sweep: core of sync_and_demodulate, cc:126-256 ---------------- */
/* One metric per (freq, lag, drift) hypothesis, in any order (grouping them by
 * frame keeps a frame's samples in L2).  sync: [H]; symbols: [H][162] soft
 * symbols (cc:240-254) or NULL to skip them (modes 0/1). */
int uwspr_sync_sweep(uwspr_ctx *ctx, const float *frames, int B,
                     const uwspr_hyp *hyps, int H, int where, float *sync,
                     uint8_t *symbols);

/* The (freq, drift, lag) grid sweep of BASELINE configs[2].  Every frame b has a
 * centre (a candidate record: freq, shift, m_type and its drift / SLM parameters)
 * and the same offsets are applied around every centre:
 *     f0    = centre.freq  + df[i]            (binary32 add, as cc:164 forms f0)
 *     drift = centre.m_linear.drift + ddrift[j]   (binary32 add; linear centres only)
 *     lag   = centre.shift + dlag[k]
 * One grid point = one hypothesis of uwspr_sync_sweep (same arithmetic, bit-identical
 * results); the grid form lets the kernel keep each symbol window on chip for all
 * of a frame's points and share the tone phasors between points that differ only in
 * lag.  df/ddrift/dlag are host arrays (nf, ndrift <= 32); centres [B], sync
 * [B][nf][ndrift][nlag], symbols [B][nf][ndrift][nlag][162] (or NULL) per `where`. */
int uwspr_sync_grid(uwspr_ctx *ctx, const float *frames, int B, int where,
                    const uwspr_candidate *centres, int nf, const float *df, int ndrift,
                    const float *ddrift, int nlag, const int32_t *dlag, float *sync,
                    uint8_t *symbols);

/* Argument-for-argument batch form of sync_and_demodulate() (cc:126-131):
 * one call = one invocation of the reference function; results are what it
 * writes back through sync/shift1/f1 (and symbols in mode 2).  Host pointers
 * for the call records; frames per `where`. */
typedef struct uwspr_sync_call {
  int32_t frame;
  uwspr_candidate candidate;
  float f1;
  int32_t ifmin, ifmax;
  float fstep;
  int32_t shift1, lagmin, lagmax, lagstep;
  float drift1;
  int32_t symfac;
  int32_t mode;
} uwspr_sync_call;
typedef struct uwspr_sync_result {
  float sync;
  int32_t shift1;
  float f1;
  uint8_t symbols[UWSPR_NSYM];
  uint8_t _pad[2];
} uwspr_sync_result;
int uwspr_sync_and_demodulate_batch(uwspr_ctx *ctx, const float *frames, int B,
                                    int where, const uwspr_sync_call *calls,
                                    int ncalls, uwspr_sync_result *results);

/* ---- refinement schedule: sync_and_demodulate_impl::demodulate ---------- */
/* cands [B][cand_stride], npk [B] as produced by uwspr_fdr_batch; the first
 * min(npk[b], max_per_frame) candidates of each frame are refined.
 * out [B][max_per_frame]; entries past npk[b] are zeroed. */
int uwspr_demod_batch(uwspr_ctx *ctx, const float *frames, int B, int where,
                      const uwspr_candidate *cands, const int32_t *npk,
                      int cand_stride, int max_per_frame, uwspr_demod_out *out);

/* Lazy jiggered shifts.  The reference stops at the first of its up to 17 mode-2 tries that
 * decodes (sync_and_demodulate_impl.cc:457-490); by default this library produces all 17 soft-symbol
 * vectors before the host sees any.  uwspr_set_tries(ctx, k), k < 17: the schedule calls that follow
 * produce only tries idt < k (the other entries of uwspr_demod_out are zero, so uwspr_decode_candidate
 * skips them) and keep what is needed to produce the rest later.  Try 0 repeats the hypothesis that won
 * the last stage: with the fused schedule kernel k = 1 costs no correlation at all, the staged form
 * runs its last stage on the k wanted tries only.  Both forms are resumed by the fused kernel.
 * uwspr_demod_resume(ctx, frames, B, where, need, max_per_frame, out): for the slots b*max_per_frame+j
 * with need[...] != 0 of the LAST schedule call (same frames, B, max_per_frame) all 17 tries are
 * produced, byte-identical to what a k = 17 call gives; the other records are left alone.
 * where == UWSPR_HOST (or UWSPR_DEVICE_FRAMES): need is host memory and `out` receives all B*max_per_frame records;
 * UWSPR_DEVICE: need and out are device memory, out being the buffer the first call wrote. */
int uwspr_set_tries(uwspr_ctx *ctx, int ntries);

/* Options of a context.  The reference's blocks have no run-time switches (their constants are
 * hard-coded); these choose between forms of THIS implementation that give the same
 * bytes -- except "fast_search":
 *   "sched"          1 (default): the whole S0..S5 schedule of a candidate in one workgroup; 0: one launch
 *                    per stage (what uwspr_pipe_* uses from three lanes up)
 *   "stage_kernels"  staged form: 1 (default) packed / ring / pair kernels, 0 the flat kernel for
 *                    every stage -- an independent form the equivalence tests compare the others with
 *   "reuse"          1 (default): the hypothesis that repeats the previous stage's winner
 *                    (sync_and_demodulate_impl.cc:416-452 evaluate it again and get the same number) is skipped
 *   "phasor_tables"  1 (default): drift-free stages read the tone phasors of cc:186-199 from per-slot tables
 *   "fast_search"    0 (default).  1: stages S0..S4 with fused multiply-adds and wavefront shuffle-tree sums --
 *                    NOT the reference's arithmetic: sync metrics agree to ~1e-6 relative (1e-5 is BASELINE's
 *                    tolerance), integer results and soft symbols were identical on every frame tried
 *                    (tests/test_gpu_fast_search.py); stage 5 -- the soft symbols -- and every other entry
 *                    point stay exact.  Staged form only (it sets "sched" 0).
 * Further names ("k4_t", "k5_lanes", "sched_stamps", "dist_force_comm", and the
 * creation-time "k1_rows", "k3_tile") are diagnostics: DESIGN.md section 9.  The one environment
 * variable the library reads, UWSPR_OPTIONS="name=value,...", presets options for every context the process
 * creates.  Unknown names: UWSPR_ERR_ARG. */
int uwspr_set_option(uwspr_ctx *ctx, const char *name, int value);
int uwspr_get_option(uwspr_ctx *ctx, const char *name, int *value);

int uwspr_demod_resume(uwspr_ctx *ctx, const float *frames, int B, int where, const uint8_t *need,
                       int max_per_frame, uwspr_demod_out *out);

/* FDR followed by the schedule with candidates kept in HBM in between (the
 * FDR -> sync_and_demodulate PDU hop of the flowgraph, examples/
 * WaveFilePlusNoiseDecode.grc).  Any output pointer may be NULL. */
int uwspr_pipeline_batch(uwspr_ctx *ctx, const float *frames, int B, int where,
                         int max_per_frame, uwspr_candidate *cands,
                         int32_t *npk, uwspr_demod_out *out);

/* Multi-GPU hand-off: packs the results of the LAST uwspr_pipeline_batch into
 * one fixed-size slab per frame, ready for a gather to the root rank:
 *   int32 npk, 12 pad bytes | candidate_t[K] (first K candidates, zero-filled past npk)
 *   | float f1, drift1, sync1; int32 shift1 of the frame's top candidate
 * = 32 + 48*K bytes per frame; slabs: [B][32+48K]. */
int uwspr_pack_slabs(uwspr_ctx *ctx, int B, int K, void *slabs, int where);
/* The same slabs without a launch of their own: the NEXT uwspr_pipeline_batch (one shot) also writes its frames' slabs
 * to slabs_device ([B][32+48K] bytes in device memory) -- from the schedule's last kernel where the schedule form has
 * one, else with the packing kernel behind it.  slabs_device = NULL cancels. */
int uwspr_pipeline_slabs(uwspr_ctx *ctx, int K, void *slabs_device);

/* ---- multi-GPU: the final gather over RCCL --------------------------------------- */
/* One process per GPU, frames sharded round-robin (global frame b on rank b mod G), no data-path
 * collective; the one exchange is the gather of the uwspr_pack_slabs output to the root rank:
 * point-to-point RCCL transfers (ncclSend / ncclRecv in one group), each peer -> root over its own xGMI
 * link.  librccl is loaded on first use; world == 1 needs no RCCL at all (the gather is a copy).
 *   uwspr_dist_unique_id(id)             rank 0: 128 bytes to hand to every rank out of band (ncclGetUniqueId)
 *   uwspr_dist_init(ctx, rank, world, id)  collective: every rank calls it with the same id
 *   uwspr_dist_gather(ctx, send, bytes, recv, root, UWSPR_DEVICE)
 *        every rank contributes `bytes` bytes of device memory (equal on all ranks: pad the shards);
 *        the root receives world * bytes in rank order (recv may be NULL elsewhere).  Asynchronous on
 *        the context's stream, after whatever produced `send` there.
 *   uwspr_dist_finalize(ctx)             (also done by uwspr_ctx_destroy) */
int uwspr_dist_unique_id(void *id128);
int uwspr_dist_init(uwspr_ctx *ctx, int rank, int world, const void *id128);
int uwspr_dist_gather(uwspr_ctx *ctx, const void *send, size_t bytes, void *recv, int root, int where);
int uwspr_dist_finalize(uwspr_ctx *ctx);

/* ---- pipelined end-to-end decoder ---------------------------------------------------------- */
/* The whole receive chain of examples/WaveFilePlusNoiseDecode.grc behind one object:
 *   sliding_window_stream_to_pdu (lib/sliding_window_stream_to_pdu_impl.cc:97-138)  -> frames in place
 *   FDR::transform               (lib/FDR_impl.cc:214-456)                          -> candidates
 *   sync_and_demodulate::demodulate (lib/sync_and_demodulate_impl.cc:315-534)       -> 7-byte messages
 * with the stages of CONSECUTIVE batches overlapped: page-locked samples go up on a copy stream while
 * the batches before are searched; the schedule produces only the first jiggered shift
 * (uwspr_set_tries(1): the reference stops at its first decoding try, cc:457-490); Fano runs on a
 * persistent pool of host threads under the kernels of the next batch; the candidates whose first
 * try did not decode are resumed on the GPU (uwspr_demod_resume) and tried again.  Results are
 * byte-for-byte those of the sequential calls (uwspr_pipeline_batch with all 17 tries +
 * uwspr_decode_batch), in frame order.  One producer thread drives a pipe. */
typedef struct uwspr_pipe uwspr_pipe;
typedef struct uwspr_pipe_opts {
  int32_t hop;            /* samples between frame starts (shift*fs = 3375); pushed streams only */
  int32_t batch_frames;   /* frames per GPU batch (256) */
  int32_t max_per_frame;  /* candidates refined per frame (cc:389 refines all npk; 1 = the strongest) */
  int32_t lanes;          /* most batches in flight, each with its own context (0: 9).  The first three have a HIP stream
                             each and take the batches in turn; the others share those streams and are spares, opened
                             only while every one of the three is busy and a host tail (Fano time-outs) has lasted > 2.5 ms */
  int32_t host_threads;   /* Fano threads (0: uwspr_host_threads() - 2, leaving the producer and the HIP runtime a core each) */
  int32_t eager;          /* 1: all 17 tries in the first pass, no resume (A/B against the lazy flow) */
  int32_t sched_form;     /* 0: staged launches from 3 lanes up, the fused kernel below (a "sched" entry of UWSPR_OPTIONS overrides), 1: fused, 2: staged */
  int32_t spare_after_us; /* a spare lane opens when every base lane is busy and a host tail has lasted this long (0: 2500) */
} uwspr_pipe_opts;
/* one refined candidate (j < min(npk, max_per_frame)) of one frame */
typedef struct uwspr_decode {
  int64_t frame;          /* running index of the frame in submission order */
  int64_t stream_pos;     /* index of its first sample in the pushed stream (-1: submitted frames) */
  int32_t cand, npk;      /* rank of this candidate, candidates found in the frame */
  uwspr_candidate coarse; /* the FDR record (candidate_t) */
  float f1, drift1, sync1;
  int32_t shift1, worth_a_try;
  int32_t decoded;        /* 1: message holds the 7 bytes sync_and_demodulate publishes (cc:528-530) */
  int32_t idt;            /* the jiggered try that decoded (-1: none) */
  int8_t message[7];
  uint8_t block;          /* 2, 3: Fano timed out on every gated try and the soft symbols of that block length decoded (option "block"); 0 otherwise */
  int16_t channel;        /* the audio channel of a multichannel pipe (uwspr_pipe_push_audio_channels); 0 otherwise.  With n > 1
                             carriers (uwspr_pipe_set_carriers): the plane index channel * n + carrier index */
  uint8_t pass;           /* 1: found by the second pass (option "passes" = 2), in the frame with its decoded signals taken out; 0 otherwise */
  uint8_t osd;            /* 1: ordered-statistics decoding, 2: list search, 3: call search -- Fano timed out on every gated try and K9
                             (option "osd"), K13 (uwspr_pipe_set_list) or K14 (uwspr_pipe_set_calls) gave the message; 4: Fano timed
                             out on every gated try and decoded K16's soft symbols along a straight-line pass
                             (uwspr_pipe_set_follow); 0 otherwise */
} uwspr_decode;
typedef struct uwspr_pipe_stats {
  int64_t frames, batches, candidates, decoded, resumed;   /* resumed: records whose other tries were produced */
  int64_t fano_calls, fano_timeouts;                       /* tries that passed the gates (cc:470) / ran to the cycle limit */
  double gpu_wait_s, fano_s, resume_s;                     /* coordinator thread: where its time went */
} uwspr_pipe_stats;
int uwspr_pipe_open(const uwspr_params *p, int device, const uwspr_pipe_opts *o, uwspr_pipe **out);
void uwspr_pipe_close(uwspr_pipe *pipe);
const char *uwspr_pipe_last_error(const uwspr_pipe *pipe);
/* A page-locked buffer for the next nsamples (I,Q) pairs of the stream (at most batch_frames*hop): fill it,
 * then commit.  Blocks only while every staging buffer still has its upload in flight. */
int uwspr_pipe_acquire(uwspr_pipe *pipe, int nsamples, float **iq);
int uwspr_pipe_commit(uwspr_pipe *pipe, int nsamples);
/* acquire + memcpy + commit for samples that live elsewhere */
int uwspr_pipe_push(uwspr_pipe *pipe, const float *iq, int nsamples);
/* The same for 12 kS/s real audio (format UWSPR_AUDIO_F32 / UWSPR_AUDIO_S16; examples/AudioSourceDecode.grc's chain
 * from audio_source (:376) on): pieces of any length are copied into the page-locked staging and go through the
 * front-end on the copy stream into the pipe's stream, as uwspr_stream_push_audio does (stream sample m = the
 * front-end's output at audio index 32 m; records' stream_pos / 375 = audio time in s).  A pipe's stream is audio or
 * (I,Q), decided by its first push; the front-end mode is the lanes' option "frontend" at that push. */
int uwspr_pipe_push_audio(uwspr_pipe *pipe, const void *audio, int nsamples, int format);
/* Several channels through one pipe: audio is [nframes][nchannels] interleaved (the WAV / ALSA layout), in either
 * format, pieces of any length, formats mixing between pushes as for one channel.  The first audio push latches the
 * channel count (1..UWSPR_PIPE_MAX_CHANNELS); a push with another count, an audio push into an (I,Q) pipe or the
 * reverse, and a bad format fail that call with UWSPR_ERR_ARG and the pipe goes on.  uwspr_pipe_push_audio(p, x, n, f)
 * is uwspr_pipe_push_audio_channels(p, x, n, 1, f).  Every channel is its own stream: a record's channel says which,
 * and per channel frame and stream_pos count as a one-channel pipe fed that channel alone counts them, so (channel,
 * frame) identifies a record.  A batch holds frames of one channel; the batches of a take (batch_frames frames of
 * every channel) are launched channel 0..nchannels-1, so records come in (take, channel, frame) order.  flush launches
 * the short last batch of every channel; the stats count frames over all channels.
 * Device memory of the stream, made by the first push (UWSPR_ERR_NOMEM, with a message, if it does not fit): two
 * buffers of nchannels planes of (ceil(lanes / nchannels) + 3) * batch_frames * hop + fl (I,Q) pairs (8 bytes; each
 * plane rounded up to 64 pairs when nchannels > 1), plus two audio buffers of ((32 J + 32) * nchannels + 4 Mi)
 * samples (4 bytes; J = 216 taps per phase in the default "grc" front-end, 32 in "compact").  Defaults (hop 3375,
 * batch_frames 256, 9 lanes): 2 x 83 MB for one channel, 2 x 28 MB per channel from 9 channels on.
 * Audio at another rate: "audio_rate" is the pipe's own option (uwspr_pipe_set_option; default 12000, any rate
 * uwspr_resample_design supports, else UWSPR_ERR_ARG), latched by the first audio push; setting another value once the
 * audio stream runs is UWSPR_ERR_ARG.  The pieces then go through K11 and the front-end as described at
 * uwspr_resample_batch, the pipe makes room for the 12 kS/s samples a piece will produce, and the resampler's buffers
 * (see there) come on top of the figures above.  nframes counts frames at that rate; stream_pos / 375 stays seconds.
 * Impulsive noise: "blank" and "blank_guard" are the pipe's own options as well (uwspr_pipe_set_option; 0 = off and 2 by
 * default, ranges as at uwspr_blank_batch, else UWSPR_ERR_ARG), latched by the first audio push; another value once the
 * audio stream runs is UWSPR_ERR_ARG.  The pieces then go through K12 first, as described at uwspr_blank_batch; the
 * last "blank_guard" samples pushed are never output.
 * Several carriers (FDMA, or one source that is not at 1500 Hz): uwspr_pipe_set_carriers(pipe, hz, n) gives K0's
 * centres in Hz, n >= 1 distinct integers whose order is kept; "frontend_hbw" (uwspr_pipe_set_option, 1 .. 150, default
 * 10) is the pipe's own half-bandwidth, and "carrier" = hz is uwspr_pipe_set_carriers(pipe, &hz, 1).  Legal only before
 * the first audio push (afterwards UWSPR_ERR_ARG); that push latches them with the channel count and checks
 * nchannels * n <= UWSPR_PIPE_MAX_CHANNELS and hb + 20 <= hz <= 6000 - hb - 20 (UWSPR_ERR_ARG, nothing latched).  Every
 * audio channel c is then heard at every carrier k: plane c * n + k is a stream of its own, K0's carrier form (see
 * uwspr_frontend_design_at: taps at hz[k], then the rotator) fills it from the same audio, and whatever is said above of
 * "every channel" holds of every plane: a take launches one batch per plane in plane order, records come in (take,
 * plane, frame) order, and per plane frame and stream_pos count as a one-carrier, one-channel pipe's.  With n > 1 a
 * record's `channel` field holds the PLANE index c * n + k (uwspr_decode has no free byte and the ABI version stays);
 * with n == 1 it is the channel.  K11 and K12 see the nchannels audio channels only.  With {1500}, 10 nothing new runs.
 * Memory: nchannels * n takes nchannels' place in the ring's formula above (the audio buffers keep nchannels), plus
 * n x 55 KB of tap images (32 J pairs of 8 bytes) and 3 KB of rotator table.
 * uwspr_params.cf (the straight-line model's Doppler scale) stays the caller's, one per pipe, as the reference's FDR
 * block has it: with one carrier set cf to it; with several, cf's scale serves them all (no per-carrier tables). */
#define UWSPR_PIPE_MAX_CHANNELS 64
int uwspr_pipe_push_audio_channels(uwspr_pipe *pipe, const void *audio, int nframes, int nchannels, int format);
int uwspr_pipe_set_carriers(uwspr_pipe *pipe, const int *hz, int n);
/* B frames already in device memory (frame b at frames + 2*stride*b floats, stride 0 = fl): searched as one
 * batch.  The memory must stay valid until the batch's results have been collected. */
int uwspr_pipe_submit_device(uwspr_pipe *pipe, const float *dev_frames, int B, int stride);
/* launch what is complete (a last, short batch of a pushed stream) and wait for everything in flight */
int uwspr_pipe_flush(uwspr_pipe *pipe);
/* up to cap finished records in frame order; wait != 0: block until at least one is there or nothing is
 * in flight.  returns the count (>= 0) or a negative status. */
int uwspr_pipe_collect(uwspr_pipe *pipe, uwspr_decode *out, int cap, int wait);
int uwspr_pipe_get_stats(uwspr_pipe *pipe, uwspr_pipe_stats *st);
/* uwspr_stream_blank_stats of the pipe's audio stream (the pipe's options "blank" / "blank_guard"): call it from the
 * producer's thread */
int uwspr_pipe_blank_stats(uwspr_pipe *pipe, long long *samples, long long *zeroed, int cap);
/* uwspr_set_option on every lane's context (e.g. "fast_search").  Only while nothing is in flight (after
 * uwspr_pipe_flush / before the first batch): UWSPR_ERR_ARG otherwise, and for "sched", which the pipe chooses by its
 * lane count (uwspr_pipe_opts.sched_form).
 * "passes" is the pipe's own option: 1 (default) or 2, anything else UWSPR_ERR_ARG.  With 2 a batch's host tail is followed
 * by a second pass on its lane: the frames that hold a decoded record go through uwspr_subtract_batch's kernels (refine =
 * 1) into a buffer of the lane -- one item per decoded record in candidate order: the symbols of its message
 * (uwspr_wspr_symbols), its f1, the jig_shift of the try that decoded, its drift1 (a NONLINEAR candidate: the constant
 * the fine search correlated with, f1 + slmFrequencyDrift at t = 0, and no drift) -- and those residual frames through FDR +
 * schedule + Fano with the same options.  A second-pass record is emitted directly behind its frame's first-pass records,
 * only if it decoded and its message is not one of that frame's first-pass messages (nor that of a second-pass record
 * already emitted for the frame: a new message appears once): pass = 1, cand counting on from the
 * frame's first-pass records, npk that of the first pass, coarse / f1 / ... what the second search found.  Frame and
 * channel order stay; the stream is read, never written.  Stats: frames and batches as with 1; candidates and decoded
 * count the emitted records, the Fano and resume figures include the second pass.  With 1 nothing changes.
 * "osd" and "osd_gap" are the pipe's own as well.  "osd" = 0 (default), 1 or 2 (anything else UWSPR_ERR_ARG): with 1 or 2, K9
 * (uwspr_osd_batch below, that order) runs on the batch's lane behind its host tail, resumed tries included -- and behind
 * the second pass's host tail with "passes" = 2 -- for every record with worth_a_try in which at least one try passed the
 * gates of cc:470 and none decoded: one item per such record, the gated try with the largest jig_sync (the first one on
 * ties), its symbols read where they lie in the lane's device records.  An item with dnext - dmin >= "osd_gap" (>= 0;
 * default UWSPR_OSD_GAP_DEFAULT) whose bytes uwspr_unpack_message accepts turns the record into a decoded one: decoded = 1,
 * idt = that try, message set, osd = 1.  It is an ordinary decoded record from there on: counted in the stats' decoded,
 * subtracted by "passes" = 2.  With "osd" = 0 every byte and statistic is what it is without the option.
 * "block" is the pipe's own too: 0 (default), 2 or 3 (anything else UWSPR_ERR_ARG).  With 2 or 3, K10
 * (uwspr_blockdemod_batch below) runs on the batch's lane behind its host tail, resumed tries included, and before "osd" --
 * and behind the second pass's host tail with "passes" = 2 -- on the records "osd" would take: one item per record with
 * worth_a_try that decoded on no try and has a gated try, the gated try with the largest jig_sync (the first one on ties).
 * The item is that try's jig_shift with the record's f1 and drift1 (a NONLINEAR candidate: the constant f1 +
 * slmFrequencyDrift at t = 0, no drift, as "passes" = 2 models it), over the batch's own frames (the second pass: the
 * residual frames).  For n = 2 .. "block" in that order: a vector whose rms (that of cc:469-474) is above the gate of
 * cc:470 is de-interleaved and goes through uwspr_fano_decode(60, 10000) on the host pool; the first that decodes and
 * whose bytes uwspr_unpack_message accepts turns the record into a decoded one: decoded = 1, idt = that try, message set,
 * block = n.  It is an ordinary decoded record from there on (counted, subtracted by "passes" = 2, no item of "osd").
 * These calls count in fano_calls / fano_timeouts, their time in resume_s.  With "block" = 0 every byte and statistic is
 * what it is without the option.
 * "deep_min" and "deep_gap" (both >= 0; defaults UWSPR_DEEP_MIN_DEFAULT and UWSPR_DEEP_GAP_DEFAULT) are the pipe's own: the
 * acceptance thresholds of the list search, see uwspr_pipe_set_list.  "call_min" and "call_gap" (both >= 0; defaults
 * UWSPR_CALL_MIN_DEFAULT and UWSPR_CALL_GAP_DEFAULT) likewise: those of the call search, see uwspr_pipe_set_calls. */
int uwspr_pipe_set_option(uwspr_pipe *pipe, const char *name, int value);
/* The list of expected messages (the rules of uwspr_deep_set_list below; host memory, copied): with a list set, K13
 * (uwspr_deep_batch below) runs on the batch's lane behind its host tail, resumed tries included, after "block" and before
 * "osd" -- and behind the second pass's host tail with "passes" = 2 -- on the records those two take: one item per record
 * with worth_a_try that decoded on no try and has a gated try (cc:470), the gated try with the largest jig_sync (the first
 * one on ties), its symbols read where they lie in the lane's device records.  An item with sbest >= "deep_min" and (M == 1
 * or sbest - snext >= "deep_gap") turns the record into a decoded one: decoded = 1, idt = that try, message = the list's
 * bytes of `best`, osd = 2.  uwspr_unpack_message is not asked: the list is the user's word.  It is an ordinary decoded
 * record from there on (counted in the stats' decoded, subtracted by "passes" = 2, no item of "osd").  Its time counts in
 * resume_s.  Only while nothing is in flight (UWSPR_ERR_ARG otherwise, as for uwspr_pipe_set_option); a list that breaks
 * the rules is UWSPR_ERR_ARG and the list in force stays.  M = 0 turns the stage off and frees the table: every byte and
 * statistic is then what it is without a list, and nothing of K13 runs or is allocated.
 * Device memory: ONE table per pipe, read by every lane, 192 bytes per message rounded up to 16 messages (M = 65536:
 * 12.6 MB), plus per lane that ran it 16 bytes per item and message chunk (at most 1024 chunks per 16 items). */
int uwspr_pipe_set_list(uwspr_pipe *pipe, const int8_t *messages7 /*[M][7]*/, int M);
/* The call set (the rules and arguments of uwspr_calls_set below; host memory, copied): with a set, K14 (uwspr_calls_batch
 * below) runs on the batch's lane behind its host tail after "block" and the list search -- a given list is the more
 * specific knowledge and goes first -- and before "osd", also behind the second pass's host tail with "passes" = 2, on the
 * records those stages take (the item rule at uwspr_pipe_set_list; a record the list search decoded is no item any more),
 * its symbols read where they lie in the lane's device records.  An item with sbest >= "call_min" and (a single allowed
 * hypothesis or sbest - snext >= "call_gap") turns the record into a decoded one: decoded = 1, idt = that try, message =
 * message(best), osd = 3.  uwspr_unpack_message is not asked: the message is valid by construction.  It is an ordinary
 * decoded record from there on (counted in the stats' decoded, subtracted by "passes" = 2, no item of "osd").  Its time
 * counts in resume_s.  Only while nothing is in flight (UWSPR_ERR_ARG otherwise); a set that breaks the rules is
 * UWSPR_ERR_ARG and the set in force stays.  A = 0 turns the stage off and frees the set: every byte and statistic is then
 * what it is without one, and nothing of K14 runs or is allocated.
 * Device memory: ONE set per pipe, read by every lane (the 6.2 MB locator table, 3648 bytes per callsign, the bitmap), plus
 * per lane that ran it 12 bytes per item and workgroup of its row (about 2048 workgroups per 16 items). */
int uwspr_pipe_set_calls(uwspr_pipe *pipe, const char *const *calls, int A, const uint8_t *grid_bitmap /*[4050] or NULL*/,
                         uint32_t power_mask);
/* Error behaviour.  An argument error (too many samples, a bad B or stride) fails THAT call with UWSPR_ERR_ARG and
 * its message; the pipe goes on.  A runtime failure (HIP, a lane's context) is sticky: the batch it hit emits
 * nothing, records of the batches before it stay collectable, every later call -- and uwspr_pipe_collect once
 * those records are gone -- returns the status; uwspr_pipe_close always returns.
 * Test hook: the batch with running number `batch` fails at its launch (where = 0) or in its host tail (where = 1). */
int uwspr_pipe_inject_failure(uwspr_pipe *pipe, long long batch, int where);

/* ---- measurement -------------------------------------------------------- */
enum { UWSPR_K_SPECTROGRAM = 0, UWSPR_K_SPECTRUM = 1, UWSPR_K_COARSE = 2,
       UWSPR_K_TONECORR = 3, UWSPR_K_FOLD = 4, UWSPR_K_SCHED = 5, UWSPR_K_COUNT = 6 };
typedef struct uwspr_prof {
  double ms[UWSPR_K_COUNT];        /* summed HIP-event time per kernel family */
  int64_t launches[UWSPR_K_COUNT];
  int64_t units[UWSPR_K_COUNT];    /* frames (K0,K1), candidates (K2), hypotheses (K3,K4) */
} uwspr_prof;
/* HIP events are recorded around the kernel launches of the selected families on
 * the context's stream; uwspr_prof_read synchronises, sums and resets them.
 * mask: bit (1 << UWSPR_K_*) per family, UWSPR_PROF_ALL for all, 0 = off.
 * (Each recorded event is a marker packet on the queue: measuring only the
 * dominant kernel keeps the timed region close to the unobserved one.) */
#define UWSPR_PROF_ALL 0x3f
int uwspr_prof_enable(uwspr_ctx *ctx, int mask);
int uwspr_prof_read(uwspr_ctx *ctx, uwspr_prof *out);
/* Start/stop times (ms after `epoch_event`, a hipEvent_t recorded by the caller
 * on the same device) of up to `cap` recorded launches of one family, WITHOUT
 * resetting them; *n receives the count.  Lets a caller that rotates batches over
 * several contexts/streams account for launches that overlap in time. */
int uwspr_prof_intervals(uwspr_ctx *ctx, int kind, void *epoch_event, double *start_ms,
                         double *stop_ms, int cap, int *n);

/* ---- host-side tail of the path ------------------ */
/* sync_and_demodulate_impl.cc:265-282 */
void uwspr_deinterleave(uint8_t *symbols162);
/* lib/Fano.cc:110-252 with the block's metric table (Fano.cc:36-45).
 * returns 0 decoded, -1 timeout (same as the reference). data: 11 bytes. */
int uwspr_fano_decode(const uint8_t *symbols162, uint8_t *data11,
                      uint32_t *metric, uint32_t *cycles, uint32_t *maxnp,
                      int delta, uint32_t maxcycles);
/* lib/Fano.cc:81-100 */
int uwspr_fano_encode(uint8_t *symbols, const uint8_t *data, uint32_t nbytes);
/* Replays cc:457-490 for one candidate on a uwspr_demod_out: gates, deinterleave,
 * Fano in reference order.  returns 1 and fills message7 on decode, else 0. */
int uwspr_decode_candidate(const uwspr_demod_out *d, int8_t *message7,
                           int32_t *idt_used);
/* CPUs this process may keep busy: hardware threads capped by the affinity mask and the cgroup CPU
 * quota (what "one per hardware thread" means below). */
int uwspr_host_threads(void);
/* One process per GPU: the `ranks` processes of a job that share this host (the launcher's LOCAL_WORLD_SIZE) share its
 * CPUs too.  After uwspr_host_set_ranks(n), uwspr_host_threads() is the share above divided by n (at least 1), and that
 * is what the process-wide host pool -- uwspr_decode_batch, the Fano stage of uwspr_pipe_* -- is sized by: eight ranks
 * decode on eight eighths of the host, not on eight full pools (BASELINE configs[4] is host-bound: Fano time-outs at low
 * SNR).  Call it before the first uwspr_decode_batch / uwspr_pipe_open of the process: once the pool exists its size is
 * fixed and the call returns UWSPR_ERR_UNSUPPORTED (nothing changes).  ranks < 1: UWSPR_ERR_ARG. */
int uwspr_host_set_ranks(int ranks);
/* The same for n records on `nthreads` host threads (<= 0: one per hardware
 * thread): the per-candidate loop of cc:389 with its Fano calls spread over the
 * host cores.  messages [n][7] (zero when not decoded), idt_used [n] or NULL,
 * decoded [n] = 0/1.  returns the number decoded (or UWSPR_ERR_ARG). */
int uwspr_decode_batch(const uwspr_demod_out *d, int n, int nthreads,
                       int8_t *messages, int32_t *idt_used, uint8_t *decoded);
/* lib/helpers.cc unpk_ (called at WSPR_unpacker_impl.cc:129), without the
 * on-disk hash table: "CALL GRID dBm" into out (>= 23 bytes). returns 0 ok. */
int uwspr_unpack_message(const int8_t *message7, char *out, size_t out_len);
/* .c2 reader, lib/c2file_source_impl.cc:80-96 (Q negated on load).
 * iq: 2*45000 floats. */
int uwspr_c2_read(const char *path, float *iq, double *dial_freq, int32_t *type);

/* ---- transmit side: the reference's sender (README "Sender": wsprsim, examples/c2ToWaveFile.grc) ---------------- */
/* Message text -> the 50 bits uwspr_unpack_message takes apart, in its 7-byte layout.  Three forms (lower case is taken
 * as upper case): type 1 "CALL GRID4 dBm" (callsign of 1-2 characters, a digit, 1-3 letters); type 2 "PFX/CALL dBm"
 * (1-3 character prefix) or "CALL/SFX dBm" (one character, or two digits 10..99); type 3 "<CALL> GRID6 dBm" (15-bit
 * hash of CALL, uwspr_nhash(call, len, 146) & 32767).  dBm is 0..60 ending in 0, 3 or 7.  Anything else: UWSPR_ERR_ARG
 * and message7 untouched. */
int uwspr_wspr_pack(const char *text, int8_t *message7);
/* lookup3 hashlittle() (the reference's nhash, lib/helpers.cc:151-319) */
uint32_t uwspr_nhash(const void *key, size_t length, uint32_t initval);
/* wsprsim's 162 channel symbols of a message: the 7 bytes zero-padded to 11 -> uwspr_fano_encode (first 162 bits) ->
 * bit-reversal interleave (the inverse of uwspr_deinterleave) -> symbol j = pr3[j] + 2 bit[j] */
int uwspr_wspr_symbols(const int8_t *message7, uint8_t *sym162);
/* .c2 writer, the inverse of uwspr_c2_read: 14-byte NUL-padded name (the file's base name), int32 type, float64 dial
 * frequency, then the nsamples = 45000 (I,Q) binary32 pairs with Q negated (uwspr_c2_read negates it back). */
int uwspr_c2_write(const char *path, const float *iq, int nsamples, double dial_freq, int32_t type);

/* One transmission.  Baseband (375 S/s) sample start + k, k = 0 .. 162*256 - 1, of its channel is
 *     gain e^{j theta(k)},  theta(k) = phase0 + sum_{u < k} 2 pi f(u) / 375,
 *     f(u) = f0_hz + (symbols[u / 256] - 1.5) 375/256 + drift_hz (u - (N - 1)/2) / (N - 1),  N = 41472
 * (wsprsim's signal: the exclusive phase accumulation, a linear drift centred on the transmission as synth.make_frames
 * has it), zero elsewhere; the signals of a channel add up in ascending index.  theta is evaluated in binary64 from
 * per-symbol prefix sums, so any window renders without a sequential scan. */
typedef struct uwspr_tx_signal {
  uint8_t symbols[UWSPR_NSYM];   /* 0..3 */
  uint8_t _pad[2];
  int32_t channel;
  int64_t start;                 /* baseband samples (audio sample 32 start) */
  double f0_hz, drift_hz, phase0;
  float gain;
  int32_t _pad2;
} uwspr_tx_signal;
/* What a channel of a rendered recording adds to its signals: AWGN of standard deviation sigma (Philox4x32-10 keyed by
 * (seed, channel, absolute audio index) + Box-Muller: the same samples however the recording is cut into calls), and
 * background[n mod background_len] x background_gain (format UWSPR_AUDIO_F32 / S16 = s / 32768; the flowgraph's
 * repeating wavfile_source; NULL: none).  background is memory of the call's `where`: with UWSPR_DEVICE, out and every
 * background must lie inside a device allocation of the context's device, else the call fails with UWSPR_ERR_ARG before
 * any launch (a host pointer would fault the kernel). */
typedef struct uwspr_tx_channel {
  double sigma;
  uint64_t seed;
  const void *background;
  int64_t background_len;
  int32_t background_format;
  float background_gain;
} uwspr_tx_channel;
/* Baseband samples [t0, t0 + n) of one channel, the signals above, as uwspr_c2_read returns a .c2 file (the file itself
 * holds the conjugate): the VE3EMB symbols at start 375, f0 0, gain 1 are examples/VE3EMB.c2.  iq: n (I,Q) pairs per `where`. */
int uwspr_tx_baseband(uwspr_ctx *ctx, const uwspr_tx_signal *sig, int nsig, int channel, long long t0, int n, float *iq,
                      int where);
/* Audio frames [t0, t0 + nframes) of a C-channel 12 kS/s recording (K7, k7_transmit.hip), interleaved [nframes][C] as
 * uwspr_pipe_push_audio_channels takes it: channel c's sample n is
 *     Re sum_j g[n - 32 j] x_c[j] + sigma_c noise + background_gain_c background_c[n mod len]
 * x_c being the channel's baseband as the .c2 file holds it (the conjugate of uwspr_tx_baseband's) and g the 3179-tap
 * composite of c2ToWaveFile.grc's chain (zero-stuff x32, low_pass(1, 12000, 200, 10, HAMMING), low_pass(1, 12000, 2500,
 * 100, HAMMING) at 1500 Hz, real part): a tone at f Hz of uwspr_tx_baseband's output comes out at 1500 + f Hz, a unit
 * baseband as a tone of amplitude ~1/32.  format UWSPR_AUDIO_F32, or UWSPR_AUDIO_S16
 * = the binary32 product 32767 x clamped to [-32768, 32767] and rounded to nearest, halves to even.  Renders of consecutive pieces concatenate to the bytes of one render; host and device
 * output are the same bytes.  chan [C], 1 <= C <= UWSPR_PIPE_MAX_CHANNELS, t0 >= 0; every signal's channel < C.  Bad
 * arguments fail the call with UWSPR_ERR_ARG before any device use.  where: UWSPR_HOST (complete on return) or
 * UWSPR_DEVICE (asynchronous on the context's stream). */
int uwspr_tx_render(uwspr_ctx *ctx, const uwspr_tx_signal *sig, int nsig, const uwspr_tx_channel *chan, int C,
                    long long t0, long long nframes, int format, void *out, int where);

/* A moving source: the straight-line model (SLM) of the receiver's nonlinear search (lib/slm.cc).  The hydrophone is
 * at the origin and the source at q(t) = (v1 t + p1, v2 t + p2) metres, R(t) = |q(t)|, c = 1500 m/s, fc = the signal's
 * carrier (1500 Hz unless uwspr_tx_render_at / uwspr_tx_baseband_at name another: each signal's Doppler phase uses its own).  Baseband index start + k of a transmission has trajectory time t = t_first + k / 375 s.  With
 * theta the static phase above (uwspr_tx_baseband's orientation, gain e^{+j theta}) and D(t) = (R(t) - R(t_first)) / c,
 * or R(t) / c with UWSPR_TX_ABSOLUTE:
 *   UWSPR_TX_STATIC   the signal as uwspr_tx_baseband makes it (the motion is ignored);
 *   UWSPR_TX_DOPPLER  y(k) = gain e^{+j [theta(k) - 2 pi fc D(t)]}, 0 <= k < N: the carrier Doppler alone.  The added
 *                     frequency is -(fc / c) dR/dt = slmFrequencyDrift(m_nl, 1500, t): a trajectory of the receiver's
 *                     grid with t_first = 0 is the hypothesis K3 scores (t = floor(k 111 / 162) s from the first symbol);
 *   UWSPR_TX_DELAY    propagation: k' = k - 375 D(t), y(k) = gain e^{+j [theta(k') - 2 pi fc D(t)]} for 0 <= k' < N, theta
 *                     at a fractional index being the per-symbol quadratic with fractional r.  This adds the time
 *                     compression to the carrier Doppler.  With UWSPR_TX_ABSOLUTE, start is the emission time and the
 *                     whole travel time R / c delays the signal.
 * R is evaluated at the reception time t, not at the emission (retarded) time: an error of first order in v / c.
 * UWSPR_TX_SPREADING multiplies the amplitude by R(t_first) / R(t) (spherical spreading).  Everything is binary64 per
 * sample, in closed form: any window renders alone.  A zero-velocity motion without ABSOLUTE or SPREADING gives the bytes
 * of no motion in either model.  Refused with UWSPR_ERR_ARG before any launch, the output untouched: a non-finite field,
 * an unknown model or flag bit, |(v1, v2)| > 100 m/s, |t_first| > 1e6 s, |p1| or |p2| > 1e9 m, SPREADING with R < 1 m somewhere in the
 * transmission.  Multipath is several signals with their own start, gain and motion. */
#define UWSPR_TX_STATIC 0
#define UWSPR_TX_DOPPLER 1
#define UWSPR_TX_DELAY 2
#define UWSPR_TX_ABSOLUTE 1
#define UWSPR_TX_SPREADING 2
typedef struct uwspr_tx_motion {
  double v1, v2;                 /* m/s */
  double p1, p2;                 /* m, at t = 0 */
  double t_first;                /* s: trajectory time of the transmission's first sample */
  int32_t model;                 /* UWSPR_TX_STATIC / DOPPLER / DELAY */
  int32_t flags;                 /* UWSPR_TX_ABSOLUTE | UWSPR_TX_SPREADING */
} uwspr_tx_motion;
/* uwspr_tx_baseband and uwspr_tx_render with a motion per signal: motion is NULL (every signal static) or has nsig
 * entries.  Same outputs, chunking and host / device identities as the static calls. */
int uwspr_tx_baseband_moving(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, int nsig,
                             int channel, long long t0, int n, float *iq, int where);
int uwspr_tx_render_moving(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, int nsig,
                           const uwspr_tx_channel *chan, int C, long long t0, long long nframes, int format, void *out,
                           int where);

/* Transmit at another carrier, and at several at once (K7's carrier form; the transpose of K0's).  carrier_hz is NULL
 * (1500 Hz for every signal) or has nsig entries, integer Hz; motion is NULL or has nsig entries.  The option "tx_cutoff"
 * (integer Hz, default 2500, 500 .. 5900) is the cut-off of the flowgraph's second low-pass.  Allowed carriers:
 * 170 <= fc <= tx_cutoff - 250 (the rotated filter is a band-pass around -fc that must pass the baseband at 0 Hz: with
 * |f0| <= 150 Hz and the 100 Hz transition centred on the cut-off the signal stays fc + 250 below it); anything else, in
 * any entry -- one whose signal the window drops included --, or more than 64 distinct carriers in one call, is
 * UWSPR_ERR_ARG before any launch.
 * The flowgraph's chain is zero-stuff x32, h1 = low_pass(1, 12000, 200, 10), freq_xlating_fir_filter holding
 * h2 = low_pass(1, 12000, tx_cutoff, 100) rotated to fc, the mixer at fc, the real part.  With audio index n = q + 32 j
 * the mixer factors, e^{-j 2 pi fc n / 12000} = e^{-j 2 pi fc q / 12000} e^{-j 2 pi fc j / 375}: the first factor goes
 * into the taps, the second is a rotator on baseband sample j with 375 values, the identity when 375 divides fc.
 * Taps (uwspr_tx_design_at: g [3179] (re, im) pairs in binary64, image [32][104] (Re g, -Im g) binary32 pairs, tap p + 32 i
 * at [p][i], +0 behind the last; either may be NULL; host only; returns 3179, or UWSPR_ERR_ARG outside the ranges above):
 *   g_fc[q] = e^{-j 2 pi fc q / 12000} sum_k h2r[k] h1[q - k],
 *   h2r[k]  = h2[k] e^{+j 2 pi fc k / 12000} rounded to binary32 pairs as freq_xlating_fir_filter holds them,
 * designed in binary64; fc k and fc q are reduced mod 12000 in integers before any cos / sin, and a multiple of pi/4 takes
 * the exact octant values, so (1500, 2500) gives the tap image it always gave, byte for byte.  3179 taps whatever fc and
 * the cut-off are (2891 + 289 - 1: the transition widths alone set the counts).
 * Channel c's audio sample n:
 *   1. the channel's kept signals are grouped by carrier, the distinct carriers ascending in Hz: f_1 < ... < f_G;
 *   2. x_f[j] = the sum of group f's signals in ascending signal index, as the .c2 file holds the baseband (the
 *      conjugate of uwspr_tx_baseband's), formed exactly as the 1500 Hz render forms its one sum;
 *   3. the rotator: if 375 divides f, xr_f is x_f's bytes; otherwise, with (c, d) = rot[((f mod 375)(j mod 375)) mod 375],
 *      j mod 375 in 0 .. 374 for negative j as well and rot the table of uwspr_frontend_rotator,
 *        xr.re = fmaf(x.re, c, -(x.im d)),   xr.im = fmaf(x.re, d, x.im c)      -- K0's one order;
 *   4. chain_f[n] = the 1500 Hz render's one chain of 208 fused multiply-adds from +0 (tap index ascending, real before
 *      imaginary) over g_f's image and xr_f;
 *   5. a = chain_{f_1}[n], then a = fl32(a + chain_{f_g}[n]) for g = 2 .. G;
 *   6. noise, background and quantiser as in uwspr_tx_render.
 * A chain starts at +0 and cannot become -0, so a group whose signals are all silent adds +0 and changes no byte: renders
 * of any pieces concatenate to the bytes of one render also where a carrier's signals begin or end partway.
 * The carrier form runs when some signal's carrier is not 1500, or "tx_cutoff" is not 2500, or the option "tx_form" is 1
 * (0, the default: only then); with everything at the defaults the 1500 Hz kernels run, nothing new is allocated and every
 * byte is what it was; "tx_form" = 1 gives those same bytes through the carrier form.  The four calls above are these with
 * carrier_hz NULL.  uwspr_tx_baseband_at's output is not rotated: there the carrier only scales a motion's Doppler. */
#define UWSPR_TX_CUTOFF_DEFAULT 2500
int uwspr_tx_render_at(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, const int32_t *carrier_hz,
                       int nsig, const uwspr_tx_channel *chan, int C, long long t0, long long nframes, int format, void *out,
                       int where);
int uwspr_tx_baseband_at(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, const int32_t *carrier_hz,
                         int nsig, int channel, long long t0, int n, float *iq, int where);
int uwspr_tx_design_at(int carrier_hz, int cutoff_hz, double *g, float *image);

/* Transmit through a medium (K7's medium form): Doppler-spread fading per signal, impulsive noise per audio channel.
 *
 * Fading.  fade is NULL (no signal fades) or has nsig entries beside sig / motion / carrier_hz.  A signal with paths = M > 0
 * is multiplied by a sum of M sinusoids (a Gaussian Doppler spectrum of standard deviation spread_hz / 2 around shift_hz:
 * spread_hz is the two-sigma Doppler spread, Watterson's convention) plus a fixed part (Rician; k_factor = 0: Rayleigh).
 * Design, on the host in binary64 (uwspr_tx_fade_design: a [2] = (a0, a1), omega [M], phi [M]; any may be NULL; returns
 * M, or UWSPR_ERR_ARG outside the ranges below or with paths = 0).  For path m = 0 .. M - 1 take words x, y, z of the
 * Philox4x32-10 block with counter (m, 0, 0x46414445, 0) and key (seed low word, seed high word):
 *     u1 = ((x >> 8) + 0.5) / 2^24,  u2 = (y >> 8) / 2^24,  u3 = (z >> 8) / 2^24,
 *     nu_m = shift_hz + (spread_hz / 2) sqrt(-2 ln u1) cos(2 pi u2)        Hz
 *     omega_m = 2 pi nu_m / 375                                            rad per baseband sample
 *     phi_m = 2 pi u3
 *     a0 = sqrt(K / (K + 1)),  a1 = sqrt(1 / ((K + 1) M)):  a0^2 + M a1^2 = 1, the signal's mean power is unchanged.
 * Gain.  k = j - start, the reception index of baseband sample j (an integer under every motion model, ABSOLUTE
 * included, and bounded by the signal's support):
 *     h(k) = a0 + a1 sum_m e^{j (omega_m k + phi_m)}
 * each angle fl64(fl64(omega_m k) + phi_m), the real and the imaginary sum in binary64 from +0 with m ascending, then
 * hr = fl64(a0 + fl64(a1 sum cos)), hi = fl64(a1 sum sin).
 * Application.  With theta and the gain g (SPREADING included) as the unfaded signal has them, in uwspr_tx_baseband's
 * orientation, and (cs, sn) = (cos theta, sin theta):
 *     yr = cs hr - sn hi,   yi = cs hi + sn hr      (binary64, in that order)
 *     re += g (float) yr,   im += g (float) yi      (binary32; the render's staging holds the conjugate)
 * where the unfaded code has re += g (float) cs, im += g (float) sn.  The support (0 <= k < N, a DELAY motion's
 * 0 <= k' < N) is the unfaded one.  paths = 1 with K = 0 is a pure Doppler shift nu_0 with phase phi_0.  Multipath stays
 * several signals, each with its own fade.
 * Refused with UWSPR_ERR_ARG before any launch, the output untouched, also where the window drops the signal: paths
 * outside 0 .. 32; with paths > 0 a non-finite field, spread_hz outside 0 .. 20, |shift_hz| > 20, k_factor outside
 * 0 .. 1e6.  An entry with paths = 0 is not read further. */
typedef struct uwspr_tx_fade {
  double spread_hz;   /* Doppler spread, 2 sigma of a Gaussian Doppler spectrum, 0 .. 20 */
  double shift_hz;    /* mean Doppler of the scattered part, |.| <= 20 */
  double k_factor;    /* Rician K, linear power ratio fixed : scattered, 0 (Rayleigh) .. 1e6 */
  uint64_t seed;
  int32_t paths;      /* M sinusoids, 1 .. 32; 0: this signal does not fade (entry ignored) */
  int32_t _pad;
} uwspr_tx_fade;
/* Impulsive noise: Bernoulli-Gaussian bursts (snapping shrimp, clicks).  impulse is NULL (none) or has C entries beside
 * chan.  With thr = (uint32) min(floor(rate 2^32), 2^32 - 1), made on the host in binary64:
 *   event    audio index e >= 0 of channel c is an event when word x of the Philox4x32-10 block with counter
 *            (e low, e high, c, 1) and key (seed low, seed high) is below thr (the AWGN's blocks have 0 in counter word
 *            3: equal seeds still give independent streams);
 *   sample   an event at e adds fl32(sigma_f32 gauss) to samples e + d, d = 0 .. length - 1, gauss being the AWGN's
 *            Box-Muller on words x, y of the block with counter (e low, e high, c, 2 + d);
 *   order    sample n collects its events in ascending d (e = n - d >= 0), one binary32 add each, after the AWGN add
 *            and before the background add; the quantiser is unchanged.
 * rate = 0 or sigma = 0: no impulses.  Nothing depends on a tile or a call: an event before t0 whose burst reaches into
 * the window contributes.  Refused with UWSPR_ERR_ARG before any launch: a non-finite field, rate outside 0 .. 0.25,
 * sigma < 0, length outside 1 .. 8. */
typedef struct uwspr_tx_impulse {
  double rate;      /* probability of an event per audio sample, 0 .. 0.25 */
  double sigma;     /* standard deviation of an impulse sample (same units as uwspr_tx_channel.sigma), >= 0 */
  uint64_t seed;
  int32_t length;   /* samples per event, 1 .. 8 */
  int32_t _pad;
} uwspr_tx_impulse;
/* uwspr_tx_render_at / uwspr_tx_baseband_at through a medium.  The medium form (new instances of the kernels, built on
 * the carrier form: a group's faded and unfaded signals add in ascending index as ever) runs only when some kept signal
 * has paths > 0 or some channel has impulses; otherwise these calls are uwspr_tx_render_at / uwspr_tx_baseband_at -- the
 * same kernels, the same bytes, nothing new allocated.  Pieces concatenate and host and device output are the same bytes,
 * as for every render. */
int uwspr_tx_render_medium(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, const int32_t *carrier_hz,
                           const uwspr_tx_fade *fade, int nsig, const uwspr_tx_channel *chan, const uwspr_tx_impulse *impulse,
                           int C, long long t0, long long nframes, int format, void *out, int where);
int uwspr_tx_baseband_medium(uwspr_ctx *ctx, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, const int32_t *carrier_hz,
                             const uwspr_tx_fade *fade, int nsig, int channel, long long t0, int n, float *iq, int where);
int uwspr_tx_fade_design(const uwspr_tx_fade *f, double a[2], double *omega, double *phi);

/* ---- known-symbol subtraction (K8, k8_subtract.hip) --------------------------------------------------------------- */
/* A decoded transmission is rebuilt from its 162 channel symbols, fitted to the samples and taken out of them, so that a
 * weaker one within a tone spacing of it can be found in what is left.  The reference has no counterpart; binary32 with
 * fused multiply-adds, phases in binary64.  N = 41472, df = 375/256.  An item models symbol i at the frequency of the
 * receiver's LINEAR hypothesis,
 *     f_i = f_hz + (drift_hz / 2)(i - 81) / 81 + (symbols[i] - 1.5) df.
 * Refinement (refine != 0): over the lags l = -24..24 and the offsets q = -4..4,
 *     M(l, q) = sum_i | sum_{k < 256} x[shift + l + 256 i + k] e^{-j 2 pi (f_i + 0.0125 q) k / 375} |
 * (samples outside [0, fl) count as 0); the first maximum in (q, l) order -- q ascending, then l -- gives shift' = shift + l,
 * f' = f_hz + 0.0125 q (formed in binary64, rounded to the binary32 of the result record) and metric = M.  refine = 0: f' =
 * f_hz, shift' = shift, metric = 0.  A call with refine = 0 on (f', shift') removes what the refining call removed.
 * NaN samples are accepted.  The pick walks M in (q, l) order from M(-24, -4) and moves on `>` alone, and a comparison with
 * a NaN is false: a NaN M is never moved to, and a NaN M(-24, -4) is never left -- the result is then (q, l) = (-4, -24) with
 * metric = NaN (one NaN sample inside every lag's windows does that).  In the cancellation a NaN or infinite sample makes
 * NaN of the outputs whose 1023 taps reach it, |k - k0| <= 511, and of nothing else; other frames' bytes never depend on it.
 * Cancellation, for k in [0, N) with shift' + k inside [0, fl) (nothing else is touched):
 *     r[k] = e^{j theta(k)}, theta(k) = 2 pi sum_{u < k} f_{u div 256} / 375      (f_i with f' in the place of f_hz)
 *     c[k] = x[shift' + k] conj r[k]                                         (0 for any other k)
 *     a[k] = sum_m w[m] c[k + m - 511] / sum_m w[m] v[k + m - 511],   m = 0..1022
 *     out[shift' + k] = x[shift' + k] - a[k] r[k]
 * w being the 1023-tap Hann window 0.5 - 0.5 cos(2 pi (m + 1) / 1024) and v = 1 where c is defined, 0 elsewhere: the
 * amplitude is a weighted mean over the samples that exist.  removed = sum |a r|^2.
 * Items of one frame apply in list order, each refined and fitted on the residual the one before left.
 * frames: B frames per `where` and uwspr_set_frame_stride; frames_out: contiguous [B][fl], host memory with UWSPR_HOST,
 * device memory with UWSPR_DEVICE and UWSPR_DEVICE_FRAMES; frames without an item are copied.  frames_out == frames is
 * allowed when the stride is 0 or fl; any other overlap of the two is refused.  items: HOST memory whatever `where` says
 * (call records), sorted by frame, frame in [0, B), symbols <= 3, f_hz and drift_hz finite (|f| <= 1e4, |drift| <= 1e3),
 * |shift| <= 2^20: anything else returns UWSPR_ERR_ARG before any launch, the output untouched.  res: nitems records in
 * item order (device memory with UWSPR_DEVICE, else host), or NULL.  Host and device calls give the same bytes. */
typedef struct uwspr_sub_item {
  int32_t frame, shift;
  float f_hz, drift_hz;
  uint8_t symbols[UWSPR_NSYM];   /* 0..3 */
  uint8_t _pad[2];
} uwspr_sub_item;
typedef struct uwspr_sub_result {
  float f_hz;       /* f' */
  int32_t shift;    /* shift' */
  float metric;     /* M at the maximum (0 without refinement) */
  float removed;    /* sum |a r|^2: the energy taken out */
} uwspr_sub_result;
int uwspr_subtract_batch(uwspr_ctx *ctx, const float *frames, int B, int where, const uwspr_sub_item *items, int nitems,
                         int refine, float *frames_out, uwspr_sub_result *res);

/* ---- ordered-statistics decoding (K9, k9_osd.hip) -------------------------------------------------------------------- */
/* What a try that Fano timed out on can still give: the transmission as the (162, 50) linear block code it is.  The
 * reference has no counterpart (every WSPR decoder in use has this fall-back); all integers, so host, device and the test's
 * restatement give the same bytes.
 * Input: one 162-byte soft-symbol vector as uwspr_demod_out.symbols[idt] holds it (interleaved).  With s[i] the byte at
 * de-interleaved position i (uwspr_deinterleave's table): hard bit h[i] = s[i] >= 128, reliability r[i] = |2 s[i] - 255|
 * (odd, 1..255).  G (50 x 162 over GF(2)): row j = uwspr_fano_encode of the 81-bit input with only bit j set.
 *   1. The positions are ordered by r descending, ties by ascending index.
 *   2. Gauss-Jordan elimination walks the columns of G in that order: the pivot of a column is the first not-yet-pivoted row
 *      with a 1; a column with no such row is skipped; at rank 50 it stops, the pivot columns being the information set.  A
 *      50 x 50 identity is carried alongside, so that message bits can be read back.
 *   3. The order-0 codeword c0 is the reduced rows combined by the hard bits at the 50 pivot positions.
 *   4. Candidates: c0 with every set of at most `order` pivot bits flipped (1, 51, 1276 candidates at order 0, 1, 2).
 *   5. D(c) = sum of r[i] over the positions where c[i] != h[i].
 *   6. The winner has the least D; ties go to fewer flips, then to the lexicographically smaller flip set in pivot order.
 *   7. dmin = its D; dnext = the least D among the other candidates (INT32_MAX at order 0); nflip; nhard = the positions
 *      where it differs from h; message = its 50 message bits packed as uwspr_fano_decode fills data[0..6].
 *   8. Accepted (the pipe's rule, not this call's) means dnext - dmin >= gap and uwspr_unpack_message accepts the bytes.
 * UWSPR_OSD_GAP_DEFAULT: profiles/osd.txt says where the number comes from.
 * symbols [n][162], res [n]: host memory (UWSPR_HOST, complete on return) or device memory (UWSPR_DEVICE, asynchronous on
 * the context's stream; both must lie inside device allocations of the context's device, else UWSPR_ERR_ARG before any
 * launch).  order 0..2, anything else UWSPR_ERR_ARG; n = 0 is fine. */
#define UWSPR_OSD_GAP_DEFAULT 485
typedef struct uwspr_osd_result {
  int32_t dmin, dnext, nhard;
  uint8_t nflip;
  int8_t message[7];
} uwspr_osd_result;
int uwspr_osd_batch(uwspr_ctx *ctx, const uint8_t *symbols /*[n][162]*/, int n, int where, int order, uwspr_osd_result *res);

/* ---- block demodulation (K10, k10_blockdemod.hip) -------------------------------------------------------------------- */
/* Soft symbols from COMPLEX tone correlations summed coherently over n = 1, 2, 3 neighbouring symbols (the transmission is
 * continuous-phase 4-FSK with a known sync bit per symbol), instead of the per-symbol magnitudes of the fine search's mode 2
 * (sync_and_demodulate_impl.cc:240-254).  The reference has no counterpart (the -B mode of the WSPR decoders in use);
 * binary32 with fused multiply-adds, phases in binary64.  df = 375/256.
 * An item is (frame, shift s, f, drift): the fields of a uwspr_sub_item without the symbols; for a NONLINEAR candidate f
 * is the constant the fine search correlated with (f1 + slmFrequencyDrift at t = 0) and drift = 0.  For symbol i = 0..161,
 *     f_i = f + (drift / 2)(i - 81) / 81.
 *   - z_i[j] = sum_{k < 256} x[s + 256 i + k] e^{-j 2 pi (f_i + (j - 1.5) df) k / 375}, tones j = 0..3.  A sample whose index
 *     n = s + 256 i + k is not in 0 < n < min(fl, 45000) counts as 0: the fine search's own bound (cc:200; 45000 whatever
 *     fl is, capped at fl where the reference would read past its arrays).  The phasor starts at (1, 0) in every symbol,
 *     as the fine search's does (cc:188).
 *   - Whatever the data, the carrier advances by theta_i = 2 pi f_i 256 / 375 + pi per symbol: every tone offset
 *     (j - 1.5) df makes an odd number of half cycles in 256 samples.
 *   - Block length n in {1, 2, 3}: block b covers the symbols i0 = n b .. i0 + n - 1 (162, 81, 54 blocks).  For every data
 *     sequence d in {0,1}^n,
 *         P(d) = | sum_{m < n} z_{i0+m}[pr3[i0+m] + 2 d_m] e^{-j psi_m} |,   psi_m = sum_{q < m} theta_{i0+q}.
 *   - soft[i0+m] = max_{d: d_m = 1} P(d) - max_{d: d_m = 0} P(d).  With n = 1 this is mode 2's p[pr3 + 2] - p[pr3].  If any
 *     P(d) of a block is NaN, soft of every symbol of that block is NaN -- the maxima propagate NaN -- so fac is NaN and
 *     all 162 bytes of that block length are 128, whatever n.
 *   - Normalisation as in mode 2 (cc:240-254): fsum and f2sum the mean and the mean square of the 162 values, fac =
 *     sqrt(f2sum - fsum^2), v = 50 soft / fac clipped to [-128, 127], byte = (uint8)(v + 128).  When fac is not a positive
 *     finite number every byte is 128.
 * Output per item: the three 162-byte vectors n = 1, 2, 3, each interleaved as uwspr_demod_out.symbols[idt] holds one; all
 * three are always produced (the work is one set of z either way).  Every sum has one owner and a fixed order: an item's
 * bytes depend neither on the rest of the batch nor on where the frames live.
 * frames: B frames per `where` and uwspr_set_frame_stride.  items: HOST memory whatever `where` says, sorted by frame, frame
 * in [0, B), f_hz and drift_hz finite (|f| <= 1e4, |drift| <= 1e3), |shift| <= 2^20: anything else returns UWSPR_ERR_ARG
 * before any launch, the output untouched.  symbols: host memory with UWSPR_HOST (complete on return); device memory with
 * UWSPR_DEVICE (asynchronous on the context's stream) and UWSPR_DEVICE_FRAMES (complete on return) -- it must lie inside a
 * device allocation of the context's device, else UWSPR_ERR_ARG before any launch.  nitems = 0 is fine. */
typedef struct uwspr_block_item {
  int32_t frame, shift;
  float f_hz, drift_hz;
} uwspr_block_item;
int uwspr_blockdemod_batch(uwspr_ctx *ctx, const float *frames, int B, int where, const uwspr_block_item *items, int nitems,
                           uint8_t *symbols /*[nitems][3][162]*/);

/* ---- list search (K13, k13_deep.hip) --------------------------------------------------------------------------------- */
/* Maximum-likelihood decoding over a list of expected messages (a deployment's callsign / locator / power texts): the 162
 * soft symbols of a try scored against every codeword of the list.  The reference has no counterpart (WSJT's "deep search"
 * against its callsign database); all integers, so host, device and the test's restatement (tests/deep_exact.py) give the
 * same bytes.
 * The list: M messages of 7 bytes each, as uwspr_wspr_pack makes them; 1 <= M <= UWSPR_DEEP_MAX, the low 6 bits of byte 6
 * zero, no two messages equal.  Anything else is UWSPR_ERR_ARG and nothing is changed.
 * The code bits: c[m][p] = uwspr_wspr_symbols(message m)[p] >> 1, p = 0..161 -- the positions in the interleaved order in
 * which uwspr_demod_out.symbols[idt] holds a vector; nothing in this stage de-interleaves.
 * The score of a vector s[0..161] of bytes:
 *     S[m] = sum_p (2 c[m][p] - 1) ((int)s[p] - 128)
 * 162 int32 terms, |S| <= 20736; the order of summation does not matter.
 * The result per vector: best = the m with the largest S, the smallest m on ties; sbest = S[best]; snext = the largest
 * S[m] over m != best (it may equal sbest; INT32_MIN when M = 1); reserved = 0.
 * Accepted (the pipe's rule, not this call's) means sbest >= deep_min and (M == 1 or sbest - snext >= deep_gap).
 * UWSPR_DEEP_MIN_DEFAULT, UWSPR_DEEP_GAP_DEFAULT: profiles/deep.txt says where the numbers come from (margins, not bounds).
 * uwspr_deep_set_list: messages7 [M][7] in HOST memory; the table (+-1 bytes, K padded from 162 to 192 with zeros, 192
 * bytes per message rounded up to 16 messages: 12.6 MB at M = 65536) is built on the host and uploaded once; it replaces
 * the list before.  M = 0 clears the list and frees the table.  The list is checked before anything else, device included.
 * uwspr_deep_batch: symbols [n][162], res [n]: host memory (UWSPR_HOST, complete on return) or device memory
 * (UWSPR_DEVICE, asynchronous on the context's stream; both must lie inside device allocations of the context's device,
 * else UWSPR_ERR_ARG before any launch).  With no list set UWSPR_ERR_ARG; n = 0 is fine. */
#define UWSPR_DEEP_MAX 65536
#define UWSPR_DEEP_MIN_DEFAULT 4373
#define UWSPR_DEEP_GAP_DEFAULT 1145
typedef struct uwspr_deep_result {
  int32_t best, sbest, snext, reserved;
} uwspr_deep_result;
int uwspr_deep_set_list(uwspr_ctx *ctx, const int8_t *messages7 /*[M][7]*/, int M);
int uwspr_deep_batch(uwspr_ctx *ctx, const uint8_t *symbols /*[n][162]*/, int n, int where, uwspr_deep_result *res);

/* ---- call search (K14, k14_calls.hip) -------------------------------------------------------------------------------- */
/* Maximum-likelihood decoding over every type-1 message "CALL GRID4 dBm" of known callsigns: the callsign is known, the
 * locator and the power are free (a glider or drifter that moves, a beacon that carries its telemetry in locator and
 * power).  The list search needs the whole text; this needs the callsign only.  The reference has no counterpart (WSJT's
 * deep search expands a callsign database by locator); all integers, so host, device and the test's restatement
 * (tests/call_exact.py) give the same bytes.
 * A call set:
 *   - A callsigns, 1 <= A <= UWSPR_CALLS_MAX: texts that uwspr_wspr_pack accepts as the callsign of a type-1 message (3 to 6
 *     letters and digits; no compound "PFX/CALL", no hashed "<CALL>"), distinct after packing (lower case is upper case);
 *   - a locator bitmap over ngrid = 0 .. UWSPR_CALL_NGRID - 1 (ngrid as uwspr_wspr_pack numbers a 4-character locator:
 *     180 (179 - 10 (c0 - 'A') - (c2 - '0')) + 10 (c1 - 'A') + (c3 - '0')), bit g = byte g >> 3, bit g & 7, 4050 bytes;
 *     NULL allows every locator;
 *   - a power mask over the UWSPR_CALL_NPOW = 19 type-1 powers P19 = 0, 3, 7, 10, 13, 17, .., 53, 57, 60 dBm, bit d = P19[d];
 *     0 allows all; a bit beyond the 19 is an error.
 * At least one hypothesis must be allowed.  Anything else is UWSPR_ERR_ARG, checked before any device is asked for, and
 * nothing is changed.
 * A hypothesis is h = (a UWSPR_CALL_NGRID + g) 19 + d -- a the index of the callsign, g its ngrid, d the index into P19 --
 * and message(h) the 7 bytes uwspr_wspr_pack("CALL GRID4 dBm") gives; uwspr_call_message composes them from (call, ngrid,
 * dBm) (UWSPR_ERR_ARG for a bad callsign, ngrid outside 0 .. 32399 or a power not in P19).
 * The code bits and the score are the list search's: c[h][p] = uwspr_wspr_symbols(message(h))[p] >> 1 and
 *     S[h] = sum_p (2 c[h][p] - 1) ((int)s[p] - 128),
 * so a list that holds message(h) gives the same S through uwspr_deep_batch.  Nothing is tabulated per hypothesis: a type-1
 * message is n1 (28 bits, the callsign) and n2 = 128 ngrid + dBm + 64, the three occupy disjoint bits of the 50, and the
 * code is linear (uwspr_fano_encode starts from the zero state, the interleaver is a permutation, the code bit is
 * sym >> 1), so c[call, g, d] = c[call only] XOR c[ngrid = g only] XOR c[dBm + 64 only]: one table of 32400 locator
 * codewords for every callsign and power (6.2 MB, built on the host once per set), and a 162-entry sign per (callsign, power).
 * The result per vector: best = the allowed h with the largest S, the smallest h on ties; call, ngrid, dbm = its parts (dbm
 * in dBm, not the index); sbest = S[best]; snext = the largest S over the other allowed h (it may equal sbest; INT32_MIN
 * with a single allowed hypothesis); reserved = 0.
 * Accepted (the pipe's rule, not this call's) means sbest >= call_min and (one allowed hypothesis or sbest - snext >=
 * call_gap).  UWSPR_CALL_MIN_DEFAULT, UWSPR_CALL_GAP_DEFAULT: profiles/calls.txt says where the numbers come from (margins,
 * not bounds).  They are not the list search's: a set is 615 600 hypotheses per callsign, and the other locators and
 * powers of the transmitted callsign are correlated with the transmitted message.
 * uwspr_calls_set: calls [A] texts and grid_bitmap in HOST memory; it replaces the set before.  A = 0 clears the set and
 * frees its memory.
 * uwspr_calls_batch: symbols [n][162], res [n]: host memory (UWSPR_HOST, complete on return) or device memory
 * (UWSPR_DEVICE, asynchronous on the context's stream; both must lie inside device allocations of the context's device,
 * else UWSPR_ERR_ARG before any launch).  With no set UWSPR_ERR_ARG; n = 0 is fine. */
#define UWSPR_CALLS_MAX 64
#define UWSPR_CALL_NGRID 32400
#define UWSPR_CALL_NPOW 19
#define UWSPR_CALL_MIN_DEFAULT 5370
#define UWSPR_CALL_GAP_DEFAULT 725
typedef struct uwspr_call_result {
  int32_t best, call, ngrid, dbm, sbest, snext;
  int32_t reserved[2];
} uwspr_call_result;
int uwspr_calls_set(uwspr_ctx *ctx, const char *const *calls, int A, const uint8_t *grid_bitmap /*[4050] or NULL*/,
                    uint32_t power_mask);
int uwspr_calls_batch(uwspr_ctx *ctx, const uint8_t *symbols /*[n][162]*/, int n, int where, uwspr_call_result *res);
int uwspr_call_message(const char *call, int ngrid, int dbm, int8_t *message7);

/* ---- track a decoded source (K15, k15_track.hip) ---------------------------------------------------------------------- */
/* A decoded transmission is the best probe of the sender's motion there is: all 162 symbols are known, so its Doppler and
 * its time compression can be fitted over 110 s.  K15 correlates the known symbols over straight-line passes, as K8's
 * refinement does over lag and frequency.  The reference has no counterpart; the definition is this project's and
 * tests/track_exact.py restates it in binary64.  Binary32 with fused multiply-adds on the device; everything that decides
 * an index or a phase is binary64.  df = 375/256, c = 1500 m/s, fc = uwspr_params.cf (the Doppler scale K3 uses).
 * A trajectory is (v, d, tc): speed in m/s, range at the closest point of approach (CPA) in m, CPA time in s counted from
 * the item's first sample -- the straight-line model of lib/slm.cc with its redundant degrees of freedom removed (one
 * hydrophone cannot see bearing).  With t in s from the item's first sample, in binary64 and in this one order,
 *     a = v (t - tc),   R(t) = sqrt(d d + a a),   Rdot(t) = (v a) / R(t)       (every product and sum rounded on its own)
 * and symbol i taken at its centre t_i = (256 i + 128) / 375 (the numerator an exact integer).  Per trajectory and symbol
 *     dfreq[i] = -((fc / c) (Rdot(t_i) - Rdot(t_81)))                     Hz: the Doppler relative to mid-transmission --
 *                the constant part cannot be told from the sender's oscillator offset and stays in the fitted frequency;
 *     tau[i]   = rint((375 (R(t_i) - R(t_81))) / c)                       samples, halves to even, with UWSPR_TX_DELAY
 *                (time compression: a receding source arrives later); 0 with UWSPR_TX_DOPPLER.
 * A symbol's frequency is constant: the chirp inside a symbol is ignored (at most about 0.1 Hz at v = 2.8 m/s, d = 50 m).
 * Allowed: 0 <= v <= 10, 1 <= d <= 1e6, |tc| <= 1e4, all finite; then |tau| <= 139.  For SLM parameters (V1, V2, p1, p2)
 * and the trajectory time t_first of the item's first sample, uwspr_track_from_slm gives v = |V|, d = |V1 p2 - V2 p1| / v,
 * tc = -(V.p) / v^2 - t_first (v = 0: d = |p|, tc = 0; d is not checked: the receiver's grid holds radial passes, d = 0),
 * and -(fc / c) Rdot(t) is slmFrequencyDrift.
 * uwspr_track_design: HOST only, no context: dfreq [n][162] and tau [n][162] of n >= 1 trajectories for model
 * UWSPR_TX_DOPPLER / UWSPR_TX_DELAY and the Doppler scale cf (Hz, 0 < cf <= 1e6); UWSPR_ERR_ARG for anything else.
 * The score.  An item is a uwspr_sub_item: frame, shift s, f_hz, drift_hz, symbols.  A hypothesis is
 * h = j nf + (q + qf): j the trajectory, q = -qf .. qf the frequency offset in K8's step of 0.0125 Hz, nf = 2 qf + 1,
 * 0 <= qf <= 16:
 *     f_i(h) = f_hz + 0.0125 q + dfreq[j][i] + (symbols[i] - 1.5) df
 *     T(h)   = sum_i | sum_{k < 256} x[s + 256 i + tau[j][i] + k] e^{-j 2 pi f_i(h) k / 375} |
 * Samples outside [0, fl) count as 0 (K8's rule, not the fine search's); the phasor starts at (1, 0) in every symbol; the
 * hypotheses do NOT use drift_hz (the motion replaces the linear drift).  T_ref is the same sum for the item's own linear
 * model, f_i = f_hz + (drift_hz / 2)(i - 81) / 81 + (symbols[i] - 1.5) df with tau = 0, through the same code: a v = 0
 * trajectory at q = 0 of an item with drift_hz = 0 gives the bytes of T_ref.
 * Result per item: best = the first maximum of T in ascending h (the walk moves on `>` alone: a NaN T is never moved to, a
 * NaN T(0) is never left -- K8's rule); t_best = T(best); t_ref; f_hz = f_hz + 0.0125 q_best, formed in binary64 and rounded
 * to binary32.  The trajectory is best / nf.  Every sum has one owner and one order: an item's bytes depend neither on the
 * rest of the batch nor on where the frames live.
 * uwspr_track_set: 1 <= n <= 4096 trajectories in HOST memory, qf, model; checked, designed on the host and uploaded before
 * anything of the context changes (UWSPR_ERR_ARG leaves the set before in place); it replaces the set before.
 * uwspr_track_batch: frames, items and `where` as for uwspr_blockdemod_batch: items are HOST memory whatever `where` says
 * and keep the rules of uwspr_subtract_batch; res [nitems] and surface [nitems][n nf] (binary32 T of every hypothesis; NULL:
 * not written) are host memory with UWSPR_HOST (complete on return), device memory with UWSPR_DEVICE (asynchronous on the
 * context's stream) and UWSPR_DEVICE_FRAMES (complete on return).  UWSPR_ERR_ARG before any launch, the outputs untouched:
 * an item that uwspr_subtract_batch would refuse, a call without a set, a device output outside a device allocation of the
 * context's device.  nitems = 0 is fine.
 * Not built: the fit is not fed back into the second pass's subtraction or into the fine search; there is no lag search
 * (a constant shift error costs every hypothesis alike); bearing, which one hydrophone cannot see.
 * In a pipe.  uwspr_pipe_set_tracks gives a pipe a trajectory set (n = 0 clears it; legal only while no batch is in flight,
 * as uwspr_pipe_set_list; UWSPR_ERR_ARG otherwise and for a set that breaks the rules, and nothing changes).  With a set,
 * every DECODED record -- of either pass, and decoded by Fano, "block", "osd", the list or the call search alike -- becomes
 * one item behind the host tail and the fallbacks: the symbols of the record's message, the jig_shift of the try that decoded,
 * f1 and drift1 as the second pass forms them (for a NONLINEAR candidate the constant f1 + slmFrequencyDrift(t = 0) the fine
 * search correlated with, without drift), over the frames that search read (the second pass's records: the residual
 * frames).  uwspr_decode has no free byte, so the fits leave by a door of their own: uwspr_pipe_collect_tracks never waits
 * and returns at most cap records {frame, cand, channel, pass, result} in the order of the decoded records; each becomes
 * available no later than its decode record (both are emitted under one lock, the track records first).  K15's time counts
 * in resume_s.  Without a set nothing of K15 runs or is allocated, and every record and statistic is what it was. */
#define UWSPR_TRACK_MAX 4096
#define UWSPR_TRACK_QF_MAX 16
typedef struct uwspr_track_traj {
  double v, d, tc;   /* m/s, m, s */
} uwspr_track_traj;
typedef struct uwspr_track_result {
  int32_t best;      /* h of the first maximum; trajectory best / nf, offset q = best % nf - qf */
  float t_best, t_ref;
  float f_hz;        /* f_hz + 0.0125 q */
} uwspr_track_result;
int uwspr_track_design(const uwspr_track_traj *traj, int n, int model, double cf, double *dfreq /*[n][162]*/, int32_t *tau /*[n][162]*/);
int uwspr_track_from_slm(double v1, double v2, double p1, double p2, double t_first, uwspr_track_traj *out);
int uwspr_track_set(uwspr_ctx *ctx, const uwspr_track_traj *traj, int n, int qf, int model);
int uwspr_track_batch(uwspr_ctx *ctx, const float *frames, int B, int where, const uwspr_sub_item *items, int nitems,
                      uwspr_track_result *res, float *surface /*[nitems][n nf] or NULL*/);
typedef struct uwspr_track_record {
  int64_t frame;     /* uwspr_decode.frame, .cand, .channel and .pass of the decoded record this fit belongs to */
  int32_t cand;
  int16_t channel;
  uint8_t pass, _pad;
  uwspr_track_result result;
} uwspr_track_record;
int uwspr_pipe_set_tracks(uwspr_pipe *pipe, const uwspr_track_traj *traj, int n, int qf, int model);
int uwspr_pipe_collect_tracks(uwspr_pipe *pipe, uwspr_track_record *out, int cap);

/* ---- decode a moving source: soft symbols along straight-line passes (K16, k16_follow.hip) ----------------------------- */
/* The fine search holds a candidate at one frequency plus a linear drift.  A source whose closest point of approach falls
 * in mid-transmission sweeps an S-curve of more than a tone spacing, and no (f, drift) pair follows it: Fano times out on
 * every try.  K16 demodulates such a record BLIND -- no symbol is known -- along the passes of a trajectory set, K15's
 * tables (uwspr_track_design: dfreq, tau) removing the motion, over a grid of frequency offsets and lags, scores every
 * hypothesis with the fine search's own sync metric and hands out the soft symbols of the best one.  The reference has no
 * counterpart; tests/follow_exact.py restates this text in binary64.  Binary32 with fused multiply-adds on the device;
 * every phase and index in binary64 or integers.
 * Constants: df = 375/256; Q = df / 8 = 375/2048 Hz, the frequency step; LSTEP = 32 samples, the lag step; pr3[i] = the
 * sync bit of symbol i (the LSB of any uwspr_wspr_symbols).
 * The set (uwspr_follow_set): 1 <= n <= 4096 trajectories (uwspr_track_traj, K15's rules), 0 <= qf <= 16 (nf = 2 qf + 1
 * offsets q = -qf .. qf), 0 <= nl <= 4 (nlg = 2 nl + 1 lags l = -nl .. nl), model UWSPR_TX_DOPPLER or UWSPR_TX_DELAY; its
 * tables are exactly uwspr_track_design's with cf = uwspr_params.cf.  K15's rules: checked and designed on the host before
 * anything of the context changes, UWSPR_ERR_ARG leaves the set before in place, read-only once built.
 * An item is a uwspr_block_item under uwspr_blockdemod_batch's rules: frame, shift s, f_hz; drift_hz is used by s_ref alone.
 * Grid powers, for trajectory j, lag l, symbol i and grid index g = -(qf + 12) .. qf + 12:
 *     f = (f_hz + dfreq[j][i]) + g Q                                                              (binary64, this order)
 *     P_i(j, l)[g] = | sum_{k < 256} x[s + 32 l + 256 i + tau[j][i] + k] e^{-j 2 pi f k / 375} |
 * Samples outside [0, fl) count as 0 (K15's rule); the phasor starts at (1, 0) in every symbol.
 * A hypothesis is h = (j nf + (q + qf)) nlg + (l + nl).  Tone t = 0..3 of symbol i is p_i[t] = P_i(j, l)[q + 8 t - 12]: the
 * tone offsets (t - 1.5) df lie on the grid.  The score is the fine search's sync metric,
 *     S(h) = sum_i (2 pr3[i] - 1) ((p_i[1] + p_i[3]) - (p_i[0] + p_i[2])) / sum_i (((p_i[0] + p_i[1]) + p_i[2]) + p_i[3]),
 * both sums in ascending i with one owner each; 0 when the denominator is 0.
 * best = the first maximum of S in ascending h (K8's rule: the walk moves on `>` alone, a NaN is never moved to and a NaN
 * S(0) is never left).  s_ref is the same S for the item's own linear model through the same code: f_i = f_hz +
 * (drift_hz / 2)(i - 81) / 81, tau = 0, l = 0, q = 0; a v = 0 trajectory at q = 0, l = 0 of an item with drift 0 gives the
 * bytes of s_ref.
 * Soft symbols at best: soft[i] = p_i[pr3[i] + 2] - p_i[pr3[i]], normalised and written as K10's text says (fsum, f2sum,
 * fac = sqrt(f2sum - fsum^2), v = 50 soft / fac clipped to [-128, 127], byte = (uint8)(v + 128); a fac that is no positive
 * finite number gives 128 in every byte), interleaved as uwspr_demod_out.symbols[idt] holds a vector.
 * Result per item: best; s_best = S(best); s_ref; f_hz = f_hz + Q q_best, formed in binary64 and rounded to binary32.  The
 * trajectory is best / (nf nlg), q = (best / nlg) % nf - qf, l = best % nlg - nl.
 * uwspr_follow_batch: frames, items and `where` as for uwspr_track_batch (items in HOST memory whatever `where` says); res
 * [nitems], symbols [nitems][162] and surface [nitems][n nf nlg] (binary32 S of every hypothesis; NULL: not written) are
 * host memory with UWSPR_HOST (complete on return), device memory with UWSPR_DEVICE (asynchronous on the context's stream)
 * and UWSPR_DEVICE_FRAMES (complete on return).  UWSPR_ERR_ARG before any launch, the outputs untouched: an item that
 * uwspr_blockdemod_batch would refuse, a call without a set, a device output outside a device allocation of the context's
 * device.  nitems = 0 is fine.  Every sum has one owner and one order: an item's bytes depend neither on the rest of the
 * batch nor on where the frames live.
 * In a pipe.  uwspr_pipe_set_follow gives a pipe a follow set (n = 0 clears it; legal only while no batch is in flight, as
 * uwspr_pipe_set_tracks; UWSPR_ERR_ARG otherwise and for a set that breaks the rules -- qf, nl and model are checked with
 * n = 0 as well --, and nothing changes).  With a set, behind "block" and before the list search -- the blind methods first -- every record that Fano gave up on becomes an item
 * by the fallbacks' common rule (the gated try with the largest jig_sync): that try's jig_shift, f and drift as for "block".
 * The record becomes a decoded one when s_best > 0.12 (strict: a NaN fails), the rms of the bytes about 128 is above the
 * fine search's gate (cc:470), and the bytes go through de-interleave, Fano (60, 10000) and uwspr_unpack_message; then
 * decoded = 1, idt = the picked try and osd = 4.  The Fano call counts in the statistics, the time in resume_s.  The fit
 * leaves by uwspr_pipe_collect_follows -- K15's door, copied: records {frame, cand, channel, pass, result} in the order of
 * the records that K16 decoded, each available no later than its decode record.  When the pipe also has a trajectory set
 * (uwspr_pipe_set_tracks), K15's item of a record that K16 decoded is taken at shift s + 32 l_best and f = result.f_hz with
 * drift 0; no other record's item changes.  Without a follow set nothing of K16 runs or is allocated, and every record,
 * statistic and byte is what it was.
 * Not built: the second pass ("passes" = 2) subtracts a record that K16 decoded with the linear model, as it does any
 * decoded record; the chirp inside a symbol; bearing. */
#define UWSPR_FOLLOW_QF_MAX 16
#define UWSPR_FOLLOW_NL_MAX 4
typedef struct uwspr_follow_result {
  int32_t best;      /* h of the first maximum */
  float s_best, s_ref;
  float f_hz;        /* f_hz + (375/2048) q */
} uwspr_follow_result;
int uwspr_follow_set(uwspr_ctx *ctx, const uwspr_track_traj *traj, int n, int qf, int nl, int model);
int uwspr_follow_batch(uwspr_ctx *ctx, const float *frames, int B, int where, const uwspr_block_item *items, int nitems,
                       uwspr_follow_result *res, uint8_t *symbols /*[nitems][162]*/, float *surface /*[nitems][n nf nlg] or NULL*/);
typedef struct uwspr_follow_record {
  int64_t frame;     /* uwspr_decode.frame, .cand, .channel and .pass of the record K16 decoded */
  int32_t cand;
  int16_t channel;
  uint8_t pass, _pad;
  uwspr_follow_result result;
} uwspr_follow_record;
int uwspr_pipe_set_follow(uwspr_pipe *pipe, const uwspr_track_traj *traj, int n, int qf, int nl, int model);
int uwspr_pipe_collect_follows(uwspr_pipe *pipe, uwspr_follow_record *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* UWSPR_HIP_H */
