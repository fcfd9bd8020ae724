// K10 -- block demodulation: soft symbols from complex tone correlations summed coherently over 1, 2 and 3 neighbouring
// symbols (uwspr_blockdemod_batch; the pipe's option "block").  The reference has no counterpart (its soft symbols are
// per-symbol magnitudes, sync_and_demodulate_impl.cc:240-254): the definition is this project's, in include/uwspr_hip.h,
// and tests/blockdemod_exact.py restates it in binary64.  Binary32 with fused multiply-adds; every phase in binary64.
//
// One workgroup of three wavefronts per item (frame, shift, f, drift).  Lane i < 162 owns symbol i: it walks the symbol's
// 256 samples once, for all four tones.  The samples come through LDS in chunks of 16 per symbol -- the loads are 128-byte
// runs of the frame, the row pitch of 17 pairs puts the 32 lanes of a 64-bit read's group on different banks -- so the
// 330 KB an item reads cross HBM / L2 once.  Sample k of symbol i is first turned by the base phasor e^{-j 2 pi (f_i - 1.5 df) k / 375}
// (its phase reduced in binary64, sincospi), then added to tone j's sum through the 256th root of unity
// e^{-j 2 pi j k / 256} of a table in LDS that every lane reads at the same address.  z[4][162] stays in LDS; the 162 / 81 /
// 54 blocks, their 2 / 4 / 8 data sequences, the two 162-term means (one lane each, ascending order, binary64) and the
// bytes follow in the same workgroup.  Every sum has one owner and a fixed order: an item's bytes depend on nothing else
// in the batch.  33 KB of LDS per workgroup (22 KB of it the sample chunk): four are resident in a CU's 160 KB.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K10_NSYM = UWSPR_NSYM, K10_SPB = 256, K10_WG = 192;
constexpr int K10_C = 16, K10_P = K10_C + 1;   // samples of a symbol per chunk, row pitch in LDS (odd: rows fall in different banks)
constexpr double K10_FS = 375.0, K10_DF = 375.0 / 256.0;
static_assert(K10_SPB % K10_C == 0 && K10_WG >= K10_NSYM, "K10 geometry");

__device__ __forceinline__ double k10_sym_freq(float f, float drift, int i) {
  return (double)f + 0.5 * (double)drift * ((double)(i - 81) / 81.0);
}
// e^{-j 2 pi t}, t in turns
__device__ __forceinline__ float2 k10_phasor(double t) {
  double sn, cs;
  t -= rint(t);
  sincospi(-2.0 * t, &sn, &cs);
  return make_float2((float)cs, (float)sn);
}
__device__ __forceinline__ float2 k10_mul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ void k10_mac(float2 &acc, float2 a, float2 b) {
  acc.x = fmaf(a.x, b.x, acc.x); acc.x = fmaf(-a.y, b.y, acc.x);
  acc.y = fmaf(a.x, b.y, acc.y); acc.y = fmaf(a.y, b.x, acc.y);
}
__device__ __forceinline__ float k10_abs(float2 a) { return sqrtf(fmaf(a.x, a.x, a.y * a.y)); }
__device__ __forceinline__ float k10_abs2(float2 a, float2 b) { return k10_abs(make_float2(a.x + b.x, a.y + b.y)); }
// the larger of two P, a NaN if either is one (fmaxf would return the other operand): the block's soft values are then NaN
__device__ __forceinline__ float k10_max(float a, float b) { return (a >= b || a != a) ? a : b; }

// out [item][3][162]
__global__ __launch_bounds__(K10_WG) void k10_blockdemod(const float2 *__restrict__ frames, size_t stride, int np,
                                                         const uwspr_block_item *__restrict__ items, uint8_t *__restrict__ out) {
  __shared__ float2 xs[K10_NSYM * K10_P];
  __shared__ float2 root[K10_SPB];
  __shared__ float2 z[4][K10_NSYM];
  __shared__ float2 r1[K10_NSYM], r2[K10_NSYM];   // e^{-j theta_i}, e^{-j (theta_i + theta_{i+1})}
  __shared__ float soft[3][K10_NSYM];
  __shared__ double fac[3];
  const int tid = threadIdx.x, it = blockIdx.x;
  const uwspr_block_item I = items[it];
  const float2 *__restrict__ x = frames + (size_t)I.frame * stride;
  const int shift = I.shift;
  for (int m = tid; m < K10_SPB; m += K10_WG) root[m] = k10_phasor((double)m / 256.0);
  const bool own = tid < K10_NSYM;
  const double fi = k10_sym_freq(I.f_hz, I.drift_hz, tid);
  const double fb = (fi - 1.5 * K10_DF) / K10_FS;   // turns per sample of the lowest tone
  float2 z0 = make_float2(0.0f, 0.0f), z1 = z0, z2 = z0, z3 = z0;
  for (int c0 = 0; c0 < K10_SPB; c0 += K10_C) {
    for (int e = tid; e < K10_NSYM * K10_C; e += K10_WG) {
      const int i = e / K10_C, k = e - i * K10_C;
      const int n = shift + K10_SPB * i + c0 + k;   // |shift| <= 2^20: no overflow
      xs[i * K10_P + k] = (n > 0 && n < np) ? x[n] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    if (own) {
      const float2 *xr = xs + tid * K10_P;
      for (int k = 0; k < K10_C; k++) {
        const int kk = c0 + k;
        const float2 y = k10_mul(xr[k], k10_phasor(fb * (double)kk));
        z0.x += y.x; z0.y += y.y;
        k10_mac(z1, y, root[kk]);
        k10_mac(z2, y, root[(2 * kk) & 255]);
        k10_mac(z3, y, root[(3 * kk) & 255]);
      }
    }
    __syncthreads();
  }
  if (own) {
    z[0][tid] = z0; z[1][tid] = z1; z[2][tid] = z2; z[3][tid] = z3;
    // theta_i / 2 pi = f_i 256 / 375 + 1/2 turns
    const double t0 = fi * ((double)K10_SPB / K10_FS) + 0.5;
    const double t1 = k10_sym_freq(I.f_hz, I.drift_hz, tid + 1) * ((double)K10_SPB / K10_FS) + 0.5;
    r1[tid] = k10_phasor(t0);
    r2[tid] = k10_phasor(t0 + t1);
  }
  __syncthreads();
  if (own) {   // n = 1
    const int p = pr3_bit(tid);
    soft[0][tid] = k10_abs(z[p + 2][tid]) - k10_abs(z[p][tid]);
  }
  if (tid < K10_NSYM / 2) {   // n = 2: block tid covers symbols i0, i0 + 1
    const int i0 = 2 * tid, p0 = pr3_bit(i0), p1 = pr3_bit(i0 + 1);
    const float2 a0 = z[p0][i0], a1 = z[p0 + 2][i0];
    const float2 b0 = k10_mul(z[p1][i0 + 1], r1[i0]), b1 = k10_mul(z[p1 + 2][i0 + 1], r1[i0]);
    const float P00 = k10_abs2(a0, b0), P01 = k10_abs2(a0, b1), P10 = k10_abs2(a1, b0), P11 = k10_abs2(a1, b1);
    soft[1][i0] = k10_max(P10, P11) - k10_max(P00, P01);
    soft[1][i0 + 1] = k10_max(P01, P11) - k10_max(P00, P10);
  }
  if (tid < K10_NSYM / 3) {   // n = 3: block tid covers symbols i0 .. i0 + 2
    const int i0 = 3 * tid, p0 = pr3_bit(i0), p1 = pr3_bit(i0 + 1), p2 = pr3_bit(i0 + 2);
    float2 a[2], b[2], c[2];
    a[0] = z[p0][i0]; a[1] = z[p0 + 2][i0];
    b[0] = k10_mul(z[p1][i0 + 1], r1[i0]); b[1] = k10_mul(z[p1 + 2][i0 + 1], r1[i0]);
    c[0] = k10_mul(z[p2][i0 + 2], r2[i0]); c[1] = k10_mul(z[p2 + 2][i0 + 2], r2[i0]);
    float m[3][2];
#pragma unroll
    for (int q = 0; q < 3; q++) { m[q][0] = 0.0f; m[q][1] = 0.0f; }   // (P >= 0)
#pragma unroll
    for (int d = 0; d < 8; d++) {
      const int d0 = d & 1, d1 = (d >> 1) & 1, d2 = d >> 2;
      const float2 s = make_float2(a[d0].x + b[d1].x, a[d0].y + b[d1].y);
      const float P = k10_abs2(s, c[d2]);
      m[0][d0] = k10_max(m[0][d0], P); m[1][d1] = k10_max(m[1][d1], P); m[2][d2] = k10_max(m[2][d2], P);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) soft[2][i0 + q] = m[q][1] - m[q][0];
  }
  __syncthreads();
  if ((tid & 63) == 0) {   // the first lane of wavefront n owns vector n's two means
    const float *s = soft[tid >> 6];
    double fsum = 0.0, f2sum = 0.0;
    for (int i = 0; i < K10_NSYM; i++) {
      const double v = (double)s[i];
      fsum += v / 162.0;
      f2sum += v * v / 162.0;
    }
    fac[tid >> 6] = sqrt(f2sum - fsum * fsum);
  }
  __syncthreads();
  if (own) {
#pragma unroll
    for (int n = 0; n < 3; n++) {
      const double fc = fac[n];
      uint8_t byte = 128;
      if (fc > 0.0 && fc - fc == 0.0) {   // a positive finite number
        double v = 50.0 * (double)soft[n][tid] / fc;
        v = v > 127.0 ? 127.0 : v;
        v = v < -128.0 ? -128.0 : v;
        byte = (v == v) ? (uint8_t)(int)(v + 128.0) : (uint8_t)128;
      }
      out[((size_t)it * 3 + n) * K10_NSYM + tid] = byte;
    }
  }
}

// ---------------------------------------------------------------- host side
struct blk_state {
  uwspr_block_item *d_items = nullptr; size_t cap_items = 0;
  // the caller's items go through page-locked memory of the context, so that a call only enqueues: the one wait is for the
  // K10 launch of the call before (`done`, behind which both item buffers are free again), never for the whole stream --
  // lanes of a pipe share streams, and a stream synchronisation would wait for the other lane's batch as well
  uwspr_block_item *h_items = nullptr; size_t cap_h = 0;
  hipEvent_t done = nullptr; bool pending = false;
  uint8_t *d_out = nullptr; size_t cap_out = 0;
  launch_timer timer;   // uwspr_debug_blockdemod_time: events around the K10 launch of the last call
};

void blk_release(uwspr_ctx *c) {
  if (!c || !c->blk) return;
  blk_state *t = c->blk;
  if (t->d_items) (void)hipFree(t->d_items);
  if (t->d_out) (void)hipFree(t->d_out);
  if (t->h_items) (void)hipHostFree(t->h_items);
  if (t->done) (void)hipEventDestroy(t->done);
  t->timer.release();
  delete t;
  c->blk = nullptr;
}

static bool blk_finite(float v) { return v == v && v - v == 0.0f; }

// what makes a list of items acceptable (the rules of subtract_check): checked before anything is launched or written
int blockdemod_check(uwspr_ctx *c, const uwspr_block_item *items, int nitems, int nframes) {
  if (nitems < 0 || (nitems > 0 && !items)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: items %p, nitems %d", (const void *)items, nitems);
  for (int i = 0; i < nitems; i++) {
    const uwspr_block_item &s = items[i];
    if (s.frame < 0 || s.frame >= nframes) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: item %d: frame %d (0..%d)", i, s.frame, nframes - 1);
    if (i > 0 && s.frame < items[i - 1].frame)
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: item %d: frame %d after frame %d (items are sorted by frame)", i, s.frame, items[i - 1].frame);
    if (!blk_finite(s.f_hz) || !blk_finite(s.drift_hz) || fabsf(s.f_hz) > 1e4f || fabsf(s.drift_hz) > 1e3f)
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: item %d: f %g Hz (|.| <= 1e4), drift %g Hz (|.| <= 1e3)", i, (double)s.f_hz, (double)s.drift_hz);
    if (s.shift < -(1 << 20) || s.shift > (1 << 20)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: item %d: shift %d (|.| <= 2^20)", i, s.shift);
  }
  return UWSPR_OK;
}

// The launch, on the context's stream.  src: device frames, frame b at src + 2 stride b floats.  items: host records that
// passed blockdemod_check, nitems > 0.  out: device memory [nitems][3][162], or null = a buffer of the context handed back
// through *out_dev.
int blockdemod_run(uwspr_ctx *c, const float *src, size_t stride, const uwspr_block_item *items, int nitems, uint8_t *out,
                   uint8_t **out_dev) {
  int rc = ctx_device_ready(c);
  if (rc) return rc;
  if (!c->blk) c->blk = new blk_state();
  blk_state *t = c->blk;
  if ((rc = ctx_grow(c, &t->d_items, &t->cap_items, (size_t)nitems))) return rc;
  if (!out) {
    if ((rc = ctx_grow(c, &t->d_out, &t->cap_out, (size_t)nitems * 3 * K10_NSYM))) return rc;
    out = t->d_out;
  }
  if (out_dev) *out_dev = out;
  if (!t->done) CTXCHK(c, hipEventCreateWithFlags(&t->done, hipEventDisableTiming));
  if (t->pending) { CTXCHK(c, hipEventSynchronize(t->done)); t->pending = false; }   // the call before has read both item buffers
  if ((size_t)nitems > t->cap_h) {
    if (t->h_items) { CTXCHK(c, hipHostFree(t->h_items)); t->h_items = nullptr; t->cap_h = 0; }
    const size_t n = nitems > 256 ? (size_t)nitems : 256;
    if (hipHostMalloc((void **)&t->h_items, n * sizeof(uwspr_block_item), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      t->h_items = nullptr;
      return ctx_fail(c, UWSPR_ERR_NOMEM, "hipHostMalloc(%zu bytes) for the items", n * sizeof(uwspr_block_item));
    }
    t->cap_h = n;
  }
  memcpy(t->h_items, items, (size_t)nitems * sizeof(uwspr_block_item));
  CTXCHK(c, hipMemcpyAsync(t->d_items, t->h_items, (size_t)nitems * sizeof(uwspr_block_item), hipMemcpyHostToDevice, c->stream));
  if ((rc = t->timer.begin(c))) return rc;
  // c->np: the fine search's sample bound, min(fl, 45000) -- 45000 for every fl that holds a whole frame
  hipLaunchKernelGGL(k10_blockdemod, dim3((unsigned)nitems), dim3(K10_WG), 0, c->stream, reinterpret_cast<const float2 *>(src), stride,
                     c->np, t->d_items, out);
  CTXCHK(c, hipGetLastError());
  CTXCHK(c, hipEventRecord(t->done, c->stream));
  t->pending = true;
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_blockdemod_batch(uwspr_ctx *c, const float *frames, int B, int where, const uwspr_block_item *items, int nitems,
                                      uint8_t *symbols) {
  if (!c) return UWSPR_ERR_ARG;
  if (!frames || B <= 0 || (where != UWSPR_HOST && where != UWSPR_DEVICE && where != UWSPR_DEVICE_FRAMES) || (nitems > 0 && !symbols))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: frames %p, B %d, where %d, symbols %p", (const void *)frames, B, where, (void *)symbols);
  int rc = blockdemod_check(c, items, nitems, B);
  if (rc) return rc;
  if (nitems == 0) return UWSPR_OK;
  if ((rc = ctx_device_ready(c))) return rc;
  const size_t bytes = (size_t)nitems * 3 * K10_NSYM;
  if (where != UWSPR_HOST && !ctx_device_range(c, symbols, bytes))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_blockdemod_batch: device output needs symbols (%zu bytes) inside a device allocation of device %d", bytes, c->device);
  const float *src = nullptr;
  if ((rc = api_frames_on_device(c, frames, B, where, &src))) return rc;
  uint8_t *dev = nullptr;
  if ((rc = blockdemod_run(c, src, (size_t)c->fstride, items, nitems, where == UWSPR_HOST ? nullptr : symbols, &dev))) return rc;
  if (where == UWSPR_HOST) CTXCHK(c, hipMemcpyAsync(symbols, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  if (where != UWSPR_DEVICE) CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// Measurement hook of tools/blockdemod_probe.py (not part of the ABI, like uwspr_debug_osd_time): enable = 1 / 0 switches
// HIP events around the K10 launch of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
// timed launch and returns its time.
extern "C" int uwspr_debug_blockdemod_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->blk) c->blk = new blk_state();   // (no device asked: the hook only keeps the switch)
  return c->blk->timer.read(c, enable, ms);
}
