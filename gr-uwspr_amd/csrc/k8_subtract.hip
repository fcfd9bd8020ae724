// K8 -- known-symbol subtraction: a decoded transmission is rebuilt from its 162 channel symbols, fitted to the samples
// and taken out of them, so that what lay under it can be searched (uwspr_subtract_batch; the second pass of
// uwspr_pipe_*).  The reference has no counterpart (lib/ holds no subtraction): the definitions are this project's, in
// include/uwspr_hip.h, and tests/test_gpu_subtract.py restates them in binary64.  Binary32 with fused multiply-adds;
// every phase in binary64.
//
// An item is (frame, symbols s[162], f Hz, shift samples, drift Hz); symbol i has the frequency of the receiver's own
// LINEAR model,  f_i = f + (drift / 2)(i - 81) / 81 + (s_i - 1.5) 375/256.
//
// k8_refine: M(l, q) = sum_i | sum_{k < 256} x[shift + l + 256 i + k] e^{-j 2 pi (f_i + 0.0125 q) k / 375} | for the 49
// lags l = -24..24 and the 9 offsets q = -4..4.  A workgroup of two wavefronts owns 18 symbols of one item (9 workgroups
// per item: 2304 of them for a batch of 256, 5 resident per CU by LDS); a wavefront stages one symbol's 256 + 48 samples
// and its 256 phasors of q = 0 in LDS once for all 441 hypotheses.  Lane 7 q' + g owns offset q' and the seven lags
// 7 g .. 7 g + 6: the samples slide through an eight-deep register ring, the phasor of (q', k) is the symbol's one
// times the workgroup's table e^{-j 2 pi 0.0125 q k / 375} and is shared by the lane's seven lags -- 28 FMAs for three
// LDS reads.  Partial sums go to HBM per workgroup and k8_pick adds the nine in ascending order (the bytes do not depend
// on the batch), takes the first maximum in (q, l) order and lays out the item's per-symbol phase table for k8_cancel.
//
// k8_cancel: r[k] = e^{j theta(k)} (continuous phase, exclusive sum of 2 pi f_i / 375 from per-symbol prefix sums),
// c[k] = x[shift' + k] conj r[k], a[k] = (1023-tap Hann-weighted mean of c around k over the samples that exist),
// y[k] = a[k] r[k].  A workgroup of nine wavefronts owns 4608 outputs of one item (9 workgroups per item) with the 511
// samples on either side in LDS, stored [k mod 8][k div 8] so that the 64 lanes of a read hit consecutive words; a lane
// owns eight consecutive outputs and a sixteen-sample register window, as K7's FIR does: 128 FMAs per 8 LDS reads.
// y goes to scratch and k8_apply takes it out of the frame (a workgroup's halo is its neighbour's output).  Items of one
// frame apply in list order, each fitted to the residual the one before left: one round of launches per rank in a frame.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K8_NSYM = UWSPR_NSYM, K8_SPB = 256, K8_N = K8_NSYM * K8_SPB;   // 41472 samples per transmission
constexpr double K8_FS = 375.0, K8_DF = 375.0 / 256.0, K8_DFQ = 0.0125;
constexpr int K8_LAG = 24, K8_NLAG = 2 * K8_LAG + 1, K8_Q = 4, K8_NQ = 2 * K8_Q + 1, K8_NHYP = K8_NLAG * K8_NQ;   // 441
constexpr int K8_PARTS = 9, K8_RSYM = 9;         // refine: workgroups per item, symbols per wavefront (9 x 2 x 9 = 162)
constexpr int K8_XS = 312;                       // staged samples per symbol: 256 + 48 and the ring's read-ahead, padded
constexpr int K8_DQP = 257;                      // row pitch of the offset phasor table (rows fall in different banks)
constexpr int K8_TAPS = 1023, K8_HALF = 511;
constexpr int K8_CWG = 576, K8_CR = 8;           // cancel: threads per workgroup, outputs per lane
constexpr int K8_TILE = K8_CWG * K8_CR;          // 4608 outputs per workgroup
constexpr int K8_TILES = K8_N / K8_TILE;         // 9
constexpr int K8_G = (K8_TILE + 1024) / 8 + 1;   // LDS column groups of 8 samples (704 used; odd pitch)
static_assert(K8_TILES * K8_TILE == K8_N && K8_PARTS * 2 * K8_RSYM == K8_NSYM, "K8 geometry");

// what k8_pick leaves for k8_cancel / k8_apply: the fitted (f', shift'), the k range [lo, hi) that lies in the frame, and
// the phase in turns: theta(256 i + r) / 2 pi = ph[i] + r w[i]
struct sub_dstate {
  float f; int32_t shift; float metric; int32_t lo, hi, _pad;
  double w[K8_NSYM], ph[K8_NSYM];
};

__device__ __forceinline__ double k8_sym_freq(float f, float drift, int i, int s) {
  return (double)f + 0.5 * (double)drift * ((double)(i - 81) / 81.0) + ((double)s - 1.5) * K8_DF;
}

// slot s of the output <- frame map[s] (or s) of the input
__global__ void k8_copy(const float2 *__restrict__ src, size_t stride, const int *__restrict__ map, float2 *__restrict__ dst, int fl) {
  const int s = blockIdx.y;
  const size_t b = map ? (size_t)map[s] : (size_t)s;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < fl; i += gridDim.x * blockDim.x)
    dst[(size_t)s * fl + i] = src[b * stride + i];
}

__global__ __launch_bounds__(128) void k8_refine(const float2 *__restrict__ frames, int fl, const uwspr_sub_item *__restrict__ items,
                                                 const int *__restrict__ order, float *__restrict__ part) {
  __shared__ float2 dq[K8_NQ * K8_DQP];
  __shared__ float2 xs[2][K8_XS];
  __shared__ float2 pb[2][K8_SPB];
  __shared__ float ms[2][448];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int it = order[blockIdx.y], p = blockIdx.x;
  const uwspr_sub_item &I = items[it];
  const float2 *__restrict__ x = frames + (size_t)I.frame * fl;
  const float f = I.f_hz, drift = I.drift_hz;
  const int shift = I.shift;
  for (int e = tid; e < K8_NQ * K8_SPB; e += 128) {
    const int q = e >> 8, k = e & 255;
    double sn, cs;
    sincospi(-2.0 * (K8_DFQ * (double)(q - K8_Q) / K8_FS) * (double)k, &sn, &cs);
    dq[q * K8_DQP + k] = make_float2((float)cs, (float)sn);
  }
  const int q = lane / 7, g = lane - 7 * q;   // (lane 63 has no hypothesis)
  float m[7];
#pragma unroll
  for (int r = 0; r < 7; r++) m[r] = 0.0f;
  float2 *xw = xs[w], *pw = pb[w];
  for (int j = 0; j < K8_RSYM; j++) {
    const int i = (p * 2 + w) * K8_RSYM + j;
    const double fi = k8_sym_freq(f, drift, i, (int)I.symbols[i]) / K8_FS;
    const long long base = (long long)shift - K8_LAG + (long long)K8_SPB * i;
    for (int e = lane; e < K8_XS; e += 64) {
      const long long idx = base + e;
      xw[e] = (e < K8_SPB + 2 * K8_LAG && idx >= 0 && idx < fl) ? x[idx] : make_float2(0.0f, 0.0f);
    }
    for (int k = lane; k < K8_SPB; k += 64) {
      double t = -fi * (double)k, sn, cs;
      t -= rint(t);
      sincospi(2.0 * t, &sn, &cs);
      pw[k] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
    if (lane < 63) {
      const float2 *xg = xw + 7 * g, *dqq = dq + q * K8_DQP;
      float2 W[8];
      float re[7], im[7];
#pragma unroll
      for (int r = 0; r < 7; r++) { W[r] = xg[r]; re[r] = 0.0f; im[r] = 0.0f; }
      for (int k0 = 0; k0 < K8_SPB; k0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int k = k0 + u;
          W[(u + 7) & 7] = xg[k + 7];   // the next step's last lag (index <= 42 + 262 < K8_XS)
          const float2 b = pw[k], d = dqq[k];
          const float pr = fmaf(b.x, d.x, -(b.y * d.y)), pi = fmaf(b.x, d.y, b.y * d.x);
#pragma unroll
          for (int r = 0; r < 7; r++) {
            const float2 s = W[(u + r) & 7];   // x[shift + l + 256 i + k], l = 7 g + r - 24
            re[r] = fmaf(s.x, pr, re[r]); re[r] = fmaf(-s.y, pi, re[r]);
            im[r] = fmaf(s.x, pi, im[r]); im[r] = fmaf(s.y, pr, im[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 7; r++) m[r] += sqrtf(fmaf(re[r], re[r], im[r] * im[r]));
    }
    __syncthreads();
  }
  if (lane < 63) {
#pragma unroll
    for (int r = 0; r < 7; r++) ms[w][q * K8_NLAG + 7 * g + r] = m[r];
  }
  __syncthreads();
  for (int h = tid; h < K8_NHYP; h += 128) part[((size_t)it * K8_PARTS + p) * K8_NHYP + h] = ms[0][h] + ms[1][h];
}

// the nine partial sums in ascending order, the first maximum in (q, l) order, and the item's phase table
__global__ __launch_bounds__(64) void k8_pick(const uwspr_sub_item *__restrict__ items, const int *__restrict__ order,
                                              const float *__restrict__ part, int refine, int fl, sub_dstate *__restrict__ st) {
  __shared__ float M[K8_NHYP];
  __shared__ double wl[K8_NSYM];
  const int it = order[blockIdx.x], tid = threadIdx.x;
  const uwspr_sub_item &I = items[it];
  float f = I.f_hz, metric = 0.0f;
  int shift = I.shift;
  if (refine) {
    for (int h = tid; h < K8_NHYP; h += 64) {
      float s = 0.0f;
      for (int p = 0; p < K8_PARTS; p++) s += part[((size_t)it * K8_PARTS + p) * K8_NHYP + h];
      M[h] = s;
    }
    __syncthreads();
    int best = 0;
    float bm = M[0];
    for (int h = 1; h < K8_NHYP; h++)
      if (M[h] > bm) { bm = M[h]; best = h; }
    f = (float)((double)I.f_hz + K8_DFQ * (double)(best / K8_NLAG - K8_Q));
    shift = I.shift + best % K8_NLAG - K8_LAG;
    metric = bm;
  }
  for (int i = tid; i < K8_NSYM; i += 64) wl[i] = k8_sym_freq(f, I.drift_hz, i, (int)I.symbols[i]) / K8_FS;
  __syncthreads();
  sub_dstate &S = st[it];
  for (int i = tid; i < K8_NSYM; i += 64) S.w[i] = wl[i];
  if (tid == 0) {
    double ph = 0.0;
    for (int i = 0; i < K8_NSYM; i++) {
      S.ph[i] = ph;
      ph += (double)K8_SPB * wl[i];
      ph -= floor(ph);
    }
    S.f = f; S.shift = shift; S.metric = metric; S._pad = 0;
    S.lo = shift < 0 ? (-(long long)shift < K8_N ? -shift : K8_N) : 0;
    const long long hi = (long long)fl - shift;
    S.hi = hi < 0 ? 0 : (hi < K8_N ? (int)hi : K8_N);
  }
}

// NT taps of a block of eight: the last block has seven (there are 1023 taps, and a 1024th of weight 0 would still turn a
// NaN or an infinite sample 512 behind the output into a NaN)
template <int NT = 8>
__device__ __forceinline__ void k8_block(float2 (&acc)[K8_CR], const float2 (&A)[8], const float2 (&B)[8], const float *__restrict__ wt) {
#pragma unroll
  for (int u = 0; u < NT; u++) {
    const float t = wt[u];
#pragma unroll
    for (int r = 0; r < K8_CR; r++) {
      const float2 s = r + u < 8 ? A[r + u] : B[r + u - 8];
      acc[r].x = fmaf(t, s.x, acc[r].x);
      acc[r].y = fmaf(t, s.y, acc[r].y);
    }
  }
}

// workgroup (t, j): outputs k = 4608 t .. 4608 t + 4607 of item order[j]; y [j][N]; rem [item][9] = the tile's sum |y|^2
__global__ __launch_bounds__(K8_CWG) void k8_cancel(const float2 *__restrict__ frames, int fl, const uwspr_sub_item *__restrict__ items,
                                                    const int *__restrict__ order, const sub_dstate *__restrict__ st,
                                                    const float *__restrict__ taps, const double *__restrict__ cw,
                                                    float2 *__restrict__ y, float *__restrict__ rem) {
  __shared__ float2 cs[8 * K8_G];
  __shared__ float wt[1024];
  __shared__ double phs[K8_NSYM], ws[K8_NSYM];
  __shared__ float red[K8_CWG / 64];
  const int tid = threadIdx.x, j = blockIdx.y, it = order[j], k0 = blockIdx.x * K8_TILE;
  const sub_dstate &S = st[it];
  const int lo = S.lo, hi = S.hi, shift = S.shift;
  if (k0 >= hi || k0 + K8_TILE <= lo) {   // nothing of this tile lies in the frame
    if (tid == 0) rem[(size_t)it * K8_TILES + blockIdx.x] = 0.0f;
    return;
  }
  const float2 *__restrict__ x = frames + (size_t)items[it].frame * fl;
  for (int i = tid; i < K8_NSYM; i += K8_CWG) { phs[i] = S.ph[i]; ws[i] = S.w[i]; }
  for (int i = tid; i < 1024; i += K8_CWG) wt[i] = taps[i];
  __syncthreads();
  // c[k], k = k0 - 511 + e, column e at [e mod 8][e div 8]
  for (int e = tid; e < 8 * K8_G; e += K8_CWG) {
    const int k = k0 - K8_HALF + e;
    float2 c = make_float2(0.0f, 0.0f);
    if (e < K8_TILE + 2 * K8_HALF && k >= lo && k < hi) {
      const float2 xv = x[shift + k];
      double sn, cn;
      sincospi(2.0 * (phs[k >> 8] + (double)(k & 255) * ws[k >> 8]), &sn, &cn);
      const float cf = (float)cn, sf = (float)sn;
      c.x = fmaf(xv.x, cf, xv.y * sf);
      c.y = fmaf(xv.y, cf, -(xv.x * sf));
    }
    cs[(e & 7) * K8_G + (e >> 3)] = c;
  }
  __syncthreads();
  // output 8 tid + r = sum_m w[m] column(8 tid + r + m): tap block b reads column groups tid + b and tid + b + 1
  float2 acc[K8_CR], A[8], B[8];
#pragma unroll
  for (int r = 0; r < K8_CR; r++) acc[r] = make_float2(0.0f, 0.0f);
#pragma unroll
  for (int v = 0; v < 8; v++) A[v] = cs[v * K8_G + tid];
  for (int b = 0; b < 126; b += 2) {   // two blocks per trip: the window's halves swap roles, no copies
#pragma unroll
    for (int v = 0; v < 8; v++) B[v] = cs[v * K8_G + tid + b + 1];
    k8_block(acc, A, B, wt + 8 * b);
#pragma unroll
    for (int v = 0; v < 8; v++) A[v] = cs[v * K8_G + tid + b + 2];
    k8_block(acc, B, A, wt + 8 * b + 8);
  }
  {   // taps 1008 .. 1022
#pragma unroll
    for (int v = 0; v < 8; v++) B[v] = cs[v * K8_G + tid + 127];
    k8_block(acc, A, B, wt + 8 * 126);
#pragma unroll
    for (int v = 0; v < 8; v++) A[v] = cs[v * K8_G + tid + 128];   // (group <= 575 + 128 = 703)
    k8_block<7>(acc, B, A, wt + 8 * 127);
  }
  float rs = 0.0f;
#pragma unroll
  for (int r = 0; r < K8_CR; r++) {
    const int k = k0 + K8_CR * tid + r;
    if (k >= lo && k < hi) {
      // sum of the window over the samples that exist: k + m - 511 in [lo, hi)
      const int mlo = min(max(lo - k + K8_HALF, 0), K8_TAPS), mhi = min(max(hi - k + K8_HALF, 0), K8_TAPS);
      const float den = (float)(cw[mhi] - cw[mlo]);
      const float ax = acc[r].x / den, ay = acc[r].y / den;
      double sn, cn;
      sincospi(2.0 * (phs[k >> 8] + (double)(k & 255) * ws[k >> 8]), &sn, &cn);
      const float cf = (float)cn, sf = (float)sn;
      const float yx = fmaf(ax, cf, -(ay * sf)), yy = fmaf(ax, sf, ay * cf);
      y[(size_t)j * K8_N + k] = make_float2(yx, yy);
      rs += fmaf(yx, yx, yy * yy);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rs += __shfl_down(rs, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = rs;
  __syncthreads();
  if (tid == 0) {
    float s = 0.0f;
    for (int v = 0; v < K8_CWG / 64; v++) s += red[v];
    rem[(size_t)it * K8_TILES + blockIdx.x] = s;
  }
}

// frame -= y over [lo, hi), and the item's result record
__global__ void k8_apply(float2 *__restrict__ frames, int fl, const uwspr_sub_item *__restrict__ items, const int *__restrict__ order,
                         const sub_dstate *__restrict__ st, const float2 *__restrict__ y, const float *__restrict__ rem,
                         uwspr_sub_result *__restrict__ res) {
  const int j = blockIdx.y, it = order[j];
  const sub_dstate &S = st[it];
  float2 *__restrict__ x = frames + (size_t)items[it].frame * fl;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= S.lo && k < S.hi) {
    const float2 v = x[S.shift + k], s = y[(size_t)j * K8_N + k];
    x[S.shift + k] = make_float2(v.x - s.x, v.y - s.y);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.0f;
    for (int t = 0; t < K8_TILES; t++) s += rem[(size_t)it * K8_TILES + t];
    uwspr_sub_result r;
    r.f_hz = S.f; r.shift = S.shift; r.metric = S.metric; r.removed = s;
    res[it] = r;
  }
}

// ---------------------------------------------------------------- host side
struct sub_state {
  float *d_taps = nullptr;       // [1024] the Hann window in binary32, w[1023] = 0
  double *d_cw = nullptr;        // [1024] cw[j] = sum_{m < j} w[m] in binary64
  uwspr_sub_item *d_items = nullptr; size_t cap_items = 0;
  int *d_order = nullptr; size_t cap_order = 0;
  int *d_map = nullptr; size_t cap_map = 0;
  float *d_part = nullptr; size_t cap_part = 0;
  sub_dstate *d_st = nullptr; size_t cap_st = 0;
  float2 *d_y = nullptr; size_t cap_y = 0;
  float *d_rem = nullptr; size_t cap_rem = 0;
  uwspr_sub_result *d_res = nullptr; size_t cap_res = 0;
  float *d_out = nullptr; size_t cap_out = 0;   // host output staged
  // uwspr_debug_subtract_times: events around the k8_refine and the k8_cancel launch of every rank of the last call
  bool timing = false;
  std::vector<hipEvent_t> ev;   // four per rank: before / after k8_refine, before / after k8_cancel
  size_t ev_used = 0;
  // uwspr_debug_subtract_surface: what the last subtract_run left in d_part
  int last_items = 0;
  bool last_refine = false;
};

void sub_release(uwspr_ctx *c) {
  if (!c || !c->sub) return;
  sub_state *t = c->sub;
  void *bufs[] = {t->d_taps, t->d_cw, t->d_items, t->d_order, t->d_map, t->d_part, t->d_st, t->d_y, t->d_rem, t->d_res, t->d_out};
  for (void *b : bufs) if (b) (void)hipFree(b);
  for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
  delete t;
  c->sub = nullptr;
}

// (not ctx_grow: at least 64 elements, and no synchronisation -- sub_begin has synchronised the stream)
template <typename T>
static int sub_grow(uwspr_ctx *c, T **buf, size_t *cap, size_t elems) {
  if (elems <= *cap && *buf) return UWSPR_OK;
  if (*buf) { CTXCHK(c, hipFree(*buf)); *buf = nullptr; *cap = 0; }
  const size_t n = elems > 64 ? elems : 64;
  const hipError_t e = hipMalloc((void **)buf, n * sizeof(T));
  if (e != hipSuccess) return ctx_fail(c, UWSPR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e));
  *cap = n;
  return UWSPR_OK;
}

static int sub_begin(uwspr_ctx *c) {
  if (const int rc0 = ctx_device_ready(c)) return rc0;
  if (!c->sub) c->sub = new sub_state();
  CTXCHK(c, hipStreamSynchronize(c->stream));   // the scratch below may still be read by the previous call's kernels
  sub_state *t = c->sub;
  if (!t->d_taps) {
    // np.hanning(1025)[1:-1]: w[m] = 0.5 - 0.5 cos(2 pi (m + 1) / 1024), m = 0..1022
    std::vector<float> w(1024, 0.0f);
    std::vector<double> cw(1024, 0.0);
    double s = 0.0;
    for (int m = 0; m < K8_TAPS; m++) {
      const double v = 0.5 - 0.5 * cos(6.283185307179586476925286766559 * (double)(m + 1) / 1024.0);
      cw[m] = s;
      s += v;
      w[m] = (float)v;
    }
    cw[K8_TAPS] = s;
    CTXCHK(c, hipMalloc((void **)&t->d_cw, 1024 * sizeof(double)));
    CTXCHK(c, hipMemcpy(t->d_cw, cw.data(), 1024 * sizeof(double), hipMemcpyHostToDevice));
    float *d = nullptr;
    CTXCHK(c, hipMalloc((void **)&d, 1024 * sizeof(float)));
    t->d_taps = d;
    CTXCHK(c, hipMemcpy(d, w.data(), 1024 * sizeof(float), hipMemcpyHostToDevice));
  }
  return UWSPR_OK;
}

static bool sub_finite(float v) { return v == v && v - v == 0.0f; }

// what makes a list of items acceptable: sorted by frame, frames in [0, nframes), symbols 0..3, finite f and drift,
// a shift no kernel index can overflow on.  Checked before anything is launched or written.
int subtract_check(uwspr_ctx *c, const uwspr_sub_item *items, int nitems, int nframes) {
  if (nitems < 0 || (nitems > 0 && !items)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: items %p, nitems %d", (const void *)items, nitems);
  for (int i = 0; i < nitems; i++) {
    const uwspr_sub_item &s = items[i];
    if (s.frame < 0 || s.frame >= nframes) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: item %d: frame %d (0..%d)", i, s.frame, nframes - 1);
    if (i > 0 && s.frame < items[i - 1].frame)
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: item %d: frame %d after frame %d (items are sorted by frame)", i, s.frame, items[i - 1].frame);
    for (int k = 0; k < K8_NSYM; k++)
      if (s.symbols[k] > 3) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: item %d symbol %d = %d (0..3)", i, k, s.symbols[k]);
    if (!sub_finite(s.f_hz) || !sub_finite(s.drift_hz) || fabsf(s.f_hz) > 1e4f || fabsf(s.drift_hz) > 1e3f)
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: item %d: f %g Hz (|.| <= 1e4), drift %g Hz (|.| <= 1e3)", i, (double)s.f_hz, (double)s.drift_hz);
    if (s.shift < -(1 << 20) || s.shift > (1 << 20)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: item %d: shift %d (|.| <= 2^20)", i, s.shift);
  }
  return UWSPR_OK;
}

// The launches.  src: device frames, frame b at src + 2 stride b floats.  dst: device [nslots][fl]; slot s starts as input
// frame slot_frame[s] (null: s; src == dst: the frames are there already, nothing is copied).  items: host records that
// passed subtract_check against nslots, `frame` being the SLOT.  Results: the context's d_res [nitems], in item order.
int subtract_run(uwspr_ctx *c, const float *src, size_t stride, int nslots, const int *slot_frame, const uwspr_sub_item *items,
                 int nitems, int refine, float *dst) {
  int rc = sub_begin(c);
  if (rc) return rc;
  sub_state *t = c->sub;
  const int fl = c->fc.fl;
  t->last_items = 0;
  t->last_refine = false;
  std::vector<int> order;
  std::vector<int> rank_at;   // order[rank_at[r] .. rank_at[r + 1]): the items that are the r-th of their frame
  if (nitems > 0) {
    std::vector<int> rk(nitems);
    int nrank = 0;
    for (int i = 0; i < nitems; i++) {
      rk[i] = (i > 0 && items[i].frame == items[i - 1].frame) ? rk[i - 1] + 1 : 0;
      nrank = std::max(nrank, rk[i] + 1);
    }
    rank_at.assign(nrank + 1, 0);
    for (int i = 0; i < nitems; i++) rank_at[rk[i] + 1]++;
    for (int r = 0; r < nrank; r++) rank_at[r + 1] += rank_at[r];
    order.resize(nitems);
    std::vector<int> at(rank_at.begin(), rank_at.end() - 1);
    for (int i = 0; i < nitems; i++) order[at[rk[i]]++] = i;
    if ((rc = sub_grow(c, &t->d_items, &t->cap_items, (size_t)nitems))) return rc;
    if ((rc = sub_grow(c, &t->d_order, &t->cap_order, (size_t)nitems))) return rc;
    if (refine && (rc = sub_grow(c, &t->d_part, &t->cap_part, (size_t)nitems * K8_PARTS * K8_NHYP))) return rc;
    if ((rc = sub_grow(c, &t->d_st, &t->cap_st, (size_t)nitems))) return rc;
    if ((rc = sub_grow(c, &t->d_y, &t->cap_y, (size_t)rank_at[1] * K8_N))) return rc;
    if ((rc = sub_grow(c, &t->d_rem, &t->cap_rem, (size_t)nitems * K8_TILES))) return rc;
    if ((rc = sub_grow(c, &t->d_res, &t->cap_res, (size_t)nitems))) return rc;
    CTXCHK(c, hipMemcpyAsync(t->d_items, items, (size_t)nitems * sizeof(uwspr_sub_item), hipMemcpyHostToDevice, c->stream));
    CTXCHK(c, hipMemcpyAsync(t->d_order, order.data(), (size_t)nitems * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  if (slot_frame) {
    if ((rc = sub_grow(c, &t->d_map, &t->cap_map, (size_t)nslots))) return rc;
    CTXCHK(c, hipMemcpyAsync(t->d_map, slot_frame, (size_t)nslots * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  CTXCHK(c, hipStreamSynchronize(c->stream));   // (the records above live in the caller's and this call's host memory)
  float2 *out = reinterpret_cast<float2 *>(dst);
  if (src != dst) {
    hipLaunchKernelGGL(k8_copy, dim3((unsigned)((fl + 1023) / 1024), (unsigned)nslots), dim3(256), 0, c->stream,
                       reinterpret_cast<const float2 *>(src), stride, slot_frame ? t->d_map : (const int *)nullptr, out, fl);
    CTXCHK(c, hipGetLastError());
  }
  t->ev_used = 0;
  if (t->timing)
    while (t->ev.size() < 4 * (rank_at.empty() ? 0 : rank_at.size() - 1)) {
      hipEvent_t e;
      CTXCHK(c, hipEventCreate(&e));
      t->ev.push_back(e);
    }
  for (size_t r = 0; r + 1 < rank_at.size(); r++) {
    const int n = rank_at[r + 1] - rank_at[r];
    const int *ord = t->d_order + rank_at[r];
    hipEvent_t *ev = t->timing ? &t->ev[4 * r] : nullptr;
    if (ev) CTXCHK(c, hipEventRecord(ev[0], c->stream));
    if (refine) hipLaunchKernelGGL(k8_refine, dim3(K8_PARTS, (unsigned)n), dim3(128), 0, c->stream, out, fl, t->d_items, ord, t->d_part);
    if (ev) CTXCHK(c, hipEventRecord(ev[1], c->stream));
    hipLaunchKernelGGL(k8_pick, dim3((unsigned)n), dim3(64), 0, c->stream, t->d_items, ord, t->d_part, refine ? 1 : 0, fl, t->d_st);
    if (ev) CTXCHK(c, hipEventRecord(ev[2], c->stream));
    hipLaunchKernelGGL(k8_cancel, dim3(K8_TILES, (unsigned)n), dim3(K8_CWG), 0, c->stream, out, fl, t->d_items, ord, t->d_st,
                       t->d_taps, t->d_cw, t->d_y, t->d_rem);
    if (ev) { CTXCHK(c, hipEventRecord(ev[3], c->stream)); t->ev_used = 4 * (r + 1); }
    hipLaunchKernelGGL(k8_apply, dim3(K8_N / 256, (unsigned)n), dim3(256), 0, c->stream, out, fl, t->d_items, ord, t->d_st, t->d_y,
                       t->d_rem, t->d_res);
    CTXCHK(c, hipGetLastError());
  }
  t->last_items = nitems;
  t->last_refine = refine != 0;
  return UWSPR_OK;
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_subtract_batch(uwspr_ctx *c, const float *frames, int B, int where, const uwspr_sub_item *items, int nitems,
                                    int refine, float *frames_out, uwspr_sub_result *res) {
  if (!c) return UWSPR_ERR_ARG;
  if (!frames || !frames_out || B <= 0 || (where != UWSPR_HOST && where != UWSPR_DEVICE && where != UWSPR_DEVICE_FRAMES))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: frames %p, frames_out %p, B %d, where %d", (const void *)frames,
                    (void *)frames_out, B, where);
  int rc = subtract_check(c, items, nitems, B);
  if (rc) return rc;
  const size_t fl = (size_t)c->fc.fl, stride = (size_t)c->fstride;
  {   // input and output may be the same contiguous frames; any other overlap would be read after it was written
    const char *a0 = (const char *)frames, *a1 = a0 + ((size_t)(B - 1) * stride + fl) * sizeof(float2);
    const char *b0 = (const char *)frames_out, *b1 = b0 + (size_t)B * fl * sizeof(float2);
    if (a0 < b1 && b0 < a1 && !(a0 == b0 && stride == fl))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_subtract_batch: frames_out overlaps frames (in place only with the frame stride 0 or fl, it is %zu)", stride);
  }
  if (const int rc0 = ctx_device_ready(c)) return rc0;
  const float *src = nullptr;
  if ((rc = api_frames_on_device(c, frames, B, where, &src))) return rc;
  float *dst = frames_out;
  if (where == UWSPR_HOST) {
    if (!c->sub) c->sub = new sub_state();
    if ((rc = sub_grow(c, &c->sub->d_out, &c->sub->cap_out, (size_t)B * fl * 2))) return rc;
    dst = c->sub->d_out;
  }
  if ((rc = subtract_run(c, src, stride, B, nullptr, items, nitems, refine, dst))) return rc;
  if (where == UWSPR_HOST)
    CTXCHK(c, hipMemcpyAsync(frames_out, dst, (size_t)B * fl * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  if (res && nitems > 0)
    CTXCHK(c, hipMemcpyAsync(res, c->sub->d_res, (size_t)nitems * sizeof(uwspr_sub_result),
                             where == UWSPR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (where != UWSPR_DEVICE) CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// Measurement hook of tools/subtract_probe.py (not part of the ABI, like uwspr_debug_sched_stamps): enable = 1 / 0 switches
// HIP events around the k8_refine and k8_cancel launches of the calls that follow on / off (< 0: unchanged); with the
// pointers given, waits for the last call and returns its summed kernel times in ms.
extern "C" int uwspr_debug_subtract_times(uwspr_ctx *c, int enable, double *refine_ms, double *cancel_ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->sub) c->sub = new sub_state();
  sub_state *t = c->sub;
  if (enable >= 0) t->timing = enable != 0;
  if (refine_ms || cancel_ms) {
    double a = 0.0, b = 0.0;
    for (size_t k = 0; k + 3 < t->ev_used; k += 4) {
      float ms = 0.0f;
      CTXCHK(c, hipEventSynchronize(t->ev[k + 3]));
      CTXCHK(c, hipEventElapsedTime(&ms, t->ev[k], t->ev[k + 1]));
      a += ms;
      CTXCHK(c, hipEventElapsedTime(&ms, t->ev[k + 2], t->ev[k + 3]));
      b += ms;
    }
    if (refine_ms) *refine_ms = a;
    if (cancel_ms) *cancel_ms = b;
  }
  return UWSPR_OK;
}

// Read-out of tests/test_gpu_subtract_edges.py (not part of the ABI either): the refine surface k8_pick saw for item `item`
// of the last call, M[(q + 4) * 49 + (l + 24)].  Waits for the context's stream, copies the item's nine partial rows out of
// d_part and adds them here in ascending part order in binary32 -- adds only, k8_pick's own operations on the same values,
// so the 441 numbers are bit-equal to the pick's.  UWSPR_ERR_ARG when the last call did not refine or has no such item.
extern "C" int uwspr_debug_subtract_surface(uwspr_ctx *c, int item, float *M) {
  if (!c) return UWSPR_ERR_ARG;
  sub_state *t = c->sub;
  if (!M || !t || !t->last_refine || item < 0 || item >= t->last_items)
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_debug_subtract_surface: item %d, M %p (the last call: %d items, refine %d)", item, (void *)M,
                    t ? t->last_items : 0, t ? (int)t->last_refine : 0);
  if (const int rc0 = ctx_device_ready(c)) return rc0;
  CTXCHK(c, hipStreamSynchronize(c->stream));
  std::vector<float> part((size_t)K8_PARTS * K8_NHYP);
  CTXCHK(c, hipMemcpy(part.data(), t->d_part + (size_t)item * K8_PARTS * K8_NHYP, part.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int h = 0; h < K8_NHYP; h++) {
    float s = 0.0f;
    for (int p = 0; p < K8_PARTS; p++) s += part[(size_t)p * K8_NHYP + h];
    M[h] = s;
  }
  return UWSPR_OK;
}
