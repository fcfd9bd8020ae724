// K11 -- audio at a sound card's rate R -> the 12 kS/s real audio K0 takes: a polyphase rational resampler
// (include/uwspr_hip.h: "Audio at other rates" holds the definition; tests/resample_exact.py restates it in numpy).
//
//     y[j] = sum_{t = T-1 .. 0} hp[p][t] x[i0 - t],    q = j M + D,  i0 = q div L,  p = q mod L,   L / M = 12000 / R
//
// one chain of binary32 fused multiply-adds per output, t descending, from +0: an output's bytes are the same wherever
// it falls in a workgroup, a launch or a stream (one owner, one order).  The reference has no such stage (its flowgraph
// reads 12 kS/s files); nothing here is compared with it.
//
// Mapping.  A 256-thread workgroup makes 256 consecutive outputs of ONE channel, a lane one output.  The input span of
// the block -- ceil(255 M / L) + T samples, at most 4269 -- is staged in LDS as binary32 (int16 widened on the way in:
// s / 32768, exact), the [L][T] tap image beside it at an odd pitch.  ds_read_b32 banks are (a / 4) mod 32 per 32-lane
// half: neighbouring lanes read the span M / L samples apart (4, 8, 16 at 48, 96, 192 kS/s: 4-, 8-, 16-way conflicts on
// a linear span), so sample i is stored at i + (i >> 5), which makes every stride that is a power of two up to 32
// conflict-free; the taps' rows are p T' apart with T' odd, and for L = 1 every lane reads the same tap (a broadcast).
// Channels: the frames are interleaved [n][C]; the workgroups of one output block (one per channel) read the same
// lines, so they are consecutive after xcd_swizzle and share an XCD's L2, as K0's multichannel form does.
// 2 T flop per output against M / L (2 or 4) + 4 bytes: small by arithmetic, LDS-read bound (2 reads per FMA).
#include <math.h>

#include <atomic>
#include <numeric>
#include <vector>

#include "uwspr_internal.h"

namespace uwspr {

constexpr int K11_WG = 256;             // threads = outputs per workgroup
constexpr int K11_SPAN_MAX = 4269;      // ceil(255 * 16) + 173 at 192 kS/s is 4253; the bound of every supported rate
__host__ __device__ constexpr int k11_sw(int i) { return i + (i >> 5); }

__device__ __forceinline__ float k11_sample(float v) { return v; }
__device__ __forceinline__ float k11_sample(int16_t v) { return (float)v * (1.0f / 32768); }

__host__ __device__ inline long long k11_floordiv(long long a, long long b) {   // b > 0
  const long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// audio: [nin][nch] interleaved frames, frame 0 = input index in0; out: [nout][nch], row 0 = output j_first.  Samples
// outside [in0, in0 + nin) count as zero.  taps: [L][TP] floats, taps[p][t] = (float) h[p + t L].
template <typename T>
__global__ __launch_bounds__(K11_WG) void k11_resample(const T *__restrict__ audio, long long nin, long long in0, int nch,
                                                       const float *__restrict__ taps, int L, int M, int NT, int TP, int D,
                                                       float *__restrict__ out, long long nout, long long j_first) {
  extern __shared__ __align__(16) float k11_lds[];
  float *xs = k11_lds;                               // k11_sw(span) floats
  float *tp = k11_lds + k11_sw(K11_SPAN_MAX) + 1;    // [L][TP]
  const int tid = threadIdx.x;
  const unsigned lb = xcd_swizzle(blockIdx.x, gridDim.x);
  const unsigned blk = lb / (unsigned)nch;
  const int ch = (int)(lb - blk * (unsigned)nch);
  const long long jrel0 = (long long)blk * K11_WG;
  const long long j0 = j_first + jrel0;
  // the block's span: from the oldest sample of its first output to the newest of its last
  const long long ibase = k11_floordiv(j0 * M + D, L) - (NT - 1);
  const long long ilast = k11_floordiv((j0 + K11_WG - 1) * M + D, L);
  int span = (int)(ilast - ibase + 1);
  if (span > K11_SPAN_MAX) span = K11_SPAN_MAX;      // (never for a supported rate: the LDS bound, not arithmetic)
  for (int e = tid; e < span; e += K11_WG) {
    const long long n = ibase + e - in0;             // frame of this buffer
    xs[k11_sw(e)] = (n >= 0 && n < nin) ? k11_sample(audio[(size_t)n * nch + ch]) : 0.0f;
  }
  for (int e = tid; e < L * TP; e += K11_WG) tp[e] = taps[e];
  __syncthreads();

  const long long jrel = jrel0 + tid;
  if (jrel >= nout) return;
  const long long q = (j0 + tid) * M + D;
  const long long i0 = k11_floordiv(q, L);
  const int p = (int)(q - i0 * L);
  const int r = (int)(i0 - ibase);                   // T - 1 <= r < span
  const float *g = tp + p * TP;
  float acc = 0.0f;
  if (r < span) {
    for (int t = NT - 1; t >= 0; t--) acc = fmaf(g[t], xs[k11_sw(r - t)], acc);
  }
  out[(size_t)jrel * nch + ch] = acc;
}

static size_t k11_lds_bytes(int L, int TP) { return ((size_t)k11_sw(K11_SPAN_MAX) + 1 + (size_t)L * TP) * sizeof(float); }

// ---------------------------------------------------------------- the design (host, binary64)
// include/uwspr_hip.h states it; K0's design code supplies I0 (gr_izero: the power series, terms down to 1e-21)
int resample_design(int rate, resample_plan &o) {
  o = resample_plan();
  if (rate < 8000 || rate > 192000) return UWSPR_ERR_ARG;
  const int g = std::gcd(rate, 12000);
  o.rate = rate; o.L = 12000 / g; o.M = rate / g;
  if (o.L > 160) return UWSPR_ERR_ARG;
  if (rate == 12000) {   // no resampler: the identity
    o.T = 1; o.N = 1; o.D = 0; o.h.assign(1, 1.0);
    return UWSPR_OK;
  }
  const double A = 100.0, beta = 0.1102 * (A - 8.7);
  const double F = (double)o.L * (double)rate;
  const double fp = 2400.0, fs = (double)(rate < 12000 ? rate : 12000) - 2400.0, fc = (fp + fs) / 2.0;
  const double dw = 2.0 * M_PI * (fs - fp) / F;
  int N = (int)ceil((A - 8.0) / (2.285 * dw)) + 1;
  if ((N & 1) == 0) N++;
  o.N = N; o.D = (N - 1) / 2; o.T = (N + o.L - 1) / o.L;
  o.h.assign((size_t)o.T * o.L, 0.0);
  const double ibeta = 1.0 / gr_izero(beta), c = 2.0 * fc / F;
  double sum = 0.0;
  for (int k = 0; k < N; k++) {
    const double u = 2.0 * (double)k / (double)(N - 1) - 1.0;
    const double w = gr_izero(beta * sqrt(1.0 - u * u > 0.0 ? 1.0 - u * u : 0.0)) * ibeta;
    const double a = M_PI * c * (double)(k - o.D);
    o.h[k] = c * (k == o.D ? 1.0 : sin(a) / a) * w;
    sum += o.h[k];
  }
  for (int k = 0; k < N; k++) o.h[k] *= (double)o.L / sum;
  return UWSPR_OK;
}

// the kernel's tap image: [L][TP] floats with TP = T | 1, img[p][t] = (float) h[p + t L]
void resample_tap_image(const resample_plan &pl, std::vector<float> &img, int *TP) {
  const int tp = pl.T | 1;
  img.assign((size_t)pl.L * tp, 0.0f);
  for (int p = 0; p < pl.L; p++)
    for (int t = 0; t < pl.T; t++) img[(size_t)p * tp + t] = (float)pl.h[(size_t)p + (size_t)t * pl.L];
  *TP = tp;
}

static std::atomic<long long> k11_launches[2];   // per instantiation (float, int16), the whole process
long long resample_launch_count(int s16) { return k11_launches[s16 ? 1 : 0].load(); }

// one launch on stream s: outputs [j_first, j_first + nout) of every channel from the buffer that holds frames
// [in0, in0 + nin)
hipError_t launch_resample(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, const float *taps,
                           const resample_plan &pl, int TP, float *out, long long nout, long long j_first) {
  if (nout <= 0) return hipSuccess;
  const long long nblk = (nout + K11_WG - 1) / K11_WG;
  if (nblk * nch > 0x7fffffffLL || (long long)ceil(255.0 * pl.M / pl.L) + pl.T > K11_SPAN_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(nblk * nch));
  const size_t lds = k11_lds_bytes(pl.L, TP);
  k11_launches[s16 ? 1 : 0]++;
  if (s16)
    hipLaunchKernelGGL(k11_resample<int16_t>, grid, dim3(K11_WG), lds, s, (const int16_t *)audio, nin, in0, nch, taps, pl.L, pl.M,
                       pl.T, TP, pl.D, out, nout, j_first);
  else
    hipLaunchKernelGGL(k11_resample<float>, grid, dim3(K11_WG), lds, s, (const float *)audio, nin, in0, nch, taps, pl.L, pl.M,
                       pl.T, TP, pl.D, out, nout, j_first);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the batch call
struct rs_state {
  int rate = 0, TP = 0;
  resample_plan pl;
  float *d_taps = nullptr;
  char *d_in = nullptr; size_t cap_in = 0;
  float *d_out = nullptr; size_t cap_out = 0;
};

void rs_release(uwspr_ctx *c) {
  if (!c->rs) return;
  if (c->rs->d_taps) (void)hipFree(c->rs->d_taps);
  if (c->rs->d_in) (void)hipFree(c->rs->d_in);
  if (c->rs->d_out) (void)hipFree(c->rs->d_out);
  delete c->rs;
  c->rs = nullptr;
}

static int rs_fail(uwspr_ctx *c, int status, const char *what, hipError_t e) {
  snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
  return status;
}

// the taps of `rate` on the device, for the context's batch call and the debug door
int rs_taps(uwspr_ctx *c, int rate) {
  if (!c->rs) c->rs = new rs_state();
  rs_state &S = *c->rs;
  if (S.d_taps && S.rate == rate) return UWSPR_OK;
  resample_plan pl;
  if (resample_design(rate, pl)) {
    snprintf(c->err, sizeof(c->err), "audio rate %d S/s is not supported (8000 .. 192000 with 12000 / gcd(rate, 12000) <= 160)", rate);
    return UWSPR_ERR_ARG;
  }
  std::vector<float> img;
  int TP = 0;
  resample_tap_image(pl, img, &TP);
  hipError_t e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "resampler taps", e);
  if (S.d_taps) { (void)hipFree(S.d_taps); S.d_taps = nullptr; }
  if ((e = hipMalloc((void **)&S.d_taps, img.size() * sizeof(float))) != hipSuccess) { S.d_taps = nullptr; return rs_fail(c, UWSPR_ERR_NOMEM, "resampler taps", e); }
  if ((e = hipMemcpy(S.d_taps, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "resampler taps", e);
  S.rate = rate; S.pl = pl; S.TP = TP;
  return UWSPR_OK;
}

int rs_batch(uwspr_ctx *c, const void *audio, long long nin, int nch, int s16, int rate, int where, float *out, long long nout) {
  int rc = rs_taps(c, rate);
  if (rc) return rc;
  rs_state &S = *c->rs;
  hipError_t e;
  const void *din = audio;
  float *dout = out;
  const size_t in_bytes = (size_t)nin * nch * (s16 ? 2 : 4), out_floats = (size_t)nout * nch;
  if (where == UWSPR_HOST) {
    if (S.cap_in < in_bytes) {
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
      if (S.d_in) { (void)hipFree(S.d_in); S.d_in = nullptr; S.cap_in = 0; }
      if ((e = hipMalloc((void **)&S.d_in, in_bytes)) != hipSuccess) { S.d_in = nullptr; return rs_fail(c, UWSPR_ERR_NOMEM, "uwspr_resample_batch input", e); }
      S.cap_in = in_bytes;
    }
    if (S.cap_out < out_floats) {
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
      if (S.d_out) { (void)hipFree(S.d_out); S.d_out = nullptr; S.cap_out = 0; }
      if ((e = hipMalloc((void **)&S.d_out, out_floats * sizeof(float))) != hipSuccess) { S.d_out = nullptr; return rs_fail(c, UWSPR_ERR_NOMEM, "uwspr_resample_batch output", e); }
      S.cap_out = out_floats;
    }
    if ((e = hipMemcpyAsync(S.d_in, audio, in_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
    din = S.d_in; dout = S.d_out;
  }
  // launches of at most 2^22 output frames (a grid below 2^31 workgroups whatever nch is)
  const long long piece = 1LL << 22;
  for (long long j = 0; j < nout; j += piece) {
    const long long k = nout - j < piece ? nout - j : piece;
    if ((e = launch_resample(c->stream, din, s16 != 0, nin, 0, nch, S.d_taps, S.pl, S.TP, dout + (size_t)j * nch, k, j)) != hipSuccess)
      return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
  }
  if (where == UWSPR_HOST) {
    if ((e = hipMemcpyAsync(out, S.d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_resample_batch", e);
  }
  return UWSPR_OK;
}

int rs_debug_launch(uwspr_ctx *c, const void *audio_dev, int s16, long long nin, long long in0, int nch, int rate, float *out_dev,
                    long long nout, long long j_first) {
  int rc = rs_taps(c, rate);
  if (rc) return rc;
  rs_state &S = *c->rs;
  hipError_t e = launch_resample(c->stream, audio_dev, s16 != 0, nin, in0, nch, S.d_taps, S.pl, S.TP, out_dev, nout, j_first);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return rs_fail(c, UWSPR_ERR_HIP, "uwspr_debug_resample_launch", e);
  return UWSPR_OK;
}

}  // namespace uwspr
