// K12 -- a noise blanker ahead of the resampler and the front-end: audio at the rate it is pushed at -> the same audio
// with impulses (and G samples either side of them) set to +0 (include/uwspr_hip.h: "Impulsive noise" holds the
// definition; tests/blank_exact.py restates it in numpy).  The reference has no such stage; nothing here is compared
// with it.  K0 reads +-10 Hz: a click that reaches it is smeared over its half-second response and lands in the band
// whole, a click zeroed ahead of it costs its own length of signal.
//
//     u(i)   = bits(x[i]) with the sign cleared                      (unsigned 32-bit)
//     med(b) = the value of rank N/2 - 1 among the u of block b      (N = 4096 samples, a selection: exact)
//     thr(b) = fl32(fl32((float) blank * med(b - 1)) * 0.25f)        (none for b = 0, med = 0, med = inf or NaN)
//     flag(i) <=> u(i) > bits(thr(block(i)))                         y[i] = any flag in [i - G, i + G] ? +0 : x[i]
//
// All integers but the two multiplies of a threshold: no result depends on an order.
//
// k12_level: one 256-thread workgroup per (block, channel), the channels of a block consecutive after xcd_swizzle (they
// read the same lines: one XCD's L2, as K0 and K11 do for interleaved input).  A lane holds 16 patterns in registers;
// the rank is found by radix selection, most significant byte first: four rounds of a 256-bin LDS histogram
// (ds_add_u32 of the patterns that still match the prefix), an inclusive prefix over the bins (one bin per lane:
// shuffles in a wavefront, four wavefront totals through LDS) and the one bin that holds the rank, chosen by the lane
// that owns it and read back by all.  One float stored per workgroup.
// k12_apply: the same grid over the blocks a launch's outputs touch.  A workgroup takes its outputs' span plus G samples
// either side -- at most 4096 + 128 -- a lane 17 of them 256 apart, kept in registers; each is judged by its OWN block's
// threshold (the levels of blocks b - 2, b - 1, b from the level table: the halo on the left belongs to block b - 1, the
// one on the right to b + 1), the flags go to LDS as a bit image (one 64-bit ballot per wavefront and round: no LDS
// atomics), and an output is zero when the window of 2 G + 1 bits around it -- at most three 64-bit words -- holds a
// one.  Outputs by ordinary vector stores, the block's zero count (wavefront sums through LDS) by one store of lane 0.
// Both are memory-bound by arithmetic: 2 or 4 bytes read once per sample and kernel, 4 written by k12_apply; the level
// kernel adds 4 x 16 LDS adds per lane.  No atomics in global memory.
#include <atomic>

#include "uwspr_internal.h"

namespace uwspr {

constexpr int K12_WG = 256;
constexpr int K12_N = UWSPR_BLANK_BLOCK;           // samples per block
constexpr int K12_PER = K12_N / K12_WG;            // patterns per lane (16)
constexpr int K12_GMAX = 64;
constexpr int K12_ROUNDS = (K12_N + 2 * K12_GMAX + K12_WG - 1) / K12_WG;   // staged samples per lane in k12_apply (17)
static_assert(K12_N == 4096 && K12_PER == 16, "k12_level holds 16 patterns per lane");
static_assert(K12_GMAX == stage::BLANK_GMAX, "stream_stage.h sizes the stream's history by the largest guard");

__device__ __forceinline__ float k12_sample(float v) { return v; }
__device__ __forceinline__ float k12_sample(int16_t v) { return (float)v * (1.0f / 32768); }

// audio: [nin][nch] interleaved frames, frame 0 = audio index in0.  lev: [nblk][nch], row 0 = block blk_first.  Samples
// outside [in0, in0 + nin) count as pattern 0 (the callers launch complete blocks only).
template <typename T>
__global__ __launch_bounds__(K12_WG) void k12_level(const T *__restrict__ audio, long long nin, long long in0, int nch,
                                                    float *__restrict__ lev, long long blk_first) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wsum[4];
  __shared__ unsigned pick[2];                       // the chosen bin, the rank inside it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned lb = xcd_swizzle(blockIdx.x, gridDim.x);
  const unsigned blk = lb / (unsigned)nch;
  const int ch = (int)(lb - blk * (unsigned)nch);
  const long long n0 = (blk_first + (long long)blk) * K12_N - in0;   // frame of this buffer the block starts at
  unsigned u[K12_PER];
#pragma unroll
  for (int r = 0; r < K12_PER; r++) {
    const long long n = n0 + r * K12_WG + tid;
    const float v = (n >= 0 && n < nin) ? k12_sample(audio[(size_t)n * nch + ch]) : 0.0f;
    u[r] = __float_as_uint(v) & 0x7fffffffu;
  }
  unsigned prefix = 0, mask = 0, k = K12_N / 2 - 1;  // the rank wanted among the patterns that match prefix under mask
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K12_PER; r++)
      if ((u[r] & mask) == prefix) atomicAdd(&hist[(u[r] >> shift) & 255u], 1u);
    __syncthreads();
    const unsigned own = hist[tid];
    unsigned inc = own;                              // inclusive prefix over the bins: lane t ends with sum hist[0..t]
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; w++) inc += wsum[w];
    const unsigned exc = inc - own;
    if (exc <= k && k < inc) { pick[0] = (unsigned)tid; pick[1] = k - exc; }   // (exactly one bin: the counts sum to > k)
    __syncthreads();
    prefix |= pick[0] << shift;
    mask |= 255u << shift;
    k = pick[1];
  }
  if (tid == 0) lev[(size_t)blk * nch + ch] = __uint_as_float(prefix);
}

// bits(thr) of the samples of block b, from the level of block b - 1; 0xffffffff: the block has no threshold
__device__ __forceinline__ unsigned k12_threshold(const float *__restrict__ lev, long long nlev, long long blk0, int nch, int ch,
                                                  long long b, float fblank) {
  const long long row = b - 1 - blk0;
  if (b < 1 || row < 0 || row >= nlev) return 0xffffffffu;
  const float med = lev[(size_t)row * nch + ch];
  const unsigned mb = __float_as_uint(med);
  if (mb == 0 || mb >= 0x7f800000u) return 0xffffffffu;
  float t = fblank * med;                            // two roundings (the build has -ffp-contract=off; subnormals kept)
  t = t * 0.25f;
  return __float_as_uint(t);
}

// Outputs [y_first, y_first + nout) of every channel -> out [nout][nch] (row 0 = y_first); nz: [blocks the outputs
// touch][nch] int32, row 0 = block y_first div N, the outputs of THIS launch set to zero.  audio as in k12_level; a
// sample outside the buffer, or before audio index 0, does not exist (it is never flagged).  lev: [nlev][nch], row 0 =
// block blk0; a block outside the table has level 0 (no threshold for the block behind it).
template <typename T>
__global__ __launch_bounds__(K12_WG) void k12_apply(const T *__restrict__ audio, long long nin, long long in0, int nch,
                                                    const float *__restrict__ lev, long long nlev, long long blk0, int blank, int G,
                                                    float *__restrict__ out, long long nout, long long y_first, int *__restrict__ nz) {
  __shared__ unsigned long long bits[K12_ROUNDS * K12_WG / 64];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned lb = xcd_swizzle(blockIdx.x, gridDim.x);
  const unsigned blk = lb / (unsigned)nch;
  const int ch = (int)(lb - blk * (unsigned)nch);
  const long long b = y_first / K12_N + (long long)blk;
  long long lo = b * K12_N, hi = lo + K12_N;         // this workgroup's outputs: [lo, hi)
  if (lo < y_first) lo = y_first;
  if (hi > y_first + nout) hi = y_first + nout;
  const int cnt = (int)(hi - lo);                    // 1 .. N
  const int S = cnt + 2 * G;                         // staged samples: audio [lo - G, hi + G)
  const float fblank = (float)blank;
  unsigned thr[3];                                   // of blocks b - 1, b, b + 1
#pragma unroll
  for (int q = 0; q < 3; q++) thr[q] = k12_threshold(lev, nlev, blk0, nch, ch, b - 1 + q, fblank);
  const long long bn = b * K12_N;

  float x[K12_ROUNDS];
#pragma unroll
  for (int r = 0; r < K12_ROUNDS; r++) {
    const int e = r * K12_WG + tid;
    const long long j = lo - G + e;                  // audio index
    const long long n = j - in0;
    bool flag = false;
    x[r] = 0.0f;
    if (e < S && j >= 0 && n >= 0 && n < nin) {
      x[r] = k12_sample(audio[(size_t)n * nch + ch]);
      const unsigned t = j < bn ? thr[0] : (j < bn + K12_N ? thr[1] : thr[2]);
      flag = t != 0xffffffffu && (__float_as_uint(x[r]) & 0x7fffffffu) > t;
    }
    const unsigned long long m = __ballot(flag);
    if (lane == 0) bits[r * (K12_WG / 64) + wave] = m;
  }
  __syncthreads();

  int zeros = 0;
#pragma unroll
  for (int r = 0; r < K12_ROUNDS; r++) {
    const int e = r * K12_WG + tid;                  // output lo + e - G: its window is staged [e - G, e + G]
    if (e >= G && e < G + cnt) {
      const int a = e - G, z = e + G;
      unsigned long long any = 0;
      for (int w = a >> 6; w <= (z >> 6); w++) {     // at most three words
        const int l = a > w * 64 ? a - w * 64 : 0, h = z < w * 64 + 63 ? z - w * 64 : 63;
        any |= bits[w] & ((~0ull >> (63 - h)) & (~0ull << l));
      }
      out[(size_t)(lo + (e - G) - y_first) * nch + ch] = any ? 0.0f : x[r];
      zeros += any ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) zeros += __shfl_xor(zeros, d, 64);
  if (lane == 0) wcnt[wave] = zeros;
  __syncthreads();
  if (tid == 0) nz[(size_t)blk * nch + ch] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

static std::atomic<long long> k12_launches[4];   // level float, level int16, apply float, apply int16: the whole process
long long blank_launch_count(int which) { return k12_launches[which & 3].load(); }

// levels of blocks [blk_first, blk_first + nblk) of every channel -> lev[nblk][nch], from the buffer that holds frames
// [in0, in0 + nin)
hipError_t launch_blank_level(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, float *lev,
                              long long nblk, long long blk_first) {
  if (nblk <= 0) return hipSuccess;
  if (nblk * nch > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(nblk * nch));
  k12_launches[s16 ? 1 : 0]++;
  if (s16)
    hipLaunchKernelGGL(k12_level<int16_t>, grid, dim3(K12_WG), 0, s, (const int16_t *)audio, nin, in0, nch, lev, blk_first);
  else
    hipLaunchKernelGGL(k12_level<float>, grid, dim3(K12_WG), 0, s, (const float *)audio, nin, in0, nch, lev, blk_first);
  return hipGetLastError();
}

// outputs [y_first, y_first + nout) of every channel -> out[nout][nch], their zero counts -> nz[stage::blank_blocks_of()][nch]
hipError_t launch_blank_apply(hipStream_t s, const void *audio, bool s16, long long nin, long long in0, int nch, const float *lev,
                              long long nlev, long long blk0, int blank, int guard, float *out, long long nout, long long y_first,
                              int *nz) {
  if (nout <= 0) return hipSuccess;
  const long long nblk = stage::blank_blocks_of(y_first, nout);
  if (nblk * nch > 0x7fffffffLL || guard < 0 || guard > K12_GMAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(nblk * nch));
  k12_launches[s16 ? 3 : 2]++;
  if (s16)
    hipLaunchKernelGGL(k12_apply<int16_t>, grid, dim3(K12_WG), 0, s, (const int16_t *)audio, nin, in0, nch, lev, nlev, blk0, blank,
                       guard, out, nout, y_first, nz);
  else
    hipLaunchKernelGGL(k12_apply<float>, grid, dim3(K12_WG), 0, s, (const float *)audio, nin, in0, nch, lev, nlev, blk0, blank,
                       guard, out, nout, y_first, nz);
  return hipGetLastError();
}

// ---------------------------------------------------------------- the batch call
struct bk_state {
  char *d_in = nullptr; size_t cap_in = 0;
  float *d_out = nullptr; size_t cap_out = 0;
  char *d_tab = nullptr; size_t cap_tab = 0;         // levels [nblocks][C] float, then zero counts [nblocks][C] int32
};

void bk_release(uwspr_ctx *c) {
  if (!c->bk) return;
  if (c->bk->d_in) (void)hipFree(c->bk->d_in);
  if (c->bk->d_out) (void)hipFree(c->bk->d_out);
  if (c->bk->d_tab) (void)hipFree(c->bk->d_tab);
  delete c->bk;
  c->bk = nullptr;
}

static int bk_fail(uwspr_ctx *c, int status, const char *what, hipError_t e) {
  snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
  return status;
}

static int bk_grow(uwspr_ctx *c, char **p, size_t *cap, size_t bytes) {
  if (*cap >= bytes) return UWSPR_OK;
  hipError_t e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
  if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
  if ((e = hipMalloc((void **)p, bytes)) != hipSuccess) { *p = nullptr; return bk_fail(c, UWSPR_ERR_NOMEM, "uwspr_blank_batch buffers", e); }
  *cap = bytes;
  return UWSPR_OK;
}

int bk_batch(uwspr_ctx *c, const void *audio, long long nin, int nch, int s16, int where, int blank, int guard, float *out,
             float *med, int *nzero) {
  if (!c->bk) c->bk = new bk_state();
  bk_state &S = *c->bk;
  hipError_t e;
  int rc;
  const long long nblk = (nin + K12_N - 1) / K12_N, nfull = nin / K12_N;
  if (nblk * nch > 0x7fffffffLL) {
    snprintf(c->err, sizeof(c->err), "uwspr_blank_batch: %lld blocks of %d channels in one call", nblk, nch);
    return UWSPR_ERR_ARG;
  }
  const size_t in_bytes = (size_t)nin * nch * (s16 ? 2 : 4), out_floats = (size_t)nin * nch, tab = (size_t)nblk * nch;
  // the level table and the counts are the call's own on the device unless the caller's device arrays take them
  const bool own_tab = where == UWSPR_HOST || !med || !nzero;
  if (own_tab && (rc = bk_grow(c, &S.d_tab, &S.cap_tab, tab * 8))) return rc;
  float *dlev = where == UWSPR_DEVICE && med ? med : (float *)S.d_tab;
  int *dnz = where == UWSPR_DEVICE && nzero ? nzero : (int *)(S.d_tab + tab * 4);
  const void *din = audio;
  float *dout = out;
  if (where == UWSPR_HOST) {
    if ((rc = bk_grow(c, &S.d_in, &S.cap_in, in_bytes))) return rc;
    if ((rc = bk_grow(c, (char **)&S.d_out, &S.cap_out, out_floats * sizeof(float)))) return rc;
    if ((e = hipMemcpyAsync(S.d_in, audio, in_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
    din = S.d_in; dout = S.d_out;
  }
  if (nblk > nfull && (e = hipMemsetAsync(dlev + (size_t)nfull * nch, 0, (size_t)nch * sizeof(float), c->stream)) != hipSuccess)
    return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
  if ((e = launch_blank_level(c->stream, din, s16 != 0, nin, 0, nch, dlev, nfull, 0)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
  if ((e = launch_blank_apply(c->stream, din, s16 != 0, nin, 0, nch, dlev, nfull, 0, blank, guard, dout, nin, 0, dnz)) != hipSuccess)
    return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
  if (where == UWSPR_HOST) {
    if ((e = hipMemcpyAsync(out, S.d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
    if (med && (e = hipMemcpyAsync(med, dlev, tab * sizeof(float), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
    if (nzero && (e = hipMemcpyAsync(nzero, dnz, tab * sizeof(int), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_blank_batch", e);
  }
  return UWSPR_OK;
}

// one launch of each kernel on device memory (the level kernel when nblk > 0, the apply kernel when nout > 0), waited for
int bk_debug_launch(uwspr_ctx *c, const void *audio_dev, int s16, long long nin, long long in0, int nch, float *lev_dev,
                    long long nlev, long long blk0, long long level_first, long long level_n, int blank, int guard, float *out_dev,
                    long long nout, long long y_first, int *nz_dev) {
  hipError_t e = launch_blank_level(c->stream, audio_dev, s16 != 0, nin, in0, nch, lev_dev + (size_t)(level_first - blk0) * nch,
                                    level_n, level_first);
  if (e == hipSuccess)
    e = launch_blank_apply(c->stream, audio_dev, s16 != 0, nin, in0, nch, lev_dev, nlev, blk0, blank, guard, out_dev, nout, y_first, nz_dev);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return bk_fail(c, UWSPR_ERR_HIP, "uwspr_debug_blank_launch", e);
  return UWSPR_OK;
}

}  // namespace uwspr
