// K16 -- blind demodulation along straight-line passes: a record that Fano gave up on is demodulated with K15's per-symbol
// Doppler and delay tables taking the motion out, over a grid of frequency offsets (Q = df / 8) and lags (32 samples), every
// hypothesis scored with the fine search's sync metric, and the soft symbols of the best one handed out (uwspr_follow_set,
// uwspr_follow_batch).  The reference has no counterpart: the definition is this project's, in include/uwspr_hip.h, and
// tests/follow_exact.py restates it in binary64.  Binary32 with fused multiply-adds; every phase and every index in binary64
// or integers.  The tables are designed on the host (uwspr_track_design): no kernel takes a square root of a range.
//
// k16_follow<QF>: a workgroup of ONE wavefront owns an item, a tile of 64 trajectories and ONE lag, and walks the 162 symbols.
// Per symbol it stages the 256 + 2 x 139 samples any delay can reach at that lag (zeros outside [0, fl)) once; lane l owns
// trajectory 64 tile + l and reads the window at its own tau, as K15's lanes do.  The base phasor of sample k = 16 a + b is
// A[a] B[b], both rounded from binary64 (32 sincospi per lane and symbol, kept in LDS at [.][lane]: no bank conflict, no
// register array).  The lane multiplies sample and base phasor once (4 FMAs) and then accumulates ALL 2 QF + 25 grid sums at 4
// FMAs each: Q / 375 = 1 / 2048, so the rotator of grid index g at sample k is W[(g k) & 2047] of one 2048-entry
// root-of-unity table.  Its address is wavefront-uniform, so the table lives in device memory and is read by SCALAR loads
// into SGPRs that the FMAs take as operands: no vector register, no LDS traffic and several loads in flight per wait (the
// same table in LDS cost one exposed LDS round trip per grid sum: profiles/follow.txt).  The 4 nf tone sums of a symbol are 2 QF + 25 grid sums:
// tone t of offset q is grid index q + 8 t - 12.  After a symbol the lane holds its magnitudes and adds them into the
// numerator and the denominator of its 2 QF + 1 offsets, in ascending symbol order: one owner, one order.  QF is the reach
// the kernel is compiled for (4, 8, 16); a set with a smaller qf runs the next larger one and writes its own offsets only --
// a grid sum's bytes do not depend on how many others the lane carries.  The last workgroup of an item computes s_ref -- the
// item's own linear model -- through the same code with the table entries replaced.  Nothing is shared between workgroups,
// so an item's bytes depend on nothing else in the batch.  20.6 KB of LDS per workgroup.
//
// k16_pick: k15_pick on S (K8's rule), and the result record.
// k16_soft: one workgroup of three wavefronts per item, thread i owns symbol i of the picked hypothesis: the same sums for
// the four tones alone, soft[i] = p[pr3 + 2] - p[pr3], then K10's normalisation (binary64 means by one thread, ascending).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K16_NSYM = UWSPR_NSYM, K16_SPB = 256, K16_MID = 81;
constexpr int K16_TMAX = 139;                          // |tau| of any allowed trajectory (K15's bound, checked by track_build)
constexpr int K16_XS = K16_SPB + 2 * K16_TMAX;         // staged samples per symbol
constexpr int K16_TILE = 64, K16_LSTEP = 32, K16_NW = 2048;
constexpr int K16_QFMAX = UWSPR_FOLLOW_QF_MAX, K16_NLMAX = UWSPR_FOLLOW_NL_MAX;
constexpr double K16_FS = 375.0, K16_Q = 375.0 / 2048.0;

// e^{-j 2 pi t}, t in turns
__device__ __forceinline__ float2 k16_phasor(double t) {
  double sn, cs;
  t -= rint(t);
  sincospi(-2.0 * t, &sn, &cs);
  return make_float2((float)cs, (float)sn);
}
__device__ __forceinline__ float2 k16_mul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ void k16_mac(float &re, float &im, float2 y, float2 w) {
  re = fmaf(y.x, w.x, re); re = fmaf(-y.y, w.y, re);
  im = fmaf(y.x, w.y, im); im = fmaf(y.y, w.x, im);
}
// f_i of the item's own linear model
__device__ __forceinline__ double k16_line(double drift, int i) { return 0.5 * drift * ((double)(i - K16_MID) / 81.0); }

// the 2048 roots of unity e^{-j 2 pi m / 2048}, each rounded from binary64: made once per set, on the device, so that
// k16_follow's table in memory and k16_soft's in LDS hold the same bytes
__global__ __launch_bounds__(256) void k16_roots(float2 *__restrict__ W) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < K16_NW) W[m] = k16_phasor((double)m / (double)K16_NW);
}

// workgroup (u, it): u < ntiles * nlg: trajectories 64 (u / nlg) .., lag u % nlg - nl; u = ntiles * nlg: s_ref.
// dfreq, tau: [162][n].  surf [item][n nf nlg], sref [item].
template <int QF>
__global__ __launch_bounds__(K16_TILE) void k16_follow(const float2 *__restrict__ frames, size_t stride, int fl,
                                                       const uwspr_block_item *__restrict__ items, const double *__restrict__ dfreq,
                                                       const int32_t *__restrict__ tau, const float2 *__restrict__ W, int n, int qf,
                                                       int nl, float *__restrict__ surf, float *__restrict__ sref) {
  constexpr int NG = 2 * QF + 25, NQ = 2 * QF + 1;
  __shared__ float2 xs[K16_XS];
  __shared__ float2 At[16][K16_TILE], Bt[16][K16_TILE];
  const int lane = threadIdx.x, it = blockIdx.y, u = blockIdx.x, nf = 2 * qf + 1, nlg = 2 * nl + 1;
  const bool ref = u == (int)gridDim.x - 1;
  const int tile = ref ? 0 : u / nlg, li = ref ? nl : u - tile * nlg;
  const int jl = tile * K16_TILE + lane, j = jl < n ? jl : n - 1;   // (lanes past the set repeat its last trajectory and write nothing)
  const uwspr_block_item I = items[it];
  const float2 *__restrict__ x = frames + (size_t)I.frame * stride;
  const double f = (double)I.f_hz, drift = (double)I.drift_hz;
  float num[NQ], den[NQ];
#pragma unroll
  for (int c = 0; c < NQ; c++) { num[c] = 0.0f; den[c] = 0.0f; }
  for (int i = 0; i < K16_NSYM; i++) {
    const long long base = (long long)I.shift + (long long)K16_LSTEP * (li - nl) + (long long)K16_SPB * i - K16_TMAX;   // |shift| <= 2^20
    __syncthreads();   // the symbol before has been read
    for (int e = lane; e < K16_XS; e += K16_TILE) {
      const long long idx = base + e;
      xs[e] = (idx >= 0 && idx < fl) ? x[idx] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const double dfi = ref ? k16_line(drift, i) : dfreq[(size_t)i * n + j];
    const int ta = ref ? 0 : tau[(size_t)i * n + j];   // |ta| <= K16_TMAX: track_build refuses anything else
    const double w = (f + dfi) / K16_FS;               // turns per sample at g = 0
#pragma unroll 1
    for (int b = 0; b < 16; b++) {
      At[b][lane] = k16_phasor(w * (double)(16 * b));
      Bt[b][lane] = k16_phasor(w * (double)b);
    }
    const float2 *xw = xs + K16_TMAX + ta;
    float re[NG], im[NG];
#pragma unroll
    for (int c = 0; c < NG; c++) { re[c] = 0.0f; im[c] = 0.0f; }
#pragma unroll 1
    for (int a = 0; a < 16; a++) {
      const float2 A = At[a][lane];
#pragma unroll 2
      for (int b = 0; b < 16; b++) {
        const int k = 16 * a + b;
        const float2 y = k16_mul(xw[k], k16_mul(A, Bt[b][lane]));
#pragma unroll
        for (int c = 0; c < NG; c++) k16_mac(re[c], im[c], y, W[((c - (QF + 12)) * k) & (K16_NW - 1)]);
      }
    }
#pragma unroll
    for (int c = 0; c < NG; c++) re[c] = sqrtf(fmaf(re[c], re[c], im[c] * im[c]));
    const float sg = pr3_bit(i) ? 1.0f : -1.0f;
#pragma unroll
    for (int c = 0; c < NQ; c++) {   // offset q = c - QF: tone t at grid index q + 8 t - 12, slot c + 8 t
      const float p0 = re[c], p1 = re[c + 8], p2 = re[c + 16], p3 = re[c + 24];
      num[c] += sg * ((p1 + p3) - (p0 + p2));
      den[c] += ((p0 + p1) + p2) + p3;
    }
  }
  if (ref) {
    if (lane == 0) sref[it] = den[QF] == 0.0f ? 0.0f : num[QF] / den[QF];
  } else if (jl < n) {
#pragma unroll
    for (int c = 0; c < NQ; c++) {
      const int qi = c - QF + qf;
      if (qi >= 0 && qi < nf) surf[(((size_t)it * n + j) * nf + qi) * nlg + li] = den[c] == 0.0f ? 0.0f : num[c] / den[c];
    }
  }
}

// the first maximum of surf[it][0 .. nh) in ascending h (k15_pick's walk: `>` keeps the first of equal values, a NaN loses
// every comparison, a NaN S(0) is never left)
__global__ __launch_bounds__(256) void k16_pick(const uwspr_block_item *__restrict__ items, const float *__restrict__ surf,
                                                const float *__restrict__ sref, int nh, int nf, int nlg, int qf,
                                                uwspr_follow_result *__restrict__ res) {
  __shared__ float bv[256];
  __shared__ int bh[256];
  const int tid = threadIdx.x, it = blockIdx.x;
  const float *__restrict__ S = surf + (size_t)it * nh;
  float m = 0.0f;
  int at = -1;   // no value that is not a NaN yet
  for (int h = tid; h < nh; h += 256) {
    const float v = S[h];
    if (v == v && (at < 0 || v > m)) { m = v; at = h; }
  }
  bv[tid] = m; bh[tid] = at;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const float v = bv[tid + o];
      const int h = bh[tid + o];
      if (h >= 0 && (bh[tid] < 0 || v > bv[tid] || (v == bv[tid] && h < bh[tid]))) { bv[tid] = v; bh[tid] = h; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float s0 = S[0];
    const int best = (s0 != s0 || bh[0] < 0) ? 0 : bh[0];
    uwspr_follow_result r;
    r.best = best;
    r.s_best = S[best];
    r.s_ref = sref[it];
    r.f_hz = (float)((double)items[it].f_hz + K16_Q * (double)((best / nlg) % nf - qf));
    res[it] = r;
  }
}

// the 162 bytes of the picked hypothesis; out [item][162]
__global__ __launch_bounds__(192) void k16_soft(const float2 *__restrict__ frames, size_t stride, int fl,
                                                const uwspr_block_item *__restrict__ items, const double *__restrict__ dfreq,
                                                const int32_t *__restrict__ tau, int n, int qf, int nl,
                                                const uwspr_follow_result *__restrict__ res, uint8_t *__restrict__ out) {
  __shared__ float2 W[K16_NW];
  __shared__ float soft[K16_NSYM];
  __shared__ double fac;
  const int tid = threadIdx.x, it = blockIdx.x, nf = 2 * qf + 1, nlg = 2 * nl + 1;
  const uwspr_block_item I = items[it];
  const float2 *__restrict__ x = frames + (size_t)I.frame * stride;
  int best = res[it].best;
  if (best < 0 || best >= n * nf * nlg) best = 0;   // (k16_pick writes nothing else)
  const int j = best / (nf * nlg), q = (best / nlg) % nf - qf, l = best % nlg - nl;
  for (int m = tid; m < K16_NW; m += 192) W[m] = k16_phasor((double)m / (double)K16_NW);
  __syncthreads();
  if (tid < K16_NSYM) {
    const int i = tid;
    const double w = ((double)I.f_hz + dfreq[(size_t)i * n + j]) / K16_FS;
    const long long base = (long long)I.shift + (long long)K16_LSTEP * l + (long long)K16_SPB * i + tau[(size_t)i * n + j];
    float re[4], im[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { re[t] = 0.0f; im[t] = 0.0f; }
    for (int a = 0; a < 16; a++) {
      const float2 A = k16_phasor(w * (double)(16 * a));
      for (int b = 0; b < 16; b++) {
        const int k = 16 * a + b;
        const long long idx = base + k;
        const float2 s = (idx >= 0 && idx < fl) ? x[idx] : make_float2(0.0f, 0.0f);
        const float2 y = k16_mul(s, k16_mul(A, k16_phasor(w * (double)b)));
#pragma unroll
        for (int t = 0; t < 4; t++) k16_mac(re[t], im[t], y, W[((q + 8 * t - 12) * k) & (K16_NW - 1)]);
      }
    }
    const int p = pr3_bit(i);
    float mag[4];
#pragma unroll
    for (int t = 0; t < 4; t++) mag[t] = sqrtf(fmaf(re[t], re[t], im[t] * im[t]));
    soft[i] = (p ? mag[3] : mag[2]) - (p ? mag[1] : mag[0]);
  }
  __syncthreads();
  if (tid == 0) {
    double fsum = 0.0, f2sum = 0.0;
    for (int i = 0; i < K16_NSYM; i++) {
      const double v = (double)soft[i];
      fsum += v / 162.0;
      f2sum += v * v / 162.0;
    }
    fac = sqrt(f2sum - fsum * fsum);
  }
  __syncthreads();
  if (tid < K16_NSYM) {
    const double fc = fac;
    uint8_t byte = 128;
    if (fc > 0.0 && fc - fc == 0.0) {   // a positive finite number
      double v = 50.0 * (double)soft[tid] / fc;
      v = v > 127.0 ? 127.0 : v;
      v = v < -128.0 ? -128.0 : v;
      byte = (v == v) ? (uint8_t)(int)(v + 128.0) : (uint8_t)128;
    }
    out[(size_t)it * K16_NSYM + tid] = byte;
  }
}


// ---------------------------------------------------------------- host side
struct fol_state {
  fol_set *set = nullptr;   // uwspr_follow_set's
  uwspr_block_item *d_items = nullptr; size_t cap_items = 0;
  // the caller's items go through page-locked memory and the one wait is for the launches of the call before (K10's door)
  uwspr_block_item *h_items = nullptr; size_t cap_h = 0;
  hipEvent_t done = nullptr; bool pending = false;
  float *d_surf = nullptr; size_t cap_surf = 0;
  float *d_sref = nullptr; size_t cap_sref = 0;
  uwspr_follow_result *d_res = nullptr; size_t cap_res = 0;
  uint8_t *d_sym = nullptr; size_t cap_sym = 0;
  launch_timer timer;   // uwspr_debug_follow_time: events around the launches of the last call
};

void follow_free_set(fol_set *s) {
  if (!s) return;
  track_free_set(s->t);
  if (s->d_W) (void)hipFree(s->d_W);
  delete s;
}

void fol_release(uwspr_ctx *c) {
  if (!c || !c->fol) return;
  fol_state *t = c->fol;
  follow_free_set(t->set);
  void *bufs[] = {t->d_items, t->d_surf, t->d_sref, t->d_res, t->d_sym};
  for (void *b : bufs) if (b) (void)hipFree(b);
  if (t->h_items) (void)hipHostFree(t->h_items);
  if (t->done) (void)hipEventDestroy(t->done);
  t->timer.release();
  delete t;
  c->fol = nullptr;
}

// what makes a follow set acceptable: null, or what is wrong (written into msg).  No device is asked.
const char *follow_check(const uwspr_track_traj *traj, int n, int qf, int nl, int model, char *msg, size_t cap) {
  if (nl < 0 || nl > K16_NLMAX) { snprintf(msg, cap, "nl %d (0..%d)", nl, K16_NLMAX); return msg; }
  static_assert(K16_QFMAX == UWSPR_TRACK_QF_MAX, "track_check holds qf to K15's reach");
  return track_check(traj, n, UWSPR_TRACK_MAX, qf, model, msg, cap);
}

fol_set *follow_build(const uwspr_track_traj *traj, int n, int qf, int nl, int model, double cf, int *status, char *msg, size_t cap) {
  trk_set *t = track_build(traj, n, qf, model, cf, status, msg, cap);
  if (!t) return nullptr;
  fol_set *s = new fol_set();
  s->t = t; s->nl = nl;
  hipError_t e = hipMalloc((void **)&s->d_W, K16_NW * sizeof(float2));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k16_roots, dim3(K16_NW / 256), dim3(256), 0, nullptr, s->d_W);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    snprintf(msg, cap, "the table of roots of unity: %s", hipGetErrorString(e));
    *status = UWSPR_ERR_HIP;
    follow_free_set(s);
    return nullptr;
  }
  return s;
}

static size_t follow_hyps(const fol_set *s) { return s ? (size_t)s->t->n * (2 * s->t->qf + 1) * (2 * s->nl + 1) : 0; }

template <int QF>
static void follow_launch(uwspr_ctx *c, const fol_set *set, const float *src, size_t stride, const uwspr_block_item *d_items, int m,
                          float *surf, float *sref) {
  const int ntiles = (set->t->n + K16_TILE - 1) / K16_TILE, nlg = 2 * set->nl + 1;
  hipLaunchKernelGGL(k16_follow<QF>, dim3((unsigned)(ntiles * nlg + 1), (unsigned)m), dim3(K16_TILE), 0, c->stream,
                     reinterpret_cast<const float2 *>(src), stride, c->fc.fl, d_items, set->t->d_dfreq, set->t->d_tau, set->d_W,
                     set->t->n, set->t->qf, set->nl, surf, sref);
}

int follow_run(uwspr_ctx *c, const fol_set *set, const float *src, size_t stride, const uwspr_block_item *items, int nitems,
               uwspr_follow_result *res, uint8_t *symbols, float *surface, uwspr_follow_result **res_out, uint8_t **sym_out) {
  int rc = ctx_device_ready(c);
  if (rc) return rc;
  if (!c->fol) c->fol = new fol_state();
  fol_state *t = c->fol;
  if (!set) set = t->set;
  if (!set) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_follow_batch: no follow set (uwspr_follow_set)");
  const trk_set *ts = set->t;
  const int qf = ts->qf, nf = 2 * qf + 1, nlg = 2 * set->nl + 1;
  const size_t nh = follow_hyps(set);
  if ((rc = ctx_grow(c, &t->d_items, &t->cap_items, (size_t)nitems))) return rc;
  if ((rc = ctx_grow(c, &t->d_sref, &t->cap_sref, (size_t)nitems))) return rc;
  if (!surface) {
    if ((rc = ctx_grow(c, &t->d_surf, &t->cap_surf, (size_t)nitems * nh))) return rc;
    surface = t->d_surf;
  }
  if (!res) {
    if ((rc = ctx_grow(c, &t->d_res, &t->cap_res, (size_t)nitems))) return rc;
    res = t->d_res;
  }
  if (!symbols) {
    if ((rc = ctx_grow(c, &t->d_sym, &t->cap_sym, (size_t)nitems * K16_NSYM))) return rc;
    symbols = t->d_sym;
  }
  if (res_out) *res_out = res;
  if (sym_out) *sym_out = symbols;
  if (!t->done) CTXCHK(c, hipEventCreateWithFlags(&t->done, hipEventDisableTiming));
  if (t->pending) { CTXCHK(c, hipEventSynchronize(t->done)); t->pending = false; }   // the call before has read both item buffers
  if ((size_t)nitems > t->cap_h) {
    if (t->h_items) { CTXCHK(c, hipHostFree(t->h_items)); t->h_items = nullptr; t->cap_h = 0; }
    const size_t m = nitems > 256 ? (size_t)nitems : 256;
    if (hipHostMalloc((void **)&t->h_items, m * sizeof(uwspr_block_item), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      t->h_items = nullptr;
      return ctx_fail(c, UWSPR_ERR_NOMEM, "hipHostMalloc(%zu bytes) for the items", m * sizeof(uwspr_block_item));
    }
    t->cap_h = m;
  }
  memcpy(t->h_items, items, (size_t)nitems * sizeof(uwspr_block_item));
  CTXCHK(c, hipMemcpyAsync(t->d_items, t->h_items, (size_t)nitems * sizeof(uwspr_block_item), hipMemcpyHostToDevice, c->stream));
  if ((rc = t->timer.begin(c))) return rc;
  for (int i0 = 0; i0 < nitems; i0 += 32768) {   // (a grid's y extent)
    const int m = nitems - i0 < 32768 ? nitems - i0 : 32768;
    float *surf = surface + (size_t)i0 * nh;
    if (qf <= 4) follow_launch<4>(c, set, src, stride, t->d_items + i0, m, surf, t->d_sref + i0);
    else if (qf <= 8) follow_launch<8>(c, set, src, stride, t->d_items + i0, m, surf, t->d_sref + i0);
    else follow_launch<16>(c, set, src, stride, t->d_items + i0, m, surf, t->d_sref + i0);
    hipLaunchKernelGGL(k16_pick, dim3((unsigned)m), dim3(256), 0, c->stream, t->d_items + i0, surf, t->d_sref + i0, (int)nh, nf, nlg, qf,
                       res + i0);
    hipLaunchKernelGGL(k16_soft, dim3((unsigned)m), dim3(192), 0, c->stream, reinterpret_cast<const float2 *>(src), stride, c->fc.fl,
                       t->d_items + i0, ts->d_dfreq, ts->d_tau, ts->n, qf, set->nl, res + i0, symbols + (size_t)i0 * K16_NSYM);
  }
  CTXCHK(c, hipGetLastError());
  CTXCHK(c, hipEventRecord(t->done, c->stream));
  t->pending = true;
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_follow_set(uwspr_ctx *c, const uwspr_track_traj *traj, int n, int qf, int nl, int model) {
  if (!c) return UWSPR_ERR_ARG;
  char msg[256];
  if (follow_check(traj, n, qf, nl, model, msg, sizeof(msg))) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_follow_set: %s", msg);
  if (const int rc0 = ctx_device_ready(c)) return rc0;
  int rc = UWSPR_OK;
  fol_set *fresh = follow_build(traj, n, qf, nl, model, (double)c->p.cf, &rc, msg, sizeof(msg));
  if (!fresh) return ctx_fail(c, rc, "uwspr_follow_set: %s", msg);
  if (!c->fol) c->fol = new fol_state();
  fol_state *t = c->fol;
  if (t->pending) {   // the set before may still be read by the call before
    const hipError_t e = hipEventSynchronize(t->done);
    if (e != hipSuccess) { follow_free_set(fresh); return ctx_fail(c, UWSPR_ERR_HIP, "uwspr_follow_set: hipEventSynchronize: %s", hipGetErrorString(e)); }
    t->pending = false;
  }
  follow_free_set(t->set);
  t->set = fresh;
  return UWSPR_OK;
}

extern "C" int uwspr_follow_batch(uwspr_ctx *c, const float *frames, int B, int where, const uwspr_block_item *items, int nitems,
                                  uwspr_follow_result *res, uint8_t *symbols, float *surface) {
  if (!c) return UWSPR_ERR_ARG;
  if (!frames || B <= 0 || (where != UWSPR_HOST && where != UWSPR_DEVICE && where != UWSPR_DEVICE_FRAMES) || (nitems > 0 && (!res || !symbols)))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_follow_batch: frames %p, B %d, where %d, res %p, symbols %p", (const void *)frames, B, where,
                    (void *)res, (void *)symbols);
  int rc = blockdemod_check(c, items, nitems, B);
  if (rc) return rc;
  const fol_set *set = c->fol ? c->fol->set : nullptr;
  if (!set) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_follow_batch: no follow set (uwspr_follow_set)");
  if (nitems == 0) return UWSPR_OK;
  if ((rc = ctx_device_ready(c))) return rc;
  const size_t nh = follow_hyps(set);
  const size_t nres = (size_t)nitems * sizeof(uwspr_follow_result), nsym = (size_t)nitems * K16_NSYM, nsurf = (size_t)nitems * nh * sizeof(float);
  const bool dev_out = where != UWSPR_HOST;
  if (dev_out && (!ctx_device_range(c, res, nres) || !ctx_device_range(c, symbols, nsym) || (surface && !ctx_device_range(c, surface, nsurf))))
    return ctx_fail(c, UWSPR_ERR_ARG,
                    "uwspr_follow_batch: device output needs res (%zu bytes), symbols (%zu bytes) and surface (%zu bytes) inside device allocations of device %d",
                    nres, nsym, nsurf, c->device);
  const float *src = nullptr;
  if ((rc = api_frames_on_device(c, frames, B, where, &src))) return rc;
  fol_state *t = c->fol;
  float *d_surf = dev_out ? surface : nullptr;
  if (!dev_out && surface) {   // (the context's own buffer is then the one follow_run would take: named here to copy it out)
    if ((rc = ctx_grow(c, &t->d_surf, &t->cap_surf, (size_t)nitems * nh))) return rc;
    d_surf = t->d_surf;
  }
  uwspr_follow_result *d_res = nullptr;
  uint8_t *d_sym = nullptr;
  if ((rc = follow_run(c, set, src, (size_t)c->fstride, items, nitems, dev_out ? res : nullptr, dev_out ? symbols : nullptr, d_surf, &d_res, &d_sym)))
    return rc;
  if (!dev_out) {
    CTXCHK(c, hipMemcpyAsync(res, d_res, nres, hipMemcpyDeviceToHost, c->stream));
    CTXCHK(c, hipMemcpyAsync(symbols, d_sym, nsym, hipMemcpyDeviceToHost, c->stream));
    if (surface) CTXCHK(c, hipMemcpyAsync(surface, d_surf, nsurf, hipMemcpyDeviceToHost, c->stream));
  }
  if (where != UWSPR_DEVICE) CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// Measurement hook of tools/follow_probe.py (not part of the ABI, like uwspr_debug_track_time): enable = 1 / 0 switches HIP
// events around the K16 launches of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last timed
// call and returns its time.
extern "C" int uwspr_debug_follow_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->fol) c->fol = new fol_state();   // (no device asked: the hook only keeps the switch)
  return c->fol->timer.read(c, enable, ms);
}
