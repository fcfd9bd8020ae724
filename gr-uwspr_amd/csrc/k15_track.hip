// K15 -- known-symbol trajectory fit: a decoded transmission's 162 known symbols are correlated over straight-line passes
// (v, d, tc) and frequency offsets, so that a decoded beacon also gives speed, CPA range and CPA time (uwspr_track_set,
// uwspr_track_batch).  The reference has no counterpart: the definition is this project's, in include/uwspr_hip.h, and
// tests/track_exact.py restates it in binary64.  Binary32 with fused multiply-adds; every phase and every index in binary64
// or integers.  The per-symbol Doppler and delay tables are designed on the host (uwspr_track_design): no kernel takes a
// square root of a range.
//
// k15_track: a workgroup of ONE wavefront owns an item, a tile of 64 trajectories and a chunk of 3 frequency offsets, and
// walks the 162 symbols.  Per symbol it stages the 256 + 2 x 139 samples any delay can reach (samples outside [0, fl) are
// zeros) once; lane l owns trajectory 64 tile + l and reads the window at its own tau -- neighbouring trajectories of a grid
// have neighbouring delays, equal addresses broadcast and 32 distinct consecutive pairs fall in 32 different bank pairs.
// The phasor of sample k = 16 a + b is A[a] B[b], both rounded from binary64 (32 sincospi per lane and symbol: no
// recurrence, so no growth of the error along the symbol); the chunk's offsets differ by the per-k rotator table
// e^{-j 2 pi 0.0125 q k / 375} of the workgroup, as K8's q-lanes do.  Per sample and offset 4 + 8 FMAs, per sample 4 more.
// A lane owns T of its (trajectory, offset) over all 162 symbols, in ascending symbol order: one owner, one order.  The last
// workgroup of an item computes T_ref -- the item's own linear model -- through the same code with the table entries
// replaced: (v = 0, q = 0, drift = 0) gives T_ref's bytes.  The window is re-staged per workgroup (4 KB per symbol from L2
// against 64 x 256 x 40 FMAs): nothing is shared between workgroups, so an item's bytes depend on nothing else in the batch.
// 10.4 KB of LDS per workgroup.
//
// k15_pick: one workgroup per item takes the first maximum of the item's n nf values (K8's rule: it moves on `>` alone, a
// NaN is never moved to and a NaN T(0) is never left) and writes the result record.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K15_NSYM = UWSPR_NSYM, K15_SPB = 256, K15_MID = 81;
constexpr int K15_TMAX = 139;                          // |tau| of any allowed trajectory (v <= 10 m/s over 55.3 s, c = 1500 m/s)
constexpr int K15_XS = K15_SPB + 2 * K15_TMAX;         // staged samples per symbol
constexpr int K15_QC = 3, K15_TILE = 64;               // offsets per workgroup, trajectories per workgroup
constexpr int K15_QFMAX = UWSPR_TRACK_QF_MAX;
constexpr double K15_FS = 375.0, K15_DF = 375.0 / 256.0, K15_DFQ = 0.0125, K15_C = 1500.0;

// e^{-j 2 pi t}, t in turns
__device__ __forceinline__ float2 k15_phasor(double t) {
  double sn, cs;
  t -= rint(t);
  sincospi(-2.0 * t, &sn, &cs);
  return make_float2((float)cs, (float)sn);
}
__device__ __forceinline__ float2 k15_mul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// workgroup (u, it): u < ntiles * nchunks: trajectories 64 (u / nchunks) .., offsets 3 (u % nchunks) ..; u = ntiles * nchunks:
// T_ref.  dfreq, tau: [162][n] (the design transposed: a wavefront reads consecutive words).  surf [item][n nf], tref [item].
__global__ __launch_bounds__(K15_TILE) void k15_track(const float2 *__restrict__ frames, size_t stride, int fl,
                                                      const uwspr_sub_item *__restrict__ items, const double *__restrict__ dfreq,
                                                      const int32_t *__restrict__ tau, int n, int qf, int nchunks,
                                                      float *__restrict__ surf, float *__restrict__ tref) {
  __shared__ float2 xs[K15_XS];
  __shared__ float2 dq[K15_QC][K15_SPB];
  const int lane = threadIdx.x, it = blockIdx.y, u = blockIdx.x, nf = 2 * qf + 1;
  const bool ref = u == (int)gridDim.x - 1;
  const int tile = ref ? 0 : u / nchunks, q0 = ref ? qf : K15_QC * (u - tile * nchunks);
  const int jl = tile * K15_TILE + lane, j = jl < n ? jl : n - 1;   // (lanes past the set repeat its last trajectory and write nothing)
  const uwspr_sub_item &I = items[it];
  const float2 *__restrict__ x = frames + (size_t)I.frame * stride;
  const double f = (double)I.f_hz, drift = (double)I.drift_hz;
  const int shift = I.shift;
  for (int e = lane; e < K15_QC * K15_SPB; e += K15_TILE) {
    const int c = e >> 8, k = e & 255, qi = q0 + c < nf ? q0 + c : nf - 1;
    dq[c][k] = k15_phasor((K15_DFQ * (double)(qi - qf) / K15_FS) * (double)k);
  }
  float T[K15_QC];
#pragma unroll
  for (int c = 0; c < K15_QC; c++) T[c] = 0.0f;
  for (int i = 0; i < K15_NSYM; i++) {
    const long long base = (long long)shift + (long long)K15_SPB * i - K15_TMAX;   // |shift| <= 2^20
    __syncthreads();   // the symbol before has been read (and dq written)
    for (int e = lane; e < K15_XS; e += K15_TILE) {
      const long long idx = base + e;
      xs[e] = (idx >= 0 && idx < fl) ? x[idx] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const double dfi = ref ? 0.5 * drift * ((double)(i - K15_MID) / 81.0) : dfreq[(size_t)i * n + j];
    const int ta = ref ? 0 : tau[(size_t)i * n + j];   // |ta| <= K15_TMAX: track_build refuses anything else
    const double w = ((f + dfi) + ((double)I.symbols[i] - 1.5) * K15_DF) / K15_FS;   // turns per sample
    float2 Bt[16];
#pragma unroll
    for (int b = 0; b < 16; b++) Bt[b] = k15_phasor(w * (double)b);
    const float2 *xw = xs + K15_TMAX + ta;
    float re[K15_QC], im[K15_QC];
#pragma unroll
    for (int c = 0; c < K15_QC; c++) { re[c] = 0.0f; im[c] = 0.0f; }
    for (int a = 0; a < 16; a++) {
      const float2 A = k15_phasor(w * (double)(16 * a));
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int k = 16 * a + b;
        const float2 p = k15_mul(A, Bt[b]), s = xw[k];
#pragma unroll
        for (int c = 0; c < K15_QC; c++) {
          const float2 r = k15_mul(p, dq[c][k]);
          re[c] = fmaf(s.x, r.x, re[c]); re[c] = fmaf(-s.y, r.y, re[c]);
          im[c] = fmaf(s.x, r.y, im[c]); im[c] = fmaf(s.y, r.x, im[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < K15_QC; c++) T[c] += sqrtf(fmaf(re[c], re[c], im[c] * im[c]));
  }
  if (ref) {
    if (lane == 0) tref[it] = T[0];
  } else if (jl < n) {
#pragma unroll
    for (int c = 0; c < K15_QC; c++)
      if (q0 + c < nf) surf[((size_t)it * n + j) * nf + q0 + c] = T[c];
  }
}

// the first maximum of surf[it][0 .. nh) in ascending h: per thread over h = tid, tid + 256, .. (`>` keeps the first of equal
// values, a NaN loses every comparison), then over the threads by (value, smaller h); a NaN T(0) is never left
__global__ __launch_bounds__(256) void k15_pick(const uwspr_sub_item *__restrict__ items, const float *__restrict__ surf,
                                                const float *__restrict__ tref, int nh, int nf, int qf, uwspr_track_result *__restrict__ res) {
  __shared__ float bv[256];
  __shared__ int bh[256];
  const int tid = threadIdx.x, it = blockIdx.x;
  const float *__restrict__ T = surf + (size_t)it * nh;
  float m = 0.0f;
  int at = -1;   // no value that is not a NaN yet
  for (int h = tid; h < nh; h += 256) {
    const float v = T[h];
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
    const float t0 = T[0];
    const int best = (t0 != t0 || bh[0] < 0) ? 0 : bh[0];
    uwspr_track_result r;
    r.best = best;
    r.t_best = T[best];
    r.t_ref = tref[it];
    r.f_hz = (float)((double)items[it].f_hz + K15_DFQ * (double)(best % nf - qf));
    res[it] = r;
  }
}


// ---------------------------------------------------------------- host side
struct trk_state {
  trk_set *set = nullptr;   // uwspr_track_set's
  uwspr_sub_item *d_items = nullptr; size_t cap_items = 0;
  // the caller's items go through page-locked memory and the one wait is for the launch of the call before (K10's door:
  // lanes of a pipe share streams, and a stream synchronisation would wait for the other lane's batch as well)
  uwspr_sub_item *h_items = nullptr; size_t cap_h = 0;
  hipEvent_t done = nullptr; bool pending = false;
  float *d_surf = nullptr; size_t cap_surf = 0;
  float *d_tref = nullptr; size_t cap_tref = 0;
  uwspr_track_result *d_res = nullptr; size_t cap_res = 0;
  launch_timer timer;   // uwspr_debug_track_time: events around the launches of the last call
};

void track_free_set(trk_set *s) {
  if (!s) return;
  if (s->d_dfreq) (void)hipFree(s->d_dfreq);
  if (s->d_tau) (void)hipFree(s->d_tau);
  delete s;
}

void trk_release(uwspr_ctx *c) {
  if (!c || !c->trk) return;
  trk_state *t = c->trk;
  track_free_set(t->set);
  void *bufs[] = {t->d_items, t->d_surf, t->d_tref, t->d_res};
  for (void *b : bufs) if (b) (void)hipFree(b);
  if (t->h_items) (void)hipHostFree(t->h_items);
  if (t->done) (void)hipEventDestroy(t->done);
  t->timer.release();
  delete t;
  c->trk = nullptr;
}

static bool trk_finite(double v) { return v == v && v - v == 0.0; }

// R(t) and Rdot(t) of a trajectory, in the header's one order
static inline void track_range(const uwspr_track_traj &t, double time, double *R, double *Rdot) {
  const double a = t.v * (time - t.tc);
  const double r = sqrt(t.d * t.d + a * a);
  *R = r;
  *Rdot = r > 0.0 ? (t.v * a) / r : 0.0;
}

static void track_tables(const uwspr_track_traj *traj, int n, int model, double cf, double *dfreq, int32_t *tau) {
  const double scale = cf / K15_C;
  for (int j = 0; j < n; j++) {
    double Rm, Dm;
    track_range(traj[j], (double)(K15_SPB * K15_MID + 128) / K15_FS, &Rm, &Dm);
    for (int i = 0; i < K15_NSYM; i++) {
      double R, D;
      track_range(traj[j], (double)(K15_SPB * i + 128) / K15_FS, &R, &D);
      dfreq[(size_t)j * K15_NSYM + i] = -(scale * (D - Dm));
      tau[(size_t)j * K15_NSYM + i] = model == UWSPR_TX_DELAY ? (int32_t)rint((K15_FS * (R - Rm)) / K15_C) : 0;
    }
  }
}

// what makes a trajectory set acceptable: null, or what is wrong (written into msg).  No device is asked.
const char *track_check(const uwspr_track_traj *traj, int n, int nmax, int qf, int model, char *msg, size_t cap) {
  if (n < 1 || n > nmax || !traj) { snprintf(msg, cap, "traj %p, n %d (1..%d)", (const void *)traj, n, nmax); return msg; }
  if (qf < 0 || qf > K15_QFMAX) { snprintf(msg, cap, "qf %d (0..%d)", qf, K15_QFMAX); return msg; }
  if (model != UWSPR_TX_DOPPLER && model != UWSPR_TX_DELAY) { snprintf(msg, cap, "model %d (UWSPR_TX_DOPPLER or UWSPR_TX_DELAY)", model); return msg; }
  for (int j = 0; j < n; j++) {
    const uwspr_track_traj &t = traj[j];
    if (!trk_finite(t.v) || !trk_finite(t.d) || !trk_finite(t.tc) || t.v < 0.0 || t.v > 10.0 || t.d < 1.0 || t.d > 1e6 || fabs(t.tc) > 1e4) {
      snprintf(msg, cap, "trajectory %d: v %g m/s (0..10), d %g m (1..1e6), tc %g s (|.| <= 1e4)", j, t.v, t.d, t.tc);
      return msg;
    }
  }
  return nullptr;
}

// a checked set designed on the host and uploaded to the current device; null with *status and msg on failure
trk_set *track_build(const uwspr_track_traj *traj, int n, int qf, int model, double cf, int *status, char *msg, size_t cap) {
  const size_t cells = (size_t)n * K15_NSYM;
  std::vector<double> df(cells), dft(cells);
  std::vector<int32_t> ta(cells), tat(cells);
  track_tables(traj, n, model, cf, df.data(), ta.data());
  for (int j = 0; j < n; j++)
    for (int i = 0; i < K15_NSYM; i++) {
      const int32_t t = ta[(size_t)j * K15_NSYM + i];
      if (t < -K15_TMAX || t > K15_TMAX) {   // (no allowed trajectory gets here: the kernel's window is made for this bound)
        snprintf(msg, cap, "trajectory %d: delay %d samples at symbol %d (|.| <= %d)", j, t, i, K15_TMAX);
        *status = UWSPR_ERR_ARG;
        return nullptr;
      }
      dft[(size_t)i * n + j] = df[(size_t)j * K15_NSYM + i];
      tat[(size_t)i * n + j] = t;
    }
  trk_set *s = new trk_set();
  s->n = n; s->qf = qf; s->model = model;
  hipError_t e = hipMalloc((void **)&s->d_dfreq, cells * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&s->d_tau, cells * sizeof(int32_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    snprintf(msg, cap, "hipMalloc(%zu bytes) for the tables: %s", cells * 12, hipGetErrorString(e));
    *status = UWSPR_ERR_NOMEM;
    track_free_set(s);
    return nullptr;
  }
  e = hipMemcpy(s->d_dfreq, dft.data(), cells * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->d_tau, tat.data(), cells * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    snprintf(msg, cap, "upload of the tables: %s", hipGetErrorString(e));
    *status = UWSPR_ERR_HIP;
    track_free_set(s);
    return nullptr;
  }
  return s;
}

static int track_hyps(const trk_set *s) { return s ? s->n * (2 * s->qf + 1) : 0; }

// The launches, on the context's stream.  set: null = the set of uwspr_track_set.  src: device frames, frame b at src +
// 2 stride b floats.  items: host records that passed subtract_check, nitems > 0.  res, surface: device memory, or null = a
// buffer of the context (the results' handed back through *res_out).
int track_run(uwspr_ctx *c, const trk_set *set, const float *src, size_t stride, const uwspr_sub_item *items, int nitems,
              uwspr_track_result *res, float *surface, uwspr_track_result **res_out) {
  int rc = ctx_device_ready(c);
  if (rc) return rc;
  if (!c->trk) c->trk = new trk_state();
  trk_state *t = c->trk;
  if (!set) set = t->set;
  if (!set) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_track_batch: no trajectory set (uwspr_track_set)");
  const int nf = 2 * set->qf + 1, nh = set->n * nf;
  if ((rc = ctx_grow(c, &t->d_items, &t->cap_items, (size_t)nitems))) return rc;
  if ((rc = ctx_grow(c, &t->d_tref, &t->cap_tref, (size_t)nitems))) return rc;
  if (!surface) {
    if ((rc = ctx_grow(c, &t->d_surf, &t->cap_surf, (size_t)nitems * nh))) return rc;
    surface = t->d_surf;
  }
  if (!res) {
    if ((rc = ctx_grow(c, &t->d_res, &t->cap_res, (size_t)nitems))) return rc;
    res = t->d_res;
  }
  if (res_out) *res_out = res;
  if (!t->done) CTXCHK(c, hipEventCreateWithFlags(&t->done, hipEventDisableTiming));
  if (t->pending) { CTXCHK(c, hipEventSynchronize(t->done)); t->pending = false; }   // the call before has read both item buffers
  if ((size_t)nitems > t->cap_h) {
    if (t->h_items) { CTXCHK(c, hipHostFree(t->h_items)); t->h_items = nullptr; t->cap_h = 0; }
    const size_t m = nitems > 256 ? (size_t)nitems : 256;
    if (hipHostMalloc((void **)&t->h_items, m * sizeof(uwspr_sub_item), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      t->h_items = nullptr;
      return ctx_fail(c, UWSPR_ERR_NOMEM, "hipHostMalloc(%zu bytes) for the items", m * sizeof(uwspr_sub_item));
    }
    t->cap_h = m;
  }
  memcpy(t->h_items, items, (size_t)nitems * sizeof(uwspr_sub_item));
  CTXCHK(c, hipMemcpyAsync(t->d_items, t->h_items, (size_t)nitems * sizeof(uwspr_sub_item), hipMemcpyHostToDevice, c->stream));
  if ((rc = t->timer.begin(c))) return rc;
  const int ntiles = (set->n + K15_TILE - 1) / K15_TILE, nchunks = (nf + K15_QC - 1) / K15_QC;
  for (int i0 = 0; i0 < nitems; i0 += 32768) {   // (a grid's y extent)
    const int m = nitems - i0 < 32768 ? nitems - i0 : 32768;
    hipLaunchKernelGGL(k15_track, dim3((unsigned)(ntiles * nchunks + 1), (unsigned)m), dim3(K15_TILE), 0, c->stream,
                       reinterpret_cast<const float2 *>(src), stride, c->fc.fl, t->d_items + i0, set->d_dfreq, set->d_tau, set->n, set->qf,
                       nchunks, surface + (size_t)i0 * nh, t->d_tref + i0);
    hipLaunchKernelGGL(k15_pick, dim3((unsigned)m), dim3(256), 0, c->stream, t->d_items + i0, surface + (size_t)i0 * nh, t->d_tref + i0,
                       nh, nf, set->qf, res + i0);
  }
  CTXCHK(c, hipGetLastError());
  CTXCHK(c, hipEventRecord(t->done, c->stream));
  t->pending = true;
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_track_design(const uwspr_track_traj *traj, int n, int model, double cf, double *dfreq, int32_t *tau) {
  char msg[256];
  if (track_check(traj, n, 1 << 20, 0, model, msg, sizeof(msg)) || !trk_finite(cf) || cf <= 0.0 || cf > 1e6 || !dfreq || !tau) return UWSPR_ERR_ARG;
  track_tables(traj, n, model, cf, dfreq, tau);
  return UWSPR_OK;
}

extern "C" int uwspr_track_from_slm(double v1, double v2, double p1, double p2, double t_first, uwspr_track_traj *out) {
  if (!out || !trk_finite(v1) || !trk_finite(v2) || !trk_finite(p1) || !trk_finite(p2) || !trk_finite(t_first)) return UWSPR_ERR_ARG;
  const double vv = v1 * v1 + v2 * v2;
  if (vv > 0.0) {
    const double v = sqrt(vv);
    out->v = v;
    out->d = fabs(v1 * p2 - v2 * p1) / v;
    out->tc = -(v1 * p1 + v2 * p2) / vv - t_first;
  } else {
    out->v = 0.0;
    out->d = sqrt(p1 * p1 + p2 * p2);
    out->tc = 0.0;
  }
  return UWSPR_OK;
}

extern "C" int uwspr_track_set(uwspr_ctx *c, const uwspr_track_traj *traj, int n, int qf, int model) {
  if (!c) return UWSPR_ERR_ARG;
  char msg[256];
  if (track_check(traj, n, UWSPR_TRACK_MAX, qf, model, msg, sizeof(msg))) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_track_set: %s", msg);
  if (const int rc0 = ctx_device_ready(c)) return rc0;
  int rc = UWSPR_OK;
  trk_set *fresh = track_build(traj, n, qf, model, (double)c->p.cf, &rc, msg, sizeof(msg));
  if (!fresh) return ctx_fail(c, rc, "uwspr_track_set: %s", msg);
  if (!c->trk) c->trk = new trk_state();
  trk_state *t = c->trk;
  if (t->pending) {   // the set before may still be read by the call before
    const hipError_t e = hipEventSynchronize(t->done);
    if (e != hipSuccess) { track_free_set(fresh); return ctx_fail(c, UWSPR_ERR_HIP, "uwspr_track_set: hipEventSynchronize: %s", hipGetErrorString(e)); }
    t->pending = false;
  }
  track_free_set(t->set);
  t->set = fresh;
  return UWSPR_OK;
}

extern "C" int uwspr_track_batch(uwspr_ctx *c, const float *frames, int B, int where, const uwspr_sub_item *items, int nitems,
                                 uwspr_track_result *res, float *surface) {
  if (!c) return UWSPR_ERR_ARG;
  if (!frames || B <= 0 || (where != UWSPR_HOST && where != UWSPR_DEVICE && where != UWSPR_DEVICE_FRAMES) || (nitems > 0 && !res))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_track_batch: frames %p, B %d, where %d, res %p", (const void *)frames, B, where, (void *)res);
  int rc = subtract_check(c, items, nitems, B);
  if (rc) return rc;
  const trk_set *set = c->trk ? c->trk->set : nullptr;
  if (!set) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_track_batch: no trajectory set (uwspr_track_set)");
  if (nitems == 0) return UWSPR_OK;
  if ((rc = ctx_device_ready(c))) return rc;
  const size_t nres = (size_t)nitems * sizeof(uwspr_track_result), nsurf = (size_t)nitems * track_hyps(set) * sizeof(float);
  const bool dev_out = where != UWSPR_HOST;
  if (dev_out && (!ctx_device_range(c, res, nres) || (surface && !ctx_device_range(c, surface, nsurf))))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_track_batch: device output needs res (%zu bytes) and surface (%zu bytes) inside device allocations of device %d",
                    nres, nsurf, c->device);
  const float *src = nullptr;
  if ((rc = api_frames_on_device(c, frames, B, where, &src))) return rc;
  trk_state *t = c->trk;
  float *d_surf = dev_out ? surface : nullptr;
  if (!dev_out && surface) {   // (the context's own buffer is then the one track_run would take: named here to copy it out)
    if ((rc = ctx_grow(c, &t->d_surf, &t->cap_surf, (size_t)nitems * track_hyps(set)))) return rc;
    d_surf = t->d_surf;
  }
  uwspr_track_result *d_res = nullptr;
  if ((rc = track_run(c, set, src, (size_t)c->fstride, items, nitems, dev_out ? res : nullptr, d_surf, &d_res))) return rc;
  if (!dev_out) {
    CTXCHK(c, hipMemcpyAsync(res, d_res, nres, hipMemcpyDeviceToHost, c->stream));
    if (surface) CTXCHK(c, hipMemcpyAsync(surface, d_surf, nsurf, hipMemcpyDeviceToHost, c->stream));
  }
  if (where != UWSPR_DEVICE) CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// Measurement hook of tools/track_probe.py (not part of the ABI, like uwspr_debug_blockdemod_time): enable = 1 / 0 switches
// HIP events around the K15 launches of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
// timed call and returns its time.
extern "C" int uwspr_debug_track_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->trk) c->trk = new trk_state();   // (no device asked: the hook only keeps the switch)
  return c->trk->timer.read(c, enable, ms);
}
