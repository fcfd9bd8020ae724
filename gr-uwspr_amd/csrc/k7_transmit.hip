// K7 -- the transmitter: WSPR channel symbols -> 375 S/s complex baseband -> 12 kS/s audio.
//
// The reference's sender is two programs.  wsprsim writes a .c2 file: unit-amplitude continuous-phase 4-FSK at 375 S/s,
// tone s at (s - 1.5) 375/256 Hz (as uwspr_c2_read returns the file), 256 samples per symbol, the phase accumulated
// exclusively from 0 (theta[i + 1] = theta[i] + 2 pi f[i] / 375), the first symbol at sample 375.  examples/c2ToWaveFile.grc turns that into
// 12 kS/s audio with GNU Radio blocks: zero-stuff x32 with h1 = low_pass(1, 12000, 200, 10, HAMMING) (2891 taps), then
// h2 = low_pass(1, 12000, 2500, 100, HAMMING) (289 taps) rotated to 1500 Hz, the output mixed by e^{-j 2 pi 1500 n / 12000}
// and its real part taken.  Every stage is linear and the mixer's period (8 samples) divides 32, so the chain is ONE
// causal complex FIR on the 375 S/s input -- the transpose of K0:
//
//     audio[n] = Re sum_j g[n - 32 j] x[j],     g[q] = e^{-j pi q / 4} sum_k h2[k] e^{+j pi k / 4} h1[q - k]   (3179 taps)
//
// Output phase p = n mod 32 meets the taps g[p + 32 i], i = 0..99 (padded to K7_T = 104): two FMAs per tap, since only
// the real part is wanted.  The file holds e^{-j theta} (uwspr_c2_read's conjugate) and the chain inverts the spectrum
// once more, so a tone at f Hz as uwspr_c2_read sees the baseband is audio 1500 + f Hz.
//
// Mapping (K0's, transposed).  A 1024-thread workgroup owns 16384 consecutive audio samples of ONE channel, i.e. 512
// baseband steps m = mb .. mb + 511.  It renders the 616 baseband samples they read (x[mb - 104 .. mb + 511]: every
// signal of the channel, in ascending signal index) straight into LDS -- no baseband in HBM.  Wavefront w owns output
// phases 2w and 2w + 1, a lane owns EIGHT consecutive steps of a phase, so one staged sample read feeds 16 FMAs (a
// sliding window of 16 samples lives in registers) and the taps come as wave-uniform LDS reads.  Baseband column col is
// stored at [col mod 8][col div 8], so the 64 lanes of a read hit consecutive words.  The results go through LDS once
// more to be written in sample order, after the channel's noise and background are added and the value quantised.
// An output's arithmetic does not depend on where it falls in a workgroup or a launch: renders of any pieces
// concatenate to the same bytes.  1.44 M outputs x 100 taps x 2 FMAs = 0.58 GFLOP per 2-minute channel record.
//
// Moving sources (uwspr_tx_*_moving, the straight-line model of include/uwspr_hip.h): a signal with a motion gets one
// more binary64 hypot per baseband sample, R(t) of its trajectory, folded into the same single sincos; in DELAY mode the
// symbol lookup takes the fractional index k' = k - 375 D(t).  Those launches are the <MOVING = true> instances of the
// kernels, so static renders run the code they ran before.  R(t_first) is evaluated once per signal ON THE DEVICE
// (k7_motion_prep), with the hypot the samples use: a zero-velocity trajectory has D = 0 exactly, so k' = k and the
// phase are the static ones bit for bit.
//
// Another carrier, and several at once (<CARRIER = true>; include/uwspr_hip.h states it to the bit).  With n = q + 32 j
// the mixer at fc factors into e^{-j 2 pi fc q / 12000}, which goes into the taps (g_fc: as many taps whatever fc is),
// and e^{-j 2 pi fc j / 375}, a rotator on baseband sample j with 375 values -- K0's table, and the identity when 375
// divides fc.  A channel's signals are grouped by carrier; the workgroup loops over its channel's groups in ascending
// Hz: render the group's 616 samples (rotated by the lane that makes them), stage that carrier's tap image, run the same
// FIR loop, and store the chain to the output staging (first group) or add it there (one binary32 add per later group).
// A chain starts at +0 and never becomes -0, so a group whose signals are all silent adds +0 and changes no byte:
// the host may drop signals outside a call's window, and pieces still concatenate.  The four <CARRIER = false>
// instances are the kernels they were; with every carrier at 1500 Hz and the cut-off at 2500 Hz they are what runs.
//
// A medium between source and hydrophone (<MEDIUM = true>, on the carrier form only; include/uwspr_hip.h states it to the
// bit).  A faded signal's sample is multiplied by h(k) = a0 + a1 sum_m e^{j (w_m k + phi_m)}, k = j - start: up to 32 more
// binary64 sincos per baseband sample, in the staging loop -- the FIR reads what it always read.  A channel's impulses
// (Bernoulli-Gaussian bursts, Philox blocks of their own) are added in the epilogue between the AWGN and the background.
// Calls in which nothing fades and no channel has impulses run the kernels they ran before.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <complex>
#include <map>
#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K7_DEC = 32;
constexpr int K7_NT = 3179;                      // composite taps (2891 + 289 - 1)
constexpr int K7_T = 104;                        // taps per output phase: ceil(3179 / 32) = 100, padded to 13 x 8
constexpr int K7_WG = 1024;                      // 16 wavefronts x 2 output phases
constexpr int K7_R = 8;                          // baseband steps per lane and phase
constexpr int K7_M = 64 * K7_R;                  // baseband steps per workgroup (512)
constexpr int K7_OUT = K7_DEC * K7_M;            // audio samples per workgroup (16384)
constexpr int K7_G = K7_M / 8 + K7_T / 8;        // LDS column groups of 8 baseband samples (77)
constexpr int K7_NX = 8 * K7_G;                  // baseband samples a workgroup reads (616)
constexpr int K7_YP = K7_M + 1;                  // output staging: floats per phase row (+1: reads in sample order hit 32 banks)
constexpr int K7_NSYM = UWSPR_NSYM, K7_SPB = 256, K7_NTX = K7_NSYM * K7_SPB;   // 41472 samples per transmission
constexpr double K7_FS = 375.0;
constexpr double K7_TWO_PI = 6.283185307179586476925286766559;

static size_t k7_lds_bytes() {
  return (size_t)K7_NX * sizeof(float2) + (size_t)K7_DEC * K7_T * sizeof(float2) + (size_t)K7_DEC * K7_YP * sizeof(float);
}

// One signal as the kernels read it.  Phase of sample k = 256 q + r (symbol q) of the transmission, binary64:
//     theta = ph[q] + r (2 pi (sym[q] - 1.5) / 256 + wf) + wd (r (256 q - (N - 1) / 2) + r (r - 1) / 2)
// = phase0 + sum_{u < k} 2 pi f[u] / 375 with f[u] = f0 + (s - 1.5) 375/256 + drift (u - (N - 1) / 2) / (N - 1): the
// exclusive accumulation, evaluated from per-symbol prefix sums so that any window renders without a sequential scan.
struct tx_dsig {
  long long start;      // baseband index of the first symbol's first sample
  int channel;
  float gain;
  double wf;            // 2 pi f0 / 375 (rad per sample)
  double wd;            // 2 pi drift / ((N - 1) 375) (rad per sample^2)
  double ph[K7_NSYM];   // phase at the first sample of each symbol, phase0 included
  uint8_t sym[K7_NSYM];
  uint16_t fc;          // the signal's carrier in Hz: a motion's Doppler phase is -2 pi fc D(t) (carved out of the padding)
  uint8_t _pad[4];
};
static_assert(sizeof(tx_dsig) % 8 == 0, "tx_dsig is 8-byte aligned in arrays");
static_assert(sizeof(tx_dsig) == 16 + 8 * (2 + K7_NSYM) + K7_NSYM + 6, "tx_dsig keeps its size: the carrier lives in the padding");

// A signal's motion as the kernels read it, beside its tx_dsig (same index).  r0 and rref are filled in on the device.
struct tx_dmot {
  double v1, v2, p1, p2, t_first;
  double r0;            // R(t_first)
  double rref;          // R(t_first), or 0 with UWSPR_TX_ABSOLUTE: D(t) = (R(t) - rref) / c
  long long lo, hi;     // k = j - start outside [lo, hi) adds nothing (DELAY: a conservative bound on the support)
  int model;            // UWSPR_TX_STATIC / DOPPLER / DELAY
  int flags;
};
static_assert(sizeof(tx_dmot) % 8 == 0, "tx_dmot is 8-byte aligned in arrays");
constexpr double K7_C = 1500.0;   // sound speed (slm.cc)

struct tx_dchan {
  float sigma, bg_gain;
  unsigned long long seed;
  const void *bg;       // device memory, or null
  long long bg_len;
  int bg_s16;
  int sig0, nsig;       // the channel's signals: sigs[sig0 .. sig0 + nsig) (sorted by channel, index order kept)
  int _pad;
};

// The carrier form's tables, one device block in place of the 1500 Hz tap image (so that the kernel's arguments are the
// other forms'): rot[375] (float2, uwspr_frontend_rotator's table), goff[K7_GOFF] (int: channel c's groups are
// grps[goff[c] .. goff[c + 1]), ascending carrier), grps[goff[C]], then the call's tap images [NG][32][K7_T] (float2).
struct tx_dgrp {
  int fcm;              // carrier mod 375 (0: no rotator)
  int img;              // the carrier's tap image in the block
  int sig0, nsig;       // the group's signals: sigs[sig0 .. sig0 + nsig) (sorted by (channel, carrier), index order kept)
};
constexpr int K7_NROT = 375;
constexpr int K7_GOFF = UWSPR_PIPE_MAX_CHANNELS + 2;   // C + 1 offsets, padded to keep what follows 16-byte aligned
constexpr int K7_MAX_CARRIERS = 64;                    // distinct carriers in one call
static_assert((K7_NROT * sizeof(float2) + K7_GOFF * sizeof(int)) % 16 == 0 && sizeof(tx_dgrp) == 16, "the block's parts stay aligned");

// A signal's fade as the kernels read it, beside its tx_dsig (same index): uwspr_tx_fade_design's output.  paths = 0: the
// signal does not fade.
constexpr int K7_FADE_MAX = 32;
struct tx_dfade {
  double a0, a1;
  int paths;
  int _pad;
  double om[K7_FADE_MAX];   // rad per baseband sample
  double ph[K7_FADE_MAX];
};
static_assert(sizeof(tx_dfade) == 24 + 16 * K7_FADE_MAX, "tx_dfade is 8-byte aligned in arrays");

// A channel's impulses as the kernels read them, beside its tx_dchan (same index).  thr = 0: none.
struct tx_dimp {
  unsigned long long seed;
  uint32_t thr;         // index e is an event when word x of its block is below thr
  float sigma;
  int length;
  int _pad;
};
static_assert(sizeof(tx_dimp) == 24, "tx_dimp is 8-byte aligned in arrays");

// ---------------------------------------------------------------- device side
__device__ __forceinline__ void tx_add(const tx_dsig &s, long long j, float &re, float &im) {
  const long long k = j - s.start;
  if (k < 0 || k >= K7_NTX) return;
  const int q = (int)(k >> 8);
  const double r = (double)(int)(k & 255);
  const double th = s.ph[q] + r * (K7_TWO_PI * ((double)s.sym[q] - 1.5) / 256.0 + s.wf) +
                    s.wd * (r * ((double)(256 * q) - 0.5 * (K7_NTX - 1)) + 0.5 * r * (r - 1.0));
  double sn, cs;
  sincos(th, &sn, &cs);
  re += s.gain * (float)cs;
  im -= s.gain * (float)sn;
}

// tx_add for a signal with a motion.  theta at k' = 256 q + r (r fractional in DELAY mode) is tx_add's expression; with
// D = 0 (zero velocity, no ABSOLUTE) k' = k and every operation below repeats tx_add's on the same values.
__device__ __forceinline__ void tx_add_moving(const tx_dsig &s, const tx_dmot &m, long long j, float &re, float &im) {
  if (m.model == UWSPR_TX_STATIC) { tx_add(s, j, re, im); return; }
  const long long k = j - s.start;
  if (k < m.lo || k >= m.hi) return;
  const double t = m.t_first + (double)k / K7_FS;
  const double R = hypot(m.v1 * t + m.p1, m.v2 * t + m.p2);
  const double d = (R - m.rref) / K7_C;                      // D(t), s
  double kp = (double)k;
  if (m.model == UWSPR_TX_DELAY) {
    kp -= K7_FS * d;
    if (!(kp >= 0.0 && kp < (double)K7_NTX)) return;
  }
  const int q = (int)floor(kp * (1.0 / 256.0));
  const double r = kp - 256.0 * (double)q;
  const double th = s.ph[q] + r * (K7_TWO_PI * ((double)s.sym[q] - 1.5) / 256.0 + s.wf) +
                    s.wd * (r * ((double)(256 * q) - 0.5 * (K7_NTX - 1)) + 0.5 * r * (r - 1.0)) -
                    (K7_TWO_PI * (double)s.fc) * d;
  const float g = (m.flags & UWSPR_TX_SPREADING) ? (float)((double)s.gain * (m.r0 / R)) : s.gain;
  double sn, cs;
  sincos(th, &sn, &cs);
  re += g * (float)cs;
  im -= g * (float)sn;
}

// The medium form's tx_add / tx_add_moving: theta, the gain and the support are theirs, expression for expression (with
// D = 0 the Doppler term is not subtracted at all, as tx_add has it); a signal with f.paths = 0 ends as they end, a faded
// one is turned by h(k), k = j - start, in binary64 before the one rounding to binary32.
template <bool MOVING>
__device__ __forceinline__ void tx_add_medium(const tx_dsig &s, const tx_dmot *m, const tx_dfade &f, long long j,
                                              float &re, float &im) {
  const long long k = j - s.start;
  bool moves = false;
  if constexpr (MOVING) moves = m->model != UWSPR_TX_STATIC;
  int q;
  double r, th;
  float g = s.gain;
  if (moves) {
    if (k < m->lo || k >= m->hi) return;
    const double t = m->t_first + (double)k / K7_FS;
    const double R = hypot(m->v1 * t + m->p1, m->v2 * t + m->p2);
    const double d = (R - m->rref) / K7_C;
    double kp = (double)k;
    if (m->model == UWSPR_TX_DELAY) {
      kp -= K7_FS * d;
      if (!(kp >= 0.0 && kp < (double)K7_NTX)) return;
    }
    q = (int)floor(kp * (1.0 / 256.0));
    r = kp - 256.0 * (double)q;
    th = s.ph[q] + r * (K7_TWO_PI * ((double)s.sym[q] - 1.5) / 256.0 + s.wf) +
         s.wd * (r * ((double)(256 * q) - 0.5 * (K7_NTX - 1)) + 0.5 * r * (r - 1.0)) -
         (K7_TWO_PI * (double)s.fc) * d;
    if (m->flags & UWSPR_TX_SPREADING) g = (float)((double)s.gain * (m->r0 / R));
  } else {
    if (k < 0 || k >= K7_NTX) return;
    q = (int)(k >> 8);
    r = (double)(int)(k & 255);
    th = s.ph[q] + r * (K7_TWO_PI * ((double)s.sym[q] - 1.5) / 256.0 + s.wf) +
         s.wd * (r * ((double)(256 * q) - 0.5 * (K7_NTX - 1)) + 0.5 * r * (r - 1.0));
  }
  double sn, cs;
  sincos(th, &sn, &cs);
  if (f.paths > 0) {
    const double kd = (double)k;
    double sr = 0.0, si = 0.0;
    for (int p = 0; p < f.paths; p++) {       // m ascending, one binary64 add each
      double sp, cp;
      sincos(f.om[p] * kd + f.ph[p], &sp, &cp);
      sr += cp;
      si += sp;
    }
    const double hr = f.a0 + f.a1 * sr, hi = f.a1 * si;
    const double yr = cs * hr - sn * hi, yi = cs * hi + sn * hr;
    re += g * (float)yr;
    im -= g * (float)yi;
  } else {
    re += g * (float)cs;
    im -= g * (float)sn;
  }
}

template <bool MOVING>
__device__ __forceinline__ float2 tx_baseband_medium(const tx_dsig *__restrict__ sigs, const tx_dmot *__restrict__ mots,
                                                     const tx_dfade *__restrict__ fades, int nsig, int ch, long long j) {
  float re = 0.0f, im = 0.0f;
  for (int s = 0; s < nsig; s++)
    if (sigs[s].channel == ch) tx_add_medium<MOVING>(sigs[s], MOVING ? mots + s : nullptr, fades[s], j, re, im);
  return make_float2(re, im);
}

// baseband sample j of a channel in the file's orientation (I + jQ = gain e^{-j theta}: what wsprsim writes and
// c2ToWaveFile reads), signals in ascending index
template <bool MOVING>
__device__ __forceinline__ float2 tx_baseband_at(const tx_dsig *__restrict__ sigs, const tx_dmot *__restrict__ mots,
                                                 int nsig, int ch, long long j) {
  float re = 0.0f, im = 0.0f;
  for (int s = 0; s < nsig; s++)
    if (sigs[s].channel == ch) {
      if constexpr (MOVING) tx_add_moving(sigs[s], mots[s], j, re, im);
      else tx_add(sigs[s], j, re, im);
    }
  return make_float2(re, im);
}

// R(t_first) of every motion, with the hypot tx_add_moving uses (one thread per signal, before the render)
__global__ void k7_motion_prep(tx_dmot *__restrict__ mots, int nsig) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsig) return;
  tx_dmot &m = mots[i];
  const double r0 = hypot(m.v1 * m.t_first + m.p1, m.v2 * m.t_first + m.p2);
  m.r0 = r0;
  m.rref = (m.flags & UWSPR_TX_ABSOLUTE) ? 0.0 : r0;
}

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so a sample's noise depends on (seed, channel, index) only
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
  }
  return c;
}

// one standard normal per (seed, channel, audio index): Box-Muller on the first two words
__device__ __forceinline__ float tx_gauss(unsigned long long seed, int ch, long long n) {
  const uint4 r = philox4x32_10(make_uint4((uint32_t)n, (uint32_t)((unsigned long long)n >> 32), (uint32_t)ch, 0u),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  // (0, 1]: from 2^23 on the + 0.5f rounds to even, so 2^24 - 1 gives u1 = 1 and a sample of exactly 0 (finite)
  const float u1 = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);            // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// tx_gauss's Box-Muller on words x, y of a block that the caller drew
__device__ __forceinline__ float tx_gauss_of(uint4 r) {
  const float u1 = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// What channel ch's impulses add to audio sample n, v being the sample after its AWGN: the events e = n - d >= 0,
// d ascending, one binary32 add each.  Event test: counter (e, ch, 1); burst sample d: counter (e, ch, 2 + d).
__device__ __forceinline__ float tx_impulses(const tx_dimp &z, int ch, long long n, float v) {
  const uint2 key = make_uint2((uint32_t)z.seed, (uint32_t)(z.seed >> 32));
  for (int d = 0; d < z.length; d++) {
    const long long e = n - d;
    if (e < 0) break;
    const uint32_t lo = (uint32_t)e, hi = (uint32_t)((unsigned long long)e >> 32);
    if (philox4x32_10(make_uint4(lo, hi, (uint32_t)ch, 1u), key).x < z.thr)
      v += z.sigma * tx_gauss_of(philox4x32_10(make_uint4(lo, hi, (uint32_t)ch, 2u + (uint32_t)d), key));
  }
  return v;
}

__device__ __forceinline__ int16_t tx_s16(float v) {   // fl32(32767 x) clamped to [-32768, 32767], then to nearest, halves to even
  const float q = fminf(fmaxf(32767.0f * v, -32768.0f), 32767.0f);
  return (int16_t)(int)rintf(q);
}

// 8 taps against the 16-sample window S = A ++ B: acc[r] += Re(g[u] x[m + r - u]) = g.x * S.x + g.y * S.y,
// S[8 + r - u] being x[m + r - u] (g.y holds -Im g)
__device__ __forceinline__ void k7_block(float (&acc)[K7_R], const float2 (&A)[8], const float2 (&B)[8],
                                         const float2 *__restrict__ g) {
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const float2 t = g[u];
#pragma unroll
    for (int r = 0; r < K7_R; r++) {
      const float2 s = r < u ? A[8 + r - u] : B[r - u];
      acc[r] = fmaf(t.x, s.x, acc[r]);
      acc[r] = fmaf(t.y, s.y, acc[r]);
    }
  }
}

// the rotator's product in K0's one order (k0_rotate): x * r with r = (c, d)
__device__ __forceinline__ float2 k7_rotate(float2 x, float2 r) {
  return make_float2(fmaf(x.x, r.x, -(x.y * r.y)), fmaf(x.x, r.y, x.y * r.x));
}

// The FIR of one staged window and tap image: lane l, phase p: steps m = mb + 8 l + r.  Tap block t (taps 8t .. 8t+7)
// reads columns 8 (l + 12 - t) .. +15, i.e. groups l + 12 - t (A) and l + 13 - t (B); the next block's B is this
// block's A.  ADD: the chain is added to what ys holds (a later carrier group), one binary32 add.
template <bool ADD>
__device__ __forceinline__ void k7_fir(const float2 *xs, const float2 *tp, float *ys, int tid) {
  const int w = tid >> 6, l = tid & 63;
  for (int h = 0; h < 2; h++) {
    const int p = 2 * w + h;
    const float2 *g = tp + p * K7_T;
    float acc[K7_R];
#pragma unroll
    for (int r = 0; r < K7_R; r++) acc[r] = 0.0f;
    float2 A[8], B[8];
#pragma unroll
    for (int v = 0; v < 8; v++) { B[v] = xs[v * K7_G + l + 13]; A[v] = xs[v * K7_G + l + 12]; }
    k7_block(acc, A, B, g);
    for (int t = 1; t < K7_T / 8; t += 2) {    // two blocks per trip: the window's halves swap roles, no copies
#pragma unroll
      for (int v = 0; v < 8; v++) B[v] = xs[v * K7_G + l + 12 - t];
      k7_block(acc, B, A, g + 8 * t);
#pragma unroll
      for (int v = 0; v < 8; v++) A[v] = xs[v * K7_G + l + 11 - t];
      k7_block(acc, A, B, g + 8 * t + 8);
    }
#pragma unroll
    for (int r = 0; r < K7_R; r++) {
      if constexpr (ADD) ys[p * K7_YP + 8 * l + r] = ys[p * K7_YP + 8 * l + r] + acc[r];
      else ys[p * K7_YP + 8 * l + r] = acc[r];
    }
  }
}

// Workgroup b renders audio [32 mb, 32 mb + 16384) of channel b mod C, mb = nb0 + 512 (b div C), and writes the
// samples that fall in [t0, t0 + nframes) to out[(n - t0) C + ch].
// CARRIER: `taps` is the carrier form's block (tx_dgrp above) and the workgroup walks its channel's carrier groups.  Between
// two groups every wavefront must be done reading the window and the taps before they are staged again (the barrier at
// the loop's head); a thread adds into the ys words it stored itself, so ys needs none until the epilogue.
// MEDIUM (with CARRIER): fades[s] belongs to sigs[s], imps[ch] to chans[ch]; the other instances never read either.
template <bool S16, bool MOVING, bool CARRIER = false, bool MEDIUM = false>
__global__ __launch_bounds__(K7_WG) void k7_render(const tx_dsig *__restrict__ sigs, const tx_dmot *__restrict__ mots, int nsig,
                                                   const tx_dchan *__restrict__ chans, int C,
                                                   const float2 *__restrict__ taps, long long t0, long long nframes,
                                                   long long nb0, void *__restrict__ out,
                                                   const tx_dfade *__restrict__ fades, const tx_dimp *__restrict__ imps) {
  static_assert(CARRIER || !MEDIUM, "the medium form is built on the carrier form");
  extern __shared__ __align__(16) float k7_lds[];
  float2 *xs = reinterpret_cast<float2 *>(k7_lds);          // [8][K7_G]
  float2 *tp = xs + K7_NX;                                  // [32][K7_T]
  float *ys = reinterpret_cast<float *>(tp + K7_DEC * K7_T); // [32][K7_YP]
  const int ch = (int)(blockIdx.x % (unsigned)C);
  const long long mb = nb0 + (long long)(blockIdx.x / (unsigned)C) * K7_M;
  const int tid = threadIdx.x;
  const tx_dchan cz = chans[ch];
  if constexpr (CARRIER) {
    const float2 *rot = taps;
    const int *goff = reinterpret_cast<const int *>(rot + K7_NROT);
    const tx_dgrp *grps = reinterpret_cast<const tx_dgrp *>(goff + K7_GOFF);
    const float2 *images = reinterpret_cast<const float2 *>(grps + goff[C]);
    const int g0 = goff[ch], g1 = goff[ch + 1];              // (the same for the whole workgroup: the barriers below are uniform)
    if (g0 == g1)                                            // no signal: the +0 a chain over silence gives
      for (int e = tid; e < K7_DEC * K7_YP; e += K7_WG) ys[e] = 0.0f;
    for (int g = g0; g < g1; g++) {
      if (g > g0) __syncthreads();
      const tx_dgrp gr = grps[g];
      const tx_dmot *mz = nullptr;
      if constexpr (MOVING) mz = mots + gr.sig0;
      for (int col = tid; col < K7_NX; col += K7_WG) {
        const long long j = mb - K7_T + col;
        float2 x;
        if constexpr (MEDIUM) x = tx_baseband_medium<MOVING>(sigs + gr.sig0, mz, fades + gr.sig0, gr.nsig, ch, j);
        else x = tx_baseband_at<MOVING>(sigs + gr.sig0, mz, gr.nsig, ch, j);
        if (gr.fcm) {
          int jm = (int)(j % K7_NROT);
          if (jm < 0) jm += K7_NROT;                         // j mod 375 in 0 .. 374 for negative j as well
          x = k7_rotate(x, rot[(gr.fcm * jm) % K7_NROT]);
        }
        xs[(col & 7) * K7_G + (col >> 3)] = x;
      }
      const float2 *img = images + (size_t)gr.img * (K7_DEC * K7_T);
      for (int i = tid; i < K7_DEC * K7_T; i += K7_WG) tp[i] = img[i];
      __syncthreads();
      if (g == g0) k7_fir<false>(xs, tp, ys, tid);
      else k7_fir<true>(xs, tp, ys, tid);
    }
  } else {
    const tx_dmot *mz = nullptr;
    if constexpr (MOVING) mz = mots + cz.sig0;
    for (int col = tid; col < K7_NX; col += K7_WG)
      xs[(col & 7) * K7_G + (col >> 3)] = tx_baseband_at<MOVING>(sigs + cz.sig0, mz, cz.nsig, ch, mb - K7_T + col);
    for (int i = tid; i < K7_DEC * K7_T; i += K7_WG) tp[i] = taps[i];
    __syncthreads();

    // (k7_fir<false>'s loop, kept in the kernel's own text: these four instances are the code they were)
    const int w = tid >> 6, l = tid & 63;
    for (int h = 0; h < 2; h++) {
      const int p = 2 * w + h;
      const float2 *g = tp + p * K7_T;
      float acc[K7_R];
#pragma unroll
      for (int r = 0; r < K7_R; r++) acc[r] = 0.0f;
      float2 A[8], B[8];
#pragma unroll
      for (int v = 0; v < 8; v++) { B[v] = xs[v * K7_G + l + 13]; A[v] = xs[v * K7_G + l + 12]; }
      k7_block(acc, A, B, g);
      for (int t = 1; t < K7_T / 8; t += 2) {    // two blocks per trip: the window's halves swap roles, no copies
#pragma unroll
        for (int v = 0; v < 8; v++) B[v] = xs[v * K7_G + l + 12 - t];
        k7_block(acc, B, A, g + 8 * t);
#pragma unroll
        for (int v = 0; v < 8; v++) A[v] = xs[v * K7_G + l + 11 - t];
        k7_block(acc, A, B, g + 8 * t + 8);
      }
#pragma unroll
      for (int r = 0; r < K7_R; r++) ys[p * K7_YP + 8 * l + r] = acc[r];
    }
  }
  __syncthreads();

  tx_dimp iz;
  if constexpr (MEDIUM) iz = imps[ch];
  const long long n0 = (long long)K7_DEC * mb;
  for (int e = tid; e < K7_OUT; e += K7_WG) {
    const long long n = n0 + e;
    if (n < t0 || n - t0 >= nframes) continue;
    float v = ys[(e & 31) * K7_YP + (e >> 5)];
    if (cz.sigma > 0.0f) v += cz.sigma * tx_gauss(cz.seed, ch, n);
    if constexpr (MEDIUM) {
      if (iz.thr) v = tx_impulses(iz, ch, n, v);
    }
    if (cz.bg) {
      const long long i = n % cz.bg_len;
      const float b = cz.bg_s16 ? (float)static_cast<const int16_t *>(cz.bg)[i] * (1.0f / 32768)
                                : static_cast<const float *>(cz.bg)[i];
      v += cz.bg_gain * b;
    }
    const size_t o = (size_t)(n - t0) * (size_t)C + (size_t)ch;
    if constexpr (S16) static_cast<int16_t *>(out)[o] = tx_s16(v);
    else static_cast<float *>(out)[o] = v;
  }
}

// baseband samples [t0, t0 + n) of one channel, as uwspr_c2_read returns a .c2 file (Q negated against the file:
// gain e^{+j theta})
template <bool MOVING, bool MEDIUM = false>
__global__ void k7_baseband(const tx_dsig *__restrict__ sigs, const tx_dmot *__restrict__ mots, int nsig, int ch,
                            long long t0, int n, float2 *__restrict__ out, const tx_dfade *__restrict__ fades) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float2 x;
    if constexpr (MEDIUM) x = tx_baseband_medium<MOVING>(sigs, mots, fades, nsig, ch, t0 + i);
    else x = tx_baseband_at<MOVING>(sigs, mots, nsig, ch, t0 + i);
    out[i] = make_float2(x.x, -x.y);
  }
}

// ---------------------------------------------------------------- host side
struct tx_state {
  float2 *d_taps = nullptr;                     // [32][K7_T] (Re g, -Im g)
  tx_dsig *d_sig = nullptr; size_t cap_sig = 0;
  tx_dmot *d_mot = nullptr; size_t cap_mot = 0;
  tx_dchan *d_chan = nullptr;
  void *d_out = nullptr; size_t cap_out = 0;    // host-output staging (bytes)
  void *d_bg = nullptr; size_t cap_bg = 0;      // host backgrounds staged (bytes)
  // the carrier form (nothing here is made until it first runs)
  void *d_car = nullptr; size_t cap_car = 0;    // the call's block: rotator, group table, tap images (tx_dgrp)
  bool car_ready = false;                       // the carrier instances were given their LDS
  std::map<std::pair<int, int>, std::vector<float2>> images;   // (carrier, cut-off) -> tap image
  // the medium form (nothing here is made until it first runs)
  tx_dfade *d_fade = nullptr; size_t cap_fade = 0;
  tx_dimp *d_imp = nullptr;
  bool med_ready = false;                       // the medium instances were given their LDS
};

void tx_release(uwspr_ctx *c) {
  if (!c || !c->tx) return;
  tx_state *t = c->tx;
  void *bufs[] = {t->d_taps, t->d_sig, t->d_mot, t->d_chan, t->d_out, t->d_bg, t->d_car, t->d_fade, t->d_imp};
  for (void *b : bufs) if (b) (void)hipFree(b);
  delete t;
  c->tx = nullptr;
}

// (not ctx_grow: sized in bytes, and no synchronisation -- tx_begin has synchronised the stream)
static int tx_grow(uwspr_ctx *c, void **buf, size_t *cap, size_t bytes) {
  if (bytes <= *cap && *buf) return UWSPR_OK;
  if (*buf) { CTXCHK(c, hipFree(*buf)); *buf = nullptr; *cap = 0; }
  const size_t n = bytes > 256 ? bytes : 256;
  const hipError_t e = hipMalloc(buf, n);
  if (e != hipSuccess) return ctx_fail(c, UWSPR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", n, hipGetErrorString(e));
  *cap = n;
  return UWSPR_OK;
}

static std::complex<double> tx_octant(long k) {   // e^{+j k pi / 4}, exact octant values
  static const double r = sqrt(0.5);
  static const double cs[8] = {1, r, 0, -r, -1, -r, 0, r}, sn[8] = {0, r, 1, r, 0, -r, -1, -r};
  const int q = (int)(((k % 8) + 8) % 8);
  return std::complex<double>(cs[q], sn[q]);
}

// e^{+j 2 pi fc k / 12000} for an integer carrier and k >= 0: fc k is reduced mod 12000 in integers first, and an angle
// that is a multiple of pi/4 (every k at 1500 Hz) takes the exact octant values
static std::complex<double> tx_mixer(int fc, long k) {
  const long r = ((long)(fc % 12000) * (k % 12000)) % 12000;
  if (r % 1500 == 0) return tx_octant(r / 1500);
  const double a = K7_TWO_PI * (double)r / 12000.0;
  return std::complex<double>(cos(a), sin(a));
}

static bool tx_carrier_ok(int fc, int cutoff) {
  return cutoff >= 500 && cutoff <= 5900 && fc >= 170 && fc <= cutoff - 250;
}

// g_fc[q] = e^{-j 2 pi fc q / 12000} sum_k h2r[k] h1[q - k], h2r[k] = h2[k] e^{+j 2 pi fc k / 12000} = the rotated taps
// as freq_xlating_fir_filter holds them (binary32 pairs), h2 = low_pass(1, 12000, cutoff, 100); designed in binary64.
// (1500, 2500): the mixer is tx_octant at every k, the composite it always was.
static std::vector<std::complex<double>> tx_composite(int fc = UWSPR_CARRIER_DEFAULT, int cutoff = UWSPR_TX_CUTOFF_DEFAULT) {
  const std::vector<float> h1 = lowpass_hamming(12000.0, 200.0, 10.0);             // 2891 taps
  const std::vector<float> h2 = lowpass_hamming(12000.0, (double)cutoff, 100.0);   // 289 taps
  std::vector<std::complex<double>> g(h1.size() + h2.size() - 1, std::complex<double>(0, 0));
  for (size_t k = 0; k < h2.size(); k++) {
    const std::complex<double> z = (double)h2[k] * tx_mixer(fc, (long)k);
    const std::complex<double> zr((double)(float)z.real(), (double)(float)z.imag());
    for (size_t i = 0; i < h1.size(); i++) g[k + i] += zr * (double)h1[i];
  }
  for (size_t q = 0; q < g.size(); q++) g[q] *= std::conj(tx_mixer(fc, (long)q));
  return g;
}

// the taps as the kernel reads them: phase p = n mod 32 holds (Re g, -Im g)[p + 32 i] at [p][i], +0 behind the last tap
static std::vector<float2> tx_tap_image(const std::vector<std::complex<double>> &g) {
  std::vector<float2> img((size_t)K7_DEC * K7_T, make_float2(0.0f, 0.0f));
  for (int p = 0; p < K7_DEC; p++)
    for (int i = 0; i < K7_T; i++) {
      const int q = p + K7_DEC * i;
      if (q < (int)g.size()) img[(size_t)p * K7_T + i] = make_float2((float)g[q].real(), (float)-g[q].imag());
    }
  return img;
}

static int tx_begin(uwspr_ctx *c) {
  if (!c) return UWSPR_ERR_ARG;
  if (const int rc = ctx_device_ready(c)) return rc;
  if (!c->tx) c->tx = new tx_state();
  CTXCHK(c, hipStreamSynchronize(c->stream));   // the scratch below may still be read by the previous call's kernels
  if (!c->tx->d_taps) {
    const std::vector<std::complex<double>> g = tx_composite();
    if ((int)g.size() != K7_NT) return ctx_fail(c, UWSPR_ERR_HIP, "transmit taps: %zu, expected %d", g.size(), K7_NT);
    const std::vector<float2> img = tx_tap_image(g);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess)
      return ctx_fail(c, UWSPR_ERR_HIP, "transmit kernel: %zu bytes of LDS refused", k7_lds_bytes());
    float2 *d = nullptr;
    CTXCHK(c, hipMalloc((void **)&d, img.size() * sizeof(float2)));
    c->tx->d_taps = d;
    CTXCHK(c, hipMemcpy(d, img.data(), img.size() * sizeof(float2), hipMemcpyHostToDevice));
  }
  return UWSPR_OK;
}

static bool tx_finite(double v) { return v == v && v - v == 0.0; }

static double tx_range_r(const uwspr_tx_motion &m, double t) { return hypot(m.v1 * t + m.p1, m.v2 * t + m.p2); }

// R over trajectory times [ta, tb]: R is convex, so its maximum is at an end and its minimum at the closest approach
// clipped to the interval
static void tx_r_range(const uwspr_tx_motion &m, double ta, double tb, double *rmin, double *rmax) {
  const double ra = tx_range_r(m, ta), rb = tx_range_r(m, tb), vv = m.v1 * m.v1 + m.v2 * m.v2;
  const double tc = vv > 0.0 ? std::min(std::max(-(m.v1 * m.p1 + m.v2 * m.p2) / vv, ta), tb) : ta;
  *rmax = std::max(ra, rb);
  *rmin = std::min(std::min(ra, rb), tx_range_r(m, tc));
}

// Check a motion and bound the k = j - start where its signal can be non-zero: [0, N) unless DELAY.  In DELAY mode
// k' = k - 375 D(t(k)) increases with k (|dR/dt| <= 100 m/s < c), so an interval [a, b] with a <= 375 min D - 2 and
// b >= N + 375 max D + 2 (extremes over [a, b] itself) holds the whole support: k' < -2 at a, k' > N + 2 at b.  It is
// found by widening [0, N] until it holds (a contraction: each widening is at most 1/15 of the last).
static int tx_motion_check(uwspr_ctx *c, int i, const uwspr_tx_motion &m, long long *lo, long long *hi) {
  *lo = 0; *hi = K7_NTX;
  if (!tx_finite(m.v1) || !tx_finite(m.v2) || !tx_finite(m.p1) || !tx_finite(m.p2) || !tx_finite(m.t_first))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: motion %d has a non-finite field", i);
  if (m.model < UWSPR_TX_STATIC || m.model > UWSPR_TX_DELAY || (m.flags & ~(UWSPR_TX_ABSOLUTE | UWSPR_TX_SPREADING)))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: motion %d: model %d, flags 0x%x", i, m.model, (unsigned)m.flags);
  if (hypot(m.v1, m.v2) > 100.0 || fabs(m.t_first) > 1e6 || fabs(m.p1) > 1e9 || fabs(m.p2) > 1e9)
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: motion %d: |v| %g m/s (<= 100), t_first %g s (|.| <= 1e6), p (%g, %g) m "
                   "(|.| <= 1e9)", i, hypot(m.v1, m.v2), m.t_first, m.p1, m.p2);
  if (m.model == UWSPR_TX_STATIC) return UWSPR_OK;
  double a = 0.0, b = (double)K7_NTX;
  if (m.model == UWSPR_TX_DELAY) {
    const double ref = (m.flags & UWSPR_TX_ABSOLUTE) ? 0.0 : tx_range_r(m, m.t_first);
    int it = 0;
    for (;; it++) {
      double rmin, rmax;
      tx_r_range(m, m.t_first + a / K7_FS, m.t_first + b / K7_FS, &rmin, &rmax);
      const double na = K7_FS * (rmin - ref) / K7_C - 2.0, nb = K7_NTX + K7_FS * (rmax - ref) / K7_C + 2.0;
      if ((a <= na && b >= nb) || it == 200) break;
      a = std::min(a, na); b = std::max(b, nb);
    }
    if (it == 200 || !(fabs(a) < 1e15 && fabs(b) < 1e15))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: motion %d: no bound on the delayed support", i);
    *lo = (long long)floor(a); *hi = (long long)ceil(b) + 1;
  }
  if (m.flags & UWSPR_TX_SPREADING) {   // R(t_first) / R(t) over the transmission
    double rmin, rmax;
    tx_r_range(m, m.t_first + (double)*lo / K7_FS, m.t_first + (double)(*hi - 1) / K7_FS, &rmin, &rmax);
    if (!(rmin >= 1.0)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: motion %d: SPREADING with R down to %g m (>= 1)", i, rmin);
  }
  return UWSPR_OK;
}

// philox4x32_10 on the host (the fade design's draws)
static void tx_philox_host(const uint32_t ctr[4], uint64_t seed, uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < 10; i++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static bool tx_fade_ok(const uwspr_tx_fade &f) {
  return f.paths >= 1 && f.paths <= K7_FADE_MAX && tx_finite(f.spread_hz) && f.spread_hz >= 0.0 && f.spread_hz <= 20.0 &&
         tx_finite(f.shift_hz) && fabs(f.shift_hz) <= 20.0 && tx_finite(f.k_factor) && f.k_factor >= 0.0 && f.k_factor <= 1e6;
}

// uwspr_tx_fade_design (include/uwspr_hip.h): binary64 throughout, each line one expression of the header's
static int tx_fade_design(const uwspr_tx_fade &f, double a[2], double *omega, double *phi) {
  if (!tx_fade_ok(f)) return UWSPR_ERR_ARG;
  const int M = f.paths;
  if (a) {
    a[0] = sqrt(f.k_factor / (f.k_factor + 1.0));
    a[1] = sqrt(1.0 / ((f.k_factor + 1.0) * (double)M));
  }
  for (int m = 0; m < M; m++) {
    const uint32_t ctr[4] = {(uint32_t)m, 0u, 0x46414445u, 0u};
    uint32_t w[4];
    tx_philox_host(ctr, f.seed, w);
    const double u1 = ((double)(w[0] >> 8) + 0.5) / 16777216.0;
    const double u2 = (double)(w[1] >> 8) / 16777216.0;
    const double u3 = (double)(w[2] >> 8) / 16777216.0;
    const double nu = f.shift_hz + ((f.spread_hz / 2.0) * sqrt(-2.0 * log(u1))) * cos(K7_TWO_PI * u2);
    if (omega) omega[m] = K7_TWO_PI * nu / K7_FS;
    if (phi) phi[m] = K7_TWO_PI * u3;
  }
  return M;
}

// check the records (channel < C when C > 0; motions, when given) and build the device form of those that pass
// keep(s, lo, hi) ([start + lo, start + hi): where the signal may be non-zero)
// car: a carrier per signal in Hz, or null (1500 for all).  Every entry is checked against the context's "tx_cutoff",
// the signals the window drops included; *other (when given) tells whether some signal's carrier is not 1500 Hz.
// fade: a fade per signal, or null; checked like the carriers, designed for the kept signals into *fout (one per kept
// signal, paths = 0 where the signal does not fade).
template <typename Keep>
static int tx_prepare(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *mot, const int32_t *car, int nsig, int C,
                      Keep keep, std::vector<tx_dsig> &out, std::vector<tx_dmot> *mout, bool *other = nullptr,
                      const uwspr_tx_fade *fade = nullptr, std::vector<tx_dfade> *fout = nullptr) {
  if (nsig < 0 || (nsig > 0 && !sig)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signals %p, nsig %d", (const void *)sig, nsig);
  out.clear();
  if (mout) mout->clear();
  if (fout) fout->clear();
  if (other) *other = false;
  const int cutoff = c->opt[UWSPR_OPT_TX_CUTOFF];
  std::vector<int> distinct;
  for (int i = 0; i < nsig; i++) {
    const int fc = car ? car[i] : UWSPR_CARRIER_DEFAULT;
    if (!tx_carrier_ok(fc, cutoff))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d carrier %d Hz (170 .. tx_cutoff - 250 = %d)", i, fc, cutoff - 250);
    if (fc != UWSPR_CARRIER_DEFAULT && other) *other = true;
    if (std::find(distinct.begin(), distinct.end(), fc) == distinct.end()) distinct.push_back(fc);
  }
  if ((int)distinct.size() > K7_MAX_CARRIERS)
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: %zu distinct carriers (<= %d)", distinct.size(), K7_MAX_CARRIERS);
  for (int i = 0; fade && i < nsig; i++)
    if (fade[i].paths != 0 && !tx_fade_ok(fade[i]))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: fade %d: spread %g Hz (0 .. 20), shift %g Hz (|.| <= 20), K %g (0 .. 1e6), paths %d (0 .. %d)",
                     i, fade[i].spread_hz, fade[i].shift_hz, fade[i].k_factor, fade[i].paths, K7_FADE_MAX);
  for (int i = 0; i < nsig; i++) {
    const uwspr_tx_signal &s = sig[i];
    for (int k = 0; k < K7_NSYM; k++)
      if (s.symbols[k] > 3) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d symbol %d = %d (0..3)", i, k, s.symbols[k]);
    if (s.channel < 0 || (C > 0 && s.channel >= C)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d channel %d", i, s.channel);
    if (!tx_finite(s.f0_hz) || !tx_finite(s.drift_hz) || !tx_finite(s.phase0) || !tx_finite((double)s.gain))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d has a non-finite f0 / drift / phase / gain", i);
    if (s.start < -(1LL << 50) || s.start > (1LL << 50)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d start %lld", i, (long long)s.start);
    long long lo = 0, hi = K7_NTX;
    if (mot) {
      const int rc = tx_motion_check(c, i, mot[i], &lo, &hi);
      if (rc) return rc;
      if (s.start + lo < -(1LL << 52) || s.start + hi > (1LL << 52))
        return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: signal %d: delayed support [%lld, %lld)", i, s.start + lo, s.start + hi);
    }
    if (!keep(s, lo, hi)) continue;
    if (mout) {
      const uwspr_tx_motion &m = mot[i];
      tx_dmot dm;
      memset(&dm, 0, sizeof(dm));
      dm.v1 = m.v1; dm.v2 = m.v2; dm.p1 = m.p1; dm.p2 = m.p2; dm.t_first = m.t_first;
      dm.lo = lo; dm.hi = hi; dm.model = m.model; dm.flags = m.flags;
      mout->push_back(dm);
    }
    if (fout) {
      tx_dfade df;
      memset(&df, 0, sizeof(df));
      if (fade && fade[i].paths != 0) {
        double a[2];
        df.paths = tx_fade_design(fade[i], a, df.om, df.ph);
        df.a0 = a[0]; df.a1 = a[1];
      }
      fout->push_back(df);
    }
    tx_dsig d;
    memset(&d, 0, sizeof(d));
    d.start = s.start; d.channel = s.channel; d.gain = s.gain;
    d.fc = (uint16_t)(car ? car[i] : UWSPR_CARRIER_DEFAULT);
    d.wf =K7_TWO_PI * s.f0_hz / K7_FS;
    d.wd = K7_TWO_PI * s.drift_hz / ((double)(K7_NTX - 1) * K7_FS);
    double ph = s.phase0;
    for (int q = 0; q < K7_NSYM; q++) {
      d.ph[q] = ph;
      d.sym[q] = s.symbols[q];
      const double r = 256.0;
      ph += r * (K7_TWO_PI * ((double)s.symbols[q] - 1.5) / 256.0 + d.wf) +
            d.wd * (r * ((double)(256 * q) - 0.5 * (K7_NTX - 1)) + 0.5 * r * (r - 1.0));
    }
    out.push_back(d);
  }
  return UWSPR_OK;
}

static int tx_upload_signals(uwspr_ctx *c, const std::vector<tx_dsig> &v) {
  tx_state *t = c->tx;
  int rc = tx_grow(c, (void **)&t->d_sig, &t->cap_sig, v.size() * sizeof(tx_dsig));
  if (rc) return rc;
  if (!v.empty()) CTXCHK(c, hipMemcpyAsync(t->d_sig, v.data(), v.size() * sizeof(tx_dsig), hipMemcpyHostToDevice, c->stream));
  return UWSPR_OK;
}

static bool tx_any_moving(const std::vector<tx_dmot> &m) {
  for (const tx_dmot &d : m)
    if (d.model != UWSPR_TX_STATIC) return true;
  return false;
}

// the motions beside the signals, R(t_first) filled in on the device
static int tx_upload_motions(uwspr_ctx *c, const std::vector<tx_dmot> &m) {
  tx_state *t = c->tx;
  int rc = tx_grow(c, (void **)&t->d_mot, &t->cap_mot, m.size() * sizeof(tx_dmot));
  if (rc) return rc;
  if (m.empty()) return UWSPR_OK;
  CTXCHK(c, hipMemcpyAsync(t->d_mot, m.data(), m.size() * sizeof(tx_dmot), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k7_motion_prep, dim3((unsigned)((m.size() + 63) / 64)), dim3(64), 0, c->stream, t->d_mot, (int)m.size());
  CTXCHK(c, hipGetLastError());
  return UWSPR_OK;
}

static std::atomic<long long> k7_carrier_launches[2];   // launches of the carrier form since the process started (f32, s16)

// The carrier form's block (tx_dgrp) for signals sorted by (channel, carrier): the rotator table, the groups of every
// channel, and one tap image per distinct carrier of the call (designed once per (carrier, cut-off) and context).  The
// first use also gives the four carrier instances their LDS.
static int tx_carrier_block(uwspr_ctx *c, const std::vector<tx_dsig> &v, int C, int cutoff, std::vector<char> &block) {
  tx_state *t = c->tx;
  if (!t->car_ready) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess)
      return ctx_fail(c, UWSPR_ERR_HIP, "transmit kernel (carrier form): %zu bytes of LDS refused", k7_lds_bytes());
    t->car_ready = true;
  }
  std::vector<int> fcs;                       // the call's distinct carriers, ascending: image index = position
  for (const tx_dsig &s : v) fcs.push_back((int)s.fc);
  std::sort(fcs.begin(), fcs.end());
  fcs.erase(std::unique(fcs.begin(), fcs.end()), fcs.end());
  if ((int)fcs.size() > K7_MAX_CARRIERS) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx: %zu distinct carriers (<= %d)", fcs.size(), K7_MAX_CARRIERS);
  std::vector<int> goff(K7_GOFF, 0);
  std::vector<tx_dgrp> grps;
  size_t i = 0;
  for (int ch = 0; ch < C; ch++) {
    goff[ch] = (int)grps.size();
    while (i < v.size() && v[i].channel == ch) {
      size_t e = i;
      while (e < v.size() && v[e].channel == ch && v[e].fc == v[i].fc) e++;
      tx_dgrp g;
      g.fcm = (int)v[i].fc % K7_NROT;
      g.img = (int)(std::lower_bound(fcs.begin(), fcs.end(), (int)v[i].fc) - fcs.begin());
      g.sig0 = (int)i; g.nsig = (int)(e - i);
      grps.push_back(g);
      i = e;
    }
  }
  for (int ch = C; ch < K7_GOFF; ch++) goff[ch] = (int)grps.size();
  if (i != v.size()) return ctx_fail(c, UWSPR_ERR_HIP, "uwspr_tx: carrier groups cover %zu of %zu signals", i, v.size());
  const size_t img_bytes = (size_t)K7_DEC * K7_T * sizeof(float2);
  const size_t at_goff = K7_NROT * sizeof(float2), at_grps = at_goff + K7_GOFF * sizeof(int);
  const size_t at_img = at_grps + grps.size() * sizeof(tx_dgrp);
  block.assign(at_img + fcs.size() * img_bytes, 0);
  frontend_rotator(reinterpret_cast<float *>(block.data()));
  memcpy(block.data() + at_goff, goff.data(), K7_GOFF * sizeof(int));
  if (!grps.empty()) memcpy(block.data() + at_grps, grps.data(), grps.size() * sizeof(tx_dgrp));
  for (size_t k = 0; k < fcs.size(); k++) {
    const std::pair<int, int> key(fcs[k], cutoff);
    auto it = t->images.find(key);
    if (it == t->images.end()) {
      if (t->images.size() >= 1024) t->images.clear();   // (a sweep over carriers does not grow the cache without bound)
      const std::vector<std::complex<double>> g = tx_composite(fcs[k], cutoff);
      if ((int)g.size() != K7_NT) return ctx_fail(c, UWSPR_ERR_HIP, "transmit taps at %d Hz, cut-off %d Hz: %zu, expected %d", fcs[k], cutoff, g.size(), K7_NT);
      it = t->images.emplace(key, tx_tap_image(g)).first;
    }
    memcpy(block.data() + at_img + k * img_bytes, it->second.data(), img_bytes);
  }
  return UWSPR_OK;
}

}  // namespace uwspr

using namespace uwspr;

static bool tx_any_fading(const std::vector<tx_dfade> &f) {
  for (const tx_dfade &d : f)
    if (d.paths > 0) return true;
  return false;
}

// the fades beside the signals
static int tx_upload_fades(uwspr_ctx *c, const std::vector<tx_dfade> &f) {
  tx_state *t = c->tx;
  int rc = tx_grow(c, (void **)&t->d_fade, &t->cap_fade, f.size() * sizeof(tx_dfade));
  if (rc) return rc;
  if (!f.empty()) CTXCHK(c, hipMemcpyAsync(t->d_fade, f.data(), f.size() * sizeof(tx_dfade), hipMemcpyHostToDevice, c->stream));
  return UWSPR_OK;
}

static std::atomic<long long> k7_medium_launches[3];   // launches of the medium form since the process started (f32, s16, baseband)

static int tx_baseband(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *mot, const int32_t *car,
                       const uwspr_tx_fade *fade, int nsig, int channel, long long t0, int n, float *iq, int where) {
  if (!c) return UWSPR_ERR_ARG;
  if (n < 0 || (n > 0 && !iq) || channel < 0 || (where != UWSPR_HOST && where != UWSPR_DEVICE))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_baseband: n %d, iq %p, channel %d, where %d", n, (void *)iq, channel, where);
  std::vector<tx_dsig> v;
  std::vector<tx_dmot> mv;
  std::vector<tx_dfade> fv;
  int rc = tx_prepare(c, sig, mot, car, nsig, 0, [&](const uwspr_tx_signal &s, long long lo, long long hi) {
    return s.channel == channel && s.start + lo < t0 + n && s.start + hi > t0;
  }, v, mot ? &mv : nullptr, nullptr, fade, fade ? &fv : nullptr);
  if (rc) return rc;
  if (n == 0) return UWSPR_OK;
  if ((rc = ctx_device_ready(c))) return rc;
  if (where == UWSPR_DEVICE && !ctx_device_range(c, iq, (size_t)n * sizeof(float2)))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_baseband: iq %p is not %zu bytes of this device's memory", (void *)iq, (size_t)n * sizeof(float2));
  if ((rc = tx_begin(c))) return rc;
  if ((rc = tx_upload_signals(c, v))) return rc;
  const bool moving = tx_any_moving(mv);
  if (moving && (rc = tx_upload_motions(c, mv))) return rc;
  const bool medium = tx_any_fading(fv);
  if (medium && (rc = tx_upload_fades(c, fv))) return rc;
  tx_state *t = c->tx;
  float2 *dst = (float2 *)iq;
  if (where == UWSPR_HOST) {
    if ((rc = tx_grow(c, &t->d_out, &t->cap_out, (size_t)n * sizeof(float2)))) return rc;
    dst = (float2 *)t->d_out;
  }
  CTXCHK(c, hipStreamSynchronize(c->stream));   // (the records live on this call's stack)
  const int blocks = (n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048;
  const tx_dfade *nofade = nullptr;
  if (medium && moving)
    hipLaunchKernelGGL((k7_baseband<true, true>), dim3(blocks), dim3(256), 0, c->stream, t->d_sig, t->d_mot, (int)v.size(), channel, t0, n, dst, t->d_fade);
  else if (medium)
    hipLaunchKernelGGL((k7_baseband<false, true>), dim3(blocks), dim3(256), 0, c->stream, t->d_sig, (const tx_dmot *)nullptr, (int)v.size(), channel, t0, n, dst, t->d_fade);
  else if (moving)
    hipLaunchKernelGGL(k7_baseband<true>, dim3(blocks), dim3(256), 0, c->stream, t->d_sig, t->d_mot, (int)v.size(), channel, t0, n, dst, nofade);
  else
    hipLaunchKernelGGL(k7_baseband<false>, dim3(blocks), dim3(256), 0, c->stream, t->d_sig, (const tx_dmot *)nullptr, (int)v.size(), channel, t0, n, dst, nofade);
  if (medium) k7_medium_launches[2]++;
  CTXCHK(c, hipGetLastError());
  if (where == UWSPR_HOST) {
    CTXCHK(c, hipMemcpyAsync(iq, dst, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    CTXCHK(c, hipStreamSynchronize(c->stream));
  }
  return UWSPR_OK;
}

static int tx_render(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *mot, const int32_t *car,
                     const uwspr_tx_fade *fade, int nsig, const uwspr_tx_channel *chan, const uwspr_tx_impulse *imp, int C,
                     long long t0, long long nframes, int format, void *out, int where) {
  if (!c) return UWSPR_ERR_ARG;
  if (C < 1 || C > UWSPR_PIPE_MAX_CHANNELS || !chan || t0 < 0 || nframes < 0 || (nframes > 0 && !out) ||
      (format != UWSPR_AUDIO_F32 && format != UWSPR_AUDIO_S16) || (where != UWSPR_HOST && where != UWSPR_DEVICE))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: C %d, chan %p, t0 %lld, nframes %lld, out %p, format %d, where %d",
                   C, (const void *)chan, t0, nframes, out, format, where);
  if (nframes > (1LL << 40) / C) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: %lld frames x %d channels", nframes, C);
  for (int k = 0; k < C; k++) {
    const uwspr_tx_channel &z = chan[k];
    if (!tx_finite(z.sigma) || z.sigma < 0 || !tx_finite((double)z.background_gain) ||
        (z.background && (z.background_len <= 0 || (z.background_format != UWSPR_AUDIO_F32 && z.background_format != UWSPR_AUDIO_S16))))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: channel %d: sigma %g, background %p len %lld format %d gain %g", k,
                     z.sigma, z.background, (long long)z.background_len, z.background_format, (double)z.background_gain);
  }
  // impulses: thr = min(floor(rate 2^32), 2^32 - 1) in binary64; rate 0 or sigma 0 (thr 0 here): none
  std::vector<tx_dimp> di;
  bool impulsive = false;
  if (imp) {
    di.resize(C);
    for (int k = 0; k < C; k++) {
      const uwspr_tx_impulse &z = imp[k];
      if (!tx_finite(z.rate) || z.rate < 0.0 || z.rate > 0.25 || !tx_finite(z.sigma) || z.sigma < 0.0 || z.length < 1 || z.length > 8)
        return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: channel %d: impulse rate %g (0 .. 0.25), sigma %g (>= 0), length %d (1 .. 8)",
                       k, z.rate, z.sigma, z.length);
      tx_dimp &d = di[k];
      memset(&d, 0, sizeof(d));
      d.seed = z.seed; d.sigma = (float)z.sigma; d.length = z.length;
      d.thr = z.sigma > 0.0 ? (uint32_t)std::min(floor(z.rate * 4294967296.0), 4294967295.0) : 0u;
      if (d.thr) impulsive = true;
    }
  }
  // signals that reach [t0, t0 + nframes): audio 32 (start + lo) .. 32 (start + hi - 1) + 3178, [lo, hi) = [0, N)
  // unless delayed (the others add exact zeros)
  std::vector<tx_dsig> v;
  std::vector<tx_dmot> mv;
  std::vector<tx_dfade> fv;
  bool other = false;
  int rc = tx_prepare(c, sig, mot, car, nsig, C, [&](const uwspr_tx_signal &s, long long lo, long long hi) {
    return K7_DEC * (s.start + lo) < t0 + nframes && K7_DEC * (s.start + hi - 1) + K7_NT - 1 >= t0;
  }, v, mot ? &mv : nullptr, &other, fade, fade ? &fv : nullptr);
  if (rc) return rc;
  if (nframes == 0) return UWSPR_OK;
  // the medium form: only when a kept signal fades or a channel has impulses; it is built on the carrier form
  const bool fading = tx_any_fading(fv);
  const bool medium = fading || impulsive;
  // the carrier form: asked for by a carrier, by the cut-off or by "tx_form"; otherwise the 1500 Hz kernels, as ever
  const int cutoff = c->opt[UWSPR_OPT_TX_CUTOFF];
  const bool carrier = medium || other || cutoff != UWSPR_TX_CUTOFF_DEFAULT || c->opt[UWSPR_OPT_TX_FORM] != 0;
  const size_t esz = format == UWSPR_AUDIO_S16 ? 2 : 4;
  if ((rc = ctx_device_ready(c))) return rc;
  if (where == UWSPR_DEVICE) {   // device pointers must be device memory: a host pointer would fault the kernel
    if (!ctx_device_range(c, out, (size_t)nframes * C * esz))
      return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: out %p is not %zu bytes of this device's memory", out, (size_t)nframes * C * esz);
    for (int k = 0; k < C; k++)
      if (chan[k].background &&
          !ctx_device_range(c, chan[k].background, (size_t)chan[k].background_len * (chan[k].background_format == UWSPR_AUDIO_S16 ? 2 : 4)))
        return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: channel %d: background %p is not %lld samples of this device's memory", k,
                       chan[k].background, (long long)chan[k].background_len);
  }
  // the kernel walks only its channel's signals: sorted by channel, ascending index within one (the order they add up in)
  // (a motion moves with its signal); the carrier form: by (channel, carrier), index order kept inside a group
  const bool moving = tx_any_moving(mv);
  const auto before = [carrier](const tx_dsig &a, const tx_dsig &b) {
    return a.channel != b.channel ? a.channel < b.channel : (carrier && a.fc < b.fc);
  };
  if (moving || medium) {   // (a fade moves with its signal too)
    std::vector<int> ix(v.size());
    for (size_t i = 0; i < ix.size(); i++) ix[i] = (int)i;
    std::stable_sort(ix.begin(), ix.end(), [&](int a, int b) { return before(v[a], v[b]); });
    std::vector<tx_dsig> vs(v.size());
    std::vector<tx_dmot> ms(mv.size());
    std::vector<tx_dfade> fs(fv.size());
    for (size_t i = 0; i < ix.size(); i++) {
      vs[i] = v[ix[i]];
      if (!mv.empty()) ms[i] = mv[ix[i]];
      if (!fv.empty()) fs[i] = fv[ix[i]];
    }
    v.swap(vs); mv.swap(ms); fv.swap(fs);
  } else {
    std::stable_sort(v.begin(), v.end(), before);
  }
  if ((rc = tx_begin(c))) return rc;
  tx_state *t = c->tx;
  if ((rc = tx_upload_signals(c, v))) return rc;
  if (moving && (rc = tx_upload_motions(c, mv))) return rc;
  if (medium) {
    if (!t->med_ready) {   // the first use gives the four medium instances their LDS
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<false, true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void *>(k7_render<true, true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k7_lds_bytes()) != hipSuccess)
        return ctx_fail(c, UWSPR_ERR_HIP, "transmit kernel (medium form): %zu bytes of LDS refused", k7_lds_bytes());
      t->med_ready = true;
    }
    if (fv.size() != v.size()) fv.assign(v.size(), tx_dfade());   // (impulses alone: no signal fades)
    if ((rc = tx_upload_fades(c, fv))) return rc;
    if (di.empty()) di.assign(C, tx_dimp());
    if (!t->d_imp) CTXCHK(c, hipMalloc((void **)&t->d_imp, UWSPR_PIPE_MAX_CHANNELS * sizeof(tx_dimp)));
    CTXCHK(c, hipMemcpyAsync(t->d_imp, di.data(), C * sizeof(tx_dimp), hipMemcpyHostToDevice, c->stream));
  }
  // channels: host backgrounds are staged behind each other
  std::vector<tx_dchan> dc(C);
  size_t bg_bytes = 0;
  for (int k = 0; k < C; k++)
    if (chan[k].background && where == UWSPR_HOST)
      bg_bytes += ((size_t)chan[k].background_len * (chan[k].background_format == UWSPR_AUDIO_S16 ? 2 : 4) + 255) / 256 * 256;
  if (bg_bytes && (rc = tx_grow(c, &t->d_bg, &t->cap_bg, bg_bytes))) return rc;
  size_t off = 0;
  for (int k = 0; k < C; k++) {
    const uwspr_tx_channel &z = chan[k];
    tx_dchan &d = dc[k];
    memset(&d, 0, sizeof(d));
    d.sigma = (float)z.sigma; d.bg_gain = z.background_gain; d.seed = z.seed;
    d.sig0 = (int)(std::lower_bound(v.begin(), v.end(), k, [](const tx_dsig &a, int ch) { return a.channel < ch; }) - v.begin());
    d.nsig = (int)(std::upper_bound(v.begin(), v.end(), k, [](int ch, const tx_dsig &a) { return ch < a.channel; }) - v.begin()) - d.sig0;
    if (z.background) {
      d.bg_len = z.background_len; d.bg_s16 = z.background_format == UWSPR_AUDIO_S16;
      if (where == UWSPR_HOST) {
        const size_t b = (size_t)z.background_len * (d.bg_s16 ? 2 : 4);
        CTXCHK(c, hipMemcpyAsync((char *)t->d_bg + off, z.background, b, hipMemcpyHostToDevice, c->stream));
        d.bg = (char *)t->d_bg + off;
        off += (b + 255) / 256 * 256;
      } else {
        d.bg = z.background;
      }
    }
  }
  if (!t->d_chan) CTXCHK(c, hipMalloc((void **)&t->d_chan, UWSPR_PIPE_MAX_CHANNELS * sizeof(tx_dchan)));
  CTXCHK(c, hipMemcpyAsync(t->d_chan, dc.data(), C * sizeof(tx_dchan), hipMemcpyHostToDevice, c->stream));
  std::vector<char> block;
  if (carrier) {
    if ((rc = tx_carrier_block(c, v, C, cutoff, block))) return rc;
    if ((rc = tx_grow(c, &t->d_car, &t->cap_car, block.size()))) return rc;
    CTXCHK(c, hipMemcpyAsync(t->d_car, block.data(), block.size(), hipMemcpyHostToDevice, c->stream));
  }
  CTXCHK(c, hipStreamSynchronize(c->stream));   // (the records above live on this call's stack)

  // device output: one launch; host output: pieces of at most 2^24 samples through a staging buffer (the render of any
  // piece is the same bytes as that part of a whole render)
  const long long piece = where == UWSPR_DEVICE ? nframes : std::max<long long>(K7_OUT, (1LL << 24) / C / K7_OUT * K7_OUT);
  if (where == UWSPR_HOST && (rc = tx_grow(c, &t->d_out, &t->cap_out, (size_t)std::min(piece, nframes) * C * esz))) return rc;
  for (long long k = 0; k < nframes; k += piece) {
    const long long a = t0 + k, len = std::min(piece, nframes - k);
    const long long nb0 = a / K7_DEC;
    const long long nblk = (a + len - K7_DEC * nb0 + K7_OUT - 1) / K7_OUT;
    if (nblk * C > 0x7fffffffLL) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_tx_render: %lld workgroups", nblk * C);
    void *dst = where == UWSPR_HOST ? t->d_out : (void *)((char *)out + (size_t)k * C * esz);
    const dim3 grid((unsigned)(nblk * C));
    const tx_dmot *dm = moving ? t->d_mot : nullptr;
    const tx_dfade *nofade = nullptr;
    const tx_dimp *noimp = nullptr;
    if (medium) {
      const float2 *blk = static_cast<const float2 *>(t->d_car);
      if (format == UWSPR_AUDIO_S16 && moving)
        hipLaunchKernelGGL((k7_render<true, true, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, t->d_fade, t->d_imp);
      else if (format == UWSPR_AUDIO_S16)
        hipLaunchKernelGGL((k7_render<true, false, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, t->d_fade, t->d_imp);
      else if (moving)
        hipLaunchKernelGGL((k7_render<false, true, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, t->d_fade, t->d_imp);
      else
        hipLaunchKernelGGL((k7_render<false, false, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, t->d_fade, t->d_imp);
      k7_medium_launches[format == UWSPR_AUDIO_S16 ? 1 : 0]++;
    } else if (carrier) {
      const float2 *blk = static_cast<const float2 *>(t->d_car);
      if (format == UWSPR_AUDIO_S16 && moving)
        hipLaunchKernelGGL((k7_render<true, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, nofade, noimp);
      else if (format == UWSPR_AUDIO_S16)
        hipLaunchKernelGGL((k7_render<true, false, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, nofade, noimp);
      else if (moving)
        hipLaunchKernelGGL((k7_render<false, true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, nofade, noimp);
      else
        hipLaunchKernelGGL((k7_render<false, false, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                           t->d_chan, C, blk, a, len, nb0, dst, nofade, noimp);
      k7_carrier_launches[format == UWSPR_AUDIO_S16 ? 1 : 0]++;
    } else if (format == UWSPR_AUDIO_S16 && moving)
      hipLaunchKernelGGL((k7_render<true, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                         t->d_chan, C, t->d_taps, a, len, nb0, dst, nofade, noimp);
    else if (format == UWSPR_AUDIO_S16)
      hipLaunchKernelGGL((k7_render<true, false>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                         t->d_chan, C, t->d_taps, a, len, nb0, dst, nofade, noimp);
    else if (moving)
      hipLaunchKernelGGL((k7_render<false, true>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                         t->d_chan, C, t->d_taps, a, len, nb0, dst, nofade, noimp);
    else
      hipLaunchKernelGGL((k7_render<false, false>), grid, dim3(K7_WG), k7_lds_bytes(), c->stream, t->d_sig, dm, (int)v.size(),
                         t->d_chan, C, t->d_taps, a, len, nb0, dst, nofade, noimp);
    CTXCHK(c, hipGetLastError());
    if (where == UWSPR_HOST) {
      CTXCHK(c, hipMemcpyAsync((char *)out + (size_t)k * C * esz, dst, (size_t)len * C * esz, hipMemcpyDeviceToHost, c->stream));
      CTXCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  return UWSPR_OK;
}

// Test door (not part of the ABI, like uwspr_debug_frontend_launch): the binary64 composite g [3179][2] (re, im) and the
// tap image [32][104][2] as tx_begin uploads it.  Host only: no context, no device.  Either pointer may be null.
extern "C" int uwspr_debug_tx_taps(double *g, float *image) {
  const std::vector<std::complex<double>> t = tx_composite();
  if ((int)t.size() != K7_NT) return UWSPR_ERR_ARG;
  if (g)
    for (int q = 0; q < K7_NT; q++) { g[2 * q] = t[q].real(); g[2 * q + 1] = t[q].imag(); }
  if (image) {
    const std::vector<float2> img = tx_tap_image(t);
    memcpy(image, img.data(), img.size() * sizeof(float2));
  }
  return K7_NT;
}

extern "C" int uwspr_tx_baseband(uwspr_ctx *c, const uwspr_tx_signal *sig, int nsig, int channel, long long t0, int n,
                                 float *iq, int where) {
  return tx_baseband(c, sig, nullptr, nullptr, nullptr, nsig, channel, t0, n, iq, where);
}

extern "C" int uwspr_tx_baseband_moving(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, int nsig,
                                        int channel, long long t0, int n, float *iq, int where) {
  return tx_baseband(c, sig, motion, nullptr, nullptr, nsig, channel, t0, n, iq, where);
}

extern "C" int uwspr_tx_render(uwspr_ctx *c, const uwspr_tx_signal *sig, int nsig, const uwspr_tx_channel *chan, int C,
                               long long t0, long long nframes, int format, void *out, int where) {
  return tx_render(c, sig, nullptr, nullptr, nullptr, nsig, chan, nullptr, C, t0, nframes, format, out, where);
}

extern "C" int uwspr_tx_render_moving(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, int nsig,
                                      const uwspr_tx_channel *chan, int C, long long t0, long long nframes, int format,
                                      void *out, int where) {
  return tx_render(c, sig, motion, nullptr, nullptr, nsig, chan, nullptr, C, t0, nframes, format, out, where);
}

extern "C" int uwspr_tx_baseband_at(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion,
                                    const int32_t *carrier_hz, int nsig, int channel, long long t0, int n, float *iq, int where) {
  return tx_baseband(c, sig, motion, carrier_hz, nullptr, nsig, channel, t0, n, iq, where);
}

extern "C" int uwspr_tx_render_at(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion, const int32_t *carrier_hz,
                                  int nsig, const uwspr_tx_channel *chan, int C, long long t0, long long nframes, int format,
                                  void *out, int where) {
  return tx_render(c, sig, motion, carrier_hz, nullptr, nsig, chan, nullptr, C, t0, nframes, format, out, where);
}

extern "C" int uwspr_tx_baseband_medium(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion,
                                        const int32_t *carrier_hz, const uwspr_tx_fade *fade, int nsig, int channel,
                                        long long t0, int n, float *iq, int where) {
  return tx_baseband(c, sig, motion, carrier_hz, fade, nsig, channel, t0, n, iq, where);
}

extern "C" int uwspr_tx_render_medium(uwspr_ctx *c, const uwspr_tx_signal *sig, const uwspr_tx_motion *motion,
                                      const int32_t *carrier_hz, const uwspr_tx_fade *fade, int nsig, const uwspr_tx_channel *chan,
                                      const uwspr_tx_impulse *impulse, int C, long long t0, long long nframes, int format,
                                      void *out, int where) {
  return tx_render(c, sig, motion, carrier_hz, fade, nsig, chan, impulse, C, t0, nframes, format, out, where);
}

extern "C" int uwspr_tx_fade_design(const uwspr_tx_fade *f, double a[2], double *omega, double *phi) {
  if (!f) return UWSPR_ERR_ARG;
  return tx_fade_design(*f, a, omega, phi);
}

// Test door (not part of the ABI): launches of K7's medium form since the process started: out[0] float32 output,
// out[1] int16 output, out[2] baseband
extern "C" int uwspr_debug_tx_medium_counts(long long *out) {
  if (!out) return UWSPR_ERR_ARG;
  for (int i = 0; i < 3; i++) out[i] = k7_medium_launches[i].load();
  return 3;
}

extern "C" int uwspr_tx_design_at(int carrier_hz, int cutoff_hz, double *g, float *image) {
  if (!tx_carrier_ok(carrier_hz, cutoff_hz)) return UWSPR_ERR_ARG;
  const std::vector<std::complex<double>> t = tx_composite(carrier_hz, cutoff_hz);
  if ((int)t.size() != K7_NT) return UWSPR_ERR_ARG;   // (the callers' buffers hold 3179)
  if (g)
    for (size_t q = 0; q < t.size(); q++) { g[2 * q] = t[q].real(); g[2 * q + 1] = t[q].imag(); }
  if (image) {
    const std::vector<float2> img = tx_tap_image(t);
    memcpy(image, img.data(), img.size() * sizeof(float2));
  }
  return (int)t.size();
}

// Test door (not part of the ABI): launches of K7's carrier form since the process started: out[0] float32 output,
// out[1] int16 output
extern "C" int uwspr_debug_tx_carrier_counts(long long *out) {
  if (!out) return UWSPR_ERR_ARG;
  out[0] = k7_carrier_launches[0].load(); out[1] = k7_carrier_launches[1].load();
  return 2;
}
