// K0 -- 12 kS/s real audio -> 375 S/s complex baseband.
//
// In the reference this stage is not gr-uwspr code: the flowgraph (examples/WaveFilePlusNoiseDecode.grc) chains GNU
// Radio's own blocks --
//     float_to_complex                                                             grc:527
//  -> freq_xlating_fft_filter_ccc(decim 1, band_pass(1, 12000, 1490, 1510, 10, HAMMING) real taps, centre 0)     grc:303-352, 840-893
//  -> freq_xlating_fft_filter_ccc(decim 1, low_pass(1, 12000, 1510, 10, HAMMING), centre 1500 Hz)                grc:358-400, 903-956
//  -> rational_resampler_ccc(interp 1, decim 32, no taps, fbw 0 -> its own Kaiser design)                       grc:1767-1808
// Mode 0 ("grc", the default) is THAT chain: the three tap sets are designed here on the host in binary64 from GNU
// Radio 3.7's published window-method formulas (gr-filter/lib/firdes.cc, gr-fft/lib/window.cc,
// gr-filter/python/filter/rational_resampler.py, freq_xlating_fft_filter.py; rounded to binary32 where the reference
// stores them so), and because every stage is linear and the 1500-Hz mixer has period 8 | 32 the whole chain is, at
// the decimated instants, ONE complex FIR on the real input:
//
//     y[m] = sum_k g[k] x[32 m + D - k],     g = h1 * (h2[k] e^{+j k pi/4}) * (h3[k] e^{+j k pi/4}),  6831 taps,  D = 0
//
// so the kernel works at the OUTPUT rate: 213 multiply-adds per input sample instead of the chain's 2 x 2891 complex
// ones at 12 kS/s.  Mode 1 ("compact") is the single-stage filter of rounds 1-4 (mix by -1500 Hz, 1025-tap Hamming
// low-pass at 100 Hz, D = 512): same kernel, other taps.  GNU Radio is absent from the reference tree and from this
// image: **parity unpinned by construction**; the independent float64 restatement is oracle/frontend_grc.py.
//
// Mapping.  Taps are split by phase p = k mod 32 (J = ceil(NT / 32) taps per phase, padded to a multiple of 8), the
// input is staged in LDS in polyphase order (row = n mod 32).  A 1024-thread workgroup makes 512 consecutive outputs:
// wavefront w owns phases 2w and 2w + 1, a lane owns EIGHT consecutive outputs, so one staged sample read feeds 16
// fused multiply-adds (the sliding window of a phase's column lives in registers: 8 new samples per 8 taps), the
// complex taps come as wave-uniform LDS reads, and the 16 partial sums per output are added in wavefront order at the
// end.  Within a row the columns are stored [column mod 8][column div 8] so that the 64 lanes of a read hit 64
// consecutive words.  LDS: 32 x (8 L + 1) samples + 32 J taps = 149 KB for the grc mode: one workgroup, 4 wavefronts
// per SIMD.  1.2 GFLOP and 5.8 MB in per 2-minute frame (213 flop / B): FP32-FMA bound.
#include <math.h>
#include <string.h>

#include <atomic>
#include <complex>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "uwspr_internal.h"

namespace uwspr {

constexpr int K0_DEC = 32;
constexpr int K0_WG = 1024;             // 16 wavefronts x 2 tap phases
constexpr int K0_R = 8;                 // outputs per lane
constexpr int K0_OUT = 64 * K0_R;       // outputs per workgroup
constexpr int K0_COMPACT_D = 512;       // read-ahead of the compact mode (the grc mode's is 0)

__host__ __device__ constexpr int k0_L(int J) { return 64 + J / 8; }          // column groups per row segment
__host__ __device__ constexpr int k0_row(int J) { return 8 * k0_L(J) + 1; }   // floats per polyphase row (+1: the loader's lanes hit 32 banks)
static size_t k0_lds_bytes(int J) { return (size_t)K0_DEC * k0_row(J) * sizeof(float) + (size_t)K0_DEC * J * sizeof(float2); }

// 8 taps of one phase against the 15 samples they touch: acc[i] += g[u] * S[i + u], S = A[0..7] then B[0..7]
__device__ __forceinline__ void k0_block(float (&ar)[K0_R], float (&ai)[K0_R], const float (&A)[8], const float (&B)[8],
                                         const float2 *__restrict__ g) {
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const float2 t = g[u];
#pragma unroll
    for (int i = 0; i < K0_R; i++) {
      const float s = (i + u < 8) ? A[i + u] : B[i + u - 8];
      ar[i] = fmaf(t.x, s, ar[i]);
      ai[i] = fmaf(t.y, s, ai[i]);
    }
  }
}

// a sample as the filter sees it: float as it is, int16 scaled by 2^-15 (exact; GNU Radio's wavfile_source)
__device__ __forceinline__ float k0_sample(float v) { return v; }
__device__ __forceinline__ float k0_sample(int16_t v) { return (float)v * (1.0f / 32768); }

// the rotator's product, one order (include/uwspr_hip.h; k8_cancel's product form): s * r with r = (c, d)
__device__ __forceinline__ float2 k0_rotate(float2 s, float2 r) {
  return make_float2(fmaf(s.x, r.x, -(s.y * r.y)), fmaf(s.x, r.y, s.y * r.x));
}

// taps: [32][J] float2, taps[p][jj] = g[32 (J - 1 - jj) + p] (zero beyond the filter); dcols = D / 32.
// Origins: audio[b][0] is sample in0 of its record and out[b][0] is output m_first, i.e. out[b][i] = y[m_first + i]
// reads audio[b][n - in0]; samples outside [in0, in0 + nin) count as zero.  The batch call passes 0 and 0, the
// stream form the absolute audio index of its buffer and the decimated index of the ring slot it writes.  An output's
// arithmetic is the same wherever it falls in a workgroup or a launch (the tap order is fixed per output).
// MC (the multichannel stream form): audio is [nin][nch] interleaved and b is a channel, not a record.  Workgroup
// (output block, channel) reads x[n nch + b] and writes plane b of the ring (out + b * plane); the channels of one
// output block read the same input lines, so they are consecutive after xcd_swizzle and share an XCD's L2.  Only the
// loader's address and the output's plane differ: channel b's outputs are bit for bit those of its one-channel stream.
// (nch and plane are not read by the other forms, whose code is that of the one-record kernel.)
// CAR (the carrier form; MC addressing): NC carriers listen to every audio channel.  Workgroup (output block, plane
// q = c NC + k) reads channel c as the MC form does, takes its taps from image k of taps[NC][32][J], and writes plane q
// after carrier k's rotator: with f = fcm[k] = fc mod 375 != 0 the sum s of output m leaves as s * rot[(f (m mod 375))
// mod 375] in k0_rotate's one order; with f == 0 the mixer is the identity at the decimated instants and s leaves as it
// is (its bytes, not a product with (1, -0)).  The planes of one output block are consecutive after xcd_swizzle.
// The form has the other forms' arguments (their kernels stay what they were, argument layout included): nch carries
// nch | NC << 8, and the tables follow the tap images in one block -- taps[NC][32][J], rot[375] (float2), fcm[NC] (int).
template <typename T, bool MC, bool CAR = false>
__global__ __launch_bounds__(K0_WG) void k0_frontend(const T *__restrict__ audio, int nin, long long in0,
                                                     const float2 *__restrict__ taps, float2 *__restrict__ out,
                                                     int nout, long long m_first, int J, int dcols, int nch,
                                                     long long plane) {
  static_assert(MC || !CAR, "the carrier form reads interleaved channels");
  [[maybe_unused]] const int NC = CAR ? nch >> 8 : 1;
  if constexpr (CAR) nch &= 255;
  [[maybe_unused]] const float2 *rot = taps + (size_t)NC * K0_DEC * J;
  [[maybe_unused]] const int *fcm = reinterpret_cast<const int *>(rot + 375);
  extern __shared__ __align__(16) float k0_lds[];
  const int L = k0_L(J), ROW = k0_row(J);
  float *xs = k0_lds;
  float2 *tp = reinterpret_cast<float2 *>(k0_lds + K0_DEC * ROW);   // (32 ROW floats: a multiple of 8 bytes)
  const int tid = threadIdx.x;
  int b;
  unsigned blk;   // (unsigned, as blockIdx.x)
  [[maybe_unused]] int q = 0, kc = 0;   // carrier form: the plane and its carrier
  if constexpr (CAR) {
    const unsigned lb = xcd_swizzle(blockIdx.x, gridDim.x), np = (unsigned)(nch * NC);
    blk = lb / np; q = (int)(lb - blk * np);
    b = q / NC; kc = q - b * NC;
    taps += (size_t)kc * K0_DEC * J;
  } else if constexpr (MC) {
    const unsigned lb = xcd_swizzle(blockIdx.x, gridDim.x);
    blk = lb / (unsigned)nch; b = (int)(lb - blk * (unsigned)nch);
  } else {
    blk = blockIdx.x; b = blockIdx.y;
  }
  const long long m0 = m_first + (long long)blk * K0_OUT;
  const T *x = MC ? audio + b : audio + (size_t)b * nin;
  // Output m, tap k = 32 j + p reads n = 32 (m - j + dcols) - p: row (32 - p) mod 32, column m - j + dcols - (p > 0).
  // With cb = m0 - J + dcols the workgroup's rows start at column cb; row 0 is stored one column late, so that for
  // every phase the sample of (output m0 + o, tap jj = J - 1 - j) sits at position o + jj of its row.
  const long long cb = m0 - J + dcols;
  const int span = K0_DEC * (K0_OUT + J);
  for (int e = tid; e < span; e += K0_WG) {
    const int r = e & (K0_DEC - 1);
    const int pos = (e >> 5) - (r == 0 ? 1 : 0);
    if (pos < 0) continue;
    const long long n = (long long)K0_DEC * cb + e - in0;   // index into this buffer
    const float v = (n >= 0 && n < nin) ? k0_sample(x[MC ? n * nch : n]) : 0.0f;
    xs[r * ROW + (pos & 7) * L + (pos >> 3)] = v;
  }
  for (int i = tid; i < K0_DEC * J; i += K0_WG) tp[i] = taps[i];
  __syncthreads();

  const int w = tid >> 6, l = tid & 63;
  float ar[K0_R], ai[K0_R];
#pragma unroll
  for (int i = 0; i < K0_R; i++) { ar[i] = 0.0f; ai[i] = 0.0f; }
  const int nblk = J / 8;
  for (int h = 0; h < 2; h++) {
    const int p = 2 * w + h;
    const float *xr = xs + ((K0_DEC - p) & (K0_DEC - 1)) * ROW + l;
    const float2 *g = tp + p * J;
    float A[8], B[8];
#pragma unroll
    for (int v = 0; v < 8; v++) A[v] = xr[v * L];
    int t = 0;
    for (; t + 2 <= nblk; t += 2) {           // two blocks per trip: the window's halves swap roles, no copies
#pragma unroll
      for (int v = 0; v < 8; v++) B[v] = xr[v * L + t + 1];
      k0_block(ar, ai, A, B, g + 8 * t);
#pragma unroll
      for (int v = 0; v < 8; v++) A[v] = xr[v * L + t + 2];
      k0_block(ar, ai, B, A, g + 8 * t + 8);
    }
    if (t < nblk) {
#pragma unroll
      for (int v = 0; v < 8; v++) B[v] = xr[v * L + t + 1];
      k0_block(ar, ai, A, B, g + 8 * t);
    }
  }
  __syncthreads();                             // every wavefront is done with the samples: their LDS becomes the partial sums
  float2 *part = reinterpret_cast<float2 *>(xs);      // [16 wavefronts][8 i][64 lanes]
#pragma unroll
  for (int i = 0; i < K0_R; i++) part[(w * K0_R + i) * 64 + l] = make_float2(ar[i], ai[i]);
  __syncthreads();
  if (tid < K0_OUT) {
    const int i = tid >> 6;                    // thread (i, l) finishes output 8 l + i
    float re = 0.0f, im = 0.0f;
#pragma unroll
    for (int ww = 0; ww < K0_WG / 64; ww++) {
      const float2 q = part[(ww * K0_R + i) * 64 + l];
      re += q.x; im += q.y;
    }
    const int m = blk * K0_OUT + K0_R * l + i;
    if constexpr (CAR) {
      const int f = fcm[kc];
      if (m < nout) {
        float2 y = make_float2(re, im);
        if (f != 0) {
          const long long ma = m_first + m;
          const int mr = (int)(ma % 375), mm = mr < 0 ? mr + 375 : mr;
          y = k0_rotate(y, rot[(f * mm) % 375]);
        }
        out[(size_t)q * plane + m] = y;
      }
    } else {
      if (m < nout) out[MC ? (size_t)b * plane + m : (size_t)b * nout + m] = make_float2(re, im);
    }
  }
}

// ---------------------------------------------------------------- tap designs (host, binary64)
// GNU Radio 3.7 gr-fft/lib/window.cc
double gr_izero(double x) {             // Izero(): I0 by its power series, terms down to 1e-21 of the sum
  double sum = 1.0, u = 1.0;
  const double halfx = x / 2.0;
  int n = 1;
  do {
    double temp = halfx / (double)n;
    n += 1;
    temp *= temp;
    u *= temp;
    sum += u;
  } while (u >= 1e-21 * sum);
  return sum;
}
enum { WIN_HAMMING = 0, WIN_KAISER = 1 };
static std::vector<float> gr_window(int type, int ntaps, double beta) {
  std::vector<float> w(ntaps);
  if (type == WIN_HAMMING) {                   // window::hamming: `float M = ntaps - 1`
    const float M = (float)(ntaps - 1);
    for (int n = 0; n < ntaps; n++) w[n] = (float)(0.54 - 0.46 * cos((2 * M_PI * n) / M));
  } else {                                     // window::kaiser
    const double ibeta = 1.0 / gr_izero(beta), inm1 = 1.0 / (double)(ntaps - 1);
    for (int i = 0; i < ntaps; i++) {
      const double temp = 2 * i * inm1 - 1;
      w[i] = (float)(gr_izero(beta * sqrt(1.0 - temp * temp)) * ibeta);
    }
  }
  return w;
}
// gr-filter/lib/firdes.cc: compute_ntaps with window::max_attenuation (Hamming 53 dB, Kaiser beta / 0.1102 + 8.7)
static int gr_compute_ntaps(double fs, double tw, int type, double beta) {
  const double a = type == WIN_HAMMING ? 53.0 : beta / 0.1102 + 8.7;
  int ntaps = (int)(a * fs / (22.0 * tw));
  if ((ntaps & 1) == 0) ntaps++;
  return ntaps;
}
// firdes::low_pass (lo < 0) / firdes::band_pass: truncated ideal response x window, unit gain at 0 Hz / the band centre
static std::vector<float> gr_firdes(double gain, double fs, double lo, double hi, double tw, int type, double beta) {
  const int ntaps = gr_compute_ntaps(fs, tw, type, beta);
  std::vector<float> taps(ntaps), w = gr_window(type, ntaps, beta);
  const int M = (ntaps - 1) / 2;
  const bool band = lo >= 0.0;
  const double fwT0 = band ? 2 * M_PI * lo / fs : 0.0, fwT1 = 2 * M_PI * hi / fs;
  for (int n = -M; n <= M; n++) {
    if (n == 0) taps[n + M] = (float)((fwT1 - fwT0) / M_PI * w[n + M]);
    else if (band) taps[n + M] = (float)((sin(n * fwT1) - sin(n * fwT0)) / (n * M_PI) * w[n + M]);
    else taps[n + M] = (float)(sin(n * fwT1) / (n * M_PI) * w[n + M]);
  }
  double fmax = taps[0 + M];
  for (int n = 1; n <= M; n++) fmax += band ? 2 * taps[n + M] * cos(n * (fwT0 + fwT1) * 0.5) : 2 * taps[n + M];
  gain /= fmax;
  for (int i = 0; i < ntaps; i++) taps[i] = (float)(taps[i] * gain);
  return taps;
}
std::vector<float> lowpass_hamming(double fs, double cutoff, double tw) {
  return gr_firdes(1.0, fs, -1.0, cutoff, tw, WIN_HAMMING, 6.76);
}
// gr-filter/python/filter/rational_resampler.py: design_filter(interp, decim, fractional_bw = 0.4 when none is given)
static std::vector<float> gr_resampler_taps(int interp, int decim) {
  const double fractional_bw = 0.4, beta = 7.0, halfband = 0.5;
  const double rate = (double)interp / (double)decim;
  double tw, mid;
  if (rate >= 1.0) { tw = halfband - fractional_bw; mid = halfband - tw / 2.0; }
  else { tw = rate * (halfband - fractional_bw); mid = rate * halfband - tw / 2.0; }
  return gr_firdes(interp, interp, -1.0, mid, tw, WIN_KAISER, beta);
}

typedef std::complex<double> cplx;
static std::vector<cplx> conv(const std::vector<cplx> &a, const std::vector<cplx> &b) {
  std::vector<cplx> c(a.size() + b.size() - 1, cplx(0, 0));
  for (size_t i = 0; i < a.size(); i++)
    for (size_t j = 0; j < b.size(); j++) c[i + j] += a[i] * b[j];
  return c;
}
// e^{+j k pi/4}: exact octant values (the mixer's period is 8 samples)
static cplx octant(long k) {
  static const double r = sqrt(0.5);
  static const double cs[8] = {1, r, 0, -r, -1, -r, 0, r}, sn[8] = {0, r, 1, r, 0, -r, -1, -r};
  const int q = (int)(((k % 8) + 8) % 8);
  return cplx(cs[q], sn[q]);
}

// e^{+j 2 pi fc k / 12000} for an integer centre: fc k is reduced in integers first, and an angle that is a multiple of
// pi/4 (every k at 1500 Hz) takes the exact octant values
static cplx mixer(int fc, long k) {
  const long r = ((((long)fc * (k % 12000)) % 12000) + 12000) % 12000;
  if (r % 1500 == 0) return octant(r / 1500);
  const double a = 2.0 * M_PI * (double)r / 12000.0;
  return cplx(cos(a), sin(a));
}

bool frontend_carrier_ok(int mode, int fc, int hb) {
  if (mode == UWSPR_FRONTEND_COMPACT) hb = 0;   // (the compact mode has no such variable)
  else if (hb < 1 || hb > 150) return false;
  return fc >= hb + 20 && fc <= 6000 - hb - 20;
}

// the rotator's table: rot[i] = e^{-j 2 pi i / 375} as binary32 pairs (cos, -sin), from the reduced index in binary64
void frontend_rotator(float *out750) {
  for (int i = 0; i < 375; i++) {
    const double a = 2.0 * M_PI * (double)i / 375.0;
    out750[2 * i] = (float)cos(a);
    out750[2 * i + 1] = (float)(-sin(a));
  }
}

// stage 0: the composite complex taps g (pairs) and the read-ahead D; stages 1..3 (grc mode): the three real designs.
// fc, hb: the flowgraph's Center_Frequency and Half_Bandwidth (integer Hz; the compact mode has no hb)
int frontend_design_at(int mode, int fc, int hb, int stage, std::vector<double> &outv, int *delay) {
  outv.clear();
  if (delay) *delay = 0;
  if (mode != UWSPR_FRONTEND_COMPACT && mode != UWSPR_FRONTEND_GRC) return UWSPR_ERR_ARG;
  if (!frontend_carrier_ok(mode, fc, hb)) return UWSPR_ERR_ARG;
  if (mode == UWSPR_FRONTEND_COMPACT) {
    if (stage != 0) return UWSPR_ERR_ARG;
    // h[k] e^{-j 2 pi fc (D - k) / 12000}: Hamming-windowed sinc, cutoff 100 Hz, 1025 taps, unit DC gain, D = 512
    const int NT = 1025, D = K0_COMPACT_D;
    std::vector<double> h(NT);
    const double fcut = 100.0 / 12000.0;
    double sum = 0.0;
    for (int k = 0; k < NT; k++) {
      const double t = (double)(k - D);
      const double sinc = t == 0.0 ? 2.0 * fcut : sin(2.0 * M_PI * fcut * t) / (M_PI * t);
      h[k] = sinc * (0.54 - 0.46 * cos(2.0 * M_PI * (double)k / (double)(NT - 1)));
      sum += h[k];
    }
    for (int k = 0; k < NT; k++) {
      const cplx g = (h[k] / sum) * std::conj(mixer(fc, D - k));
      outv.push_back(g.real()); outv.push_back(g.imag());
    }
    if (delay) *delay = D;
    return UWSPR_OK;
  }
  const std::vector<float> h1 = gr_firdes(1.0, 12000.0, (double)fc - (double)hb, (double)fc + (double)hb, 10.0, WIN_HAMMING, 6.76);
  const std::vector<float> h2 = gr_firdes(1.0, 12000.0, -1.0, (double)fc + (double)hb, 10.0, WIN_HAMMING, 6.76);
  const std::vector<float> h3 = gr_resampler_taps(1, 32);
  if (stage >= 1 && stage <= 3) {
    const std::vector<float> &h = stage == 1 ? h1 : stage == 2 ? h2 : h3;
    for (float v : h) outv.push_back((double)v);
    return UWSPR_OK;
  }
  if (stage != 0) return UWSPR_ERR_ARG;
  std::vector<cplx> a(h1.size()), bq(h2.size()), cq(h3.size());
  for (size_t k = 0; k < h1.size(); k++) a[k] = cplx(h1[k], 0.0);
  // freq_xlating_fft_filter_ccc hands fft_filter_ccc gr_complex taps: the rotated taps are binary32 pairs
  for (size_t k = 0; k < h2.size(); k++) {
    const cplx z = (double)h2[k] * mixer(fc, (long)k);
    bq[k] = cplx((double)(float)z.real(), (double)(float)z.imag());
  }
  // the resampler filters BEHIND the mixer: its taps meet the input rotated, in exact arithmetic
  for (size_t k = 0; k < h3.size(); k++) cq[k] = (double)h3[k] * mixer(fc, (long)k);
  const std::vector<cplx> g = conv(conv(a, bq), cq);
  for (const cplx &z : g) { outv.push_back(z.real()); outv.push_back(z.imag()); }
  return UWSPR_OK;
}

int frontend_design(int mode, int stage, std::vector<double> &outv, int *delay) {
  return frontend_design_at(mode, UWSPR_CARRIER_DEFAULT, UWSPR_FRONTEND_HBW_DEFAULT, stage, outv, delay);
}

// the kernel's tap image: [32][J] float2, jj ascending = tap index descending
int frontend_tap_image(int mode, std::vector<float> &img, int *J_out, int *dcols_out) {
  return frontend_tap_image_at(mode, UWSPR_CARRIER_DEFAULT, UWSPR_FRONTEND_HBW_DEFAULT, img, J_out, dcols_out);
}

// (the images of the last designs are kept: a pipe with 64 carriers, or one opened again, designs each of them once)
namespace {
struct tap_image { std::vector<float> img; int J, dcols, rc; };
std::mutex k0_img_mutex;
std::map<std::tuple<int, int, int>, tap_image> k0_images;
}  // namespace

static int tap_image_build(int mode, int fc, int hb, std::vector<float> &img, int *J_out, int *dcols_out);

int frontend_tap_image_at(int mode, int fc, int hb, std::vector<float> &img, int *J_out, int *dcols_out) {
  if (mode == UWSPR_FRONTEND_COMPACT) hb = 0;   // (not read by that design)
  const auto key = std::make_tuple(mode, fc, hb);
  {
    std::lock_guard<std::mutex> lk(k0_img_mutex);
    const auto it = k0_images.find(key);
    if (it != k0_images.end()) { img = it->second.img; *J_out = it->second.J; *dcols_out = it->second.dcols; return it->second.rc; }
  }
  const int rc = tap_image_build(mode, fc, hb, img, J_out, dcols_out);
  if (rc == UWSPR_OK) {
    std::lock_guard<std::mutex> lk(k0_img_mutex);
    if (k0_images.size() >= 128) k0_images.clear();
    k0_images[key] = tap_image{img, *J_out, *dcols_out, rc};
  }
  return rc;
}

static int tap_image_build(int mode, int fc, int hb, std::vector<float> &img, int *J_out, int *dcols_out) {
  std::vector<double> g;
  int D = 0;
  const int rc = frontend_design_at(mode, fc, hb, 0, g, &D);
  if (rc) return rc;
  const int NT = (int)g.size() / 2;
  int J = (NT + K0_DEC - 1) / K0_DEC;
  J = (J + 7) / 8 * 8;
  img.assign((size_t)2 * K0_DEC * J, 0.0f);
  for (int p = 0; p < K0_DEC; p++)
    for (int jj = 0; jj < J; jj++) {
      const int k = K0_DEC * (J - 1 - jj) + p;
      if (k < NT) { img[2 * ((size_t)p * J + jj)] = (float)g[2 * k]; img[2 * ((size_t)p * J + jj) + 1] = (float)g[2 * k + 1]; }
    }
  *J_out = J; *dcols_out = D / K0_DEC;
  return (D % K0_DEC) ? UWSPR_ERR_ARG : UWSPR_OK;
}

int frontend_read_ahead(int mode) {
  return mode == UWSPR_FRONTEND_COMPACT ? K0_COMPACT_D : mode == UWSPR_FRONTEND_GRC ? 0 : -1;
}

int frontend_prepare() {
  // up to 160 KB of dynamic LDS (149 KB in the grc mode); int16 samples are widened before they reach LDS
  const void *k[] = {reinterpret_cast<const void *>(k0_frontend<float, false>), reinterpret_cast<const void *>(k0_frontend<int16_t, false>),
                     reinterpret_cast<const void *>(k0_frontend<float, true>), reinterpret_cast<const void *>(k0_frontend<int16_t, true>),
                     reinterpret_cast<const void *>(k0_frontend<float, true, true>),
                     reinterpret_cast<const void *>(k0_frontend<int16_t, true, true>)};
  for (const void *f : k)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return -1;
  return 0;
}

void launch_frontend(uwspr_ctx *c, const float *audio, int B, int nin, float2 *out, int nout) {
  prof_scope ps(c, UWSPR_K_SPECTROGRAM, B);
  dim3 grid((nout + K0_OUT - 1) / K0_OUT, B);
  hipLaunchKernelGGL((k0_frontend<float, false>), grid, dim3(K0_WG), k0_lds_bytes(c->fe_J), c->stream, audio, nin, 0LL,
                     (const float2 *)c->d_fe_taps, out, nout, 0LL, c->fe_J, c->fe_dcols, 1, 0LL);
}

// the stream form (stream_ring::push_audio): outputs m_first .. m_first + nout - 1 from the buffer that holds audio
// [in0, in0 + nin) -- one record, or with nch > 1 frames of nch interleaved channels, channel c's outputs at
// out + 2 * c * plane floats
void launch_frontend_stream(hipStream_t s, const void *audio, bool s16, int nin, long long in0, const float *taps,
                            int J, int dcols, float *out, int nout, long long m_first, int nch, long long plane) {
  const int nblk = (nout + K0_OUT - 1) / K0_OUT;
  if (nch > 1) {
    const dim3 grid(nblk * nch, 1);
    if (s16)
      hipLaunchKernelGGL((k0_frontend<int16_t, true>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const int16_t *)audio, nin, in0,
                         (const float2 *)taps, (float2 *)out, nout, m_first, J, dcols, nch, plane);
    else
      hipLaunchKernelGGL((k0_frontend<float, true>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const float *)audio, nin, in0,
                         (const float2 *)taps, (float2 *)out, nout, m_first, J, dcols, nch, plane);
    return;
  }
  dim3 grid(nblk, 1);
  if (s16)
    hipLaunchKernelGGL((k0_frontend<int16_t, false>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const int16_t *)audio, nin, in0,
                       (const float2 *)taps, (float2 *)out, nout, m_first, J, dcols, 1, 0LL);
  else
    hipLaunchKernelGGL((k0_frontend<float, false>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const float *)audio, nin, in0,
                       (const float2 *)taps, (float2 *)out, nout, m_first, J, dcols, 1, 0LL);
}

// the carrier form's device block for `carriers` (Hz) at half-bandwidth hb: taps[NC][32][J] float2, the rotator table
// (375 float2), carrier k mod 375 (NC ints)
int frontend_carrier_tables(int mode, const std::vector<int> &carriers, int hb, std::vector<float> &blk, int *J_out, int *dcols_out) {
  blk.clear();
  std::vector<float> img;
  for (int fc : carriers) {
    const int rc = frontend_tap_image_at(mode, fc, hb, img, J_out, dcols_out);
    if (rc) return rc;
    blk.insert(blk.end(), img.begin(), img.end());
  }
  const size_t at = blk.size();
  blk.resize(at + 750 + carriers.size());
  frontend_rotator(&blk[at]);
  for (size_t k = 0; k < carriers.size(); k++) { const int f = carriers[k] % 375; memcpy(&blk[at + 750 + k], &f, sizeof(int)); }
  return carriers.empty() ? UWSPR_ERR_ARG : UWSPR_OK;
}

// the carrier form: planes q = c NC + k (audio channel c, carrier k) of outputs m_first .. m_first + nout - 1, plane q at
// out + 2 * q * plane floats; tables: frontend_carrier_tables' block on the device
static std::atomic<long long> k0_carrier_launches[2];
long long frontend_carrier_launch_count(int s16) { return k0_carrier_launches[s16 ? 1 : 0].load(); }

void launch_frontend_carrier(hipStream_t s, const void *audio, bool s16, int nin, long long in0, const float *tables, int J,
                             int dcols, float *out, int nout, long long m_first, int nch, int NC, long long plane) {
  const int nblk = (nout + K0_OUT - 1) / K0_OUT;
  const dim3 grid(nblk * nch * NC, 1);
  k0_carrier_launches[s16 ? 1 : 0]++;
  if (s16)
    hipLaunchKernelGGL((k0_frontend<int16_t, true, true>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const int16_t *)audio, nin, in0,
                       (const float2 *)tables, (float2 *)out, nout, m_first, J, dcols, nch | NC << 8, plane);
  else
    hipLaunchKernelGGL((k0_frontend<float, true, true>), grid, dim3(K0_WG), k0_lds_bytes(J), s, (const float *)audio, nin, in0,
                       (const float2 *)tables, (float2 *)out, nout, m_first, J, dcols, nch | NC << 8, plane);
}

// int16 samples into a float stream buffer: the value K0's int16 loader computes (k0_sample)
__global__ void k_widen_s16(const int16_t *__restrict__ in, float *__restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = k0_sample(in[i]);
}

void launch_widen_s16(hipStream_t s, const int16_t *in, float *out, size_t n) {
  if (n == 0) return;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_widen_s16, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, in, out, n);
}

}  // namespace uwspr
