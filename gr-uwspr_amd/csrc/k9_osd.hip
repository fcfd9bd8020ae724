// k9_osd.hip -- K9: ordered-statistics decoding of the (162, 50) code (uwspr_osd_batch, the pipe's option "osd").
// The definition is the comment at uwspr_osd_batch in include/uwspr_hip.h; the reference has no counterpart.  All
// integers: results are the same bytes as the numpy restatement in tests/test_gpu_osd.py.
//
// One wavefront per item.  Lane j < 50 owns row j of [G | I]: 162 + 50 bits in eight 32-bit registers, code bits at
// their de-interleaved positions.  The rank of every position's reliability comes from counting in LDS; one
// elimination step is a ballot over the not-yet-pivoted lanes whose row has the column's bit, a broadcast of the
// pivot lane's row and an XOR in every other lane that has the bit.  The reduced rows go to LDS in pivot order; flip
// sets are scored with per-byte weight tables (21 bytes cover the 162 positions), the pairs (a, b) with a uniform and
// one b per lane; a packed (distance, flips, a, b) key makes the minimum the definition's winner.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K9_N = 162, K9_K = 50, K9_W = 6, K9_ROW = 8, K9_BYTES = 21;
// the context's table: G as 50 rows of 6 words (bit i of a row = word i / 32, bit i % 32), then the de-interleave
// sources (destination p takes interleaved byte src[p]) as 162 words
constexpr int K9_TAB_WORDS = K9_K * K9_W + K9_N;

struct osd_state {
  uint32_t *d_tab = nullptr;
  symbols_stage stage;                                          // host symbols staged
  uwspr_osd_result *d_res = nullptr; size_t cap_res = 0;
  unsigned long long *d_off = nullptr; size_t cap_off = 0;      // byte offsets of scattered items
  launch_timer timer;                                           // uwspr_debug_osd_time
};

__device__ __forceinline__ uint32_t k9_pick(const uint32_t (&w)[K9_ROW], int wi) {   // wi is wave-uniform
  uint32_t v = w[0];
#pragma unroll
  for (int q = 1; q < K9_W; q++) v = wi == q ? w[q] : v;
  return v;
}

__device__ __forceinline__ uint32_t k9_min_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = o < v ? o : v; }
  return v;
}

// base + off[item] (off null: 162 * item): the item's 162 interleaved soft symbols
__global__ void __launch_bounds__(64) k9_osd(const uint8_t *__restrict__ base, const unsigned long long *__restrict__ off,
                                             const uint32_t *__restrict__ tab, int order, uwspr_osd_result *__restrict__ res) {
  __shared__ uint8_t rel[K9_BYTES * 8];           // reliabilities by de-interleaved position (0 past 162)
  __shared__ uint8_t perm[K9_N];                  // positions in elimination order
  __shared__ uint32_t hbits[K9_W];                // hard bits
  __shared__ uint32_t rows[K9_K][K9_ROW];         // reduced rows in pivot order
  __shared__ uint8_t pivcol[K9_K];
  __shared__ uint16_t wt[K9_BYTES][256];          // wt[B][v] = sum of rel[8 B + t] over the bits t of v
  const int lane = threadIdx.x, item = blockIdx.x;
  const uint8_t *sym = base + (off ? off[item] : (unsigned long long)item * K9_N);

  if (lane < K9_W) hbits[lane] = 0u;
  if (lane < K9_BYTES * 8 - K9_N) rel[K9_N + lane] = 0;
  __syncthreads();
  for (int p = lane; p < K9_N; p += 64) {
    const int s = sym[tab[K9_K * K9_W + p]];
    const int r = 2 * s - 255;
    rel[p] = (uint8_t)(r < 0 ? -r : r);
    if (s >= 128) atomicOr(&hbits[p >> 5], 1u << (p & 31));
  }
  __syncthreads();
  // rank = positions that come before p: more reliable, or as reliable with a smaller index
  for (int p = lane; p < K9_N; p += 64) {
    const int r = rel[p];
    int rank = 0;
    for (int j = 0; j < K9_N; j++) { const int rj = rel[j]; rank += (rj > r || (rj == r && j < p)) ? 1 : 0; }
    perm[rank] = (uint8_t)p;
  }
  // weight tables
  for (int e = lane; e < K9_BYTES * 256; e += 64) {
    const int B = e >> 8, v = e & 255;
    int s = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) s += ((v >> t) & 1) ? (int)rel[8 * B + t] : 0;
    wt[B][v] = (uint16_t)s;
  }
  __syncthreads();

  // Gauss-Jordan over the columns in reliability order
  uint32_t w[K9_ROW];
#pragma unroll
  for (int q = 0; q < K9_W; q++) w[q] = lane < K9_K ? tab[lane * K9_W + q] : 0u;
  w[6] = lane < 32 ? 1u << lane : 0u;
  w[7] = (lane >= 32 && lane < K9_K) ? 1u << (lane - 32) : 0u;
  int mypiv = -1, npiv = 0;
  for (int c = 0; c < K9_N && npiv < K9_K; c++) {
    const int col = perm[c];
    const bool bit = (k9_pick(w, col >> 5) >> (col & 31)) & 1u;
    const unsigned long long cand = __ballot(bit && mypiv < 0 && lane < K9_K);
    if (cand == 0ull) continue;                   // in the span of the columns taken so far
    const int p = __ffsll((long long)cand) - 1;   // the first not-yet-pivoted row with a 1
    uint32_t pr[K9_ROW];
#pragma unroll
    for (int q = 0; q < K9_ROW; q++) pr[q] = (uint32_t)__shfl((int)w[q], p);
    if (lane == p) { mypiv = npiv; pivcol[npiv] = (uint8_t)col; }
    else if (bit) {
#pragma unroll
      for (int q = 0; q < K9_ROW; q++) w[q] ^= pr[q];
    }
    npiv++;
  }
  if (mypiv >= 0) {
#pragma unroll
    for (int q = 0; q < K9_ROW; q++) rows[mypiv][q] = w[q];
  }
  __syncthreads();

  // order-0 codeword: the reduced rows combined by the hard bits at the pivot positions; z = c0 ^ h
  uint32_t z[K9_ROW];
#pragma unroll
  for (int q = 0; q < K9_ROW; q++) z[q] = q < K9_W ? hbits[q] : 0u;
  for (int k = 0; k < K9_K; k++) {
    const int col = pivcol[k];
    if ((hbits[col >> 5] >> (col & 31)) & 1u) {
#pragma unroll
      for (int q = 0; q < K9_ROW; q++) z[q] ^= rows[k][q];
    }
  }
  auto dist = [&](const uint32_t (&x)[K9_W]) {
    int d = 0;
#pragma unroll
    for (int B = 0; B < K9_BYTES; B++) d += (int)wt[B][(x[B >> 2] >> (8 * (B & 3))) & 255u];
    return d;
  };
  // key = distance << 14 | flips << 12 | a << 6 | b: its minimum is the least distance, then fewer flips, then the
  // lexicographically smaller flip set.  d2 = this lane's second smallest distance.
  constexpr uint32_t NONE = 0xffffffffu;
  uint32_t best = NONE, d2 = NONE;
  auto offer = [&](uint32_t key) {
    if (key < best) { d2 = best == NONE ? NONE : best >> 14; best = key; }
    else if ((key >> 14) < d2) d2 = key >> 14;
  };
  uint32_t x[K9_W];
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < K9_W; q++) x[q] = z[q];
    offer((uint32_t)dist(x) << 14);
  }
  if (order >= 1 && lane < K9_K) {
#pragma unroll
    for (int q = 0; q < K9_W; q++) x[q] = z[q] ^ rows[lane][q];
    offer(((uint32_t)dist(x) << 14) | (1u << 12) | ((uint32_t)lane << 6));
  }
  if (order >= 2) {
    for (int a = 0; a < K9_K - 1; a++) {
      const int b = a + 1 + lane;
      if (b < K9_K) {
#pragma unroll
        for (int q = 0; q < K9_W; q++) x[q] = z[q] ^ rows[a][q] ^ rows[b][q];
        offer(((uint32_t)dist(x) << 14) | (2u << 12) | ((uint32_t)a << 6) | (uint32_t)b);
      }
    }
  }
  // the winner, and the least distance among everything else: the losing lanes' best and every lane's second
  const uint32_t win = k9_min_u32(best);
  const uint32_t mine = best == NONE ? NONE : best >> 14;
  const uint32_t other = k9_min_u32(best == win ? d2 : (mine < d2 ? mine : d2));
  if (lane == 0) {
    const int nflip = (int)((win >> 12) & 3u), a = (int)((win >> 6) & 63u), b = (int)(win & 63u);
    uint32_t e[K9_ROW];
#pragma unroll
    for (int q = 0; q < K9_ROW; q++) {
      e[q] = z[q];
      if (nflip >= 1) e[q] ^= rows[a][q];
      if (nflip >= 2) e[q] ^= rows[b][q];
    }
    int nhard = 0;
#pragma unroll
    for (int q = 0; q < K9_W; q++) nhard += __popc(e[q]);
    // message bit j (bit j of the identity half) -> byte j / 8, most significant bit first, as uwspr_fano_decode packs
    const unsigned long long m = ((unsigned long long)e[7] << 32) | (unsigned long long)e[6];
    uwspr_osd_result &r = res[item];
    r.dmin = (int32_t)(win >> 14);
    r.dnext = other == NONE ? INT32_MAX : (int32_t)other;
    r.nhard = nhard;
    r.nflip = (uint8_t)nflip;
#pragma unroll
    for (int n = 0; n < 7; n++) r.message[n] = (int8_t)(__brev((uint32_t)((m >> (8 * n)) & 0xffull)) >> 24);
  }
}

// ---------------------------------------------------------------- host side
void osd_release(uwspr_ctx *c) {
  if (!c || !c->osd) return;
  osd_state *t = c->osd;
  void *bufs[] = {t->d_tab, t->stage.d_sym, t->d_res, t->d_off};
  for (void *b : bufs) if (b) (void)hipFree(b);
  t->timer.release();
  delete t;
  c->osd = nullptr;
}

// G (row j = uwspr_fano_encode of the 81-bit input with only bit j set) and the de-interleave table, once per context
static int osd_begin(uwspr_ctx *c) {
  if (const int rc = ctx_device_ready(c)) return rc;
  if (!c->osd) c->osd = new osd_state();
  osd_state *t = c->osd;
  if (!t->d_tab) {
    std::vector<uint32_t> tab(K9_TAB_WORDS, 0u);
    for (int j = 0; j < K9_K; j++) {
      uint8_t data[11], symbols[176];
      memset(data, 0, sizeof(data));
      data[j >> 3] = (uint8_t)(0x80u >> (j & 7));
      uwspr_fano_encode(symbols, data, 11);
      for (int i = 0; i < K9_N; i++)
        if (symbols[i]) tab[j * K9_W + (i >> 5)] |= 1u << (i & 31);
    }
    uint8_t idx[K9_N];
    for (int i = 0; i < K9_N; i++) idx[i] = (uint8_t)i;
    uwspr_deinterleave(idx);   // idx[p] = the interleaved position destination p takes
    for (int p = 0; p < K9_N; p++) tab[K9_K * K9_W + p] = idx[p];
    CTXCHK(c, hipMalloc((void **)&t->d_tab, tab.size() * sizeof(uint32_t)));
    CTXCHK(c, hipMemcpy(t->d_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return UWSPR_OK;
}

// n items on the context's stream: item i reads base + off[i] (host array; null: 162 i), results to res (device memory;
// null: the context's own buffer, returned through *res_out)
int osd_run(uwspr_ctx *c, const uint8_t *base, const unsigned long long *off, int n, int order, uwspr_osd_result *res,
            uwspr_osd_result **res_out) {
  int rc = osd_begin(c);
  if (rc) return rc;
  osd_state *t = c->osd;
  if (!res) {
    if ((rc = ctx_grow(c, &t->d_res, &t->cap_res, (size_t)n))) return rc;
    res = t->d_res;
  }
  if (res_out) *res_out = res;
  if (off && (rc = scattered_offsets(c, &t->d_off, &t->cap_off, off, n))) return rc;
  if ((rc = t->timer.begin(c))) return rc;
  hipLaunchKernelGGL(k9_osd, dim3((unsigned)n), dim3(64), 0, c->stream, base, off ? t->d_off : (const unsigned long long *)nullptr,
                     t->d_tab, order, res);
  CTXCHK(c, hipGetLastError());
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_osd_batch(uwspr_ctx *c, const uint8_t *symbols, int n, int where, int order, uwspr_osd_result *res) {
  if (!c) return UWSPR_ERR_ARG;
  if (order < 0 || order > 2) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_osd_batch: order %d (0..2)", order);
  return symbols_batch(c, "uwspr_osd_batch", symbols, n, where, res, nullptr,
                       [&](symbols_stage **st) { const int rc = osd_begin(c); if (!rc) *st = &c->osd->stage; return rc; },
                       [&](const uint8_t *d_sym, uwspr_osd_result *d_res, uwspr_osd_result **d_out) { return osd_run(c, d_sym, nullptr, n, order, d_res, d_out); });
}

// Measurement hook of tools/osd_probe.py (not part of the ABI, like uwspr_debug_subtract_times): enable = 1 / 0 switches
// HIP events around the K9 launch of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
// timed launch and returns its time.
extern "C" int uwspr_debug_osd_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->osd) c->osd = new osd_state();   // (no device asked: the hook only keeps the switch)
  return c->osd->timer.read(c, enable, ms);
}
