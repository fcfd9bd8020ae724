// k13_deep.hip -- K13: the soft symbols of a candidate scored against every codeword of a list of expected messages
// (uwspr_deep_set_list / uwspr_deep_batch, the pipe's uwspr_pipe_set_list).  The definition is the comment at
// uwspr_deep_batch in include/uwspr_hip.h; the reference has no counterpart.  All integers: results are the same bytes as
// the numpy restatement in tests/deep_exact.py.
//
// The score is one int8 x int8 -> int32 product, messages x 192 x items (K = 162 padded with zeros on both operands), on
// v_mfma_i32_16x16x64_i8: three k-steps per 16 x 16 tile.  A = the table (+-1, a message per row), B = the vectors
// (s - 128, an item per column), so that the accumulator has the item on the lane (col = lane & 15) and four messages in
// its registers (row = 4 (lane >> 4) + reg): every lane keeps a running (best, sbest, snext) of ONE item and the loop over
// the message tiles needs no lane movement.  Both operands have k = 64 t + 16 (lane >> 4) + j in byte j of the lane's
// 16-byte fragment of k-step t; the table is stored in exactly that order -- tile T, k-step t, lane l at byte
// ((3 T + t) 64 + l) 16 -- so a wavefront's fragment load is 1 KiB contiguous.
// Grid: x = message chunks, y = tiles of 16 items.  A workgroup is four wavefronts that walk the 16-message tiles of its
// chunk; its (best, sbest, snext) per item goes to a partial array, and a second launch merges each item's partials.
// Every merge uses the total order (score descending, index ascending), so the bytes depend neither on the split nor on
// who arrives first.  No floating point anywhere.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K13_N = 162, K13_KPAD = 192, K13_KSTEPS = 3, K13_TILE = 16, K13_WAVES = 4;
constexpr int K13_TILE_BYTES = K13_TILE * K13_KPAD;   // 3072: one 16-message tile of the table
constexpr int K13_MAX_CHUNKS = 1024;

typedef int k13_v4i __attribute__((ext_vector_type(4)));

// a running winner and runner-up score: (s, m) is better than (s', m') when s > s', or s == s' and m < m'
struct k13_top {
  int32_t best, sbest, snext;
};
__device__ __forceinline__ k13_top k13_empty() { return k13_top{INT32_MAX, INT32_MIN, INT32_MIN}; }
__device__ __forceinline__ void k13_offer(k13_top &t, int32_t s, int32_t m) {
  if (s > t.sbest || (s == t.sbest && m < t.best)) { t.snext = t.sbest; t.sbest = s; t.best = m; }
  else if (s > t.snext) t.snext = s;
}
// two disjoint sets of messages: the winner is the better winner, the runner-up the best of everything else
__device__ __forceinline__ k13_top k13_merge(const k13_top &a, const k13_top &b) {
  const bool a_wins = a.sbest > b.sbest || (a.sbest == b.sbest && a.best < b.best);
  const k13_top &w = a_wins ? a : b, &l = a_wins ? b : a;
  return k13_top{w.best, w.sbest, w.snext > l.sbest ? w.snext : l.sbest};
}
__device__ __forceinline__ k13_top k13_shfl_xor(const k13_top &t, int d) {
  return k13_top{__shfl_xor(t.best, d), __shfl_xor(t.sbest, d), __shfl_xor(t.snext, d)};
}

// base + off[item] (off null: 162 * item): the item's 162 interleaved soft symbols.  tab: ceil(M / 16) tiles in the
// operand layout above (rows past M are zeros and never offered).  part [n][gridDim.x].
__global__ void __launch_bounds__(64 * K13_WAVES) k13_score(const uint8_t *__restrict__ base, const unsigned long long *__restrict__ off,
                                                            int n, const int8_t *__restrict__ tab, int M, int tiles_per_chunk,
                                                            k13_top *__restrict__ part) {
  __shared__ k13_top red[K13_WAVES][K13_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int item = blockIdx.y * K13_TILE + col;
  const int ntiles = (M + K13_TILE - 1) / K13_TILE;
  const int tile0 = blockIdx.x * tiles_per_chunk;
  const int tile1 = tile0 + tiles_per_chunk < ntiles ? tile0 + tiles_per_chunk : ntiles;

  // B: this lane's 3 x 16 bytes of its item, s - 128 (= s ^ 0x80 as int8), zeros from k = 162 on and for items past n
  k13_v4i b[K13_KSTEPS];
  {
    const uint8_t *sym = item < n ? base + (off ? off[item] : (unsigned long long)item * K13_N) : nullptr;
#pragma unroll
    for (int t = 0; t < K13_KSTEPS; t++) {
      const int k0 = 64 * t + 16 * grp;
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int k = k0 + 4 * q + j;
          const uint32_t byte = (sym && k < K13_N) ? (uint32_t)(sym[k] ^ 0x80u) : 0u;
          v |= byte << (8 * j);
        }
        w[q] = v;
      }
      b[t] = k13_v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }
  }

  k13_top top = k13_empty();
  for (int T = tile0 + wave; T < tile1; T += K13_WAVES) {
    const k13_v4i *a = (const k13_v4i *)(tab + (size_t)T * K13_TILE_BYTES) + lane;
    k13_v4i acc = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < K13_KSTEPS; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[64 * t], b[t], acc, 0, 0, 0);
    const int m0 = T * K13_TILE + 4 * grp;   // acc[r] = S[message m0 + r][item]
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (m0 + r < M) k13_offer(top, acc[r], m0 + r);
  }
  // the four lane groups of a wavefront hold disjoint messages of the same item, then the four wavefronts
  top = k13_merge(top, k13_shfl_xor(top, 16));
  top = k13_merge(top, k13_shfl_xor(top, 32));
  if (grp == 0) red[wave][col] = top;
  __syncthreads();
  if (wave == 0 && grp == 0 && item < n) {
#pragma unroll
    for (int w = 1; w < K13_WAVES; w++) top = k13_merge(top, red[w][col]);
    part[(size_t)item * gridDim.x + blockIdx.x] = top;
  }
}

// one wavefront per item: its nchunks partials (disjoint message ranges) -> the result
__global__ void __launch_bounds__(64) k13_reduce(const k13_top *__restrict__ part, int nchunks, uwspr_deep_result *__restrict__ res) {
  const int lane = threadIdx.x, item = blockIdx.x;
  k13_top top = k13_empty();
  for (int c = lane; c < nchunks; c += 64) top = k13_merge(top, part[(size_t)item * nchunks + c]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) top = k13_merge(top, k13_shfl_xor(top, d));
  if (lane == 0) {
    uwspr_deep_result r;
    r.best = top.best; r.sbest = top.sbest; r.snext = top.snext; r.reserved = 0;
    res[item] = r;
  }
}

// ---------------------------------------------------------------- host side
struct deep_state {
  int8_t *d_tab = nullptr; int M = 0;                           // uwspr_deep_set_list's table
  symbols_stage stage;                                          // host symbols staged
  uwspr_deep_result *d_res = nullptr; size_t cap_res = 0;
  unsigned long long *d_off = nullptr; size_t cap_off = 0;      // byte offsets of scattered items
  k13_top *d_part = nullptr; size_t cap_part = 0;
  launch_timer timer;                                           // uwspr_debug_deep_time
};

void deep_release(uwspr_ctx *c) {
  if (!c || !c->deep) return;
  deep_state *t = c->deep;
  void *bufs[] = {t->d_tab, t->stage.d_sym, t->d_res, t->d_off, t->d_part};
  for (void *b : bufs) if (b) (void)hipFree(b);
  t->timer.release();
  delete t;
  c->deep = nullptr;
}

// the list's rules (include/uwspr_hip.h): null on success, else what is wrong (into msg)
const char *deep_check_list(const int8_t *messages7, int M, char *msg, size_t cap) {
  if (!messages7 || M < 1 || M > UWSPR_DEEP_MAX) { snprintf(msg, cap, "messages %p, M %d (1..%d)", (const void *)messages7, M, UWSPR_DEEP_MAX); return msg; }
  std::vector<uint64_t> key((size_t)M);
  for (int m = 0; m < M; m++) {
    const uint8_t *b = (const uint8_t *)messages7 + 7 * (size_t)m;
    if (b[6] & 0x3f) { snprintf(msg, cap, "message %d: the low 6 bits of byte 6 are not zero (not 50 bits)", m); return msg; }
    uint64_t k = 0;
    for (int i = 0; i < 7; i++) k = (k << 8) | b[i];
    key[m] = k;
  }
  std::sort(key.begin(), key.end());
  for (int m = 1; m < M; m++)
    if (key[m] == key[m - 1]) { snprintf(msg, cap, "a message appears twice in the list (bytes %014llx)", (unsigned long long)key[m]); return msg; }
  return nullptr;
}

// the table in the kernel's operand layout: ceil(M / 16) tiles of 3072 bytes, +-1 at k < 162 of the rows m < M, else 0
int deep_build_table(const int8_t *messages7, int M, std::vector<int8_t> &tab) {
  const int ntiles = (M + K13_TILE - 1) / K13_TILE;
  tab.assign((size_t)ntiles * K13_TILE_BYTES, 0);
  for (int m = 0; m < M; m++) {
    uint8_t sym[K13_N];
    if (uwspr_wspr_symbols(messages7 + 7 * (size_t)m, sym)) return UWSPR_ERR_ARG;
    const int T = m / K13_TILE, row = m % K13_TILE;
    for (int k = 0; k < K13_N; k++) {
      const int t = k / 64, grp = (k % 64) / 16, j = k % 16, lane = 16 * grp + row;
      tab[(size_t)T * K13_TILE_BYTES + ((size_t)(t * 64 + lane)) * 16 + j] = (sym[k] >> 1) ? 1 : -1;
    }
  }
  return UWSPR_OK;
}

static int deep_begin(uwspr_ctx *c) {
  if (const int rc = ctx_device_ready(c)) return rc;
  if (!c->deep) c->deep = new deep_state();
  return UWSPR_OK;
}

// n > 0 items on the context's stream against a table of M messages (d_tab null: the context's own list): item i reads
// base + off[i] (host array; null: 162 i), results to res (device memory; null: the context's own buffer, returned
// through *res_out)
int deep_run(uwspr_ctx *c, const int8_t *d_tab, int M, const uint8_t *base, const unsigned long long *off, int n,
             uwspr_deep_result *res, uwspr_deep_result **res_out) {
  int rc = deep_begin(c);
  if (rc) return rc;
  deep_state *t = c->deep;
  if (!d_tab) { d_tab = t->d_tab; M = t->M; }
  if (!d_tab || M < 1) return ctx_fail(c, UWSPR_ERR_ARG, "list search: no list is set");
  if (n < 1 || n > (1 << 20)) return ctx_fail(c, UWSPR_ERR_ARG, "list search: %d items in one call (1..%d)", n, 1 << 20);
  if (!res) {
    if ((rc = ctx_grow(c, &t->d_res, &t->cap_res, (size_t)n))) return rc;
    res = t->d_res;
  }
  if (res_out) *res_out = res;
  // the split: enough workgroups for every CU a few times over, at least one tile per wavefront of a workgroup
  const int ntiles = (M + K13_TILE - 1) / K13_TILE, itiles = (n + K13_TILE - 1) / K13_TILE;
  int want = (K13_MAX_CHUNKS + itiles - 1) / itiles;
  int per = (ntiles + want - 1) / want;
  if (per < K13_WAVES) per = K13_WAVES;
  const int nchunks = (ntiles + per - 1) / per;
  if ((rc = ctx_grow(c, &t->d_part, &t->cap_part, (size_t)n * nchunks))) return rc;
  if (off && (rc = scattered_offsets(c, &t->d_off, &t->cap_off, off, n))) return rc;
  if ((rc = t->timer.begin(c))) return rc;
  hipLaunchKernelGGL(k13_score, dim3((unsigned)nchunks, (unsigned)itiles), dim3(64 * K13_WAVES), 0, c->stream, base,
                     off ? t->d_off : (const unsigned long long *)nullptr, n, d_tab, M, per, t->d_part);
  CTXCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k13_reduce, dim3((unsigned)n), dim3(64), 0, c->stream, t->d_part, nchunks, res);
  CTXCHK(c, hipGetLastError());
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_deep_set_list(uwspr_ctx *c, const int8_t *messages7, int M) {
  if (!c) return UWSPR_ERR_ARG;
  if (M != 0) {
    char why[160];
    if (deep_check_list(messages7, M, why, sizeof(why))) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_deep_set_list: %s", why);
  }
  if (M == 0 && !c->deep) return UWSPR_OK;
  int rc = deep_begin(c);
  if (rc) return rc;
  deep_state *t = c->deep;
  int8_t *d_new = nullptr;
  if (M > 0) {
    std::vector<int8_t> tab;
    if (deep_build_table(messages7, M, tab)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_deep_set_list: symbols of a message");
    const hipError_t e = hipMalloc((void **)&d_new, tab.size());
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx_fail(c, UWSPR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", tab.size(), hipGetErrorString(e)); }
    const hipError_t e2 = hipMemcpy(d_new, tab.data(), tab.size(), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) { (void)hipFree(d_new); return ctx_fail(c, UWSPR_ERR_HIP, "hipMemcpy of the table: %s", hipGetErrorString(e2)); }
  }
  CTXCHK(c, hipStreamSynchronize(c->stream));   // a call before may still read the old table
  if (t->d_tab) (void)hipFree(t->d_tab);
  t->d_tab = d_new;
  t->M = M;
  return UWSPR_OK;
}

extern "C" int uwspr_deep_batch(uwspr_ctx *c, const uint8_t *symbols, int n, int where, uwspr_deep_result *res) {
  if (!c) return UWSPR_ERR_ARG;
  return symbols_batch(c, "uwspr_deep_batch", symbols, n, where, res,
                       !c->deep || !c->deep->d_tab ? "no list is set (uwspr_deep_set_list)" : nullptr,
                       [&](symbols_stage **st) { *st = &c->deep->stage; return (int)UWSPR_OK; },
                       [&](const uint8_t *d_sym, uwspr_deep_result *d_res, uwspr_deep_result **d_out) { return deep_run(c, nullptr, 0, d_sym, nullptr, n, d_res, d_out); });
}

// Measurement hook of tools/deep_probe.py (not part of the ABI, like uwspr_debug_osd_time): enable = 1 / 0 switches HIP
// events around the K13 launches of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
// timed pair of launches and returns its time.
extern "C" int uwspr_debug_deep_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->deep) c->deep = new deep_state();   // (no device asked: the hook only keeps the switch)
  return c->deep->timer.read(c, enable, ms);
}
