// k14_calls.hip -- K14: the soft symbols of a candidate scored against every type-1 message of a call set -- known
// callsigns, any locator, any power (uwspr_calls_set / uwspr_calls_batch, the pipe's uwspr_pipe_set_calls).  The definition
// is the comment at uwspr_calls_batch in include/uwspr_hip.h; the reference has no counterpart.  All integers: results are
// the same bytes as the numpy restatement in tests/call_exact.py.
//
// The code is linear and callsign, locator and power sit in disjoint bits of the 50, so with signs 2 c - 1
//     sign[call, g, d][p] = sign[call only][p] * sign[ngrid = g only][p] * sign[dBm + 64 only][p].
// ONE table of the 32400 locator codewords (2025 tiles of 16 rows x 192 bytes in K13's operand layout: tile T, k-step t,
// lane l at byte ((3 T + t) 64 + l) 16, +-1, zero from k = 162 on) serves every callsign and power; a (callsign, power)
// pair is a 162-entry sign, kept as 192 bytes that are 0xFE where the sign is -1 and 0 elsewhere (k >= 162 included).
// XOR of a table byte with 0xFE turns +1 (0x01) into -1 (0xFF) and back and leaves 0 alone, so the sign is folded into A
// and never into B: s = 0 gives -128, whose negation is no int8.
// The product is K13's: v_mfma_i32_16x16x64_i8, A = locators x k, B = k x items (s - 128), the item on the lane
// (col = lane & 15), four locators in the registers (row = 4 (lane >> 4) + reg); both operands have
// k = 64 t + 16 (lane >> 4) + j in byte j of the lane's 16-byte fragment, so the mask fragment of a lane depends on
// lane >> 4 only and a wavefront reads it from LDS as four broadcasts.
// Grid: x = chunks of locator tiles, y = tiles of 16 items, z = callsign.  A workgroup keeps its callsign's masks of the
// allowed powers in LDS (at most 19 x 192 bytes); each of its four wavefronts walks tiles of the chunk: the tile's three A
// fragments are loaded once, then per allowed power 3 XORs, 3 MFMAs and 4 offers.  Tiles with no allowed locator are
// skipped and a disallowed locator or power is never offered.  (best, sbest, snext) per item and workgroup goes to a
// partial array and a second launch merges each item's partials.  Every merge uses the total order (score descending,
// h ascending), so the bytes depend neither on the split nor on the loop order nor on who arrives first.  |S| <= 162 * 128:
// no int32 overflows, and there is no floating point anywhere.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx_util.h"
#include "uwspr_internal.h"

namespace uwspr {

constexpr int K14_N = 162, K14_KPAD = 192, K14_KSTEPS = 3, K14_TILE = 16, K14_WAVES = 4;
constexpr int K14_NGRID = UWSPR_CALL_NGRID, K14_NPOW = UWSPR_CALL_NPOW;
constexpr int K14_TILES = K14_NGRID / K14_TILE;       // 2025: 32400 is a multiple of 16
constexpr int K14_TILE_BYTES = K14_TILE * K14_KPAD;   // 3072
constexpr int K14_MAX_GROUPS = 2048;                  // workgroups aimed at per launch
static_assert(K14_TILES * K14_TILE == K14_NGRID, "the locator table has no partial tile");
static const int kP19[K14_NPOW] = {0, 3, 7, 10, 13, 17, 20, 23, 27, 30, 33, 37, 40, 43, 47, 50, 53, 57, 60};

typedef int k14_v4i __attribute__((ext_vector_type(4)));

// a running winner and runner-up score: (s, h) is better than (s', h') when s > s', or s == s' and h < h'
struct k14_top {
  int32_t best, sbest, snext;
};
__device__ __forceinline__ k14_top k14_empty() { return k14_top{INT32_MAX, INT32_MIN, INT32_MIN}; }
__device__ __forceinline__ void k14_offer(k14_top &t, int32_t s, int32_t h) {
  if (s > t.sbest || (s == t.sbest && h < t.best)) { t.snext = t.sbest; t.sbest = s; t.best = h; }
  else if (s > t.snext) t.snext = s;
}
// two disjoint sets of hypotheses: the winner is the better winner, the runner-up the best of everything else
__device__ __forceinline__ k14_top k14_merge(const k14_top &a, const k14_top &b) {
  const bool a_wins = a.sbest > b.sbest || (a.sbest == b.sbest && a.best < b.best);
  const k14_top &w = a_wins ? a : b, &l = a_wins ? b : a;
  return k14_top{w.best, w.sbest, w.snext > l.sbest ? w.snext : l.sbest};
}
__device__ __forceinline__ k14_top k14_shfl_xor(const k14_top &t, int d) {
  return k14_top{__shfl_xor(t.best, d), __shfl_xor(t.sbest, d), __shfl_xor(t.snext, d)};
}

// base + off[item] (off null: 162 * item): the item's 162 interleaved soft symbols.  tab: the 2025 locator tiles.
// bitmap16[T]: bit r = locator 16 T + r is allowed.  masks [A][19][192]: the (callsign, power) signs as XOR bytes in k
// order.  pow_idx[0 .. npow): the allowed indices into P19, ascending.  part [n][gridDim.z * gridDim.x].
__global__ void __launch_bounds__(64 * K14_WAVES) k14_score(const uint8_t *__restrict__ base, const unsigned long long *__restrict__ off,
                                                            int n, const int8_t *__restrict__ tab, const uint16_t *__restrict__ bitmap16,
                                                            const uint8_t *__restrict__ masks, const int *__restrict__ pow_idx, int npow,
                                                            int tiles_per_chunk, k14_top *__restrict__ part) {
  __shared__ k14_v4i smask[K14_NPOW][K14_KSTEPS][4];   // [power slot][k-step][lane >> 4]: 16 bytes each, 3648 bytes
  __shared__ int spow[K14_NPOW];
  __shared__ k14_top red[K14_WAVES][K14_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int item = blockIdx.y * K14_TILE + col, call = blockIdx.z;
  const int tile0 = blockIdx.x * tiles_per_chunk;
  const int tile1 = tile0 + tiles_per_chunk < K14_TILES ? tile0 + tiles_per_chunk : K14_TILES;

  // the callsign's masks of the allowed powers: 12 fragments of 16 bytes per power, k0 = 64 t + 16 g
  for (int i = threadIdx.x; i < npow * K14_KSTEPS * 4; i += 64 * K14_WAVES) {
    const int slot = i / (K14_KSTEPS * 4), frag = i % (K14_KSTEPS * 4);
    const uint8_t *src = masks + ((size_t)call * K14_NPOW + pow_idx[slot]) * K14_KPAD + 16 * frag;
    (&smask[slot][0][0])[frag] = *(const k14_v4i *)src;
  }
  if ((int)threadIdx.x < npow) spow[threadIdx.x] = pow_idx[threadIdx.x];

  // B: this lane's 3 x 16 bytes of its item, s - 128 (= s ^ 0x80 as int8), zeros from k = 162 on and for items past n
  k14_v4i b[K14_KSTEPS];
  {
    const uint8_t *sym = item < n ? base + (off ? off[item] : (unsigned long long)item * K14_N) : nullptr;
#pragma unroll
    for (int t = 0; t < K14_KSTEPS; t++) {
      const int k0 = 64 * t + 16 * grp;
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int k = k0 + 4 * q + j;
          const uint32_t byte = (sym && k < K14_N) ? (uint32_t)(sym[k] ^ 0x80u) : 0u;
          v |= byte << (8 * j);
        }
        w[q] = v;
      }
      b[t] = k14_v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }
  }
  __syncthreads();

  k14_top top = k14_empty();
  for (int T = tile0 + wave; T < tile1; T += K14_WAVES) {
    const uint32_t allowed = bitmap16[T];
    if (allowed == 0u) continue;   // (uniform over the wavefront)
    const k14_v4i *ap = (const k14_v4i *)(tab + (size_t)T * K14_TILE_BYTES) + lane;
    k14_v4i a[K14_KSTEPS];
#pragma unroll
    for (int t = 0; t < K14_KSTEPS; t++) a[t] = ap[64 * t];
    const int g0 = T * K14_TILE + 4 * grp;   // acc[r] = S[call, locator g0 + r, power][item]
    const uint32_t mine = (allowed >> (4 * grp)) & 15u;
    for (int slot = 0; slot < npow; slot++) {
      k14_v4i acc = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < K14_KSTEPS; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t] ^ smask[slot][t][grp], b[t], acc, 0, 0, 0);
      const int d = spow[slot];
#pragma unroll
      for (int r = 0; r < 4; r++)
        if ((mine >> r) & 1u) k14_offer(top, acc[r], (call * K14_NGRID + g0 + r) * K14_NPOW + d);
    }
  }
  // the four lane groups of a wavefront hold disjoint hypotheses of the same item, then the four wavefronts
  top = k14_merge(top, k14_shfl_xor(top, 16));
  top = k14_merge(top, k14_shfl_xor(top, 32));
  if (grp == 0) red[wave][col] = top;
  __syncthreads();
  if (wave == 0 && grp == 0 && item < n) {
#pragma unroll
    for (int w = 1; w < K14_WAVES; w++) top = k14_merge(top, red[w][col]);
    part[(size_t)item * (gridDim.z * gridDim.x) + blockIdx.z * gridDim.x + blockIdx.x] = top;
  }
}

// one wavefront per item: its nparts partials (disjoint sets of hypotheses, some of them empty) -> the result
__global__ void __launch_bounds__(64) k14_reduce(const k14_top *__restrict__ part, int nparts, uwspr_call_result *__restrict__ res) {
  const int lane = threadIdx.x, item = blockIdx.x;
  k14_top top = k14_empty();
  for (int c = lane; c < nparts; c += 64) top = k14_merge(top, part[(size_t)item * nparts + c]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) top = k14_merge(top, k14_shfl_xor(top, d));
  if (lane == 0) {
    const int dbm[K14_NPOW] = {0, 3, 7, 10, 13, 17, 20, 23, 27, 30, 33, 37, 40, 43, 47, 50, 53, 57, 60};
    uwspr_call_result r;
    r.best = top.best;
    r.call = top.best / (K14_NGRID * K14_NPOW);
    r.ngrid = (top.best / K14_NPOW) % K14_NGRID;
    r.dbm = dbm[top.best % K14_NPOW];
    r.sbest = top.sbest; r.snext = top.snext; r.reserved[0] = r.reserved[1] = 0;
    res[item] = r;
  }
}

// ---------------------------------------------------------------- host side
// A call set on the device (read-only once made): the locator table, the bitmap as one 16-bit word per tile, the masks and
// the allowed powers; on the host the callsigns' n1 for message(h).
struct calls_set {
  int A = 0, npow = 0;
  long long nhyp = 0;
  int8_t *d_tab = nullptr;
  uint16_t *d_bitmap = nullptr;
  uint8_t *d_masks = nullptr;
  int *d_pow = nullptr;
  int32_t n1[UWSPR_CALLS_MAX];
};

struct calls_state {
  calls_set *set = nullptr;                                     // uwspr_calls_set's
  symbols_stage stage;                                          // host symbols staged
  uwspr_call_result *d_res = nullptr; size_t cap_res = 0;
  unsigned long long *d_off = nullptr; size_t cap_off = 0;      // byte offsets of scattered items
  k14_top *d_part = nullptr; size_t cap_part = 0;
  launch_timer timer;                                           // uwspr_debug_calls_time
};

void calls_free_set(calls_set *s) {
  if (!s) return;
  void *bufs[] = {s->d_tab, s->d_bitmap, s->d_masks, s->d_pow};
  for (void *b : bufs) if (b) (void)hipFree(b);
  delete s;
}

void calls_release(uwspr_ctx *c) {
  if (!c || !c->calls) return;
  calls_state *t = c->calls;
  calls_free_set(t->set);
  void *bufs[] = {t->stage.d_sym, t->d_res, t->d_off, t->d_part};
  for (void *b : bufs) if (b) (void)hipFree(b);
  t->timer.release();
  delete t;
  c->calls = nullptr;
}

static void calls_put50(int32_t n1, int32_t n2, int8_t *m) {
  uint8_t *d = (uint8_t *)m;
  d[0] = (uint8_t)(n1 >> 20); d[1] = (uint8_t)(n1 >> 12); d[2] = (uint8_t)(n1 >> 4);
  d[3] = (uint8_t)(((n1 & 15) << 4) | ((n2 >> 18) & 15));
  d[4] = (uint8_t)(n2 >> 10); d[5] = (uint8_t)(n2 >> 2); d[6] = (uint8_t)((n2 & 3) << 6);
}

// a text uwspr_wspr_pack takes as the callsign of a type-1 message -> its 28 bits
static bool calls_n1(const char *call, int32_t *n1) {
  if (!call) return false;
  const size_t len = strlen(call);
  if (len < 3 || len > 6) return false;
  for (size_t i = 0; i < len; i++) {
    const char ch = call[i];
    if (!((ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'))) return false;   // no '/', '<', blank
  }
  char text[32];
  int8_t m[7];
  snprintf(text, sizeof(text), "%s AA00 0", call);
  if (uwspr_wspr_pack(text, m) != UWSPR_OK) return false;
  const uint8_t *d = (const uint8_t *)m;
  *n1 = ((int32_t)d[0] << 20) | ((int32_t)d[1] << 12) | ((int32_t)d[2] << 4) | (d[3] >> 4);
  return true;
}

static int calls_power_index(int dbm) {
  for (int d = 0; d < K14_NPOW; d++) if (kP19[d] == dbm) return d;
  return -1;
}

// message(h) of a set
void calls_message(const calls_set *s, int h, int8_t *message7) {
  const int a = h / (K14_NGRID * K14_NPOW), g = (h / K14_NPOW) % K14_NGRID, d = h % K14_NPOW;
  calls_put50(s->n1[a], 128 * g + kP19[d] + 64, message7);
}
long long calls_count(const calls_set *s) { return s ? s->nhyp : 0; }

// the rules of a call set (include/uwspr_hip.h), no device asked: null on success, else what is wrong (into msg)
const char *calls_check(const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask, int32_t *n1_out,
                        char *msg, size_t cap) {
  if (!calls || A < 1 || A > UWSPR_CALLS_MAX) { snprintf(msg, cap, "calls %p, A %d (1..%d)", (const void *)calls, A, UWSPR_CALLS_MAX); return msg; }
  if (power_mask >> K14_NPOW) { snprintf(msg, cap, "power_mask 0x%x has bits beyond the %d powers", power_mask, K14_NPOW); return msg; }
  int32_t n1[UWSPR_CALLS_MAX];
  for (int a = 0; a < A; a++) {
    if (!calls_n1(calls[a], &n1[a])) {
      snprintf(msg, cap, "callsign %d (\"%.12s\") is not the callsign of a type-1 message (3 to 6 letters and digits, no compound or hashed callsign)",
               a, calls[a] ? calls[a] : "(null)");
      return msg;
    }
    for (int b = 0; b < a; b++)
      if (n1[b] == n1[a]) { snprintf(msg, cap, "callsign %d (\"%.12s\") appears twice in the set", a, calls[a]); return msg; }
  }
  if (grid_bitmap) {
    bool any = false;
    for (int i = 0; i < K14_NGRID / 8 && !any; i++) any = grid_bitmap[i] != 0;
    if (!any) { snprintf(msg, cap, "the set is empty: the locator bitmap allows no locator"); return msg; }
  }
  if (n1_out) memcpy(n1_out, n1, sizeof(int32_t) * (size_t)A);
  return nullptr;
}

// a checked set -> device memory of the current device; null with why in msg
calls_set *calls_build(const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask, int *status, char *msg, size_t cap) {
  calls_set *s = new calls_set();
  *status = UWSPR_ERR_ARG;
  if (calls_check(calls, A, grid_bitmap, power_mask, s->n1, msg, cap)) { delete s; return nullptr; }
  s->A = A;
  if (!power_mask) power_mask = (1u << K14_NPOW) - 1u;
  int pw[K14_NPOW];
  for (int d = 0; d < K14_NPOW; d++) if ((power_mask >> d) & 1u) pw[s->npow++] = d;
  // the locator table: the messages with only ngrid set, through the list search's table builder (the same operand layout)
  std::vector<int8_t> msgs((size_t)K14_NGRID * 7), tab;
  for (int g = 0; g < K14_NGRID; g++) calls_put50(0, 128 * g, &msgs[7 * (size_t)g]);
  std::vector<uint16_t> bm((size_t)K14_TILES);
  long long ngrids = 0;
  for (int T = 0; T < K14_TILES; T++) {
    bm[T] = grid_bitmap ? (uint16_t)(grid_bitmap[2 * T] | (grid_bitmap[2 * T + 1] << 8)) : (uint16_t)0xffff;
    ngrids += __builtin_popcount(bm[T]);
  }
  s->nhyp = (long long)A * ngrids * s->npow;
  // the masks: 0xFE where the (callsign, power) sign is -1, that is where the two partial code bits differ
  std::vector<uint8_t> masks((size_t)A * K14_NPOW * K14_KPAD, 0);
  uint8_t csym[K14_N], psym[K14_NPOW][K14_N];
  int8_t m7[7];
  bool ok = deep_build_table(msgs.data(), K14_NGRID, tab) == UWSPR_OK && tab.size() == (size_t)K14_TILES * K14_TILE_BYTES;
  for (int d = 0; d < K14_NPOW && ok; d++) { calls_put50(0, kP19[d] + 64, m7); ok = uwspr_wspr_symbols(m7, psym[d]) == UWSPR_OK; }
  for (int a = 0; a < A && ok; a++) {
    calls_put50(s->n1[a], 0, m7);
    ok = uwspr_wspr_symbols(m7, csym) == UWSPR_OK;
    for (int d = 0; d < K14_NPOW; d++)
      for (int k = 0; k < K14_N; k++)
        masks[((size_t)a * K14_NPOW + d) * K14_KPAD + k] = ((csym[k] >> 1) ^ (psym[d][k] >> 1)) ? 0xFE : 0x00;
  }
  if (!ok) { snprintf(msg, cap, "symbols of a partial message"); delete s; return nullptr; }
  struct { void **dst; const void *src; size_t bytes; } up[] = {
      {(void **)&s->d_tab, tab.data(), tab.size()},
      {(void **)&s->d_bitmap, bm.data(), bm.size() * sizeof(uint16_t)},
      {(void **)&s->d_masks, masks.data(), masks.size()},
      {(void **)&s->d_pow, pw, sizeof(int) * (size_t)s->npow}};
  for (auto &u : up) {
    hipError_t e = hipMalloc(u.dst, u.bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *status = UWSPR_ERR_NOMEM; snprintf(msg, cap, "hipMalloc(%zu bytes): %s", u.bytes, hipGetErrorString(e)); calls_free_set(s); return nullptr; }
    e = hipMemcpy(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { *status = UWSPR_ERR_HIP; snprintf(msg, cap, "hipMemcpy of the call set: %s", hipGetErrorString(e)); calls_free_set(s); return nullptr; }
  }
  *status = UWSPR_OK;
  return s;
}

static int calls_begin(uwspr_ctx *c) {
  if (const int rc = ctx_device_ready(c)) return rc;
  if (!c->calls) c->calls = new calls_state();
  return UWSPR_OK;
}

// n > 0 items on the context's stream against a set (null: the context's own): item i reads base + off[i] (host array;
// null: 162 i), results to res (device memory; null: the context's own buffer, returned through *res_out)
int calls_run(uwspr_ctx *c, const calls_set *set, const uint8_t *base, const unsigned long long *off, int n,
              uwspr_call_result *res, uwspr_call_result **res_out) {
  int rc = calls_begin(c);
  if (rc) return rc;
  calls_state *t = c->calls;
  if (!set) set = t->set;
  if (!set) return ctx_fail(c, UWSPR_ERR_ARG, "call search: no call set is set");
  if (n < 1 || n > (1 << 20)) return ctx_fail(c, UWSPR_ERR_ARG, "call search: %d items in one call (1..%d)", n, 1 << 20);
  if (!res) {
    if ((rc = ctx_grow(c, &t->d_res, &t->cap_res, (size_t)n))) return rc;
    res = t->d_res;
  }
  if (res_out) *res_out = res;
  // the split of the 2025 locator tiles: enough workgroups for every CU a few times over, at least one tile per wavefront
  const int itiles = (n + K14_TILE - 1) / K14_TILE;
  int want = (K14_MAX_GROUPS + itiles * set->A - 1) / (itiles * set->A);
  int per = (K14_TILES + want - 1) / want;
  if (per < K14_WAVES) per = K14_WAVES;
  const int nchunks = (K14_TILES + per - 1) / per, nparts = nchunks * set->A;
  if ((rc = ctx_grow(c, &t->d_part, &t->cap_part, (size_t)n * nparts))) return rc;
  if (off && (rc = scattered_offsets(c, &t->d_off, &t->cap_off, off, n))) return rc;
  if ((rc = t->timer.begin(c))) return rc;
  // item tiles go in slices of at most 65535 on the grid's y
  for (int y0 = 0; y0 < itiles; y0 += 65535) {
    const int ny = itiles - y0 < 65535 ? itiles - y0 : 65535, i0 = y0 * K14_TILE;
    hipLaunchKernelGGL(k14_score, dim3((unsigned)nchunks, (unsigned)ny, (unsigned)set->A), dim3(64 * K14_WAVES), 0, c->stream,
                       off ? base : base + (size_t)i0 * K14_N, off ? t->d_off + i0 : (const unsigned long long *)nullptr, n - i0,
                       set->d_tab, set->d_bitmap, set->d_masks, set->d_pow, set->npow, per, t->d_part + (size_t)i0 * nparts);
    CTXCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k14_reduce, dim3((unsigned)n), dim3(64), 0, c->stream, t->d_part, nparts, res);
  CTXCHK(c, hipGetLastError());
  return t->timer.end(c);
}

}  // namespace uwspr

using namespace uwspr;

extern "C" int uwspr_call_message(const char *call, int ngrid, int dbm, int8_t *message7) {
  int32_t n1;
  if (!message7 || !calls_n1(call, &n1) || ngrid < 0 || ngrid >= K14_NGRID || calls_power_index(dbm) < 0) return UWSPR_ERR_ARG;
  calls_put50(n1, 128 * ngrid + dbm + 64, message7);
  return UWSPR_OK;
}

extern "C" int uwspr_calls_set(uwspr_ctx *c, const char *const *calls, int A, const uint8_t *grid_bitmap, uint32_t power_mask) {
  if (!c) return UWSPR_ERR_ARG;
  char why[200];
  if (A != 0 && calls_check(calls, A, grid_bitmap, power_mask, nullptr, why, sizeof(why)))
    return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_calls_set: %s", why);
  if (A == 0 && !c->calls) return UWSPR_OK;
  int rc = calls_begin(c);
  if (rc) return rc;
  calls_state *t = c->calls;
  calls_set *fresh = nullptr;
  if (A > 0) {
    fresh = calls_build(calls, A, grid_bitmap, power_mask, &rc, why, sizeof(why));
    if (!fresh) return ctx_fail(c, rc, "uwspr_calls_set: %s", why);
  }
  const hipError_t e = hipStreamSynchronize(c->stream);   // a call before may still read the old set
  if (e != hipSuccess) { calls_free_set(fresh); return ctx_fail(c, UWSPR_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e)); }
  calls_free_set(t->set);
  t->set = fresh;
  return UWSPR_OK;
}

extern "C" int uwspr_calls_batch(uwspr_ctx *c, const uint8_t *symbols, int n, int where, uwspr_call_result *res) {
  if (!c) return UWSPR_ERR_ARG;
  return symbols_batch(c, "uwspr_calls_batch", symbols, n, where, res,
                       !c->calls || !c->calls->set ? "no call set is set (uwspr_calls_set)" : nullptr,
                       [&](symbols_stage **st) { *st = &c->calls->stage; return (int)UWSPR_OK; },
                       [&](const uint8_t *d_sym, uwspr_call_result *d_res, uwspr_call_result **d_out) { return calls_run(c, nullptr, d_sym, nullptr, n, d_res, d_out); });
}

// The pipe's item form for tests/test_gpu_calls.py (not part of the ABI): item i = the 162 bytes at base + off[i], base in
// device memory, off and res in host memory; every item must lie inside base's allocation.
extern "C" int uwspr_debug_calls_scattered(uwspr_ctx *c, const uint8_t *base, const unsigned long long *off, int n, uwspr_call_result *res) {
  if (!c) return UWSPR_ERR_ARG;
  if (!base || !off || !res || n < 1 || !c->calls || !c->calls->set) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_debug_calls_scattered: arguments, or no call set");
  if (const int rc = ctx_device_ready(c)) return rc;
  unsigned long long last = 0;
  for (int i = 0; i < n; i++) last = off[i] > last ? off[i] : last;
  if (!ctx_device_range(c, base, (size_t)last + K14_N)) return ctx_fail(c, UWSPR_ERR_ARG, "uwspr_debug_calls_scattered: an item lies outside base's allocation");
  uwspr_call_result *d_res = nullptr;
  if (const int rc = calls_run(c, nullptr, base, off, n, nullptr, &d_res)) return rc;
  CTXCHK(c, hipMemcpyAsync(res, d_res, (size_t)n * sizeof(uwspr_call_result), hipMemcpyDeviceToHost, c->stream));
  CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// Measurement hook of tools/call_probe.py (not part of the ABI, like uwspr_debug_deep_time): enable = 1 / 0 switches HIP
// events around the K14 launches of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
// timed run's launches and returns their time.
extern "C" int uwspr_debug_calls_time(uwspr_ctx *c, int enable, double *ms) {
  if (!c) return UWSPR_ERR_ARG;
  if (!c->calls) c->calls = new calls_state();   // (no device asked: the hook only keeps the switch)
  return c->calls->timer.read(c, enable, ms);
}
