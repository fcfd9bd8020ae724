// The audio chain's bookkeeping (gr-uwspr_amd/csrc/stream_stage.h) walked on the CPU: K12 -> K11 -> K0 as counters,
// no samples, over every chain, resampler plan, channel count and a set of cut schedules.  After every piece:
//   (a) each launch's read window -- the first and last input its outputs read -- lies in the stage's buffer
//       [i_base, i_base + hist + k); inputs before index 0 do not exist (K11 and K12 read them as nothing).  K0's
//       history is zero-filled at the latch, so its window is held to the buffer without exception;
//   (b) hist + k, the outputs of the piece, the level rows and the zero counts in use fit the sizes the header computes
//       (what the ring allocates);
//   (c) after all pieces every stage has made complete(total) outputs: the cuts do not matter;
//   (d) what the counters predict for a push before it is what the stages then make.
// Carriers only multiply the ring's planes (no formula of the header reads their count), so they are carried along
// and held to the plane limit only.
// usage: stream_stage_main fe:J:dcols ... rs:rate:L:M:T:D ...   (from tests/test_host_tail.py)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "stream_stage.h"

namespace st = uwspr::stage;

static const char *g_case = "";
#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) { printf("FAILED %s\n  %s (line %d)\n", #cond, g_case, __LINE__); exit(1); }           \
  } while (0)

constexpr size_t AUDIO_PIECE = 4u << 20;   // stream_ring::AUDIO_PIECE
constexpr int MAX_PLANES = 64;             // UWSPR_PIPE_MAX_CHANNELS

struct plan { int rate, L, M, T, D; };
struct frontend { int J, dcols; };

struct k0_stage {
  frontend fe; size_t C, piece; long long m0, m_next; st::history h;
  void latch(frontend f, size_t C_, long long p) {
    fe = f; C = C_; piece = AUDIO_PIECE / C; m0 = m_next = p;
    h.i_base = st::audio_keep(p, fe.J, fe.dcols); h.hist = (size_t)(32 * p - h.i_base);   // (zero-filled)
  }
  long long predict(long long n) const { return st::added(st::audio_complete(h.i_base + (long long)h.hist + n, fe.dcols), m_next); }
  void push(size_t n) {
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      const long long held = (long long)(h.hist + k), a_end = h.i_base + held;
      CHECK((size_t)held * C <= st::audio_need(fe.J, piece, C) && held <= INT32_MAX);                       // (b)
      const long long m_end = st::audio_complete(a_end, fe.dcols);
      if (m_end > m_next) {   // outputs [m_next, m_end): taps k < 32 J of x[32 (m + dcols) - k]
        const long long first = 32 * (m_next + fe.dcols - fe.J) + 1, last = 32 * (m_end - 1 + fe.dcols);
        CHECK(first >= h.i_base && last < a_end);                                                           // (a)
        m_next = m_end;
      }
      h.advance(k, st::audio_keep(m_next, fe.J, fe.dcols));
      CHECK(h.i_base + (long long)h.hist == a_end);
      off += k;
    }
  }
};

struct k11_stage {
  plan pl; size_t C, outp, piece; long long n_in, j_next; st::history h; k0_stage *next;
  void latch(plan p, size_t C_, k0_stage *nx) {
    pl = p; C = C_; outp = AUDIO_PIECE / C; piece = st::resample_piece_frames(outp, pl.L, pl.M); n_in = j_next = 0; h = st::history(); next = nx;
    CHECK(piece >= 1);
  }
  long long predict(long long n) const { return st::added(st::resample_complete(n_in + n, pl.L, pl.M, pl.D), j_next); }
  void push(size_t n) {
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      const long long held = (long long)(h.hist + k);
      CHECK((size_t)held * C <= st::resample_in_need(pl.T, piece, C));                                      // (b)
      n_in += (long long)k;
      CHECK(h.i_base + held == n_in);
      const long long j_end = st::resample_complete(n_in, pl.L, pl.M, pl.D);
      if (j_end > j_next) {
        const long long nout = j_end - j_next;
        CHECK((size_t)nout * C <= st::resample_out_need(outp, C));                                          // (b)
        const long long first = st::resample_last_input(j_next, pl.L, pl.M, pl.D) - (pl.T - 1);
        const long long last = st::resample_last_input(j_end - 1, pl.L, pl.M, pl.D);
        CHECK((first < 0 ? 0 : first) >= h.i_base && last < n_in);                                          // (a)
        j_next = j_end;
        next->push((size_t)nout);
      }
      h.advance(k, st::resample_keep(j_next, pl.L, pl.M, pl.T, pl.D));
      off += k;
    }
  }
};

struct k12_stage {
  int G; size_t C, piece, nz_used; long long n_in, y_next, lev0, blk_done; st::history h; k11_stage *rs; k0_stage *k0;
  void latch(int guard, size_t C_, k11_stage *r, k0_stage *z) {
    G = guard; C = C_; piece = AUDIO_PIECE / C; nz_used = 0; n_in = y_next = lev0 = blk_done = 0; h = st::history(); rs = r; k0 = z;
  }
  long long predict(long long n) const { return st::added(st::blank_complete(n_in + n, G), y_next); }
  void push(size_t n) {
    const long long N = st::BLANK_N;
    for (size_t off = 0; off < n;) {
      const size_t k = n - off < piece ? n - off : piece;
      const long long held = (long long)(h.hist + k);
      CHECK((size_t)held * C <= st::blank_in_need(piece, C));                                               // (b)
      n_in += (long long)k;
      CHECK(h.i_base + held == n_in);
      const long long done = st::blank_blocks_done(n_in);
      if (done > blk_done) {   // levels of blocks [blk_done, done): each reads its own block
        CHECK((size_t)(done - lev0) <= st::blank_lev_rows(piece));                                          // (b)
        CHECK(blk_done * N >= h.i_base && done * N <= n_in);                                                // (a)
        blk_done = done;
      }
      const long long y_end = st::blank_complete(n_in, G);
      if (y_end > y_next) {   // outputs [y_next, y_end): inputs [i - G, i + G], each judged by the level of the block before its own
        const long long nout = y_end - y_next, first = y_next - G < 0 ? 0 : y_next - G, last = y_end - 1 + G;
        const size_t nzn = (size_t)st::blank_blocks_of(y_next, nout) * C;
        CHECK((size_t)nout * C <= piece * C && nzn <= st::blank_nz_cap(piece, C));                          // (b)
        if (nz_used + nzn > st::blank_nz_cap(piece, C)) nz_used = 0;   // (the ring drains the queue)
        nz_used += nzn;
        CHECK(first >= h.i_base && last < n_in);                                                            // (a)
        const long long lev_first = first / N - 1 < 0 ? 0 : first / N - 1, lev_last = last / N - 1;
        CHECK(lev_last < 0 || (lev_first >= lev0 && lev_last < blk_done));                                  // (a): the table
        y_next = y_end;
        if (rs) rs->push((size_t)nout); else k0->push((size_t)nout);
      }
      lev0 = st::blank_lev_first(blk_done);
      CHECK((size_t)(blk_done - lev0) <= st::blank_lev_rows(piece));
      h.advance(k, st::blank_keep(y_next, G, blk_done));
      off += k;
    }
  }
};

static std::vector<std::vector<size_t>> schedules(size_t C) {
  const size_t piece = AUDIO_PIECE / C;
  std::vector<std::vector<size_t>> s;
  s.push_back(std::vector<size_t>(9001, 1));
  s.push_back(std::vector<size_t>(3001, 7));
  for (size_t n : {(size_t)4096, (size_t)4095, (size_t)4097, (size_t)10007}) s.push_back(std::vector<size_t>(9, n));
  s.push_back({5, piece + 12345, 7, piece, 2 * piece + 1});   // pushes the ring cuts into several pieces
  uint64_t x = 0x9e3779b97f4a7c15ull;                         // a fixed-seed schedule: xorshift64
  std::vector<size_t> r;
  for (int i = 0; i < 300; i++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    r.push_back((size_t)(x % (i % 10 == 0 ? 200000 : i % 3 == 0 ? 64 : 9000)));   // (zero-length pushes included)
  }
  s.push_back(r);
  return s;
}

static long long walk(int blank, int guard, const plan *pl, frontend fe, size_t C, int ncar, long long p0, const std::vector<size_t> &cuts) {
  CHECK((long long)C * ncar <= MAX_PLANES);
  k0_stage k0; k11_stage rs; k12_stage bk;
  k0.latch(fe, C, p0);
  if (pl) rs.latch(*pl, C, &k0);
  if (blank) bk.latch(guard, C, pl ? &rs : nullptr, &k0);
  long long total = 0;
  for (size_t n : cuts) {
    // (d) the composition the doors check the ring's room by
    long long want = (long long)n;
    if (blank) want = bk.predict(want);
    if (pl) want = rs.predict(want);
    want = k0.predict(want);
    const long long before = k0.m_next;
    if (blank) bk.push(n); else if (pl) rs.push(n); else k0.push(n);
    CHECK(k0.m_next - before == want);
    total += (long long)n;
  }
  // (c) what one push of everything completes
  long long t = total;
  if (blank) { t = st::added(st::blank_complete(t, guard), 0); CHECK(bk.y_next == t && bk.n_in == total); }
  if (pl) { const long long in = t; t = st::resample_complete(in, pl->L, pl->M, pl->D); CHECK(rs.j_next == t && rs.n_in == in); }
  CHECK(k0.m_next == st::added(st::audio_complete(32 * p0 + t, fe.dcols), p0) + p0);
  return k0.m_next - p0;
}

int main(int argc, char **argv) {
  std::vector<frontend> fes;
  std::vector<plan> plans;
  for (int i = 1; i < argc; i++) {
    frontend f; plan p;
    if (sscanf(argv[i], "fe:%d:%d", &f.J, &f.dcols) == 2) fes.push_back(f);
    else if (sscanf(argv[i], "rs:%d:%d:%d:%d:%d", &p.rate, &p.L, &p.M, &p.T, &p.D) == 5) plans.push_back(p);
    else { printf("bad argument %s\n", argv[i]); return 2; }
  }
  if (fes.empty() || plans.empty()) { printf("usage: stream_stage_main fe:J:dcols ... rs:rate:L:M:T:D ...\n"); return 2; }
  static const int blanks[4][2] = {{0, 0}, {24, 0}, {24, 2}, {24, 64}};
  long long walks = 0, outputs = 0;
  char name[200];
  for (size_t C : {(size_t)1, (size_t)2, (size_t)64}) {
    const std::vector<std::vector<size_t>> sch = schedules(C);
    for (const frontend &fe : fes)
      for (const int (&b)[2] : blanks)
        for (size_t r = 0; r <= plans.size(); r++)   // (r == 0: 12 kS/s, no resampler)
          for (int ncar : {1, 3})
            for (size_t s = 0; s < sch.size(); s++) {
              if (C * ncar > (size_t)MAX_PLANES) continue;
              const long long p0 = (s + ncar) % 2 ? 0 : (1LL << 40) + 5;   // streams reset at a 64-bit origin too
              snprintf(name, sizeof(name), "C %zu J %d dcols %d blank %d guard %d rate %d ncar %d origin %lld schedule %zu", C, fe.J, fe.dcols,
                       b[0], b[1], r ? plans[r - 1].rate : 12000, ncar, p0, s);
              g_case = name;
              outputs += walk(b[0], b[1], r ? &plans[r - 1] : nullptr, fe, C, ncar, p0, sch[s]);
              walks++;
            }
  }
  printf("stream stages ok: %lld walks, %lld ring samples\n", walks, outputs);
  return 0;
}
