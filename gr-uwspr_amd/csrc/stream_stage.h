// stream_stage.h -- the integer bookkeeping of the audio stages ahead of the ring (K12 -> K11 -> K0, stream_ring.h):
// which output a push completes, from which input on a stage must keep its history, and how large its buffers have to
// be for the pieces it is given.  Plain integers, nothing of HIP: tests/host/stream_stage_main.cc walks these formulas
// over cut schedules on the CPU, and stream_ring.h launches and allocates by them and by nothing else.
//
// A stage holds the inputs [i_base, i_base + hist) and is given k more.  A kernel's output reads a window of inputs;
// whatever of it lies outside the buffer reads as zero (K0, K11) or does not exist (K12), which is right only before
// the stream's first sample: every keep index below is the first input the stage's NEXT output reads.
#pragma once

#include <stddef.h>

namespace uwspr {
namespace stage {

// The inputs a stage holds.  advance(): k_new inputs arrived behind them and everything before input `keep` is done
// with (clamped to what is held); the tail [off, off + len) of the buffer is the new history, and when `moves` it goes
// to the front of the other buffer.
struct history {
  long long i_base = 0;                // input index of the buffer's first frame
  size_t hist = 0;                     // frames held: inputs [i_base, i_base + hist)
  struct tail { size_t off, len; bool moves; };
  tail advance(size_t k_new, long long keep) {
    const long long end = i_base + (long long)(hist + k_new);
    if (keep > end) keep = end;
    if (keep < i_base) keep = i_base;
    const tail t = {(size_t)(keep - i_base), (size_t)(end - keep), keep != i_base};
    i_base = keep; hist = t.len;
    return t;
  }
};

inline long long floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
// outputs [next, complete) are new; none when the stage is ahead
inline long long added(long long complete, long long next) { return complete > next ? complete - next : 0; }

// ---- K0: y[m] = sum_k g[k] x[32 m + D - k], k < 32 J, D = 32 dcols: output m reads (32 (m + dcols - J), 32 (m + dcols)]
// stream index one past the last output that audio [.., a_end) completes (a_end may be < D)
inline long long audio_complete(long long a_end, int dcols) { return floordiv(a_end - 1 - 32LL * dcols, 32) + 1; }
// the history's origin: a multiple of 32 just below output m_next's window
inline long long audio_keep(long long m_next, int J, int dcols) { return 32 * (m_next + dcols - J); }
// samples per buffer: at most 32 J of history (and one output's 32 of slack) plus a piece, of C channels
inline size_t audio_need(int J, size_t piece, size_t C) { return ((32 * (size_t)J + 32) + piece) * C; }

// ---- K11: y[j] = sum_{t < T} h[p][t] x[i0 - t], i0 = (j M + D) div L: output j reads [i0 - (T - 1), i0]
inline long long resample_last_input(long long j, int L, int M, int D) { return (j * M + D) / L; }
// one past the last output that n_in pushed inputs complete
inline long long resample_complete(long long n_in, int L, int M, int D) {
  const long long t = n_in * L - 1 - D;
  return t >= 0 ? t / M + 1 : 0;
}
inline long long resample_keep(long long j_next, int L, int M, int T, int D) { return resample_last_input(j_next, L, M, D) - (T - 1); }
// most input frames per launch: their outputs fit a buffer of `outp` frames (one K0 piece) whatever L / M is
inline size_t resample_piece_frames(size_t outp, int L, int M) {
  const size_t by_out = (size_t)((long long)(outp - 2) * M / L);
  return by_out < outp ? by_out : outp;
}
inline size_t resample_in_need(int T, size_t piece, size_t C) { return ((size_t)T + piece) * C; }   // samples per input buffer
inline size_t resample_out_need(size_t outp, size_t C) { return outp * C; }

// ---- K12: output i reads [i - G, i + G] and the levels of blocks b - 2 .. b (b = i div N); level b reads block b
constexpr long long BLANK_N = 4096;    // UWSPR_BLANK_BLOCK
constexpr long long BLANK_GMAX = 64;
inline long long blank_complete(long long n_in, int G) { return n_in - G; }      // one past the last complete output
inline long long blank_blocks_done(long long n_in) { return n_in / BLANK_N; }
// what is not yet output with its guard, and the incomplete block
inline long long blank_keep(long long y_next, int G, long long blk_done) {
  return y_next - G < blk_done * BLANK_N ? y_next - G : blk_done * BLANK_N;
}
// the level table's first block: it keeps the last three complete ones
inline long long blank_lev_first(long long blk_done) { return blk_done > 3 ? blk_done - 3 : 0; }
// blocks the outputs [y_first, y_first + nout) touch: the zero counts of a launch
inline long long blank_blocks_of(long long y_first, long long nout) {
  return nout > 0 ? (y_first + nout - 1) / BLANK_N - y_first / BLANK_N + 1 : 0;
}
inline size_t blank_in_need(size_t piece, size_t C) { return ((size_t)BLANK_N + 2 * (size_t)BLANK_GMAX + piece) * C; }
inline size_t blank_lev_rows(size_t piece) { return piece / (size_t)BLANK_N + 6; }               // rows of C levels
inline size_t blank_nz_cap(size_t piece, size_t C) { return (piece / (size_t)BLANK_N + 2) * C * 64; }   // ints in the queue

}  // namespace stage
}  // namespace uwspr
