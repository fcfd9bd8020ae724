"""TEST INFRASTRUCTURE ONLY -- K11 (gr-uwspr_amd/csrc/k11_resample.hip), the rational resampler ahead of K0, restated
to the bit in numpy from the text of include/uwspr_hip.h ("audio at other rates"); no GPU needed.

  design          the prototype low-pass in binary64: (h [T L], L, M, T, N, D)
  taps32          hp[p][t] = (float) h[p + t L]
  restate         y[j] for chosen absolute outputs of audio that counts as zero outside its buffer: one chain of
                  binary32 fused multiply-adds per output, t = T - 1 .. 0, from +0 (fma32 of tests/frontend_exact.py)
  convolve64      the same outputs in binary64 from the same binary32 taps, and sum |hp x| for the rounding bound
  impulse_train   isolated impulses that meet every (p, t) pair, with the closed-form expectation (one rounding)
  MUTATIONS       the indexing mistakes the tests must be able to see, as changed restatements

and the inputs + expectations the CPU and GPU tests share, built once per rate."""
import math

import numpy as np

from frontend_exact import _fma_core, noise32, noise16, s16_to_f32  # noqa: F401

OUT_RATE = 12000
RATES = (8000, 9600, 10000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000)
WG_OUT = 256            # outputs per workgroup of K11


def supported(rate):
    if not 8000 <= rate <= 192000:
        return False
    return OUT_RATE // math.gcd(rate, OUT_RATE) <= 160


def design(rate):
    """-> (h float64 [T * L], L, M, T, N, D), from the header's text"""
    assert supported(rate) and rate != OUT_RATE
    g = math.gcd(rate, OUT_RATE)
    L, M = OUT_RATE // g, rate // g
    A = 100.0
    beta = 0.1102 * (A - 8.7)
    F = float(L) * rate
    fp, fs = 2400.0, min(rate, OUT_RATE) - 2400.0
    fc = (fp + fs) / 2.0
    dw = 2.0 * math.pi * (fs - fp) / F
    N = int(math.ceil((A - 8.0) / (2.285 * dw))) + 1
    N += 1 - (N & 1)
    T = -(-N // L)
    D = (N - 1) // 2
    k = np.arange(N, dtype=np.float64)
    w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * k / (N - 1) - 1.0) ** 2))) / np.i0(beta)
    h = (2.0 * fc / F) * np.sinc((2.0 * fc / F) * (k - D)) * w
    h *= L / h.sum()
    out = np.zeros(T * L, np.float64)
    out[:N] = h
    return out, L, M, T, N, D


def taps32(h, L, T):
    """[L, T] binary32: hp[p][t] = (float) h[p + t L]"""
    return np.ascontiguousarray(h.reshape(T, L).T.astype(np.float32))


_plans = {}


def plan(rate):
    """-> (hp [L, T] float32, L, M, T, N, D), built once per rate.  L .. D come from `design` above; the taps are the
    LIBRARY's binary64 design (uwspr_resample_design: host code, no GPU) rounded to binary32 here.  tests/test_resample.py
    holds that design to `design` within 1e-12 of the largest tap, which is all that can be asked: where the sinc
    crosses zero (8000 S/s: every third tap) a tap is rounding noise of size 1e-17 whose bits depend on the libm that
    computed sin(), so two correct binary64 designs do not round to the same binary32 there."""
    if rate not in _plans:
        import gr_uwspr_amd as G
        h, L, M, T, N, D = design(rate)
        lib = G.resample_design(rate)
        assert lib[1:] == (L, M, T, D) and len(lib[0]) == N
        assert np.abs(lib[0] - h[:N]).max() <= 1e-12 * np.abs(h).max()
        hl = np.zeros(T * L, np.float64)
        hl[:N] = lib[0]
        _plans[rate] = (taps32(hl, L, T), L, M, T, N, D)
    return _plans[rate]


# ---- the kernel's sums -----------------------------------------------------------------------------------------
def indices(js, L, M, D, d_off=0, round_up=False):
    """-> (i0, p) of absolute outputs js (python ints inside: 64-bit exact)"""
    q = np.asarray(js, np.int64) * M + (D + d_off)
    i0 = -((-q) // L) if round_up else q // L
    return i0, q % L


def _window(x, x_origin, i0, T):
    """W[t] = x[i0 - t] (zero outside the buffer) as float64, [T, len(i0)]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    X = np.concatenate([np.zeros(1, np.float64), x.astype(np.float64)])
    idx = i0[None, :] - np.arange(T, dtype=np.int64)[:, None] - int(x_origin)
    ok = (idx >= 0) & (idx < len(x))
    return X[np.where(ok, idx + 1, 0)]


def restate(rate, x, x_origin, js, mutation=None, chunk=4096):
    """K11's bytes: float32 [len(js)] for absolute outputs js of x = audio [x_origin, x_origin + len(x))"""
    hp, L, M, T, N, D = plan(rate)
    js = np.asarray(js, np.int64)
    out = np.zeros(len(js), np.float32)
    hp64 = hp.astype(np.float64)
    for a in range(0, len(js), chunk):
        i0, p = indices(js[a:a + chunk], L, M, D, d_off=1 if mutation == "delay_off_by_one" else 0,
                        round_up=mutation == "i0_rounded_up")
        if mutation == "phases_swapped":          # phases p and p + 1 exchanged (pairs 2k, 2k + 1; a last odd one stays)
            p = np.where((p ^ 1) < L, p ^ 1, p)
        W = _window(x, x_origin, i0, T)
        acc = np.zeros(len(i0), np.float64)       # (binary32 values, carried in binary64)
        t_lo = 0
        t_hi = T - 2 if mutation == "last_tap_dropped" else T - 1
        for t in range(t_hi, t_lo - 1, -1):
            acc = _fma_core(hp64[p, t] * W[t], acc).astype(np.float64)
        out[a:a + chunk] = acc.astype(np.float32)
    return out


MUTATIONS = ("phases_swapped", "last_tap_dropped", "delay_off_by_one", "i0_rounded_up")


def convolve64(rate, x, x_origin, js):
    """-> (the same outputs in binary64 from the same binary32 taps and samples, sum_t |hp x| per output)"""
    hp, L, M, T, N, D = plan(rate)
    i0, p = indices(js, L, M, D)
    W = _window(x, x_origin, i0, T)
    G = hp.astype(np.float64)[p, :].T             # [T, n]
    return (G * W).sum(axis=0), np.abs(G * W).sum(axis=0)


# ---- impulse trains ------------------------------------------------------------------------------------------------
def impulse_train(rate, nin):
    """-> (x float32 [nin], positions, amplitudes).  Impulses at least T + 1 apart, so every output's window holds at
    most one and the output is one rounding of one tap.  An impulse at n meets output j with tap k = p + t L =
    j M + D - n L, i.e. the taps k = D - n L (mod M); gcd(L, M) = 1, so the positions have to run through every residue
    mod M: the stride is the first number >= T + 1 that is 1 mod M.  (The first impulses lie closer than D / L to the
    record's start and miss their low taps: the train goes through the residues more than twice.)  The coverage is
    ASSERTED where the train is used (impulse_expect's hit counts)."""
    hp, L, M, T, N, D = plan(rate)
    rng = np.random.default_rng(1100 + rate % 997)
    stride = M * (-(-T // M)) + 1
    assert stride >= T + 1 and nin > (2 * M + D // L + 2) * stride
    pos = np.arange(0, nin, stride, dtype=np.int64)
    amp = (rng.uniform(0.5, 2.0, len(pos)) * rng.choice([-1.0, 1.0], len(pos))).astype(np.float32)
    amp[np.abs(np.frexp(amp)[0]) == 0.5] *= np.float32(1.25)       # no powers of two
    x = np.zeros(nin, np.float32)
    x[pos] = amp
    return x, pos, amp


def impulse_expect(rate, x, nout, j_first=0, x_origin=0):
    """closed form for an isolated-impulse input: out[j] = fl32(hp[p][t] a) for the one impulse in the window (every
    other fused multiply-add meets a zero: +0 stays +0 and a value stays itself), +0 where there is none.
    -> (expectation float32 [nout], hit [L, T] counts of the (p, t) pairs met)"""
    hp, L, M, T, N, D = plan(rate)
    js = j_first + np.arange(nout, dtype=np.int64)
    i0, p = indices(js, L, M, D)
    W = _window(x, x_origin, i0, T)
    nz = W != 0.0
    assert (nz.sum(axis=0) <= 1).all(), "impulses closer than a window"
    t = nz.argmax(axis=0)
    has = nz.any(axis=0)
    a = W[t, np.arange(nout)]
    out = np.where(has, (hp.astype(np.float64)[p, t] * a).astype(np.float32), np.float32(0)).astype(np.float32)
    out = out + np.float32(0)                                       # (a -0 product added to the chain's +0 is +0)
    hit = np.zeros((L, T), np.int64)
    np.add.at(hit, (p[has], t[has]), 1)
    return out, hit


# ---- shared cases ----------------------------------------------------------------------------------------------------
IMP_RATES = (48000, 44100, 8000, 11025)
GPU_RATES = (8000, 11025, 44100, 48000, 192000)
_cache = {}


def impulse_nin(rate):
    """enough input for every (p, t) pair (asserted where it is used), around 20 000 where that suffices"""
    return {44100: 60013, 11025: 50021, 192000: 30011}.get(rate, 20011)


def impulse_nout(rate, nin):
    """the record ends inside an output's window and the last output block is ragged: up to the first output whose
    whole window lies behind the record, which is no multiple of the workgroup's 256 (one more if it is)"""
    hp, L, M, T, N, D = plan(rate)
    j = ((nin + T) * L - D) // M + 2
    return j + 1 if j % WG_OUT == 0 else j


def impulse_case(rate):
    """-> (x [nin] float32, expectation [nout] float32, hit [L, T])"""
    key = ("imp", rate)
    if key not in _cache:
        nin = impulse_nin(rate)
        x, _, _ = impulse_train(rate, nin)
        exp, hit = impulse_expect(rate, x, impulse_nout(rate, nin))
        _cache[key] = (x, exp, hit)
    return _cache[key]


DENSE_NIN = 20003


def dense_case(rate, nch):
    """-> (x int16 [DENSE_NIN, nch], expectation float32 [nout, nch]) -- dense noise, every output restated"""
    key = ("dense", rate, nch)
    if key not in _cache:
        x = noise16(np.random.default_rng(1200 + nch), (DENSE_NIN, nch))
        nout = impulse_nout(rate, DENSE_NIN)
        js = np.arange(nout)
        exp = np.stack([restate(rate, s16_to_f32(x[:, c]), 0, js) for c in range(nch)], axis=1)
        _cache[key] = (x, exp)
    return _cache[key]
