"""TEST INFRASTRUCTURE ONLY -- K0 (gr-uwspr_amd/csrc/k0_frontend.hip) restated to the bit, in numpy, no GPU needed.

K0's arithmetic is fixed per output (its comment: "the tap order is fixed per output"): wavefront w = 0..15 owns the
tap phases 2w and 2w + 1 and runs, per output, ONE chain of binary32 fused multiply-adds -- phase 2w with the tap index
descending (jj = 0..J-1, k = 32 (J - 1 - jj) + p), then phase 2w + 1 likewise -- from +0; the 16 partial sums are
added in wavefront order, in binary32, from +0.  The library is built with -ffp-contract=off and without fast-math and
nothing transcendental is involved, so every output can be stated exactly:

  fma32          the correctly rounded binary32 fused multiply-add (round to odd in binary64, then one cast)
  restate        out[m] for chosen absolute output indices, of audio that counts as zero outside its buffer
  restate_many   the same for several (audio, origin, outputs) items in one pass (the cost is per tap, not per item)
  impulse_expect the closed form for isolated impulses: one rounding of tap x amplitude, +0 elsewhere
  mutate_taps    the loader / tap-image mistakes the tests must be able to see, as a changed tap array

and the inputs + expectations the CPU tests and the GPU tests share (impulse_case, dense_case), built once per mode.
Inputs keep |x| >= 2^-15 or 0, so that no product or sum is subnormal."""
import numpy as np

DEC = 32
WG_OUT = 512            # outputs per workgroup (K0_OUT)
NOUT_BATCH = 45000      # uwspr_frontend_batch: fl outputs per record


# ---- the fused multiply-add ------------------------------------------------------------------------------------
def _fma_core(p, c):
    """fl32(p + c) for binary64 arrays p (an exact product of two binary32 values) and c (a binary32 value): TwoSum
    gives the rounding error of the binary64 sum; a sum that is inexact and even is stepped to its odd neighbour on the
    error's side (round to odd), after which the cast to binary32 rounds once (53 >= 24 + 2 bits)."""
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    need = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(need, np.nextafter(s, np.copysign(np.inf, err)), s)
    return s.astype(np.float32)


def fma32(a, b, c):
    """the correctly rounded binary32 a * b + c of binary32 arrays (fmaf)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p, c = np.broadcast_arrays(a * b, c)                       # (the product of two binary32 values is exact in binary64)
    return _fma_core(p, c)


# ---- the kernel's sums -----------------------------------------------------------------------------------------
def taps_J(nt):
    """taps per phase: ceil(nt / 32), rounded up to a multiple of 8 (frontend_tap_image)"""
    return (-(-nt // DEC) + 7) // 8 * 8


def _padded(taps32):
    g = np.asarray(taps32, np.complex64)
    J = taps_J(len(g))
    gp = np.zeros(DEC * J, np.complex64)
    gp[:len(g)] = g
    return gp, J


def restate_many(taps32, D, items, chunk=1024):
    """items: (x, x_origin, ms) -- x binary32 audio [x_origin, x_origin + len(x)), zero outside; ms absolute output
    indices -> one float32 [len(ms), 2] array per item, K0's bytes."""
    gp, J = _padded(taps32)
    gre, gim = gp.real.astype(np.float64), gp.imag.astype(np.float64)
    flat = [np.zeros(1, np.float32)]
    base, off, ln = [], [], []
    at = 1
    for x, x_origin, ms in items:
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 1
        ms = np.asarray(ms, np.int64)
        flat.append(x)
        base.append(DEC * ms + int(D) - int(x_origin))         # index into x of tap 0's sample
        off.append(np.full(len(ms), at, np.int64))
        ln.append(np.full(len(ms), len(x), np.int64))
        at += len(x)
    X = np.concatenate(flat).astype(np.float64)
    base, off, ln = np.concatenate(base), np.concatenate(off), np.concatenate(ln)
    Q = len(base)
    out = np.zeros((Q, 2), np.float32)
    ks = np.arange(DEC * J, dtype=np.int64)
    for q0 in range(0, Q, chunk):
        q1 = min(Q, q0 + chunk)
        idx = base[None, q0:q1] - ks[:, None]                  # [32 J, q]: the sample of tap k
        ok = (idx >= 0) & (idx < ln[None, q0:q1])
        W = X[np.where(ok, idx + off[None, q0:q1], 0)]         # (slot 0 of X is the zero outside a buffer)
        del idx, ok
        tot = np.zeros((2, q1 - q0), np.float32)
        for w in range(16):
            acc = np.zeros((2, q1 - q0), np.float64)           # (binary32 values, carried in binary64)
            for h in range(2):
                p = 2 * w + h
                for jj in range(J):
                    k = DEC * (J - 1 - jj) + p
                    gk = np.array([[gre[k]], [gim[k]]])
                    acc = _fma_core(gk * W[k][None, :], acc).astype(np.float64)
            tot = tot + acc.astype(np.float32)                 # binary32 add, wavefront order
        out[q0:q1] = tot.T
    res, at = [], 0
    for _, _, ms in items:
        res.append(out[at:at + len(ms)])
        at += len(ms)
    return res


def restate(taps32, D, x, x_origin, ms):
    return restate_many(taps32, D, [(x, x_origin, ms)])[0]


def convolve64(taps32, D, x, x_origin, ms):
    """the same outputs in binary64 (the same binary32 taps and samples; no claim about order) -> complex128"""
    g = np.asarray(taps32, np.complex64).astype(np.complex128)
    x = np.asarray(x, np.float64)
    ms = np.asarray(ms, np.int64)
    z = np.convolve(x, g)                                      # z[n] = sum_k g[k] x[n - k], n relative to x_origin
    n = DEC * ms + int(D) - int(x_origin)
    return np.where((n >= 0) & (n < len(z)), z[np.clip(n, 0, len(z) - 1)], 0.0)


def impulse_expect(taps32, D, nout, impulses, m_first=0):
    """isolated impulses (n0, a), each output meeting at most one: out[m] = (fl32(g.re[k] a), fl32(g.im[k] a)) with
    k = 32 m + D - n0 -- one rounding, every later fused multiply-add and add meets a zero -- and +0 elsewhere (a zero
    product of either sign added to the chain's +0 is +0)."""
    g = np.asarray(taps32, np.complex64)
    out = np.zeros((nout, 2), np.float32)
    hit = np.zeros(nout, bool)
    for n0, a in impulses:
        k = np.arange(len(g), dtype=np.int64)
        k = k[(k + int(n0) - int(D)) % DEC == 0]
        m = (k + int(n0) - int(D)) // DEC - int(m_first)
        sel = (m >= 0) & (m < nout)
        k, m = k[sel], m[sel]
        assert not hit[m].any(), "impulses closer than a window"
        hit[m] = True
        a64 = float(np.float32(a))
        out[m, 0] = (g.real[k].astype(np.float64) * a64).astype(np.float32) + np.float32(0)
        out[m, 1] = (g.imag[k].astype(np.float64) * a64).astype(np.float32) + np.float32(0)
    return out


# ---- what a wrong loader or tap image would compute ---------------------------------------------------------------
MUTATIONS = ("row0_column", "drop_first_256_taps", "drop_trailing_block", "drop_leading_block", "swap_phase_pairs")
TAP_DROPS = ("drop_first_256_taps", "drop_trailing_block", "drop_leading_block")


def mutate_taps(taps32, name):
    """The padded [32 J] tap array that restate / impulse_expect turn into the outputs of a kernel with one mistake:
      row0_column          row 0 of the staged input (tap phase 0) is read one column off: tap 32 j meets tap 32 (j + 1)'s sample
      drop_first_256_taps  taps k < 256 never reach the tap image
      drop_trailing_block  the last 8-tap block of every phase (jj >= J - 8: what the odd block count leaves behind the
                           two-blocks-per-trip loop) is not run.  jj descends in k, so these ARE the taps k < 256: the
                           same outputs as the mutation above, reached from the loop's side
      drop_leading_block   the first 8-tap block of every phase (jj < 8: the taps k >= 32 (J - 8)) is not run
      swap_phase_pairs     the tap images of phases 2w and 2w + 1 are exchanged"""
    gp, J = _padded(taps32)
    k = np.arange(DEC * J)
    jj = J - 1 - k // DEC
    if name == "row0_column":
        out = gp.copy()
        out[DEC::DEC] = gp[:-DEC:DEC]
        out[0] = 0
        return out
    if name == "drop_first_256_taps":
        return np.where(k < 256, 0, gp).astype(np.complex64)
    if name == "drop_trailing_block":
        return np.where(jj >= J - 8, 0, gp).astype(np.complex64)
    if name == "drop_leading_block":
        return np.where(jj < 8, 0, gp).astype(np.complex64)
    if name == "swap_phase_pairs":
        return gp[k ^ 1]
    raise KeyError(name)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def noise32(rng, n, sigma=1.0):
    """unit white noise in binary32 with |x| >= 2^-15 or 0"""
    x = (rng.standard_normal(n) * sigma).astype(np.float32)
    x[np.abs(x) < 2.0 ** -15] = 0.0
    return x


def noise16(rng, shape, sigma=6000.0):
    """int16 white noise that reaches both ends of the range"""
    x = np.clip(np.rint(rng.standard_normal(shape) * sigma), -32768, 32767).astype(np.int16)
    f = x.reshape(-1)
    f[len(f) // 3] = -32768
    f[(2 * len(f)) // 3] = 32767
    return x


def s16_to_f32(x):
    """k0_sample: s / 32768, exact"""
    return x.astype(np.float32) / np.float32(32768)


# ---- 4a: impulse trains through the batch call -------------------------------------------------------------------
IMP_NIN = 250003
IMP_STEP = 7040          # a multiple of 32; neighbours are >= 7040 - 31 >= 32 (216 + 2) apart


def impulse_trains():
    """-> (audio [3, IMP_NIN] float32, per record a list of (n0, amplitude)).  A grid of impulses whose positions step
    through the residues mod 32, with the edge positions put in and the grid points they crowd taken out."""
    rng = np.random.default_rng(4001)
    special = {0: [IMP_NIN - 1], 1: [16384 - 1, 5 * 16384 + 1], 2: [16384 + 1, 7 * 16384 - 1]}
    gap = DEC * (216 + 2)
    x = np.zeros((3, IMP_NIN), np.float32)
    trains = []
    for r in range(3):
        pos = list(special[r])
        for i in range(35):
            n0 = IMP_STEP * i + (11 * r + i) % DEC
            if n0 < IMP_NIN and all(abs(n0 - s) >= gap for s in special[r]):
                pos.append(n0)
        pos.sort()
        assert all(b - a >= gap for a, b in zip(pos, pos[1:]))
        amp = (rng.uniform(0.5, 2.0, len(pos)) * rng.choice([-1.0, 1.0], len(pos))).astype(np.float32)
        frac = np.frexp(amp)[0]
        amp[np.abs(frac) == 0.5] *= np.float32(1.25)           # no powers of two
        x[r, pos] = amp
        trains.append(list(zip(pos, amp)))
    return x, trains


_cache = {}


def impulse_case(mode, taps32, D):
    """-> (audio [3, IMP_NIN], expectation [3, 45000, 2]) for the taps of `mode` (built once)"""
    key = ("imp", mode)
    if key not in _cache:
        x, trains = impulse_trains()
        _cache[key] = (x, np.stack([impulse_expect(taps32, D, NOUT_BATCH, t) for t in trains]))
    return _cache[key]


# ---- 4b: dense noise through the batch call ------------------------------------------------------------------------
DENSE_NIN = 32 * 1100 + 5


def dense_outputs(nt, D):
    """the outputs of the dense record that reach an edge: the window starts before the record, a workgroup seam, the
    second one, the window runs off the end up to the first output past the last tap, and 64 behind it (all +0)"""
    past = (DENSE_NIN - 1 + nt - 1 - D) // DEC + 1             # first m with 32 m + D - (nt - 1) > nin - 1
    ms = np.concatenate([np.arange(0, 40), np.arange(470, 561), np.arange(1016, 1033), np.arange(1090, past + 1),
                         np.arange(past + 1, past + 65)])
    return ms, past


def dense_audio():
    return noise32(np.random.default_rng(4002), DENSE_NIN)


def dense_case(mode, taps32, D):
    """-> (audio [DENSE_NIN], output indices, expectation [len, 2], first output past the last tap); built once"""
    key = ("dense", mode)
    if key not in _cache:
        x = dense_audio()
        ms, past = dense_outputs(len(taps32), D)
        _cache[key] = (x, ms, restate(taps32, D, x, 0, ms), past)
    return _cache[key]
