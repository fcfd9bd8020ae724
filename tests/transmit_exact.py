"""TEST INFRASTRUCTURE ONLY -- K7 (gr-uwspr_amd/csrc/k7_transmit.hip) restated to the bit, in numpy, no GPU needed.

Everything in K7 but sincos (the baseband), logf and cospif (the noise) is exact binary32 arithmetic in a fixed order, and
the library is built with -ffp-contract=off.  So, GIVEN the device's own baseband and the device's own Gaussian draws,
every audio sample can be stated to the byte:

  chain          k7_render's filter sum of one output, in k7_block's order
  philox4x32_10  the counter-based generator; gauss_inputs: the two uniforms tx_gauss hands to Box-Muller, as binary32
  gauss_ref      Box-Muller in binary64 (what the device's logf / cospif are measured against)
  compose        chain + sigma noise + gain background, the kernel's separate roundings
  quantise       tx_s16
  MUTATIONS      the kernel mistakes the byte comparison must be able to see, as changed expectations

and the case (signals, windows) that the CPU mutation tests and the GPU tests share."""
import numpy as np

from frontend_exact import fma32

DEC = 32
NT = 3179               # composite taps
T = 104                 # taps per output phase (K7_T)
NTX = 162 * 256         # baseband samples per transmission
TILE = 16384            # audio samples per workgroup (K7_OUT)
MASK32 = np.uint64(0xFFFFFFFF)


# ---- the filter sum -------------------------------------------------------------------------------------------------
def window(t0, nframes):
    """the baseband samples [j0, j0 + nbb) that audio [t0, t0 + nframes) reads: x[m - 103 .. m], m = n div 32"""
    j0 = int(t0) // DEC - (T - 1)
    return j0, (int(t0) + int(nframes) - 1) // DEC - j0 + 1


def file_orientation(iq):
    """uwspr_tx_baseband's output [n, 2] -> (re, im) of the channel's baseband as the .c2 file holds it and as
    k7_render stages it: the conjugate (k7_baseband negates Q; negating again is exact and restores the kernel's value)"""
    iq = np.asarray(iq)
    assert iq.dtype == np.float32 and iq.ndim == 2 and iq.shape[1] == 2
    return iq[:, 0].copy(), -iq[:, 1]


def chain(image, x, n, x0=0, mutation=None):
    """Audio outputs n (absolute indices, an int64 array) of k7_render before noise, background and quantiser, as float32.

    image: the tap image [32, 104, 2] = (Re g, -Im g)[p + 32 i] at [p, i]; x = (re, im): the channel's baseband samples
    [x0, x0 + len) in the file orientation (file_orientation), binary32.

    Read from the kernel: wavefront w runs output phases p = 2w and 2w + 1; a lane's acc[r] (baseband step m, output
    n = 32 m + p) starts at +0.0f and goes through thirteen k7_block calls, tap blocks t = 0 .. 12 in that order; inside a
    block u = 0 .. 7 ascending, and for tap i = 8 t + u
        acc = fmaf(image[p][i].re, x[m - i].re, acc);   acc = fmaf(image[p][i].im, x[m - i].im, acc);
    (S[8 + r - u] is x[m + r - u]).  So ONE chain of 208 fused multiply-adds from +0, i = 0 .. 103 ascending, real part
    before imaginary.  Nothing depends on where the output falls in a workgroup or a launch.

    mutation: None, or one of MUTATIONS -- what a kernel with that one mistake would give."""
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape == (DEC, T, 2)
    xr, xi = (np.asarray(v) for v in x)
    assert xr.dtype == np.float32 and xi.dtype == np.float32 and xr.shape == xi.shape and xr.ndim == 1
    n = np.asarray(n, np.int64).reshape(-1)
    shift, order, imag_first = 0, range(T), False
    if mutation is not None:
        image, shift, order, imag_first = _mutate(image, mutation)
    p = n % DEC
    base = n // DEC - int(x0) - shift                          # index into x of tap 0's sample
    assert len(n) == 0 or (base.min() - (T - 1) >= 0 and base.max() < len(xr)), "the baseband does not cover the window"
    acc = np.zeros(len(n), np.float32)
    for i in order:
        k = base - i
        if imag_first:
            acc = fma32(image[p, i, 1], xi[k], acc)
            acc = fma32(image[p, i, 0], xr[k], acc)
        else:
            acc = fma32(image[p, i, 0], xr[k], acc)
            acc = fma32(image[p, i, 1], xi[k], acc)
    return acc


def chain64(image, x, n, x0=0):
    """the same sum of the same binary32 taps and samples in binary64 (no claim about order), and sum_i |g| |x|"""
    image = np.asarray(image, np.float64)
    xr, xi = (np.asarray(v, np.float64) for v in x)
    n = np.asarray(n, np.int64).reshape(-1)
    p = n % DEC
    base = n // DEC - int(x0)
    tot, mag = np.zeros(len(n)), np.zeros(len(n))
    for i in range(T):
        a, b = image[p, i, 0] * xr[base - i], image[p, i, 1] * xi[base - i]
        tot += a + b
        mag += np.abs(a) + np.abs(b)
    return tot, mag


MUTATIONS = ("drop_last_block", "drop_first_block", "swap_phase_pairs", "window_off_by_one", "imag_before_real",
             "drop_one_small_tap", "taps_descending")


def small_tap(image):
    """(p, i) of the tap the drop_one_small_tap mutation loses: of the taps with 0 < |g| < 2e-6 -- the ones a bound of
    2e-6 on the audio cannot see -- the one nearest 1e-6"""
    mag = np.hypot(image[:, :, 0].astype(np.float64), image[:, :, 1].astype(np.float64))
    ok = (mag > 0) & (mag < 2e-6)
    cost = np.where(ok, np.abs(mag - 1e-6), np.inf)
    p, i = np.unravel_index(int(np.argmin(cost)), cost.shape)
    return int(p), int(i)


def _mutate(image, name):
    """-> (image, window shift, tap order, imaginary first) of a kernel with one mistake:
      drop_last_block     the last 8-tap block of every phase (what an odd block count leaves behind a two-blocks-per-trip
                          loop) is not run
      drop_first_block    the block ahead of the loop is not run
      swap_phase_pairs    the tap images of phases 2w and 2w + 1 are exchanged
      window_off_by_one   the staged window sits one baseband sample early: tap i meets x[m - i - 1]
      imag_before_real    the two fused multiply-adds of a tap in the other order
      drop_one_small_tap  one tap under 2e-6 (small_tap) never reaches the image
      taps_descending     the chain runs i = 103 .. 0"""
    img = image.copy()
    shift, order, imag_first = 0, range(T), False
    if name == "drop_last_block":
        img[:, T - 8:] = 0
    elif name == "drop_first_block":
        img[:, :8] = 0
    elif name == "swap_phase_pairs":
        img = img[np.arange(DEC) ^ 1]
    elif name == "window_off_by_one":
        shift = 1
    elif name == "imag_before_real":
        imag_first = True
    elif name == "drop_one_small_tap":
        p, i = small_tap(image)
        img[p, i] = 0
    elif name == "taps_descending":
        order = range(T - 1, -1, -1)
    else:
        raise KeyError(name)
    return img, shift, order, imag_first


# ---- the noise ------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter [..., 4], key [..., 2], 32-bit words carried in uint64
    lanes -> [..., 4] uint64 (each < 2^32)"""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                              # (32 x 32 bits: exact in 64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def philox4x32_10_int(counter, key):
    """the same on plain Python integers (one counter, one key) -> a 4-tuple"""
    c0, c1, c2, c3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    m = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def uniforms(r0, r1):
    """tx_gauss's u1, u2 from words 0 and 1, formed in binary32 as the kernel forms them: u1 = ((float)(r0 >> 8) + 0.5f)
    2^-24, in (0, 1] -- from 2^23 on the + 0.5f is a tie and rounds to even, so 2^24 - 1 gives exactly 1 --, and
    u2 = (float)(r1 >> 8) 2^-24, in [0, 1)"""
    a = (np.asarray(r0, np.uint64) >> np.uint64(8)).astype(np.float32)          # (< 2^24: exact)
    b = (np.asarray(r1, np.uint64) >> np.uint64(8)).astype(np.float32)
    scale = np.float32(2.0 ** -24)
    u1 = (a + np.float32(0.5)) * scale
    u2 = b * scale
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def gauss_inputs(seed, ch, n):
    """(u1, u2) of the noise sample of (seed, channel, absolute audio index n): counter (n low, n high, channel, 0), key
    (seed low, seed high), words 0 and 1"""
    n = np.asarray(n, np.int64).reshape(-1).astype(np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    ctr = np.stack([n & MASK32, n >> np.uint64(32), np.full(len(n), int(ch), np.uint64), np.zeros(len(n), np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    r = philox4x32_10(ctr, key)
    return uniforms(r[..., 0], r[..., 1])


def gauss_radius(u1):
    """sqrt(-2 ln u1) in binary64"""
    return np.sqrt(-2.0 * np.log(np.asarray(u1, np.float32).astype(np.float64)))


def gauss_ref(u1, u2):
    """Box-Muller in binary64: sqrt(-2 ln u1) cos(2 pi u2)"""
    return gauss_radius(u1) * np.cos(2.0 * np.pi * np.asarray(u2, np.float32).astype(np.float64))


# ---- quantiser and composition ---------------------------------------------------------------------------------------
def quantise(v):
    """tx_s16: fl32(32767 v), clamped to [-32768, 32767], rint (halves to even), int16"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    q = np.float32(32767.0) * v
    assert q.dtype == np.float32
    q = np.minimum(np.maximum(q, np.float32(-32768.0)), np.float32(32767.0))
    return np.rint(q).astype(np.int16)


def exact_halves():
    """b_k = fl32((k + 0.5) / 32767), k = -32768 .. 32767: fl32(32767 b_k) is k + 0.5 exactly, for every k"""
    k = np.arange(-32768, 32768, dtype=np.float64)
    return k, ((k + 0.5) / 32767.0).astype(np.float32)


def background_index(n, length):
    """n mod length for absolute audio indices n, in Python integers"""
    return np.fromiter((int(v) % int(length) for v in np.asarray(n).reshape(-1)), np.int64)


def compose(chain32, g32, sigma, bg, bg_gain, n):
    """k7_render's output sample n: fl32(fl32(chain32 + fl32(sigma32 g32)) + fl32(bg_gain b[n mod len])), each term
    present only when the kernel adds it (sigma32 > 0; a background given).  sigma32 = (float)sigma as the library casts
    the channel's double; an int16 background sample is fl32(s) 2^-15 (exact); separate roundings (-ffp-contract=off)."""
    v = np.asarray(chain32)
    assert v.dtype == np.float32
    sigma32 = np.float32(sigma)
    if sigma32 > 0:
        g32 = np.asarray(g32)
        assert g32.dtype == np.float32 and g32.shape == v.shape
        v = v + sigma32 * g32
    if bg is not None:
        bg = np.asarray(bg)
        assert bg.dtype in (np.int16, np.float32) and bg.ndim == 1
        b = bg[background_index(n, len(bg))]
        if b.dtype == np.int16:
            b = b.astype(np.float32) * np.float32(2.0 ** -15)
        v = v + np.float32(bg_gain) * b
    assert v.dtype == np.float32
    return v


# ---- the float64 model of the baseband ---------------------------------------------------------------------------------
def baseband_model(sigs, symbols, t0, n):
    """uwspr_tx_baseband's samples [t0, t0 + n) (gain e^{+j theta}), binary64: theta = phase0 + the exclusive sum of
    2 pi f[u] / 375, f[u] = f0 + (s - 1.5) 375/256 + drift (u - (N - 1) / 2) / (N - 1).  symbols: text -> 162 symbols."""
    y = np.zeros(int(n), np.complex128)
    u = np.arange(NTX, dtype=np.float64)
    for s in sigs:
        sym = np.asarray(symbols(s["text"]), np.float64)
        f = s.get("f0", 0.0) + (np.repeat(sym, 256) - 1.5) * 375.0 / 256 + s.get("drift", 0.0) * (u - (NTX - 1) / 2) / (NTX - 1)
        th = s.get("phase0", 0.0) + np.concatenate([[0.0], np.cumsum(2 * np.pi * f / 375.0)[:-1]])
        a = int(s["start"]) - int(t0)                          # index in y of the transmission's sample 0
        lo, hi = max(a, 0), min(a + NTX, int(n))
        if lo < hi:
            y[lo:hi] += s.get("gain", 1.0) * np.exp(1j * th[lo - a:hi - a])
    return y


# ---- the case the CPU mutation tests and the GPU tests share -------------------------------------------------------------
def dense_signals(start):
    """one channel, three overlapping transmissions, the first at baseband index `start`"""
    return [{"text": "K1ABC FN42 37", "start": int(start), "f0": -150.0, "drift": -20.0, "gain": 0.3, "phase0": 1e3},
            {"text": "VE3EMB FN25 30", "start": int(start) + 317, "f0": 3.1, "drift": 0.0, "gain": 1.0, "phase0": -1e3},
            {"text": "PJ4/K1ABC 37", "start": int(start) + 2911, "f0": 120.0, "drift": 4.0, "gain": 1.7, "phase0": 0.4}]


DENSE_LAST = 2911       # the last signal's start behind the first's
WINDOW = 3 * TILE       # 49 152 frames
MIDDLE = 25000          # baseband samples from the first signal's start to the middle window (all three signals run there)


def dense_windows(start):
    """name -> (t0, nframes) around dense_signals(start): across the first signal's first audio sample, across the last
    one's last contribution, in the middle with t0 no multiple of 32, one frame, and one wholly before every signal
    (where a negative start leaves no room before the signals the windows begin at 0 or are left out)"""
    first = DEC * int(start)
    last = DEC * (int(start) + DENSE_LAST + NTX - 1) + NT - 1
    w = {"last": (last - 30001, WINDOW), "middle": (first + DEC * MIDDLE + 13, WINDOW), "one": (first + DEC * 30000 + 7, 1)}
    if first - 20005 >= 0:
        w["first"] = (first - 20005, WINDOW)
    else:
        w["first"] = (0, WINDOW)
    if first - 20005 - WINDOW - 3 >= 0:
        w["before"] = (first - 20005 - WINDOW - 3, WINDOW)
    return w


def start_for_middle(t0):
    """the `start` that puts the window (t0, WINDOW) where dense_windows' middle window lies: MIDDLE baseband samples
    into the first signal"""
    return int(t0) // DEC - MIDDLE
