"""TEST INFRASTRUCTURE ONLY -- K7's medium form (gr-uwspr_amd/csrc/k7_transmit.hip, template flag MEDIUM) restated in
numpy, no GPU needed, on top of tests/transmit_exact.py.  include/uwspr_hip.h ("Transmit through a medium") is the text.

Fading (binary64; the device's sincos is not bit-pinned, so the baseband is held to a bound, not to bytes):

  fade_design      uwspr_tx_fade_design: (a0, a1, omega [M], phi [M]) of a "fading" dict
  fade_gain        h(k) = a0 + a1 sum_m e^{j (omega_m k + phi_m)}
  faded_model      uwspr_tx_baseband_medium's samples: every signal (static, DOPPLER, DELAY) times its own h(j - start)

Impulses (exact: integers and binary32 in a fixed order, GIVEN the device's own Gaussian draws):

  impulse_thr      the event threshold, from the rate
  impulse_events   the events e of a channel whose bursts reach a window, as exact integers
  impulse_inputs   the two uniforms of burst sample (e, d), as binary32;  impulse_ref: Box-Muller on them in binary64
  impulse_terms    per d = 0 .. length - 1: which outputs of a window get an add, and from which event
  compose_medium   chain, + noise, + impulses in ascending d, + background: the kernel's separate roundings

  MUTATIONS        the kernel mistakes the comparisons must be able to see, as changed expectations
  and the case (signals, fades, windows, impulses) that the CPU mutation tests and the GPU tests share."""
import numpy as np

import transmit_exact as X

NTX = X.NTX
FS = 375.0
FADE_TAG = 0x46414445
MASK32 = X.MASK32

FADE_MUTATIONS = ("gain_conjugated", "gain_at_absolute_j", "scatter_not_normalised", "a0_dropped")
IMPULSE_MUTATIONS = ("event_stream_is_awgn_stream", "event_on_word_y", "burst_backwards", "thr_less_or_equal",
                     "impulses_before_awgn", "amplitude_blocks_all_on_2")
MUTATIONS = FADE_MUTATIONS + IMPULSE_MUTATIONS


# ---- fading -----------------------------------------------------------------------------------------------------------
def fade_design(fade):
    """uwspr_tx_fade_design in numpy's binary64: fade = {"spread", "shift": 0, "k": 0, "seed": 0, "paths": 16} ->
    (a0, a1, omega [M] rad per baseband sample, phi [M]).  Path m: words x, y, z of the Philox block with counter
    (m, 0, 0x46414445, 0), key (seed low, seed high)."""
    M = int(fade.get("paths", 16))
    K, spread, shift = float(fade.get("k", 0.0)), float(fade["spread"]), float(fade.get("shift", 0.0))
    seed = int(fade.get("seed", 0)) & (2 ** 64 - 1)
    om, ph = np.zeros(M), np.zeros(M)
    for m in range(M):
        x, y, z, _ = X.philox4x32_10_int((m, 0, FADE_TAG, 0), (seed & 0xFFFFFFFF, seed >> 32))
        u1 = ((x >> 8) + 0.5) / 2.0 ** 24
        u2 = (y >> 8) / 2.0 ** 24
        u3 = (z >> 8) / 2.0 ** 24
        nu = shift + ((spread / 2.0) * np.sqrt(-2.0 * np.log(u1))) * np.cos(2.0 * np.pi * u2)
        om[m] = 2.0 * np.pi * nu / FS
        ph[m] = 2.0 * np.pi * u3
    return float(np.sqrt(K / (K + 1.0))), float(np.sqrt(1.0 / ((K + 1.0) * M))), om, ph


def fade_gain(design, k, mutation=None):
    """h(k), complex128, for reception indices k (integers counted from the transmission's first sample)"""
    a0, a1, om, ph = design
    k = np.asarray(k, np.float64)
    s = np.zeros(k.shape, np.complex128)
    for m in range(len(om)):                                   # m ascending
        s = s + np.exp(1j * (om[m] * k + ph[m]))
    if mutation == "scatter_not_normalised":
        a1 = a1 * np.sqrt(len(om))
    if mutation == "a0_dropped":
        a0 = 0.0
    h = a0 + a1 * s
    return np.conj(h) if mutation == "gain_conjugated" else h


def max_gain(design):
    """the largest |h| possible: a0 + a1 M"""
    return design[0] + design[1] * len(design[2])


def _theta(s, symbols, kp):
    """theta at (fractional) transmission index kp: the per-symbol quadratic of include/uwspr_hip.h"""
    sym = np.asarray(symbols(s["text"]), np.float64)
    f0, drift, phase0 = s.get("f0", 0.0), s.get("drift", 0.0), s.get("phase0", 0.0)
    u = np.arange(NTX, dtype=np.float64)
    f = f0 + (np.repeat(sym, 256) - 1.5) * FS / 256 + drift * (u - (NTX - 1) / 2) / (NTX - 1)
    acc = phase0 + np.concatenate([[0.0], np.cumsum(2 * np.pi * f / FS)])
    q = np.clip(np.floor(kp / 256.0).astype(np.int64), 0, 161)
    r = kp - 256.0 * q
    wf, wd = 2 * np.pi * f0 / FS, 2 * np.pi * drift / ((NTX - 1) * FS)
    return acc[256 * q] + r * (2 * np.pi * (sym[q] - 1.5) / 256.0 + wf) + wd * (r * (256.0 * q - 0.5 * (NTX - 1)) + 0.5 * r * (r - 1.0))


def faded_model(sigs, symbols, t0, n, mutation=None):
    """uwspr_tx_baseband_medium's samples [t0, t0 + n) of the signals given (one channel), binary64 complex: signal by
    signal gain e^{+j [theta(k') - 2 pi fc D]} h(k), k = j - start, h = 1 without a "fading"; a "motion" as
    tests/test_gpu_tx_motion.py models it (relative delay: D = (R(t) - R(t_first)) / c; "absolute": D = R / c)."""
    y = np.zeros(int(n), np.complex128)
    j = int(t0) + np.arange(int(n), dtype=np.int64)
    for s in sigs:
        k = j - int(s["start"])
        kf = k.astype(np.float64)
        m = s.get("motion")
        D = np.zeros(len(k))
        kp = kf
        amp = np.full(len(k), float(s.get("gain", 1.0)))
        if m is not None and m.get("model", "doppler") != "static":
            (v1, v2), (p1, p2), tf = m.get("v", (0.0, 0.0)), m.get("p", (0.0, 0.0)), m.get("t", 0.0)
            t = tf + kf / FS
            R = np.hypot(v1 * t + p1, v2 * t + p2)
            r0 = np.hypot(v1 * tf + p1, v2 * tf + p2)
            D = (R - (0.0 if m.get("absolute", False) else r0)) / 1500.0
            if m.get("model", "doppler") == "delay":
                kp = kf - FS * D
            if m.get("spreading", False):
                amp = amp * r0 / R
        ok = (kp >= 0) & (kp < NTX)
        if not ok.any():
            continue
        z = amp[ok] * np.exp(1j * (_theta(s, symbols, kp[ok]) - 2 * np.pi * float(s.get("carrier", 1500)) * D[ok]))
        if s.get("fading") is not None:
            at = j[ok] if mutation == "gain_at_absolute_j" else k[ok]
            z = z * fade_gain(fade_design(s["fading"]), at, mutation)
        y[ok] += z
    return y


def faded_bound(sigs):
    """the bound the faded baseband is held to: 1e-6 (test_baseband_extremes_match_the_float64_model's, per unit gain) times
    gain times the largest |h| possible, summed over the signals"""
    return sum(1e-6 * abs(s.get("gain", 1.0)) * (max_gain(fade_design(s["fading"])) if s.get("fading") is not None else 1.0)
               for s in sigs)


# ---- impulses ---------------------------------------------------------------------------------------------------------
def impulse_thr(rate):
    """(uint32) min(floor(rate 2^32), 2^32 - 1), the product in binary64"""
    return int(min(np.floor(float(rate) * 4294967296.0), 4294967295.0))


def _blocks(seed, ch, e, word3):
    e = np.asarray(e, np.int64).reshape(-1).astype(np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    w3 = np.broadcast_to(np.asarray(word3, np.uint64), e.shape)
    ctr = np.stack([e & MASK32, e >> np.uint64(32), np.full(len(e), int(ch), np.uint64), w3], axis=-1)
    return X.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def is_event(imp, ch, e, mutation=None):
    """which of the audio indices e >= 0 are events of channel ch: word x of block (e, ch, 1) below thr"""
    thr = impulse_thr(imp["rate"]) if float(imp["sigma"]) > 0 else 0
    r = _blocks(imp.get("seed", 0), ch, e, 0 if mutation == "event_stream_is_awgn_stream" else 1)
    w = r[..., 1 if mutation == "event_on_word_y" else 0]
    return (w <= np.uint64(thr)) if mutation == "thr_less_or_equal" else (w < np.uint64(thr))


def impulse_events(imp, ch, t0, nframes, mutation=None):
    """the events e (exact integers, ascending) whose bursts can reach [t0, t0 + nframes): e >= 0,
    t0 - (length - 1) <= e < t0 + nframes (burst_backwards: t0 <= e < t0 + nframes + length - 1)"""
    L = int(imp.get("length", 1))
    lo, hi = max(int(t0) - (L - 1), 0), int(t0) + int(nframes)
    if mutation == "burst_backwards":
        lo, hi = int(t0), int(t0) + int(nframes) + L - 1
    e = np.arange(lo, hi, dtype=np.int64)
    return e[is_event(imp, ch, e, mutation)]


def impulse_inputs(imp, ch, e, d, mutation=None):
    """(u1, u2), binary32, of burst sample d of event e: words x, y of block (e, ch, 2 + d)"""
    r = _blocks(imp.get("seed", 0), ch, e, 2 if mutation == "amplitude_blocks_all_on_2" else 2 + int(d))
    return X.uniforms(r[..., 0], r[..., 1])


def impulse_ref(u1, u2):
    """Box-Muller in binary64 on the binary32 uniforms (what the device's logf / cospif are measured against)"""
    return X.gauss_ref(u1, u2)


def impulse_terms(imp, ch, t0, nframes, mutation=None):
    """[(d, off, e)] for d = 0 .. length - 1: outputs t0 + off (ascending int64 offsets into the window) get an add from
    event e = t0 + off - d (burst_backwards: e = t0 + off + d)"""
    ev = impulse_events(imp, ch, t0, nframes, mutation)
    out = []
    for d in range(int(imp.get("length", 1))):
        n = ev - d if mutation == "burst_backwards" else ev + d
        ok = (n >= int(t0)) & (n < int(t0) + int(nframes))
        out.append((d, (n[ok] - int(t0)).astype(np.int64), ev[ok]))
    return out


def impulse_support(imp, ch, t0, nframes, mutation=None):
    """how many adds every output of the window gets (int array [nframes])"""
    cnt = np.zeros(int(nframes), np.int64)
    for _, off, _ in impulse_terms(imp, ch, t0, nframes, mutation):
        cnt[off] += 1
    return cnt


def compose_medium(chain32, g32, sigma, terms, imp_sigma, draw, bg, bg_gain, n, mutation=None):
    """k7_render<MEDIUM>'s output samples n (the whole window, in order):
        v = chain;  v = fl32(v + fl32(sigma32 g32)) when sigma32 > 0;
        for d ascending: v = fl32(v + fl32(isigma32 draw(d, e))) where an event e = n - d exists;
        v = fl32(v + fl32(bg_gain b[n mod len])) with a background.
    terms: impulse_terms' list; draw(d, e) -> the Gaussian draws of burst samples (e, d) as float32 (the device's own, or
    impulse_ref's rounded); sigma32 = (float) sigma as the library casts the doubles."""
    v = np.asarray(chain32).copy()
    assert v.dtype == np.float32
    s32 = np.float32(imp_sigma)

    def add_impulses(v):
        for d, off, e in terms:
            if len(off):
                g = np.asarray(draw(d, e))
                assert g.dtype == np.float32 and g.shape == off.shape
                v[off] = v[off] + s32 * g
        return v
    if mutation == "impulses_before_awgn":
        v = add_impulses(v)
    v = X.compose(v, g32, sigma, None, 0.0, n)
    if mutation != "impulses_before_awgn":
        v = add_impulses(v.copy())
    v = X.compose(v, None, 0.0, bg, bg_gain, n)
    assert v.dtype == np.float32
    return v


def ref_draw(imp, ch, mutation=None):
    """draw(d, e) for compose_medium from impulse_ref, rounded to binary32 (CPU tests; the GPU tests pass the device's)"""
    return lambda d, e: impulse_ref(*impulse_inputs(imp, ch, e, d, mutation)).astype(np.float32)


# ---- the case the CPU mutation tests and the GPU tests share ----------------------------------------------------------------
RAYLEIGH = {"spread": 1.0, "shift": 0.3, "k": 0.0, "seed": 7, "paths": 16}
RICIAN = {"spread": 0.1, "shift": -0.2, "k": 10.0, "seed": 8, "paths": 5}
SHIFT_ONLY = {"spread": 2.0, "shift": 1.5, "k": 0.0, "seed": 9, "paths": 1}


def faded_signals(start):
    """one channel: a Rayleigh-faded and an unfaded transmission overlapping, then a Rician one"""
    return [{"text": "K1ABC FN42 37", "start": int(start), "f0": -150.0, "drift": -20.0, "gain": 0.3, "phase0": 1e3, "fading": RAYLEIGH},
            {"text": "VE3EMB FN25 30", "start": int(start) + 317, "f0": 3.1, "gain": 1.0, "phase0": -1e3},
            {"text": "PJ4/K1ABC 37", "start": int(start) + 2911, "f0": 120.0, "drift": 4.0, "gain": 1.7, "phase0": 0.4, "fading": RICIAN}]


def faded_windows(start):
    """name -> (t0, n) in baseband samples around faded_signals(start): k = 0 of the first signal, k = 41471 of the last,
    and one that begins mid-transmission"""
    return {"k0": (int(start) - 5, 600), "k_last": (int(start) + 2911 + NTX - 300, 600), "middle": (int(start) + 20011, 700)}


IMPULSE = {"rate": 1.0 / 250.0, "sigma": 0.5, "seed": 21, "length": 3}
IMPULSE_WINDOW = (5 * X.TILE - 1000, 2000)      # across a tile boundary (audio 81920)


def edge_impulse(imp=IMPULSE, ch=0, window=IMPULSE_WINDOW):
    """imp with the rate moved so that thr EQUALS word x of one index of the window (the smallest word there that still
    gives a rate <= 0.25; w / 2^32 is exact in binary64): that index is an event only to a kernel that compares with <=.
    -> (the impulse dict, the index)"""
    e = np.arange(window[0], window[0] + window[1], dtype=np.int64)
    w = _blocks(imp.get("seed", 0), ch, e, 1)[..., 0]
    near = np.abs(w.astype(np.int64) - impulse_thr(imp["rate"]))
    near[w > np.uint64(2 ** 30)] = 2 ** 40
    i = int(np.argmin(near))
    out = dict(imp, rate=float(int(w[i])) / 4294967296.0)
    assert impulse_thr(out["rate"]) == int(w[i])
    return out, int(e[i])
