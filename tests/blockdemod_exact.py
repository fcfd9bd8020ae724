"""Block demodulation (K10, uwspr_blockdemod_batch) without a GPU: the definition of include/uwspr_hip.h restated in
binary64 (block_restate, written from the header's text, not from the kernel), the same definition with every product
and sum rounded to binary32 (emulate32: what binary32 alone costs), named misreadings of the text (mutate=), and the
frames and items that tests/test_blockdemod.py and tests/test_gpu_blockdemod_edges.py share (edge_frames, edge_items).

The NaN rule, stated once: if any P(d) of a block is NaN, soft of every symbol of that block is NaN -- so fac is NaN
and all 162 bytes of that block length are 128.  Every maximum here propagates NaN (numpy's max and maximum do;
Python's max returns a NaN or not depending on the order of its arguments).  An infinite sample makes P infinite or
NaN, soft infinite or NaN, fac NaN: 128 again."""
import itertools

import numpy as np

DF = 375.0 / 256.0
NSYM, NP, HOP = 162, 45000, 3375
FULL = NSYM * 256                 # 41472 samples of a transmission
LAST = NP - FULL + 300            # a shift with which the last symbols run off the end
FL_LONG = 48000                   # the builders' frame length: 3000 samples the sample bound hides

MUTATIONS = ("n_ge_0", "n_le_np", "np_is_fl", "slope_162", "drift_not_halved", "phasor_from_1", "phasor_not_restarted",
             "theta_no_pi", "theta_next", "psi_own", "psi_plus", "tone_2pr3_d", "spacing_512", "round", "clip_127", "mean_161")


def frame_offset(seed):
    """the frequency offset text_frame draws for `seed` (its generator's first draw)"""
    return np.random.Generator(np.random.Philox(0x05D7E87 + seed)).uniform(-6.0, 6.0)


def clean_frame(G, text, seed, off=None, drift=0.0):
    """text_frame's signal without its noise (off: another frequency offset than the seed's; drift: the item model's
    (drift / 2)(i - 81) / 81 per symbol on top of it)"""
    sym = G.wspr_symbols(text).astype(np.float64)
    off = frame_offset(seed) if off is None else off
    fi = off + (drift / 2.0) * (np.arange(NSYM) - 81.0) / 81.0
    phase = 2.0 * np.pi * np.cumsum(np.repeat((sym - 1.5) * DF + fi, 256)) / 375.0
    sig = np.zeros((NP, 2), np.float64)
    sig[375:375 + NSYM * 256, 0] = np.cos(phase)
    sig[375:375 + NSYM * 256, 1] = np.sin(phase)
    return sig.astype(np.float32)


def _samples(frame, shift, np_points, mutate):
    """x[s + 256 i + k] as [162, 256] complex128, 0 where the index is not in 0 < n < np_points or behind the buffer"""
    x = frame[:, 0].astype(np.float64) + 1j * frame[:, 1].astype(np.float64)
    if mutate == "np_is_fl":
        np_points = len(x)
    n = int(shift) + 256 * np.arange(NSYM)[:, None] + np.arange(256)[None, :]
    ok = (n > 0) & (n < np_points)
    if mutate == "n_ge_0":
        ok = (n >= 0) & (n < np_points)
    if mutate == "n_le_np":
        ok = (n > 0) & (n <= np_points)
    ok &= n < len(x)
    return np.where(ok, x[np.clip(n, 0, len(x) - 1)], 0.0)


def _freqs(f, drift, mutate, i):
    half = float(np.float32(drift)) if mutate == "drift_not_halved" else float(np.float32(drift)) / 2.0
    return float(np.float32(f)) + half * (i - 81) / (162.0 if mutate == "slope_162" else 81.0)


def _sample_index(mutate):
    """the k of the phasor e^{-j 2 pi f k / 375}, [162, 256] by broadcasting"""
    i, k = np.arange(NSYM), np.arange(256)
    if mutate == "phasor_from_1":
        return k[None, :] + 1
    if mutate == "phasor_not_restarted":
        return 256 * i[:, None] + k[None, :]
    return k[None, :]


def _theta(f, drift, mutate):
    i = np.arange(NSYM)
    fi = _freqs(f, drift, mutate, i + 1 if mutate == "theta_next" else i)
    return 2.0 * np.pi * fi * 256.0 / 375.0 + (0.0 if mutate == "theta_no_pi" else np.pi)


def _quantise(soft, mutate=None):
    """mode 2's normalisation in binary64 -> 162 bytes; all 128 when fac is not a positive finite number"""
    out = np.full(NSYM, 128, np.uint8)
    s = soft[:161] if mutate == "mean_161" else soft
    fsum, f2sum = s.mean(), (s * s).mean()
    with np.errstate(invalid="ignore"):
        fac = np.sqrt(f2sum - fsum * fsum)
    if np.isfinite(fac) and fac > 0:
        v = np.clip(50.0 * soft / fac, -127.0 if mutate == "clip_127" else -128.0, 127.0) + 128.0
        out[:] = (np.rint(v) if mutate == "round" else np.trunc(v)).astype(np.uint8)
    return out


def block_restate(frame, shift, f, drift, pr3, np_points=NP, mutate=None):
    """include/uwspr_hip.h, "block demodulation", in binary64 -> [3, 162] uint8 (block lengths 1, 2, 3).  frame: [fl, 2],
    fl >= np_points or not -- a sample at n >= np_points, or behind the buffer, counts as 0.  mutate: one of MUTATIONS,
    a misreading of the text."""
    assert mutate is None or mutate in MUTATIONS, mutate
    i = np.arange(NSYM)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = _samples(frame, shift, np_points, mutate)
        fi = _freqs(f, drift, mutate, i)
        kk = _sample_index(mutate)
        df = 375.0 / 512.0 if mutate == "spacing_512" else DF
        z = np.empty((NSYM, 4), np.complex128)
        for j in range(4):
            z[:, j] = (xs * np.exp(-2j * np.pi * (fi[:, None] + (j - 1.5) * df) * kk / 375.0)).sum(axis=1)
        theta = _theta(f, drift, mutate)
        sign = 1j if mutate == "psi_plus" else -1j
        pr3 = np.asarray(pr3).astype(np.int64)
        out = np.full((3, NSYM), 128, np.uint8)
        for nb in (1, 2, 3):
            i0 = nb * np.arange(NSYM // nb)   # the blocks' first symbols
            term = []   # term[m][d]: z_{i0+m}[pr3[i0+m] + 2 d] e^{-j psi_m}, psi_m = theta_{i0} + .. + theta_{i0+m-1}
            for m in range(nb):
                psi = theta[i0[:, None] + np.arange(m + 1 if mutate == "psi_own" else m)[None, :]].sum(axis=1)
                tone = (lambda d: 2 * pr3[i0 + m] + d) if mutate == "tone_2pr3_d" else (lambda d: pr3[i0 + m] + 2 * d)
                term.append([z[i0 + m, tone(d)] * np.exp(sign * psi) for d in (0, 1)])
            best = np.full((nb, 2, len(i0)), -np.inf)
            for d in itertools.product((0, 1), repeat=nb):
                P = np.abs(sum(term[m][d[m]] for m in range(nb)))
                for m in range(nb):   # np.maximum propagates a NaN, whichever P holds it
                    best[m, d[m]] = np.maximum(best[m, d[m]], P)
            soft = np.zeros(NSYM)
            for m in range(nb):
                soft[i0 + m] = best[m, 1] - best[m, 0]
            out[nb - 1] = _quantise(soft, mutate)
    return out


def emulate32(frame, shift, f, drift, pr3, np_points=NP):
    """The same definition with every product and sum rounded to binary32, in the definition's order: sample times
    phasor as four products, a difference and a sum; the 256 terms of a z added with k ascending, each tone on its own;
    the terms of a P added with m ascending; |.| as sqrt(re re + im im); the means as running sums.  Every phase is taken
    in binary64 and its cosine and sine rounded once.  No fused multiply-add, no recurrence: it bounds what binary32
    costs the bytes, it does not predict the kernel's bits.  Finite input only.  -> [3, 162] uint8"""
    f32 = np.float32
    i, k = np.arange(NSYM), np.arange(256)
    xs = _samples(frame, shift, np_points, None)
    xr, xi = xs.real.astype(f32), xs.imag.astype(f32)
    fi = _freqs(f, drift, None, i)
    zr, zi = np.empty((NSYM, 4), f32), np.empty((NSYM, 4), f32)
    for j in range(4):
        ph = -2.0 * np.pi * (fi[:, None] + (j - 1.5) * DF) * k[None, :] / 375.0
        c, s = np.cos(ph).astype(f32), np.sin(ph).astype(f32)
        zr[:, j] = np.add.accumulate(xr * c - xi * s, axis=1, dtype=f32)[:, -1]
        zi[:, j] = np.add.accumulate(xr * s + xi * c, axis=1, dtype=f32)[:, -1]
    theta = _theta(f, drift, None)
    pr3 = np.asarray(pr3).astype(np.int64)
    out = np.full((3, NSYM), 128, np.uint8)
    for nb in (1, 2, 3):
        i0 = nb * np.arange(NSYM // nb)
        term = []   # term[m][d]: z_{i0+m}[pr3 + 2 d] e^{-j psi_m}, (re, im)
        for m in range(nb):
            psi = np.zeros(len(i0)) if m == 0 else theta[i0[:, None] + np.arange(m)[None, :]].sum(axis=1)
            c, s = np.cos(-psi).astype(f32), np.sin(-psi).astype(f32)
            term.append([])
            for d in (0, 1):
                ar, ai = zr[i0 + m, pr3[i0 + m] + 2 * d], zi[i0 + m, pr3[i0 + m] + 2 * d]
                term[m].append((ar * c - ai * s, ar * s + ai * c))
        best = np.full((nb, 2, len(i0)), -np.inf, f32)
        for d in itertools.product((0, 1), repeat=nb):
            re, im = term[0][d[0]]
            for m in range(1, nb):
                re, im = re + term[m][d[m]][0], im + term[m][d[m]][1]
            P = np.sqrt(re * re + im * im)
            for m in range(nb):
                best[m, d[m]] = np.maximum(best[m, d[m]], P)
        soft = np.empty(NSYM, f32)
        for m in range(nb):
            soft[i0 + m] = best[m, 1] - best[m, 0]
        fsum = np.add.accumulate(soft, dtype=f32)[-1] / f32(162)
        f2sum = np.add.accumulate(soft * soft, dtype=f32)[-1] / f32(162)
        with np.errstate(invalid="ignore"):
            fac = np.sqrt(f2sum - fsum * fsum)
        assert fac.dtype == f32 and soft.dtype == f32
        if np.isfinite(fac) and fac > 0:
            out[nb - 1] = np.trunc(np.clip(f32(50) * soft / fac, f32(-128), f32(127)) + f32(128)).astype(np.uint8)
    return out


def slm_at_zero(c, cf=1500.0):
    """slmFrequencyDrift (lib/slm.cc:36-73) at t = 0 for a NONLINEAR candidate record, as the fine search adds it to f0"""
    v1, v2, q1, q2 = float(c["V1"]), float(c["V2"]), float(c["p1"]), float(c["p2"])
    den = np.sqrt(q1 * q1 + q2 * q2)
    if den == 0:
        return np.float32(0.0)
    sign = 1.0 if (q1 * v1 + q2 * v2) > 0 else -1.0
    return np.float32(-sign * abs(v1 * q1 + v2 * q2) / den * cf / 1500.0)


def close_figures(got, want):
    """(bytes that differ, bytes, largest difference): what the GPU criterion is stated in"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int((d > 0).sum()), d.size, int(d.max())


def meets_criterion(got, want, share=0.01):
    """the GPU tests' criterion: every byte within 1, at most `share` of the bytes different"""
    ndiff, size, largest = close_figures(got, want)
    return largest <= 1 and ndiff <= share * size


# ------------------------------------------------------------------ frames
TEXT, SNR_DB = "K1ABC FN42 37", -24.0
SEEDS = [11, 12, 13]          # the noisy frames of tests/test_gpu_blockdemod.py; CLEAN_SEED's frame is noise-free
CLEAN_SEED = 14
SPIKE_SEED, NOISE_SEED, LOUD_SEED = 0xB10C0001, 0xB10C0002, 15
DRIFT_SEEDS = {2.0: 16, -2.0: 17, -40.0: 18}
SPIKES = {0: (37.0, -41.0), NP - 1: (-48.0, 33.0), NP: (44.0, 39.0)}   # sample: (I, Q), 30 .. 50 sigma each


def text_frame(G, text, seed, snr_db):
    from test_gpu_osd_pipe import text_frame as model
    return model(G, text, seed, snr_db)


def noise_frame(seed, n=FL_LONG, sigma=1.0):
    """complex white noise alone"""
    return (sigma * np.random.Generator(np.random.Philox(seed)).standard_normal((n, 2))).astype(np.float32)


def spike_frame(seed=SPIKE_SEED):
    """noise of sigma = 1, 48 000 samples, with single samples of 30 .. 50 sigma where the sample bound 0 < n < 45000 ends:
    n = 0 (excluded), n = 44 999 (the last one counted) and n = 45 000 (excluded, present when fl > 45 000)"""
    fr = noise_frame(seed)
    for n, v in SPIKES.items():
        fr[n] = v
    return fr


def loud_symbols(G, text):
    """five symbols of `text`, seven or more apart, two with data bit 1 and three with data bit 0"""
    bit = G.wspr_symbols(text) >> 1
    pick, need = [], {1: 2, 0: 3}
    for i in range(5, NSYM, 7):
        if need[int(bit[i])]:
            need[int(bit[i])] -= 1
            pick.append(i)
    assert len(pick) == 5
    return pick


def loud_symbols_frame(G, text, seed=LOUD_SEED):
    """clean_frame with five symbols at 8 x the amplitude: their soft values are 8 x the others', and 50 soft / fac
    leaves [-128, 127] on both sides, so bytes 0 and 255 occur"""
    fr = clean_frame(G, text, seed)
    for i in loud_symbols(G, text):
        fr[375 + 256 * i:375 + 256 * (i + 1)] *= np.float32(8.0)
    return fr


def _long(fr, seed=None, sigma=0.0):
    """a 45 000-sample frame continued to 48 000 with noise of its own level (or zeros)"""
    tail = noise_frame(seed, FL_LONG - len(fr), sigma) if seed is not None else np.zeros((FL_LONG - len(fr), 2), np.float32)
    return np.concatenate([fr, tail])


_frames_made = {}


def edge_frames(G, fl=FL_LONG):
    """the frames edge_items() names, [10, fl, 2] float32: 0 .. 2 text_frame at -24 dB, 3 noise-free, 4 the spike frame,
    5 noise alone, 6 .. 8 noisy signals drifting by +2, -2 and -40 Hz, 9 the loud symbols.  Built at 48 000 samples
    (the text frames continued with noise of their level, the noise-free ones with zeros) and cut to fl."""
    if "long" not in _frames_made:
        sigma = G.synth.sigma_for_snr(SNR_DB)
        fr = [_long(text_frame(G, TEXT, s, SNR_DB), 0xB10C1000 + s, sigma) for s in SEEDS]
        fr.append(_long(clean_frame(G, TEXT, CLEAN_SEED)))
        fr += [spike_frame(), noise_frame(NOISE_SEED)]
        for drift, s in DRIFT_SEEDS.items():
            sig = clean_frame(G, TEXT, s, drift=drift).astype(np.float64) + noise_frame(0xB10C2000 + s, NP, sigma)
            fr.append(_long(sig.astype(np.float32), 0xB10C3000 + s, sigma))
        fr.append(_long(loud_symbols_frame(G, TEXT)))
        _frames_made["long"] = np.stack(fr)
        _frames_made["long"].setflags(write=False)
    return np.ascontiguousarray(_frames_made["long"][:, :fl])


ALIGN_BASE = [-20, -7, 6, 19, 32, 45, 58, 71, 84, 97, 110, 123, 136, 149, 221, 230]   # x 16 + r: the last two run off


def edge_items():
    """One list for the CPU and the GPU tests, sorted by frame; "name" is what assertions call an item by.  A window is
    n = shift .. shift + 41 471: it reads sample 0 when shift <= 0, and samples from 45 000 on when shift > 3528."""
    offs = [frame_offset(s) for s in SEEDS + [CLEAN_SEED]]
    end = NP - FULL   # 3528: the last sample of the window is n = 44 999
    items = [
        {"name": "nominal", "frame": 0, "shift": 375, "f": offs[0], "drift": 0.0},
        {"name": "second in its frame", "frame": 0, "shift": 371, "f": offs[0] + 0.3, "drift": 2.0},
        {"name": "leading samples missing", "frame": 1, "shift": -200, "f": offs[1], "drift": -2.0},
        {"name": "runs off the end", "frame": 2, "shift": LAST, "f": offs[2], "drift": 0.0},
        {"name": "noise-free", "frame": 3, "shift": 375, "f": offs[3], "drift": 0.0},
        {"name": "spike, shift 0", "frame": 4, "shift": 0, "f": 0.7, "drift": 0.0},         # n = 0 is k = 0 of symbol 0
        {"name": "spike, shift -255", "frame": 4, "shift": -255, "f": 0.7, "drift": 0.0},   # n = 0 is k = 255 of symbol 0
        {"name": "spike, shift 1", "frame": 4, "shift": 1, "f": 0.7, "drift": 0.0},         # n = 0 is just ahead of the window
        {"name": "spike, last sample 44999", "frame": 4, "shift": end, "f": -0.4, "drift": 0.0},
        {"name": "spike, last sample 45000", "frame": 4, "shift": end + 1, "f": -0.4, "drift": 0.0},   # k = 255 of symbol 161
        {"name": "spike, last sample 44998", "frame": 4, "shift": end - 1, "f": -0.4, "drift": 0.0},
    ]
    for r, q in enumerate(ALIGN_BASE):
        items.append({"name": "alignment %d" % r, "frame": 5, "shift": 16 * q + r, "f": 0.25 * r - 2.0, "drift": 0.0})
    for b, (drift, s) in enumerate(DRIFT_SEEDS.items()):
        items.append({"name": "drift %+g" % drift, "frame": 6 + b, "shift": 375, "f": frame_offset(s), "drift": drift})
    items.append({"name": "loud symbols", "frame": 9, "shift": 375, "f": frame_offset(LOUD_SEED), "drift": 0.0})
    return items


EDGE_NAMES = [it["name"] for it in edge_items()]


def reads_from_45000_on(item):
    return item["shift"] + FULL > NP


_restated = {}


def edge_want(G, np_points=NP):
    """block_restate of every item of edge_items() on the 48 000-sample frames, [items, 3, 162]; computed once"""
    if np_points not in _restated:
        fr = edge_frames(G)
        _restated[np_points] = np.stack([block_restate(fr[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3, np_points)
                                         for it in edge_items()])
        _restated[np_points].setflags(write=False)
    return _restated[np_points]


# ------------------------------------------------------------------ NaN and infinities
SPECIAL_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
# where the one special sample goes (in I; Q stays noise), for items at shift 375: (sample, items that read it, items that do not)
SPECIAL_PLACES = {
    "symbol 0": (375 + 100, [(375, 0.5, 0.0), (-200, -1.0, 2.0)], [(476, 0.5, 0.0)]),
    "middle of a block of 3": (375 + 256 * 82 + 7, [(375, 0.5, 0.0), (3528, 1.5, -2.0)], [(375 + 256 * 82 + 8, 0.5, 0.0), (7 - 256 * 80, 0.5, 2.0)]),
    "symbol 161": (375 + 256 * 161 + 200, [(375, 0.5, 0.0)], [(375 + 256 * 161 + 200 - FULL, 0.5, 0.0), (-300, 0.5, 0.0)]),
}


def special_frame(clean, place, value):
    """`clean` with the I of one sample replaced"""
    fr = np.array(clean, np.float32)
    fr[SPECIAL_PLACES[place][0], 0] = SPECIAL_VALUES[value]
    return fr


def special_items(place, frame):
    """-> (items whose windows include the place's sample, items whose windows do not), all in `frame`"""
    n, hit, miss = SPECIAL_PLACES[place]
    assert all(s <= n < s + FULL for s, _, _ in hit) and not any(s <= n < s + FULL for s, _, _ in miss)
    mk = lambda t: {"frame": frame, "shift": t[0], "f": t[1], "drift": t[2]}
    return [mk(t) for t in hit], [mk(t) for t in miss]
