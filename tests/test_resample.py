"""The rational resampler ahead of K0 (K11), without a GPU: the host design against its numpy restatement, the filter
it defines, the restated sums against a float64 convolution, impulse trains that pin every tap to one rounding, the
mutations the GPU tests must be able to see, and the ABI / WAV boundary.  (tests/resample_exact.py holds the
restatement; tests/test_gpu_resample.py holds the kernel to it byte for byte.)"""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

import resample_exact as X


# ---- 1. the design ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", X.RATES)
def test_design_equals_the_numpy_restatement(G, rate):
    taps, L, M, T, D = G.resample_design(rate)
    h, eL, eM, eT, eN, eD = X.design(rate)
    assert (L, M, T, len(taps), D) == (eL, eM, eT, eN, eD)
    assert L * rate == M * 12000 and L <= 160 and L * T <= 1920
    assert np.abs(taps - h[:eN]).max() <= 1e-12 * np.abs(h).max()
    assert abs(taps.sum() - L) <= 1e-9 * L


def test_design_ranges(G):
    ts = {r: G.resample_design(r)[3] for r in X.RATES}
    assert ts[11025] == 12 and ts[192000] == 173 and min(ts.values()) == 12 and max(ts.values()) == 173


@pytest.mark.parametrize("rate", [7999, 192001, 12345, 0])
def test_unsupported_rates_are_refused(G, rate):
    L = G.native.lib()
    assert L.uwspr_resample_design(rate, None, 0, None, None, None, None) < 0
    with pytest.raises(ValueError):
        G.resample_design(rate)
    assert not G.supported_rate(rate) and not X.supported(rate)


def test_12000_is_the_identity(G):
    taps, L, M, T, D = G.resample_design(12000)
    assert (list(taps), L, M, T, D) == ([1.0], 1, 1, 1, 0)


# ---- 2. the filter (conditions fixed in advance: the design as specified gives 2.2e-5 and -97.6 dB) ----------------
@pytest.mark.parametrize("rate", X.RATES)
def test_filter_quality(G, rate):
    taps, L, M, T, D = G.resample_design(rate)
    h32 = np.zeros(T * L)
    h32[:len(taps)] = taps
    h32 = h32.reshape(T, L).astype(np.float32).astype(np.float64).reshape(-1)[:len(taps)]     # the taps the kernel uses
    F = float(L) * rate
    fs = min(rate, 12000) - 2400.0
    k = np.arange(len(h32)) - D

    def resp(f):
        return np.abs(np.exp(-2j * np.pi * np.outer(f, k) / F) @ h32) / L

    dev = np.abs(resp(np.linspace(0.0, 2400.0, 241)) - 1.0).max()
    stop = resp(np.concatenate([np.linspace(fs, min(F / 2, fs + 20000.0), 2001), np.linspace(fs, F / 2, 2001)])).max()
    print("rate %d: pass-band deviation %.3g, stop band %.2f dB" % (rate, dev, 20 * np.log10(stop)))
    assert dev <= 1e-4
    assert 20 * np.log10(stop) <= -95.0


# ---- 3. the restatement against a float64 convolution ------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 11025, 44100, 48000, 192000])
def test_restatement_is_a_rounded_convolution(rate):
    hp, L, M, T, N, D = X.plan(rate)
    x = X.noise32(np.random.default_rng(7 + rate), 6000)
    js = np.arange(0, ((6000 + T) * L - D) // M + 3)
    got = X.restate(rate, x, 0, js).astype(np.float64)
    ref, mag = X.convolve64(rate, x, 0, js)
    # T fused multiply-adds, each one rounding of at most 2^-24 relative to a partial sum bounded by sum |hp x|
    assert (np.abs(got - ref) <= T * 2.0 ** -24 * mag + 1e-300).all()
    assert np.abs(got).max() > 0.1


# ---- 4. impulse trains ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", X.IMP_RATES)
def test_impulse_trains_pin_every_tap(rate):
    hp, L, M, T, N, D = X.plan(rate)
    x, exp, hit = X.impulse_case(rate)
    pos = np.flatnonzero(x)
    assert (np.diff(pos) >= T + 1).all()
    assert hit.shape == (L, T) and (hit >= 1).all(), "the train misses %d of the %d (p, t) pairs" % ((hit == 0).sum(), L * T)
    got = X.restate(rate, x, 0, np.arange(len(exp)))
    assert got.tobytes() == exp.tobytes()                     # the fma chain IS one rounding of one tap here
    # every meeting with a tap that is not zero (the padding N .. T L - 1 is) shows in the output
    assert (exp != 0).sum() == (hit * (hp != 0)).sum()


# ---- 5. mutations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", X.IMP_RATES)
@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_mutations_change_the_expectations(rate, mutation):
    hp, L, M, T, N, D = X.plan(rate)
    x, exp, _ = X.impulse_case(rate)
    got = X.restate(rate, x, 0, np.arange(len(exp)), mutation=mutation)
    if L == 1 and mutation in ("phases_swapped", "i0_rounded_up"):
        # one phase and an exact division: these two mistakes do not exist at L = 1 (48000 S/s); they are seen at the
        # other three rates
        assert got.tobytes() == exp.tobytes()
        return
    assert got.tobytes() != exp.tobytes()
    assert (got != exp).sum() >= 8


# ---- 6. the ABI and the WAV boundary ---------------------------------------------------------------------------------
def test_abi(G):
    N = G.native
    L = N.lib()
    hdr = open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read()
    for name in ("uwspr_resample_design", "uwspr_resample_batch"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in N.ABI_SYMBOLS and hasattr(L, name)
    assert "\"audio_rate\"" in hdr
    # the door is exported and bound, but not part of the header
    assert hasattr(L, "uwspr_debug_resample_launch") and "uwspr_debug_resample_launch" not in hdr
    assert hasattr(G.Context, "debug_resample_launch") and hasattr(G.Context, "resample")
    assert int(re.search(r"#define UWSPR_ABI_VERSION (\d+)", hdr).group(1)) == 6


def _write_wav(path, rate, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x, "<i2").tobytes())


def test_read_wav_any_rate(G, tmp_path):
    x = X.noise16(np.random.default_rng(5), (300, 2))
    for rate in (48000, 44100):
        p = tmp_path / ("r%d.wav" % rate)
        _write_wav(p, rate, x)
        y, r = G.read_wav(p, channels="all", any_rate=True)
        assert r == rate and y.dtype == np.int16 and y.tobytes() == x.tobytes()
        y, r = G.read_wav(p, any_rate=True)
        assert r == rate and y.tobytes() == np.ascontiguousarray(x[:, 0]).tobytes()
    p = tmp_path / "r7000.wav"
    _write_wav(p, 7000, x)
    with pytest.raises(ValueError, match="7000"):
        G.read_wav(p, any_rate=True)
    p = tmp_path / "r48000.wav"
    with pytest.raises(ValueError, match="48000 S/s; the front-end takes 12000 S/s"):
        G.read_wav(p)
    p = tmp_path / "r12000.wav"
    _write_wav(p, 12000, x)
    assert G.read_wav(p, any_rate=True)[1] == 12000 and G.read_wav(p)[1] == 12000
