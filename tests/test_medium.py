"""K7's medium form without a GPU: the host-side fade design (uwspr_tx_fade_design) against tests/medium_exact.py, the
statistics of the sum-of-sinusoids gain, the refusals of the design, the header's declarations, and -- the reason the
GPU comparisons of tests/test_gpu_medium.py mean something -- that every mistake in medium_exact.MUTATIONS changes the
expectation on the case those tests share."""
import os

import numpy as np
import pytest

import medium_exact as MX
import transmit_exact as X


# ================================================================ the design =================================================
@pytest.mark.parametrize("fade", [MX.RAYLEIGH, MX.RICIAN, MX.SHIFT_ONLY,
                                  {"spread": 20.0, "shift": -20.0, "k": 1e6, "seed": 2 ** 64 - 1, "paths": 32},
                                  {"spread": 0.0, "shift": 0.0, "k": 0.0, "seed": 2 ** 33 + 5, "paths": 3}])
def test_fade_design_is_the_restated_design(G, fade):
    """the host's libm (log, cos, sqrt) is not bit-pinned, so omega and phi are held to 1e-12 relative, not to the bit;
    a0 and a1 are two correctly rounded operations each and are held exactly"""
    a0, a1, om, ph = G.tx_fade_design(fade)
    b0, b1, bom, bph = MX.fade_design(fade)
    M = fade["paths"]
    assert om.shape == (M,) and ph.shape == (M,)
    assert abs(a0 - b0) <= 1e-15 and abs(a1 - b1) <= 1e-15
    assert np.all(np.abs(om - bom) <= 1e-12 * np.abs(bom)), np.abs(om - bom).max()
    assert np.all(np.abs(ph - bph) <= 1e-12 * np.abs(bph)), np.abs(ph - bph).max()
    assert abs(a0 * a0 + M * a1 * a1 - 1.0) <= 4e-16
    assert np.all((ph >= 0) & (ph < 2 * np.pi))
    if fade["spread"] == 0.0:
        assert np.all(om == 2 * np.pi * fade["shift"] / 375.0)
    else:
        assert len(np.unique(om)) == M                             # every path its own Doppler


def test_seeds_and_paths_draw_their_own_blocks():
    a = MX.fade_design(MX.RAYLEIGH)
    b = MX.fade_design(dict(MX.RAYLEIGH, seed=MX.RAYLEIGH["seed"] + 2 ** 32))      # the seed's high word is in the key
    assert not np.array_equal(a[2], b[2]) and not np.array_equal(a[3], b[3])
    c = MX.fade_design(dict(MX.RAYLEIGH, paths=4))
    assert np.array_equal(c[2], a[2][:4]) and np.array_equal(c[3], a[3][:4])        # path m depends on (seed, m) only
    assert c[1] == 0.5 and c[0] == 0.0


def test_ensemble_power_and_doppler_spread():
    """256 seeds at spread 1 Hz, Rayleigh, 16 paths: the ensemble mean of |h|^2 (each seed averaged over its transmission,
    every 64th sample) is 1, and the power-weighted rms Doppler -- the paths have equal power, so the root of the mean of
    nu_m^2 -- is spread / 2; each within three standard errors of the ensemble, computed here"""
    k = np.arange(0, X.NTX, 64)
    power, nu2 = [], []
    for seed in range(256):
        d = MX.fade_design({"spread": 1.0, "seed": seed, "paths": 16})
        power.append(np.mean(np.abs(MX.fade_gain(d, k)) ** 2))
        nu2.append(np.mean((d[2] * 375.0 / (2 * np.pi)) ** 2))
    power, nu2 = np.array(power), np.array(nu2)
    se_p = power.std(ddof=1) / np.sqrt(len(power))
    print("mean |h|^2 %.5f (standard error %.5f)" % (power.mean(), se_p))
    assert abs(power.mean() - 1.0) <= 3 * se_p
    rms = np.sqrt(nu2.mean())
    se_rms = nu2.std(ddof=1) / np.sqrt(len(nu2)) / (2 * rms)       # (first order: d sqrt(x) = dx / (2 sqrt(x)))
    print("rms Doppler %.5f Hz (standard error %.5f), expected 0.5" % (rms, se_rms))
    assert abs(rms - 0.5) <= 3 * se_rms


def test_one_path_is_a_pure_doppler_shift():
    a0, a1, om, ph = MX.fade_design(MX.SHIFT_ONLY)
    assert a0 == 0.0 and a1 == 1.0
    k = np.arange(0, 5000)
    h = MX.fade_gain((a0, a1, om, ph), k)
    assert np.abs(np.abs(h) - 1.0).max() <= 1e-12
    assert np.abs(h - np.exp(1j * (om[0] * k + ph[0]))).max() <= 1e-12


def test_design_refuses_what_the_header_refuses(G):
    ok = {"spread": 1.0, "shift": 0.0, "k": 0.0, "seed": 1, "paths": 16}
    G.tx_fade_design(ok)
    for bad in ({"spread": -0.001}, {"spread": 20.001}, {"spread": float("nan")}, {"spread": float("inf")},
                {"shift": 20.001}, {"shift": -20.001}, {"shift": float("nan")},
                {"k": -1e-9}, {"k": 1.0001e6}, {"k": float("inf")}, {"k": float("nan")},
                {"paths": 0}, {"paths": -1}, {"paths": 33}):
        with pytest.raises(ValueError):
            G.tx_fade_design(dict(ok, **bad))
    for edge in ({"spread": 0.0}, {"spread": 20.0}, {"shift": 20.0}, {"shift": -20.0}, {"k": 1e6}, {"paths": 1}, {"paths": 32}):
        G.tx_fade_design(dict(ok, **edge))
    with pytest.raises(ValueError):
        G.tx_fades([{"text": "K1ABC FN42 37", "fading": dict(ok, doppler=1.0)}])
    assert G.tx_fades([{"text": "K1ABC FN42 37"}]) is None
    arr = G.tx_fades([{"text": "K1ABC FN42 37"}, {"text": "K1ABC FN42 37", "fading": {"spread": 0.5}}])
    assert arr[0].paths == 0 and arr[1].paths == 16 and arr[1].spread_hz == 0.5 and arr[1].k_factor == 0.0
    assert G.tx_impulses(None, 2) is None and G.tx_impulses([None, None], 2) is None
    imp = G.tx_impulses([None, {"rate": 0.01, "sigma": 2.0}], 2)
    assert imp[0].rate == 0.0 and imp[0].length == 1 and imp[1].rate == 0.01 and imp[1].length == 1
    with pytest.raises(ValueError):
        G.tx_impulses([{"rate": 0.01, "sigma": 2.0}], 2)


def test_header_carries_the_medium_form(G):
    N = G.native
    hdr = open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read()
    for s in ("typedef struct uwspr_tx_fade {", "typedef struct uwspr_tx_impulse {", "int uwspr_tx_render_medium(",
              "int uwspr_tx_baseband_medium(", "int uwspr_tx_fade_design(const uwspr_tx_fade *f, double a[2], double *omega, double *phi);",
              "0x46414445", "double spread_hz;", "double k_factor;", "int32_t paths;", "double rate;", "int32_t length;"):
        assert s in hdr, s
    assert "#define UWSPR_ABI_VERSION 6 " in hdr
    for s in ("uwspr_tx_render_medium", "uwspr_tx_baseband_medium", "uwspr_tx_fade_design"):
        assert s in N.ABI_SYMBOLS
    assert MX.impulse_thr(0.25) == 2 ** 30 and MX.impulse_thr(0.0) == 0 and MX.impulse_thr(2.0 ** -33) == 0


# ================================================================ the mutations ==============================================
def _symbols(G):
    return G.wspr_symbols


@pytest.mark.parametrize("mutation", MX.FADE_MUTATIONS)
def test_fade_mutations_change_the_model_beyond_the_bound(G, mutation):
    """on the windows of the shared case where a signal with that part of the gain runs (a0: the Rician one, which the
    "k0" window does not reach) a wrong gain moves the binary64 model by far more than the bound the device's baseband
    is held to"""
    sigs = MX.faded_signals(3000)
    for name, (t0, n) in MX.faded_windows(3000).items():
        if mutation == "a0_dropped" and name == "k0":
            continue
        good = MX.faded_model(sigs, _symbols(G), t0, n)
        bad = MX.faded_model(sigs, _symbols(G), t0, n, mutation=mutation)
        assert np.abs(good).max() > 0.1
        assert np.abs(good - bad).max() > 1000 * MX.faded_bound(sigs), (name, mutation)


def _impulse_case():
    """the shared window with a chain, AWGN and a background of the sizes a render has: everything but the impulses is
    made up here (the GPU tests take the device's)"""
    t0, nf = MX.IMPULSE_WINDOW
    rng = np.random.default_rng(5)
    chain = (rng.standard_normal(nf) / 32).astype(np.float32)
    n = t0 + np.arange(nf, dtype=np.int64)
    g32 = X.gauss_ref(*X.gauss_inputs(21, 0, n)).astype(np.float32)
    bg = (rng.standard_normal(777) * 0.01).astype(np.float32)
    return t0, nf, chain, n, g32, bg


def _expectation(imp, mutation=None):
    t0, nf, chain, n, g32, bg = _impulse_case()
    terms = MX.impulse_terms(imp, 0, t0, nf, mutation)
    return MX.compose_medium(chain, g32, 0.05, terms, imp["sigma"], MX.ref_draw(imp, 0, mutation), bg, 0.7, n, mutation)


@pytest.mark.parametrize("mutation", MX.IMPULSE_MUTATIONS)
def test_impulse_mutations_change_the_expected_bytes(mutation):
    """the AWGN seed equals the impulse seed here, as in the GPU test of their independence"""
    imp = MX.edge_impulse()[0] if mutation == "thr_less_or_equal" else MX.IMPULSE
    good, bad = _expectation(imp), _expectation(imp, mutation)
    assert good.tobytes() != bad.tobytes(), mutation
    _, _, chain, n, g32, bg = _impulse_case()
    plain = MX.compose_medium(chain, g32, 0.05, [], 0.0, None, bg, 0.7, n)
    assert 5 <= (good != plain).sum() <= 60                        # about 2000 * 3 / 250 outputs carry an impulse


def test_impulse_supports_are_integers_from_the_blocks():
    t0, nf = MX.IMPULSE_WINDOW
    imp, at = MX.edge_impulse()
    assert t0 <= at < t0 + nf
    assert at not in MX.impulse_events(imp, 0, t0, nf) and at in MX.impulse_events(imp, 0, t0, nf, "thr_less_or_equal")
    ev = MX.impulse_events(MX.IMPULSE, 0, t0, nf)
    assert np.all(np.diff(ev) > 0) and 2 <= len(ev) <= 30
    # an event before t0 reaches into the window; no index is negative
    first = MX.impulse_events(MX.IMPULSE, 0, 0, 4000)
    assert first.min() >= 0
    e = int(ev[0])
    cnt = MX.impulse_support(MX.IMPULSE, 0, e + 1, 10)
    assert cnt[0] >= 1 and cnt[1] >= 1                             # the burst of e: samples e + 1 and e + 2
    assert MX.impulse_support(dict(MX.IMPULSE, rate=0.0), 0, t0, nf).sum() == 0
    assert MX.impulse_support(dict(MX.IMPULSE, sigma=0.0), 0, t0, nf).sum() == 0
    # other channels, other streams
    assert not np.array_equal(MX.impulse_events(MX.IMPULSE, 1, t0, nf), ev)
