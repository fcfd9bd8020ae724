"""K0 front-end: 12 kS/s real audio -> 375 S/s complex frames.

In the reference this stage is the flowgraph's chain of GNU Radio blocks (examples/WaveFilePlusNoiseDecode.grc:303-400,
527, 840-956, 1767-1808) -- third-party, unpinned, absent from the reference tree and from this image: **parity
unpinned by construction**.  What CAN be checked, and is:
  * the oracle's tap designs (oracle/frontend_grc.py, restating GNU Radio 3.7's firdes / window / design_filter)
    against a second, independent window-method implementation (scipy.signal.firwin);
  * the product's designs and its composite 6831-tap filter (C++, uwspr_frontend_design) against the oracle's;
  * the HIP kernel against the oracle's stage-by-stage float64 chain at 1e-5 of the output's peak, on noise, on the
    reference's closed-loop demo mix and on the reference's recording;
  * both README demos decode through that chain: `VE3EMB FN25 30` (README.md:37, 61) and `VE3EMB FN42 33`
    (examples/150613_1920.wav), on the CPU oracle and end to end on the GPU.
The compact single-stage mode (option frontend = 1) keeps its own formula test."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

TOL = 1e-5          # relative to the peak magnitude of the float64 reference output


@pytest.fixture(scope="module")
def FE():
    import frontend_grc
    return frontend_grc


# ---- tap designs (CPU) --------------------------------------------------------------------------------
def test_oracle_designs_match_scipy_firwin(FE):
    """Two independent statements of the window method: the oracle (GNU Radio's formulas, binary32 taps) and scipy."""
    import scipy.signal as ss
    h1, h2, h3 = FE.stage_taps()
    assert (len(h1), len(h2), len(h3)) == (2891, 2891, 1051)      # compute_ntaps: 53 dB Hamming / 72.2 dB Kaiser
    s1 = ss.firwin(len(h1), [1490.0, 1510.0], window="hamming", pass_zero=False, fs=12000.0)
    s2 = ss.firwin(len(h2), 1510.0, window="hamming", fs=12000.0)
    s3 = ss.firwin(len(h3), 0.0140625, window=("kaiser", 7.0), fs=1.0)
    for a, b in ((h1, s1), (h2, s2), (h3, s3)):
        assert np.abs(a - b).max() <= 2e-7 * np.abs(b).max()      # binary32 rounding of the reference's taps


def test_product_designs_match_the_independent_oracle(G, FE):
    for stage, h in zip((1, 2, 3), FE.stage_taps()):
        got = G.frontend_design(G.FRONTEND_GRC, stage)
        assert len(got) == len(h)
        g32 = got.astype(np.float32)
        assert (g32.astype(np.float64) == got).all()              # the product holds binary32 designs too
        # same formulas in C++ (glibc sin / cos) and numpy: equal but for a last-place rounding of a few taps
        assert np.abs(g32 - h).max() <= 2.0 ** -23 * np.abs(h).max()
        assert (g32 != h).mean() < 0.02
    g, delay = G.frontend_design(G.FRONTEND_GRC, 0)
    want = FE.composite_taps()
    assert delay == 0 and len(g) == len(want) == 2891 + 2891 + 1051 - 2
    assert np.abs(g - want).max() <= 1e-7 * np.abs(want).max()


def test_composite_filter_is_the_chain(FE):
    """The one-FIR form the kernel applies equals the stage-by-stage chain (float64, 4e-11) and passes 1500 +- 10 Hz
    with unit gain while the image at -1500 Hz and everything the /32 would alias is >= 50 dB down."""
    import scipy.signal as ss
    rng = np.random.default_rng(0)
    x = rng.standard_normal(200000).astype(np.float32)
    g = FE.composite_taps()
    y = FE.chain(x, nout=6000)
    z = ss.oaconvolve(x.astype(np.float64), g)[:len(x)][::32][:6000]
    assert np.abs(y - z).max() <= 1e-9 * np.abs(y).max()
    H = np.abs(np.fft.fft(g, 1 << 18))
    f = np.fft.fftfreq(1 << 18, 1 / 12000.0)
    assert abs(H[np.abs(f - 1500.0) < 2.0] - 1.0).max() < 2e-2
    assert H[np.abs(f - 1500.0) > 375.0 / 2].max() < 10 ** (-50 / 20.0)


def test_compact_taps_are_a_unit_gain_lowpass_times_the_mixer(G):
    g, D = G.frontend_design(G.FRONTEND_COMPACT, 0)
    assert len(g) == 1025 and D == 512
    h = np.abs(g)
    assert np.allclose(h, h[::-1], atol=1e-12)                # linear phase
    k = np.arange(1025)
    mix = np.exp(-1j * np.pi * (D - k) / 4)
    hr = (g / mix).real
    assert abs(hr.sum() - 1.0) < 1e-9                         # unit DC gain
    assert np.abs((g / mix).imag).max() < 1e-12
    H = np.abs(np.fft.rfft(hr, 1 << 16))
    f = np.fft.rfftfreq(1 << 16, 1 / 12000.0)
    assert H[f < 60].min() > 0.98 and H[f > 187.5].max() < 2e-3   # pass band / alias band


# ---- the reference's two demo inputs ---------------------------------------------------------------
def _closed_loop_audio(seconds=120, whales_gain=None):
    """examples/WaveFilePlusNoiseDecode.grc: test_1500_Hz.wav x 0.1 (grc:636, 751) + whales_12000sps.wav x 1
    (grc:585, 802), both sources repeating; wavfile_source scales int16 by 1/32768."""
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    n = seconds * 12000
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    wg = float(rec["whales_gain"]) if whales_gain is None else whales_gain
    return (float(rec["tx_gain"]) * tx + wg * wh).astype(np.float32)


def _recording():
    return np.load(os.path.join(GOLDEN, "150613_1920_int16.npz"))["x"].astype(np.float32) / 32768.0


def _decode_set(G, recs):
    out = set()
    for r in recs:
        dec = G.decode_candidate(r)
        if dec is not None:
            out.add(G.unpack_message(dec[0])[1])
    return out


def _oracle_records(G, oracle, frame, ncand):
    recs = []
    for c in oracle.FDR().transform(frame)[:ncand]:
        d = oracle.demod_candidate(c, 1500, frame)
        rec = np.zeros(1, G.native.DEMOD_DTYPE)[0]
        for k in ("f1", "drift1", "sync1", "shift1", "worth_a_try", "jig_sync", "jig_rms", "jig_shift", "symbols"):
            rec[k] = d[k]
        recs.append(rec)
    return recs


def _as_frame(y):
    return np.stack([y.real, y.imag], axis=1).astype(np.float32)


def test_both_demos_decode_on_the_cpu_oracle_through_the_grc_chain(G, oracle, FE):
    """The inputs the reference's authors demo, through the float64 restatement of THEIR front-end chain, the oracle's
    FDR + schedule and the host tail: `VE3EMB FN25 30` (README.md:37; a reference-held known answer for the oracle on a
    noisy frame) and `VE3EMB FN42 33` (the recording)."""
    assert _decode_set(G, _oracle_records(G, oracle, _as_frame(FE.chain(_closed_loop_audio())), 2)) == {"VE3EMB FN25 30"}
    assert "VE3EMB FN42 33" in _decode_set(G, _oracle_records(G, oracle, _as_frame(FE.chain(_recording())), 3))


# ---- the kernel ---------------------------------------------------------------------------------------
def _close(got, ref):
    z = got[:, 0].astype(np.float64) + 1j * got[:, 1].astype(np.float64)
    return np.abs(z - ref).max() / np.abs(ref).max()


# 64 outputs of a full-size record: its first, a workgroup seam in its middle (40 x 512), its last
EXACT_64 = np.concatenate([np.arange(16), np.arange(20464, 20496), np.arange(44984, 45000)])


def _restated(G, mode, x):
    """the outputs EXACT_64 of record x as the kernel's own binary32 sums give them (tests/frontend_exact.py, which
    tests/test_gpu_frontend_exact.py holds K0 to at small shapes): ties the full-size record to those"""
    import frontend_exact
    g, D = G.frontend_design(mode, 0)
    return frontend_exact.restate(g.astype(np.complex64), D, x, 0, EXACT_64)


@pytest.mark.gpu
def test_kernel_matches_the_float64_chain(G, FE):
    """uwspr_frontend_batch (grc mode, the default) against the oracle's stage-by-stage chain: white noise (a full
    record, one that goes silent, a short one: zero beyond the end), the closed-loop mix, the recording."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 45000 * 32)).astype(np.float32)
    x[1, 700000:] = 0.0
    demo = np.stack([_closed_loop_audio(), np.resize(_recording(), 120 * 12000)])
    ctx = G.Context()
    try:
        y = ctx.frontend(x)
        ys = ctx.frontend(x[:, :500000])
        yd = ctx.frontend(demo)
        rec = _recording()
        yr = ctx.frontend(rec[None])                   # the recording at its own length
    finally:
        ctx.close()
    for b in range(2):
        assert _close(y[b], FE.chain(x[b])) <= TOL
        assert _close(yd[b], FE.chain(demo[b])) <= TOL
    assert _close(ys[0], FE.chain(x[0, :500000])) <= TOL
    assert not ys[0, (500000 + 6831) // 32 + 1:].any()      # nothing after the last tap has left the record
    assert _close(yr[0], FE.chain(rec)) <= TOL
    assert y[0][EXACT_64].tobytes() == _restated(G, G.FRONTEND_GRC, x[0]).tobytes()


@pytest.mark.gpu
def test_compact_kernel_matches_its_float64_formula(G):
    import scipy.signal as ss
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 45000 * 32)).astype(np.float32)
    x[1, 600000:] = 0.0
    ctx = G.Context(options={"frontend": G.FRONTEND_COMPACT})
    try:
        y = ctx.frontend(x)
        ctx.set_option("frontend", G.FRONTEND_GRC)     # the taps follow the option
        y0 = ctx.frontend(x[:1])
    finally:
        ctx.close()
    g, D = G.frontend_design(G.FRONTEND_COMPACT, 0)
    for b in range(2):
        z = ss.oaconvolve(x[b].astype(np.float64), g)
        idx = D + 32 * np.arange(45000)
        ref = np.where(idx < len(z), z[np.minimum(idx, len(z) - 1)], 0.0)
        assert _close(y[b], ref) <= TOL
    g0, _ = G.frontend_design(G.FRONTEND_GRC, 0)
    ref0 = ss.oaconvolve(x[0].astype(np.float64), g0)[:x.shape[1]][::32][:45000]
    assert _close(y0[0], ref0) <= TOL
    assert y[0][EXACT_64].tobytes() == _restated(G, G.FRONTEND_COMPACT, x[0]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_reference_recording_decodes_end_to_end(G, mode):
    """BASELINE configs[4] plumbing: wav -> K0 -> FDR -> schedule -> Fano -> unpack, with and without added noise,
    through either front-end."""
    x = _recording()
    rng = np.random.default_rng(1)
    ctx = G.Context(options={"frontend": mode})
    try:
        frames = ctx.frontend(np.stack([x, x + 0.5 * rng.standard_normal(x.size).astype(np.float32)]))
        cands, out = ctx.pipeline_batch(frames, max_per_frame=2)
    finally:
        ctx.close()
    for b in range(2):
        texts = []
        for j in range(min(2, len(cands[b]))):
            dec = G.decode_candidate(out[b, j])
            if dec is not None:
                texts.append(G.unpack_message(dec[0])[1])
        assert "VE3EMB FN42 33" in texts, (b, texts)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_synthetic_audio_round_trip(G, mode):
    audio, meta = G.synth.make_audio(3, snr_db=-18.0)
    ctx = G.Context(options={"frontend": mode})
    try:
        frames = ctx.frontend(audio)
        cands, out = ctx.pipeline_batch(frames, max_per_frame=1)
    finally:
        ctx.close()
    for b in range(3):
        dec = G.decode_candidate(out[b, 0])
        assert dec is not None
        assert (np.unpackbits(dec[0].view(np.uint8))[:50] == meta[b]["bits"]).all()
        assert abs(float(out[b, 0]["f1"]) - meta[b]["f_off"]) < 0.2


@pytest.mark.gpu
def test_closed_loop_demo_decodes_end_to_end_on_the_gpu(G, oracle):
    """BASELINE configs[0]'s flowgraph input on the HIP path: wav mix -> K0 (the flowgraph's chain) -> FDR -> schedule
    -> Fano -> unpack = `VE3EMB FN25 30`; the set of messages decoded from the GPU's records equals the set the CPU
    (oracle FDR + schedule on the same 375 S/s frame, same host tail) decodes, and every record field equals the
    oracle's.  Also with the whale noise three times as loud."""
    ctx = G.Context()
    try:
        frames = ctx.frontend(np.stack([_closed_loop_audio(), _closed_loop_audio(whales_gain=3.0)]))
        cands, out = ctx.pipeline_batch(frames, max_per_frame=2)
    finally:
        ctx.close()
    for b in range(2):
        n = min(2, len(cands[b]))
        gpu = _decode_set(G, [out[b, j] for j in range(n)])
        orc = _oracle_records(G, oracle, frames[b], 2)
        assert gpu == _decode_set(G, orc), b
        for j in range(n):
            assert int(out[b, j]["shift1"]) == int(orc[j]["shift1"]) and int(out[b, j]["worth_a_try"]) == int(orc[j]["worth_a_try"])
            assert out[b, j]["symbols"].tobytes() == orc[j]["symbols"].tobytes(), (b, j)
            assert np.float32(out[b, j]["sync1"]).tobytes() == np.float32(orc[j]["sync1"]).tobytes()
        if b == 0:
            assert gpu == {"VE3EMB FN25 30"}
