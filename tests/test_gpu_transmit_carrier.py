"""K7's carrier form on the device (uwspr_tx_render_at, uwspr_tx_baseband_at, the options "tx_cutoff" / "tx_form"), held
to the bit against tests/transmit_carrier_exact.py on the device's own baseband of every carrier group, then against a
float64 two-stage restatement of the flowgraph at the carrier, the binary64 motion model with the carrier in the Doppler
term, and closed through the multi-carrier receiver.  tests/test_transmit_carrier.py shows on the CPU that the byte
expectations see a wrong rotator sign, index, remainder, reduction, group pairing and group order.

1 bytes  2 several groups in one channel  3 chunk and placement invariance  4 defaults  5 independent chain  6 moving
7 closed loop  8 refusals"""
import numpy as np
import pytest

import transmit_carrier_exact as TC
import transmit_exact as X

NTX = X.NTX


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx59(G):
    c = G.Context(options={"tx_cutoff": 5900})
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(G):
    return G.frontend_rotator()


_images = {}


def _image(G, fc, cutoff=2500):
    if (fc, cutoff) not in _images:
        _images[(fc, cutoff)] = G.tx_design(fc, cutoff)[1]
    return _images[(fc, cutoff)]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _where(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return "shapes %s %s" % (a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else np.flatnonzero(a != b)
    return "%d of %d differ, first at %d: %r against %r" % (len(bad), len(a), bad[0] if len(bad) else -1,
                                                           a[bad[:1]], b[bad[:1]])


def _device(ctx, sigs, nf, fmt="f32", channels=1, **kw):
    import torch
    dev = torch.empty((nf, channels), dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
    ctx.tx_render(sigs, nf, format=fmt, channels=channels, out=dev, **kw)
    return dev.cpu().numpy()


def _restated(t0, nf):
    """the outputs of window [t0, t0 + nf) that are restated, as offsets: the first and last 16, 1024 across the first
    tile seam (workgroups start at 32 (t0 div 32) + 16384 k) and 2048 consecutive ones further on -- every phase n mod 32
    many times over.  The other outputs are held by chunk invariance (test 3)."""
    if nf <= 4096:
        return np.arange(nf, dtype=np.int64)
    seam = 32 * (t0 // 32) + X.TILE - t0
    mid = seam + X.TILE // 2 + 5
    off = np.concatenate([np.arange(16), np.arange(seam - 512, seam + 512), np.arange(mid, mid + 2048), np.arange(nf - 16, nf)])
    off = np.unique(off[(off >= 0) & (off < nf)]).astype(np.int64)
    assert len(off) >= 2048 and len(np.unique((t0 + off) % 32)) == 32
    return off


def _expect(G, ctx, table, sigs, t0, off, channel=0, cutoff=2500):
    """TC.expect of outputs t0 + off of one channel, the baseband of every carrier group being the device's own"""
    j0, nbb = X.window(t0, int(off.max()) + 1)
    groups = {}
    for s in sigs:
        if s.get("channel", 0) == channel:
            groups.setdefault(s.get("carrier", 1500), []).append(s)
    if not groups:
        return np.zeros(len(off), np.float32)
    for fc in groups:
        x = X.file_orientation(ctx.tx_baseband(groups[fc], nbb, t0=j0, channel=channel))
        groups[fc] = (_image(G, fc, cutoff), x)
    return TC.expect(groups, t0 + off, j0, table)


def _at(sigs, fc):
    return [dict(s, carrier=fc) for s in sigs]


# ================================================================ 1. bytes ===============================================
@pytest.mark.gpu
@pytest.mark.parametrize("fc", [1875, 1501, 497, 2203, 5650])
def test_render_at_a_carrier_is_the_restated_chain(G, ctx, ctx59, table, fc):
    """the dense case of the 1500 Hz byte tests at another carrier: 1875 (other taps, no rotator), 1501, 497, 2203, and 5650
    with tx_cutoff 5900; f32 and s16, host and device output"""
    c, cutoff = (ctx59, 5900) if fc == 5650 else (ctx, 2500)
    sigs = _at(X.dense_signals(3000), fc)
    before = G.tx_carrier_launch_counts()
    for wname in ("first", "middle", "last"):
        t0, nf = X.dense_windows(3000)[wname]
        off = _restated(t0, nf)
        got = c.tx_render(sigs, nf, t0=t0)
        assert got.shape == (nf, 1) and got.dtype == np.float32
        want = _expect(G, c, table, sigs, t0, off, cutoff=cutoff)
        assert (want != 0).sum() > len(off) // 4
        assert _same(got[off, 0], want), (fc, wname, _where(got[off, 0], want))
        assert _same(_device(c, sigs, nf, t0=t0), got), (fc, wname)
        s16 = c.tx_render(sigs, nf, t0=t0, format="s16")
        assert _same(s16[:, 0], X.quantise(got[:, 0])), (fc, wname)
        assert _same(_device(c, sigs, nf, fmt="s16", t0=t0), s16), (fc, wname)
    after = G.tx_carrier_launch_counts()
    assert after[0] - before[0] == 6 and after[1] - before[1] == 6       # the carrier form is what ran
    # ... and it is another signal than the 1500 Hz render of the same messages
    if cutoff == 2500:
        t0, nf = X.dense_windows(3000)["middle"]
        assert not _same(c.tx_render(X.dense_signals(3000), nf, t0=t0), c.tx_render(sigs, nf, t0=t0))


# ================================================================ 2. several groups in one channel ===========================
def _fdma():
    """C = 3: channel 0 with three carriers in shuffled signal order (2203 twice), channel 1 empty, channel 2 at 1500 only"""
    d = X.dense_signals(3000)
    return [dict(d[0], channel=0, carrier=2203), dict(d[1], channel=2), dict(d[1], channel=0, carrier=497),
            dict(d[2], channel=0, carrier=2203), dict(d[0], channel=2, carrier=1500, start=3100),
            dict(d[2], channel=0, carrier=1501, start=3500, f0=-60.0)]


@pytest.mark.gpu
def test_groups_of_one_channel_add_in_ascending_hz(G, ctx, table):
    sigs = _fdma()
    t0, nf = X.dense_windows(3000)["middle"]
    off = _restated(t0, nf)
    got = ctx.tx_render(sigs, nf, t0=t0, channels=3)
    want = _expect(G, ctx, table, sigs, t0, off, channel=0)
    assert _same(got[off, 0], want), _where(got[off, 0], want)
    assert (got[:, 1] == 0).all() and not np.signbit(got[:, 1]).any()
    # channel 2 is at 1500 Hz only: the bytes of the 1500 Hz kernels on those signals
    plain = ctx.tx_render([{k: v for k, v in s.items() if k != "carrier"} for s in sigs if s["channel"] == 2], nf, t0=t0, channels=3)
    assert _same(got[:, 2], plain[:, 2]) and (plain[:, 2] != 0).any()
    assert _same(_device(ctx, sigs, nf, t0=t0, channels=3), got)
    s16 = ctx.tx_render(sigs, nf, t0=t0, channels=3, format="s16")
    assert _same(s16, X.quantise(got.reshape(-1)).reshape(got.shape))
    # the order the signals are given in does not matter between groups (it does inside one: index order)
    shuffled = [sigs[i] for i in (5, 2, 1, 0, 4, 3)]
    assert _same(ctx.tx_render(shuffled, nf, t0=t0, channels=3), got)
    # one group of the multi-group render is that carrier rendered alone when the others have gain 0
    for fc in (497, 1501, 2203):
        muted = [s if s.get("carrier", 1500) == fc or s["channel"] != 0 else dict(s, gain=0.0) for s in sigs]
        alone = [s for s in sigs if s["channel"] == 0 and s.get("carrier") == fc]
        a = ctx.tx_render(muted, nf, t0=t0, channels=3)[:, 0]
        b = ctx.tx_render(alone, nf, t0=t0)[:, 0]
        assert _same(a, b), (fc, _where(a, b))
        assert not _same(a, got[:, 0])


# ================================================================ 3. chunks, placement, groups that come and go ==============
def _come_and_go(base):
    """around baseband index `base`: a 497 Hz signal -- its carrier's only one -- whose last contribution falls about
    28 700 frames into the window that starts at audio 32 base, a 2203 Hz one running through, a 1501 Hz one that begins
    inside, a second 2203 Hz one"""
    return [{"text": "K1ABC FN42 37", "start": base - NTX + 800, "f0": -150.0, "drift": -20.0, "gain": 0.3, "phase0": 1e3, "carrier": 497},
            {"text": "VE3EMB FN25 30", "start": base - 20000, "f0": 3.1, "gain": 1.0, "phase0": -1e3, "carrier": 2203},
            {"text": "PJ4/K1ABC 37", "start": base + 700, "f0": 120.0, "drift": 4.0, "gain": 1.7, "phase0": 0.4, "carrier": 1501},
            {"text": "G4XYZ/7 10", "start": base - 9000, "f0": -40.0, "gain": 0.8, "phase0": 2.0, "carrier": 2203}]


@pytest.mark.gpu
@pytest.mark.parametrize("base", [0, 2 ** 40], ids=["negative_start_t0_0", "start_2^40"])
def test_pieces_concatenate_while_groups_come_and_go(G, ctx, table, base):
    """base 0: signals with negative `start` and t0 = 0, so the rotator meets j = -103 .. -1; base 2^40: t0 = 2^45"""
    sigs = _come_and_go(base)
    t0, nf = 32 * base, X.WINDOW
    end497 = 32 * (sigs[0]["start"] + NTX - 1) + X.NT - 1 - t0
    assert 16 < end497 < nf - X.TILE
    for fmt in ("f32", "s16"):
        whole = ctx.tx_render(sigs, nf, t0=t0, format=fmt, sigma=0.01, seed=11)
        parts, k, i = [], 0, 0
        while k < nf:
            ln = min(nf - k, (1, 7, 16384, 20001)[i % 4])
            parts.append(ctx.tx_render(sigs, ln, t0=t0 + k, format=fmt, sigma=0.01, seed=11))
            k, i = k + ln, i + 1
        assert _same(np.concatenate(parts), whole), fmt
        assert _same(_device(ctx, sigs, nf, fmt=fmt, t0=t0, sigma=0.01, seed=11), whole), fmt
    # the noise-free render is the restated sum, where all four run, and where the 497 Hz group has gone
    clean = ctx.tx_render(sigs, nf, t0=t0)
    off = _restated(t0, nf)
    want = _expect(G, ctx, table, sigs, t0, off)
    assert _same(clean[off, 0], want), _where(clean[off, 0], want)
    tail = np.arange(end497 + 1, nf, dtype=np.int64)[-2048:]
    assert _same(clean[tail, 0], _expect(G, ctx, table, sigs[1:], t0, tail))
    assert not _same(clean[:end497, 0], ctx.tx_render(sigs[1:], nf, t0=t0)[:end497, 0])
    if base == 0:
        j0, _ = X.window(t0, nf)
        assert j0 == -(X.T - 1)                                   # the first outputs read negative baseband indices


# ================================================================ 4. defaults =================================================
@pytest.mark.gpu
def test_default_carrier_runs_the_old_kernels_and_tx_form_gives_their_bytes(G, ctx):
    sigs = X.dense_signals(3000) + [dict(s, channel=1, start=s["start"] + 50) for s in X.dense_signals(3000)[:2]]
    t0, nf = X.dense_windows(3000)["middle"]
    kw = dict(t0=t0, channels=2, sigma=0.02, seed=[3, 4])
    before = G.tx_carrier_launch_counts()
    plain = {fmt: ctx.tx_render(sigs, nf, format=fmt, **kw) for fmt in ("f32", "s16")}
    keyed = {fmt: ctx.tx_render(_at(sigs, 1500), nf, format=fmt, **kw) for fmt in ("f32", "s16")}
    assert G.tx_carrier_launch_counts() == before                 # no carrier-form launch
    assert _same(keyed["f32"], plain["f32"]) and _same(keyed["s16"], plain["s16"])
    bb = ctx.tx_baseband(sigs, 2000, t0=30000)
    assert _same(ctx.tx_baseband(_at(sigs, 1500), 2000, t0=30000), bb)
    forced = G.Context(options={"tx_form": 1})
    try:
        for fmt in ("f32", "s16"):
            a = forced.tx_render(sigs, nf, format=fmt, **kw)
            assert _same(a, plain[fmt]), (fmt, _where(a, plain[fmt]))
        after = G.tx_carrier_launch_counts()
        assert after[0] == before[0] + 1 and after[1] == before[1] + 1
        assert _same(forced.tx_render([], 4096, t0=5, channels=2, sigma=1.0, seed=9), ctx.tx_render([], 4096, t0=5, channels=2, sigma=1.0, seed=9))
    finally:
        forced.close()
    assert ctx.get_option("tx_cutoff") == 2500 and ctx.get_option("tx_form") == 0


# ================================================================ 5. the independent chain ====================================
def _baseband_file64(G, sig, n):
    """a channel's baseband as the .c2 FILE holds it (gain e^{-j theta}), binary64, samples [0, n)"""
    return np.conj(X.baseband_model(sig, G.wspr_symbols, 0, n))


@pytest.mark.gpu
@pytest.mark.parametrize("fc", [497, 2203])
def test_render_matches_the_two_stage_chain_at_the_carrier(G, ctx, fc):
    """zero-stuff x32, h1, the rotated h2, the mixer at fc, the real part, in float64 from sample 0: under the 2e-6 that
    tests/test_gpu_transmit.py::test_render_matches_the_two_stage_chain holds the 1500 Hz render to"""
    rng = np.random.default_rng(fc)
    texts = ["K1ABC FN42 37", "PJ4/K1ABC 37", "VE3EMB FN25 30"]
    sig = [{"text": texts[i], "start": int(rng.integers(0, 2500)), "f0": float(rng.uniform(-80, 80)),
            "drift": float(rng.uniform(-4, 4)), "phase0": float(rng.uniform(-np.pi, np.pi)),
            "gain": float(rng.uniform(0.2, 1.5)), "carrier": fc} for i in range(3)]
    t0, nf = 100003, 4 * X.TILE
    got = ctx.tx_render(sig, nf, t0=t0)[:, 0]
    nbb = (t0 + nf) // 32 + 2
    ref = TC.two_stage(_baseband_file64(G, sig, nbb), t0 + nf, fc)[t0:]
    err = np.abs(got.astype(np.float64) - ref).max()
    print("%d Hz: render against the float64 two-stage chain: %.3g (bound 2e-6)" % (fc, err))
    assert err <= 2e-6, (fc, err)
    assert np.abs(ref).max() > 0.02
    assert (ctx.tx_render(sig, 1000, t0=0) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fc", [497, 1875, 2203])
def test_a_tone_comes_out_at_the_carrier_plus_f0(G, ctx, fc):
    """one constant symbol (2: +0.5 tone spacings) at f0 = 2 Hz, no noise: the audio's spectrum peaks at
    fc + 2 + 0.5 * 375 / 256 Hz, to the bin"""
    nfft = 8 * X.TILE
    a = ctx.tx_render([{"symbols": np.full(162, 2, np.uint8), "start": 0, "f0": 2.0, "carrier": fc}], nfft, t0=40000)[:, 0]
    spec = np.abs(np.fft.rfft(a.astype(np.float64) * np.hanning(nfft)))
    peak = np.argmax(spec) * 12000.0 / nfft
    want = fc + 2.0 + 0.5 * 375.0 / 256.0
    print("%d Hz: peak at %.3f Hz, expected %.3f" % (fc, peak, want))
    assert abs(peak - want) <= 12000.0 / nfft
    assert abs(np.abs(a).max() - 1.0 / 32) <= 0.01 / 32                # a unit baseband as a tone of amplitude 1/32


# ================================================================ 6. moving ===================================================
def _theta(G, s, kp):
    sym = G.wspr_symbols(s["text"]).astype(np.float64)
    f0, drift, phase0 = s.get("f0", 0.0), s.get("drift", 0.0), s.get("phase0", 0.0)
    u = np.arange(NTX, dtype=np.float64)
    f = f0 + (np.repeat(sym, 256) - 1.5) * 375.0 / 256 + drift * (u - (NTX - 1) / 2) / (NTX - 1)
    acc = phase0 + np.concatenate([[0.0], np.cumsum(2 * np.pi * f / 375.0)])
    ph = acc[::256][:162]
    q = np.clip(np.floor(kp / 256.0).astype(np.int64), 0, 161)
    r = kp - 256.0 * q
    wf = 2 * np.pi * f0 / 375.0
    wd = 2 * np.pi * drift / ((NTX - 1) * 375.0)
    return ph[q] + r * (2 * np.pi * (sym[q] - 1.5) / 256.0 + wf) + wd * (r * (256.0 * q - 0.5 * (NTX - 1)) + 0.5 * r * (r - 1.0))


def _moving_model(G, s, n, fc):
    """tests/test_gpu_tx_motion.py's binary64 model of one DOPPLER / DELAY signal, the carrier fc in the Doppler term"""
    m = s["motion"]
    k = (np.arange(n, dtype=np.int64) - s["start"]).astype(np.float64)
    (v1, v2), (p1, p2), tf = m["v"], m["p"], m.get("t", 0.0)
    t = tf + k / 375.0
    R = np.hypot(v1 * t + p1, v2 * t + p2)
    D = (R - np.hypot(v1 * tf + p1, v2 * tf + p2)) / 1500.0
    kp = k - 375.0 * D if m["model"] == "delay" else k
    ok = (kp >= 0) & (kp < NTX)
    y = np.zeros(n, np.complex128)
    y[ok] = s.get("gain", 1.0) * np.exp(1j * (_theta(G, s, kp[ok]) - 2 * np.pi * float(fc) * D[ok]))
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["doppler", "delay"])
def test_a_motions_doppler_scales_with_the_signals_carrier(G, ctx, model):
    n = 45600
    s = {"text": "K1ABC FN42 37", "start": 375, "f0": 3.1, "drift": 1.7, "phase0": 0.4, "gain": 0.9,
         "motion": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": model}}
    got = ctx.tx_baseband([dict(s, carrier=2203)], n)
    ref = _moving_model(G, s, n, 2203)
    err = max(np.abs(got[:, 0] - ref.real).max(), np.abs(got[:, 1] - ref.imag).max())
    print("%s at 2203 Hz: baseband error %.3g (bound 2e-6)" % (model, err))
    assert err <= 2e-6, err
    at1500 = ctx.tx_baseband([s], n)
    ref1500 = _moving_model(G, s, n, 1500)
    assert max(np.abs(at1500[:, 0] - ref1500.real).max(), np.abs(at1500[:, 1] - ref1500.imag).max()) <= 2e-6
    assert np.abs(got - at1500).max() > 0.5                        # another Doppler: another signal
    assert _same(ctx.tx_baseband([dict(s, carrier=1500)], n), at1500)
    # a zero-velocity motion at 2203 Hz gives the static bytes, baseband and audio
    still = dict(s, carrier=2203, motion={"v": (0.0, 0.0), "p": (120.0, -35.0), "t": 17.0, "model": model})
    static = {k: v for k, v in still.items() if k != "motion"}
    assert _same(ctx.tx_baseband([still], n), ctx.tx_baseband([static], n))
    t0, nf = 32 * 20000 + 5, 2 * X.TILE
    for fmt in ("f32", "s16"):
        assert _same(ctx.tx_render([still], nf, t0=t0, format=fmt), ctx.tx_render([static], nf, t0=t0, format=fmt)), fmt
    # the moving render at the carrier is the chain on the moving baseband (the moving carrier instances)
    mov = ctx.tx_render([dict(s, carrier=2203)], nf, t0=t0)
    assert not _same(mov, ctx.tx_render([dict(static, carrier=2203)], nf, t0=t0))


@pytest.mark.gpu
def test_moving_render_at_a_carrier_is_the_restated_chain(G, ctx, table):
    sigs = [{"text": "K1ABC FN42 37", "start": 3000, "f0": 2.0, "drift": 0.5, "phase0": 0.3, "carrier": 2203,
             "motion": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "doppler"}},
            {"text": "VE3EMB FN25 30", "start": 3100, "f0": -3.0, "gain": 0.6, "carrier": 497,
             "motion": {"v": (1.0, -0.5), "p": (0.0, 600.0), "model": "delay"}},
            {"text": "PJ4/K1ABC 37", "start": 2500, "f0": 40.0, "gain": 0.5, "carrier": 2203}]
    t0, nf = 32 * 23000 + 9, X.WINDOW
    off = _restated(t0, nf)
    got = ctx.tx_render(sigs, nf, t0=t0)
    want = _expect(G, ctx, table, sigs, t0, off)
    assert _same(got[off, 0], want), _where(got[off, 0], want)
    assert _same(_device(ctx, sigs, nf, t0=t0), got)
    s16 = ctx.tx_render(sigs, nf, t0=t0, format="s16")
    assert _same(s16[:, 0], X.quantise(got[:, 0])) and _same(_device(ctx, sigs, nf, fmt="s16", t0=t0), s16)


# ================================================================ 7. closed loop ==============================================
FDMA = [("K1ABC FN42 37", 497, 2.0), ("VE3EMB FN25 30", 1500, -3.0), ("PJ4/K1ABC 37", 2203, 1.0)]


@pytest.mark.gpu
def test_three_messages_on_three_carriers_decode_each_at_its_own(G, ctx):
    """one channel, three different messages at 497, 1500 and 2203 Hz, -20 dB in 2500 Hz each, 125 s: the multi-carrier
    pipe decodes every text at its own carrier and at no other"""
    sig = [{"text": t, "start": 375, "f0": f0, "carrier": fc} for t, fc, f0 in FDMA]
    n = 125 * 12000
    x = np.ascontiguousarray(ctx.tx_render(sig, n, sigma=G.tx_sigma(-20.0), seed=77)[:, 0])
    pipe = G.Pipe(batch_frames=8, max_per_frame=2, carriers=[497, 1500, 2203])
    try:
        for k in range(0, n, 500000):
            pipe.push_audio(x[k:k + 500000])
        pipe.flush()
        recs = pipe.collect(cap=1 << 16)
        planes = [pipe.split_plane(q) for q in range(3)]
    finally:
        pipe.close()
    assert planes == [(0, 497), (0, 1500), (0, 2203)]
    for q, (t, fc, _) in enumerate(FDMA):
        got = {G.unpack_message(r["message"])[1] for r in recs[(recs["channel"] == q) & (recs["decoded"] != 0)]}
        assert got == {G.unpack_message(G.wspr_pack(t))[1]}, (fc, got)


@pytest.mark.gpu
def test_encode_wav_with_carriers_then_decode_wav(G, tmp_path):
    p = str(tmp_path / "fdma.wav")
    G.encode_wav(p, [{"text": t, "start": 375, "f0": f0, "carrier": fc} for t, fc, f0 in FDMA], snr_db=-20.0, seed=5, seconds=125)
    out = G.decode_wav(p, carriers=[497, 1500, 2203], batch_frames=8, max_per_frame=2)
    assert {(d["carrier"], d["text"]) for d in out} == {(fc, G.unpack_message(G.wspr_pack(t))[1]) for t, fc, _ in FDMA}


# ================================================================ 8. refusals =================================================
@pytest.mark.gpu
def test_bad_carriers_fail_their_call_and_the_context_goes_on(G, ctx, ctx59):
    N = G.native
    good = _at(X.dense_signals(3000), 2203)
    t0, nf = X.dense_windows(3000)["middle"]
    ref = ctx.tx_render(good, 4096, t0=t0)
    before = G.tx_carrier_launch_counts()

    def refused(c, sigs, **kw):
        with pytest.raises(N.UwsprError) as e:
            c.tx_render(sigs, 4096, t0=t0, **kw)
        assert e.value.status == -6, e.value
        with pytest.raises(N.UwsprError) as e:
            c.tx_baseband(sigs, 100, t0=t0 // 32)
        assert e.value.status == -6, e.value
        assert _same(ctx.tx_render(good, 4096, t0=t0), ref)       # the context goes on
    refused(ctx, _at(good, 169))
    refused(ctx, _at(good, 2251))                                  # tx_cutoff - 249
    refused(ctx59, _at(good, 5651))
    refused(ctx, _at(good, -2203))
    ctx.tx_render(_at(good, 170), 4096, t0=t0)
    ctx.tx_render(_at(good, 2250), 4096, t0=t0)
    ctx59.tx_render(_at(good, 5650), 4096, t0=t0)
    ctx59.tx_render(_at(good, 2251), 4096, t0=t0)
    # 65 distinct carriers in one call; 64 pass
    many = [dict(good[0], carrier=200 + 7 * i, gain=0.1) for i in range(65)]
    refused(ctx, many)
    a = ctx.tx_render(many[:64], 4096, t0=t0)
    assert (a != 0).any()
    # a bad entry for a signal the window would have dropped is still refused
    far = dict(good[0], start=10 ** 9, carrier=169)
    refused(ctx, good + [far])
    assert _same(ctx.tx_render(good + [dict(far, carrier=170)], 4096, t0=t0), ref)
    # a cut-off under which 1500 Hz does not fit refuses the signals without a carrier as well
    low = G.Context(options={"tx_cutoff": 1000})
    try:
        with pytest.raises(N.UwsprError) as e:
            low.tx_render(X.dense_signals(3000), 4096, t0=t0)
        assert e.value.status == -6
        assert (low.tx_render(_at(X.dense_signals(3000), 497), 4096, t0=t0) != 0).any()
        for name, bad in (("tx_cutoff", 499), ("tx_cutoff", 5901), ("tx_form", 2), ("tx_form", -1)):
            with pytest.raises(N.UwsprError):
                low.set_option(name, bad)
        assert low.get_option("tx_cutoff") == 1000
    finally:
        low.close()
    assert G.tx_carrier_launch_counts()[0] > before[0]
