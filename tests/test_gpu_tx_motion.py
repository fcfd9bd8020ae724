"""K7 with a moving source (uwspr_tx_baseband_moving, uwspr_tx_render_moving): the straight-line model of
include/uwspr_hip.h against a float64 numpy restatement, the sign and scale of its Doppler against the receiver's own
slmFrequencyDrift, the audio against the float64 two-stage chain, and closed through the coarse search and the decoder."""
import ctypes as C

import numpy as np
import pytest

NTX = 162 * 256
DF = 375.0 / 512


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


# ---- float64 restatement of the model (include/uwspr_hip.h, uwspr_tx_motion) ------------------------------------------
def _theta(G, s, kp):
    """the static phase at (fractional) transmission index kp: per-symbol phases from the exclusive accumulation of
    per-sample frequencies, the per-symbol quadratic within a symbol"""
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


def _model(G, sigs, n, t0=0):
    """the channel's baseband [t0, t0 + n) in uwspr_tx_baseband's orientation (gain e^{+j phase}), binary64"""
    y = np.zeros(n, np.complex128)
    j = np.arange(t0, t0 + n, dtype=np.int64)
    for s in sigs:
        m = s.get("motion") or {}
        model = m.get("model", "static") if m else "static"
        k = (j - s["start"]).astype(np.float64)
        gain = s.get("gain", 1.0)
        if model == "static":
            ok = (k >= 0) & (k < NTX)
            y[ok] += gain * np.exp(1j * _theta(G, s, k[ok]))
            continue
        (v1, v2), (p1, p2), tf = m["v"], m["p"], m.get("t", 0.0)
        t = tf + k / 375.0
        R = np.hypot(v1 * t + p1, v2 * t + p2)
        R0 = np.hypot(v1 * tf + p1, v2 * tf + p2)
        D = (R - (0.0 if m.get("absolute") else R0)) / 1500.0
        kp = k - 375.0 * D if model == "delay" else k
        ok = (kp >= 0) & (kp < NTX)
        amp = gain * (R0 / R if m.get("spreading") else 1.0)
        ph = _theta(G, s, kp[ok]) - 2 * np.pi * 1500.0 * D[ok]
        y[ok] += (amp * np.ones_like(k))[ok] * np.exp(1j * ph)
    return y


def _two_stage(x_file, nout):
    """c2ToWaveFile.grc in float64 on the baseband as the .c2 FILE holds it (test_gpu_transmit's restatement)"""
    import scipy.signal as ss
    import frontend_grc as F
    h1 = F.low_pass(1, 12000, 200, 10).astype(np.float64)
    h2 = F.low_pass(1, 12000, 2500, 100)
    h2r = F.xlating_taps(h2, 1500.0).astype(np.complex128)
    u = np.zeros(len(x_file) * 32, np.complex128)
    u[::32] = x_file
    v = ss.oaconvolve(ss.oaconvolve(u, h1)[:len(u)], h2r)[:nout]
    return (v * np.exp(-1j * np.pi * np.arange(nout) / 4)).real


def _cplx(iq):
    return iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)


def _motion(traj, model="doppler", **kw):
    return dict({"v": (float(traj[0]), float(traj[1])), "p": (float(traj[2]), float(traj[3])), "model": model}, **kw)


# ---- 1. identity -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_motion_static_and_zero_velocity_are_the_static_bytes(G, ctx):
    import torch
    N, L = G.native, G.native.lib()
    base = [{"text": "K1ABC FN42 37", "channel": 0, "start": 300, "f0": 2.5, "drift": 1.3, "phase0": 0.7, "gain": 0.8},
            {"text": "VE3EMB FN25 30", "channel": 1, "start": 1234, "f0": -4.0, "drift": -0.6, "phase0": -2.0},
            {"text": "PJ4/K1ABC 37", "channel": 0, "start": 9000, "f0": 0.3, "gain": 0.5}]
    n_bb, n_au = 50000, 1_500_000
    ref_bb = [ctx.tx_baseband(base, n_bb, channel=c) for c in (0, 1)]
    ref_au = {fmt: ctx.tx_render(base, n_au, channels=2, sigma=0.01, seed=3, format=fmt) for fmt in ("s16", "f32")}
    # motion = NULL at the C ABI
    sig = G.tx_signals(base)
    iq = np.zeros((n_bb, 2), np.float32)
    assert L.uwspr_tx_baseband_moving(ctx.h, C.byref(sig), None, 3, 0, 0, n_bb, C.c_void_p(iq.ctypes.data), N.HOST) == 0
    assert iq.tobytes() == ref_bb[0].tobytes()
    ch = (N.TxChannel * 2)()
    a = np.zeros((n_au, 2), np.int16)
    assert L.uwspr_tx_render_moving(ctx.h, C.byref(sig), None, 3, C.byref(ch), 2, 0, n_au, N.AUDIO_S16,
                                    C.c_void_p(a.ctypes.data), N.HOST) == 0
    assert a.tobytes() == ctx.tx_render(base, n_au, channels=2, format="s16").tobytes()
    motions = [{"model": "static", "v": (1.0, 2.0), "p": (3.0, 40.0)}]
    for model in ("doppler", "delay"):
        motions.append({"v": (0.0, 0.0), "p": (120.0, -35.0), "t": 17.0, "model": model})
        motions.append({"v": (0.0, -0.0), "p": (0.0, 850.0), "model": model, "spreading": True})
    for mo in motions:
        sigs = [dict(s, motion=mo) for s in base]
        for c in (0, 1):
            assert ctx.tx_baseband(sigs, n_bb, channel=c).tobytes() == ref_bb[c].tobytes(), (mo, c)
            dev = torch.empty((n_bb, 2), dtype=torch.float32, device="cuda:0")
            ctx.tx_baseband(sigs, n_bb, channel=c, out=dev)
            assert dev.cpu().numpy().tobytes() == ref_bb[c].tobytes(), (mo, c)
        for fmt in ("s16", "f32"):
            a = ctx.tx_render(sigs, n_au, channels=2, sigma=0.01, seed=3, format=fmt)
            assert a.tobytes() == ref_au[fmt].tobytes(), (mo, fmt)
            dev = torch.empty(a.shape, dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
            ctx.tx_render(sigs, n_au, channels=2, sigma=0.01, seed=3, format=fmt, out=dev)
            assert dev.cpu().numpy().tobytes() == ref_au[fmt].tobytes(), (mo, fmt)


# ---- 2. the model, sample by sample -----------------------------------------------------------------------------------
TRAJS = [(2.0, -2.0, 0.0, 50.0),      # |V| = 2 sqrt 2, closest approach (35 m) at t = 12.5 s, inside the transmission
         (-2.0, -2.0, 0.0, 50.0),
         (-1.0, 2.0, 0.0, 450.0),
         (1.5, -0.5, 30.0, 850.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["doppler", "delay"])
def test_baseband_matches_the_float64_model(G, ctx, model):
    import torch
    n = 45600
    for i, tr in enumerate(TRAJS):
        for flags in ({}, {"absolute": True}, {"spreading": True}, {"absolute": True, "spreading": True}):
            tf = 7.3 if i == 3 else 0.0
            s = [{"text": "K1ABC FN42 37", "start": 375, "f0": 3.1 - i, "drift": 1.7, "phase0": 0.4, "gain": 0.9,
                  "motion": _motion(tr, model, t=tf, **flags)}]
            got = ctx.tx_baseband(s, n)
            ref = _model(G, s, n)
            err = max(np.abs(got[:, 0] - ref.real).max(), np.abs(got[:, 1] - ref.imag).max())
            assert err <= 2e-6, (tr, flags, err)
            if model == "delay" and not flags:
                assert (got[:375] == 0).all() and np.abs(got[375 + 200:375 + NTX - 200]).min() > 0
            part = ctx.tx_baseband(s, 1001, t0=20017)
            assert part.tobytes() == got[20017:21018].tobytes()
            dev = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
            ctx.tx_baseband(s, n, out=dev)
            assert dev.cpu().numpy().tobytes() == got.tobytes()


# ---- 3. sign and scale against the receiver's model ------------------------------------------------------------------
@pytest.mark.gpu
def test_doppler_is_slm_frequency_drift_on_every_grid_trajectory(G, ctx):
    grid = G.slm_trajectories()
    static = [{"text": "VE3EMB FN25 30", "start": 0, "f0": 1.5}]
    x = _cplx(ctx.tx_baseband(static, NTX))
    dx = np.angle(x[1:] * np.conj(x[:-1]))
    t_mid = (np.arange(NTX - 1) + 0.5) / 375.0
    worst = 0.0
    for tr in grid:
        y = _cplx(ctx.tx_baseband([dict(static[0], motion=_motion(tr))], NTX))
        dphi = np.angle(np.exp(1j * (np.angle(y[1:] * np.conj(y[:-1])) - dx)))
        err = np.abs(dphi * 375.0 / (2 * np.pi) - G.slm_drift(tr, t_mid)).max()
        worst = max(worst, err)
        assert err <= 1e-3, (tr, err)
    assert worst > 0.0


# ---- 4. audio ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_moving_audio_matches_the_two_stage_chain_and_is_invariant_to_chunking(G, ctx):
    import torch
    sigs = [{"text": "K1ABC FN42 37", "channel": 0, "start": 500, "f0": 2.0, "drift": 0.5, "phase0": 0.3,
             "motion": _motion(TRAJS[0], "delay", spreading=True)},
            {"text": "VE3EMB FN25 30", "channel": 0, "start": 2000, "f0": -3.0, "gain": 0.6,
             "motion": _motion(TRAJS[2], "doppler")},
            {"text": "PJ4/K1ABC 37", "channel": 1, "start": 100, "f0": 1.0,
             "motion": _motion(TRAJS[3], "delay", absolute=True, t=4.0)},
            {"text": "W9ZZZ EM10 0", "channel": 1, "start": 700, "f0": -1.0, "gain": 0.5}]
    t0, nf = 300_000, 600_000
    nbb = (t0 + nf) // 32 + 2
    f32 = ctx.tx_render(sigs, nf, t0=t0, channels=2)
    s16 = ctx.tx_render(sigs, nf, t0=t0, channels=2, format="s16")
    for c in range(2):
        ref = _two_stage(np.conj(_model(G, [s for s in sigs if s["channel"] == c], nbb)), t0 + nf)[t0:]
        err = np.abs(f32[:, c].astype(np.float64) - ref).max()
        assert err <= 1e-6, (c, err)
        q = np.clip(np.rint(32767.0 * ref), -32768, 32767)
        assert np.abs(s16[:, c].astype(np.int64) - q).max() <= 1, c
    rng = np.random.default_rng(8)
    kw = dict(channels=2, sigma=[0.01, 0.0], seed=[4, 5])
    for fmt in ("s16", "f32"):
        whole = ctx.tx_render(sigs, nf, t0=t0, format=fmt, **kw)
        parts, k = [], 0
        while k < nf:
            ln = min(nf - k, int(rng.choice([1, 31, 33, 1000, 16383, 16385, 70001])))
            parts.append(ctx.tx_render(sigs, ln, t0=t0 + k, format=fmt, **kw))
            k += ln
        assert np.concatenate(parts).tobytes() == whole.tobytes(), fmt
        dev = torch.empty(whole.shape, dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
        ctx.tx_render(sigs, nf, t0=t0, format=fmt, out=dev, **kw)
        assert dev.cpu().numpy().tobytes() == whole.tobytes(), fmt


# ---- 5. closed loop through the coarse search ------------------------------------------------------------------------
def _offsets(info, traj, ifr, cf=1500.0):
    """ifd - ifr, k = 0..161, as FDR_impl.cc:382-385 quantises a trajectory: t = k*111/162 (integers), slmFrequencyDrift
    in binary64 returned as binary32, (int)((float)ifr + drift / df) in binary32"""
    V1, V2, p1, p2 = (float(x) for x in traj)
    df = np.float32(info.df)
    out = np.zeros(162, np.int64)
    for k in range(162):
        t = float(k * 111 // 162)
        q1, q2 = V1 * t + p1, V2 * t + p2
        sign = 1.0 if (q1 * V1 + q2 * V2) > 0 else -1.0
        den = np.sqrt(q1 * q1 + q2 * q2)
        d = np.float32(0.0) if den == 0 else np.float32(-sign * abs(V1 * q1 + V2 * q2) / den * cf / 1500.0)
        out[k] = int(np.float32(np.float32(ifr) + np.float32(d / df))) - ifr
    return out


# Grid indices (slmGenerator order) whose noise-free DOPPLER render gives, at threshold 1, a nonlinear candidate at
# freq == f0 with the transmitted bin-offset sequence: profiles/moving_source.txt, table 2, column "thr1 seq" (all four
# it measured: (V1, V2, p2) = (-2, -2, 250), (2, -2, 250), (-1, -1, 50), (1, -1, 50)).
COARSE = [1, 21, 30, 40]


@pytest.mark.gpu
def test_coarse_search_finds_the_transmitted_trajectory(G, ctx):
    import torch
    N = G.native
    grid = G.slm_trajectories()
    f0 = 4 * DF
    nin = 45000 * 32
    audio = torch.zeros((len(COARSE), nin), dtype=torch.float32, device="cuda:0")
    for b, i in enumerate(COARSE):
        ctx.tx_render([{"text": "K1ABC FN42 37", "start": 375, "f0": f0, "motion": _motion(grid[i])}], nin, out=audio[b])
    rx = G.Context(threshold=1)
    try:
        cands = rx.fdr_batch(rx.frontend(audio))
        info = rx.info
        for b, i in enumerate(COARSE):
            hits = []
            for c in cands[b]:
                if int(c["m_type"]) != N.NONLINEAR or c["freq"] != np.float32(f0):
                    continue
                ifr = info.m + int(round(float(c["freq"]) / float(info.df)))
                hits.append((_offsets(info, (c["V1"], c["V2"], c["p1"], c["p2"]), ifr) == _offsets(info, grid[i], ifr)).all())
            assert any(hits), (i, grid[i], cands[b][["freq", "m_type", "V1", "V2", "p2"]])
    finally:
        rx.close()


# ---- 6. closed loop through the decoder -------------------------------------------------------------------------------
def _decode(G, x, batch_frames=8):
    pipe = G.Pipe(batch_frames=batch_frames)
    try:
        pipe.push_audio(x)
        pipe.flush()
        recs = pipe.collect()
    finally:
        pipe.close()
    return {(int(r["channel"]), G.unpack_message(r["message"])[1]) for r in recs if r["decoded"]}


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["doppler", "delay"])
def test_a_mild_trajectory_decodes(G, ctx, model):
    text = "K1ABC FN42 37"
    s = [{"text": text, "start": 375, "f0": 1.0, "motion": _motion((1.0, 0.0, 0.0, 850.0), model)}]
    x = ctx.tx_render(s, 122 * 12000, sigma=G.tx_sigma(-20.0), seed=12, format="s16")[:, 0]
    assert (0, text) in _decode(G, x)


@pytest.mark.gpu
def test_a_four_hydrophone_array_decodes_on_every_channel(G, ctx):
    text = "VE3EMB FN25 30"
    phones = [(0.0, 0.0), (100.0, 0.0), (0.0, 100.0), (100.0, 100.0)]
    s = [{"text": text, "channel": c, "start": 375, "f0": -2.0,
          "motion": {"v": (1.0, -0.5), "p": (-60.0 - x, 700.0 - y), "model": "delay", "absolute": True,
                     "spreading": True}} for c, (x, y) in enumerate(phones)]
    clean = ctx.tx_baseband(s, 45000 + 1000, channel=0), ctx.tx_baseband(s, 45000 + 1000, channel=3)
    first = [int(np.argmax(np.abs(b[:, 0]) > 0)) for b in clean]
    assert 375 + 150 < first[1] < first[0]   # the travel time: 703 m to hydrophone 0, 621 m to hydrophone 3
    x = ctx.tx_render(s, 123 * 12000, channels=4, sigma=G.tx_sigma(-20.0), seed=[1, 2, 3, 4], format="s16")
    assert _decode(G, x) == {(c, text) for c in range(4)}


# ---- 7. errors --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_motions_fail_only_their_call(G, ctx):
    N, L = G.native, G.native.lib()
    good = [{"text": "K1ABC FN42 37", "start": 375, "f0": 1.0, "motion": _motion(TRAJS[0], "delay")}]
    want_bb = ctx.tx_baseband(good, 45000)
    want_au = ctx.tx_render(good, 200000, format="s16")
    sig = G.tx_signals(good)
    ch = (N.TxChannel * 1)()
    bad = []
    for f in ("v1", "v2", "p1", "p2", "t_first"):
        for v in (float("nan"), float("inf")):
            bad.append({f: v})
    bad += [{"model": 3}, {"model": -1}, {"flags": 4}, {"flags": 1 << 30}, {"v1": 80.0, "v2": 61.0},
            {"v1": 0.0, "v2": -100.5}, {"t_first": 1e6 + 1}, {"t_first": -2e6},
            {"v1": 0.0, "v2": 0.0, "p1": 0.3, "p2": 0.5, "flags": 2},
            {"v1": 1.0, "v2": 0.0, "p1": -50.0, "p2": 0.5, "flags": 2, "model": 1},   # passes 0.5 m at t = 50 s
            {"v1": 1.0, "v2": 0.0, "p1": -50.0, "p2": 0.5, "flags": 3, "model": 2},
            {"model": 0, "p1": float("nan")}]
    for b in bad:
        mot = G.tx_motions(good)
        for k, v in b.items():
            setattr(mot[0], k, v)
        iq = np.full((45000, 2), 7.0, np.float32)
        assert L.uwspr_tx_baseband_moving(ctx.h, C.byref(sig), C.byref(mot), 1, 0, 0, 45000,
                                          C.c_void_p(iq.ctypes.data), N.HOST) == -6, b
        assert (iq == 7.0).all()
        a = np.full((200000, 1), 7, np.int16)
        assert L.uwspr_tx_render_moving(ctx.h, C.byref(sig), C.byref(mot), 1, C.byref(ch), 1, 0, 200000, N.AUDIO_S16,
                                        C.c_void_p(a.ctypes.data), N.HOST) == -6, b
        assert (a == 7).all()
        assert "motion" in L.uwspr_last_error(ctx.h).decode()
        assert ctx.tx_baseband(good, 45000).tobytes() == want_bb.tobytes()
    assert ctx.tx_render(good, 200000, format="s16").tobytes() == want_au.tobytes()
    with pytest.raises(G.UwsprError):
        ctx.tx_render([dict(good[0], motion=dict(good[0]["motion"], v=(90.0, 90.0)))], 1000)
    with pytest.raises(ValueError):
        G.tx_motions([dict(good[0], motion={"velocity": (1, 2)})])


@pytest.mark.gpu
def test_encode_wav_takes_a_moving_source(G, ctx, tmp_path):
    passing = {"text": "VE3EMB FN25 30", "start": 375, "f0": 2.0,
               "motion": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "delay", "spreading": True}}
    p = str(tmp_path / "passing.wav")
    G.encode_wav(p, [passing, ("K1ABC FN42 37", 0, 0, -3.0)], ctx=ctx)
    x, rate = G.read_wav(p)
    ref = ctx.tx_render([passing, {"text": "K1ABC FN42 37", "start": 375, "f0": -3.0}], 121 * 12000, format="s16")
    assert rate == 12000 and x.tobytes() == ref[:, 0].tobytes()
