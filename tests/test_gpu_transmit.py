"""K7, the transmitter, on the device: .c2 baseband and 12 kS/s audio from message text, pinned against the reference's
own files (examples/VE3EMB.c2 and test_1500_Hz.wav, the output of examples/c2ToWaveFile.grc) and a float64 two-stage
restatement of the chain, and closed through the receiver."""
import ctypes as C
import math
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NTX = 162 * 256


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


def _loop():
    return np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))


# ---- float64 restatement of c2ToWaveFile.grc: baseband model, zero-stuff x32, h1, rotated h2, mixer, real part --------
def _baseband_file(G, sig, n):
    """the channel's baseband as the .c2 FILE holds it (conjugate of c2_read's), binary64"""
    x = np.zeros(n, np.complex128)
    for s in sig:
        sym = G.wspr_symbols(s["text"]).astype(np.float64)
        u = np.arange(NTX, dtype=np.float64)
        f = s.get("f0", 0.0) + (np.repeat(sym, 256) - 1.5) * 375.0 / 256 + s.get("drift", 0.0) * (u - (NTX - 1) / 2) / (NTX - 1)
        th = s.get("phase0", 0.0) + np.concatenate([[0.0], np.cumsum(2 * np.pi * f / 375.0)[:-1]])
        a, b = s["start"], s["start"] + NTX
        lo, hi = max(a, 0), min(b, n)
        if lo < hi:
            x[lo:hi] += s.get("gain", 1.0) * np.exp(-1j * th[lo - a:hi - a])
    return x


def _two_stage(x, nout):
    import scipy.signal as ss
    import frontend_grc as F
    h1 = F.low_pass(1, 12000, 200, 10).astype(np.float64)
    h2 = F.low_pass(1, 12000, 2500, 100)
    h2r = F.xlating_taps(h2, 1500.0).astype(np.complex128)
    u = np.zeros(len(x) * 32, np.complex128)
    u[::32] = x
    v = ss.oaconvolve(ss.oaconvolve(u, h1)[:len(u)], h2r)[:nout]
    return (v * np.exp(-1j * np.pi * np.arange(nout) / 4)).real


@pytest.mark.gpu
def test_baseband_is_the_reference_c2(G, ctx):
    import torch
    sig = [{"text": "VE3EMB FN25 30", "start": 375}]
    iq = ctx.tx_baseband(sig, 45000)
    ref, _, _ = G.c2_read(os.path.join(GOLDEN, "VE3EMB.c2"))
    assert np.abs(iq - ref).max() <= 1e-6
    assert (iq[:375] == 0).all() and (iq[375 + NTX:] == 0).all()
    dev = torch.empty((45000, 2), dtype=torch.float32, device="cuda:0")
    ctx.tx_baseband(sig, 45000, out=dev)
    assert (dev.cpu().numpy() == iq).all()
    part = ctx.tx_baseband(sig, 1000, t0=20000)
    assert (part == iq[20000:21000]).all()


@pytest.mark.gpu
def test_render_pins_the_reference_recording(G, ctx):
    tx = _loop()["tx"]
    a = ctx.tx_render([{"text": "VE3EMB FN25 30", "start": 375}], len(tx), format="s16")
    assert a.shape == (len(tx), 1) and a.dtype == np.int16
    d = a[:, 0].astype(np.int32) - tx.astype(np.int32)
    assert np.abs(d).max() <= 1, np.abs(d).max()
    assert np.mean(d == 0) >= 0.99, np.mean(d == 0)


@pytest.mark.gpu
def test_render_matches_the_two_stage_chain(G, ctx):
    rng = np.random.default_rng(11)
    texts = ["K1ABC FN42 37", "PJ4/K1ABC 37", "VE3EMB FN25 30", "G4XYZ/7 10", "W9ZZZ EM10 0"]
    Cn = 3
    sig = []
    for i in range(7):
        sig.append({"text": texts[i % len(texts)], "channel": int(rng.integers(0, Cn)), "start": int(rng.integers(0, 8000)),
                    "f0": float(rng.uniform(-80, 80)), "drift": float(rng.uniform(-4, 4)),
                    "phase0": float(rng.uniform(-np.pi, np.pi)), "gain": float(rng.uniform(0.2, 1.5))})
    t0, nf = 200000, 700000
    a = ctx.tx_render(sig, nf, t0=t0, channels=Cn)
    nbb = (t0 + nf) // 32 + 2
    for c in range(Cn):
        ref = _two_stage(_baseband_file(G, [s for s in sig if s["channel"] == c], nbb), t0 + nf)[t0:]
        err = np.abs(a[:, c].astype(np.float64) - ref).max()
        assert err <= 2e-6, (c, err)
    # before the signals the output is exact silence
    assert (ctx.tx_render(sig, 1000, t0=0, channels=Cn) == 0).all()


@pytest.mark.gpu
def test_renders_are_invariant_to_chunking_and_placement(G, ctx):
    import torch
    rng = np.random.default_rng(5)
    sig = [{"text": "K1ABC FN42 37", "channel": 0, "start": 100, "f0": 3.0},
           {"text": "VE3EMB FN25 30", "channel": 1, "start": 700, "f0": -2.0, "drift": 1.0}]
    bg = rng.integers(-3000, 3000, 12345).astype(np.int16)
    kw = dict(channels=2, sigma=[0.01, 0.02], seed=[9, 10], background=[bg, None], background_gain=0.5)
    t0, n = 31 * 1000 + 7, 150000
    for fmt in ("s16", "f32"):
        whole = ctx.tx_render(sig, n, t0=t0, format=fmt, **kw)
        parts, k = [], 0
        while k < n:
            ln = min(n - k, int(rng.choice([1, 2, 31, 32, 33, 1000, 16383, 16385, 40000])))
            parts.append(ctx.tx_render(sig, ln, t0=t0 + k, format=fmt, **kw))
            k += ln
        assert np.concatenate(parts).tobytes() == whole.tobytes(), fmt
        dev = torch.empty(whole.shape, dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
        dkw = dict(kw, background=[torch.from_numpy(bg).to("cuda:0"), None])
        ctx.tx_render(sig, n, t0=t0, format=fmt, out=dev, **dkw)
        assert dev.cpu().numpy().tobytes() == whole.tobytes(), fmt
    # host output of more than one staging piece (2^24 samples / C) is still the same bytes
    big = 9_000_000
    a = ctx.tx_render(sig, big, t0=0, channels=2, sigma=0.01, seed=3, format="s16")
    b = ctx.tx_render(sig, 5000, t0=big - 5000, channels=2, sigma=0.01, seed=3, format="s16")
    assert (a[-5000:] == b).all()


@pytest.mark.gpu
def test_noise_statistics_and_seeding(G, ctx):
    n = 10_000_000
    a = ctx.tx_render([], n, channels=2, sigma=1.0, seed=1234).astype(np.float64)
    for c in range(2):
        assert abs(a[:, c].mean()) < 0.01 and abs(a[:, c].var() - 1.0) < 0.01, (a[:, c].mean(), a[:, c].var())
    assert abs(np.mean(a[:, 0] * a[:, 1])) < 1e-3
    assert abs(np.mean(a[1:, 0] * a[:-1, 0])) < 1e-3
    x = ctx.tx_render([], 100000, t0=777, channels=1, sigma=0.5, seed=1)
    y = ctx.tx_render([], 100000, t0=777, channels=1, sigma=0.5, seed=1)
    z = ctx.tx_render([], 100000, t0=777, channels=1, sigma=0.5, seed=2)
    assert (x == y).all() and np.mean(x == z) < 1e-3


def _random_messages(rng, k):
    L = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    out = []
    for i in range(k):
        call = "".join(rng.choice(list(L), 2)) + str(int(rng.integers(0, 10))) + "".join(rng.choice(list(L), 3))
        p = int(rng.choice([0, 3, 7, 10, 23, 30, 37, 40, 50, 57, 60]))
        if i % 3 == 2:
            out.append("%s/%d %d" % (call, int(rng.integers(0, 10)), p))
        else:
            grid = rng.choice(list(L[:18])) + rng.choice(list(L[:18])) + str(int(rng.integers(0, 10))) + str(int(rng.integers(0, 10)))
            out.append("%s %s %d" % (call, grid, p))
    return out


@pytest.mark.gpu
def test_closed_loop_four_channels_three_slots(G, ctx):
    rng = np.random.default_rng(2024)
    # two-minute transmissions in slots 126 s apart: on the receiver's 9-s frame grid (hop 3375 samples), so that each
    # slot's transmission starts 1 s into one frame, as in a .c2 file
    Cn, slots, slot_s = 4, 3, 126
    msgs = _random_messages(rng, Cn * slots)
    sig, want = [], set()
    for c in range(Cn):
        for s in range(slots):
            t = msgs[c * slots + s]
            sig.append({"text": t, "channel": c, "start": 375 * slot_s * s + 375, "f0": float(rng.uniform(-6, 6))})
            want.add((c, s, G.unpack_message(G.wspr_pack(t))[1]))
    n = (slot_s * (slots - 1) + 122) * 12000
    x = ctx.tx_render(sig, n, channels=Cn, sigma=G.tx_sigma(-20.0), seed=77)
    pipe = G.Pipe(batch_frames=16, max_per_frame=4)
    try:
        for k in range(0, n, 1_000_000):
            pipe.push_audio(x[k:k + 1_000_000])
        pipe.flush()
        recs = pipe.collect(cap=1 << 16)
    finally:
        pipe.close()
    got = set()
    for r in recs[recs["decoded"] == 1]:
        c = int(r["channel"])
        text = G.unpack_message(r["message"])[1]
        got.add((c, int(round(int(r["stream_pos"]) / 375.0 / slot_s)), text))
    assert got == want, (sorted(got - want), sorted(want - got))


@pytest.mark.gpu
def test_the_flowgraph_demo_from_text(G, ctx):
    rec = _loop()
    n = len(rec["tx"])
    wh = rec["whales"]
    sig = [{"text": "VE3EMB FN25 30", "start": 375, "gain": float(rec["tx_gain"])}]
    a = ctx.tx_render(sig, n, background=wh, background_gain=float(rec["whales_gain"]))[:, 0]
    loop = (float(rec["tx_gain"]) * np.resize(rec["tx"].astype(np.float64) / 32768.0, n) +
            float(rec["whales_gain"]) * np.resize(wh.astype(np.float64) / 32768.0, n)).astype(np.float32)
    assert np.abs(a - loop).max() <= 2.0 / 32768
    pipe = G.Pipe(batch_frames=4)
    try:
        pipe.push_audio(a)
        pipe.flush()
        recs = pipe.collect()
    finally:
        pipe.close()
    texts = {G.unpack_message(r["message"])[1] for r in recs if r["decoded"]}
    assert texts == {"VE3EMB FN25 30"}, texts


@pytest.mark.gpu
def test_encode_wav_then_decode_wav(G, tmp_path):
    mono = [("K1ABC FN42 37", 0, 0, 2.0)]
    p = str(tmp_path / "mono.wav")
    G.encode_wav(p, mono)
    x, rate = G.read_wav(p)
    assert rate == 12000 and x.dtype == np.int16 and len(x) == 121 * 12000
    out = G.decode_wav(p, batch_frames=8)
    assert {d["text"] for d in out} == {"K1ABC FN42 37"} and 0.0 in {d["t"] for d in out}
    stereo = [("K1ABC FN42 37", 0, 0, 2.0), ("PJ4/K1ABC 37", 1, 0, -3.0), ("VE3EMB FN25 30", 1, 9, 0.5)]
    p = str(tmp_path / "stereo.wav")
    G.encode_wav(p, stereo, channels=2, snr_db=-15.0, seed=5)
    out = G.decode_wav(p, channels="all", batch_frames=8)
    assert {(d["channel"], d["text"]) for d in out} == {(c, t) for t, c, _, _ in stereo}
    assert {(d["channel"], d["text"], d["t"]) for d in out} >= {(c, t, float(s)) for t, c, s, _ in stereo}


@pytest.mark.gpu
def test_bad_arguments_fail_the_call_and_the_context_goes_on(G, ctx):
    N = G.native
    L = N.lib()
    sig = G.tx_signals([{"text": "K1ABC FN42 37", "channel": 1}])
    ch = (N.TxChannel * 65)()
    out = np.zeros((1000, 65), np.float32)
    o = C.c_void_p(out.ctypes.data)

    def render(s=sig, ns=1, C_=2, t0=0, nf=1000, fmt=0, where=0, chan=ch):
        return L.uwspr_tx_render(ctx.h, C.byref(s) if s is not None else None, ns, C.byref(chan) if chan is not None else None,
                                 C_, t0, nf, fmt, o, where)
    assert render() == 0
    for kw in (dict(C_=0), dict(C_=65), dict(C_=1), dict(t0=-1), dict(nf=-5), dict(fmt=2), dict(where=5),
               dict(chan=None), dict(ns=-1)):
        assert render(**kw) == -6, kw
    bad = G.tx_signals([{"text": "K1ABC FN42 37"}])
    bad[0].symbols[17] = 4
    assert render(s=bad) == -6
    bad = G.tx_signals([{"text": "K1ABC FN42 37", "f0": float("nan")}])
    assert render(s=bad) == -6
    ch[0].sigma = -1.0
    assert render() == -6
    ch[0].sigma = 0.0
    ch[0].background, ch[0].background_len = out.ctypes.data, 0
    assert render() == -6
    ch[0].background, ch[0].background_len = None, 0
    iq = np.zeros((10, 2), np.float32)
    assert L.uwspr_tx_baseband(ctx.h, C.byref(sig), 1, 0, 0, -1, C.c_void_p(iq.ctypes.data), 0) == -6
    assert L.uwspr_tx_baseband(ctx.h, C.byref(sig), 1, -1, 0, 10, C.c_void_p(iq.ctypes.data), 0) == -6
    assert "uwspr_tx" in L.uwspr_last_error(ctx.h).decode()
    with pytest.raises(G.UwsprError):
        ctx.tx_render([{"text": "K1ABC FN42 37", "channel": 3}], 100, channels=2)
    # the context still works: transmit and receive
    a = ctx.tx_render([{"text": "VE3EMB FN25 30", "start": 375}], len(_loop()["tx"]), format="s16")
    assert np.abs(a[:, 0].astype(np.int32) - _loop()["tx"]).max() <= 1
    iq = ctx.tx_baseband([{"text": "VE3EMB FN25 30", "start": 375}], 45000)
    cands, _ = ctx.pipeline_batch(iq[None], max_per_frame=1)
    assert len(cands[0]) > 0


@pytest.mark.gpu
def test_device_output_takes_host_backgrounds_and_refuses_host_pointers(G, ctx):
    """The device-resident closed loop with a host background (numpy, torch CPU) is made on the device: the background is
    moved there, the bytes are the host render's.  At the C ABI a host pointer with UWSPR_DEVICE is refused with
    UWSPR_ERR_ARG before any launch, as is a device range past its allocation, and the context goes on."""
    import torch
    N, L = G.native, G.native.lib()
    rec = _loop()
    wh = rec["whales"]
    sig = [{"text": "VE3EMB FN25 30", "start": 375, "gain": 0.1}]
    n = 200000
    host = ctx.tx_render(sig, n, background=wh, format="s16")
    for b in (wh, torch.from_numpy(wh), torch.from_numpy(wh).to("cuda:0"), [torch.from_numpy(wh)]):
        dev = torch.empty((n, 1), dtype=torch.int16, device="cuda:0")
        ctx.tx_render(sig, n, background=b, format="s16", out=dev)
        assert dev.cpu().numpy().tobytes() == host.tobytes()
    host_f = ctx.tx_baseband(sig, 5000)
    with pytest.raises(TypeError):
        ctx.tx_baseband(sig, 5000, out=torch.empty((5000, 2), dtype=torch.float16, device="cuda:0"))
    with pytest.raises(TypeError):
        ctx.tx_render(sig, 100, out=torch.empty((100, 1), dtype=torch.float64, device="cuda:0"))

    sigs = G.tx_signals(sig)
    out = torch.empty((n, 1), dtype=torch.int16, device="cuda:0")
    ch = (N.TxChannel * 1)()
    ch[0].background, ch[0].background_len, ch[0].background_format = wh.ctypes.data, wh.size, N.AUDIO_S16
    assert L.uwspr_tx_render(ctx.h, C.byref(sigs), 1, C.byref(ch), 1, 0, n, N.AUDIO_S16, C.c_void_p(out.data_ptr()),
                             N.DEVICE) == -6
    assert "background" in L.uwspr_last_error(ctx.h).decode()
    small = torch.zeros(1000, dtype=torch.int16, device="cuda:0")
    ch[0].background, ch[0].background_len = small.data_ptr(), 1 << 40          # past its allocation
    assert L.uwspr_tx_render(ctx.h, C.byref(sigs), 1, C.byref(ch), 1, 0, n, N.AUDIO_S16, C.c_void_p(out.data_ptr()),
                             N.DEVICE) == -6
    ch[0].background, ch[0].background_len = None, 0
    h_out = np.zeros((n, 1), np.int16)
    assert L.uwspr_tx_render(ctx.h, C.byref(sigs), 1, C.byref(ch), 1, 0, n, N.AUDIO_S16, C.c_void_p(h_out.ctypes.data),
                             N.DEVICE) == -6
    iq = np.zeros((5000, 2), np.float32)
    assert L.uwspr_tx_baseband(ctx.h, C.byref(sigs), 1, 0, 0, 5000, C.c_void_p(iq.ctypes.data), N.DEVICE) == -6
    assert (h_out == 0).all() and (iq == 0).all()
    # the context goes on
    again = ctx.tx_render(sig, n, background=wh, format="s16")
    assert again.tobytes() == host.tobytes() and (ctx.tx_baseband(sig, 5000) == host_f).all()
