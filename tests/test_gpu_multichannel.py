"""Multichannel audio through one pipe (uwspr_pipe_push_audio_channels, Pipe.push_audio on [n, C] arrays): C
interleaved 12 kS/s channels go through one K0 launch per piece into C planes of the pipe's ring, and every take is
searched as C single-channel batches.

Each output of K0's multichannel form has the arithmetic of the one-channel kernel, and a channel's batches are its own
frames, so channel c of a C-channel pipe must give, byte for byte, the records of a one-channel pipe fed channel c
alone (with the record's channel field = c).  The checks hold that across channel counts, both tap modes, both sample
formats and formats mixing, random piece lengths (single frames; pieces longer than a K0 launch), the ring's plane
tail moves and argument errors; the demos decode on the channel that carries them; a stereo WAV decodes per channel."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN

HOP, FL = 3375, 45000
OPTS = dict(hop=HOP, batch_frames=3, max_per_frame=2, lanes=3)


def _recording_s16():
    return np.load(os.path.join(GOLDEN, "150613_1920_int16.npz"))["x"]


def _closed_loop_s16(n):
    """examples/WaveFilePlusNoiseDecode.grc's mix (tx x 0.1 + whales, both repeating), as int16"""
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    x = float(rec["tx_gain"]) * tx + float(rec["whales_gain"]) * wh
    return np.clip(np.rint(x.astype(np.float32) * 32768.0), -32768, 32767).astype(np.int16)


def _noise_s16(n, seed, sigma=3000.0):
    x = np.random.default_rng(seed).standard_normal(n) * sigma
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _content(c, n):
    """channel c's distinct content: the recording, the closed-loop mix, noise (seed by c), a shifted recording"""
    kind = c % 4
    if kind == 0:
        return np.resize(_recording_s16(), n)
    if kind == 1:
        return _closed_loop_s16(n)
    if kind == 2:
        return _noise_s16(n, 200 + c)
    return np.resize(np.concatenate([_noise_s16(3 * HOP * 32 + 1000 * c, 300 + c, 300.0), _recording_s16()]), n)


def _f32(x):
    return (x.astype(np.float32) / np.float32(32768)).astype(np.float32)


def _pieces(n, seed, big=400000):
    """random piece lengths: single frames, short pieces, pieces longer than one K0 launch of the pipe"""
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < n:
        r = rng.random()
        k = 1 if r < 0.15 else int(rng.integers(2, 5000)) if r < 0.5 else int(rng.integers(5000, big))
        k = min(k, n - pos)
        out.append((pos, k))
        pos += k
    return out


def _run(G, feed, mode=0, **opts):
    o = dict(OPTS)
    o.update(opts)
    pipe = G.Pipe(**o)
    try:
        if mode:
            pipe.set_option("frontend", mode)
        feed(pipe)
        pipe.flush()
        return pipe.collect(cap=1 << 20), pipe.stats()
    finally:
        pipe.close()


_ONE = {}


def _one(G, x, mode=0, **opts):
    """the records of a one-channel pipe fed x (cached by content and options)"""
    key = (x.tobytes(), mode, tuple(sorted(opts.items())))
    if key not in _ONE:
        def feed(pipe):
            for k in range(0, x.size, 250000):
                pipe.push_audio(x[k: k + 250000])
        _ONE[key] = _run(G, feed, mode, **opts)[0]
    return _ONE[key]


def _frames(n, mode=0):
    """frames of a one-channel stream of n audio samples: output m needs x[32 m + D] (D = 0 / 512)"""
    outputs = (n - 1 - (512 if mode else 0)) // 32 + 1
    return (outputs - FL) // HOP + 1


def _check_order(recs, nch):
    """(take, channel, frame): a take ends where the channel goes down; frames rise within a channel and from one take
    to the next"""
    last = {}
    take_max, prev_max, prev_c = -1, -1, None
    for r in recs:
        c, f = int(r["channel"]), int(r["frame"])
        assert 0 <= c < nch
        if prev_c is not None and c < prev_c:
            prev_max = take_max
        assert f > prev_max, (c, f, prev_max)
        assert f >= last.get(c, -1)
        last[c] = f
        take_max = max(take_max, f)
        prev_c = c


def _assert_channels_equal_one_channel(G, recs, X, mode=0, **opts):
    nch = X.shape[1]
    assert len(recs) > 0 and (recs["channel"] >= 0).all() and (recs["channel"] < nch).all()
    for c in range(nch):
        got = recs[recs["channel"] == c].copy()
        got["channel"] = 0
        want = _one(G, np.ascontiguousarray(X[:, c]), mode, **opts)
        assert len(got) == len(want), (c, len(got), len(want))   # (a noise channel may have no candidate at all)
        assert got.tobytes() == want.tobytes(), c
        assert (got["stream_pos"] == got["frame"] * HOP).all()


# ---- 1. channel c is a one-channel pipe fed channel c ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nch", [2, 3, 8])
def test_every_channel_equals_its_one_channel_pipe(G, nch, mode):
    n = 185 * 12000
    X = np.stack([_content(c, n) for c in range(nch)], axis=1)
    for fmt in ("s16", "f32"):
        src = X if fmt == "s16" else _f32(X)

        def feed(pipe):
            for pos, k in _pieces(n, 10 * nch + mode + (fmt == "f32")):
                pipe.push_audio(src[pos: pos + k])
        recs, st = _run(G, feed, mode)
        _check_order(recs, nch)
        _assert_channels_equal_one_channel(G, recs, X, mode)
        assert st["frames"] == nch * _frames(n, mode)


# ---- 2. one channel through the channels entry point is push_audio ------------------------------------------------------
@pytest.mark.gpu
def test_one_channel_through_the_channels_call_is_push_audio(G):
    x = _closed_loop_s16(200 * 12000)
    pieces = _pieces(x.size, 5)

    def flat(pipe):
        for pos, k in pieces:
            pipe.push_audio(x[pos: pos + k])

    def two_d(pipe):
        for pos, k in pieces:
            pipe.push_audio(x[pos: pos + k, None])
    a, sa = _run(G, flat)
    b, sb = _run(G, two_d)
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    assert (a["channel"] == 0).all() and sa["frames"] == sb["frames"]


# ---- 3. decodes land on the channel that carries them -------------------------------------------------------------------
def _texts(G, recs, channel, frame=None):
    return {G.unpack_message(r["message"])[1] for r in recs
            if r["decoded"] and r["channel"] == channel and (frame is None or r["frame"] == frame)}


@pytest.mark.gpu
def test_decodes_land_on_their_channel(G):
    lead = 3 * HOP * 32
    n = lead + _recording_s16().size + 20 * 12000
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))   # the closed loop in float, as its demo pushes it
    loop = (float(rec["tx_gain"]) * np.resize(rec["tx"].astype(np.float64) / 32768.0, n) +
            float(rec["whales_gain"]) * np.resize(rec["whales"].astype(np.float64) / 32768.0, n)).astype(np.float32)
    X = np.stack([loop,
                  _f32(_noise_s16(n, 90)),
                  _f32(np.concatenate([_noise_s16(lead, 91, 300.0), _recording_s16(), _noise_s16(20 * 12000, 92, 300.0)])),
                  _f32(_noise_s16(n, 93))], axis=1)

    def feed(pipe):
        for k in range(0, n, 250000):
            pipe.push_audio(X[k: k + 250000])
    recs, _ = _run(G, feed, batch_frames=8)
    fn25 = {c for c in range(4) if "VE3EMB FN25 30" in _texts(G, recs, c)}
    fn42 = {c for c in range(4) if "VE3EMB FN42 33" in _texts(G, recs, c)}
    assert fn25 == {0} and fn42 == {2}, (fn25, fn42)
    assert "VE3EMB FN42 33" in _texts(G, recs, 2, frame=3)
    assert "VE3EMB FN25 30" in _texts(G, recs, 0, frame=0)


# ---- 4. the plane tail moves ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plane_compaction(G):
    # per plane: (ceil(3 / 4) + 3) takes of 4 frames + fl = 99000 pairs, 264 s of audio; 800 s moves the tail ~3 times
    n = 800 * 12000
    X = np.stack([_content(c, n) for c in (1, 2, 3, 6)], axis=1)
    opts = dict(batch_frames=4, lanes=3, max_per_frame=1)

    def feed(pipe):
        for pos, k in _pieces(n, 44, big=1500000):
            pipe.push_audio(X[pos: pos + k])
    recs, st = _run(G, feed, **opts)
    _check_order(recs, 4)
    _assert_channels_equal_one_channel(G, recs, X, **opts)
    assert st["frames"] == 4 * _frames(n)


# ---- 5. argument errors are not sticky ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_are_not_sticky(G):
    N = G.native
    n = 160 * 12000
    X = np.stack([_content(c, n) for c in range(3)], axis=1)
    want, _ = _run(G, lambda p: p.push_audio(X))

    def raw(pipe, arr, nframes, nch, fmt):
        return pipe.L.uwspr_pipe_push_audio_channels(pipe.h, C.c_void_p(arr.ctypes.data), nframes, nch, fmt)

    def err(pipe):
        return pipe.L.uwspr_pipe_last_error(pipe.h).decode()

    pipe = G.Pipe(**OPTS)
    try:
        assert raw(pipe, X, 1000, 0, N.AUDIO_S16) == -6 and "nchannels" in err(pipe)
        assert raw(pipe, X, 1000, 65, N.AUDIO_S16) == -6 and "nchannels" in err(pipe)
        pipe.push_audio(X[:500000])
        X2 = np.ascontiguousarray(X[:, :2])
        assert raw(pipe, X2, 1000, 2, N.AUDIO_S16) == -6 and "channels" in err(pipe)
        with pytest.raises(N.UwsprError) as e:
            pipe.push(np.zeros((100, 2), np.float32))      # (I,Q) into an audio pipe
        assert e.value.status == -6
        seg = np.ascontiguousarray(X[500000:600000])
        assert raw(pipe, seg, seg.shape[0], 3, 7) == -6 and "format" in err(pipe)
        with pytest.raises(N.UwsprError) as e:
            pipe.push_audio(X[500000:600000, 0])            # one channel into a three-channel stream
        assert e.value.status == -6
        pipe.push_audio(X[500000:])
        pipe.flush()
        got = pipe.collect(cap=1 << 20)
    finally:
        pipe.close()
    assert len(want) > 0 and got.tobytes() == want.tobytes()

    # an (I,Q) pipe refuses audio and goes on
    iq = np.random.default_rng(95).standard_normal((FL + 2 * HOP, 2)).astype(np.float32)

    def iq_feed(pipe, bad):
        pipe.push(iq[:1000])
        if bad:
            assert raw(pipe, X, 1000, 2, N.AUDIO_S16) == -6 and "(I,Q)" in err(pipe)
        pipe.push(iq[1000:])
    ok, _ = _run(G, lambda p: iq_feed(p, False))
    bad, st = _run(G, lambda p: iq_feed(p, True))
    assert st["frames"] == 3 and bad.tobytes() == ok.tobytes() and (bad["channel"] == 0).all()


# ---- 6. formats mix between pushes ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_formats(G):
    n = 170 * 12000
    X = np.stack([_content(c, n) for c in (3, 1, 2)], axis=1)
    Xf = _f32(X)
    cuts = [0, 700001, 1300003, n]

    def feed(pipe):
        pipe.push_audio(X[cuts[0]: cuts[1]])
        pipe.push_audio(Xf[cuts[1]: cuts[2]])
        pipe.push_audio(X[cuts[2]: cuts[3]])
    recs, _ = _run(G, feed)
    _check_order(recs, 3)
    _assert_channels_equal_one_channel(G, recs, X)


# ---- 7. a stereo WAV ------------------------------------------------------------------------------------------------------
def _write_wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(np.ascontiguousarray(x).tobytes())


@pytest.mark.gpu
def test_stereo_wav_decodes_per_channel(G, tmp_path):
    lead = 3 * HOP * 32
    rec = np.concatenate([_noise_s16(lead, 80, 300.0), _recording_s16(), _noise_s16(12000 * 20, 81, 300.0)])
    X = np.stack([_noise_s16(rec.size, 82), rec], axis=1)
    path = tmp_path / "stereo.wav"
    _write_wav(path, X)
    dec = G.decode_wav(path, channels="all", max_per_frame=2)
    hits = [d for d in dec if d["text"] == "VE3EMB FN42 33"]
    assert hits and all(d["channel"] == 1 for d in hits), dec
    assert any(d["t"] == 27.0 and d["frame"] == 3 for d in hits), dec
    # the default call is channel 0 alone, as a mono file of it decodes
    mono = tmp_path / "ch0.wav"
    _write_wav(mono, X[:, 0])
    d0 = G.decode_wav(path, max_per_frame=2)
    assert d0 == G.decode_wav(mono, max_per_frame=2)
    assert all("channel" not in d for d in d0)


# ---- device memory of a 64-channel pipe --------------------------------------------------------------------------------
def _ingest_bytes(nch, batch_frames=256, hop=HOP, fl=FL, lanes=9, J=216):
    """the header's formula: the ring's two buffers of nch planes and K0's two interleaved audio buffers"""
    plane = ((lanes + nch - 1) // nch + 3) * batch_frames * hop + fl
    if nch > 1:
        plane = (plane + 63) // 64 * 64
    return 2 * nch * plane * 8 + 2 * ((32 * J + 32) * nch + (4 << 20)) * 4


@pytest.mark.gpu
def test_64_channels_memory_and_decode(G):
    import torch
    nch = 64
    n = 122 * 12000
    X = np.stack([_noise_s16(n, 500 + c, 1000.0) for c in range(nch)], axis=1)
    pipe = G.Pipe(hop=HOP)
    try:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        pipe.push_audio(X[:1])                           # the ring and K0's buffers, one output, no batch yet
        torch.cuda.synchronize()
        used = free0 - torch.cuda.mem_get_info(0)[0]
        want = _ingest_bytes(nch)
        assert abs(used - want) <= 0.03 * want + (64 << 20), (used, want)
        assert want < 4.0e9                             # 2 x 28 MB of ring per channel against 2 x 83 MB for a pipe of its own
        pipe.push_audio(X[1:])
        pipe.flush()
        recs = pipe.collect(cap=1 << 20)
        st = pipe.stats()
    finally:
        pipe.close()
    assert st["frames"] == nch and st["batches"] == nch
    assert (recs["frame"] == 0).all() and set(recs["channel"].tolist()) <= set(range(nch))
    _check_order(recs, nch)
