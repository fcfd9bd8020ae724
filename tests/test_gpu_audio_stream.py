"""Audio streams: 12 kS/s real audio pushed into the stream (uwspr_stream_push_audio) and the pipe
(uwspr_pipe_push_audio) -- the receiver flowgraph examples/AudioSourceDecode.grc runs as one chain: audio_source ->
float_to_complex -> band-pass -> low-pass -> rational_resampler /32 -> sliding_window_stream_to_pdu -> FDR ->
sync_and_demodulate -> WSPR_unpacker.

Stream sample m is y[m] = sum_k g[k] x[32 m + D - k] over the pushed audio x (zero before its first sample), made by
the same K0 kernel as uwspr_frontend_batch with the same per-output arithmetic, so the checks are byte for byte:
against the batch call, across chunkings, memory kinds and sample formats, across a reset, and the pipe fed audio
against the pipe fed the decimated stream.  The float64 chain of oracle/frontend_grc.py checks the seam between two
records; the reference's two demos decode from streams."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

HOP, FL, P = 3375, 45000, 216          # P >= the grc filter's 6831 taps / 32 (J = 216 per phase)
READ_AHEAD = {0: 0, 1: 512}             # D of the two tap modes


@pytest.fixture(scope="module")
def FE():
    import frontend_grc
    return frontend_grc


def _closed_loop_audio(seconds):
    """examples/WaveFilePlusNoiseDecode.grc's mix (tx x 0.1 + whales, both repeating; int16 / 32768)"""
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    n = seconds * 12000
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    return (float(rec["tx_gain"]) * tx + float(rec["whales_gain"]) * wh).astype(np.float32)


def _recording_s16():
    return np.load(os.path.join(GOLDEN, "150613_1920_int16.npz"))["x"]


def _noise_s16(n, seed, sigma=3000.0):
    x = np.random.default_rng(seed).standard_normal(n) * sigma
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _take_all(ctx):
    """every complete frame of the context's stream -> (numpy [k, fl, 2], first_pos)"""
    import torch
    n = ctx.stream_push_audio(np.zeros(0, np.float32))
    assert n > 0
    out = torch.empty((n, FL, 2), dtype=torch.float32, device="cuda:0")
    pos = ctx.stream_take(n, out)
    ctx.synchronize()
    return out.cpu().numpy(), pos


def _stream_samples(frames):
    """the decimated stream the overlapping frames (hop HOP) cover"""
    k = frames.shape[0]
    s = np.zeros(((k - 1) * HOP + FL, 2), np.float32)
    for j in range(k):
        s[j * HOP: j * HOP + FL] = frames[j]
    for j in range(1, k):   # the overlaps agree (frames are views of one stream)
        assert frames[j][: FL - HOP].tobytes() == frames[j - 1][HOP:].tobytes()
    return s


def _streamed(G, pieces, mode=0, max_frames=64, reset=None):
    ctx = G.Context(options={"frontend": mode})
    try:
        ctx.stream_open(HOP, max_frames)
        if reset is not None:
            ctx.stream_reset(reset)
        for x in pieces:
            ctx.stream_push_audio(x)
        return _take_all(ctx)
    finally:
        ctx.close()


# ---- 1. frame 0 is the batch call ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_frame0_equals_the_batch_call(G, mode):
    x = np.random.default_rng(10 + mode).standard_normal(32 * FL).astype(np.float32)
    ctx = G.Context(options={"frontend": mode})
    try:
        batch = ctx.frontend(x[None])[0]
    finally:
        ctx.close()
    # the batch counts the samples after the record as zero; the stream needs them pushed (the last output reads D on)
    frames, pos = _streamed(G, [x, np.zeros(READ_AHEAD[mode], np.float32)], mode)
    assert pos == 0 and frames.shape[0] == 1
    assert frames[0].tobytes() == batch.tobytes()


# ---- 2. later frames are pre-rolled batches -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_later_frames_equal_a_pre_rolled_batch(G, mode):
    x = np.random.default_rng(20 + mode).standard_normal(5 * 60 * 12000).astype(np.float32)
    frames, _ = _streamed(G, [x[k: k + 12000 * 60] for k in range(0, x.size, 12000 * 60)], mode)
    nf = frames.shape[0]
    assert nf == (x.size // 32 - READ_AHEAD[mode] // 32 - FL) // HOP + 1
    s = _stream_samples(frames)
    nin = 32 * FL
    rows = np.stack([x[32 * (k * HOP - P): 32 * (k * HOP - P) + nin] for k in range(1, nf)])
    ctx = G.Context(options={"frontend": mode})
    try:
        batch = ctx.frontend(rows)
    finally:
        ctx.close()
    hi = FL if mode == 0 else (nin - 1 - READ_AHEAD[mode]) // 32 + 1   # the batch window inside its record
    for k in range(1, nf):
        got = s[k * HOP: k * HOP + hi - P]
        assert got.tobytes() == batch[k - 1][P:hi].tobytes(), k


# ---- 3. chunking, memory kinds and sample formats do not matter ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_chunking_memory_and_format_do_not_matter(G, mode):
    import torch
    xs = _noise_s16(360 * 12000, 30 + mode)          # longer than one K0 launch of the stream (4 Mi samples)
    xf = (xs.astype(np.float32) / np.float32(32768)).astype(np.float32)
    ref, _ = _streamed(G, [xf], mode)
    assert xs.size > 4 << 20 and ref.shape[0] == 27

    rng = np.random.default_rng(3)
    sizes = [1, 31, 32, 33, 4800, 1 << 20]
    while sum(sizes) < xs.size:
        sizes.append(int(rng.integers(1, 60000)))
    rng.shuffle(sizes)
    cuts = np.cumsum(sizes)[:-1]
    cuts = cuts[cuts < xs.size]
    got, _ = _streamed(G, np.split(xs, cuts), mode)
    assert got.tobytes() == ref.tobytes(), "int16 in ragged pieces"
    got, _ = _streamed(G, np.split(xf, cuts), mode)
    assert got.tobytes() == ref.tobytes(), "float32 in ragged pieces"
    got, _ = _streamed(G, [xs], mode)
    assert got.tobytes() == ref.tobytes(), "int16 in one piece"
    mixed = [p if k % 2 else p.astype(np.float32) / np.float32(32768) for k, p in enumerate(np.split(xs, cuts))]
    got, _ = _streamed(G, mixed, mode)
    assert got.tobytes() == ref.tobytes(), "float32 and int16 pieces alternating"
    got, _ = _streamed(G, [xs[:3000000], xf[3000000:3000100], xs[3000100:]], mode)
    assert got.tobytes() == ref.tobytes(), "int16, one float32 piece, int16"

    buf = G.host_alloc(xf.nbytes)
    try:
        pinned = np.frombuffer(buf, np.float32)
        pinned[:] = xf
        got, _ = _streamed(G, [pinned], mode)
        assert got.tobytes() == ref.tobytes(), "page-locked"
        ctx = G.Context(options={"frontend": mode})
        try:
            ctx.stream_open(HOP, 64)
            for a, b in ((0, 700000), (700000, xf.size)):
                ctx.stream_push_audio(pinned[a:b], where="async")
            ctx.stream_wait_uploads()
            got, _ = _take_all(ctx)
        finally:
            ctx.close()
        assert got.tobytes() == ref.tobytes(), "page-locked, asynchronous"
    finally:
        G.host_free(buf)

    for host in (xs, xf):
        dev = torch.from_numpy(host).to("cuda:0")
        got, _ = _streamed(G, [dev[: 400001], dev[400001:]], mode)
        assert got.tobytes() == ref.tobytes(), "device %s" % dev.dtype
    strided = torch.stack([torch.from_numpy(xs).to("cuda:0"), torch.zeros(xs.size, dtype=torch.int16, device="cuda:0")], 1)[:, 0]
    assert not strided.is_contiguous()
    got, _ = _streamed(G, [strided[: 400001], strided[400001:]], mode)
    assert got.tobytes() == ref.tobytes(), "non-contiguous device tensor"


# ---- 4. the seam between two records, against the float64 chain --------------------------------------------------
@pytest.mark.gpu
def test_two_records_back_to_back_match_the_float64_chain(G, FE):
    x = np.concatenate([_closed_loop_audio(120), _recording_s16().astype(np.float32) / np.float32(32768)])
    frames, _ = _streamed(G, [x[: 1000003], x[1000003:]])
    s = _stream_samples(frames)
    ref = FE.chain(x, nout=s.shape[0])
    z = s[:, 0].astype(np.float64) + 1j * s[:, 1].astype(np.float64)
    assert np.abs(z - ref).max() / np.abs(ref).max() <= 1e-5
    seam = slice(FL - 400, FL + 400)                     # the outputs that read both records
    assert np.abs(z[seam] - ref[seam]).max() / np.abs(ref).max() <= 1e-5


# ---- 5. reset --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_reset_equals_a_fresh_stream_at_pos(G, mode):
    a = _noise_s16(30 * 12000, 50)
    b = _noise_s16(140 * 12000, 51)
    pos = 123457
    ctx = G.Context(options={"frontend": mode})
    try:
        ctx.stream_open(HOP, 64)
        ctx.stream_push_audio(a)
        ctx.stream_reset(pos)
        ctx.stream_push_audio(b[:77777])
        ctx.stream_push_audio(b[77777:])
        got, gpos = _take_all(ctx)
    finally:
        ctx.close()
    want, wpos = _streamed(G, [b], mode, reset=pos)
    assert gpos == wpos == pos
    assert got.tobytes() == want.tobytes()
    first, _ = _streamed(G, [b], mode)                    # the history was zeroed: the same values as a stream at 0
    assert got.tobytes() == first.tobytes()


# ---- 6. argument errors --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_are_not_sticky(G):
    import ctypes as C
    N = G.native
    x = _noise_s16(130 * 12000, 60)
    xf = (x.astype(np.float32) / np.float32(32768)).astype(np.float32)
    want, _ = _streamed(G, [xf])

    def raw(ctx, arr, n, fmt):
        nr = C.c_int(0)
        return ctx.L.uwspr_stream_push_audio(ctx.h, C.c_void_p(arr.ctypes.data), n, fmt, N.HOST, C.byref(nr))

    ctx = G.Context()
    try:
        with pytest.raises(N.UwsprError) as e:
            ctx.stream_push_audio(xf[:100])                 # before stream_open
        assert e.value.status == -6
        ctx.stream_open(HOP, 64)
        ctx.stream_push_audio(xf[:500000])
        assert raw(ctx, xf, 100, 7) == -6                    # bad format
        assert raw(ctx, xf, -1, N.AUDIO_F32) == -6           # n < 0
        with pytest.raises(N.UwsprError) as e:
            ctx.stream_push(np.zeros((100, 2), np.float32))  # (I,Q) into an audio stream
        assert e.value.status == -6
        ctx.set_option("frontend", 1)
        with pytest.raises(N.UwsprError) as e:
            ctx.stream_push_audio(xf[500000:600000])         # the tap mode changed under a live stream
        assert e.value.status == -6 and "frontend" in str(e.value)
        ctx.set_option("frontend", 0)
        ctx.stream_push_audio(x[500000:600000])              # int16 into a float32 stream: formats mix
        ctx.stream_push_audio(xf[600000:])
        got, _ = _take_all(ctx)
        assert got.tobytes() == want.tobytes()

        # an (I,Q) stream refuses audio and goes on
        ctx.stream_reset(0)
        iq = np.random.default_rng(61).standard_normal((FL + HOP, 2)).astype(np.float32)
        ctx.stream_push(iq[:1000])
        with pytest.raises(N.UwsprError) as e:
            ctx.stream_push_audio(xf[:100])
        assert e.value.status == -6
        assert ctx.stream_push(iq[1000:]) == 2
        import torch
        out = torch.empty((2, FL, 2), dtype=torch.float32, device="cuda:0")
        assert ctx.stream_take(2, out) == 0
        ctx.synchronize()
        o = out.cpu().numpy()
        assert o[0].tobytes() == iq[:FL].tobytes() and o[1].tobytes() == iq[HOP:].tobytes()
    finally:
        ctx.close()


# ---- 7. the pipe on audio is the pipe on the decimated stream ---------------------------------------------------------
def _records(recs):
    return [r.tobytes() for r in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_pipe_on_audio_equals_pipe_on_iq(G, lanes):
    xs = np.clip(np.rint(_closed_loop_audio(240) * 32768.0), -32768, 32767).astype(np.int16)
    frames, _ = _streamed(G, [xs])
    nf = frames.shape[0]
    assert nf == 14
    iq = _stream_samples(frames)

    def run(feed):
        pipe = G.Pipe(hop=HOP, batch_frames=4, max_per_frame=2, lanes=lanes)
        try:
            feed(pipe)
            pipe.flush()
            return pipe.collect(), pipe.stats()
        finally:
            pipe.close()

    def audio(pipe):
        rng = np.random.default_rng(70 + lanes)
        pos = 0
        while pos < xs.size:
            n = int(rng.integers(1, 400000))
            pipe.push_audio(xs[pos: pos + n])
            pos += n

    def decimated(pipe):
        for k in range(0, iq.shape[0], 50000):
            pipe.push(iq[k: k + 50000])

    ra, sa = run(audio)
    ri, si = run(decimated)
    assert sa["frames"] == si["frames"] == nf
    assert (ra["stream_pos"] == ra["frame"] * HOP).all()
    assert _records(ra) == _records(ri)
    assert ra["decoded"].sum() >= 1


# ---- 8. the demos decode as streams --------------------------------------------------------------------------------------
def _texts(G, recs, frame=None):
    return {G.unpack_message(r["message"])[1] for r in recs if r["decoded"] and (frame is None or r["frame"] == frame)}


@pytest.mark.gpu
def test_closed_loop_demo_decodes_as_a_stream(G):
    x = _closed_loop_audio(360)
    pipe = G.Pipe(hop=HOP, batch_frames=8)
    try:
        for k in range(0, x.size, 12000 * 45):
            pipe.push_audio(x[k: k + 12000 * 45])
        pipe.flush()
        recs = pipe.collect()
    finally:
        pipe.close()
    assert _texts(G, recs, 0) == {"VE3EMB FN25 30"}
    # the decode set over all frames is that of the sequential calls on the same frames
    import torch
    ctx = G.Context()
    try:
        ctx.stream_open(HOP, 64)
        ctx.stream_push_audio(x)
        frames, _ = _take_all(ctx)
        assert frames.shape[0] == recs["frame"].max() + 1
        cands, out = ctx.pipeline_batch(torch.from_numpy(frames).to("cuda:0"), max_per_frame=1)
    finally:
        ctx.close()
    recs_s = np.stack([out[b, 0] for b in range(len(cands)) if len(cands[b])])
    msgs, _, ok = G.decode_batch(recs_s)
    seq = {G.unpack_message(msgs[i])[1] for i in range(len(ok)) if ok[i]}
    assert _texts(G, recs) == seq


@pytest.mark.gpu
def test_recording_decodes_three_hops_into_a_stream_and_from_a_wav(G, tmp_path):
    import wave
    lead = 3 * HOP * 32
    x = np.concatenate([_noise_s16(lead, 80, 300.0), _recording_s16(), _noise_s16(12000 * 20, 81, 300.0)])
    pipe = G.Pipe(hop=HOP, batch_frames=8, max_per_frame=2)
    try:
        for k in range(0, x.size, 250000):
            pipe.push_audio(x[k: k + 250000])
        pipe.flush()
        recs = pipe.collect()
    finally:
        pipe.close()
    assert "VE3EMB FN42 33" in _texts(G, recs, 3)
    path = tmp_path / "rec.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(x.tobytes())
    dec = G.decode_wav(path, max_per_frame=2)
    hits = [d for d in dec if d["text"] == "VE3EMB FN42 33"]
    assert any(d["t"] == 27.0 and d["frame"] == 3 for d in hits), dec
