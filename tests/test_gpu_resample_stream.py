"""Audio at a sound card's rate through the stream, the pipe and decode_wav: option "audio_rate" puts K11 (the rational
resampler, tests/test_gpu_resample.py) ahead of K0.  Every output of K11 has one owner and one order, so the checks are
byte for byte: a stream's samples do not depend on how the audio was cut or which format a piece had, they are those of
a default stream fed Context.resample's output, a reset restarts the resampler at audio time pos / 375 s, a pipe at
48 kS/s gives the records of a default pipe fed the resampled audio, and WAVs written here at 12, 44.1 and 48 kS/s
decode to the same text, frame, time and frequency.  With the default rate nothing of K11 runs."""
import wave

import numpy as np
import pytest

import resample_exact as X

HOP, FL = 3375, 45000
ERR_ARG = -6


def _noise_s16(n, seed, sigma=3000.0):
    x = np.random.default_rng(seed).standard_normal(n) * sigma
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _f32(x):
    return (x.astype(np.float32) / np.float32(32768)).astype(np.float32)


def _take_all(ctx):
    """every complete frame of the context's stream -> (numpy [k, fl, 2], first_pos)"""
    import torch
    n = ctx.stream_push_audio(np.zeros(0, np.float32))
    assert n > 0
    out = torch.empty((n, FL, 2), dtype=torch.float32, device="cuda:0")
    pos = ctx.stream_take(n, out)
    ctx.synchronize()
    return out.cpu().numpy(), pos


def _streamed(G, pieces, rate=None, reset=None):
    ctx = G.Context(options={} if rate is None else {"audio_rate": rate})
    try:
        ctx.stream_open(HOP, 8)
        if reset is not None:
            ctx.stream_reset(reset)
        for x in pieces:
            ctx.stream_push_audio(x)
        return _take_all(ctx)
    finally:
        ctx.close()


def _complete(n_in, rate):
    """12 kS/s outputs that n_in pushed samples complete: i0(j) <= n_in - 1"""
    hp, L, M, T, N, D = X.plan(rate)
    t = n_in * L - 1 - D
    return t // M + 1 if t >= 0 else 0


# ---- the audio of the cut tests: about 3 s of noise, then silence until one frame is complete ------------------------
_audio = {}


def _head_and_tail(rate):
    if rate not in _audio:
        head = _noise_s16(3 * rate + 17, 2000 + rate % 89)
        hp, L, M, T, N, D = X.plan(rate)
        n12 = 32 * (FL - 1) + 1                                   # K0 (grc, D = 0) completes frame 0 with 12 kS/s sample 32 (fl - 1)
        n_in = -(-((n12 - 1) * M + D + 1) // L) + 5               # inputs that complete n12 outputs, and a few more
        assert _complete(n_in, rate) >= n12 and _complete(n_in, rate) < n12 + 32
        _audio[rate] = (head, np.zeros(n_in - len(head), np.int16))
    return _audio[rate]


_whole = {}


def _whole_push(G, rate):
    """the reference of the cut tests: head and tail in one push each (cached)"""
    if rate not in _whole:
        head, tail = _head_and_tail(rate)
        fr, pos = _streamed(G, [head, tail], rate)
        assert fr.shape[0] == 1 and pos == 0
        _whole[rate] = fr
    return _whole[rate]


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 7, 10007])
@pytest.mark.parametrize("rate", [48000, 44100])
def test_cuts_and_formats_do_not_matter(G, rate, cut):
    head, tail = _head_and_tail(rate)
    ref = _whole_push(G, rate)
    assert np.abs(ref[0, :300]).max() > 0
    # pieces of `cut` samples, int16 and float32 in runs of 1000 pieces (the first switch widens the int16 history)
    pieces = [head[k: k + cut] for k in range(0, len(head), cut)]
    pieces = [p if (i // 1000) % 2 == 0 else _f32(p) for i, p in enumerate(pieces)]
    got, pos = _streamed(G, pieces + [tail], rate)
    assert pos == 0 and got.tobytes() == ref.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [48000, 44100])
def test_stream_equals_the_batch_form_pushed_at_12k(G, rate):
    head, tail = _head_and_tail(rate)
    ref = _whole_push(G, rate)
    x = np.concatenate([head, tail])
    ctx = G.Context()
    try:
        y = ctx.resample(x, rate, nout=_complete(len(x), rate))
    finally:
        ctx.close()
    before = G.resample_launch_counts()
    got, pos = _streamed(G, [y[:123457], y[123457:]])            # plain 12 kS/s float audio, default audio_rate
    assert G.resample_launch_counts() == before                  # (K11 does not run at the default rate)
    assert pos == 0 and got.tobytes() == ref.tobytes()


# ---- reset, and a changed rate ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reset_restarts_the_resampler_at_pos(G):
    import torch
    rate, pos = 44100, 123457
    assert pos % 5 != 0
    head, tail = _head_and_tail(rate)
    x = np.concatenate([head, tail])
    ctx = G.Context(options={"audio_rate": rate})
    try:
        ctx.stream_open(HOP, 8)
        ctx.stream_push_audio(_noise_s16(50001, 2100))           # something before the reset: it must leave no trace
        ctx.stream_reset(pos)
        ctx.stream_push_audio(x[:100003])
        # a changed rate fails that push and leaves the stream unharmed
        ctx.set_option("audio_rate", 48000)
        with pytest.raises(G.UwsprError) as e:
            ctx.stream_push_audio(x[100003:200000])
        assert e.value.status == ERR_ARG and "audio_rate" in str(e.value)
        with pytest.raises(G.UwsprError) as e:
            ctx.set_option("audio_rate", 12345)                  # not a supported rate
        assert e.value.status == ERR_ARG
        ctx.set_option("audio_rate", rate)
        ctx.stream_push_audio(_f32(x[100003:200000]))
        ctx.stream_push_audio(x[200000:])
        got, gpos = _take_all(ctx)
        assert gpos == pos and got.shape[0] == 1
        # the batch form, fed to K0's door at origin 32 pos: output j of the resampler is 12 kS/s sample 32 pos + j
        y = ctx.resample(x, rate, nout=_complete(len(x), rate))
        out = torch.empty((FL, 2), dtype=torch.float32, device="cuda:0")
        ctx.debug_frontend_launch(torch.from_numpy(y).to("cuda:0"), 32 * pos, out, pos)
        ctx.synchronize()
        assert got[0].tobytes() == out.cpu().numpy().tobytes()
    finally:
        ctx.close()
    # the same samples as a stream that starts at 0
    assert got.tobytes() == _whole_push(G, rate).tobytes()


# ---- signals ---------------------------------------------------------------------------------------------------------
SYMBOL_S = 8192.0 / 12000.0
TEXTS = ("K1ABC FN42 37", "VE3EMB FN25 30")
F0 = (2.0, -3.0)


def _cpfsk(G, text, f0, rate, seconds, amp):
    """numpy CPFSK at `rate`: symbol k at t in [1 + k 8192 / 12000, ...), tones (s - 1.5) 12000 / 8192 Hz around
    1500 + f0 Hz, continuous phase; zero outside the 162 symbols"""
    sym = G.wspr_symbols(G.wspr_pack(text)).astype(np.float64)
    n = int(round(seconds * rate))
    t = np.arange(n) / float(rate)
    k = np.floor((t - 1.0) / SYMBOL_S).astype(np.int64)
    on = (k >= 0) & (k < 162)
    f = 1500.0 + f0 + (sym[np.clip(k, 0, 161)] - 1.5) / SYMBOL_S
    phase = 2.0 * np.pi * np.cumsum(np.where(on, f, 0.0)) / rate
    return np.where(on, amp * np.sin(phase), 0.0)


AMP = 300.0
SIGMA_12K = AMP * np.sqrt(0.5 * (12000.0 / 2.0) / 2500.0 * 10.0 ** 1.5)   # -15 dB in 2500 Hz at 12 kS/s


def _recording(G, texts, f0s, rate, seconds, seed):
    """[n, C] int16: channel c carries texts[c] at -15 dB in 2500 Hz; white noise of the same density at every rate
    (sigma_R = sigma_12k sqrt(R / 12000))"""
    rng = np.random.default_rng(seed)
    chans = []
    for text, f0 in zip(texts, f0s):
        s = _cpfsk(G, text, f0, rate, seconds, AMP)
        s = s + rng.standard_normal(len(s)) * SIGMA_12K * np.sqrt(rate / 12000.0)
        chans.append(np.clip(np.rint(s), -32768, 32767).astype(np.int16))
    return np.stack(chans, axis=1)


def _write_wav(path, rate, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x, "<i2").tobytes())


# ---- the pipe ----------------------------------------------------------------------------------------------------------
def _run_pipe(G, feed, **opts):
    pipe = G.Pipe(hop=HOP, batch_frames=3, max_per_frame=2, lanes=3, **opts)
    try:
        feed(pipe)
        pipe.flush()
        return pipe.collect(cap=1 << 16), pipe.stats()
    finally:
        pipe.close()


@pytest.mark.gpu
def test_pipe_at_48k_equals_default_pipe_on_the_resampled_audio(G):
    rate = 48000
    x = _recording(G, TEXTS, F0, rate, 130.0, 2200)               # two channels, frames 0 and 1 complete
    ctx = G.Context()
    try:
        y = ctx.resample(x, rate, nout=_complete(len(x), rate))
    finally:
        ctx.close()

    def ragged(pipe):
        rng = np.random.default_rng(2201)
        pos, i = 0, 0
        while pos < len(x):
            n = 1 if i % 5 == 0 else int(rng.integers(2, 900000))
            piece = x[pos: pos + n]
            pipe.push_audio(piece if i % 3 else piece.astype(np.float32) / np.float32(32768))   # formats mix
            pos += n
            i += 1

    def resampled(pipe):
        for k in range(0, len(y), 250000):
            pipe.push_audio(y[k: k + 250000])

    before = G.resample_launch_counts()
    rb, sb = _run_pipe(G, resampled)
    assert G.resample_launch_counts() == before                   # the default pipe never runs K11
    ra, sa = _run_pipe(G, ragged, audio_rate=rate)
    assert sum(G.resample_launch_counts()) > sum(before)
    assert sa["frames"] == sb["frames"] == 4                      # 2 frames x 2 channels
    assert [r.tobytes() for r in ra] == [r.tobytes() for r in rb]
    texts = {(int(r["channel"]), G.unpack_message(r["message"])[1]) for r in ra if r["decoded"] and r["frame"] == 0}
    assert texts >= {(0, TEXTS[0]), (1, TEXTS[1])}
    assert (ra["stream_pos"] == ra["frame"] * HOP).all()


@pytest.mark.gpu
def test_pipe_audio_rate_errors(G):
    pipe = G.Pipe(hop=HOP, batch_frames=3, lanes=2, audio_rate=44100)
    try:
        with pytest.raises(G.UwsprError) as e:
            pipe.set_option("audio_rate", 12345)
        assert e.value.status == ERR_ARG
        pipe.push_audio(_noise_s16(5000, 2300))
        with pytest.raises(G.UwsprError) as e:
            pipe.set_option("audio_rate", 48000)                  # the stream runs at 44100
        assert e.value.status == ERR_ARG
        pipe.set_option("audio_rate", 44100)
        pipe.push_audio(_noise_s16(5000, 2301))
        pipe.flush()
    finally:
        pipe.close()
    with pytest.raises(G.UwsprError):
        G.Pipe(hop=HOP, batch_frames=3, lanes=2, audio_rate=7000)


# ---- decode_wav ----------------------------------------------------------------------------------------------------
# The seed is fixed in advance, not searched: -15 dB in 2500 Hz is more than 10 dB above where WSPR stops decoding, and
# the control (the 12 kS/s file, the path that existed before) is asserted first -- if IT does not decode, the input is
# at fault.  (The decoder needs the GPU, so no seed could be tried without one.)
SECONDS = 121.0            # one complete frame (120 s) and no second one


def _decode(G, path, **kw):
    return G.decode_wav(path, batch_frames=2, lanes=2, max_per_frame=2, **kw)


@pytest.fixture(scope="module")
def controls(G, tmp_path_factory):
    d = tmp_path_factory.mktemp("ctl")
    out = []
    for c in range(2):
        p = d / ("c%d.wav" % c)
        _write_wav(p, 12000, _recording(G, TEXTS[c:c + 1], F0[c:c + 1], 12000, SECONDS, 2400 + c))
        hits = [r for r in _decode(G, p) if r["text"] == TEXTS[c]]
        assert len(hits) >= 1, "the 12 kS/s control does not decode: the input is at fault, not the resampler"
        assert hits[0]["frame"] == 0 and hits[0]["t"] == 0.0
        out.append(hits[0])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [44100, 48000])
def test_decode_wav_at_other_rates(G, tmp_path, controls, rate):
    p = tmp_path / ("r%d.wav" % rate)
    _write_wav(p, rate, _recording(G, TEXTS[:1], F0[:1], rate, SECONDS, 2400))
    hits = [r for r in _decode(G, p) if r["text"] == TEXTS[0]]
    assert len(hits) >= 1
    assert hits[0]["frame"] == controls[0]["frame"] and hits[0]["t"] == controls[0]["t"]
    assert abs(hits[0]["freq"] - controls[0]["freq"]) <= 0.05


@pytest.mark.gpu
def test_decode_wav_stereo_48k(G, tmp_path, controls):
    p = tmp_path / "stereo48k.wav"
    _write_wav(p, 48000, _recording(G, TEXTS, F0, 48000, SECONDS, 2410))
    recs = _decode(G, p, channels="all")
    for c in range(2):
        hits = [r for r in recs if r["text"] == TEXTS[c]]
        assert len(hits) >= 1 and {r["channel"] for r in hits} == {c}
        assert hits[0]["frame"] == controls[c]["frame"] and hits[0]["t"] == controls[c]["t"]
        assert abs(hits[0]["freq"] - controls[c]["freq"]) <= 0.05
    # channel 0 alone, the default of decode_wav
    assert {r["text"] for r in _decode(G, p)} == {TEXTS[0]}


# ---- the default is untouched ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_default_rate_is_the_path_without_a_resampler(G):
    xs = _noise_s16(32 * FL, 2500)
    ctx = G.Context()
    try:
        batch = ctx.frontend(_f32(xs)[None])[0]                   # uwspr_frontend_batch: the path that existed before
    finally:
        ctx.close()
    before = G.resample_launch_counts()
    for rate in (None, 12000):
        fr, pos = _streamed(G, [xs[:700001], xs[700001:]], rate)
        assert pos == 0 and fr.shape[0] == 1 and fr[0].tobytes() == batch.tobytes()

    def feed(pipe):
        for k in range(0, len(xs), 250000):
            pipe.push_audio(xs[k: k + 250000])

    ra, sa = _run_pipe(G, feed)
    rb, sb = _run_pipe(G, feed, audio_rate=12000)
    assert sa["frames"] == sb["frames"] == 1 and [r.tobytes() for r in ra] == [r.tobytes() for r in rb]
    assert G.resample_launch_counts() == before                   # K11 never ran
