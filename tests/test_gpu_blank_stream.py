"""The noise blanker in the stream, the pipe and decode_wav: options "blank" / "blank_guard" put K12
(tests/test_gpu_blank.py) ahead of the resampler and the front-end.  Its outputs are integers' work, so the checks are byte
for byte on the ring's frames: a stream does not depend on how the audio was cut or which format a piece had, it is a
blank = 0 stream fed Context.blank's output without its last G samples (at 12 kS/s, and at 48 kS/s where K11 follows), a
reset restarts the block count, a changed option is refused, a two-channel pipe is two one-channel pipes, the statistics
are the restatement's counts, and with blank = 0 nothing of K12 runs.  Then what it is for: clean audio decodes as
before, and the closed-loop signal under Gaussian noise PLUS impulses decodes with the blanker and not without."""
import os

import numpy as np
import pytest

import blank_exact as BX

HOP, FL = 3375, 45000
N = BX.N
ERR_ARG = -6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEED = 32 * (FL - 1) + 1          # 12 kS/s samples that complete frame 0 (K0 in its default mode reads no sample ahead)


def _f32(x):
    return (x.astype(np.float32) / np.float32(32768)).astype(np.float32)


def _audio_s16(n, seed, C=None):
    """noise of sigma 300 whose level drops tenfold for two blocks now and then, impulses of 40 sigma with probability
    1/250, a run of three, and spikes on and beside block edges"""
    r = np.random.Generator(np.random.Philox(seed))
    shape = (n,) if C is None else (n, C)
    x = r.standard_normal(shape) * 300.0
    blk = np.arange(n) // N
    quiet = (blk % 7 == 3) | (blk % 7 == 4)
    x[quiet] *= 0.1
    hit = r.random(shape) < 1.0 / 250
    x = np.where(hit, r.standard_normal(shape) * 12000.0, x)
    for i in (N - 1, N, N + 1, 2 * N - 1, 5 * N, 5 * N + 1, 5 * N + 2, 9 * N - 2):
        if i < n:
            x[i] = 20000.0
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _take_all(ctx, expect=None):
    import torch
    n = ctx.stream_push_audio(np.zeros(0, np.float32))
    assert n > 0 and (expect is None or n == expect)
    out = torch.empty((n, FL, 2), dtype=torch.float32, device="cuda:0")
    pos = ctx.stream_take(n, out)
    ctx.synchronize()
    return out.cpu().numpy(), pos


def _streamed(G, pieces, options=None, reset=None, stats=False):
    ctx = G.Context(options=options or {})
    try:
        ctx.stream_open(HOP, 8)
        if reset is not None:
            ctx.stream_reset(reset)
        for x in pieces:
            ctx.stream_push_audio(x)
        fr, pos = _take_all(ctx)
        return (fr, pos, ctx.stream_blank_stats(1)) if stats else (fr, pos)
    finally:
        ctx.close()


# ---- the audio of the cut tests: a head that is cut in pieces, a tail pushed whole ------------------------------------
G_CUT = 2
HEAD = 5 * N + 17
_cache = {}


def _head_and_tail():
    if "x" not in _cache:
        x = _audio_s16(NEED + G_CUT + 5, 3000)
        _cache["x"] = (x[:HEAD], x[HEAD:])
    return _cache["x"]


def _whole(G):
    if "whole" not in _cache:
        head, tail = _head_and_tail()
        fr, pos, st = _streamed(G, [head, tail], {"blank": 24, "blank_guard": G_CUT}, stats=True)
        assert fr.shape[0] == 1 and pos == 0
        _cache["whole"] = (fr, st)
    return _cache["whole"]


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 7, 4096, 10007])
def test_cuts_and_formats_do_not_matter(G, cut):
    head, tail = _head_and_tail()
    ref, _ = _whole(G)
    run = 1000 if cut < 100 else 1
    x = head if cut < 100 else np.concatenate([head, tail[:6 * 10007]])
    rest = tail if cut < 100 else tail[6 * 10007:]
    pieces = [x[k: k + cut] for k in range(0, len(x), cut)]
    pieces = [p if (i // run) % 2 == 0 else _f32(p) for i, p in enumerate(pieces)]   # (the first switch widens the int16 history)
    got, pos = _streamed(G, pieces + [rest], {"blank": 24, "blank_guard": G_CUT})
    assert pos == 0 and got.tobytes() == ref.tobytes()


@pytest.mark.gpu
def test_stats_are_the_restatements_counts(G):
    head, tail = _head_and_tail()
    _, (samples, zeroed) = _whole(G)
    x = np.concatenate([head, tail])
    y, med, nz = BX.blank(x, 24, G_CUT)
    hit = BX.dilate(BX.flags(x.reshape(-1, 1), 24), G_CUT)[:, 0]
    assert samples[0] == len(x) - G_CUT and zeroed[0] == hit[:len(x) - G_CUT].sum()
    assert 0.01 * len(x) < zeroed[0] < 0.2 * len(x)                # impulses and their guards, and the level steps' blocks


@pytest.mark.gpu
def test_stream_equals_blank_off_stream_fed_the_batch_output(G):
    head, tail = _head_and_tail()
    ref, _ = _whole(G)
    x = np.concatenate([head, tail])
    ctx = G.Context()
    try:
        y = ctx.blank(x, 24, G_CUT)[0]
    finally:
        ctx.close()
    assert y.tobytes() == BX.blank(x, 24, G_CUT)[0].tobytes()
    before = G.blank_launch_counts()
    got, pos = _streamed(G, [y[:123457], y[123457:len(y) - G_CUT]])
    assert G.blank_launch_counts() == before                       # blank = 0: no K12 launch
    assert pos == 0 and got.tobytes() == ref.tobytes()


@pytest.mark.gpu
def test_at_48k_the_resampler_follows(G):
    rate, g = 48000, 3
    n = 4 * NEED + 400                                             # completes 12 kS/s sample NEED - 1 behind K11's delay
    x = _audio_s16(n + g, 3100)
    opts = {"audio_rate": rate, "blank": 24, "blank_guard": g}
    cut = 1000003
    pieces = [x[k: k + cut] if (k // cut) % 2 == 0 else _f32(x[k: k + cut]) for k in range(0, len(x), cut)]
    got, pos, (samples, zeroed) = _streamed(G, pieces, opts, stats=True)
    assert samples[0] == len(x) - g and zeroed[0] > 0
    ctx = G.Context()
    try:
        y = ctx.blank(x, 24, g)[0]
    finally:
        ctx.close()
    want, wpos = _streamed(G, [y[:len(y) - g]], {"audio_rate": rate})
    assert got.shape == want.shape and got.shape[0] == 1 and pos == wpos == 0 and got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_reset_restarts_the_blocks_and_a_changed_option_is_refused(G):
    head, tail = _head_and_tail()
    ref, (rs, rz) = _whole(G)
    x = np.concatenate([head, tail])
    pos = 123457
    ctx = G.Context(options={"blank": 24, "blank_guard": G_CUT})
    try:
        ctx.stream_open(HOP, 8)
        junk = _audio_s16(50001, 3200)
        assert len(junk) % N != 0
        ctx.stream_push_audio(junk)                                # it must leave no trace: block 0 starts at the reset
        ctx.stream_reset(pos)
        assert (ctx.stream_blank_stats(1)[0] == 0).all()
        ctx.stream_push_audio(x[:100003])
        for name, value, old in (("blank", 28, 24), ("blank_guard", 3, G_CUT), ("blank", 0, 24)):
            ctx.set_option(name, value)
            with pytest.raises(G.UwsprError) as e:
                ctx.stream_push_audio(x[100003:200000])
            assert e.value.status == ERR_ARG and "blank" in str(e.value)
            ctx.set_option(name, old)
        ctx.stream_push_audio(_f32(x[100003:200000]))
        ctx.stream_push_audio(x[200000:])
        got, gpos = _take_all(ctx, 1)
        s, z = ctx.stream_blank_stats(1)
        assert gpos == pos and got.tobytes() == ref.tobytes()
        assert s[0] == rs[0] and z[0] == rz[0]
    finally:
        ctx.close()


# ---- the pipe ----------------------------------------------------------------------------------------------------------
def _run_pipe(G, x, piece=250000, channels=1, **opts):
    pipe = G.Pipe(hop=HOP, batch_frames=3, max_per_frame=2, lanes=3, **opts)
    try:
        for k in range(0, len(x), piece):
            pipe.push_audio(x[k: k + piece])
        pipe.flush()
        return pipe.collect(cap=1 << 16), pipe.stats(), pipe.blank_stats(channels)
    finally:
        pipe.close()


def _texts(G, recs):
    return sorted(G.unpack_message(r["message"])[1] for r in recs if r["decoded"])


@pytest.mark.gpu
def test_two_channel_pipe_is_two_one_channel_pipes(G):
    x = _audio_s16(NEED + 2 + 9000, 3300, C=2)
    x[:, 1] = _closed_loop_s16(len(x))                             # one channel with something to find
    recs, st, (samples, zeroed) = _run_pipe(G, x, piece=333331, channels=2, blank=24)
    assert st["frames"] == 2 and (samples == len(x) - 2).all()
    for c in range(2):
        xc = np.ascontiguousarray(x[:, c])
        one, st1, (s1, z1) = _run_pipe(G, xc, blank=24)
        got = recs[recs["channel"] == c].copy()
        got["channel"] = 0
        assert [r.tobytes() for r in got] == [r.tobytes() for r in one]
        hit = BX.dilate(BX.flags(xc.reshape(-1, 1), 24), 2)[:, 0]
        assert zeroed[c] == z1[0] == hit[:len(xc) - 2].sum()
    assert "VE3EMB FN25 30" in _texts(G, recs[recs["channel"] == 1])


@pytest.mark.gpu
def test_pipe_options(G):
    pipe = G.Pipe(hop=HOP, batch_frames=3, lanes=2, blank=24, blank_guard=5)
    try:
        for name, bad in (("blank", 3), ("blank", 1025), ("blank_guard", 65), ("blank_guard", -1)):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_option(name, bad)
            assert e.value.status == ERR_ARG
        pipe.push_audio(_audio_s16(5000, 3400))
        for name, other in (("blank", 28), ("blank", 0), ("blank_guard", 2)):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_option(name, other)                       # the stream runs with 24 / 5
            assert e.value.status == ERR_ARG
        pipe.set_option("blank", 24)
        pipe.set_option("blank_guard", 5)
        pipe.push_audio(_audio_s16(5000, 3401))
        s, z = pipe.blank_stats(1)
        assert s[0] == 10000 - 5
        pipe.flush()
    finally:
        pipe.close()
    with pytest.raises(G.UwsprError):
        G.Pipe(hop=HOP, batch_frames=3, lanes=2, blank=2)


@pytest.mark.gpu
def test_blank_off_runs_nothing_of_k12(G):
    xs = _audio_s16(NEED + 40, 3500)
    before = G.blank_launch_counts()
    a, pa = _streamed(G, [xs[:700001], xs[700001:]])
    b, pb = _streamed(G, [xs[:700001], xs[700001:]], {"blank": 0, "blank_guard": 64})
    assert a.tobytes() == b.tobytes() and pa == pb == 0
    ra, sa, (s, z) = _run_pipe(G, xs)
    rb, sb, _ = _run_pipe(G, xs, blank=0, blank_guard=7)
    assert sa["frames"] == sb["frames"] == 1 and [r.tobytes() for r in ra] == [r.tobytes() for r in rb]
    assert s[0] == 0 and z[0] == 0
    assert G.blank_launch_counts() == before


# ---- what it is for ----------------------------------------------------------------------------------------------------
def _closed_loop_s16(n):
    """examples/WaveFilePlusNoiseDecode.grc's mix (tx x 0.1 + whales, both repeating) at the stored gains, as int16"""
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    x = float(rec["tx_gain"]) * tx + float(rec["whales_gain"]) * wh
    return np.clip(np.rint(x.astype(np.float32) * 32768.0), -32768, 32767).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["closed_loop", "recording"])
def test_clean_audio_decodes_as_before(G, which):
    if which == "closed_loop":
        x, text = _closed_loop_s16(1440000), "VE3EMB FN25 30"
    else:
        x, text = np.load(os.path.join(GOLDEN, "150613_1920_int16.npz"))["x"], "VE3EMB FN42 33"
    off, _, _ = _run_pipe(G, x)
    on, _, (s, z) = _run_pipe(G, x, blank=24)
    assert text in _texts(G, off) and _texts(G, on) == _texts(G, off)
    print("%s: %d of %d samples zeroed" % (which, z[0], s[0]))


@pytest.mark.gpu
def test_decode_wav_takes_blank(G, tmp_path):
    import wave
    x = _closed_loop_s16(1440000)
    p = tmp_path / "loop.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(np.ascontiguousarray(x, "<i2").tobytes())
    a = G.decode_wav(p, max_per_frame=2)
    b = G.decode_wav(p, max_per_frame=2, blank=24, blank_guard=2)
    assert "VE3EMB FN25 30" in [d["text"] for d in a] and [d["text"] for d in a] == [d["text"] for d in b]
    with pytest.raises(G.UwsprError):
        G.decode_wav(p, blank=3)


SNR_DB, P_IMP, AMP_IMP = -22.0, 1.0 / 250, 60.0


def _impulsive(seed):
    """tx + sigma N(0, 1) at -22 dB in 2500 Hz + impulses (probability 1/250, 60 sigma): the three draws in that order
    from Philox(1000 + seed)"""
    tx = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))["tx"].astype(np.float64) / 32768.0
    sigma = np.sqrt(tx.var() * 6000.0 / (2500.0 * 10.0 ** (SNR_DB / 10.0)))
    r = np.random.Generator(np.random.Philox(1000 + seed))
    gauss = r.standard_normal(len(tx))
    where = r.random(len(tx)) < P_IMP
    imp = r.standard_normal(len(tx))
    return (tx + sigma * gauss + np.where(where, AMP_IMP * sigma * imp, 0.0)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_impulsive_noise_decodes_with_the_blanker_only(G, seed):
    x = _impulsive(seed)
    off, _, _ = _run_pipe(G, x)
    on, _, (s, z) = _run_pipe(G, x, blank=24)
    print("seed %d: blank=0 %r; blank=24 %r; %d of %d samples zeroed" % (seed, _texts(G, off), _texts(G, on), z[0], s[0]))
    assert not any("VE3EMB" in t for t in _texts(G, off))
    assert "VE3EMB FN25 30" in _texts(G, on)
