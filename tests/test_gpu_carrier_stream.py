"""Carriers through the streams and the pipe (options "carrier" / "frontend_hbw", uwspr_pipe_set_carriers): a stream
at another carrier does not depend on how it was cut, sits behind K11 and K12 as the 1500 Hz one does, restarts at any
position with the rotator's row of that position, survives a refused option change; a pipe with several carriers on
several channels gives, per plane, the records of a one-channel, one-carrier pipe; and a recording with the closed-loop
signal at three carriers decodes at all three."""
import os

import numpy as np
import pytest

import carrier_exact as CX
import frontend_exact as X
from conftest import GOLDEN

HOP, FL, J = 3375, 45000, 216
OPTS = dict(hop=HOP, batch_frames=3, max_per_frame=2, lanes=3)
FC = 2203


def _take_all(ctx):
    import torch
    n = ctx.stream_push_audio(np.zeros(0, np.float32))
    assert n > 0
    out = torch.empty((n, FL, 2), dtype=torch.float32, device="cuda:0")
    pos = ctx.stream_take(n, out)
    ctx.synchronize()
    return out.cpu().numpy(), pos


def _streamed(G, pieces, reset=None, between=None, **options):
    ctx = G.Context(options=options)
    try:
        ctx.stream_open(HOP, 8)
        if reset is not None:
            ctx.stream_reset(reset)
        for i, x in enumerate(pieces):
            if between is not None:
                between(ctx, i)
            ctx.stream_push_audio(x)
        return _take_all(ctx)
    finally:
        ctx.close()


def _cut(x, sizes=(1, 7, 10007)):
    """x in pieces of 1, 7 and 10 007 samples in turn, int16 and float32 pieces mixing"""
    out, pos, i = [], 0, 0
    while pos < len(x):
        k = min(sizes[i % len(sizes)], len(x) - pos)
        p = x[pos: pos + k]
        out.append(p if (i // 2) % 2 == 0 else X.s16_to_f32(p))
        pos += k
        i += 1
    return out


@pytest.fixture(scope="module")
def audio():
    return X.noise16(np.random.default_rng(900), 32 * (FL + HOP) + 999, sigma=3000.0)


@pytest.fixture(scope="module")
def whole(G, audio):
    frames, pos = _streamed(G, [audio], carrier=FC)
    assert pos == 0 and frames.shape[0] == 2 and frames.any()
    return frames


# ---- 1. the cuts and the formats do not matter; frame 0 is the batch call ------------------------------------------------
@pytest.mark.gpu
def test_a_carrier_stream_does_not_depend_on_its_cuts(G, audio, whole):
    frames, pos = _streamed(G, _cut(audio), carrier=FC)
    assert pos == 0 and frames.tobytes() == whole.tobytes()
    ctx = G.Context(options={"carrier": FC})
    try:
        batch = ctx.frontend(X.s16_to_f32(audio)[None, :32 * FL])[0]
    finally:
        ctx.close()
    assert batch.tobytes() == whole[0].tobytes()
    at_1500, _ = _streamed(G, [audio])
    assert at_1500.tobytes() != whole.tobytes()


@pytest.mark.gpu
def test_the_stream_is_the_sums_through_the_rotator(G, audio, whole):
    """the door of the forms without a rotator gives the sums at 2203 Hz; the stream is those, rotated by stream index"""
    import torch
    ctx = G.Context(options={"carrier": FC})
    try:
        out = torch.empty((FL + HOP, 2), dtype=torch.float32, device="cuda:0")
        ctx.debug_frontend_launch(torch.from_numpy(audio).to("cuda:0"), 0, out, 0)
        s = out.cpu().numpy()
    finally:
        ctx.close()
    table = G.frontend_rotator()
    want = CX.rotate(s, FC, np.arange(FL + HOP), table)
    assert whole[0].tobytes() == want[:FL].tobytes() and whole[1].tobytes() == want[HOP:].tobytes()


# ---- 2. behind K11 and behind K12 ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_behind_the_resampler_and_the_blanker(G):
    x48 = X.noise16(np.random.default_rng(901), 4 * 32 * FL + 40000, sigma=3000.0)
    a, pa = _streamed(G, [x48], carrier=FC, audio_rate=48000)
    b, pb = _streamed(G, _cut(x48, (1, 7, 10007, 400003)), carrier=FC, audio_rate=48000)
    assert pa == pb == 0 and a.shape[0] == 1 and a.any() and a.tobytes() == b.tobytes()
    ref, _ = _streamed(G, [x48], audio_rate=48000)
    assert ref.tobytes() != a.tobytes()
    x12 = X.noise16(np.random.default_rng(902), 32 * FL + 5000, sigma=3000.0)
    x12[::9973] = 32767                                           # clicks for the blanker to take out
    c, _ = _streamed(G, [x12], carrier=FC, blank=16)
    d, _ = _streamed(G, _cut(x12), carrier=FC, blank=16)
    plain, _ = _streamed(G, [x12], carrier=FC)
    assert c.shape[0] == 1 and c.tobytes() == d.tobytes() and c.tobytes() != plain.tobytes()


# ---- 3. a reset at a position that is no multiple of 375 ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pos", [1000, 2 ** 31 + 7])
def test_reset_takes_the_rotators_row_of_its_position(G, audio, whole, pos):
    assert pos % 375
    frames, first = _streamed(G, [audio[:700001], X.s16_to_f32(audio[700001:])], reset=pos, carrier=FC)
    assert first == pos and frames.shape == whole.shape
    # the same sums (they do not depend on the origin), another row: undo one rotation in binary64, apply the other
    table = G.frontend_rotator().astype(np.float64)
    r = table[:, 0] + 1j * table[:, 1]
    i = np.arange(FL)
    z0 = whole[0][:, 0].astype(np.float64) + 1j * whole[0][:, 1]
    z1 = frames[0][:, 0].astype(np.float64) + 1j * frames[0][:, 1]
    want = z0 * np.conj(r[CX.rot_index(FC, i)]) * r[CX.rot_index(FC, pos + i)]
    assert np.abs(z1 - want).max() <= 1e-6 * np.abs(z0).max()
    assert np.abs(z1 - z0).max() > 0.1 * np.abs(z0).max()
    # and to the bit: the sums from the door, rotated by the stream index
    import torch
    ctx = G.Context(options={"carrier": FC})
    try:
        out = torch.empty((FL, 2), dtype=torch.float32, device="cuda:0")
        ctx.debug_frontend_launch(torch.from_numpy(audio).to("cuda:0"), 0, out, 0)
        s = out.cpu().numpy()
    finally:
        ctx.close()
    assert frames[0].tobytes() == CX.rotate(s, FC, pos + i, G.frontend_rotator()).tobytes()


# ---- 4. a refused option change leaves the stream unharmed ----------------------------------------------------------------
@pytest.mark.gpu
def test_a_refused_option_change_leaves_the_stream_unharmed(G, audio, whole):
    pieces = [audio[:500000], audio[500000:900000], audio[900000:]]
    refused = []

    def between(ctx, i):
        if i != 1:
            return
        for name, bad, good in (("carrier", 1501, FC), ("frontend_hbw", 40, 10)):
            ctx.set_option(name, bad)
            with pytest.raises(G.UwsprError) as e:
                ctx.stream_push_audio(pieces[1])
            refused.append(e.value.status)
            ctx.set_option(name, good)
        for name, bad in (("carrier", 19), ("carrier", 5981), ("frontend_hbw", 0), ("frontend_hbw", 151)):
            with pytest.raises(G.UwsprError):
                ctx.set_option(name, bad)
    frames, pos = _streamed(G, pieces, between=between, carrier=FC)
    assert refused == [-6, -6] and pos == 0 and frames.tobytes() == whole.tobytes()


# ---- 5. the pipe -----------------------------------------------------------------------------------------------------------
def _closed_loop_f64(n):
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    return float(rec["tx_gain"]) * tx + float(rec["whales_gain"]) * wh


@pytest.fixture(scope="module")
def three_carriers():
    """the closed-loop mix's band 1500 +- 150 Hz, and that band moved to 497 and to 2203 Hz, summed (masked first, so
    the copies do not stack their noise) -> float32, frames enough for three"""
    n = 32 * (FL + 2 * HOP) + 4000
    x = _closed_loop_f64(n)
    band = CX.shift_band(x, 1350.0, 1650.0, 0)
    return (band + CX.shift_band(x, 1350.0, 1650.0, 497 - 1500) + CX.shift_band(x, 1350.0, 1650.0, 2203 - 1500)).astype(np.float32)


def _run(G, feed, **opts):
    o = dict(OPTS)
    o.update(opts)
    pipe = G.Pipe(**o)
    try:
        feed(pipe)
        pipe.flush()
        return pipe.collect(cap=1 << 20), pipe
    finally:
        pipe.close()


def _feed(x, step=250000):
    def feed(pipe):
        for k in range(0, x.shape[0], step):
            pipe.push_audio(x[k: k + step])
    return feed


@pytest.mark.gpu
def test_pipe_planes_are_one_channel_one_carrier_pipes(G, three_carriers):
    carriers = [1500, 2203, 1100]
    rec = np.load(os.path.join(GOLDEN, "150613_1920_int16.npz"))["x"]
    n = three_carriers.shape[0]
    ch1 = (np.resize(rec, n).astype(np.float32) / np.float32(32768)).astype(np.float32)
    xx = np.ascontiguousarray(np.stack([three_carriers, ch1], 1))
    recs, pipe = _run(G, _feed(xx), carriers=carriers)
    assert len(recs) > 0 and recs["decoded"].any()
    assert (recs["channel"] >= 0).all() and (recs["channel"] < 6).all()
    assert pipe.split_plane(4) == (1, 2203) and pipe.split_plane(2) == (0, 1100)
    seen = 0
    for c in range(2):
        for k, fc in enumerate(carriers):
            got = recs[recs["channel"] == c * 3 + k].copy()
            got["channel"] = 0
            want, _ = _run(G, _feed(np.ascontiguousarray(xx[:, c])), carriers=[fc])
            assert (want["channel"] == 0).all()
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), (c, fc)
            seen += len(got)
    assert seen == len(recs)
    # (take, plane, frame): planes rise within a take, frames rise from take to take
    prev_q, take_max, prev_max = None, -1, -1
    for r in recs:
        q, f = int(r["channel"]), int(r["frame"])
        if prev_q is not None and q < prev_q:
            prev_max = take_max
        assert f > prev_max
        take_max, prev_q = max(take_max, f), q


@pytest.mark.gpu
def test_one_default_carrier_is_the_default_pipe(G, three_carriers):
    before = G.frontend_carrier_launch_counts()
    a, _ = _run(G, _feed(three_carriers))
    b, _ = _run(G, _feed(three_carriers), carriers=[1500])
    c, _ = _run(G, _feed(three_carriers), carriers=[1500], frontend_hbw=10)
    assert G.frontend_carrier_launch_counts() == before           # the forms there were
    assert len(a) > 0 and a.tobytes() == b.tobytes() == c.tobytes()


@pytest.mark.gpu
def test_three_carriers_decode_the_controls_text(G, three_carriers):
    control, _ = _run(G, _feed(three_carriers))
    dec = control[control["decoded"] != 0]
    texts = {G.unpack_message(r["message"])[1] for r in dec}
    assert texts == {"VE3EMB FN25 30"}                            # a default pipe hears it once per frame
    recs, pipe = _run(G, _feed(three_carriers), carriers=[497, 1500, 2203])
    want = sorted((int(r["frame"]), int(r["stream_pos"]), float(r["coarse"]["freq"])) for r in dec)
    for k, fc in enumerate([497, 1500, 2203]):
        got = recs[(recs["channel"] == k) & (recs["decoded"] != 0)]
        assert {G.unpack_message(r["message"])[1] for r in got} == {"VE3EMB FN25 30"}, fc
        assert sorted((int(r["frame"]), int(r["stream_pos"]), float(r["coarse"]["freq"])) for r in got) == want, fc
        assert all(pipe.split_plane(r["channel"]) == (0, fc) for r in got)


@pytest.mark.gpu
def test_decode_wav_names_the_carrier(G, three_carriers, tmp_path):
    import wave
    x = np.clip(np.rint(three_carriers * 32768.0), -32768, 32767).astype(np.int16)
    path = str(tmp_path / "fdma.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(x.tobytes())
    got = G.decode_wav(path, carriers=[497, 1500, 2203], **OPTS)
    assert {d["carrier"] for d in got} == {497, 1500, 2203} and all("channel" not in d for d in got)
    assert {d["text"] for d in got} == {"VE3EMB FN25 30"}
    per = {fc: sorted((d["frame"], d["t"], d["freq"]) for d in got if d["carrier"] == fc) for fc in (497, 1500, 2203)}
    assert per[497] == per[1500] == per[2203] and len(per[1500]) > 0
    plain = G.decode_wav(path, **OPTS)
    assert all("carrier" not in d for d in plain) and sorted((d["frame"], d["t"], d["freq"]) for d in plain) == per[1500]


# ---- 6. the pipe's argument errors -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipe_refuses_bad_carriers_and_goes_on(G):
    x = np.zeros((1000, 5), np.float32)
    pipe = G.Pipe(**OPTS)
    try:
        for bad in ([1500, 1500], [], [2203, 497, 2203], [19], [5981]):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_carriers(bad)
            assert e.value.status == -6, bad
        with pytest.raises(G.UwsprError):
            pipe.set_option("frontend_hbw", 0)
        with pytest.raises(G.UwsprError):
            pipe.set_option("frontend_hbw", 151)
        pipe.set_carriers(list(range(1000, 1013)))                # 13 carriers x 5 channels = 65 planes
        with pytest.raises(G.UwsprError) as e:
            pipe.push_audio(x)
        assert e.value.status == -6
        pipe.set_carriers([25])                                   # in range at hb 1, not at the pipe's 10
        with pytest.raises(G.UwsprError) as e:
            pipe.push_audio(x)
        assert e.value.status == -6
        pipe.set_carriers(list(range(1000, 1012)))                # 60 planes
        pipe.push_audio(x)
        for late in ([1500], list(range(1000, 1012))):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_carriers(late)                           # after a push
            assert e.value.status == -6
        with pytest.raises(G.UwsprError):
            pipe.set_option("frontend_hbw", 11)
        pipe.push_audio(x)
        pipe.flush()
        assert len(pipe.collect()) == 0
    finally:
        pipe.close()
