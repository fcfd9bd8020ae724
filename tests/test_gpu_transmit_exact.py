"""K7 (message symbols -> 375 S/s baseband -> 12 kS/s audio) held to the bit against tests/transmit_exact.py.

The device's binary64 sincos (uwspr_tx_baseband) and its logf / cospif (the sigma = 1 noise render) are taken as given;
everything after them -- the order a channel's signals add up in, the 208-step filter chain, the noise's counter, key and
words, the composition with noise and background, the quantiser, the per-channel signal ranges, the keep filters,
absolute indices beyond 2^32 -- is compared as bytes.  The noise itself is compared with Box-Muller in binary64 on the
restated Philox words, in units of 2^-24 of the radius.  tests/test_transmit_exact.py shows on the CPU that these
expectations see a lost tap under 2e-6, a swapped phase, the other order.

(a) chain bytes, static  (b) baseband order, grid stride, model  (c) noise  (d) composition  (e) quantiser
(f) channel ranges  (g) moving forms"""
import numpy as np
import pytest

import transmit_exact as X

NTX = X.NTX
# (c): the largest |got - ref| / (2^-24 sqrt(-2 ln u1)) measured on an MI355X against gauss_ref is NOISE_E_MEASURED
# (profiles/transmit.txt); the bound is 4 x that, for another release's logf / cospif (a few ulp, not bit-stable), and
# must stay <= 64: a wrong word, counter, key or branch gives an independent draw and a figure in the millions.
NOISE_E_MEASURED = 3.080
NOISE_BOUND = 4.0 * NOISE_E_MEASURED
assert NOISE_BOUND <= 64.0


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def image(G):
    return G.tx_taps()[1]


_expect = {}


def _chain(ctx, image, sigs, t0, nf, key=None):
    """the restated chain of audio [t0, t0 + nf) on the device's own baseband of `sigs` (one channel); kept under `key`"""
    if key is not None and key in _expect:
        return _expect[key]
    j0, nbb = X.window(t0, nf)
    x = X.file_orientation(ctx.tx_baseband(sigs, nbb, t0=j0))
    out = X.chain(image, x, np.arange(t0, t0 + nf, dtype=np.int64), x0=j0)
    if key is not None:
        _expect[key] = out
    return out


def _device(ctx, sigs, nf, fmt="f32", channels=1, **kw):
    import torch
    dev = torch.empty((nf, channels), dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
    ctx.tx_render(sigs, nf, format=fmt, channels=channels, out=dev, **kw)
    return dev.cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _where(a, b):
    """for the assertion message: how many differ, the first index, the values there"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return "shapes %s %s" % (a.shape, b.shape)
    bad = np.flatnonzero((a != b) | (np.signbit(a) != np.signbit(b))) if a.dtype.kind == "f" else np.flatnonzero(a != b)
    return "%d of %d differ, first at %d: %r against %r" % (len(bad), len(a), bad[0] if len(bad) else -1,
                                                           a[bad[:1]], b[bad[:1]])


CROSS32 = 2 ** 32 - 8192 - 5
FAR45 = 2 ** 45 + 49159


def _placement(name):
    """-> (signals, windows) of one placement of the dense case"""
    if name in ("static", "running", "far"):
        start = {"static": 3000, "running": -20000, "far": 2 ** 40}[name]
        return X.dense_signals(start), X.dense_windows(start)
    t0 = {"cross32": CROSS32, "far45": FAR45}[name]
    assert t0 % 32 != 0
    return X.dense_signals(X.start_for_middle(t0)), {"middle": (t0, X.WINDOW)}


# ================================================================ (a) + (e): chain bytes, static ========================
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["static", "running", "far", "cross32", "far45"])
def test_static_render_is_the_restated_chain(G, ctx, image, name):
    """three overlapping signals of one channel, no noise, no background: every f32 output is chain()'s bytes on the
    device's own baseband; host and device output agree; the s16 render is quantise() of the f32 one.  static: start
    3000; running: start -20000, the signals already running at n = 0; far: start 2^40, t0 about 2^45; cross32: the
    window crosses audio index 2^32; far45: t0 = 2^45 + 49159."""
    sigs, windows = _placement(name)
    compared = 0
    for wname, (t0, nf) in sorted(windows.items()):
        assert t0 >= 0
        got = ctx.tx_render(sigs, nf, t0=t0)
        assert got.shape == (nf, 1) and got.dtype == np.float32
        if wname == "before":
            want = np.zeros(nf, np.float32)
        else:
            want = _chain(ctx, image, sigs, t0, nf, key=(name, wname))
            if wname != "one":
                assert (want != 0).sum() > nf // 4, (name, wname)
        assert _same(got[:, 0], want), (name, wname, _where(got[:, 0], want))
        assert _same(_device(ctx, sigs, nf, t0=t0), got), (name, wname)
        s16 = ctx.tx_render(sigs, nf, t0=t0, format="s16")
        assert _same(s16[:, 0], X.quantise(got[:, 0])), (name, wname, _where(s16[:, 0], X.quantise(got[:, 0])))
        assert _same(_device(ctx, sigs, nf, fmt="s16", t0=t0), s16), (name, wname)
        compared += nf
    if name in ("static", "far"):
        t0, nf = windows["first"]                               # the first window holds the first signal's first sample
        edge = 32 * sigs[0]["start"] - t0
        first = _chain(ctx, image, sigs, t0, nf, key=(name, "first"))
        assert 0 < edge < nf and (first[:edge] == 0).all() and (first[edge:edge + 64] != 0).any()
        t0, nf = windows["last"]                                # ... and the last one the last contribution
        edge = 32 * (sigs[2]["start"] + NTX - 1) + X.NT - 1 - t0
        last = _chain(ctx, image, sigs, t0, nf, key=(name, "last"))
        assert 64 < edge < nf - 1 and (last[edge + 1:] == 0).all() and (last[edge - 63:edge + 1] != 0).any()
    print("%s: %d outputs compared as bytes (f32; as many s16)" % (name, compared))


# ================================================================ (b): baseband ==========================================
@pytest.mark.gpu
def test_baseband_adds_a_channels_signals_in_ascending_index(G, ctx):
    sigs = X.dense_signals(3000)
    t0, n = 2950, 44600                                          # before the first signal to behind the last
    whole = ctx.tx_baseband(sigs, n, t0=t0)
    a, b, c = (ctx.tx_baseband([s], n, t0=t0) for s in sigs)
    asc = (a + b) + c
    desc = (c + b) + a
    assert asc.dtype == np.float32
    assert _same(whole, asc), _where(whole, asc)
    differ = int((desc != whole).any(axis=1).sum())
    print("baseband: %d samples compared as bytes; the descending sum differs on %d" % (n, differ))
    assert differ > 0
    # the same list in another order is another sum
    rev = ctx.tx_baseband(sigs[::-1], n, t0=t0)
    assert _same(rev, desc), _where(rev, desc)


@pytest.mark.gpu
def test_baseband_grid_stride_second_trip(G, ctx):
    """2048 x 256 threads: samples from 524 288 on are a thread's second trip"""
    first = 2048 * 256
    sigs = X.dense_signals(0) + X.dense_signals(first - 20000)
    n = first + 4096
    whole = ctx.tx_baseband(sigs, n)
    assert _same(whole[:first], ctx.tx_baseband(sigs, first))
    tail = ctx.tx_baseband(sigs, 4106, t0=first - 10)
    assert _same(whole[first - 10:], tail), _where(whole[first - 10:], tail)
    assert (np.abs(whole[first:]).max(axis=1) > 0).all()
    print("grid stride: %d samples compared as bytes" % (first + 4106))


@pytest.mark.gpu
@pytest.mark.parametrize("start", [3000, -20000, 2 ** 40])
def test_baseband_extremes_match_the_float64_model(G, ctx, start):
    """f0 +-150 Hz, drift +-20 Hz, phase0 +-1e3 rad, at start 3000, -20000 and 2^40: within the 1e-6 of
    tests/test_gpu_transmit.py of the float64 model"""
    sigs = X.dense_signals(start)
    flipped = [dict(s, f0=-s["f0"], drift=-s["drift"], phase0=-s["phase0"]) for s in sigs]
    t0, n = start - 100, 45000
    for ss in (sigs, flipped):
        got = ctx.tx_baseband(ss, n, t0=t0)
        ref = X.baseband_model(ss, G.wspr_symbols, t0, n)
        err = max(np.abs(got[:, 0] - ref.real).max(), np.abs(got[:, 1] - ref.imag).max())
        print("start %d: baseband error %.3g" % (start, err))
        assert err <= 1e-6, (start, err)
        assert (got[:100] == 0).all() and np.abs(got[100:200]).max() > 0


# ================================================================ (c): noise =============================================
SEEDS = [0, 1, 2 ** 32, 0x0123456789abcdef, 2 ** 64 - 1]
RANGES = [(0, 4096), (2 ** 32 - 2048, 4096), (2 ** 40 + 5, 4096)]


def _noise_error(got, seed, ch, n):
    """|got - ref| in units of 2^-24 r, r = sqrt(-2 ln u1); where r = 0 (u1 = 1) the sample must be 0"""
    u1, u2 = X.gauss_inputs(seed, ch, n)
    r = X.gauss_radius(u1)
    ref = X.gauss_ref(u1, u2)
    zero = r == 0
    assert (got[zero] == 0).all()
    return np.abs(got.astype(np.float64) - ref)[~zero] / (2.0 ** -24 * r[~zero])


@pytest.mark.gpu
def test_noise_is_box_muller_on_philox_words_0_and_1(G, ctx):
    worst, compared = 0.0, 0
    for seed in SEEDS:
        for t0, nf in RANGES:
            n = np.arange(t0, t0 + nf, dtype=np.int64)
            wide = ctx.tx_render([], nf, t0=t0, channels=64, sigma=1.0, seed=seed)
            six = ctx.tx_render([], nf, t0=t0, channels=6, sigma=1.0, seed=seed)
            assert _same(wide[:, 5], six[:, 5]), (seed, t0)
            for ch in (0, 1, 5, 63):
                e = _noise_error(wide[:, ch], seed, ch, n)
                assert e.max() <= NOISE_BOUND, (seed, t0, ch, e.max(), int(np.argmax(e)))
                worst = max(worst, float(e.max()))
                compared += nf
            e = _noise_error(six[:, 5], seed, 5, n)
            assert e.max() <= NOISE_BOUND, (seed, t0, e.max())
            compared += nf
    print("noise: %d samples, worst error %.3f x 2^-24 r (bound %.1f)" % (compared, worst, NOISE_BOUND))
    # per-channel seeds are per channel: channel 3 under seed 9 is channel 3 of a render whose other channels differ
    a = ctx.tx_render([], 512, t0=7, channels=4, sigma=1.0, seed=[5, 6, 7, 9])
    b = ctx.tx_render([], 512, t0=7, channels=4, sigma=1.0, seed=9)
    assert _same(a[:, 3], b[:, 3]) and not _same(a[:, 2], b[:, 2])
    assert _noise_error(a[:, 2], 7, 2, np.arange(7, 519)).max() <= NOISE_BOUND


# ================================================================ (d) + (e): composition ===================================
@pytest.mark.gpu
def test_composition_with_noise_and_background_is_three_roundings(G, ctx, image):
    """the middle window across audio index 2^32: chain + fl32(sigma32 g32) + fl32(gain b[n mod len]), g32 the sigma = 1
    render of the same (seed, channel, n), the background index (t0 + i) mod len in Python integers"""
    import torch
    sigs, windows = _placement("cross32")
    t0, nf = windows["middle"]
    n = np.arange(t0, t0 + nf, dtype=np.int64)
    chain32 = _chain(ctx, image, sigs, t0, nf, key=("cross32", "middle"))
    seed = 0x0123456789abcdef
    g32 = ctx.tx_render([], nf, t0=t0, sigma=1.0, seed=seed)[:, 0]
    assert _noise_error(g32, seed, 0, n).max() <= NOISE_BOUND
    rng = np.random.default_rng(81)
    bg16 = rng.integers(-32768, 32768, 16385).astype(np.int16)
    bg16[[0, 16384]] = (-32768, 32767)
    bg7 = rng.uniform(-0.2, 0.2, 7).astype(np.float32)
    bg1 = np.array([-0.0123], np.float32)
    cases = [("s16 background of 16385", 0.37, bg16), ("f32 background of 7", 0.37, bg7), ("background of 1", 0.37, bg1),
             ("no noise", 0.0, bg16), ("no background", 0.37, None)]
    for what, sigma, bg in cases:
        kw = dict(t0=t0, sigma=sigma, seed=seed, background=bg, background_gain=0.5)
        got = ctx.tx_render(sigs, nf, **kw)
        want = X.compose(chain32, g32, sigma, bg, 0.5, n)
        assert _same(got[:, 0], want), (what, _where(got[:, 0], want))
        s16 = ctx.tx_render(sigs, nf, format="s16", **kw)
        assert _same(s16[:, 0], X.quantise(got[:, 0])), (what, _where(s16[:, 0], X.quantise(got[:, 0])))
        dkw = dict(kw, background=None if bg is None else torch.from_numpy(bg).to("cuda:0"))
        assert _same(_device(ctx, sigs, nf, **dkw), got), what
    print("composition: %d outputs compared as bytes in each of %d cases (f32; as many s16)" % (nf, len(cases)))


# ================================================================ (e): quantiser ===========================================
@pytest.mark.gpu
def test_quantiser_reaches_both_rails(G, ctx, image):
    sigs = X.dense_signals(3000)
    sigs[1]["gain"] = 40.0                                       # amplitude 40 / 32 = 1.25
    t0, nf = X.dense_windows(3000)["middle"]
    f32 = ctx.tx_render(sigs, nf, t0=t0)
    want = _chain(ctx, image, sigs, t0, nf)
    assert _same(f32[:, 0], want), _where(f32[:, 0], want)
    assert f32.max() > 1.2 and f32.min() < -1.2
    s16 = ctx.tx_render(sigs, nf, t0=t0, format="s16")
    assert _same(s16[:, 0], X.quantise(f32[:, 0])), _where(s16[:, 0], X.quantise(f32[:, 0]))
    lo, hi = int((s16 == -32768).sum()), int((s16 == 32767).sum())
    print("quantiser: %d outputs compared as bytes, %d at -32768, %d at 32767" % (nf, lo, hi))
    assert lo > 0 and hi > 0
    assert _same(_device(ctx, sigs, nf, fmt="s16", t0=t0), s16)


@pytest.mark.gpu
def test_quantiser_rounds_every_exact_half_to_even(G, ctx):
    """the 65 536 values b_k with fl32(32767 b_k) = k + 0.5 exactly, as a background of gain 1 with nothing else"""
    _, b = X.exact_halves()
    for t0 in (0, 2 ** 32 + 11):
        idx = X.background_index(np.arange(t0, t0 + 65536, dtype=np.int64), 65536)
        f32 = ctx.tx_render([], 65536, t0=t0, background=b, background_gain=1.0)
        assert _same(f32[:, 0], b[idx]), _where(f32[:, 0], b[idx])
        s16 = ctx.tx_render([], 65536, t0=t0, background=b, background_gain=1.0, format="s16")
        want = X.quantise(b[idx])
        assert _same(s16[:, 0], want), _where(s16[:, 0], want)
        assert s16.min() == -32768 and s16.max() == 32767


# ================================================================ (f): channel ranges ======================================
TEXTS = ["K1ABC FN42 37", "PJ4/K1ABC 37", "VE3EMB FN25 30", "G4XYZ/7 10", "W9ZZZ EM10 0"]
SEAM = (1 << 24) // 64                                          # frames per host staging piece at C = 64 (262 144)


def _crowd(G):
    """512 signals over C = 64 in shuffled channel order: channels 1, 31 and 62 empty, channel 63 with twenty, forty
    signals far outside every window used here (the keep filter takes them out of the middle of the list)"""
    rng = np.random.default_rng(82)
    sym = {t: G.wspr_symbols(t) for t in TEXTS}
    free = [c for c in range(63) if c not in (1, 31, 62)]
    chans = [63] * 20 + free + [int(rng.choice(free)) for _ in range(512 - 20 - len(free))]
    assert len(chans) == 512
    sigs = []
    for i, c in enumerate(chans):
        outside = i % 13 == 5
        sigs.append({"symbols": sym[TEXTS[i % len(TEXTS)]], "channel": c,
                     "start": int(rng.integers(10 ** 6, 2 * 10 ** 6)) if outside else int(rng.integers(-30000, 8000)),
                     "f0": float(rng.uniform(-100, 100)), "drift": float(rng.uniform(-4, 4)),
                     "phase0": float(rng.uniform(-np.pi, np.pi)), "gain": float(rng.uniform(0.2, 1.5))})
    assert sum(1 for i in range(512) if i % 13 == 5) >= 39
    order = rng.permutation(512)
    sigs = [sigs[i] for i in order]
    assert [s["channel"] for s in sigs] != sorted(s["channel"] for s in sigs)
    return sigs


@pytest.mark.gpu
def test_every_channel_of_64_renders_its_own_signals(G, ctx):
    sigs = _crowd(G)
    t0, nf = SEAM + 5 - 20003, 2 * X.TILE
    wide = ctx.tx_render(sigs, nf, t0=t0, channels=64)
    zero = np.zeros(nf, np.float32)
    count = {c: sum(1 for s in sigs if s["channel"] == c) for c in range(64)}
    assert count[63] == 20 and count[1] == count[31] == count[62] == 0 and sum(count.values()) == 512
    for c in range(64):
        mine = [dict(s, channel=0) for s in sigs if s["channel"] == c]
        if not mine:
            assert _same(wide[:, c], zero), c
            continue
        alone = ctx.tx_render(mine, nf, t0=t0)
        assert _same(wide[:, c], alone[:, 0]), (c, len(mine), _where(wide[:, c], alone[:, 0]))
        assert (alone != 0).any(), c
    print("channel ranges: %d outputs compared as bytes" % (64 * nf))


@pytest.mark.gpu
def test_host_output_across_the_staging_seam_at_64_channels(G, ctx):
    sigs = _crowd(G)
    t0, nf = 5, SEAM + 20000
    host = ctx.tx_render(sigs, nf, t0=t0, channels=64, format="s16")
    assert _same(_device(ctx, sigs, nf, fmt="s16", channels=64, t0=t0), host)
    a = ctx.tx_render(sigs, SEAM, t0=t0, channels=64, format="s16")
    b = ctx.tx_render(sigs, 20000, t0=t0 + SEAM, channels=64, format="s16")
    assert _same(host[:SEAM], a) and _same(host[SEAM:], b)
    assert (host[SEAM - 100:SEAM + 100, 63] != 0).any() and (host[:, [1, 31, 62]] == 0).all()
    print("staging seam: %d outputs compared as bytes" % (64 * nf))


# ================================================================ (g): moving forms ========================================
@pytest.mark.gpu
def test_moving_render_is_the_restated_chain(G, ctx, image):
    """a DOPPLER signal, a DELAY | ABSOLUTE one 15 km away (10 s: its support begins about 3750 baseband samples after
    `start`, far outside [0, N)), a static one, through uwspr_tx_render_moving"""
    sigs = [{"text": "K1ABC FN42 37", "start": 3000, "f0": 2.0, "drift": 0.5, "phase0": 0.3,
             "motion": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "doppler"}},
            {"text": "VE3EMB FN25 30", "start": 3100, "f0": -3.0, "gain": 0.6,
             "motion": {"v": (1.0, -0.5), "p": (0.0, 15000.0), "model": "delay", "absolute": True}},
            {"text": "PJ4/K1ABC 37", "start": 2500, "f0": 40.0, "gain": 0.5}]
    lead = ctx.tx_baseband([sigs[1]], 6000, t0=3100 + 2000)
    on = np.flatnonzero(np.abs(lead).max(axis=1) > 0)
    assert len(on) and 1000 < on[0] < 2500 and on[-1] == 5999     # about 3750 behind `start`, then on to the end
    j_first = 3100 + 2000 + int(on[0])
    trail = ctx.tx_baseband([sigs[1]], 4000, t0=3100 + NTX + 2000)
    on = np.flatnonzero(np.abs(trail).max(axis=1) > 0)
    assert len(on) and on[0] == 0 and 1000 < on[-1] < 2500
    j_last = 3100 + NTX + 2000 + int(on[-1])
    windows = {"first": (32 * j_first - 20003, X.WINDOW), "inside": (32 * (j_first + 20000) + 9, X.WINDOW),
               "last": (32 * j_last + X.NT - 1 - 30001, X.WINDOW)}
    for wname, (t0, nf) in sorted(windows.items()):
        got = ctx.tx_render(sigs, nf, t0=t0)
        want = _chain(ctx, image, sigs, t0, nf)
        assert _same(got[:, 0], want), (wname, _where(got[:, 0], want))
        s16 = ctx.tx_render(sigs, nf, t0=t0, format="s16")
        assert _same(s16[:, 0], X.quantise(got[:, 0])), wname
        assert _same(_device(ctx, sigs, nf, t0=t0), got), wname
    # before the delayed signal arrives the audio is the other two signals' alone
    t0, nf = 32 * j_first - 20003 - 2 * X.TILE, 2 * X.TILE
    assert t0 > 32 * 3000 + X.NT
    both = ctx.tx_render(sigs, nf, t0=t0)
    others = ctx.tx_render([sigs[0], sigs[2]], nf, t0=t0)
    assert _same(both, others) and (both != 0).sum() > nf // 2
    # ... and where it arrives the three differ from the two
    t0 = 32 * j_first
    assert not _same(ctx.tx_render(sigs, nf, t0=t0), ctx.tx_render([sigs[0], sigs[2]], nf, t0=t0))
    print("moving: %d outputs compared as bytes (f32; as many s16)" % (3 * X.WINDOW + nf))
