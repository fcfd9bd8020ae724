"""K7's medium form on the device (uwspr_tx_render_medium, uwspr_tx_baseband_medium): Doppler-spread fading per signal,
impulsive noise per audio channel.  The faded baseband is held to the binary64 model of tests/medium_exact.py under the
bound of the unfaded one times the largest gain possible; everything behind the baseband -- the carrier groups' chains,
the AWGN, the impulses, the background, the quantiser -- is held to the byte, given the device's own baseband and its
own Gaussian draws.  tests/test_medium.py shows on the CPU that these expectations see the mistakes of
medium_exact.MUTATIONS.

1 defaults  2 faded baseband  3 faded render  4 pieces and placement  5 impulses alone  6 composition  7 refusals
8 closed loops"""
import numpy as np
import pytest

import medium_exact as MX
import transmit_carrier_exact as TC
import transmit_exact as X
from test_gpu_transmit_exact import NOISE_BOUND

NTX = X.NTX
HOP, FL = 3375, 45000


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(G):
    return G.frontend_rotator()


_images = {}


def _image(G, fc):
    if fc not in _images:
        _images[fc] = G.tx_design(fc, 2500)[1]
    return _images[fc]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _where(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return "shapes %s %s" % (a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else np.flatnonzero(a != b)
    return "%d of %d differ, first at %d: %r against %r" % (len(bad), len(a), bad[0] if len(bad) else -1, a[bad[:1]], b[bad[:1]])


def _device(ctx, sigs, nf, fmt="f32", channels=1, **kw):
    import torch
    dev = torch.empty((nf, channels), dtype=torch.int16 if fmt == "s16" else torch.float32, device="cuda:0")
    ctx.tx_render(sigs, nf, format=fmt, channels=channels, out=dev, **kw)
    return dev.cpu().numpy()


def _expect(G, ctx, table, sigs, t0, off, channel=0):
    """the chain of outputs t0 + off of one channel (transmit_carrier_exact.expect), the baseband of every carrier group
    being the device's own -- faded where its signals fade"""
    j0, nbb = X.window(t0, int(off.max()) + 1)
    groups = {}
    for s in sigs:
        if s.get("channel", 0) == channel:
            groups.setdefault(s.get("carrier", 1500), []).append(s)
    for fc in groups:
        x = X.file_orientation(ctx.tx_baseband(groups[fc], nbb, t0=j0, channel=channel))
        groups[fc] = (_image(G, fc), x)
    return TC.expect(groups, t0 + off, j0, table)


def _err(got, ref):
    return max(np.abs(got[:, 0] - ref.real).max(), np.abs(got[:, 1] - ref.imag).max())


NOFADE = {"spread": 1.0, "paths": 0}


# ================================================================ 1. defaults ================================================
@pytest.mark.gpu
def test_without_fades_and_impulses_the_old_kernels_give_the_old_bytes(G, ctx):
    """an all-paths = 0 fade array, impulses that are off (rate 0; sigma 0; a rate under 2^-32), and NULL for both, through
    the new calls: the bytes of tx_render / tx_baseband, f32 and s16, host and device, and no medium or carrier launch"""
    import ctypes as C
    N = G.native
    sigs = X.dense_signals(3000) + [dict(s, channel=1, start=s["start"] + 50) for s in X.dense_signals(3000)[:2]]
    t0, nf = X.dense_windows(3000)["middle"]
    kw = dict(t0=t0, channels=2, sigma=0.02, seed=[3, 4])
    plain = {fmt: ctx.tx_render(sigs, nf, format=fmt, **kw) for fmt in ("f32", "s16")}
    bb = ctx.tx_baseband(sigs, 2000, t0=30000)
    before = (G.tx_medium_launch_counts(), G.tx_carrier_launch_counts())
    unfaded = [dict(s, fading=NOFADE) for s in sigs]
    assert G.tx_fades(unfaded) is not None
    off = [{"rate": 0.0, "sigma": 1.0, "length": 8}, {"rate": 0.25, "sigma": 0.0}]
    for fmt in ("f32", "s16"):
        for s_, imp in ((unfaded, None), (sigs, off), (unfaded, off), (sigs, {"rate": 2.0 ** -33, "sigma": 5.0})):
            a = ctx.tx_render(s_, nf, format=fmt, impulses=imp, **kw)
            assert _same(a, plain[fmt]), (fmt, _where(a, plain[fmt]))
        assert _same(_device(ctx, unfaded, nf, fmt=fmt, impulses=off, **kw), plain[fmt]), fmt
    assert _same(ctx.tx_baseband(unfaded, 2000, t0=30000), bb)
    # NULL fade and NULL impulse arrays, straight through the C entry points
    arr = G.tx_signals(sigs)
    ch = (N.TxChannel * 2)()
    for k in range(2):
        ch[k].sigma, ch[k].seed = 0.02, 3 + k
    out = np.empty((nf, 2), np.float32)
    assert N.lib().uwspr_tx_render_medium(ctx.h, C.byref(arr), None, None, None, len(sigs), C.byref(ch), None, 2, t0, nf,
                                          N.AUDIO_F32, C.c_void_p(out.ctypes.data), N.HOST) == 0
    assert _same(out, plain["f32"])
    iq = np.empty((2000, 2), np.float32)
    assert N.lib().uwspr_tx_baseband_medium(ctx.h, C.byref(arr), None, None, None, len(sigs), 0, 30000, 2000,
                                            C.c_void_p(iq.ctypes.data), N.HOST) == 0
    assert _same(iq, bb)
    assert (G.tx_medium_launch_counts(), G.tx_carrier_launch_counts()) == before


# ================================================================ 2. the faded baseband ======================================
@pytest.mark.gpu
@pytest.mark.parametrize("start", [3000, -20000], ids=["start_3000", "negative_start"])
def test_faded_baseband_matches_the_float64_model(G, ctx, start):
    """the shared case -- a Rayleigh-faded, an unfaded and a Rician transmission in one channel, added in ascending index
    -- around k = 0, around k = 41471 and from the middle of the transmissions.  Bound: the 1e-6 of
    test_baseband_extremes_match_the_float64_model per unit gain, times gain (a0 + a1 M), summed over the signals."""
    sigs = MX.faded_signals(start)
    bound = MX.faded_bound(sigs)
    before = G.tx_medium_launch_counts()
    for name, (t0, n) in MX.faded_windows(start).items():
        got = ctx.tx_baseband(sigs, n, t0=t0)
        ref = MX.faded_model(sigs, G.wspr_symbols, t0, n)
        err = _err(got, ref)
        print("start %d, %s: faded baseband error %.3g (bound %.3g)" % (start, name, err, bound))
        assert err <= bound, (name, err)
        assert np.abs(ref).max() > 0.2
        import torch
        dev = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
        ctx.tx_baseband(sigs, n, t0=t0, out=dev)
        assert _same(dev.cpu().numpy(), got)
    t0, n = MX.faded_windows(start)["k0"]
    got = ctx.tx_baseband(sigs, n, t0=t0)
    assert (got[:5] == 0).all() and np.abs(got[5]).max() > 0         # k = 0 is the first sample that sounds
    t0, n = MX.faded_windows(start)["k_last"]
    last = start + 2911 + NTX - 1 - t0
    got = ctx.tx_baseband(sigs, n, t0=t0)
    assert np.abs(got[last]).max() > 0 and (got[last + 1:] == 0).all()   # k = 41471 the last
    # the unfaded signal of the mix alone is the bytes of the old kernel: fading one signal does not touch another
    t0, n = MX.faded_windows(start)["middle"]
    alone = ctx.tx_baseband([dict(sigs[1], fading=NOFADE), dict(sigs[0], gain=0.0)], n, t0=t0)
    assert _same(alone, ctx.tx_baseband([sigs[1]], n, t0=t0)) and np.abs(alone).max() > 0.5
    after = G.tx_medium_launch_counts()
    assert after[2] - before[2] == 9 and after[:2] == before[:2]


MOTIONS = {"static_model": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "static"},
           "doppler": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "doppler"},
           "delay": {"v": (2.0, -2.0), "p": (0.0, 50.0), "model": "delay"},
           "delay_absolute_spreading": {"v": (1.0, -0.5), "p": (0.0, 600.0), "t": 3.0, "model": "delay", "absolute": True,
                                        "spreading": True}}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MOTIONS))
def test_faded_baseband_under_each_motion_model(G, ctx, name):
    """h is indexed by the reception index k = j - start, an integer under every model: DELAY's k' only moves theta"""
    s = {"text": "K1ABC FN42 37", "start": 375, "f0": 3.1, "drift": 1.7, "phase0": 0.4, "gain": 0.9, "fading": MX.RAYLEIGH,
         "motion": MOTIONS[name]}
    bound = MX.faded_bound([s])
    shift = 375 * 600 // 1500 if "absolute" in name else 0          # the travel time R / c in samples, about
    for t0, n in ((370 + shift - 20, 1500), (20000, 1500), (375 + NTX + shift - 1400, 1500)):
        got = ctx.tx_baseband([s], n, t0=t0)
        ref = MX.faded_model([s], G.wspr_symbols, t0, n)
        err = _err(got, ref)
        print("%s, t0 %d: faded baseband error %.3g (bound %.3g)" % (name, t0, err, bound))
        assert err <= bound, (name, t0, err)
        assert np.abs(ref).max() > 0.05 and (np.abs(ref) == 0).any() == (t0 != 20000)
    if name == "static_model":
        still = dict(s, motion=None)
        assert _same(ctx.tx_baseband([s], 1500, t0=20000), ctx.tx_baseband([still], 1500, t0=20000))


@pytest.mark.gpu
def test_one_path_is_a_doppler_shift(G, ctx):
    """paths = 1, K = 0: the unfaded signal at f0 + nu_0 with phase0 + phi_0, within the same bound"""
    _, _, om, ph = MX.fade_design(MX.SHIFT_ONLY)
    s = {"text": "VE3EMB FN25 30", "start": 1000, "f0": -7.0, "drift": 0.5, "phase0": 0.25, "gain": 0.8}
    for t0, n in ((990, 2000), (30000, 2000)):
        faded = ctx.tx_baseband([dict(s, fading=MX.SHIFT_ONLY)], n, t0=t0)
        moved = ctx.tx_baseband([dict(s, f0=s["f0"] + om[0] * 375.0 / (2 * np.pi), phase0=s["phase0"] + ph[0])], n, t0=t0)
        err = np.abs(faded - moved).max()
        print("one path against the shifted signal: %.3g (bound %.3g)" % (err, 1e-6 * 0.8))
        assert err <= 1e-6 * 0.8 and np.abs(faded).max() > 0.5
        assert np.abs(faded - ctx.tx_baseband([s], n, t0=t0)).max() > 0.5


# ================================================================ 3. the faded render ========================================
def _restated(t0, nf):
    seam = 32 * (t0 // 32) + X.TILE - t0
    mid = seam + X.TILE // 2 + 5
    off = np.concatenate([np.arange(16), np.arange(seam - 512, seam + 512), np.arange(mid, mid + 2048), np.arange(nf - 16, nf)])
    return np.unique(off[(off >= 0) & (off < nf)]).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", [None, "doppler", "delay"])
def test_faded_render_is_the_restated_chain(G, ctx, table, motion):
    """two carrier groups in one channel -- 497 Hz (a Rician signal) and 1500 Hz (a Rayleigh one, moving or not, and an
    unfaded one) --: byte for byte the carrier form's restated chain on the device's own faded baseband, f32 and s16,
    host and device"""
    m = None if motion is None else MOTIONS[motion]
    sigs = [{"text": "K1ABC FN42 37", "start": 3000, "f0": 2.0, "drift": 0.5, "phase0": 0.3, "fading": MX.RAYLEIGH, "motion": m},
            {"text": "VE3EMB FN25 30", "start": 3100, "f0": -3.0, "gain": 0.6, "carrier": 497, "fading": MX.RICIAN},
            {"text": "PJ4/K1ABC 37", "start": 2500, "f0": 40.0, "gain": 0.5}]
    t0, nf = 32 * 23000 + 9, X.WINDOW
    off = _restated(t0, nf)
    before = G.tx_medium_launch_counts()
    got = ctx.tx_render(sigs, nf, t0=t0)
    want = _expect(G, ctx, table, sigs, t0, off)
    assert (want != 0).sum() > len(off) // 2
    assert _same(got[off, 0], want), (motion, _where(got[off, 0], want))
    assert _same(_device(ctx, sigs, nf, t0=t0), got)
    s16 = ctx.tx_render(sigs, nf, t0=t0, format="s16")
    assert _same(s16[:, 0], X.quantise(got[:, 0])) and _same(_device(ctx, sigs, nf, fmt="s16", t0=t0), s16)
    after = G.tx_medium_launch_counts()
    assert after[0] - before[0] == 2 and after[1] - before[1] == 2     # the medium instances are what ran
    unfaded = [{k: v for k, v in s.items() if k != "fading"} for s in sigs]
    assert not _same(ctx.tx_render(unfaded, nf, t0=t0), got)


# ================================================================ 4. pieces and placement ====================================
@pytest.mark.gpu
def test_pieces_concatenate_and_host_equals_device(G, ctx):
    """faded signals, AWGN and bursts of 3: pieces cut at odd lengths -- inside a 16384-sample tile, at n = 16383 and at
    n = 16384 -- concatenate to one render's bytes; a burst that straddles a cut is added by both pieces' renders"""
    sigs = MX.faded_signals(20000)
    t0, nf = 32 * 40000, 3 * X.TILE
    kw = dict(sigma=0.01, seed=11, impulses=dict(MX.IMPULSE, sigma=0.3, rate=1.0 / 50))
    for fmt in ("f32", "s16"):
        whole = ctx.tx_render(sigs, nf, t0=t0, format=fmt, **kw)
        for cuts in ((5, 16383, 16384, 20001, 33333), (1, 16384, 32767, 32769)):
            edges = [0] + list(cuts) + [nf]
            parts = [ctx.tx_render(sigs, b - a, t0=t0 + a, format=fmt, **kw) for a, b in zip(edges[:-1], edges[1:])]
            assert _same(np.concatenate(parts), whole), (fmt, cuts)
        assert _same(_device(ctx, sigs, nf, fmt=fmt, t0=t0, **kw), whole), fmt
    cnt = MX.impulse_support(kw["impulses"], 0, t0, nf)
    assert (cnt > 1).any()                                         # bursts overlap in this render


# ================================================================ 5. impulses alone ==========================================
def _alone(ctx, imp, t0, nf, channels=1, **kw):
    return ctx.tx_render([], nf, t0=t0, channels=channels, impulses=imp, **kw)


def _draw_errors(got, imp, ch, t0, nf):
    """where exactly one burst sample lands on an output, |got - ref| in units of 2^-24 r (test_gpu_transmit_exact's
    measure), for impulses of sigma 1"""
    cnt = MX.impulse_support(imp, ch, t0, nf)
    errs = []
    for d, off, e in MX.impulse_terms(imp, ch, t0, nf):
        one = cnt[off] == 1
        u1, u2 = MX.impulse_inputs(imp, ch, e[one], d)
        r = X.gauss_radius(u1)
        ref = MX.impulse_ref(u1, u2)
        ok = r > 0
        errs.append(np.abs(got[off[one]].astype(np.float64) - ref)[ok] / (2.0 ** -24 * r[ok]))
    return np.concatenate(errs + [np.zeros(1)])


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1, 3, 8])
def test_impulses_alone_sit_on_the_restated_supports(G, ctx, length):
    """no signal, no AWGN, impulse sigma 1: the non-zero samples are exactly the restated supports -- from audio index 0
    (n < length: no negative event index), across a tile boundary, with an event before t0 reaching into the window --
    and a lone burst sample is the binary64 Box-Muller of its own block within the AWGN's bound"""
    imp = dict(MX.IMPULSE, sigma=1.0, length=length)
    before = G.tx_medium_launch_counts()
    ev = MX.impulse_events(imp, 0, 0, 6 * X.TILE)
    reach = int(ev[len(ev) // 2]) + 1                              # a window that begins one sample behind an event
    worst = 0.0
    for t0, nf in ((0, 4000), MX.IMPULSE_WINDOW, (reach, 50), (reach + max(length - 1, 1), 50)):
        got = _alone(ctx, imp, t0, nf)[:, 0]
        cnt = MX.impulse_support(imp, 0, t0, nf)
        assert np.array_equal(got != 0, cnt > 0), (length, t0, np.flatnonzero((got != 0) != (cnt > 0))[:8])
        if cnt.any():
            worst = max(worst, float(_draw_errors(got, imp, 0, t0, nf).max()))
    print("length %d: worst lone burst sample %.3f x 2^-24 r (bound %.1f)" % (length, worst, NOISE_BOUND))
    assert worst <= NOISE_BOUND
    if length > 1:
        assert MX.impulse_support(imp, 0, reach, 50)[0] >= 1       # the event before t0 is heard
    # the burst of an event just before a tile boundary crosses it
    t0, nf = MX.IMPULSE_WINDOW
    assert G.tx_medium_launch_counts()[0] - before[0] == 4
    # thr = 0 (a rate under 2^-32): nothing, and nothing of the medium form runs
    mid = G.tx_medium_launch_counts()
    assert (_alone(ctx, dict(imp, rate=2.0 ** -33), t0, nf) == 0).all() and G.tx_medium_launch_counts() == mid


@pytest.mark.gpu
def test_event_threshold_is_strict_and_tiles_do_not_matter(G, ctx):
    imp, at = MX.edge_impulse(dict(MX.IMPULSE, sigma=1.0, length=1))
    t0, nf = MX.IMPULSE_WINDOW
    got = _alone(ctx, imp, t0, nf)[:, 0]
    assert got[at - t0] == 0                                       # word x == thr: no event
    assert np.array_equal(got != 0, MX.impulse_support(imp, 0, t0, nf) > 0)
    # bursts of 8 across a tile boundary: the first boundary with an event on the tile's last sample, whose other seven
    # samples fall in the next tile
    imp8 = dict(MX.IMPULSE, sigma=1.0, length=8, rate=0.25)
    seam = next(k * X.TILE for k in range(1, 64) if MX.is_event(imp8, 0, [k * X.TILE - 1])[0])
    got = _alone(ctx, imp8, seam - 64, 128)[:, 0]
    cnt = MX.impulse_support(imp8, 0, seam - 64, 128)
    assert np.array_equal(got != 0, cnt > 0) and (cnt[63:71] > 0).all()
    assert _same(np.concatenate([_alone(ctx, imp8, seam - 64, 64), _alone(ctx, imp8, seam, 64)])[:, 0], got)


@pytest.mark.gpu
def test_64_channels_each_with_its_own_stream(G, ctx):
    """one seed for all 64 channels: the channel index in the counter makes 64 streams; per-channel dicts are per channel"""
    imp = dict(MX.IMPULSE, sigma=1.0, length=3)
    t0, nf = MX.IMPULSE_WINDOW
    wide = _alone(ctx, imp, t0, nf, channels=64)
    for ch in (0, 1, 31, 63):
        cnt = MX.impulse_support(imp, ch, t0, nf)
        assert np.array_equal(wide[:, ch] != 0, cnt > 0), ch
        assert _draw_errors(wide[:, ch], imp, ch, t0, nf).max() <= NOISE_BOUND
    supports = {(wide[:, ch] != 0).tobytes() for ch in range(64)}
    assert len(supports) == 64
    assert _same(wide[:, 0], _alone(ctx, imp, t0, nf)[:, 0])
    mixed = _alone(ctx, [None, imp, dict(imp, seed=99), None], t0, nf, channels=4)
    assert (mixed[:, 0] == 0).all() and (mixed[:, 3] == 0).all() and _same(mixed[:, 1], wide[:, 1])
    assert np.array_equal(mixed[:, 2] != 0, MX.impulse_support(dict(imp, seed=99), 2, t0, nf) > 0)


@pytest.mark.gpu
def test_equal_awgn_and_impulse_seeds_give_uncorrelated_draws(G, ctx):
    """counter word 3 keeps the streams apart: with one seed for both, the impulse draws at the events and the AWGN
    draws of the same samples have a correlation within four standard errors 1 / sqrt(N) of 0 -- on the AWGN's own
    blocks (word 3 = 0) it would be 1"""
    imp = {"rate": 0.25, "sigma": 1.0, "seed": 21, "length": 1}
    t0, nf = 7 * X.TILE + 3, X.TILE
    a = ctx.tx_render([], nf, t0=t0, sigma=1.0, seed=21)[:, 0].astype(np.float64)
    b = _alone(ctx, imp, t0, nf)[:, 0].astype(np.float64)
    at = np.flatnonzero(b != 0)
    assert 3500 < len(at) < 4700
    rho = np.corrcoef(a[at], b[at])[0, 1]
    print("correlation over %d events: %.4f (4 / sqrt(N) = %.4f)" % (len(at), rho, 4 / np.sqrt(len(at))))
    assert abs(rho) <= 4 / np.sqrt(len(at))
    # and the events are not where the AWGN's word x is small
    small = X.philox4x32_10(np.stack([np.uint64(t0) + np.arange(nf, dtype=np.uint64) & X.MASK32, np.zeros(nf, np.uint64),
                                      np.zeros(nf, np.uint64), np.zeros(nf, np.uint64)], axis=-1), np.array([21, 0], np.uint64))[:, 0] < 2 ** 30
    assert 0.15 < (small & (b != 0)).sum() / max(small.sum(), 1) < 0.35


# ================================================================ 6. composition =============================================
@pytest.mark.gpu
def test_composition_is_four_roundings(G, ctx, table):
    """chain + fl32(sigma g) + fl32(isigma draw) per burst sample + fl32(gain b): byte for byte given the device's chain,
    its AWGN draws (the sigma = 1 render) and its burst draws (the impulses-alone render at sigma 1, where one burst
    sample lands on an output; the few outputs where two land are left out); impulses of sigma 3 drive the quantiser
    onto both rails"""
    sigs = MX.faded_signals(20000)
    t0, nf = 32 * 40000 + 5, 2 * X.TILE
    n = np.arange(t0, t0 + nf, dtype=np.int64)
    imp = {"rate": 1.0 / 100, "sigma": 3.0, "seed": 21, "length": 3}
    chain32 = ctx.tx_render(sigs, nf, t0=t0)[:, 0]
    g32 = ctx.tx_render([], nf, t0=t0, sigma=1.0, seed=21)[:, 0]
    lone = _alone(ctx, dict(imp, sigma=1.0), t0, nf)[:, 0]
    cnt = MX.impulse_support(imp, 0, t0, nf)
    known = cnt <= 1
    assert (cnt == 1).sum() > 500 and known.mean() > 0.95
    bg = np.random.default_rng(81).uniform(-0.2, 0.2, 777).astype(np.float32)
    terms = [(d, off[cnt[off] == 1], e[cnt[off] == 1]) for d, off, e in MX.impulse_terms(imp, 0, t0, nf)]
    by_off = lambda d, e: lone[(e + d - t0).astype(np.int64)]      # noqa: E731
    want = MX.compose_medium(chain32, g32, 0.05, terms, imp["sigma"], by_off, bg, 0.37, n)
    kw = dict(t0=t0, sigma=0.05, seed=21, impulses=imp, background=bg, background_gain=0.37)
    got = ctx.tx_render(sigs, nf, **kw)[:, 0]
    assert _same(got[known], want[known]), _where(got[known], want[known])
    early = MX.compose_medium(chain32, g32, 0.05, terms, imp["sigma"], by_off, bg, 0.37, n, mutation="impulses_before_awgn")
    assert not _same(early[known], want[known])
    s16 = ctx.tx_render(sigs, nf, format="s16", **kw)[:, 0]
    assert _same(s16, X.quantise(got))
    assert (s16 == 32767).any() and (s16 == -32768).any() and (np.abs(got) > 1.5).any()
    assert _same(_device(ctx, sigs, nf, fmt="s16", **kw)[:, 0], s16)


# ================================================================ 7. refusals ================================================
@pytest.mark.gpu
def test_bad_fades_and_impulses_fail_their_call_only(G, ctx):
    import torch
    N = G.native
    good = MX.faded_signals(3000)
    t0, nf = 32 * 23000 + 9, 4096
    gimp = dict(MX.IMPULSE)
    ref = ctx.tx_render(good, nf, t0=t0, impulses=gimp)
    ref_bb = ctx.tx_baseband(good, 500, t0=23000)
    dev = torch.full((nf, 1), 7.5, dtype=torch.float32, device="cuda:0")

    def refused(sigs, imp=gimp, baseband=True):
        with pytest.raises(N.UwsprError) as e:
            ctx.tx_render(sigs, nf, t0=t0, impulses=imp, out=dev)
        assert e.value.status == -6, e.value
        assert (dev.cpu().numpy() == 7.5).all()                       # the output is untouched
        if baseband:
            with pytest.raises(N.UwsprError) as e:
                ctx.tx_baseband(sigs, 500, t0=23000)
            assert e.value.status == -6, e.value
        assert _same(ctx.tx_render(good, nf, t0=t0, impulses=gimp), ref)   # the context goes on
    for bad in ({"spread": -0.1}, {"spread": 20.5}, {"spread": float("nan")}, {"shift": 21.0}, {"shift": float("-inf")},
                {"k": -1.0}, {"k": 2e6}, {"k": float("nan")}, {"paths": 33}, {"paths": -2}):
        refused([good[0], good[1], dict(good[2], fading=dict(MX.RICIAN, **bad))])
    # a bad entry is refused also where the window drops its signal; paths = 0 makes the entry unread
    far = dict(good[0], start=10 ** 9, fading=dict(MX.RAYLEIGH, spread=99.0))
    refused(good + [far])
    assert _same(ctx.tx_render(good + [dict(far, fading=dict(far["fading"], paths=0))], nf, t0=t0, impulses=gimp), ref)
    for bad in ({"rate": -1e-9}, {"rate": 0.2501}, {"rate": float("nan")}, {"sigma": -1.0}, {"sigma": float("inf")},
                {"length": 0}, {"length": 9}):
        refused(good, dict(gimp, **bad), baseband=False)
    assert _same(ctx.tx_baseband(good, 500, t0=23000), ref_bb)
    for edge in ({"rate": 0.25}, {"length": 8}, {"rate": 0.0}, {"sigma": 0.0}):
        ctx.tx_render(good, nf, t0=t0, impulses=dict(gimp, **edge))


# ================================================================ 8. closed loops ============================================
def _decode_on_device(G, dev, blank=0):
    """a rendered CUDA tensor [n] -> the texts decoded from its first frame: the context's stream front-end (with the
    blanker when asked) and a pipe fed the device frames; the audio never leaves the device"""
    import torch
    c = G.Context(options={"blank": blank} if blank else {})
    pipe = G.Pipe(hop=FL, batch_frames=1, max_per_frame=2, lanes=1)
    try:
        c.stream_open(HOP, 4)
        assert c.stream_push_audio(dev) >= 1
        frames = torch.empty((1, FL, 2), dtype=torch.float32, device="cuda:0")
        c.stream_take(1, frames)
        c.synchronize()
        pipe.submit_device(frames)
        pipe.flush()
        recs = pipe.collect()
    finally:
        pipe.close()
        c.close()
    return sorted(G.unpack_message(r["message"])[1] for r in recs if r["decoded"])


IMPULSE_SEEDS = [0, 1, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", IMPULSE_SEEDS)
def test_impulsive_render_decodes_with_the_blanker_only(G, ctx, seed):
    """"VE3EMB FN25 30" at -22 dB in 2500 Hz plus impulses of probability 1/250 and 60 sigma, rendered, blanked, filtered and
    decoded on the device.  Seeds 0, 1, 2, 3: chosen on the CPU chain of tools/medium_cpu_seeds.py (the golden closed-loop
    transmission, the restated noise and impulses, blank_exact, the float64 front-end, the oracle and the real Fano),
    where all four decode with the blanker and none without; none had to be replaced."""
    import torch
    n = 1440000 + 64
    sigma = G.tx_sigma(-22.0)
    dev = torch.empty((n, 1), dtype=torch.float32, device="cuda:0")
    ctx.tx_render([{"text": "VE3EMB FN25 30", "start": 375}], n, sigma=sigma, seed=seed, out=dev,
                  impulses={"rate": 1.0 / 250, "sigma": 60.0 * sigma, "seed": seed, "length": 1})
    x = dev.reshape(-1)
    off, on = _decode_on_device(G, x), _decode_on_device(G, x, blank=24)
    print("seed %d: blank=0 %r; blank=24 %r" % (seed, off, on))
    assert "VE3EMB FN25 30" in on
    assert not any("VE3EMB" in t for t in off)


FADING_SEEDS = [0, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FADING_SEEDS)
def test_rician_transmission_decodes_through_the_pipe(G, ctx, seed):
    """one Rician transmission (K = 10, spread 0.1 Hz) at -18 dB: the sign and the orientation of h survive the chain.
    Seeds 0, 1: chosen on the CPU at baseband (tools/medium_cpu_seeds.py: the unit transmission times the restated
    gain plus noise, through the oracle and the real Fano), where both decode."""
    import torch
    n = 1440000 + 64
    dev = torch.empty((n, 1), dtype=torch.float32, device="cuda:0")
    ctx.tx_render([{"text": "VE3EMB FN25 30", "start": 375, "f0": 2.0,
                    "fading": {"spread": 0.1, "k": 10.0, "seed": seed, "paths": 16}}], n, sigma=G.tx_sigma(-18.0), seed=100 + seed, out=dev)
    got = _decode_on_device(G, dev.reshape(-1))
    print("fading seed %d: %r" % (seed, got))
    assert "VE3EMB FN25 30" in got
