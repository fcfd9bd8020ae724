"""K0's carrier form to the bit: what uwspr_debug_frontend_carrier_launch writes -- one launch of k0_frontend<T, true,
true>, the kernel a stream runs for any carriers but {1500 Hz} at 10 Hz -- against tests/carrier_exact.py, with the
library's own binary32 taps and rotator table.  All device comparisons are tobytes() equality.

How every output gets its check without restating every one of them: at carrier fc the sums s come from the door of the
forms WITHOUT a rotator (uwspr_debug_frontend_launch with the context's "carrier" = fc: the same chains, other taps) and
are themselves held to the restatement on the outputs tests/test_gpu_frontend_exact.py picks (a launch's first 16, its
workgroup seam, its last 16); the carrier form must then equal rotate(s) on EVERY output, a multi-plane launch must
equal its one-plane launches on every output, and a few planes are restated end to end."""
import ctypes as C

import numpy as np
import pytest

import carrier_exact as CX
import frontend_exact as X

NAN_FILL = 0x7FC5A5A5
NOUTS = (1, 511, 512, 513, 1025)
CARRIERS = ((1500, 10), (1875, 10), (1501, 10), (497, 10), (2203, 10), (170, 150), (5830, 150))
SHAPES = ((1, 1), (1, 2), (3, 1), (2, 5), (8, 8), (1, 64), (64, 1))
M_FIRSTS = (0, 374, 375, 2 ** 31 + 7, 2 ** 40 + 11)
J = 216


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _filled(npairs):
    import torch
    return torch.full((npairs, 2), NAN_FILL, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _is_fill(a):
    return (np.ascontiguousarray(a).view(np.uint32) == NAN_FILL).all()


def _picked(nout):
    m = np.concatenate([np.arange(0, 16), np.arange(504, 520), np.arange(nout - 16, nout)])
    return np.unique(m[(m >= 0) & (m < nout)])


@pytest.fixture(scope="module")
def ctxs(G):
    made = {}

    def get(hb):
        if hb not in made:
            made[hb] = G.Context(options={"frontend_hbw": hb})
        return made[hb]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def table(G):
    return G.frontend_rotator()


_TAPS = {}


def _taps(G, fc, hb):
    if (fc, hb) not in _TAPS:
        g, D = G.frontend_design(0, 0, centre=fc, half_bw=hb)
        assert D == 0 and X.taps_J(len(g)) == J
        _TAPS[(fc, hb)] = g.astype(np.complex64)
    return _TAPS[(fc, hb)]


def _sums(ctx, fc, audio, in0, m_first, nout, nin, nch=1, plane=None):
    """the sums at carrier fc from the forms without a rotator -> [nch, nout, 2]"""
    plane = nout if plane is None else plane
    ctx.set_option("carrier", fc)
    try:
        out = _filled(nch * plane + 8)
        ctx.debug_frontend_launch(audio, in0, out, m_first, nch=nch, plane=plane, nout=nout, nin=nin)
        o = out.cpu().numpy()
    finally:
        ctx.set_option("carrier", 1500)
    assert _is_fill(o[nch * plane:])
    return np.stack([o[b * plane: b * plane + nout] for b in range(nch)])


def _carrier(ctx, carriers, audio, in0, m_first, nout, nin, nch=1, gap=37):
    """one launch of the carrier form -> [nch * NC, nout, 2]; nothing is written between or behind the planes"""
    npl = nch * len(carriers)
    plane = nout + gap
    out = _filled(npl * plane + 64)
    ctx.debug_frontend_carrier_launch(audio, in0, out, m_first, carriers, nch=nch, plane=plane, nout=nout, nin=nin)
    o = out.cpu().numpy()
    assert _is_fill(o[npl * plane:])
    for q in range(npl):
        assert _is_fill(o[q * plane + nout: (q + 1) * plane]), q
    return np.stack([o[q * plane: q * plane + nout] for q in range(npl)])


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1. every carrier, both formats, the launch sizes: sums held to the restatement, every output to rotate(sums) -------
@pytest.mark.gpu
@pytest.mark.parametrize("fc,hb", CARRIERS)
def test_one_plane_is_the_restated_sums_through_the_rotator(G, ctxs, table, fc, hb):
    ctx = ctxs(hb)
    g32 = _taps(G, fc, hb)
    m_first = 1000
    in0 = 32 * (m_first - J)
    nin_of = lambda n: 32 * (n - 1 + J) + 1
    xs = X.noise16(np.random.default_rng(fc), nin_of(max(NOUTS)))
    xf = X.s16_to_f32(xs)
    ms = np.unique(np.concatenate([_picked(n) for n in NOUTS]))
    want = X.restate(g32, 0, xf, in0, m_first + ms)
    assert want.any(-1).all()
    before = G.frontend_carrier_launch_counts()
    for dt, x in (("int16", xs), ("float32", xf)):
        d = _dev(x)
        for nout in NOUTS:
            s = _sums(ctx, fc, d, in0, m_first, nout, nin_of(nout))[0]
            sel = ms[ms < nout]
            assert _same(s[sel], want[ms < nout]), (dt, nout)
            y = _carrier(ctx, [fc], d, in0, m_first, nout, nin_of(nout))[0]
            assert _same(y, CX.rotate(s, fc, m_first + np.arange(nout), table)), (dt, nout)
            if fc % 375 == 0:
                assert _same(y, s)
            else:
                assert not _same(y, s)
    after = G.frontend_carrier_launch_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (len(NOUTS), len(NOUTS))     # the carrier form ran, per format


# ---- 2. channels x carriers: the planes of one launch are the one-plane launches, in plane order c NC + k --------------
@pytest.mark.gpu
@pytest.mark.parametrize("nch,NC", SHAPES)
def test_planes_of_a_launch_are_its_one_plane_launches(G, ctxs, table, nch, NC):
    ctx = ctxs(10)
    pool = [1501, 497, 2203, 1875, 1500] + [600 + 37 * i for i in range(59)]
    carriers = pool[:NC]
    assert len(set(carriers)) == NC
    nouts = (513,) if nch * NC >= 64 else (1, 511, 512, 513, 1025)
    m_first = 2 ** 31 + 7
    in0 = 32 * (m_first - J)
    nin_of = lambda n: 32 * (n - 1 + J) + 1
    xs = X.noise16(np.random.default_rng(1000 * nch + NC), (nin_of(max(nouts)), nch))
    xf = X.s16_to_f32(xs)
    d16, d32 = _dev(xs), _dev(xf)
    one16 = [_dev(xs[:, c]) for c in range(nch)]
    for nout in nouts:
        got = _carrier(ctx, carriers, d16, in0, m_first, nout, nin_of(nout), nch=nch)
        assert _same(got, _carrier(ctx, carriers, d32, in0, m_first, nout, nin_of(nout), nch=nch)), nout
        for k, fc in enumerate(carriers):
            if nch * NC >= 64 and k % 9 and k != NC - 1:
                continue                                          # (every plane is compared below; one-plane launches thinned)
            for c in range(nch):
                if nch >= 64 and c % 9 and c != nch - 1:
                    continue
                one = _carrier(ctx, [fc], one16[c], in0, m_first, nout, nin_of(nout))[0]
                assert _same(got[c * NC + k], one), (nout, c, k)
        # every plane, every output: the sums of (channel, carrier) from the forms without a rotator, rotated
        for k, fc in enumerate(carriers):
            s = _sums(ctx, fc, d16, in0, m_first, nout, nin_of(nout), nch=nch, plane=nout + 3)
            for c in range(nch):
                assert _same(got[c * NC + k], CX.rotate(s[c], fc, m_first + np.arange(nout), table)), (nout, c, k)
    # and end to end against the restatement: a few outputs of every plane of the small shapes, of some of the large
    nout = nouts[-1]
    ms = m_first + np.array([0, 1, nout // 2, nout - 1]) if nout > 1 else m_first + np.array([0])
    ms = np.unique(ms)
    ks = list(range(NC)) if NC <= 8 else [0, 31, 63]
    cs = list(range(nch)) if nch <= 8 else [0, 31, 63]
    want = CX.restate_planes([_taps(G, carriers[k], 10) for k in ks], 0, table, [carriers[k] for k in ks],
                             xf[:, cs], in0, ms)
    for i, c in enumerate(cs):
        for j, k in enumerate(ks):
            assert _same(got[c * NC + k][ms - m_first], want[i * len(ks) + j]), (c, k)


# ---- 3. origins: m_first decides the rotator's row and nothing else -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fc", [1501, 2203, 1875])
def test_origins_and_short_buffers(G, ctxs, table, fc):
    ctx = ctxs(10)
    nout, nch = 600, 2
    nin = 32 * (nout - 1 + J) + 1
    rng = np.random.default_rng(300 + fc)
    x = np.stack([X.noise32(rng, nin) for _ in range(nch)], 1)
    d_x = _dev(x)
    lead = np.full((77, nch), np.nan, np.float32)
    d_lead = _dev(np.concatenate([lead, x]))
    cut = nin - 32 * 100 + 17
    one_at = 4001
    s0 = _sums(ctx, fc, d_x, 32 * (0 - J), 0, nout, nin, nch=nch, plane=nout + 5)
    assert s0.any(-1).all()
    for m_first in M_FIRSTS:
        in0 = 32 * (m_first - J)
        ms = m_first + np.arange(nout)

        def both(audio, i0, n_in):
            s = _sums(ctx, fc, audio, i0, m_first, nout, n_in, nch=nch, plane=nout + 5)
            y = _carrier(ctx, [fc], audio, i0, m_first, nout, n_in, nch=nch)
            for c in range(nch):
                assert _same(y[c], CX.rotate(s[c], fc, ms, table)), (m_first, c)
            return s
        s = both(d_x, in0, nin)
        assert _same(s, s0), m_first                                        # (the sums do not depend on the origin)
        assert _same(both(d_lead, in0 - 77, nin + 77), s0), m_first         # the buffer starts sooner: NaN never read
        s_late = both(d_x[4000:].contiguous(), in0 + 4000, nin - 4000)      # starts late
        assert not _same(s_late[:, :200], s0[:, :200]) and _same(s_late[:, 260:], s0[:, 260:])
        s_cut = both(d_x, in0, cut)                                         # ends soon
        assert _same(s_cut[:, :nout - 110], s0[:, :nout - 110]) and not _same(s_cut, s0)
        s_one = both(d_x[one_at:].contiguous(), in0 + one_at, 1)            # one sample
        for c in range(nch):
            assert _same(s_one[c], X.impulse_expect(_taps(G, fc, 10), 0, nout, [(in0 + one_at, x[one_at, c])], m_first=m_first))
    # the rows the origins choose differ (374 | 375 | 2^31 + 7 ...) unless the carrier is an identity one
    rows = {int(CX.rot_index(fc, [m])[0]) for m in M_FIRSTS}
    assert (len(rows) == 1) == (fc % 375 == 0)


# ---- 4. a NaN sample reaches its own windows of every carrier of its channel and of no other channel -----------------
@pytest.mark.gpu
def test_a_nan_sample_stays_in_its_channel(G, ctxs, table):
    ctx = ctxs(10)
    nout, nch = 700, 3
    carriers = [1875, 2203, 1501]
    m_first = 375
    in0 = 32 * (m_first - J)
    nin = 32 * (nout - 1 + J) + 1
    rng = np.random.default_rng(44)
    x = np.stack([X.noise32(rng, nin) for _ in range(nch)], 1)
    n0 = 32 * (J + 300) + 5
    x[n0, 1] = np.nan
    y = _carrier(ctx, carriers, _dev(x), in0, m_first, nout, nin, nch=nch)
    k = 32 * (m_first + np.arange(nout)) - (in0 + n0)                       # the tap that meets the sample (D = 0)
    hit = (k >= 0) & (k < 32 * J)                                           # (the image's zero padding multiplies it too)
    assert 0 < hit.sum() == J
    for c in range(nch):
        for kk in range(len(carriers)):
            nan = np.isnan(y[c * 3 + kk]).any(-1)
            assert (nan == (hit if c == 1 else np.zeros(nout, bool))).all(), (c, kk)
    s = _sums(ctx, 1875, _dev(x), in0, m_first, nout, nin, nch=nch, plane=nout)
    assert _same(y[3], s[1]) and np.isnan(s[1]).any()                       # the identity carrier: the sums' bytes, NaN included


# ---- 5. identity carriers are the multichannel form; the default set does not run the carrier form -------------------
@pytest.mark.gpu
def test_identity_carriers_equal_the_multichannel_form(G, ctxs):
    ctx = ctxs(10)
    nout, nch = 1025, 3
    m_first = 374
    in0 = 32 * (m_first - J)
    nin = 32 * (nout - 1 + J) + 1
    xs = X.noise16(np.random.default_rng(55), (nin, nch))
    d = _dev(xs)
    for fc in (1500, 1875, 375, 5625):
        mc = _sums(ctx, fc, d, in0, m_first, nout, nin, nch=nch, plane=nout + 11)
        assert _same(_carrier(ctx, [fc], d, in0, m_first, nout, nin, nch=nch), mc), fc
    both = _carrier(ctx, [1875, 1500], d, in0, m_first, nout, nin, nch=nch)
    assert _same(both[1::2], _sums(ctx, 1500, d, in0, m_first, nout, nin, nch=nch, plane=nout))


@pytest.mark.gpu
def test_the_default_set_runs_the_forms_there_were(G):
    x = X.noise16(np.random.default_rng(66), 32 * 4000)
    for opts, ran in (({}, False), ({"carrier": 1500, "frontend_hbw": 10}, False), ({"carrier": 2203}, True),
                      ({"frontend_hbw": 11}, True)):
        before = G.frontend_carrier_launch_counts()
        ctx = G.Context(options=opts)
        try:
            ctx.stream_open(3375, 2)
            ctx.stream_push_audio(x)
            ctx.stream_push_audio(x.astype(np.float32))
            ctx.frontend(x[None, :20000].astype(np.float32))
            ctx.synchronize()
        finally:
            ctx.close()
        after = G.frontend_carrier_launch_counts()
        assert (sum(after) > sum(before)) == ran, (opts, before, after)


# ---- 6. the door's argument errors ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_door_refuses_bad_arguments_and_goes_on(G, ctxs):
    ctx = ctxs(10)
    nout, nch = 40, 2
    nin = 32 * (nout - 1 + J) + 1
    x = _dev(X.noise32(np.random.default_rng(400), nin * nch))
    out = _filled(64 * (nout + 1))
    f = ctx.L.uwspr_debug_frontend_carrier_launch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_longlong, C.c_longlong]
    f.restype = C.c_int
    a, o = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())

    def call(car, nch_=nch, nout_=nout, plane=nout, fmt=0, nin_=nin):
        arr = np.array(car, np.int32)
        return f(ctx.h, a, fmt, nin_, 0, nch_, len(car), C.c_void_p(arr.ctypes.data), o, nout_, 0, plane)
    assert call([2203, 497]) == 0
    for bad in (call([19]), call([5981]), call([2203] * 33), call([2203], nch_=0), call([2203], nout_=0), call([2203], plane=nout - 1),
                call([2203], fmt=2), call([2203], nin_=0), call(list(range(100, 165)), nch_=1)):
        assert bad == -6
    assert call([2203, 497]) == 0
