"""K0 (12 kS/s audio -> 375 S/s) held to the bit: every instantiation of k0_frontend<float|int16_t, MC> and every way
in -- the batch call, the stream form through its launcher (uwspr_debug_frontend_launch), the stream itself -- against
tests/frontend_exact.py, the numpy restatement of the kernel's own binary32 sums.  All device comparisons are
tobytes() equality.

The tolerance tests (tests/test_frontend.py, tests/test_gpu_audio_stream.py: 1e-5 of the peak against the float64
chain) cannot see more than half the composite filter: the CPU tests below measure that (a kernel that loses the first
256 taps, or the last 8-tap block of every phase, stays 4 orders under that bound) and show that the byte expectations
the GPU tests use do see it.

CPU tests (no mark): fma32 against rational arithmetic, restate against a float64 convolution, the mutation checks.
GPU tests: (a) impulse trains, (b) dense noise at the edges, (c) the four instantiations, (d) origins up to 2^40,
(e) the stream at large positions, (f) the door's argument errors."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import frontend_exact as X

OLD_TOL = 1e-5                      # the max-norm bound of the tolerance tests, relative to the output's peak
NAN_FILL = 0x7FC5A5A5               # a quiet NaN no arithmetic here produces


@pytest.fixture(scope="module")
def taps(G):
    """mode -> (g32: frontend_design(mode, 0) rounded to binary32, what frontend_tap_image stores; D; J)"""
    out = {}
    for mode in (0, 1):
        g, D = G.frontend_design(mode, 0)
        g32 = g.astype(np.complex64)
        out[mode] = (g32, D, X.taps_J(len(g32)))
    assert (len(out[0][0]), out[0][1], out[0][2]) == (6831, 0, 216) and (len(out[1][0]), out[1][1], out[1][2]) == (1025, 512, 40)
    return out


# =============================================================== CPU =================================================
def _round32(fr):
    """a rational, correctly rounded to binary32 (ties to even; the binary32 normal range)"""
    if fr == 0:
        return np.float32(0)
    sgn, fr = (-1, -fr) if fr < 0 else (1, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length() - 24
    while fr >= Fraction(2) ** (e + 24):
        e += 1
    while fr < Fraction(2) ** (e + 23):
        e -= 1
    assert -149 <= e <= 104
    n = fr / Fraction(2) ** e                                   # in [2^23, 2^24)
    q, rem = divmod(n.numerator, n.denominator)
    twice = 2 * rem
    if twice > n.denominator or (twice == n.denominator and (q & 1)):
        q += 1
    return np.float32(sgn * float(np.ldexp(float(q), e)))


def _exact32(a, b, c):
    return np.array([_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float32)


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    """20 000 random triples, the addend over eleven decades around the product (cancellation included)"""
    rng = np.random.default_rng(11)
    n = 20000
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    c = (a.astype(np.float64) * b.astype(np.float64) * rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.5, 5.5, n)).astype(np.float32)
    c[:500] = (-(a[:500].astype(np.float64) * b[:500].astype(np.float64))).astype(np.float32)      # near-total cancellation
    c[500:600] = 0.0
    got = X.fma32(a, b, c)
    want = _exact32(a, b, c)
    assert got.tobytes() == want.tobytes()


def _tie_cases(n):
    """a * b + c a hair off a binary32 rounding tie: c = an odd-or-even multiple N of u = 2^e, a * b = +-(u / 2)
    (1 - i^2 2^-46) from a = 1 + i 2^-23, b = 1 - 2 i 2^-24 (scaled by powers of two), so the exact value is
    (N +- 1/2) u -+ i^2 2^-47 u: within i^2 2^-70 <= 2^-53 (i < 362) of the tie, on the side of c.  The binary64 sum
    of the exact product and c rounds ONTO the tie (the offset is under half its last place), and the cast then
    rounds to even: wrong whenever N is odd."""
    rng = np.random.default_rng(12)
    i = rng.integers(1, 362, n).astype(np.float64)
    e = rng.integers(-20, 11, n)
    s1 = rng.integers(-12, 13, n)
    sign_p = rng.choice([-1.0, 1.0], n)
    N = rng.integers(1 << 23, 1 << 24, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)
    a = np.ldexp(1.0 + i * 2.0 ** -23, s1)
    b = sign_p * np.ldexp(1.0 - 2.0 * i * 2.0 ** -24, e - 1 - s1)
    c = np.ldexp(N, e)
    a32, b32, c32 = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    assert (a32 == a).all() and (b32 == b).all() and (c32 == c).all()
    return a32, b32, c32


def test_fma32_on_rounding_ties_where_double_rounding_fails():
    a, b, c = _tie_cases(2400)
    exact = [Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)) for x, y, z in zip(a, b, c)]
    # every case lies within 2^-53 (relative) of the midpoint of two neighbouring binary32 values, and not on it
    for fr, z in zip(exact, c):
        u = Fraction(float(np.spacing(np.float32(abs(z)))))
        tie = Fraction(float(z)) + (u / 2 if fr > Fraction(float(z)) else -u / 2)
        assert 0 < abs(fr - tie) <= abs(tie) * Fraction(1, 2 ** 53)
    want = np.array([_round32(fr) for fr in exact], np.float32)
    assert (want == c).all()                                    # the side of c, always
    got = X.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    nwrong = int((naive != want).sum())
    print("tie cases %d, naive binary64 evaluation wrong on %d, fma32 wrong on %d" % (len(a), nwrong, int((got != want).sum())))
    assert nwrong >= 100
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("mode", [0, 1])
def test_restate_matches_a_float64_convolution(taps, mode):
    """1 300 outputs of unit noise: the restated binary32 sums against the same taps and samples convolved in
    binary64.  Bound 1e-6 of the peak (3x the 3.2e-7 measured for the grc mode; 6 912 fused multiply-adds of
    unit-variance terms in 16 chains round off at about sqrt(6912 / 16) x 2^-24 of a chain, well inside it)."""
    g32, D, J = taps[mode]
    x = X.noise32(np.random.default_rng(13 + mode), 32 * 1400)
    ms = np.arange(50, 1350)
    y = X.restate(g32, D, x, 0, ms)
    z = X.convolve64(g32, D, x, 0, ms)
    err = np.abs(y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64) - z).max() / np.abs(z).max()
    print("mode %d: restate vs float64, 1300 outputs: %.3g of the peak" % (mode, err))
    assert err <= 1e-6


def _rel_change(a, b):
    za = a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)
    zb = b[..., 0].astype(np.float64) + 1j * b[..., 1].astype(np.float64)
    return np.abs(za - zb).max() / np.abs(za).max()


@pytest.mark.parametrize("mode", [0, 1])
def test_each_mutation_changes_the_byte_expectations(taps, mode):
    """What today's 1e-5 bound cannot see and the byte expectations of (a) and (b) below can: every mutation of
    frontend_exact.mutate_taps changes bytes of both.  In the grc mode (6 831 taps, the filter the gap was measured on)
    the tap-dropping ones do so while moving the output by less than the old bound, which is asserted.  In the compact
    mode 256 taps are a quarter of the 1 025-tap filter and losing them moves the output by percents: there the old
    bound does see them, the figure is printed and the byte change alone is asserted."""
    g32, D, J = taps[mode]
    ximp, want_imp = X.impulse_case(mode, g32, D)
    xd, ms, want_dense, past = X.dense_case(mode, g32, D)
    _, trains = X.impulse_trains()
    for name in X.MUTATIONS:
        gm = X.mutate_taps(g32, name)
        assert len(gm) == 32 * J
        imp = np.stack([X.impulse_expect(gm, D, X.NOUT_BATCH, t) for t in trains])
        dense = X.restate(gm, D, xd, 0, ms)
        assert imp.tobytes() != want_imp.tobytes(), name
        assert dense.tobytes() != want_dense.tobytes(), name
        ci, cd = _rel_change(want_imp, imp), _rel_change(want_dense, dense)
        print("mode %d %-20s impulse trains: %6d outputs change, %.3g of the peak; dense edges: %4d change, %.3g of the peak"
              % (mode, name, int((imp != want_imp).any(-1).sum()), ci, int((dense != want_dense).any(-1).sum()), cd))
        if name in X.TAP_DROPS and mode == 0:
            assert ci < OLD_TOL and cd < OLD_TOL, (name, ci, cd)


# =============================================================== GPU =================================================
@pytest.fixture(scope="module")
def ctxs(G):
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = G.Context(options={"frontend": mode})
        return made[mode]
    yield get
    for c in made.values():
        c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _filled(npairs):
    import torch
    return torch.full((npairs, 2), NAN_FILL, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _host(t):
    return t.cpu().numpy()


def _is_fill(a):
    return (np.ascontiguousarray(a).view(np.uint32) == NAN_FILL).all()


# ---- a. impulse trains ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_impulse_trains_pin_every_tap_to_its_place_and_bits(G, taps, ctxs, mode):
    """uwspr_frontend_batch on 3 records of isolated impulses (every residue mod 32, n0 = 0 and nin - 1, row 0, either
    side of a multiple of 16 384): all 3 x 45 000 outputs are one rounding of tap x amplitude, or +0."""
    g32, D, J = taps[mode]
    x, want = X.impulse_case(mode, g32, D)
    _, trains = X.impulse_trains()
    pos = np.array([n0 for t in trains for n0, _ in t])
    assert set(pos % 32) == set(range(32)) and 0 in pos and X.IMP_NIN - 1 in pos and ((pos % 32 == 0) & (pos > 0)).any()
    assert {16383, 16385} <= set(pos.tolist()) and X.IMP_NIN % 32 != 0
    got = ctxs(mode).frontend(x)
    assert got.shape == want.shape
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(-1))
    assert got.tobytes() == want.tobytes(), (len(bad), bad[:5].tolist())


# ---- b. dense noise at the record's edges and a workgroup seam ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_dense_noise_at_the_edges_equals_the_restatement(G, taps, ctxs, mode):
    g32, D, J = taps[mode]
    x, ms, want, past = X.dense_case(mode, g32, D)
    assert not want[ms >= past].any() and want[ms == past - 1].any()
    got = ctxs(mode).frontend(x[None])[0]
    bad = ms[(got[ms].view(np.uint32) != want.view(np.uint32)).any(-1)]
    assert got[ms].tobytes() == want.tobytes(), (len(bad), bad[:8].tolist())
    assert got[past:].tobytes() == np.zeros_like(got[past:]).tobytes()       # +0, sign included, to the frame's end


# ---- c. the four instantiations through the door -------------------------------------------------------------------
DOOR_M_FIRST = 1000
DOOR_NOUTS = (1, 8, 511, 512, 513, 1031)
DOOR_MORE = {3: (1600,), 7: (2051,)}     # 4 and 5 workgroups per channel: grids of 12 and 35


def _door_nouts(nch):
    return (513,) if nch == 64 else DOOR_NOUTS + DOOR_MORE.get(nch, ())


def _picked(nout):
    """48 outputs of a launch: its first, its workgroup seam, its last"""
    m = np.concatenate([np.arange(0, 16), np.arange(504, 520), np.arange(nout - 16, nout)])
    return np.unique(m[(m >= 0) & (m < nout)])


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [1, 2, 3, 5, 7, 64])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation_through_the_launcher(G, taps, ctxs, mode, nch):
    g32, D, J = taps[mode]
    ctx = ctxs(mode)
    nouts = _door_nouts(nch)
    # workgroups per launch over the whole parametrisation: grids smaller than the 8 of xcd_swizzle, and every
    # remainder mod 8 of a larger one
    grids = {(-(-n // 512)) * c for c in (1, 2, 3, 5, 7, 64) for n in _door_nouts(c)}
    assert grids >= {1, 3, 9, 35, 128} and {g % 8 for g in grids if g >= 8} == set(range(8))
    in0 = 32 * (DOOR_M_FIRST + D // 32 - J)                      # the stream's own convention
    nin = 32 * (max(nouts) - 1 + J) + 1                          # the last output's newest sample is the buffer's last
    xs = X.noise16(np.random.default_rng(100 * mode + nch), (nin, nch))      # [frames][channels], each its own noise
    assert xs.min() == -32768 and xs.max() == 32767
    xf = X.s16_to_f32(xs)
    ms = np.unique(np.concatenate([_picked(n) for n in nouts]))
    want = X.restate_many(g32, D, [(np.ascontiguousarray(xf[:, b]), in0, DOOR_M_FIRST + ms) for b in range(nch)])
    ref = {}
    for dt, x in (("int16", xs), ("float32", xf)):
        d_all = _dev(x)
        d_one = [_dev(x[:, b]) for b in range(nch)]
        for nout in nouts:
            plane = nout + 37
            one = []
            for b in range(nch):                                 # MC = false, one channel at a time
                out = _filled(nout + 64)
                ctx.debug_frontend_launch(d_one[b], in0, out, DOOR_M_FIRST, nout=nout, nin=32 * (nout - 1 + J) + 1)
                o = _host(out)
                assert _is_fill(o[nout:]), (dt, nout, b)
                one.append(o[:nout])
                sel = ms[ms < nout]
                assert set(_picked(nout)) <= set(sel)
                assert o[sel].tobytes() == want[b][ms < nout].tobytes(), (dt, nout, b)
            if dt == "int16":
                ref[nout] = one
            else:                                                # float32 fed s / 32768 gives the int16 bytes
                assert all(one[b].tobytes() == ref[nout][b].tobytes() for b in range(nch)), (nout,)
            if nch == 1:
                continue
            out = _filled(nch * plane + 64)                      # MC = true: all channels in one launch
            ctx.debug_frontend_launch(d_all, in0, out, DOOR_M_FIRST, nch=nch, plane=plane, nout=nout,
                                      nin=32 * (nout - 1 + J) + 1)
            o = _host(out)
            assert _is_fill(o[nch * plane:]), (dt, nout)
            for b in range(nch):
                assert o[b * plane: b * plane + nout].tobytes() == one[b].tobytes(), (dt, nout, b)
                assert _is_fill(o[b * plane + nout: (b + 1) * plane]), (dt, nout, b)


# ---- d. origins ---------------------------------------------------------------------------------------------------------
ORIGINS = (0, 1, 511, 2 ** 26 - 300, 2 ** 27 - 300, 2 ** 31 - 300, 2 ** 40 + 7)
ORG_NOUT = 600


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
def test_origins_up_to_2_40_give_the_bytes_of_origin_0(G, taps, ctxs, mode, nch):
    """The same audio with its first output at m_first (audio index 32 m_first crosses 2^31 and 2^32 inside a launch):
    the bytes of m_first = 0; a buffer that starts later, ends sooner or holds one sample: the restatement with the
    missing samples zero; a buffer that starts sooner: no output reads the extra samples (NaN)."""
    g32, D, J = taps[mode]
    ctx = ctxs(mode)
    nout = ORG_NOUT
    nin = 32 * (nout - 1 + J) + 1
    rng = np.random.default_rng(200 + 10 * mode + nch)
    x = np.stack([X.noise32(rng, nin) for _ in range(nch)], 1)               # [frames][channels]
    plane = nout + 37
    shifts = (1, 31, 32, 4000)
    cut = nin - 32 * 100 + 17                                               # ends inside the last 100 outputs' windows
    # the restatement does not depend on where the origin is: computed once, at origin 0, for every m_first below
    i0 = 32 * (D // 32 - J)
    items = [(np.ascontiguousarray(x[s:, b]), i0 + s, np.arange(260)) for s in shifts for b in range(nch)]
    items += [(np.ascontiguousarray(x[:cut, b]), i0, np.arange(nout - 110, nout)) for b in range(nch)]
    want = X.restate_many(g32, D, items)
    want_shift = {(s, b): want[k * nch + b] for k, s in enumerate(shifts) for b in range(nch)}
    want_cut = {b: want[len(shifts) * nch + b] for b in range(nch)}
    one_at = 4001                                                           # nin = 1: that frame alone, as an impulse
    lead = np.full((77, nch), np.nan, np.float32)
    d_x, d_lead = _dev(x), _dev(np.concatenate([lead, x]))

    def launch(audio, in0, m_first, n_in):
        out = _filled(nch * plane + 64)
        ctx.debug_frontend_launch(audio, in0, out, m_first, nch=nch, plane=plane, nout=nout, nin=n_in)
        o = _host(out)
        assert _is_fill(o[nch * plane:])
        for b in range(nch):
            assert _is_fill(o[b * plane + nout: (b + 1) * plane])
        return np.stack([o[b * plane: b * plane + nout] for b in range(nch)])

    base = None
    for m_first in ORIGINS:
        in0 = 32 * (m_first + D // 32 - J)
        got = launch(d_x, in0, m_first, nin)
        if base is None:
            base = got
            assert base.any(-1).all()
        assert got.tobytes() == base.tobytes(), m_first
        for s in shifts:                                                    # the buffer starts s samples later
            got = launch(d_x[s:].contiguous(), in0 + s, m_first, nin - s)
            for b in range(nch):
                assert got[b, :260].tobytes() == want_shift[(s, b)].tobytes(), (m_first, s, b)
            assert got[:, 260:].tobytes() == base[:, 260:].tobytes(), (m_first, s)     # (their windows are whole)
        got = launch(d_lead, in0 - 77, m_first, nin + 77)                   # 77 samples sooner
        assert got.tobytes() == base.tobytes(), m_first
        got = launch(d_x, in0, m_first, cut)                                # ends sooner
        for b in range(nch):
            assert got[b, nout - 110:].tobytes() == want_cut[b].tobytes(), (m_first, b)
        assert got[:, :nout - 110].tobytes() == base[:, :nout - 110].tobytes(), m_first
        got = launch(d_x, in0, m_first, 1)                                  # one sample, behind every tap: +0
        assert got.tobytes() == np.zeros_like(got).tobytes(), m_first
        got = launch(d_x[one_at:].contiguous(), in0 + one_at, m_first, 1)   # one sample that the outputs do meet
        for b in range(nch):
            imp = X.impulse_expect(g32, D, nout, [(in0 + one_at, x[one_at, b])], m_first=m_first)
            assert imp.any() and got[b].tobytes() == imp.tobytes(), (m_first, b)
    # and the restatement's own index arithmetic at the far origin, on a few outputs
    m_first = ORIGINS[-1]
    far = X.restate(g32, D, np.ascontiguousarray(x[:, 0]), 32 * (m_first + D // 32 - J), m_first + np.arange(8))
    assert far.tobytes() == base[0, :8].tobytes()


# ---- e. the stream at large positions ---------------------------------------------------------------------------------
HOP, FL = 3375, 45000


def _one_frame(G, mode, pieces, pos):
    import torch
    ctx = G.Context(options={"frontend": mode})
    try:
        ctx.stream_open(HOP, 4)
        if pos is not None:
            ctx.stream_reset(pos)
        for p in pieces:
            n = ctx.stream_push_audio(p)
        assert n == 1
        out = torch.empty((1, FL, 2), dtype=torch.float32, device="cuda:0")
        first = ctx.stream_take(1, out)
        ctx.synchronize()
        return out.cpu().numpy(), first
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def stream_at_0(G):
    x = X.noise16(np.random.default_rng(300), 46000 * 32, sigma=3000.0)
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = _one_frame(G, mode, [x], None)
        return x, made[mode]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [2 ** 26 - 20000, 2 ** 31 - 20000, 2 ** 40])
@pytest.mark.parametrize("mode", [0, 1])
def test_stream_reset_far_out_equals_a_stream_at_0(G, stream_at_0, mode, pos):
    """uwspr_stream_reset(pos): "the same values as a stream at 0", where the audio index 32 pos crosses 2^31 inside
    the frame, the stream index does, and both are far beyond 32 bits"""
    x, (want, first0) = stream_at_0(mode)
    assert first0 == 0 and want.any()
    got, first = _one_frame(G, mode, [x[:777777], x[777777:]], pos)
    assert first == pos
    assert got.tobytes() == want.tobytes()


# ---- f. the door's argument errors ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_launcher_door_refuses_bad_arguments_and_goes_on(G, taps, ctxs):
    g32, D, J = taps[0]
    ctx = ctxs(0)
    N = G.native
    nout, nch = 40, 2
    nin = 32 * (nout - 1 + J) + 1
    x = _dev(X.noise32(np.random.default_rng(400), nin * nch))
    out = _filled(nch * nout + 64)
    f = ctx.L.uwspr_debug_frontend_launch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong]
    f.restype = C.c_int
    a, o = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    in0 = 32 * (0 - J)
    bad = [(None, N.AUDIO_F32, nin, 1, o, nout, nout), (a, N.AUDIO_F32, nin, 1, None, nout, nout),
           (a, N.AUDIO_F32, 0, 1, o, nout, nout), (a, N.AUDIO_F32, -5, 1, o, nout, nout),
           (a, N.AUDIO_F32, nin, 1, o, 0, nout), (a, N.AUDIO_F32, nin, 1, o, -1, nout),
           (a, N.AUDIO_F32, nin, 0, o, nout, nout), (a, N.AUDIO_F32, nin, -1, o, nout, nout), (a, N.AUDIO_F32, nin, 65, o, nout, nout),
           (a, 2, nin, 1, o, nout, nout), (a, -1, nin, 1, o, nout, nout),
           (a, N.AUDIO_F32, nin, 2, o, nout, nout - 1), (a, N.AUDIO_F32, nin, 2, o, nout, 0)]
    for au, fmt, n_in, n_ch, ou, n_out, pl in bad:
        assert f(ctx.h, au, fmt, n_in, in0, n_ch, ou, n_out, 0, pl) == -6, (fmt, n_in, n_ch, n_out, pl)     # UWSPR_ERR_ARG
    assert f(None, a, N.AUDIO_F32, nin, in0, 1, o, nout, 0, nout) == -6
    ctx.synchronize()
    assert _is_fill(_host(out))
    assert f(ctx.h, a, N.AUDIO_F32, nin, in0, 2, o, nout, 0, nout) == 0      # plane == nout is allowed
    got = _host(out)
    assert _is_fill(got[nch * nout:]) and not np.isnan(got[:nch * nout]).any() and got[:nch * nout].any(-1).all()
    with pytest.raises(ValueError):
        ctx.debug_frontend_launch(x, in0, out, 0, nch=2, plane=nout, nout=nout, nin=nin + 1)    # does not fit the tensor
