"""K7's restatement (tests/transmit_exact.py) checked on the CPU: Philox against its published vectors, the binary32
uniforms at their ends, the tap door against the two designers, the restated chain against exact arithmetic, the
mutations a byte comparison must see, and the quantiser on every exact half.  tests/test_gpu_transmit_exact.py holds the
device to these expectations."""
import numpy as np
import pytest

import transmit_exact as X


@pytest.fixture(scope="module")
def taps(G):
    return G.tx_taps()


# ---- Philox ----------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10, through both forms"""
    for ctr, key, want in KAT:
        assert X.philox4x32_10_int(ctr, key) == want
        got = X.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want
    ctr = np.array([k[0] for k in KAT], np.uint64)
    key = np.array([k[1] for k in KAT], np.uint64)
    assert (X.philox4x32_10(ctr, key) == np.array([k[2] for k in KAT], np.uint64)).all()


def test_philox_vectorised_is_the_integer_form():
    rng = np.random.default_rng(71)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    ctr[:8] = [[0xffffffff, 0, 0, 0], [0, 0xffffffff, 0, 0], [0, 0, 0xffffffff, 0], [0, 0, 0, 0xffffffff],
               [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    got = X.philox4x32_10(ctr, key)
    assert got.dtype == np.uint64 and int(got.max()) < 2 ** 32
    for c, k, g in zip(ctr, key, got):
        assert X.philox4x32_10_int(c, k) == tuple(int(v) for v in g)


def test_gauss_inputs_take_the_counter_and_key_the_kernel_states():
    """(n low, n high, channel, 0) under (seed low, seed high), words 0 and 1"""
    for seed, ch, n in ((0, 0, 0), (0x0123456789abcdef, 5, 2 ** 40 + 5), (2 ** 64 - 1, 63, 2 ** 32 - 1), (2 ** 32, 1, 2 ** 32)):
        r = X.philox4x32_10_int((n & 0xffffffff, n >> 32, ch, 0), (seed & 0xffffffff, seed >> 32))
        u1, u2 = X.gauss_inputs(seed, ch, [n])
        w1, w2 = X.uniforms([r[0]], [r[1]])
        assert u1[0] == w1[0] and u2[0] == w2[0] and float(u2[0]) == (r[1] >> 8) / 2 ** 24
    # every ingredient matters: the high words, the channel, which word feeds which uniform
    a = X.gauss_inputs(7, 2, np.arange(64))
    for other in (X.gauss_inputs(7, 2, np.arange(64) + 2 ** 32), X.gauss_inputs(7 + 2 ** 32, 2, np.arange(64)),
                  X.gauss_inputs(7, 6, np.arange(64))):
        assert (a[0] != other[0]).mean() > 0.9 and (a[1] != other[1]).mean() > 0.9


# ---- u1, u2 as binary32 -------------------------------------------------------------------------------------------------
def test_uniforms_at_their_ends():
    """u1 is in (0, 1], not (0, 1): from 2^23 on, + 0.5f is a tie and rounds to even, and 2^24 - 1 gives exactly 1 -- a
    noise sample of exactly 0.  u2 stays below 1."""
    top = 2 ** 24 - 1
    words = np.array([0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, top - 1, top], np.uint64) << np.uint64(8)
    u1, u2 = X.uniforms(words | np.uint64(0xff), words | np.uint64(0xff))      # (the low 8 bits are dropped)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert u1[0] == np.float32(2.0 ** -25) and u1[1] == np.float32(1.5 * 2.0 ** -24)
    assert u1[2] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)                     # the last half that binary32 holds
    assert u1[3] == np.float32(0.5) and u1[4] == np.float32((2 ** 23 + 2) * 2.0 ** -24)    # ties: down to even, up to even
    assert u1[5] == np.float32((top - 1) * 2.0 ** -24) and u1[6] == np.float32(1.0)
    assert X.gauss_ref(u1[6:], u2[:1])[0] == 0.0
    assert u2[0] == 0 and u2[6] == np.float32(top * 2.0 ** -24) and u2[6] < 1
    every = np.arange(0, 2 ** 24, dtype=np.uint64) << np.uint64(8)
    u1, u2 = X.uniforms(every, every)
    assert u1.min() > 0 and u1.max() == 1 and u2.min() == 0 and u2.max() < 1
    assert np.isfinite(X.gauss_ref(u1[::4097], u2[::4097])).all()


# ---- the taps ----------------------------------------------------------------------------------------------------------
def test_tap_door_is_the_two_designers_composite(taps):
    import frontend_grc as F
    g, image = taps
    assert g.shape == (X.NT,) and g.dtype == np.complex128 and image.shape == (X.DEC, X.T, 2) and image.dtype == np.float32
    h1 = F.low_pass(1, 12000, 200, 10).astype(np.float64)
    h2r = F.xlating_taps(F.low_pass(1, 12000, 2500, 100), 1500.0).astype(np.complex128)
    want = np.convolve(h1, h2r) * np.exp(-1j * np.pi * np.arange(len(h1) + len(h2r) - 1) / 4)
    assert len(want) == X.NT
    assert np.abs(g - want).max() <= 1e-7 * np.abs(want).max()
    small = int((np.abs(g) < 2e-6).sum())
    print("taps below 2e-6: %d of %d" % (small, X.NT))
    assert small > 300


def test_tap_image_is_the_phase_split_of_the_taps(taps):
    g, image = taps
    want = np.zeros((X.DEC, X.T, 2), np.float32)
    for p in range(X.DEC):
        for i in range(X.T):
            q = p + X.DEC * i
            if q < X.NT:
                want[p, i] = (np.float32(g[q].real), np.float32(-g[q].imag))
    assert image.tobytes() == want.tobytes()                    # (+0 behind the last tap, sign included)


# ---- the chain against exact arithmetic -----------------------------------------------------------------------------------
def test_chain_stays_within_the_bound_of_a_208_step_chain(taps):
    """dense random baseband, |x| <= 2: the restated chain against a binary64 evaluation of the same sum, within
    208 2^-24 sum_i |g| |x| (each of the 208 fused multiply-adds rounds once, by at most 2^-24 of a partial sum that
    sum_i |g| |x| bounds, to first order)"""
    _, image = taps
    rng = np.random.default_rng(72)
    nbb = 700
    r, ph = 2.0 * np.sqrt(rng.uniform(0, 1, nbb)), rng.uniform(0, 2 * np.pi, nbb)
    x = (r * np.cos(ph)).astype(np.float32), (r * np.sin(ph)).astype(np.float32)
    assert np.hypot(x[0].astype(np.float64), x[1].astype(np.float64)).max() <= 2.0 + 1e-6
    n = np.arange(X.DEC * (X.T - 1), X.DEC * nbb, dtype=np.int64)
    got = X.chain(image, x, n)
    ref, mag = X.chain64(image, x, n)
    err = np.abs(got.astype(np.float64) - ref)
    print("chain vs binary64: worst %.3g of the bound" % (err / (208 * 2.0 ** -24 * mag)).max())
    assert (err <= 208 * 2.0 ** -24 * mag).all()
    assert (got != 0).all()


# ---- the mutations ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(G, taps):
    """the middle window of the GPU tests' dense case (transmit_exact.dense_signals at start 3000), its baseband from
    the float64 model rounded to binary32 (the device's differs in the last place of some samples: the same signal)"""
    _, image = taps
    sigs = X.dense_signals(3000)
    t0, nf = X.dense_windows(3000)["middle"]
    j0, nbb = X.window(t0, nf)
    j0 -= 1                                                      # (room for window_off_by_one)
    y = X.baseband_model(sigs, G.wspr_symbols, j0, nbb + 1)
    x = y.real.astype(np.float32), (-y.imag).astype(np.float32)
    n = np.arange(t0, t0 + nf, dtype=np.int64)
    return image, x, j0, n, X.chain(image, x, n, x0=j0)


@pytest.mark.parametrize("name", X.MUTATIONS)
def test_byte_expectations_see_the_mutation(dense, name):
    image, x, j0, n, want = dense
    got = X.chain(image, x, n, x0=j0, mutation=name)
    changed = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("%s: %d of %d outputs change" % (name, changed, len(n)))
    assert changed >= 1
    if name == "drop_one_small_tap":
        p, i = X.small_tap(image)
        assert 0 < np.hypot(*image[p, i].astype(np.float64)) < 2e-6
        assert (n[got != want] % X.DEC == p).all()              # only that tap's phase


# ---- the quantiser -----------------------------------------------------------------------------------------------------------
def test_quantise_rounds_every_exact_half_to_even():
    k, b = X.exact_halves()
    assert len(b) == 65536 and b.dtype == np.float32
    prod = np.float32(32767.0) * b
    assert prod.dtype == np.float32 and (prod.astype(np.float64) == k + 0.5).all()
    lo = np.floor(k + 0.5)
    even = np.where(lo % 2 == 0, lo, lo + 1)
    want = np.clip(even, -32768, 32767).astype(np.int16)
    got = X.quantise(b)
    assert got.dtype == np.int16 and got.tobytes() == want.tobytes()
    assert got.min() == -32768 and got.max() == 32767
    away = np.clip(np.where(k + 0.5 > 0, lo + 1, lo), -32768, 32767)
    differ = int((away != want).sum())
    print("round-half-away disagrees on %d of 65536" % differ)
    assert 32000 <= differ <= 33536


def test_quantise_clamps_before_it_rounds():
    v = np.array([1.0, 1.00002, 1.25, -1.0, -1.00002, -1.00004, -1.25, 0.0, -0.0, 1e30, -1e30], np.float32)
    assert X.quantise(v).tolist() == [32767, 32767, 32767, -32767, -32768, -32768, -32768, 0, 0, 32767, -32768]


def test_compose_adds_only_what_the_kernel_adds():
    c = np.array([0.25, -0.5, 1.0 / 3], np.float32)
    g = np.array([1.5, -2.0, 0.75], np.float32)
    n = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1], np.int64)
    assert X.compose(c, None, 0.0, None, 0.5, n).tobytes() == c.tobytes()
    s = np.float32(0.37)
    assert X.compose(c, g, 0.37, None, 0.5, n).tobytes() == (c + s * g).astype(np.float32).tobytes()
    bg = np.array([100, -200, 300, 32767, -32768, 5, 6], np.int16)
    idx = [(2 ** 32 - 1 + i) % 7 for i in range(3)]
    want = (c + s * g) + np.float32(0.5) * (bg[idx].astype(np.float32) / np.float32(32768))
    assert X.compose(c, g, 0.37, bg, 0.5, n).tobytes() == want.astype(np.float32).tobytes()
    bf = np.array([0.125, -0.3], np.float32)
    want = c + np.float32(0.5) * bf[[(2 ** 32 - 1 + i) % 2 for i in range(3)]]
    assert X.compose(c, g, 0.0, bf, 0.5, n).tobytes() == want.astype(np.float32).tobytes()
