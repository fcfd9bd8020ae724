"""K0 at a centre fc and half-bandwidth hb, and the rotator behind it (options "carrier" / "frontend_hbw",
uwspr_frontend_design_at, uwspr_frontend_rotator): everything that needs no GPU.

  * the design at (1500, 10) is the design there always was, and its 1500 Hz rotation takes exact octant values;
  * the composite taps at five (fc, hb) against the independent restatement oracle/frontend_grc.py (its CENTER /
    HALF_BW set from here and restored), within 1e-6 of the largest tap, and its stage-by-stage chain() on 2 s of noise
    against the one-FIR form plus the rotator at 1e-5 of the peak (tests/test_frontend.py's bound);
  * the rotator table within one binary32 ulp of numpy, rot[0] = (1, -0), the index against Python's big integers;
  * the mistakes tests/carrier_exact.py can state each change the expectations;
  * the argument errors of the design call (the pipe's: tests/test_gpu_carrier_stream.py, a pipe needs a device);
  * the two shifted recordings the GPU decode test relies on decode on the CPU chain."""
import os

import numpy as np
import pytest

import carrier_exact as CX
import frontend_exact as X
from conftest import GOLDEN

TOL = 1e-5
CASES = ((497, 10), (2203, 10), (1500, 40), (5830, 150), (170, 150))


@pytest.fixture(scope="module")
def FE():
    import frontend_grc
    return frontend_grc


class _centre:
    """oracle/frontend_grc.py at another centre: its module attributes set and restored"""

    def __init__(self, FE, fc, hb):
        self.FE, self.new = FE, (float(fc), float(hb))

    def __enter__(self):
        self.old = (self.FE.CENTER, self.FE.HALF_BW)
        self.FE.CENTER, self.FE.HALF_BW = self.new
        return self.FE

    def __exit__(self, *a):
        self.FE.CENTER, self.FE.HALF_BW = self.old


# ---- design ---------------------------------------------------------------------------------------------------------
def test_design_at_1500_10_is_the_design(G):
    for stage in range(4):
        a, b = G.frontend_design(0, stage), G.frontend_design(0, stage, centre=1500, half_bw=10)
        if stage == 0:
            assert a[1] == b[1] == 0
            a, b = a[0], b[0]
        assert len(a) == (6831, 2891, 2891, 1051)[stage] and a.tobytes() == b.tobytes(), stage
    (a, da), (b, db) = G.frontend_design(1, 0), G.frontend_design(1, 0, centre=1500, half_bw=10)
    assert da == db == 512 and len(a) == 1025 and a.tobytes() == b.tobytes()
    # the tap image the kernel gets is these taps rounded to binary32: equal taps, equal image; hb does not reach mode 1
    assert G.frontend_design(1, 0, centre=1500, half_bw=77)[0].tobytes() == a.tobytes()


def test_the_1500_hz_rotation_takes_exact_octant_values(G):
    """libm's cos(pi / 2) is 6e-17, not 0: the compact taps at 1500 Hz have exact zeros and exactly equal parts where
    the mixer's angle is a multiple of pi / 4, as they always had -- and not at 1501 Hz"""
    g, D = G.frontend_design(1, 0)
    o = (D - np.arange(len(g))) % 8
    assert (g.real[(o == 2) | (o == 6)] == 0).all() and (g.imag[(o == 0) | (o == 4)] == 0).all()
    odd = (o % 2) == 1
    assert (np.abs(g.real[odd]) == np.abs(g.imag[odd])).all() and np.abs(g[odd]).min() > 0
    g1, _ = G.frontend_design(1, 0, centre=1501)
    assert (g1.real[(o == 2) | (o == 6)] != 0).sum() > 200


def test_tap_counts_do_not_depend_on_the_centre(G):
    for fc, hb in CASES:
        g, D = G.frontend_design(0, 0, centre=fc, half_bw=hb)
        assert (len(g), D, X.taps_J(len(g))) == (6831, 0, 216)
        assert [len(G.frontend_design(0, s, centre=fc, half_bw=hb)) for s in (1, 2, 3)] == [2891, 2891, 1051]


@pytest.mark.parametrize("fc,hb", CASES)
def test_composite_taps_match_the_independent_restatement(G, FE, fc, hb):
    g, D = G.frontend_design(0, 0, centre=fc, half_bw=hb)
    with _centre(FE, fc, hb):
        want = FE.composite_taps()
        stages = FE.stage_taps()
    assert (FE.CENTER, FE.HALF_BW) == (1500.0, 10.0)
    assert D == 0 and len(g) == len(want)
    assert np.abs(g - want).max() <= 1e-6 * np.abs(want).max()
    for s, h in zip((1, 2, 3), stages):
        got = G.frontend_design(0, s, centre=fc, half_bw=hb)
        assert np.abs(got - h).max() <= 2.0 ** -22 * np.abs(h).max(), s
    # and it passes its own band: unit gain at the centre, 50 dB down beyond what the / 32 would alias
    H = np.abs(np.fft.fft(g, 1 << 18))
    f = np.fft.fftfreq(1 << 18, 1 / 12000.0)
    assert abs(H[np.abs(f - fc) < 2.0] - 1.0).max() < 2e-2
    if hb <= 40:    # (at hb 150 the band-pass's first side lobes, 53 dB down, lie where the resampler has not cut yet)
        assert H[np.abs(f - fc) > 375.0 / 2].max() < 10 ** (-50 / 20.0)


@pytest.mark.parametrize("fc,hb", CASES)
def test_chain_on_noise_is_the_sums_plus_the_rotator(G, FE, fc, hb):
    """the flowgraph's order of operations in binary64 against what the kernel computes: K0's sums with the library's
    binary32 taps (restated in binary64: no claim about order at this tolerance) times the library's rotator row"""
    x = X.noise32(np.random.default_rng(fc), 24000)
    nout = 750
    with _centre(FE, fc, hb):
        want = FE.chain(x, nout=nout)
    g, D = G.frontend_design(0, 0, centre=fc, half_bw=hb)
    ms = np.arange(nout)
    s = X.convolve64(g.astype(np.complex64), D, x, 0, ms)
    rot = G.frontend_rotator().astype(np.float64)
    r = rot[:, 0] + 1j * rot[:, 1]
    got = s if fc % 375 == 0 else s * r[CX.rot_index(fc, ms)]
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    if fc % 375:                                                  # and without the rotator it is NOT the chain
        assert np.abs(s - want).max() > 0.1 * np.abs(want).max()


def test_compact_mode_at_a_centre_is_the_mixed_low_pass(G):
    g0, D = G.frontend_design(1, 0)
    h = (g0 / np.exp(-1j * np.pi * (D - np.arange(1025)) / 4)).real
    for fc in (497, 2203, 5980, 20):
        g, D2 = G.frontend_design(1, 0, centre=fc, half_bw=10)
        k = np.arange(1025)
        want = h * np.exp(-2j * np.pi * ((fc * (D - k)) % 12000) / 12000.0)
        assert D2 == 512 and np.abs(g - want).max() <= 1e-12 * np.abs(want).max()


# ---- rotator --------------------------------------------------------------------------------------------------------
def test_rotator_table(G):
    rot = G.frontend_rotator()
    assert rot.shape == (375, 2) and rot.dtype == np.float32
    assert rot[0, 0] == 1.0 and rot[0, 1] == 0.0 and np.signbit(rot[0, 1]) and not np.signbit(rot[0, 0])
    a = 2.0 * np.pi * np.arange(375) / 375.0
    for got, want in ((rot[:, 0], np.cos(a)), (rot[:, 1], -np.sin(a))):
        w32 = want.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)).all()
    assert np.abs(np.hypot(rot[:, 0].astype(np.float64), rot[:, 1].astype(np.float64)) - 1.0).max() < 1e-7


def test_rotator_index_against_big_integers():
    rng = np.random.default_rng(5)
    ms = np.concatenate([np.arange(0, 800), 2 ** 31 + np.arange(-3, 400), 2 ** 40 + np.arange(0, 400),
                         rng.integers(0, 2 ** 45, 4000), [2 ** 45]]).astype(np.int64)
    for fc in (20, 170, 374, 375, 376, 497, 1500, 1501, 1875, 2203, 5830, 5980):
        got = CX.rot_index(fc, ms)
        want = np.array([(fc * int(m)) % 375 for m in ms])        # e^{-j 2 pi fc m / 375}: the angle's row, exactly
        assert (got == want).all(), fc
        assert (got == 0).all() == (fc % 375 == 0)


# ---- the mistakes the expectations can see -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_case(G):
    carriers = [2203, 1501, 497]
    taps = [G.frontend_design(0, 0, centre=fc)[0].astype(np.complex64) for fc in carriers]
    rng = np.random.default_rng(77)
    J = X.taps_J(6831)
    m_first = 2 ** 31 + 7
    ms = m_first + np.array([0, 1, 2, 5, 11, 40])
    x = np.stack([X.noise32(rng, 32 * (45 + J)) for _ in range(2)], 1)
    x_origin = 32 * (m_first - J)
    table = G.frontend_rotator()
    return taps, table, carriers, x, x_origin, ms


def test_restatement_is_the_sums_then_the_one_order(G, small_case):
    taps, table, carriers, x, x_origin, ms = small_case
    planes = CX.restate_planes(taps, 0, table, carriers, x, x_origin, ms)
    assert len(planes) == 6 and all(p.shape == (len(ms), 2) and p.any(-1).all() for p in planes)
    for c in range(2):
        for k, fc in enumerate(carriers):
            s = X.restate(taps[k], 0, np.ascontiguousarray(x[:, c]), x_origin, ms)
            r = table[CX.rot_index(fc, ms)]
            y = planes[c * 3 + k]
            assert y[:, 0].tobytes() == X.fma32(s[:, 0], r[:, 0], -(s[:, 1] * r[:, 1])).tobytes()
            assert y[:, 1].tobytes() == X.fma32(s[:, 0], r[:, 1], s[:, 1] * r[:, 0]).tobytes()
            z = (s[:, 0].astype(np.float64) + 1j * s[:, 1]) * (r[:, 0].astype(np.float64) + 1j * r[:, 1])
            assert np.abs((y[:, 0] + 1j * y[:, 1].astype(np.float64)) - z).max() <= 3e-7 * np.abs(z).max()
    # an identity carrier leaves the sums' bytes, NaN included
    s = np.array([[np.nan, 1.0], [np.inf, -0.0]], np.float32)
    assert CX.rotate(s, 1875, [3, 4], table).tobytes() == s.tobytes()
    assert CX.rotate(s, 1501, [0, 375], table).tobytes() != s.tobytes()          # (1, -0) is NOT the identity on bytes


@pytest.mark.parametrize("name", CX.MUTATIONS)
def test_every_mutation_changes_the_expectations(G, small_case, name):
    taps, table, carriers, x, x_origin, ms = small_case
    good = CX.restate_planes(taps, 0, table, carriers, x, x_origin, ms)
    bad = CX.restate_planes(taps, 0, table, carriers, x, x_origin, ms, mutation=name)
    differ = [q for q in range(len(good)) if good[q].tobytes() != bad[q].tobytes()]
    assert len(differ) >= 4, (name, differ)


# ---- argument errors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc,hb", [(19, 10), (5981, 10), (29, 10), (5971, 10), (1500, 0), (1500, 151), (169, 150), (5831, 150)])
def test_design_refuses_what_is_out_of_range(G, fc, hb):
    with pytest.raises(G.UwsprError) as e:
        G.frontend_design(0, 0, centre=fc, half_bw=hb)
    assert e.value.status == -6                                    # UWSPR_ERR_ARG


def test_design_accepts_the_ends_of_the_range(G):
    for fc, hb in ((30, 10), (5970, 10), (21, 1), (5979, 1), (170, 150), (5830, 150)):
        assert len(G.frontend_design(0, 0, centre=fc, half_bw=hb)[0]) == 6831
    for fc in (20, 5980):                                          # the compact mode has no hb
        assert len(G.frontend_design(1, 0, centre=fc, half_bw=0)[0]) == 1025
    for fc in (19, 5981):
        with pytest.raises(G.UwsprError):
            G.frontend_design(1, 0, centre=fc)
    with pytest.raises(G.UwsprError):
        G.frontend_design(2, 0, centre=1500)


def test_entry_points_are_declared_and_bound(G):
    for name in ("uwspr_frontend_design_at", "uwspr_frontend_rotator", "uwspr_pipe_set_carriers"):
        assert name in G.native.ABI_SYMBOLS and hasattr(G.native.lib(), name)


# ---- the decode test's inputs decode on the CPU ------------------------------------------------------------------------
def closed_loop_f64(n):
    """examples/WaveFilePlusNoiseDecode.grc's mix (tx x 0.1 + whales, both repeating)"""
    rec = np.load(os.path.join(GOLDEN, "closed_loop_int16.npz"))
    tx = np.resize(rec["tx"].astype(np.float64) / 32768.0, n)
    wh = np.resize(rec["whales"].astype(np.float64) / 32768.0, n)
    return float(rec["tx_gain"]) * tx + float(rec["whales_gain"]) * wh


def _decode_set(G, oracle, frame):
    out = set()
    for c in oracle.FDR().transform(frame)[:2]:
        d = oracle.demod_candidate(c, 1500, frame)
        rec = np.zeros(1, G.native.DEMOD_DTYPE)[0]
        for k in ("f1", "drift1", "sync1", "shift1", "worth_a_try", "jig_sync", "jig_rms", "jig_shift", "symbols"):
            rec[k] = d[k]
        dec = G.decode_candidate(rec)
        if dec is not None:
            out.add(G.unpack_message(dec[0])[1])
    return out


@pytest.mark.parametrize("fc", [497, 2203])
def test_shifted_recordings_decode_on_the_cpu_chain(G, oracle, FE, fc):
    """the closed-loop mix masked to 1500 +- 150 Hz and moved to fc, through frontend_grc.chain at that centre, the
    oracle's FDR + schedule and Fano: the control's text"""
    x = CX.shift_band(closed_loop_f64(120 * 12000), 1350.0, 1650.0, fc - 1500)
    with _centre(FE, fc, 10):
        y = FE.chain(x.astype(np.float32))
    frame = np.stack([y.real, y.imag], axis=1).astype(np.float32)
    assert _decode_set(G, oracle, frame) == {"VE3EMB FN25 30"}
