"""K7 at another carrier (uwspr_tx_design_at, the options "tx_cutoff" / "tx_form", uwspr_tx_render_at,
uwspr_tx_baseband_at): everything that needs no GPU.  The design against the two designers of oracle/frontend_grc.py, the
pass band against the 1500 Hz one, the ranges, the ABI, and the mistakes tests/transmit_carrier_exact.py's expectation
must see.  tests/test_gpu_transmit_carrier.py holds the device to that expectation."""
import os
import re

import numpy as np
import pytest

import transmit_carrier_exact as TC
import transmit_exact as X

# (carrier, cut-off): both ends of the carrier range at both ends of the cut-off range, and the carriers of the GPU tests
DESIGNS = [(1500, 2500), (170, 2500), (2250, 2500), (497, 2500), (1501, 2500), (1875, 2500), (2203, 2500),
           (170, 500), (250, 500), (170, 5900), (5650, 5900), (3000, 4000)]


@pytest.fixture(scope="module")
def table(G):
    return G.frontend_rotator()


def test_default_design_is_the_tap_door_byte_for_byte(G):
    g0, image0 = G.tx_taps()
    g, image = G.tx_design(1500, 2500)
    assert g.tobytes() == g0.tobytes() and image.tobytes() == image0.tobytes()
    g, image = G.tx_design()
    assert g.tobytes() == g0.tobytes() and image.tobytes() == image0.tobytes()


@pytest.mark.parametrize("fc,cutoff", DESIGNS)
def test_design_is_the_two_designers_composite_rotated(G, fc, cutoff):
    """3179 taps whatever (carrier, cut-off) is, and the composite of the two designers within the 1e-7 of
    tests/test_transmit_exact.py; the image is the phase split of the taps"""
    import frontend_grc as F
    g, image = G.tx_design(fc, cutoff)
    assert g.shape == (X.NT,) and g.dtype == np.complex128 and image.shape == (X.DEC, X.T, 2) and image.dtype == np.float32
    h1 = F.low_pass(1, 12000, 200, 10).astype(np.float64)
    h2 = F.low_pass(1, 12000, cutoff, 100)
    assert len(h1) == 2891 and len(h2) == 289
    h2r = F.xlating_taps(h2, float(fc)).astype(np.complex128)
    q = np.arange(X.NT, dtype=np.int64)
    want = np.convolve(h1, h2r) * np.exp(-2j * np.pi * ((fc * q) % 12000) / 12000.0)
    assert len(want) == X.NT
    err = np.abs(g - want).max() / np.abs(want).max()
    print("(%d, %d): design error %.3g of the largest tap" % (fc, cutoff, err))
    assert err <= 1e-7
    img = np.zeros((X.DEC, X.T, 2), np.float32)
    for p in range(X.DEC):
        for i in range(X.T):
            if p + X.DEC * i < X.NT:
                img[p, i] = (np.float32(g[p + X.DEC * i].real), np.float32(-g[p + X.DEC * i].imag))
    assert image.tobytes() == img.tobytes()


@pytest.mark.parametrize("fc,cutoff", [(170, 2500), (497, 2500), (1501, 2500), (1875, 2500), (2203, 2500), (2250, 2500),
                                       (5650, 5900)])
def test_pass_band_is_the_1500_hz_one_within_a_percent(G, fc, cutoff):
    """audio = Re sum g x: a baseband tone e^{-j 2 pi f j / 375} (file orientation) leaves at fc + f Hz with gain
    G(-(fc + f)).  |f| <= 150: within 1 % of the 1500 Hz design's at 1500 + f (two Hamming designs of <= 0.3 % each)."""
    f = np.linspace(-150.0, 150.0, 31)
    ref = np.abs(TC.response(G.tx_design(1500, 2500)[0], -(1500 + f)))
    got = np.abs(TC.response(G.tx_design(fc, cutoff)[0], -(fc + f)))
    dev = np.abs(got / ref - 1.0).max()
    print("(%d, %d): pass band within %.3g of the 1500 Hz design's (unity within %.3g)" % (fc, cutoff, dev, np.abs(got - 1).max()))
    assert dev <= 0.01
    assert np.abs(ref - 1.0).max() <= 0.01


def test_design_range_checks(G):
    for fc, cutoff in ((169, 2500), (2251, 2500), (1500, 499), (1500, 5901), (251, 500), (5651, 5900), (-1500, 2500),
                       (0, 2500), (6000, 5900)):
        with pytest.raises(ValueError):
            G.tx_design(fc, cutoff)
    L = G.native.lib()
    assert L.uwspr_tx_design_at(169, 2500, None, None) == -6
    assert L.uwspr_tx_design_at(170, 2500, None, None) == X.NT        # (either pointer may be null)


def test_abi_names_and_options(G):
    N = G.native
    L = N.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "uwspr_hip.h")).read()
    entry6 = hdr[hdr.index("6: audio streams"):hdr.index("*/", hdr.index("6: audio streams"))]
    assert re.search(r"#define UWSPR_ABI_VERSION 6\b", hdr)
    for name in ("uwspr_tx_render_at", "uwspr_tx_baseband_at", "uwspr_tx_design_at"):
        assert name in entry6 and name in N.ABI_SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert "tx_cutoff" in entry6 and "tx_form" in entry6
    assert "Not built: transmit" not in hdr
    api = open(os.path.join(root, "gr-uwspr_amd", "csrc", "uwspr_api.hip")).read()
    assert re.search(r'\{"tx_cutoff", UWSPR_TX_CUTOFF_DEFAULT, 500, 5900\}', api) and re.search(r'\{"tx_form", 0, 0, 1\}', api)
    assert re.search(r"#define UWSPR_TX_CUTOFF_DEFAULT 2500\b", hdr)


def test_carrier_array_of_a_signal_list(G):
    sigs = [{"text": "K1ABC FN42 37"}, {"text": "VE3EMB FN25 30", "carrier": 2203}, {"text": "PJ4/K1ABC 37", "carrier": 497}]
    car = G.tx_carriers(sigs)
    assert car.dtype == np.int32 and car.tolist() == [1500, 2203, 497]
    assert G.tx_carriers(sigs[:1]) is None and G.tx_carriers([]) is None
    with pytest.raises(ValueError):
        G.tx_carriers([{"text": "K1ABC FN42 37", "carrier": 1500.5}])
    counts = G.tx_carrier_launch_counts()                            # (the door is there; what it counts needs a GPU)
    assert len(counts) == 2 and all(v >= 0 for v in counts)


# ---- the mutations ---------------------------------------------------------------------------------------------------------
# One channel, three carriers given in the order 2203, 497, 1501 (not ascending), the 2203 Hz group with two signals; the
# window starts at audio 0 with the signals already running (start < 0), so that the staged basebands reach back to
# j = -103: the rotator meets negative j.
CASE = [{"text": "K1ABC FN42 37", "start": -20000, "f0": -150.0, "drift": -20.0, "gain": 0.3, "phase0": 1e3, "carrier": 2203},
        {"text": "VE3EMB FN25 30", "start": -19683, "f0": 3.1, "gain": 1.0, "phase0": -1e3, "carrier": 497},
        {"text": "PJ4/K1ABC 37", "start": -17089, "f0": 120.0, "drift": 4.0, "gain": 1.7, "phase0": 0.4, "carrier": 2203},
        {"text": "G4XYZ/7 10", "start": -15000, "f0": -40.0, "gain": 0.8, "phase0": 2.0, "carrier": 1501}]
CASE_T0, CASE_NF = 0, 6000


@pytest.fixture(scope="module")
def case(G, table):
    """the groups of CASE from the float64 model rounded to binary32 (the device's baseband differs in the last place of
    some samples: the same signals), in the order the carriers are given in"""
    j0, nbb = X.window(CASE_T0, CASE_NF)
    assert j0 < 0
    groups, singles = {}, {}
    for fc in (2203, 497, 1501):
        mine = [s for s in CASE if s["carrier"] == fc]
        y = X.baseband_model(mine, G.wspr_symbols, j0, nbb)
        groups[fc] = (G.tx_design(fc, 2500)[1], (y.real.astype(np.float32), (-y.imag).astype(np.float32)))
        singles[fc] = []
        for s in mine:
            y = X.baseband_model([s], G.wspr_symbols, j0, nbb)
            singles[fc].append((y.real.astype(np.float32), (-y.imag).astype(np.float32)))
    n = np.arange(CASE_T0, CASE_T0 + CASE_NF, dtype=np.int64)
    return groups, singles, j0, n, TC.expect(groups, n, j0, table)


def _changed(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.mark.parametrize("name", TC.MUTATIONS)
def test_byte_expectations_see_the_mutation(case, table, name):
    groups, _, j0, n, want = case
    assert list(groups) != sorted(groups) and (want != 0).all()
    got = TC.expect(groups, n, j0, table, mutation=name)
    changed = _changed(got, want)
    print("%s: %d of %d outputs change" % (name, changed, len(n)))
    assert changed >= 1
    if name == "c_remainder":
        # only outputs that read a sample with j < 0: taps reach back 103 samples, so audio below 32 * 103 + 32
        assert (n[got.view(np.uint32) != want.view(np.uint32)] < 32 * X.T).all()


def test_rotating_each_signal_is_another_sum_than_rotating_the_group(case, table):
    """the rotator is applied to the group's SUM (one product per sample and group); rotating every signal after its gain
    and adding the products rounds elsewhere, and the bytes differ -- so the tests tell the two apart"""
    groups, singles, j0, n, _ = case
    image, x = groups[2203]
    group = TC.expect({2203: (image, x)}, n, j0, table)
    each = TC.per_signal_rotation(image, singles[2203], 2203, n, j0, table)
    changed = _changed(group, each)
    print("per-signal rotation: %d of %d outputs differ from the group-sum rotation" % (changed, len(n)))
    assert changed >= 1
    # with one signal in the group the two are the same thing
    image, x = groups[497]
    assert _changed(TC.expect({497: (image, x)}, n, j0, table), TC.per_signal_rotation(image, singles[497], 497, n, j0, table)) == 0


def test_a_multiple_of_375_takes_no_rotator(case, table):
    groups, _, j0, n, _ = case
    x = groups[497][1]
    image = groups[497][0]
    j = j0 + np.arange(len(x[0]), dtype=np.int64)
    for fc in (375, 1500, 1875):
        r = TC.rotated(x, fc, j, table)
        assert r[0].tobytes() == x[0].tobytes() and r[1].tobytes() == x[1].tobytes()
    assert TC.expect({1875: (image, x)}, n, j0, table).tobytes() == X.chain(image, x, n, x0=j0).tobytes()
    r = TC.rotated(x, 1501, j, table)
    assert (r[0] != x[0]).any()


def test_two_stage_restatement_is_the_design(G):
    """the float64 two-stage chain at a carrier against the one-FIR form with the binary64 taps: the same linear map"""
    rng = np.random.default_rng(5)
    nbb = 400
    x = rng.normal(size=nbb) + 1j * rng.normal(size=nbb)
    for fc, cutoff in ((497, 2500), (2203, 2500), (5650, 5900)):
        g, _ = G.tx_design(fc, cutoff)
        nout = 32 * nbb
        ref = TC.two_stage(x, nout, fc, cutoff)
        j = np.arange(nbb, dtype=np.int64)
        xr = x * np.exp(-2j * np.pi * ((fc % 375) * (j % 375) % 375) / 375.0)
        u = np.zeros(nout, np.complex128)
        u[::32] = xr
        one = np.convolve(u, g)[:nout].real
        err = np.abs(one - ref).max()
        print("%d Hz: one FIR + rotator against the two-stage chain: %.3g" % (fc, err))
        assert err <= 1e-7 * np.abs(ref).max() + 1e-9
