"""Block demodulation's definition (include/uwspr_hip.h, K10) without a GPU: the binary64 restatement the GPU tests compare
bytes with (tests/blockdemod_exact.py) decodes what was sent; binary32 alone costs the bytes nothing on the inputs the GPU
tests use, so their tolerance belongs wholly to the kernel; sixteen misreadings of the text each FAIL the GPU tests'
criterion (every byte within 1, at most 1 % of a call's bytes different) on a named item of edge_items(); the NaN rule."""
import numpy as np
import pytest

import blockdemod_exact as BX

NSYM = BX.NSYM


def _restate(G, name, **kw):
    it = BX.edge_items()[BX.EDGE_NAMES.index(name)]
    return BX.block_restate(BX.edge_frames(G)[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3, **kw)


def _want(G, name):
    return BX.edge_want(G)[BX.EDGE_NAMES.index(name)]


def test_restatement_needs_no_gpu(G):
    """the restatement alone, on the noise-free frame: every vector carries the transmitted bits and decodes"""
    sym = G.wspr_symbols(BX.TEXT)
    for nb in range(3):
        v = _want(G, "noise-free")[nb]
        assert np.array_equal(v >= 128, (sym >> 1).astype(bool)), nb
        rc, msg = G.fano_decode(G.deinterleave(v))[:2]
        assert rc == 0 and G.unpack_message(msg[:7].astype(np.int8)) == (0, BX.TEXT)


def test_the_items_are_what_the_tests_take_them_for(G):
    items = BX.edge_items()
    assert len(items) == len(BX.EDGE_NAMES) == len(set(BX.EDGE_NAMES)) == 31
    assert [it["frame"] for it in items] == sorted(it["frame"] for it in items)          # as the call wants them
    assert sorted(it["shift"] % 16 for it in items if it["name"].startswith("alignment")) == list(range(16))
    fr = BX.edge_frames(G)
    assert fr.shape == (10, BX.FL_LONG, 2) and fr.dtype == np.float32 and np.isfinite(fr).all()
    assert np.array_equal(BX.edge_frames(G, BX.NP), fr[:, :BX.NP])
    for n in (0, BX.NP - 1, BX.NP):        # 30 .. 50 sigma of the spike frame's noise, I and Q both non-zero
        assert (np.abs(fr[4][n]) >= 30).all() and (np.abs(fr[4][n]) <= 50).all()
    assert 0.9 < fr[4][1:BX.NP - 1].std() < 1.1 and np.abs(fr[4][1:BX.NP - 1]).max() < 6
    assert (fr[2][BX.NP:] != 0).all() and (fr[4][BX.NP:] != 0).all()                     # something to ignore from 45 000 on
    run_off = [it["name"] for it in items if BX.reads_from_45000_on(it)]
    assert run_off == ["runs off the end", "spike, last sample 45000", "alignment 14", "alignment 15"]


@pytest.mark.parametrize("name", BX.EDGE_NAMES)
def test_binary32_alone_costs_the_bytes_nothing(G, name):
    """The cap is a condition on the inputs: the definition with every product and sum rounded to binary32 stays within 1
    per byte of the binary64 restatement and differs in at most 0.25 % of an item's bytes (here: in none, on all 31), so
    the GPU criterion's 1 % is room for the kernel's own arithmetic -- fused multiply-adds, the two-step phasor -- alone."""
    it = BX.edge_items()[BX.EDGE_NAMES.index(name)]
    got = BX.emulate32(BX.edge_frames(G)[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3)
    ndiff, size, largest = BX.close_figures(got, _want(G, name))
    print("emulate32, %s: %d of %d bytes differ, largest difference %d" % (name, ndiff, size, largest))
    assert largest <= 1 and ndiff <= 0.0025 * size, name


def test_binary32_is_not_binary64_in_disguise(G):
    """emulate32's sums do carry binary32's error: its z differ from the binary64 ones by 1e-8 .. 1e-5 relative"""
    it = BX.edge_items()[0]
    fr = BX.edge_frames(G)[it["frame"]]
    xs = BX._samples(fr, it["shift"], BX.NP, None)
    k = np.arange(256)
    ph = -2.0 * np.pi * (BX._freqs(it["f"], it["drift"], None, np.arange(NSYM))[:, None] - 1.5 * BX.DF) * k[None, :] / 375.0
    exact = (xs.real * np.cos(ph) - xs.imag * np.sin(ph)).sum(axis=1)
    c, s = np.cos(ph).astype(np.float32), np.sin(ph).astype(np.float32)
    single = np.add.accumulate(xs.real.astype(np.float32) * c - xs.imag.astype(np.float32) * s, axis=1, dtype=np.float32)[:, -1]
    assert single.dtype == np.float32
    rel = np.abs(single - exact).max() / np.abs(exact).max()
    assert 1e-8 < rel < 1e-5, rel


# misreading: (items on which it must FAIL the criterion, items on which it passes -- why the failing ones exist)
MISREADINGS = {
    "n_ge_0": (["spike, shift 0", "spike, shift -255"], ["spike, shift 1", "nominal"]),
    "n_le_np": (["spike, last sample 45000"], ["spike, last sample 44999", "spike, last sample 44998", "nominal"]),
    "np_is_fl": (["spike, last sample 45000", "runs off the end"], ["spike, last sample 44999", "nominal"]),
    "slope_162": (["drift +2", "drift -2", "drift -40"], ["nominal"]),
    "drift_not_halved": (["drift +2", "drift -2", "drift -40"], ["nominal"]),
    "phasor_from_1": (["nominal", "alignment 0"], []),
    "phasor_not_restarted": (["nominal", "noise-free"], []),
    "theta_no_pi": (["nominal", "noise-free"], []),
    "theta_next": (["drift +2", "drift -2", "drift -40"], ["nominal", "noise-free", "alignment 0"]),
    "psi_own": (["drift +2", "drift -2", "drift -40"], ["nominal", "noise-free", "alignment 0"]),
    "psi_plus": (["nominal", "noise-free"], []),
    "tone_2pr3_d": (["nominal", "noise-free"], []),
    "spacing_512": (["nominal", "noise-free"], []),
    "round": (["nominal", "loud symbols"], []),
    "clip_127": (["loud symbols"], ["nominal", "drift +2"]),
    "mean_161": (["nominal", "spike, last sample 44999"], ["noise-free"]),
}


def test_every_misreading_is_listed():
    assert sorted(MISREADINGS) == sorted(BX.MUTATIONS) and len(BX.MUTATIONS) == 16


@pytest.mark.parametrize("mutate", BX.MUTATIONS)
def test_misreadings_fail_the_gpu_criterion(G, mutate):
    """n >= 0; n <= np; np = fl; drift slope (i - 81) / 162; drift not halved; phasor from k = 1; phasor not restarted per
    symbol; theta without pi; theta of the next symbol; psi including its own symbol; e^{+j psi}; tone 2 pr3 + d; tone
    spacing 375 / 512; rounding instead of truncation; clipping at +-127; means over 161 values.  Each, taken for the
    definition, misses "every byte within 1, at most 1 % different" against the unmutated restatement on the items named
    -- the sample bounds on the spike items, the theta / psi indexing on the drifting ones only."""
    fails, passes = MISREADINGS[mutate]
    for name in fails:
        got, want = _restate(G, name, mutate=mutate), _want(G, name)
        ndiff, size, largest = BX.close_figures(got, want)
        print("%s on %s: %d of %d bytes differ, largest difference %d" % (mutate, name, ndiff, size, largest))
        assert not BX.meets_criterion(got, want), \
            "%s is invisible on '%s': %d of %d bytes differ, largest difference %d (it passes on %s by design: the items %s are " \
            "there to show it)" % (mutate, name, ndiff, size, largest, passes or "no listed item", fails)
    for name in passes:
        assert BX.meets_criterion(_restate(G, name, mutate=mutate), _want(G, name)), \
            "%s no longer passes on '%s': the items %s are there because it does" % (mutate, name, fails)


def test_an_unmutated_restatement_meets_the_criterion(G):
    for name in ("nominal", "drift -40", "spike, shift 0"):
        assert np.array_equal(_restate(G, name), _want(G, name))
    assert BX.meets_criterion(_want(G, "nominal"), _want(G, "nominal"))
    off = np.array(_want(G, "nominal"))
    off[0, :5] ^= 1                                        # 5 of 486 bytes: 1.03 %
    assert not BX.meets_criterion(off, _want(G, "nominal"))
    off = np.array(_want(G, "nominal"))
    off[2, 7] = off[2, 7] + 2 if off[2, 7] < 128 else off[2, 7] - 2
    assert not BX.meets_criterion(off, _want(G, "nominal"))


def test_the_sample_bound_follows_np_points_not_the_frame_length(G):
    """items that read no sample from 45 000 on do not care what np_points is; the others do, or the GPU test with fl = 48 000
    could not tell np = 45 000 from np = fl"""
    w45, w48 = BX.edge_want(G, BX.NP), BX.edge_want(G, BX.FL_LONG)
    for q, it in enumerate(BX.edge_items()):
        if BX.reads_from_45000_on(it):
            assert not BX.meets_criterion(w48[q], w45[q]), it["name"]
        else:
            assert np.array_equal(w48[q], w45[q]), it["name"]
    # cut to 45 000 samples, "behind the buffer" is the same zero
    short = BX.edge_frames(G, BX.NP)
    for q, it in enumerate(BX.edge_items()):
        if BX.reads_from_45000_on(it):
            assert np.array_equal(BX.block_restate(short[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3), w45[q]), it["name"]


def test_loud_symbols_reach_both_ends_of_the_byte(G):
    want = _want(G, "loud symbols")
    bit = G.wspr_symbols(BX.TEXT) >> 1
    loud = BX.loud_symbols(G, BX.TEXT)
    assert sorted(int(bit[i]) for i in loud) == [0, 0, 0, 1, 1]
    for nb in range(3):
        assert (want[nb] == 0).any() and (want[nb] == 255).any(), nb
        assert np.array_equal(want[nb] >= 128, bit.astype(bool)), nb
        for i in loud:
            assert want[nb][i] == (255 if bit[i] else 0), (nb, i)


@pytest.mark.parametrize("value", list(BX.SPECIAL_VALUES))
def test_a_nan_or_an_infinity_gives_128_for_whoever_reads_it(G, value):
    """A NaN, a +inf or a -inf in one sample of a noise frame: every item whose window includes the sample gets 128 in
    every byte of all three block lengths (a block that holds a NaN P has NaN soft values, whichever P it is); items of
    the same frame whose windows exclude it keep their bytes."""
    clean = BX.edge_frames(G, BX.NP)[5]
    for place in BX.SPECIAL_PLACES:
        fr = BX.special_frame(clean, place, value)
        assert (~np.isfinite(fr)).sum() == 1
        hit, miss = BX.special_items(place, 0)
        for it in hit:
            got = BX.block_restate(fr, it["shift"], it["f"], it["drift"], G.synth.PR3)
            assert (got == 128).all(), (place, it)
            assert not (BX.block_restate(clean, it["shift"], it["f"], it["drift"], G.synth.PR3) == 128).all()
        for it in miss:
            got = BX.block_restate(fr, it["shift"], it["f"], it["drift"], G.synth.PR3)
            assert np.array_equal(got, BX.block_restate(clean, it["shift"], it["f"], it["drift"], G.synth.PR3)), (place, it)
