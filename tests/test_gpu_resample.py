"""K11, the rational resampler ahead of K0 (gr-uwspr_amd/csrc/k11_resample.hip), held to its numpy restatement
(tests/resample_exact.py) byte for byte: through the batch call (impulse trains that pin every tap, dense noise, both
sample formats, 1 .. 64 channels, ragged ends), through the one-launch door (far origins, buffers that start late or
early, end soon or hold one sample, single outputs and workgroup seams, both instantiations) and with a NaN that must
reach the outputs whose window holds it and nothing else."""
import numpy as np
import pytest

import resample_exact as X


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


# ---- the batch call --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rate", X.GPU_RATES)
def test_impulse_trains(ctx, rate):
    x, exp, hit = X.impulse_case(rate)
    assert (hit >= 1).all()                                   # every (p, t) pair is met
    got = ctx.resample(x, rate, nout=len(exp))
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert got.tobytes() == exp.tobytes()
    # as channel 1 of three (the others silent): the same bytes, and +0 beside them
    x3 = np.zeros((len(x), 3), np.float32)
    x3[:, 1] = x
    got = ctx.resample(x3, rate, nout=len(exp))
    assert got[:, 1].tobytes() == exp.tobytes()
    assert got[:, 0].tobytes() == np.zeros(len(exp), np.float32).tobytes() == got[:, 2].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [1, 2, 3, 64])
@pytest.mark.parametrize("rate", X.GPU_RATES)
def test_dense_noise_formats_and_channels(ctx, rate, nch):
    x, exp = X.dense_case(rate, nch)
    nout = exp.shape[0]
    hp, L, M, T, N, D = X.plan(rate)
    assert nout % X.WG_OUT != 0                               # a ragged last output block
    assert ((nout - 1) * M + D) // L - (T - 1) >= x.shape[0]  # the last output's window lies behind the record: +0 ...
    assert ((nout - 4) * M + D) // L - (T - 1) < x.shape[0] <= ((nout - 4) * M + D) // L   # ... the record ends inside this one's
    xi = x if nch > 1 else x[:, 0]
    got16 = ctx.resample(xi, rate, nout=nout)
    got32 = ctx.resample(X.s16_to_f32(xi), rate, nout=nout)
    assert got16.tobytes() == got32.tobytes()                 # int16 counts as s / 32768, exactly
    assert got16.reshape(nout, nch).tobytes() == exp.tobytes()
    assert exp[-1].tobytes() == np.zeros(nch, np.float32).tobytes()


# ---- the door ----------------------------------------------------------------------------------------------------------
def _door(ctx, x, rate, in0, j_first, nout, nch=1):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    out = torch.full((nout + 64, nch), 7.0, dtype=torch.float32, device="cuda:0")     # (64 rows of guard behind)
    ctx.debug_resample_launch(xd, rate, in0, out, j_first, nch=nch, nout=nout)
    got = out.cpu().numpy()
    assert (got[nout:] == 7.0).all(), "a store behind the last output"
    return got[:nout]


def _first_input(rate, j):
    hp, L, M, T, N, D = X.plan(rate)
    return (j * M + D) // L - (T - 1)


DOOR = [  # (rate, j_first, in0 - (first input the first output reads), nin, nout)
    (44100, (1 << 40) - 77, 0, 4000, 700),          # far origins, L = 40: the buffer starts where the first window does
    (176400, (1 << 40) + 3, -5, 9000, 300),         # in0 near 2^44, L = 10; starts early
    (44100, 123456789, 37, 3000, 257),              # starts late (the first windows begin before it); one more than a workgroup
    (44100, 5, -100000, 100900, 600),               # starts long before: the early frames are never read
    (8000, 1 << 33, 3, 200, 900),                   # ends soon: most windows lie behind it (L = 3 > M = 2)
    (11025, (1 << 39) + 11, 9, 1, 300),             # holds one sample
    (44100, (1 << 40) - 1, 20, 500, 1),             # nout = 1
    (48000, 999, 0, 1100, 257),                     # L = 1
]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "s16"])
@pytest.mark.parametrize("case", range(len(DOOR)))
def test_door_origins_and_edges(G, ctx, case, fmt):
    rate, j_first, d0, nin, nout = DOOR[case]
    in0 = _first_input(rate, j_first) + d0
    if case < 2:
        assert in0 > 1 << 41 and j_first >= (1 << 40) - 77
    xs = X.noise16(np.random.default_rng(1300 + case), nin + 2)[:nin]
    xf = X.s16_to_f32(xs)
    exp = X.restate(rate, xf, in0, j_first + np.arange(nout))
    assert (exp != 0).any()
    before = G.resample_launch_counts()
    got = _door(ctx, xf if fmt == "f32" else xs, rate, in0, j_first, nout)
    after = G.resample_launch_counts()
    # the instantiation of the input's format ran, once; the other did not
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if fmt == "f32" else (0, 1))
    assert got[:, 0].tobytes() == exp.tobytes()


@pytest.mark.gpu
def test_door_far_origin_is_the_near_one(ctx):
    """the same samples under the same phases at the origin and 40 * 2^34 outputs later (L = 40 divides the shift, so p
    repeats): the bytes do not depend on where the stream stands"""
    rate = 44100
    hp, L, M, T, N, D = X.plan(rate)
    x = X.noise32(np.random.default_rng(1400), 5000)
    dj = 40 << 34
    near = _door(ctx, x, rate, 10, 50, 900)
    far = _door(ctx, x, rate, 10 + dj // L * M, 50 + dj, 900)
    assert near.tobytes() == far.tobytes()
    assert near[:, 0].tobytes() == X.restate(rate, x, 10, 50 + np.arange(900)).tobytes()


@pytest.mark.gpu
def test_door_channels(ctx):
    """three and 64 interleaved channels through one launch: every channel is its own one-channel launch"""
    rate, j_first, nin, nout = 44100, 70000, 3000, 513
    in0 = _first_input(rate, j_first) + 7
    for nch in (3, 64):
        x = X.noise16(np.random.default_rng(1500 + nch), (nin, nch))
        got = _door(ctx, x, rate, in0, j_first, nout, nch=nch)
        for c in (range(nch) if nch == 3 else (0, 1, 31, 62, 63)):
            exp = X.restate(rate, X.s16_to_f32(x[:, c]), in0, j_first + np.arange(nout))
            assert got[:, c].tobytes() == exp.tobytes(), (nch, c)
        one = _door(ctx, np.ascontiguousarray(x[:, nch - 2]), rate, in0, j_first, nout)
        assert one[:, 0].tobytes() == np.ascontiguousarray(got[:, nch - 2]).tobytes()


# ---- NaN -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rate", [44100, 48000, 8000])
def test_nan_reaches_its_windows_only(ctx, rate):
    hp, L, M, T, N, D = X.plan(rate)
    nin, nch, n_bad = 6000, 3, 3111
    x = np.stack([X.noise32(np.random.default_rng(1600 + c), nin) for c in range(nch)], axis=1)
    nout = ((nin + T) * L - D) // M + 2
    clean = ctx.resample(x, rate, nout=nout)
    bad = x.copy()
    bad[n_bad, 1] = np.nan
    got = ctx.resample(bad, rate, nout=nout)
    i0, _ = X.indices(np.arange(nout), L, M, D)
    holds = (i0 - (T - 1) <= n_bad) & (n_bad <= i0)
    assert holds.sum() >= T * L // M - 1 and not holds.all()
    assert np.isnan(got[holds, 1]).all()                      # (also where the tap is the zero padding: 0 x NaN)
    assert got[~holds, 1].tobytes() == clean[~holds, 1].tobytes()
    assert got[:, 0].tobytes() == clean[:, 0].tobytes() and got[:, 2].tobytes() == clean[:, 2].tobytes()
    for c in range(nch):
        assert clean[:, c].tobytes() == X.restate(rate, np.ascontiguousarray(x[:, c]), 0, np.arange(nout)).tobytes()
