"""K12, the noise blanker (uwspr_blank_batch; include/uwspr_hip.h, "impulsive noise"), on the GPU against the numpy
restatement of the header's text (tests/blank_exact.py, held to a brute-force route and to four mutations by
tests/test_blank.py without a GPU).  Everything is integers but the two multiplies of a threshold, so the checks are
byte for byte: out, med and nzero, at the smallest shapes that can still go wrong -- records that end on, before and
behind a block edge, guards 0 .. 64, both sample formats, 1 .. 64 channels, host and device memory, and the one-launch
door with 64-bit origins and buffers that start late or hold one sample."""
import numpy as np
import pytest

import blank_exact as BX

N = BX.N
ERR_ARG = -6


def _bytes_equal(got, exp):
    for g, e, what in zip(got, exp, ("out", "med", "nzero")):
        g = np.asarray(g)
        assert g.dtype == e.dtype and g.shape == e.shape, what
        bad = np.nonzero(g.view(np.uint32).reshape(-1) != e.view(np.uint32).reshape(-1))[0]
        assert len(bad) == 0, "%s: %d of %d differ, first at flat index %d" % (what, len(bad), g.size, bad[0])


def _signal(n, C, G, seed, s16=False):
    """[n, C]: blocks at the levels 1, 0.01, 0.01, (a block of 2048-way ties), 0.01, ... with spikes at 4095, 4096,
    4096 -+ G and n - 1, and at the edge 2 N between blocks 1 and 2 -- both quiet, but block 1 is judged by loud block 0
    and block 2 by quiet block 1 -- a 0.3 spike on 2 N - 1 (even channels: NOT flagged, though block 2's workgroup reads
    it in its halo) or on 2 N (odd channels: flagged, though block 1's workgroup reads it in its halo)"""
    r = np.random.Generator(np.random.Philox(seed))
    x = r.standard_normal((n, C))
    blk = np.arange(n) // N
    scale = np.where(blk % 5 == 0, 1.0, 0.01)
    x *= scale[:, None] * (1.0 + 0.25 * np.arange(C))[None, :]
    tie = blk % 5 == 3
    x[tie] = np.where((np.arange(n)[tie] % 2 == 0)[:, None], 0.02, -0.005) * np.sign(x[tie])
    for i in (N - 1, N, N - G, N + G, n - 1):
        if 0 <= i < n:
            x[i] = 50.0 * (1 if i % 2 else -1)
    for c in range(C):
        i = 2 * N - 1 + (c % 2)
        if i < n:
            x[i, c] = 0.3
    if s16:
        return np.clip(np.rint(x * 300.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G_", [0, 1, 2, 64])
def test_record_lengths_and_guards(ctx, G_):
    for nin in (1, G_, N - 1, N, N + 1, 2 * N + G_, 5 * N - 1):
        if nin < 1:
            continue
        for s16 in (False, True):
            x = _signal(nin, 1, G_, 100 + nin % 97, s16)[:, 0].copy()
            exp = BX.blank(x, 24, G_)
            _bytes_equal(ctx.blank(x, 24, G_), exp)
            if nin == 5 * N - 1:   # the input does what it is for
                y, med, nz = exp
                xf = BX.as_float(x)
                assert nz[0] == min(G_, N) and nz[1] >= 1 and y[N] == 0 and y[-1] == 0 and med[4] == 0 and med[3] != 0
                assert y[2 * N - 1] == xf[2 * N - 1] != 0 and nz[2] < N // 4     # the 0.3 spike of block 1 stays, block 2 is not blanked


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 64])
@pytest.mark.parametrize("s16", [False, True])
def test_channels_formats_and_thresholds(ctx, C, s16):
    nin = 5 * N - 1
    for G_, blank in ((2, 24), (64, 24), (2, 4), (1, 1024)):
        x = _signal(nin, C, G_, 200 + C, s16)
        exp = BX.blank(x, blank, G_)
        _bytes_equal(ctx.blank(x, blank, G_), exp)
        # each channel is treated on its own
        one = ctx.blank(np.ascontiguousarray(x[:, C - 1]), blank, G_)
        _bytes_equal(one, [np.ascontiguousarray(e[:, C - 1]) for e in exp])
    y, med, nz = BX.blank(_signal(nin, C, 2, 200 + C, s16), 24, 2)
    xf = BX.as_float(_signal(nin, C, 2, 200 + C, s16))
    same = y.view(np.uint32) == xf.view(np.uint32)
    assert y[2 * N - 1, 0] != 0 and same[2 * N - 1:2 * N + 3, 0].all()                   # even channel: the halo sample is not flagged
    assert (y[2 * N - 2:2 * N + 3, 1] == 0).all() and same[2 * N - 3, 1]                 # odd channel: flagged across the edge


@pytest.mark.gpu
def test_special_values(ctx):
    """tests/test_blank.py's inputs: ties at the median, an all-equal block, a zero block followed by signal, a block of
    subnormals, NaN and inf in blocks with and without a threshold -- one channel and three interleaved"""
    for blank, G_ in ((24, 2), (4, 0), (1024, 64)):
        for x in (BX.make_input(0), BX.make_input(1, nblocks=8, extra=0), BX.tie_input()):
            _bytes_equal(ctx.blank(x, blank, G_), BX.blank(x, blank, G_))
        x3 = np.stack([BX.make_input(s) for s in (0, 2, 3)], axis=1)
        x3[:, 1] = np.roll(x3[:, 1], N)
        _bytes_equal(ctx.blank(x3, blank, G_), BX.blank(x3, blank, G_))


@pytest.mark.gpu
def test_device_memory_and_optional_outputs(G, ctx):
    import torch
    for s16 in (False, True):
        x = _signal(3 * N + 5, 2, 2, 300, s16)
        exp = BX.blank(x, 24, 2)
        got = ctx.blank(torch.from_numpy(x).to("cuda:0"), 24, 2)
        _bytes_equal([g.cpu().numpy() for g in got], exp)
    # med and nzero may be NULL; bad arguments are refused before any launch
    import ctypes as C_
    x = _signal(N + 3, 1, 2, 301)
    out = np.full(x.shape, 7.0, np.float32)
    L = ctx.L
    before = G.blank_launch_counts()
    assert L.uwspr_blank_batch(ctx.h, C_.c_void_p(x.ctypes.data), len(x), 1, 0, 0, 24, 2, C_.c_void_p(out.ctypes.data), None, None) == 0
    assert out.tobytes() == BX.blank(x, 24, 2)[0].tobytes()
    mid = G.blank_launch_counts()
    assert (mid[0] - before[0], mid[2] - before[2]) == (1, 1) and mid[1] == before[1] and mid[3] == before[3]
    for blank, guard in ((3, 2), (0, 2), (1025, 2), (24, -1), (24, 65)):
        assert L.uwspr_blank_batch(ctx.h, C_.c_void_p(x.ctypes.data), len(x), 1, 0, 0, blank, guard, C_.c_void_p(out.ctypes.data), None, None) == ERR_ARG
    assert L.uwspr_blank_batch(ctx.h, C_.c_void_p(x.ctypes.data), len(x), 65, 0, 0, 24, 2, C_.c_void_p(out.ctypes.data), None, None) == ERR_ARG
    assert G.blank_launch_counts() == mid
    for name, bad in (("blank", 3), ("blank", 1025), ("blank", -1), ("blank_guard", 65), ("blank_guard", -1)):
        with pytest.raises(G.UwsprError) as e:
            ctx.set_option(name, bad)
        assert e.value.status == ERR_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True])
def test_one_launch_door_with_64_bit_origins(G, ctx, s16):
    """ONE launch of each kernel: the record's blocks sit at block 2^32 - 1 on (audio index near 2^44), the level table
    starts there, and the buffer starts late, ends soon or holds one sample.  Samples outside the buffer do not exist
    (never flagged); an output outside it is +0."""
    import torch
    B0, G_, C, blank = (1 << 32) - 1, 2, 2, 24
    K = 4
    x = _signal(K * N, C, G_, 400, s16)
    xf = BX.as_float(x)
    dev = torch.from_numpy(x).to("cuda:0")
    lev_exp = BX.levels(x).view(np.float32)                      # [K, C]; local block k is block B0 + k
    flags = BX.flags(x, blank)

    def expect(a, b, y0, nout):
        """buffer = local frames [a, b), outputs local [y0, y0 + nout)"""
        f = flags.copy()
        f[:a] = False
        f[b:] = False
        hit = BX.dilate(f, G_)
        ex = np.zeros_like(xf)
        ex[a:b] = xf[a:b]
        y = np.where(hit, np.float32(0), ex).astype(np.float32)[y0:y0 + nout]
        nb = (y0 + nout - 1) // N - y0 // N + 1
        nz = np.array([hit[max(y0, k * N):min(y0 + nout, (k + 1) * N)].sum(axis=0) for k in range(y0 // N, y0 // N + nb)], np.int32)
        return y, nz

    before = G.blank_launch_counts()
    # the whole record: levels of all K blocks, then every output
    lev = torch.zeros((K, C), dtype=torch.float32, device="cuda:0")
    out = torch.full((K * N, C), 7.0, dtype=torch.float32, device="cuda:0")
    nz = torch.full((K, C), -1, dtype=torch.int32, device="cuda:0")
    ctx.debug_blank_launch(dev, B0 * N, lev, B0, B0, K, blank, G_, out, B0 * N, nz, nch=C)
    assert lev.cpu().numpy().tobytes() == lev_exp.tobytes()
    ey, enz = expect(0, K * N, 0, K * N)
    assert out.cpu().numpy().tobytes() == ey.tobytes() and (nz.cpu().numpy() == enz).all()
    assert enz[1:].sum() > 0
    # levels only, of the two middle blocks, into their rows of a table that starts one block early
    lev2 = torch.full((K + 1, C), -1.0, dtype=torch.float32, device="cuda:0")
    ctx.debug_blank_launch(dev, B0 * N, lev2, B0 - 1, B0 + 1, 2, blank, G_, None, 0, None, nch=C)
    l2 = lev2.cpu().numpy()
    assert l2[2:4].tobytes() == lev_exp[1:3].tobytes() and (l2[[0, 1, 4]] == -1).all()
    # buffers that start late, end soon or hold one sample; outputs that start and end inside blocks
    cases = [(N + 100, 3 * N - 7, N + 90, 2 * N), (2 * N - 1, 2 * N, 2 * N - 1 - G_, 1 + 2 * G_), (2 * N, 2 * N + 1, 2 * N - G_, 1 + 2 * G_),
             (0, K * N, 2 * N - 1, 2), (N - G_, K * N, N, N)]
    for a, b, y0, nout in cases:
        out = torch.full((nout, C), 7.0, dtype=torch.float32, device="cuda:0")
        nb = (y0 + nout - 1) // N - y0 // N + 1
        nz = torch.full((nb, C), -1, dtype=torch.int32, device="cuda:0")
        ctx.debug_blank_launch(dev[a:b], B0 * N + a, lev, B0, B0, 0, blank, G_, out, B0 * N + y0, nz, nch=C)
        ey, enz = expect(a, b, y0, nout)
        assert out.cpu().numpy().tobytes() == ey.tobytes(), (a, b, y0, nout)
        assert (nz.cpu().numpy() == enz).all(), (a, b, y0, nout)
    after = G.blank_launch_counts()
    d = tuple(p - q for p, q in zip(after, before))
    assert d == ((0, 2, 0, 1 + len(cases)) if s16 else (2, 0, 1 + len(cases), 0)), d
    # a level launch outside the table is refused
    with pytest.raises(G.UwsprError) as e:
        ctx.debug_blank_launch(dev, B0 * N, lev, B0, B0 + K, 1, blank, G_, None, 0, None, nch=C)
    assert e.value.status == ERR_ARG
