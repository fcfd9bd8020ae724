"""K2 (spectrum statistics, peak pick, rank sort) and K3 (coarse search, running-best selection) on DESIGNED spectrograms,
handed to the kernels directly (Context.fdr_from_ps) and compared with the CPU oracle: oracle.stats, oracle.peaks and
oracle.search(..., want_grid=True).  The inputs and what each of them reaches are in tests/spectrum_cases.py; that they
reach it is asserted on the oracle alone in tests/test_spectrum_cases.py.  Here: bytes (NaN by position).

The oracle is given the band tile embedded in a full spectrogram with a large finite poison outside the band, so what it
computes rests on nothing the library was not given.
"""
import ctypes as C

import numpy as np
import pytest

import spectrum_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(G, oracle):
    """one context per set of constructor arguments"""
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = G.Context(**kw)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def cand_slots(ctx):
    return min(ctx.maxfreqs, max(1, (ctx.info.finpb - 1) // 2))


def tiles_of(ctx, fulls):
    lo, w = ctx.info.band_lo, ctx.info.band_w
    return S.cut(np.stack(fulls), lo, w)


def searched(npk, maxfreqs, limit=13):
    """which candidates the CPU searches: all of a short list; of a long one the first, the last, the maxfreqs-th and
    four in between (a search costs the oracle about 50 ms)"""
    if npk <= limit:
        return list(range(npk))
    return sorted(set([0, npk - 1, min(npk, maxfreqs) - 1] + [npk * q // 5 for q in range(1, 5)]))


def check_k2(ctx, g, fulls, with_search=True):
    """every K2 output of every frame against the oracle, then the searched candidates' records"""
    lo, w = ctx.info.band_lo, ctx.info.band_w
    assert (ctx.info.finpb, ctx.info.n, ctx.info.noiseidx) == (g.finpb, g.n, g.noiseidx)
    tiles = tiles_of(ctx, fulls)
    got = ctx.fdr_from_ps(tiles)
    ps, psavg, smraw, smspec, noise = ctx.fdr_spectrum(len(fulls))
    assert ps.tobytes() == tiles.tobytes()
    npks = []
    for b in range(len(fulls)):
        full = S.embed(tiles[b], lo)
        k2 = S.k2_oracle(g, full)
        assert psavg[b].tobytes() == k2["psavg"][lo:lo + w].tobytes(), b
        assert smraw[b].tobytes() == k2["smraw"].tobytes(), b
        assert S.same_float(smspec[b], k2["smspec"]), b
        assert S.same_float(noise[b], k2["noise"]), b
        pk = k2["peaks"]
        assert len(got[b]) == len(pk), (b, len(got[b]), len(pk))
        npks.append(len(pk))
        assert got[b]["snr"].tobytes() == pk["snr"].tobytes(), b             # in order
        # the search moves `freq` to the winning tuned bin, at most two bins from where K2 put it (cc:362,398)
        bins = [S.bin_of(g, f) for f in pk["freq"]]
        for q, a in enumerate(got[b]):
            near = [np.float32(np.float32(g.col(bins[q]) - 2 + i - g.m) * g.df).tobytes() for i in range(S.NIFR)]
            assert np.float32(a["freq"]).tobytes() in near, (b, q)
        if with_search:
            for q in searched(len(pk), g.maxfreqs):
                e, _ = g.fdr.search(full, pk[q:q + 1])
                assert S.record_diff(got[b][q], e) == [], (b, q, S.record_diff(got[b][q], e))
    return got, npks


def check_k3(ctx, g, fulls, kept=True):
    """all ntot metrics and the record of every candidate of every frame against the oracle (kept grid: everything is
    evaluated), or the records alone (no grid: the pruned evaluation)"""
    lo = ctx.info.band_lo
    tiles = tiles_of(ctx, fulls)
    ctx.keep_syncgrid(cand_slots(ctx) if kept else 0)
    try:
        got = ctx.fdr_from_ps(tiles)
        grid = ctx.fdr_syncgrid(len(fulls)) if kept else None
    finally:
        ctx.keep_syncgrid(0)
    for b in range(len(fulls)):
        full = S.embed(tiles[b], lo)
        pk = S.k2_oracle(g, full)["peaks"]
        assert len(got[b]) == len(pk) >= 1, (b, len(got[b]), len(pk))
        for q in range(len(pk)):
            e, egrid = g.fdr.search(full, pk[q:q + 1], want_grid=kept)
            if kept:
                assert grid[b, q].shape == egrid.shape
                assert S.same_float(grid[b, q], egrid), (b, q, int((grid[b, q] != egrid).sum()))
            assert S.record_diff(got[b][q], e) == [], (b, q, kept, S.record_diff(got[b][q], e))
    return got


# ------------------------------------------------------------------------------------------------------- the door
def test_door_equals_batch(G, ctxs):
    """K2 and K3 behind the door are K2 and K3 of uwspr_fdr_batch: fed the spectrogram a batch left behind, the door
    returns the same bytes -- candidates, npk, statistics, kept grids -- from host memory and from device memory"""
    import torch
    ctx = ctxs()
    frames = G.synth.make_frames(2, seed=0x5EED, snr_db=-20.0)
    ctx.keep_syncgrid(2)
    try:
        a = ctx.fdr_batch(frames)
        sa = ctx.fdr_spectrum(2)
        ga = ctx.fdr_syncgrid(2)
        for ps in (sa[0], torch.from_numpy(sa[0]).to("cuda:0")):
            b = ctx.fdr_from_ps(ps)
            sb = ctx.fdr_spectrum(2)
            gb = ctx.fdr_syncgrid(2)
            for f in range(2):
                assert len(a[f]) == len(b[f]) >= 1 and a[f].tobytes() == b[f].tobytes()
                for q in range(min(2, len(a[f]))):
                    assert ga[f, q].tobytes() == gb[f, q].tobytes()
            for x, y in zip(sa, sb):
                assert x.tobytes() == y.tobytes()
    finally:
        ctx.keep_syncgrid(0)


def test_door_argument_errors(G, ctxs):
    """null pointers, B <= 0, an unknown `where`, host memory called device memory, a device range too short: status
    codes before any launch, and the context works afterwards"""
    import torch
    ctx = ctxs()
    g = S.geom()
    N = G.native
    tile = tiles_of(ctx, [S.comb(g)])
    want = ctx.fdr_from_ps(tile)
    f = ctx.L.uwspr_debug_fdr_from_ps
    cands = np.zeros((1, ctx.maxfreqs), N.CAND_DTYPE)
    npk = np.zeros(1, np.int32)
    hp, hc, hn = (C.c_void_p(a.ctypes.data) for a in (tile, cands, npk))
    ARG = -6
    assert f(None, hp, 1, N.HOST, hc, hn) == ARG
    assert f(ctx.h, None, 1, N.HOST, hc, hn) == ARG
    assert f(ctx.h, hp, 0, N.HOST, hc, hn) == ARG
    assert f(ctx.h, hp, -1, N.HOST, hc, hn) == ARG
    assert f(ctx.h, hp, 1, 7, hc, hn) == ARG
    assert f(ctx.h, hp, 1, N.DEVICE, hc, hn) == ARG                     # pageable host memory is not device memory
    dps = torch.from_numpy(tile).to("cuda:0")
    dc = torch.zeros(ctx.maxfreqs * 48, dtype=torch.uint8, device="cuda:0")
    dn = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dp = lambda t: C.c_void_p(t.data_ptr())
    assert f(ctx.h, dp(dps), 1, N.DEVICE, hc, dp(dn)) == ARG            # cands on the host
    assert f(ctx.h, dp(dps), 1, N.DEVICE, dp(dc), hn) == ARG            # npk on the host
    raw = C.c_void_p()                                                  # (an allocation of its own: a tensor may lie
    assert ctx.L.uwspr_device_alloc(tile.nbytes, C.byref(raw)) == 0     #  inside a larger block of the caching allocator)
    try:
        assert f(ctx.h, raw, 2, N.DEVICE, dp(dc), dp(dn)) == ARG        # two frames asked of a one-frame allocation
    finally:
        ctx.L.uwspr_device_free(raw)
    assert b"device memory" in ctx.L.uwspr_last_error(ctx.h)
    assert f(ctx.h, dp(dps), 1, N.DEVICE, dp(dc), dp(dn)) == 0
    ctx.synchronize()
    assert int(dn.cpu()[0]) == len(want[0])
    assert dc.cpu().numpy().tobytes()[:48 * len(want[0])] == want[0].tobytes()
    assert f(ctx.h, hp, 1, N.HOST, None, None) == 0                     # results may stay in the context
    again = ctx.fdr_from_ps(tile)
    assert again[0].tobytes() == want[0].tobytes()


# --------------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("name", sorted(S.K2_CASES))
def test_k2_case(ctxs, name):
    kw, build, cond = S.K2_CASES[name]
    g, ctx = S.geom(**kw), ctxs(**kw)
    fulls = [build(g)]
    if name in ("comb_scalar_copy", "comb_vector_copy"):
        fulls.append(S.comb(g, parity=0))        # a second frame: its tile starts n * band_w floats further on
        tot = ctx.info.n * ctx.info.band_w
        assert ctx.info.n == 349 and tot * 4 <= 60 * 1024
        assert (ctx.info.band_w % 2 == 1 and tot % 4 != 0) if name == "comb_scalar_copy" else tot % 4 == 0
    if name == "comb_hb60_unstaged":
        assert ctx.info.n * ctx.info.band_w * 4 > 60 * 1024
    got, npks = check_k2(ctx, g, fulls)
    figures = cond(g, S.k2_oracle(g, S.embed(tiles_of(ctx, fulls)[0], ctx.info.band_lo)))
    if "peaks" in figures:
        assert npks[0] == figures["peaks"]


def test_k2_widest_pass_band_is_the_library_limit(G):
    """the next wider pass band is refused by the constructor with the range error (and by the oracle)"""
    with pytest.raises(G.native.UwsprError) as e:
        G.Context(halfbandwidth=S.WIDEST_HALFBANDWIDTH + 1)
    assert e.value.status == -2
    with pytest.raises(ValueError):
        S.Geom(halfbandwidth=S.WIDEST_HALFBANDWIDTH + 1)


def test_k2_frames_without_a_peak_beside_frames_with_peaks(ctxs):
    """a batch whose frames 0 and 2 are flat (npk = 0) and whose frames 1 and 3 are combs: the work list K2 compacts
    for the coarse search holds frames 1 and 3 only, and every candidate of those is searched"""
    g, ctx = S.geom(), ctxs()
    fulls = [S.K2_CASES[n][1](g) for n in S.BATCH_K2]
    got, npks = check_k2(ctx, g, fulls)
    assert npks == [0, 13, 0, 13]
    assert got[1].tobytes() == got[3].tobytes()


# --------------------------------------------------------------------------------------------------------- K3
@pytest.mark.parametrize("name", sorted(S.K3_CASES))
def test_k3_case(ctxs, name):
    """every metric of the grid, then the record; again without the kept grid, so that the evaluation is pruned"""
    thr = S.K3_CASES[name][0]
    g, ctx = S.geom(threshold=thr), ctxs(threshold=thr)
    full, j = S.k3_build(g, name)
    a = check_k3(ctx, g, [full], kept=True)
    b = check_k3(ctx, g, [full], kept=False)
    assert a[0].tobytes() == b[0].tobytes() or np.isnan(a[0]["sync"]).any()
    assert j in [S.bin_of(g, f) for f in S.k2_oracle(g, S.embed(tiles_of(ctx, [full])[0], ctx.info.band_lo))["peaks"]["freq"]]


OTHER = ["allneg_flat_first_t10", "allneg_flat_last_t10", "allneg_tail_t10", "pruned_t10", "seeded_t10"]


@pytest.mark.parametrize("tile", ["0", "1", "2"])
def test_k3_tile_forms(G, monkeypatch, tile):
    """the three tile forms (float4 per centre in LDS, plain sqrt rows in LDS, sqrt rows in HBM) against the ORACLE"""
    monkeypatch.setenv("UWSPR_OPTIONS", "k3_tile=" + tile)       # (shapes the context when it is created)
    g = S.geom(threshold=10)
    ctx = G.Context(threshold=10)
    try:
        fulls = [S.k3_build(g, n)[0] for n in OTHER]
        check_k3(ctx, g, fulls, kept=True)
        check_k3(ctx, g, fulls, kept=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("kw", [dict(maxdrift=2), dict(cf=6000), dict(cf=24000), dict(halfbandwidth=60)],
                         ids=["maxdrift2", "cf6000", "cf24000", "hb60"])
def test_k3_other_geometries(ctxs, kw):
    """drift hypotheses (five linear ones per cell), the tile forms chosen by size at a wider search reach, a wide pass
    band: the cases designed anew for the context's own columns"""
    g, ctx = S.geom(threshold=10, **kw), ctxs(threshold=10, **kw)
    assert (ctx.info.band_lo, ctx.info.band_w, ctx.info.cell_hyps) == g.band() + (g.hc,)
    fulls = [S.k3_build(g, n)[0] for n in OTHER]
    check_k3(ctx, g, fulls, kept=True)
    check_k3(ctx, g, fulls, kept=False)


@pytest.mark.parametrize("kept", [True, False], ids=["grid", "pruned"])
def test_batching_gives_the_bytes_of_single_frames(ctxs, kept):
    """cases mixed in one call at B = 1, 3 and 5 -- frames with one, no, thirteen, one and one candidate -- give what each
    gives alone: the work list across frames, and nothing of one frame in another's result"""
    g, ctx = S.geom(threshold=10), ctxs(threshold=10)
    fulls = [S.k3_build(g, "allneg_flat_first_t10")[0], S.flat(g), S.comb(g), S.k3_build(g, "pruned_t10")[0],
             S.k3_build(g, "nan_t10")[0]]
    tiles = tiles_of(ctx, fulls)
    cap = cand_slots(ctx)
    ctx.keep_syncgrid(cap if kept else 0)
    try:
        def run(t):
            got = ctx.fdr_from_ps(t)
            return got, ctx.fdr_spectrum(len(t))[1:], (ctx.fdr_syncgrid(len(t)) if kept else None)
        alone = [run(tiles[b:b + 1]) for b in range(len(fulls))]
        assert [len(r[0][0]) for r in alone] == [1, 0, 13, 1, 1]
        for B in (1, 3, 5):
            got, spec, grid = run(tiles[:B])
            for b in range(B):
                g1, s1, k1 = alone[b]
                assert len(got[b]) == len(g1[0])
                assert S.same_float(got[b]["sync"], g1[0]["sync"])
                for fld in ("freq", "snr", "shift", "m_type", "V1", "V2", "p1", "p2"):
                    assert got[b][fld].tobytes() == g1[0][fld].tobytes(), (B, b, fld)
                for x, y in zip(spec, s1):
                    assert S.same_float(x[b], y[0]), (B, b)
                for q in range(len(g1[0]) if kept else 0):
                    assert S.same_float(grid[b, q], k1[0, q]), (B, b, q)
    finally:
        ctx.keep_syncgrid(0)
