"""K14, the call search (uwspr_calls_set / uwspr_calls_batch): Context.calls equals the numpy restatement
(tests/call_exact.py) byte for byte, over the host form, the device form and the pipe's scattered-offset form.

Random asymmetric bytes against numpy are the lane-map check of the int8 MFMA and of the sign fold into the A operand: a
mask applied to the wrong k, a sign folded into B (bytes 0 are -128) or a pad byte that is not zero changes `best` or the
scores.  Item counts walk the 16-item tile; callsign counts the grid's z; the locator sets walk the bitmap (all, the 100
scattered locators of a field, one locator, a random bitmap whose last bit is set) and the power sets the loop over the
masks.  The restatement's cost is callsigns x locators x powers x items, so the full 615 600 hypotheses per callsign go
with few callsigns and items, and 64 callsigns with a thinned bitmap and three powers."""
import ctypes as C

import numpy as np
import pytest

import call_exact as CX
import deep_exact as X

pytestmark = pytest.mark.gpu
NS = (1, 15, 16, 17, 33)
ERR_ARG = -6
P3 = (0, 37, 60)


@pytest.fixture(scope="module")
def calls64():
    return CX.random_calls(np.random.Generator(np.random.Philox(0xCA111000)), 64)


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


def random_vectors(n, seed):
    rng = np.random.Generator(np.random.Philox(0xCA112000 + seed))
    s = rng.integers(0, 256, (n, 162), dtype=np.uint8)
    s[:, 0], s[:, 161], s[:, 64], s[:, 63] = 0, 255, 0, 255   # the int8 edges at the ends and across a k-step
    return s


def random_bitmap(seed, last=True):
    """about one locator in eight, the last one (the bitmap's last bit) among them"""
    rng = np.random.Generator(np.random.Philox(0xCA113000 + seed))
    r = rng.integers(0, 256, (3, CX.NGRID // 8), dtype=np.uint8)
    bm = r[0] & r[1] & r[2]
    if last:
        bm[-1] |= 0x80
    return bm


def bitmap_of(grids):
    return None if grids is None else (grids if isinstance(grids, np.ndarray) else CX.grids_bitmap(grids))


def set_both(G, ctx, calls, grids, powers):
    """the set through the Python layer (a bitmap array goes straight to the C call) -> (bitmap, power mask) for the restatement"""
    bm = bitmap_of(grids)
    if isinstance(grids, np.ndarray):
        arr = (C.c_char_p * len(calls))(*[c.encode() for c in calls])
        ctx._chk(ctx.L.uwspr_calls_set(ctx.h, arr, len(calls), C.c_void_p(bm.ctypes.data), CX.powers_mask(powers) if powers else 0))
    else:
        ctx.calls_set(calls, grids=grids, powers=powers)
    return bm, (CX.powers_mask(powers) if powers else 0)


def check(G, ctx, calls, grids, powers, sym, device=True):
    import torch
    bm, pm = set_both(G, ctx, calls, grids, powers)
    want = CX.call_restate(G, calls, bm, pm, sym)
    host = ctx.calls(sym)
    assert host.dtype == G.native.CALL_RESULT_DTYPE == CX.CALL_DTYPE
    assert host.tobytes() == want.tobytes(), (host[:4], want[:4])
    if device:
        dev = ctx.calls(torch.from_numpy(np.ascontiguousarray(sym)).to("cuda:0"))
        assert dev.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("A", (1, 2, 3))
@pytest.mark.parametrize("n", NS)
def test_items_and_callsigns_equal_the_restatement(G, ctx, calls64, n, A):
    check(G, ctx, calls64[:A], random_bitmap(n), None, random_vectors(n, 16 * n + A))


def test_64_callsigns_equal_the_restatement(G, ctx, calls64):
    want = check(G, ctx, calls64, random_bitmap(64), P3, random_vectors(17, 64))
    assert len(set(want["call"].tolist())) > 4   # (the winners are spread over the callsigns)


@pytest.mark.parametrize("grids,powers,A,n", [
    (None, None, 1, 17),            # all 615 600 hypotheses of a callsign
    (None, (37,), 3, 33),           # every locator at one power
    (["FN"], None, 3, 16),          # one field: 100 locators scattered over 10 rows of the table
    (["FN", "JO22"], P3, 2, 15),
    (["FN42"], None, 2, 17),        # a single locator
    (["RR99", "AA00"], P3, 3, 33),  # ngrid 0 .. 32399's two ends: AA00 is ngrid 32220, RR99 is 179
])
def test_locator_and_power_sets_equal_the_restatement(G, ctx, calls64, grids, powers, A, n):
    check(G, ctx, calls64[:A], grids, powers, random_vectors(n, 7 * n + A))


def test_ngrid_corners_are_reached(G, ctx, calls64):
    # the first and the last locator of the table, noiseless, among all locators
    calls = calls64[:2]
    bits = CX.call_bits(G, calls)[1][None] ^ CX.grid_bits(G)[[0, 32399]] ^ CX.power_bits(G)[[0, 18]]
    sym = (255 * bits).astype(np.uint8)
    want = check(G, ctx, calls, None, None, sym)
    assert want["best"].tolist() == [CX.join_h(1, 0, 0), CX.join_h(1, 32399, 18)]
    assert want["dbm"].tolist() == [0, 60] and want["ngrid"].tolist() == [0, 32399] and want["call"].tolist() == [1, 1]


def test_special_vectors(G, ctx, calls64):
    calls = calls64[:3]
    bm = random_bitmap(5)
    gl, dl = CX.bitmap_list(bm), CX.power_list(CX.powers_mask(P3))
    assert gl[-1] == CX.NGRID - 1
    cb, gb, pb = CX.call_bits(G, calls), CX.grid_bits(G), CX.power_bits(G)
    first = cb[0] ^ gb[gl[0]] ^ pb[dl[0]]                       # the first allowed hypothesis
    last = cb[2] ^ gb[gl[-1]] ^ pb[dl[-1]]                      # the last one, allowed by the bitmap's last bit only
    lastbit = cb[1] ^ gb[CX.NGRID - 1] ^ pb[dl[1]]
    rng = np.random.Generator(np.random.Philox(0xCA114000))
    rails = (255 * rng.integers(0, 2, (4, 162))).astype(np.uint8)   # only 0 and 255: -128 and 127
    twice = random_vectors(1, 99)[0]
    sym = np.stack([np.full(162, 128, np.uint8), np.full(162, 255, np.uint8), np.zeros(162, np.uint8),
                    (255 * first).astype(np.uint8), (255 * last).astype(np.uint8), (255 * lastbit).astype(np.uint8),
                    twice, *rails, twice])
    want = check(G, ctx, calls, bm, P3, sym)
    # all 128: every score is 0, the smallest allowed h wins
    assert (int(want[0]["best"]), int(want[0]["sbest"]), int(want[0]["snext"])) == (CX.join_h(0, gl[0], dl[0]), 0, 0)
    noiseless = 162 * 128 - int(first.sum())   # |255 - 128| = 127 where the bit is 1, |0 - 128| = 128 where it is 0
    assert (int(want[3]["best"]), int(want[3]["sbest"])) == (CX.join_h(0, gl[0], dl[0]), noiseless)
    assert int(want[4]["best"]) == CX.join_h(2, gl[-1], dl[-1]) and int(want[4]["ngrid"]) == CX.NGRID - 1
    assert int(want[5]["best"]) == CX.join_h(1, CX.NGRID - 1, dl[1])
    assert want[6].tobytes() == want[-1].tobytes()
    assert not want["reserved"].any()


def test_a_disallowed_hypothesis_is_never_offered(G, ctx, calls64):
    # the noiseless codeword of a hypothesis the set excludes: by its locator, then by its power
    calls = calls64[:2]
    g, d = CX.grid_ngrid("FN42"), CX.P19.index(37)
    sym = (255 * (CX.call_bits(G, calls)[1] ^ CX.grid_bits(G)[g] ^ CX.power_bits(G)[d])).astype(np.uint8)[None]
    bm = CX.grids_bitmap(None)
    bm[g >> 3] &= ~np.uint8(1 << (g & 7))
    a = check(G, ctx, calls, bm, None, sym)
    assert int(a[0]["best"]) != CX.join_h(1, g, d) and int(a[0]["sbest"]) < 162 * 127
    b = check(G, ctx, calls, None, [p for p in CX.P19 if p != 37], sym)
    assert int(b[0]["dbm"]) != 37 and int(b[0]["sbest"]) < 162 * 127
    c = check(G, ctx, calls, None, None, sym)
    assert int(c[0]["best"]) == CX.join_h(1, g, d)


def test_single_hypothesis(G, ctx, calls64):
    sym = random_vectors(17, 3)
    want = check(G, ctx, calls64[5:6], ["JO22"], (23,), sym)
    assert (want["snext"] == CX.INT32_MIN).all() and (want["best"] == CX.join_h(0, CX.grid_ngrid("JO22"), 7)).all()
    assert CX.accepted(want[0], 1, int(want[0]["sbest"]), 10 ** 9)


def test_scattered_offsets_as_the_pipe_reads_them(G, ctx, calls64):
    import torch
    calls = calls64[:3]
    bm, pm = set_both(G, ctx, calls, ["FN", "EM"], P3)
    rng = np.random.Generator(np.random.Philox(0xCA115000))
    buf = rng.integers(0, 256, 40000, dtype=np.uint8)
    off = np.sort(rng.choice(40000 - 162, 33, replace=False)).astype(np.uint64)[::-1].copy()   # unaligned, descending, overlapping allowed
    dev = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()
    res = np.zeros(len(off), G.native.CALL_RESULT_DTYPE)
    fn = ctx.L.uwspr_debug_calls_scattered
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    ctx._chk(fn(ctx.h, C.c_void_p(dev.data_ptr()), C.c_void_p(off.ctypes.data), len(off), C.c_void_p(res.ctypes.data)))
    sym = np.stack([buf[int(o):int(o) + 162] for o in off])
    assert res.tobytes() == CX.call_restate(G, calls, bm, pm, sym).tobytes()


def test_the_list_search_gives_the_same_score(G, ctx, calls64):
    calls = calls64[:3]
    sym = random_vectors(17, 11)
    want = check(G, ctx, calls, random_bitmap(8), None, sym)
    msgs = np.stack([G.call_message(calls[int(r["call"])], int(r["ngrid"]), int(r["dbm"])) for r in want])
    for r, m in zip(want, msgs):
        assert np.array_equal(m, G.wspr_pack("%s %s %d" % (calls[int(r["call"])], CX.ngrid_grid(int(r["ngrid"])), int(r["dbm"]))))
    # a list of every item's message(best): all of them are hypotheses of the set, so no list score exceeds the set's sbest,
    # and the item's own message reaches it
    ctx.deep_set_list(np.unique(msgs, axis=0))
    deep = ctx.deep(sym)
    assert deep["sbest"].tolist() == want["sbest"].tolist()
    assert X.scores(X.code_table(G, msgs), sym).diagonal().tolist() == want["sbest"].tolist()
    for i in (0, 16):   # one message on the list: exactly that message's score
        ctx.deep_set_list(msgs[i][None])
        assert int(ctx.deep(sym[i])[0]["sbest"]) == int(want[i]["sbest"])
    ctx.deep_set_list([])


def test_the_second_set_replaces_the_first(G, ctx, calls64):
    sym = random_vectors(16, 21)
    a = check(G, ctx, calls64[:2], ["FN"], None, sym, device=False)
    b = check(G, ctx, calls64[2:5], ["EM"], P3, sym, device=False)
    assert a.tobytes() != b.tobytes()


def test_no_set_is_an_argument_error(G, ctx, calls64):
    ctx.calls_set(calls64[:1])
    ctx.calls_set([])
    with pytest.raises(G.UwsprError) as e:
        ctx.calls(random_vectors(2, 1))
    assert e.value.status == ERR_ARG and "no call set" in str(e.value)
    fresh = G.Context()
    try:
        with pytest.raises(G.UwsprError) as e:
            fresh.calls(random_vectors(2, 1))
        assert e.value.status == ERR_ARG
        fresh.calls_set([])   # clearing what was never set is fine
    finally:
        fresh.close()
