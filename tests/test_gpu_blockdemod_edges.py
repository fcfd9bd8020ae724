"""K10 (uwspr_blockdemod_batch) at the edges of its definition and of its host side.  tests/blockdemod_exact.py holds the
binary64 restatement, the frames and the items; tests/test_blockdemod.py shows, without a GPU, which misreading of the
definition each item can see and that binary32 alone costs these inputs no byte.  Here: the sample bound 0 < n < 45000
with 30 .. 50 sigma samples at n = 0, 44 999 and 45 000, in contexts with fl = 45 000 and fl = 48 000 and per frame of a
stream read in place; every alignment of the 128-byte staging runs; drifts; bytes 0 and 255; NaN and infinite samples in
every block length; calls that cross the first allocation of 256 items; the asynchronous form (where = UWSPR_DEVICE).
Every comparison is tests/test_gpu_blockdemod.py's criterion against block_restate (every byte within 1, at most 1 % of a
call's bytes different) or byte equality between two results of the kernel."""
import ctypes as C

import numpy as np
import pytest

import blockdemod_exact as BX
from test_gpu_blockdemod import _close

pytestmark = pytest.mark.gpu
NSYM, NP, HOP = BX.NSYM, BX.NP, BX.HOP


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge(G, ctx):
    """edge_items() in one call on frames cut to 45 000 samples: beyond the buffer = 0"""
    items = BX.edge_items()
    return {"items": items, "got": ctx.blockdemod(BX.edge_frames(G, NP), items)}


def _restate(G, frames, items):
    return np.stack([BX.block_restate(frames[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3) for it in items])


def _raw(G, c, frames_ptr, B, where, items, out_ptr):
    arr = G.block_items(items)
    return G.native.lib().uwspr_blockdemod_batch(c.h, C.c_void_p(frames_ptr), B, where, C.c_void_p(arr.ctypes.data), len(arr),
                                                 C.c_void_p(out_ptr))


def test_edge_items_fl_45000(G, edge):
    got = edge["got"]
    assert got.shape == (len(BX.EDGE_NAMES), 3, NSYM)
    _close(got, BX.edge_want(G), "edge items, fl = 45000")
    loud = got[BX.EDGE_NAMES.index("loud symbols")]
    for nb in range(3):
        assert (loud[nb] == 0).any() and (loud[nb] == 255).any(), nb
    # what tests/test_blockdemod.py shows the restatement to tell apart, the kernel tells apart as well
    q0, q1 = BX.EDGE_NAMES.index("spike, shift 0"), BX.EDGE_NAMES.index("spike, last sample 45000")
    for q, mutate in ((q0, "n_ge_0"), (q1, "n_le_np")):
        it = edge["items"][q]
        wrong = BX.block_restate(BX.edge_frames(G)[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3, mutate=mutate)
        assert not BX.meets_criterion(got[q], wrong), mutate


def test_edge_items_fl_48000(G, edge):
    """np = 45 000 whatever fl: the 44 + 39 j at n = 45 000 and the noise up to 47 999 are present and ignored"""
    items = edge["items"]
    c = G.Context(fl=BX.FL_LONG)
    try:
        got = c.blockdemod(BX.edge_frames(G), items)
    finally:
        c.close()
    _close(got, BX.edge_want(G), "edge items, fl = 48000")
    w48 = BX.edge_want(G, BX.FL_LONG)
    for q, it in enumerate(items):
        if BX.reads_from_45000_on(it):   # the restatement with np = fl is something else there, and the kernel is not that
            assert not BX.meets_criterion(w48[q], BX.edge_want(G)[q]), it["name"]
            assert not BX.meets_criterion(got[q], w48[q]), it["name"]
        assert np.array_equal(got[q], edge["got"][q]), it["name"]   # the fl = 45 000 run on the same leading samples


SPECIAL = [(v, p) for v in BX.SPECIAL_VALUES for p in BX.SPECIAL_PLACES]


def test_nan_and_infinities(G, ctx):
    """One NaN, +inf or -inf sample in symbol 0, in symbol 161 or in the middle of a block of 3: all three vectors of every
    item that reads it are 128 (with fmaxf for the maxima, n = 3 lost a NaN -- all eight P NaN left the running maxima at
    their initial 0, soft = 0 for the block's three symbols and the vector was emitted as if nothing had happened -- and
    n = 2 could lose one of two); every item of the same frame and call that does not read it has the clean frame's bytes."""
    clean = BX.edge_frames(G, NP)[5]
    frames = np.stack([clean] + [BX.special_frame(clean, p, v) for v, p in SPECIAL])
    items, hits, twins = [], [], []
    for b, (v, p) in enumerate(SPECIAL):
        hit, miss = BX.special_items(p, 1 + b)
        hits += [len(items) + q for q in range(len(hit))]
        items += hit + miss
        twins += [dict(it, frame=0) for it in hit + miss]
    got = ctx.blockdemod(frames, items)
    ref = ctx.blockdemod(frames, twins)            # the same items on the clean frame
    few = twins[:8]
    _close(ref[:8], _restate(G, frames, few), "noise frame, %d items" % len(few))
    assert not (ref == 128).all(axis=(1, 2)).any()
    for q, it in enumerate(items):
        v, p = SPECIAL[it["frame"] - 1]
        if q in hits:
            for nb in range(3):
                assert (got[q][nb] == 128).all(), "%s in %s, shift %d, n = %d: %d bytes are not 128" % (
                    v, p, it["shift"], nb + 1, int((got[q][nb] != 128).sum()))
        else:
            assert np.array_equal(got[q], ref[q]), (v, p, it["shift"])


def test_calls_that_cross_the_first_allocation(G):
    """the context's item and output buffers start at 256 items: 6 items, then 300 (freed and allocated anew), then the 6"""
    frames = BX.edge_frames(G, NP)[:4]
    offs = [BX.frame_offset(s) for s in BX.SEEDS + [BX.CLEAN_SEED]]
    rng = np.random.Generator(np.random.Philox(0xB10C6))
    items = [{"frame": q // 75, "shift": int(rng.integers(-300, 4301)), "f": offs[q // 75] + float(rng.uniform(-1.0, 1.0)),
              "drift": float(rng.choice([0.0, 2.0, -2.0]))} for q in range(300)]
    six = [items[q] for q in (0, 60, 100, 160, 230, 299)]
    c = G.Context()   # a context of its own: nothing has grown its buffers
    try:
        first = c.blockdemod(frames, six)
        got = c.blockdemod(frames, items)
        again = c.blockdemod(frames, six)
        alone = c.blockdemod(frames, [items[q] for q in (0, 255, 256, 299)])
    finally:
        c.close()
    _close(got, _restate(G, frames, items), "300 items in one call")
    assert np.array_equal(first, again)
    assert np.array_equal(first, got[[0, 60, 100, 160, 230, 299]])
    assert np.array_equal(alone, got[[0, 255, 256, 299]])


def test_device_form_is_asynchronous_and_ordered(G, edge):
    """where = UWSPR_DEVICE through the C ABI: two calls back to back, nothing between them, separate outputs; the second
    call reuses the page-locked items and the device items of the first while the first may still be pending -- once with
    a shorter list, once with one longer than 256, so that both buffers are freed and made anew."""
    import torch
    N = G.native
    frames = BX.edge_frames(G, NP)
    dev = torch.from_numpy(frames).to("cuda:0")
    items = edge["items"]
    rng = np.random.Generator(np.random.Philox(0xB10C7))
    many = [{"frame": q // 30, "shift": int(rng.integers(-300, 4301)), "f": float(rng.uniform(-3.0, 3.0)),
             "drift": float(rng.choice([0.0, 2.0, -2.0]))} for q in range(300)]
    c = G.Context()   # a context of its own: the first calls meet no buffer
    try:
        for first, second in ((items, items[20:27]), (items[3:], many)):
            o1 = torch.full((len(first) * 3 * NSYM,), 0xAA, dtype=torch.uint8, device="cuda:0")
            o2 = torch.full((len(second) * 3 * NSYM,), 0xAA, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rc1 = _raw(G, c, dev.data_ptr(), len(frames), N.DEVICE, first, o1.data_ptr())
            rc2 = _raw(G, c, dev.data_ptr(), len(frames), N.DEVICE, second, o2.data_ptr())
            c.synchronize()
            assert rc1 == 0 and rc2 == 0
            g1, g2 = o1.cpu().numpy().reshape(-1, 3, NSYM), o2.cpu().numpy().reshape(-1, 3, NSYM)
            assert np.array_equal(g1, c.blockdemod(frames, first)) and np.array_equal(g2, c.blockdemod(frames, second))
            if first is items:
                assert np.array_equal(g1, edge["got"])
        _close(g2, _restate(G, frames, many), "300 items, device form")
        # an output that is no device memory: refused before any launch, nothing written anywhere
        before1, before2 = o1.clone(), o2.clone()
        host_out = np.full((len(items), 3, NSYM), 0xAA, np.uint8)
        torch.cuda.synchronize()
        assert _raw(G, c, dev.data_ptr(), len(frames), N.DEVICE, items, host_out.ctypes.data) == -6
        c.synchronize()
        torch.cuda.synchronize()
        assert (host_out == 0xAA).all() and torch.equal(o1, before1) and torch.equal(o2, before2)
    finally:
        c.close()


def test_the_bound_is_per_frame_of_a_stream_read_in_place(G, ctx):
    """frames at hop 3375 read where they lie: sample 0 of frame 1 is stream sample 3375 and n = 45 000 of frame 0 is stream
    sample 45 000 -- both are there (30 .. 50 sigma, so that reading them shows) and both are excluded"""
    import torch
    stream = BX.noise_frame(0xB10C8, HOP + NP)
    stream[HOP] = (-43.0, 36.0)
    stream[NP] = (39.0, 47.0)
    cut = np.stack([stream[HOP * b:HOP * b + NP] for b in range(2)])
    end = NP - BX.FULL
    items = [{"frame": 0, "shift": HOP, "f": 0.7, "drift": 0.0},        # reads stream[3375] as its n = 3375
             {"frame": 0, "shift": end + 1, "f": 0.7, "drift": 0.0},    # its last sample would be n = 45 000
             {"frame": 1, "shift": 0, "f": 0.7, "drift": 0.0},          # its first sample would be n = 0 = stream[3375]
             {"frame": 1, "shift": -255, "f": 0.7, "drift": 2.0},
             {"frame": 1, "shift": NP - HOP - 255, "f": 0.7, "drift": 0.0}]   # reads stream[45000] as its n = 41 625
    want = _restate(G, cut, items)
    longer = np.stack([stream, np.concatenate([stream[HOP:], np.zeros((HOP, 2), np.float32)])])   # the frames with what follows them
    for q, mutate in ((1, "n_le_np"), (2, "n_ge_0"), (3, "n_ge_0")):       # a bound per stream would be seen
        it = items[q]
        wrong = BX.block_restate(longer[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3, mutate=mutate)
        assert not BX.meets_criterion(wrong, want[q]), q
    copied = ctx.blockdemod(cut, items)
    _close(copied, want, "two frames of a stream, copied out")
    sdev = torch.from_numpy(stream).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_frame_stride(HOP)
    try:
        assert np.array_equal(ctx.blockdemod(G.FrameView(2, host=stream), items), copied)
        assert np.array_equal(ctx.blockdemod(G.FrameView(2, ptr=sdev.data_ptr()), items), copied)
    finally:
        ctx.set_frame_stride(0)
