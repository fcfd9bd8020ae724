"""K10 (uwspr_blockdemod_batch) against a binary64 numpy restatement of the definition in include/uwspr_hip.h: complex tone
correlations per symbol, the per-symbol carrier rotation theta_i = 2 pi f_i 256 / 375 + pi, blocks of 1, 2 and 3 symbols,
the maxima over their data sequences, mode 2's normalisation.  block_restate (tests/blockdemod_exact.py, importable from
here as before) is written from the header's text, not from the kernel, and is what tests/golden/make_block_pipe_seeds.py
picks the pipe test's seeds with.  The edges of the definition are in tests/test_gpu_blockdemod_edges.py.

Frames: three of tests/test_gpu_osd_pipe.py's text_frame model at -24 dB and one noise-free frame of the same model.
Tolerance: every byte within 1 of the restatement's and at most 1 % of a call's bytes different at all -- a 256-term
binary32 sum is off by <= 1.5e-5 relative at worst (typically 1e-6), which after 50 / fac puts v within ~1e-3 of its exact
value, so a byte flips with probability <= ~2e-3; an error in the definition changes tens of per cent."""
import ctypes as C

import numpy as np
import pytest

from blockdemod_exact import block_restate, clean_frame, frame_offset, slm_at_zero  # noqa: F401 (the pipe test and the seed script import them from here)
from test_gpu_osd_pipe import text_frame

TEXT, SNR_DB = "K1ABC FN42 37", -24.0
SEEDS = [11, 12, 13]          # the noisy frames; CLEAN_SEED's frame is noise-free
CLEAN_SEED = 14
DF = 375.0 / 256.0
NSYM, NP, HOP = 162, 45000, 3375
LAST = 45000 - 41472 + 300    # a shift with which the last symbols run off the end


@pytest.fixture(scope="module")
def data(G):
    frames = np.stack([text_frame(G, TEXT, s, SNR_DB) for s in SEEDS] + [clean_frame(G, TEXT, CLEAN_SEED)])
    offs = [frame_offset(s) for s in SEEDS + [CLEAN_SEED]]
    items = [
        {"frame": 0, "shift": 375, "f": offs[0], "drift": 0.0},      # nominal
        {"frame": 0, "shift": 371, "f": offs[0] + 0.3, "drift": 2.0},   # two items in one frame; a drift
        {"frame": 1, "shift": -200, "f": offs[1], "drift": -2.0},    # leading samples missing, sample 0 excluded
        {"frame": 2, "shift": LAST, "f": offs[2], "drift": 0.0},     # the last symbols run off the end
        {"frame": 3, "shift": 375, "f": offs[3], "drift": 0.0},      # noise-free
    ]
    want = np.stack([block_restate(frames[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3) for it in items])
    return {"frames": frames, "offs": offs, "items": items, "want": want}


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


def _close(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d bytes differ (%.3f %%), largest difference %d" % (what, int((d > 0).sum()), d.size, 100.0 * (d > 0).mean(), int(d.max())))
    assert d.max() <= 1, what
    assert (d > 0).mean() <= 0.01, what


@pytest.mark.gpu
def test_bytes_equal_the_restatement(ctx, data):
    got = ctx.blockdemod(data["frames"], data["items"])
    assert got.shape == (len(data["items"]), 3, NSYM) and got.dtype == np.uint8
    _close(got, data["want"], "host frames, 5 items")
    for nb in range(3):   # no block length is a copy of another
        assert not np.array_equal(got[0][nb], got[0][(nb + 1) % 3])


@pytest.mark.gpu
def test_no_items(ctx, data):
    assert ctx.blockdemod(data["frames"], []).shape == (0, 3, NSYM)


@pytest.mark.gpu
def test_seventy_items_and_an_item_alone(G, ctx, data):
    rng = np.random.Generator(np.random.Philox(0xB10C))
    items = []
    for q in range(70):
        b = min(q // 18, 3)
        items.append({"frame": b, "shift": int(rng.integers(-300, LAST + 400)), "f": data["offs"][b] + float(rng.uniform(-1.0, 1.0)),
                      "drift": float(rng.choice([0.0, 2.0, -2.0]))})
    items[5] = dict(data["items"][0])                     # (frame 0)
    items[40] = dict(data["items"][3])                    # (frame 2)
    got = ctx.blockdemod(data["frames"], items)
    want = np.stack([block_restate(data["frames"][it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3) for it in items])
    _close(got, want, "70 items in one call")
    alone = ctx.blockdemod(data["frames"], [items[5], items[40]])
    assert np.array_equal(alone[0], got[5]) and np.array_equal(alone[1], got[40])
    for q in (17, 69):
        assert np.array_equal(ctx.blockdemod(data["frames"], [items[q]])[0], got[q]), q


@pytest.mark.gpu
def test_the_limits_of_the_item_parameters(G, ctx, data):
    """|f| <= 1e4 Hz, |drift| <= 1e3 Hz, |shift| <= 2^20 are accepted: the noise-free signal at the alias of +-9999.7 Hz
    (9999.7 - 27 x 375 = -125.3: the same samples), a noise-free signal that drifts by +-1000 Hz, and items all of whose
    samples are missing.  The phases (up to 6800 turns within a symbol) are reduced in binary64 on both sides."""
    wide = float(np.float32(9999.7))
    frames = np.stack([clean_frame(G, TEXT, CLEAN_SEED, off=wide - 27 * 375.0), clean_frame(G, TEXT, CLEAN_SEED, off=27 * 375.0 - wide),
                       clean_frame(G, TEXT, CLEAN_SEED, off=1.25, drift=1000.0), clean_frame(G, TEXT, CLEAN_SEED, off=-2.5, drift=-1000.0),
                       data["frames"][0]])
    items = [{"frame": 0, "shift": 375, "f": wide, "drift": 0.0}, {"frame": 1, "shift": 375, "f": -wide, "drift": 0.0},
             {"frame": 2, "shift": 375, "f": 1.25, "drift": 1000.0}, {"frame": 3, "shift": 375, "f": -2.5, "drift": -1000.0},
             {"frame": 4, "shift": 1 << 20, "f": data["offs"][0], "drift": 0.0}, {"frame": 4, "shift": -(1 << 20), "f": data["offs"][0], "drift": 2.0}]
    want = np.stack([block_restate(frames[it["frame"]], it["shift"], it["f"], it["drift"], G.synth.PR3) for it in items])
    got = ctx.blockdemod(frames, items)
    _close(got[:4], want[:4], "f = +-9999.7 Hz and drift = +-1000 Hz")
    sym = G.wspr_symbols(TEXT)
    for q in range(4):       # the restatement and the kernel both still read the transmitted bits there
        for nb in range(3):
            assert np.array_equal(want[q][nb] >= 128, (sym >> 1).astype(bool)), (q, nb)
            assert np.array_equal(got[q][nb] >= 128, (sym >> 1).astype(bool)), (q, nb)
    assert (want[4:] == 128).all() and got[4:].tobytes() == bytes([128]) * (2 * 3 * NSYM)    # every sample missing


@pytest.mark.gpu
def test_host_device_and_in_place_frames_agree(G, ctx, data):
    import torch
    host = ctx.blockdemod(data["frames"], data["items"])
    dev = torch.from_numpy(data["frames"]).to("cuda:0")
    torch.cuda.synchronize()
    assert np.array_equal(ctx.blockdemod(dev, data["items"]), host)
    # a stretch of stream at hop 3375: frame b = stream[3375 b : 3375 b + 45000], read where it lies
    rng = np.random.Generator(np.random.Philox(0x57EA))
    stream = np.concatenate([data["frames"][0], (0.5 * rng.standard_normal((2 * HOP, 2))).astype(np.float32)])
    cut = np.stack([stream[HOP * b:HOP * b + NP] for b in range(3)])
    items = [{"frame": 0, "shift": 375, "f": data["offs"][0], "drift": 0.0},
             {"frame": 1, "shift": 375 - HOP, "f": data["offs"][0], "drift": 2.0},
             {"frame": 2, "shift": 375 - 2 * HOP, "f": data["offs"][0], "drift": 0.0}]
    want = ctx.blockdemod(cut, items)
    assert np.array_equal(want[0], host[0])
    sdev = torch.from_numpy(stream).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_frame_stride(HOP)
    try:
        assert np.array_equal(ctx.blockdemod(G.FrameView(3, host=stream), items), want)
        assert np.array_equal(ctx.blockdemod(G.FrameView(3, ptr=sdev.data_ptr()), items), want)
    finally:
        ctx.set_frame_stride(0)


@pytest.mark.gpu
def test_noise_free_frame_carries_the_sent_bits(G, ctx, data):
    got = ctx.blockdemod(data["frames"], [data["items"][4]])[0]
    sym = G.wspr_symbols(TEXT)
    for nb in range(3):
        assert np.array_equal(got[nb] >= 128, (sym >> 1).astype(bool)), nb
        rc, msg = G.fano_decode(G.deinterleave(got[nb]))[:2]
        assert rc == 0 and G.unpack_message(msg[:7].astype(np.int8)) == (0, TEXT), nb


@pytest.mark.gpu
def test_block_length_one_is_the_schedules_vector(G, ctx, data):
    """n = 1 at a try's (f1, jig_shift, drift1) against that try's mode-2 vector of the schedule (the reference's no-FMA
    arithmetic and phasor recurrences: within 1 per byte, not equal)"""
    cands, out = ctx.pipeline_batch(data["frames"][:3], max_per_frame=1)
    items, want = [], []
    for b in range(3):
        if not len(cands[b]) or not out[b, 0]["worth_a_try"]:
            continue
        o, c = out[b, 0], cands[b][0]
        f, drift = np.float32(o["f1"]), np.float32(o["drift1"])
        if int(c["m_type"]) == G.native.NONLINEAR:
            f, drift = np.float32(f + slm_at_zero(c)), np.float32(0.0)
        for idt in (0, 16):
            items.append({"frame": b, "shift": int(o["jig_shift"][idt]), "f": float(f), "drift": float(drift)})
            want.append(o["symbols"][idt])
    assert items
    got = ctx.blockdemod(data["frames"], items)[:, 0, :]
    d = np.abs(got.astype(np.int32) - np.stack(want).astype(np.int32))
    print("n = 1 against the schedule: %d of %d bytes differ, largest difference %d" % (int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1


@pytest.mark.gpu
def test_bad_items_are_refused_before_any_write(G, ctx, data):
    L = G.native.lib()
    fr = np.ascontiguousarray(data["frames"])
    good = {"frame": 1, "shift": 375, "f": 1.0, "drift": 0.0}
    bad = [dict(good, f=2e4), dict(good, f=float("nan")), dict(good, drift=-2e3), dict(good, drift=float("inf")),
           dict(good, shift=(1 << 20) + 1), dict(good, shift=-(1 << 20) - 1), dict(good, frame=4), dict(good, frame=-1)]
    for it in bad:
        for items in ([good, it], [it]):
            arr = G.block_items(items)
            out = np.full((len(arr), 3, NSYM), 0xAA, np.uint8)
            rc = L.uwspr_blockdemod_batch(ctx.h, C.c_void_p(fr.ctypes.data), 4, G.native.HOST, C.c_void_p(arr.ctypes.data), len(arr),
                                          C.c_void_p(out.ctypes.data))
            assert rc == -6 and (out == 0xAA).all(), it
    arr = G.block_items([dict(good, frame=2), dict(good, frame=1)])   # not sorted by frame
    out = np.full((2, 3, NSYM), 0xAA, np.uint8)
    rc = L.uwspr_blockdemod_batch(ctx.h, C.c_void_p(fr.ctypes.data), 4, G.native.HOST, C.c_void_p(arr.ctypes.data), 2, C.c_void_p(out.ctypes.data))
    assert rc == -6 and (out == 0xAA).all()
    with pytest.raises(G.native.UwsprError):
        ctx.blockdemod(data["frames"], [dict(good, f=2e4)])
    # a device output that is no device memory is refused as well
    import torch
    dev = torch.from_numpy(fr).to("cuda:0")
    torch.cuda.synchronize()
    arr = G.block_items([good])
    rc = L.uwspr_blockdemod_batch(ctx.h, C.c_void_p(dev.data_ptr()), 4, G.native.DEVICE_FRAMES, C.c_void_p(arr.ctypes.data), 1,
                                  C.c_void_p(out.ctypes.data))
    assert rc == -6 and (out == 0xAA).all()
