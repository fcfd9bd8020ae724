"""The pipe's option "osd": K9 behind a batch's host tail, on the records Fano timed out on.

One short batch: frames that carry TEXT at -30 dB (synth.make_frames' signal model with a packed message), whose seeds were
picked on the CPU with the oracle's records, the host Fano decoder and the restatement (tests/golden/make_osd_pipe_seeds.py):
SEEDS_OSD are recovered only by ordered-statistics decoding at the default gap, on SEEDS_LOST Fano times out and OSD's
answer does not clear the gap, SEEDS_FANO decode as they always did; four signal-free frames follow.  The run with osd = 2 is compared
with the run with osd = 0 record by record, and every record K9 decoded with the restatement (tests/test_gpu_osd.py) applied
to that candidate's eager record -- uwspr_pipeline_batch with all 17 tries -- under the item rule: the gated try with the
largest jig_sync, the first one on ties.  The gap is set to 0 here so that the acceptance rule is exercised on more than
the rare record that clears the default; the default gap's own run must accept a subset of those."""
import numpy as np
import pytest

from test_gpu_osd import osd_restate

pytestmark = pytest.mark.gpu
TEXT, SNR_DB = "K1ABC FN42 37", -30.0
SEEDS_OSD, SEEDS_LOST, SEEDS_FANO = [38, 53, 60, 81], [0, 2, 4, 7, 8, 9], [1, 3, 5, 6]
NF = len(SEEDS_OSD) + len(SEEDS_LOST) + len(SEEDS_FANO)


def text_frame(G, text, seed, snr_db):
    """one frame of synth.make_frames' model carrying a packed message: 4-FSK at 375 / 256 Hz spacing from sample 375 on, a
    seeded frequency offset within +-6 Hz, complex white noise for snr_db in 2500 Hz"""
    rng = np.random.Generator(np.random.Philox(0x05D7E87 + seed))
    sym = G.wspr_symbols(text).astype(np.float64)
    f_off = rng.uniform(-6.0, 6.0)
    phase = 2.0 * np.pi * np.cumsum(np.repeat((sym - 1.5) * 375.0 / 256.0, 256) + f_off) / 375.0
    sig = np.zeros((45000, 2), np.float64)
    sig[375:375 + 162 * 256, 0] = np.cos(phase)
    sig[375:375 + 162 * 256, 1] = np.sin(phase)
    sig += G.synth.sigma_for_snr(snr_db) * rng.standard_normal((45000, 2))
    return sig.astype(np.float32)


@pytest.fixture(scope="module")
def runs(G):
    import torch
    frames = np.stack([text_frame(G, TEXT, s, SNR_DB) for s in SEEDS_OSD + SEEDS_LOST + SEEDS_FANO])
    noise = np.stack([np.random.Generator(np.random.Philox(0x05D0000 + b)).standard_normal((45000, 2)) for b in range(4)])
    allf = np.concatenate([frames, noise.astype(np.float32)])
    dev = torch.from_numpy(allf).to("cuda:0")
    torch.cuda.synchronize()

    def run(**kw):
        pipe = G.Pipe(hop=45000, batch_frames=len(allf), lanes=1, **kw)
        try:
            pipe.submit_device(dev)
            pipe.flush()
            return pipe.collect(), pipe.stats()
        finally:
            pipe.close()

    ctx = G.Context()
    _, eager = ctx.pipeline_batch(dev, max_per_frame=1)
    ctx.close()
    return {"base": run(), "base2": run(osd=0, osd_gap=0), "osd": run(osd=2, osd_gap=0), "dflt": run(osd=2),
            "order1": run(osd=1, osd_gap=0), "two": run(osd=2, osd_gap=0, passes=2), "eager": eager, "n": len(allf)}


def _item(rec):
    g = [t for t in range(17) if rec["jig_sync"][t] > np.float32(0.12) and rec["jig_rms"][t] > np.float32(52.0 * (50 / 64.0))]
    return max(g, key=lambda t: (rec["jig_sync"][t], -t)) if g else None


def test_osd_zero_changes_nothing(runs):
    (a, sa), (b, sb) = runs["base"], runs["base2"]
    assert a.tobytes() == b.tobytes() and not a["osd"].any()
    for k in ("frames", "batches", "candidates", "decoded", "resumed", "fano_calls", "fano_timeouts"):
        assert sa[k] == sb[k], k


@pytest.mark.parametrize("which,order", [("osd", 2), ("order1", 1)])
def test_osd_records_equal_the_restatement(G, runs, which, order):
    base, recs = runs["base"][0], runs[which][0]
    assert len(base) == len(recs)
    nosd = 0
    for r0, r in zip(base, recs):
        e = runs["eager"][int(r["frame"]), 0]
        want = None
        if r0["worth_a_try"] and not r0["decoded"] and _item(e) is not None:
            t = _item(e)
            d = osd_restate(e["symbols"][t], order)
            if G.unpack_message(d[4])[0] == 0:   # gap 0: every item that unpacks is accepted
                want = (t, d[4].tobytes())
        if want is None:
            assert r["osd"] == 0 and r.tobytes() == r0.tobytes()
        else:
            nosd += 1
            assert r["osd"] == 1 and r["decoded"] == 1 and (int(r["idt"]), r["message"].tobytes()) == want
            x, y = r.copy(), r0.copy()
            for k in ("decoded", "idt", "message", "osd"):
                x[k] = y[k]
            assert x.tobytes() == y.tobytes()   # nothing else in the record moved
    assert nosd > 0
    assert runs[which][1]["decoded"] == runs["base"][1]["decoded"] + nosd


def test_default_gap_accepts_a_subset_and_never_noise(G, runs):
    recs, wide = runs["dflt"][0], runs["osd"][0]
    for r, w in zip(recs, wide):
        if r["osd"]:
            assert w["osd"] == 1 and r.tobytes() == w.tobytes()
            e = runs["eager"][int(r["frame"]), 0]
            d = osd_restate(e["symbols"][int(r["idt"])], 2)
            assert d[1] - d[0] >= G.native.OSD_GAP_DEFAULT
    for rr in (recs, wide):
        assert not rr["osd"][rr["frame"] >= NF].any()   # the signal-free frames
    # the frames picked for it are recovered only by OSD, and every message accepted at the default gap is the transmitted text
    base = runs["base"][0]
    for b in range(len(SEEDS_OSD)):
        r = recs[recs["frame"] == b]
        assert len(r) == 1 and r[0]["osd"] == 1 and not base[base["frame"] == b][0]["decoded"]
    for r in recs[recs["osd"] == 1]:
        assert G.unpack_message(r["message"]) == (0, TEXT)
    lost = recs[(recs["frame"] >= len(SEEDS_OSD)) & (recs["frame"] < len(SEEDS_OSD) + len(SEEDS_LOST))]
    assert not lost["decoded"].any()
    fano = recs[(recs["frame"] >= len(SEEDS_OSD) + len(SEEDS_LOST)) & (recs["frame"] < NF)]
    assert fano["decoded"].all() and not fano["osd"].any()


def test_two_passes_with_osd_keep_the_frame_order(runs):
    recs = runs["two"][0]
    assert (np.diff(recs["frame"]) >= 0).all() and set(recs["frame"].tolist()) <= set(range(runs["n"]))
    first = recs[recs["pass"] == 0]
    assert first.tobytes() == runs["osd"][0].tobytes()   # the first pass is the one-pass run
