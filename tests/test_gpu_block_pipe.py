"""The pipe's option "block": K10 behind a batch's host tail, on the records Fano timed out on.

One short batch: frames that carry TEXT at SNR_DB (tests/test_gpu_osd_pipe.py's text_frame), whose seeds were picked on the
CPU with the oracle's records, the host Fano decoder and the restatement of block demodulation
(tests/golden/make_block_pipe_seeds.py; profiles/blockdemod.txt keeps its output): on SEEDS_BLOCK Fano decodes no try of
the strongest candidate and the restated n = 2 or n = 3 vector of the item decodes to TEXT (with a wide margin of Fano
cycles), on SEEDS_LOST those time out as well -- also with ten times the cycle limit and with 2 % of their bytes moved by
+-1, so that a byte in which the kernel differs from the restatement cannot turn either outcome -- SEEDS_FANO decode as
they always did; four signal-free frames follow.  The run with block = 3 is compared with the
run with block = 0 record by record."""
import numpy as np
import pytest

from test_gpu_osd_pipe import text_frame

pytestmark = pytest.mark.gpu
TEXT, SNR_DB = "K1ABC FN42 37", -30.0
SEEDS_BLOCK, SEEDS_LOST, SEEDS_FANO = [8, 30, 56, 78, 54, 93], [9, 16, 22, 23], [1, 3, 5, 6]   # (54, 93: n = 3 only)
NB, NL, NF = len(SEEDS_BLOCK), len(SEEDS_LOST), len(SEEDS_BLOCK) + len(SEEDS_LOST) + len(SEEDS_FANO)


@pytest.fixture(scope="module")
def runs(G):
    import torch
    frames = np.stack([text_frame(G, TEXT, s, SNR_DB) for s in SEEDS_BLOCK + SEEDS_LOST + SEEDS_FANO])
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
    return {"base": run(), "base0": run(block=0), "b3": run(block=3), "b2": run(block=2), "osd": run(block=3, osd=2, osd_gap=0),
            "two": run(block=3, passes=2), "eager": eager, "n": len(allf)}


def _item(rec):
    g = [t for t in range(17) if rec["jig_sync"][t] > np.float32(0.12) and rec["jig_rms"][t] > np.float32(52.0 * (50 / 64.0))]
    return max(g, key=lambda t: (rec["jig_sync"][t], -t)) if g else None


def _block_set(recs):
    return {(int(r["frame"]), int(r["cand"])) for r in recs if r["block"]}


def test_seed_lists_are_what_the_issue_asks_for():
    assert len(SEEDS_BLOCK) >= 3 and len(SEEDS_LOST) >= 3 and len(SEEDS_FANO) >= 3


def test_block_zero_changes_nothing(runs):
    (a, sa), (b, sb) = runs["base"], runs["base0"]
    assert a.tobytes() == b.tobytes() and not a["block"].any()
    for k in ("frames", "batches", "candidates", "decoded", "resumed", "fano_calls", "fano_timeouts"):
        assert sa[k] == sb[k], k


def test_block_three_against_block_zero(G, runs):
    base, recs = runs["base"][0], runs["b3"][0]
    assert len(base) == len(recs)
    sent = G.wspr_pack(TEXT).tobytes()
    nblk = 0
    for r0, r in zip(base, recs):
        if r0["decoded"] or r.tobytes() == r0.tobytes():
            assert r.tobytes() == r0.tobytes()
            continue
        nblk += 1
        e = runs["eager"][int(r["frame"]), 0]
        assert r0["worth_a_try"] and _item(e) is not None
        assert r["decoded"] == 1 and r["block"] in (2, 3) and r["osd"] == 0
        assert int(r["idt"]) == _item(e) and r["message"].tobytes() == sent
        x, y = r.copy(), r0.copy()
        for k in ("decoded", "idt", "message", "block"):
            x[k] = y[k]
        assert x.tobytes() == y.tobytes()   # nothing else in the record moved
    assert nblk > 0
    assert runs["b3"][1]["decoded"] == runs["base"][1]["decoded"] + nblk
    # the frames picked for it are recovered only by block demodulation; the lost ones stay lost; Fano's stay Fano's
    for b in range(NB):
        r = recs[recs["frame"] == b]
        assert len(r) == 1 and r[0]["block"] in (2, 3) and not base[base["frame"] == b][0]["decoded"], b
    lost = recs[(recs["frame"] >= NB) & (recs["frame"] < NB + NL)]
    assert not lost["decoded"].any()
    fano = recs[(recs["frame"] >= NB + NL) & (recs["frame"] < NF)]
    assert fano["decoded"].all() and not fano["block"].any()
    assert not recs["decoded"][recs["frame"] >= NF].any()   # the signal-free frames
    # the extra Fano calls are counted
    assert runs["b3"][1]["fano_calls"] > runs["base"][1]["fano_calls"]


def test_block_two_decodes_a_subset(runs):
    two, three = runs["b2"][0], runs["b3"][0]
    assert _block_set(two) <= _block_set(three)
    assert set(two["block"].tolist()) <= {0, 2}
    for r, w in zip(two, three):
        if r["block"]:
            assert r.tobytes() == w.tobytes()


def test_block_and_osd_never_share_a_record(runs):
    recs = runs["osd"][0]
    assert not ((recs["block"] != 0) & (recs["osd"] != 0)).any()
    assert _block_set(recs) == _block_set(runs["b3"][0])
    for r, w in zip(recs, runs["b3"][0]):
        if r["block"]:
            assert r.tobytes() == w.tobytes()


def test_two_passes_with_block_keep_the_frame_order(runs):
    recs = runs["two"][0]
    assert (np.diff(recs["frame"]) >= 0).all() and set(recs["frame"].tolist()) <= set(range(runs["n"]))
    first = recs[recs["pass"] == 0]
    assert first.tobytes() == runs["b3"][0].tobytes()   # the first pass is the one-pass run


@pytest.mark.parametrize("value", [1, 4, -1])
def test_other_block_lengths_are_refused(G, value):
    with pytest.raises(G.native.UwsprError) as e:
        G.Pipe(hop=45000, batch_frames=4, lanes=1, block=value)
    assert e.value.status == -6
