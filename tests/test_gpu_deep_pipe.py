"""The pipe's list search (uwspr_pipe_set_list, Pipe(known=...)): K13 behind a batch's host tail, on the records Fano timed
out on, after "block" and before "osd".

One short batch: frames that carry TEXT at -31 dB (text_frame of tests/test_gpu_osd_pipe.py), whose seeds were picked on the
CPU with the oracle's records, the host Fano decoder and the restatement (tests/golden/make_deep_pipe_seeds.py) against a
list of 1024 messages of which TEXT is one: SEEDS_DEEP are recovered only by the list search at the default thresholds (and
not accepted when TEXT is taken off the list), on SEEDS_LOST Fano times out and the list's answer does not clear the
defaults, SEEDS_FANO decode as they always did; four signal-free frames follow.  The run with a list is compared with the run
without one record by record, and every record K13 decoded with the restatement (tests/deep_exact.py) applied to that
candidate's eager record -- uwspr_pipeline_batch with all 17 tries -- under the item rule: the gated try with the largest
jig_sync, the first one on ties.  With both thresholds 0 every item is accepted, so the rule is exercised on every item;
the defaults' own run must accept a subset of those."""
import numpy as np
import pytest

import deep_exact as X
from test_gpu_osd_pipe import text_frame

pytestmark = pytest.mark.gpu
TEXT, SNR_DB = "K1ABC FN42 37", -31.0
NLIST, TEXT_AT = 1024, 700
SEEDS_DEEP, SEEDS_LOST, SEEDS_FANO = [1, 11, 13, 14], [0, 2, 9, 12, 16, 17], [5, 89, 152, 156]
NF = len(SEEDS_DEEP) + len(SEEDS_LOST) + len(SEEDS_FANO)


def known_list(G):
    """1023 random messages with TEXT at index TEXT_AT"""
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE94000)), NLIST - 1)
    text = G.wspr_pack(TEXT)
    assert not (msgs == text).all(axis=1).any()
    return np.ascontiguousarray(np.insert(msgs, TEXT_AT, text, axis=0))


@pytest.fixture(scope="module")
def runs(G):
    import torch
    frames = np.stack([text_frame(G, TEXT, s, SNR_DB) for s in SEEDS_DEEP + SEEDS_LOST + SEEDS_FANO])
    noise = np.stack([np.random.Generator(np.random.Philox(0x05D0000 + b)).standard_normal((45000, 2)) for b in range(4)])
    allf = np.concatenate([frames, noise.astype(np.float32)])
    dev = torch.from_numpy(allf).to("cuda:0")
    torch.cuda.synchronize()
    msgs = known_list(G)
    minus = np.ascontiguousarray(np.delete(msgs, TEXT_AT, axis=0))

    def run(**kw):
        pipe = G.Pipe(hop=45000, batch_frames=len(allf), lanes=1, **kw)
        try:
            pipe.submit_device(dev)
            pipe.flush()
            return pipe.collect(), pipe.stats()
        finally:
            pipe.close()

    def run_cleared():
        pipe = G.Pipe(hop=45000, batch_frames=len(allf), lanes=1, known=msgs, deep_min=0, deep_gap=0)
        try:
            pipe.set_list([])   # M = 0 turns the stage off again
            pipe.submit_device(dev)
            pipe.flush()
            return pipe.collect(), pipe.stats()
        finally:
            pipe.close()

    ctx = G.Context()
    _, eager = ctx.pipeline_batch(dev, max_per_frame=1)
    ctx.close()
    return {"base": run(), "empty": run(known=[]), "cleared": run_cleared(), "wide": run(known=msgs, deep_min=0, deep_gap=0),
            "dflt": run(known=msgs), "minus": run(known=minus), "osd": run(known=msgs, osd=2),
            "two": run(known=msgs, passes=2), "eager": eager, "n": len(allf), "msgs": msgs, "tab": X.code_table(G, msgs),
            "minus_tab": X.code_table(G, minus)}


def _item(rec):
    g = [t for t in range(17) if rec["jig_sync"][t] > np.float32(0.12) and rec["jig_rms"][t] > np.float32(52.0 * (50 / 64.0))]
    return max(g, key=lambda t: (rec["jig_sync"][t], -t)) if g else None


@pytest.mark.parametrize("which", ["empty", "cleared"])
def test_no_list_changes_nothing(runs, which):
    (a, sa), (b, sb) = runs["base"], runs[which]
    assert a.tobytes() == b.tobytes() and not a["osd"].any()
    for k in ("frames", "batches", "candidates", "decoded", "resumed", "fano_calls", "fano_timeouts"):
        assert sa[k] == sb[k], k


def test_records_equal_the_restatement(G, runs):
    base, recs = runs["base"][0], runs["wide"][0]
    assert len(base) == len(recs)
    ndeep = 0
    for r0, r in zip(base, recs):
        e = runs["eager"][int(r["frame"]), 0]
        if r0["worth_a_try"] and not r0["decoded"] and _item(e) is not None:   # thresholds 0: every item is accepted
            t = _item(e)
            d = X.deep_restate(runs["tab"], e["symbols"][t])[0]
            ndeep += 1
            assert r["osd"] == 2 and r["decoded"] == 1 and int(r["idt"]) == t
            assert r["message"].tobytes() == runs["msgs"][int(d["best"])].tobytes()
            x, y = r.copy(), r0.copy()
            for k in ("decoded", "idt", "message", "osd"):
                x[k] = y[k]
            assert x.tobytes() == y.tobytes()   # nothing else in the record moved
        else:
            assert r["osd"] == 0 and r.tobytes() == r0.tobytes()
    assert ndeep >= len(SEEDS_DEEP) + len(SEEDS_LOST)
    assert runs["wide"][1]["decoded"] == runs["base"][1]["decoded"] + ndeep


def test_defaults_accept_a_subset_and_only_the_text(G, runs):
    recs, wide, base = runs["dflt"][0], runs["wide"][0], runs["base"][0]
    N = G.native
    for r, w, r0 in zip(recs, wide, base):
        if r["osd"]:
            assert r["osd"] == 2 and w["osd"] == 2 and r.tobytes() == w.tobytes()
            e = runs["eager"][int(r["frame"]), 0]
            d = X.deep_restate(runs["tab"], e["symbols"][int(r["idt"])])[0]
            assert X.accepted(d, NLIST, N.DEEP_MIN_DEFAULT, N.DEEP_GAP_DEFAULT)
            assert G.unpack_message(r["message"]) == (0, TEXT)
        else:
            assert r.tobytes() == r0.tobytes()
    assert not recs["osd"][recs["frame"] >= NF].any()   # the signal-free frames
    for b in range(len(SEEDS_DEEP)):   # recovered only by the list search
        r = recs[recs["frame"] == b]
        assert len(r) == 1 and r[0]["osd"] == 2 and r[0]["decoded"] == 1 and not base[base["frame"] == b][0]["decoded"]
    lost = recs[(recs["frame"] >= len(SEEDS_DEEP)) & (recs["frame"] < len(SEEDS_DEEP) + len(SEEDS_LOST))]
    assert not lost["decoded"].any()
    fano = recs[(recs["frame"] >= len(SEEDS_DEEP) + len(SEEDS_LOST)) & (recs["frame"] < NF)]
    assert fano["decoded"].all() and not fano["osd"].any()
    assert runs["dflt"][1]["decoded"] == runs["base"][1]["decoded"] + int((recs["osd"] == 2).sum())


def test_the_list_without_the_text_decodes_nothing(G, runs):
    N = G.native
    # the seed-picking condition, on the CPU first: the restatement accepts no item against the list without TEXT
    for r0 in runs["base"][0]:
        e = runs["eager"][int(r0["frame"]), 0]
        if r0["worth_a_try"] and not r0["decoded"] and _item(e) is not None:
            d = X.deep_restate(runs["minus_tab"], e["symbols"][_item(e)])[0]
            assert not X.accepted(d, NLIST - 1, N.DEEP_MIN_DEFAULT, N.DEEP_GAP_DEFAULT)
    recs = runs["minus"][0]
    assert not recs["osd"].any() and recs.tobytes() == runs["base"][0].tobytes()


def test_osd_takes_only_what_the_list_left(runs):
    recs, dflt, base = runs["osd"][0], runs["dflt"][0], runs["base"][0]
    assert len(recs) == len(dflt)
    for r, d, r0 in zip(recs, dflt, base):
        if d["osd"] == 2:
            assert r.tobytes() == d.tobytes()   # K13 took it: K9 never saw it
        else:
            assert r["osd"] in (0, 1)
            if r["osd"] == 0:
                assert r.tobytes() == r0.tobytes()
    assert (dflt["osd"] == 2).sum() == (recs["osd"] == 2).sum() >= len(SEEDS_DEEP)


def test_two_passes_keep_the_frame_order(runs):
    recs = runs["two"][0]
    assert (np.diff(recs["frame"]) >= 0).all() and set(recs["frame"].tolist()) <= set(range(runs["n"]))
    first = recs[recs["pass"] == 0]
    assert first.tobytes() == runs["dflt"][0].tobytes()   # the first pass is the one-pass run


def test_options_and_list_rules_through_the_pipe(G, runs):
    msgs = runs["msgs"]
    pipe = G.Pipe(hop=45000, batch_frames=2, lanes=1)
    try:
        for name in ("deep_min", "deep_gap"):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_option(name, -1)
            assert e.value.status == -6
            pipe.set_option(name, 0)
        bad = msgs[:8].copy()
        bad[7] = bad[2]
        with pytest.raises(G.UwsprError) as e:
            pipe.set_list(bad)
        assert e.value.status == -6
        pipe.set_list(msgs[:8])
        pipe.set_list([TEXT])
        pipe.set_list([])
    finally:
        pipe.close()


def test_decode_wav_dicts_carry_deep(G, tmp_path):
    p = str(tmp_path / "mono.wav")
    G.encode_wav(p, [(TEXT, 0, 0, 2.0)])
    plain = G.decode_wav(p, batch_frames=8)
    out = G.decode_wav(p, batch_frames=8, known=[TEXT, "W1AW EM10 30"])
    assert out and all(d["deep"] in (0, 1) and d["osd"] in (0, 1) for d in out)
    assert {d["text"] for d in out} == {TEXT}
    assert [dict(d, deep=0) for d in plain] == plain and all("deep" in d for d in plain)
    # what Fano decodes is not the list's to take
    assert [d for d in out if not d["deep"]] == plain
