"""The pipe's call search (uwspr_pipe_set_calls, Pipe(calls=...)): K14 behind a batch's host tail, on the records Fano
timed out on, after "block" and the list search and before "osd".

The closed loop of tests/test_gpu_deep_pipe.py: one short batch of frames that carry TEXT at SNR_DB (text_frame of
tests/test_gpu_osd_pipe.py).  Seeds and level were picked on the CPU with the oracle's records, the host Fano decoder and the
restatement at the default thresholds (tests/golden/make_call_pipe_seeds.py; SNR_DB is the level at which it finds at least
four seeds of class "call": 1 among seeds 0 .. 999 at -29 dB, the 6 used here among 0 .. 3999 at -30 dB): on SEEDS_CALL Fano times out on every gated try, the restatement accepts
TEXT with CALLS_WITH (8 callsigns, TEXT's among them, every locator and power: 4.9 M hypotheses) and nothing with
CALLS_OTHER; on SEEDS_LOST it accepts nothing with either; SEEDS_FANO decode as they always did; four signal-free frames
follow.  Every record K14 decoded is compared with the restatement (tests/call_exact.py) applied to that candidate's eager
record -- uwspr_pipeline_batch with all 17 tries -- under the item rule: the gated try with the largest jig_sync, the first
one on ties.  With both thresholds 0 every item is accepted, so the rule is exercised on every item."""
import numpy as np
import pytest

import call_exact as CX
from test_gpu_deep_pipe import _item
from test_gpu_osd_pipe import text_frame

pytestmark = pytest.mark.gpu
TEXT, SNR_DB = "K1ABC FN42 37", -30.0
CALLS_WITH = ["W1AW", "G4ABC", "K1ABC", "JA1XYZ", "VK2DEF", "9A1AA", "DL1QRS", "A1B"]
CALLS_OTHER = ["W1AX", "G4ABD", "K1ABD", "JA1XYW", "VK2DEG", "9A1AB", "DL1QRT", "A1C"]
SEEDS_CALL, SEEDS_LOST, SEEDS_FANO = [38, 853, 2363, 2650, 2871, 3165], [0, 2, 4, 7], [1, 3, 5, 6]
NF = len(SEEDS_CALL) + len(SEEDS_LOST) + len(SEEDS_FANO)
NHYP = 8 * CX.NGRID * CX.NPOW


@pytest.fixture(scope="module")
def runs(G):
    import torch
    frames = np.stack([text_frame(G, TEXT, s, SNR_DB) for s in SEEDS_CALL + SEEDS_LOST + SEEDS_FANO])
    noise = np.stack([np.random.Generator(np.random.Philox(0x05D0000 + b)).standard_normal((45000, 2)) for b in range(4)])
    allf = np.concatenate([frames, noise.astype(np.float32)])
    dev = torch.from_numpy(allf).to("cuda:0")
    torch.cuda.synchronize()

    def run(clear=False, **kw):
        pipe = G.Pipe(hop=45000, batch_frames=len(allf), lanes=1, **kw)
        try:
            if clear:
                pipe.set_calls([])   # A = 0 turns the stage off again
            pipe.submit_device(dev)
            pipe.flush()
            return pipe.collect(), pipe.stats()
        finally:
            pipe.close()

    ctx = G.Context()
    _, eager = ctx.pipeline_batch(dev, max_per_frame=1)
    ctx.close()
    out = {"base": run(), "cleared": run(clear=True, calls=CALLS_WITH, call_min=0, call_gap=0),
           "wide": run(calls=CALLS_WITH, call_min=0, call_gap=0), "dflt": run(calls=CALLS_WITH), "other": run(calls=CALLS_OTHER),
           "both": run(calls=CALLS_WITH, known=[TEXT, "W1AW EM10 30"]), "osd": run(calls=CALLS_WITH, osd=2),
           "two": run(calls=CALLS_WITH, passes=2), "eager": eager, "n": len(allf)}
    items = {}   # frame -> (try, the restatement with CALLS_WITH, with CALLS_OTHER)
    for r0 in out["base"][0]:
        e = eager[int(r0["frame"]), 0]
        if r0["worth_a_try"] and not r0["decoded"] and _item(e) is not None:
            t = _item(e)
            items[int(r0["frame"])] = (t, CX.call_restate(G, CALLS_WITH, None, 0, e["symbols"][t])[0],
                                       CX.call_restate(G, CALLS_OTHER, None, 0, e["symbols"][t])[0])
    out["items"] = items
    return out


def test_without_calls_the_records_are_undecoded(G, runs):
    base = runs["base"][0]
    for b in range(len(SEEDS_CALL) + len(SEEDS_LOST)):
        r = base[base["frame"] == b]
        assert len(r) == 1 and not r[0]["decoded"] and b in runs["items"]
    assert not base["osd"].any()


def test_a_cleared_set_changes_nothing(runs):
    (a, sa), (b, sb) = runs["base"], runs["cleared"]
    assert a.tobytes() == b.tobytes()
    for k in ("frames", "batches", "candidates", "decoded", "resumed", "fano_calls", "fano_timeouts"):
        assert sa[k] == sb[k], k


def test_records_equal_the_restatement(G, runs):
    base, recs = runs["base"][0], runs["wide"][0]
    assert len(base) == len(recs)
    ncall = 0
    for r0, r in zip(base, recs):
        it = runs["items"].get(int(r0["frame"]))
        if it is not None:   # thresholds 0: every item is accepted
            t, d, _ = it
            ncall += 1
            assert r["osd"] == 3 and r["decoded"] == 1 and int(r["idt"]) == t
            want = G.call_message(CALLS_WITH[int(d["call"])], int(d["ngrid"]), int(d["dbm"]))
            assert r["message"].tobytes() == want.tobytes()
            x, y = r.copy(), r0.copy()
            for k in ("decoded", "idt", "message", "osd"):
                x[k] = y[k]
            assert x.tobytes() == y.tobytes()   # nothing else in the record moved
        else:
            assert r["osd"] == 0 and r.tobytes() == r0.tobytes()
    assert ncall >= len(SEEDS_CALL) + len(SEEDS_LOST)
    assert runs["wide"][1]["decoded"] == runs["base"][1]["decoded"] + ncall


def test_its_callsign_among_8_decodes_the_text(G, runs):
    recs, wide, base = runs["dflt"][0], runs["wide"][0], runs["base"][0]
    N = G.native
    for r, w, r0 in zip(recs, wide, base):
        if r["osd"]:
            assert r["osd"] == 3 and r.tobytes() == w.tobytes()
            assert CX.accepted(runs["items"][int(r["frame"])][1], NHYP, N.CALL_MIN_DEFAULT, N.CALL_GAP_DEFAULT)
        else:
            assert r.tobytes() == r0.tobytes()
            it = runs["items"].get(int(r["frame"]))
            assert it is None or not CX.accepted(it[1], NHYP, N.CALL_MIN_DEFAULT, N.CALL_GAP_DEFAULT)
    assert not recs["osd"][recs["frame"] >= NF].any()   # the signal-free frames
    assert len(SEEDS_CALL) >= 4
    for b in range(len(SEEDS_CALL)):   # recovered only by the call search
        r = recs[recs["frame"] == b]
        assert len(r) == 1 and r[0]["decoded"] == 1 and r[0]["osd"] == 3
        assert r[0]["message"].tobytes() == G.wspr_pack(TEXT).tobytes()
        assert G.unpack_message(r[0]["message"]) == (0, TEXT)
    lost = recs[(recs["frame"] >= len(SEEDS_CALL)) & (recs["frame"] < len(SEEDS_CALL) + len(SEEDS_LOST))]
    assert not lost["decoded"].any()
    fano = recs[(recs["frame"] >= len(SEEDS_CALL) + len(SEEDS_LOST)) & (recs["frame"] < NF)]
    assert fano["decoded"].all() and not fano["osd"].any()
    assert runs["dflt"][1]["decoded"] == runs["base"][1]["decoded"] + int((recs["osd"] == 3).sum())


def test_8_other_callsigns_decode_nothing(G, runs):
    N = G.native
    for _, _, d in runs["items"].values():   # the seed-picking condition, on the CPU first
        assert not CX.accepted(d, NHYP, N.CALL_MIN_DEFAULT, N.CALL_GAP_DEFAULT)
    recs = runs["other"][0]
    assert not recs["osd"].any() and recs.tobytes() == runs["base"][0].tobytes()


def test_the_list_goes_first(G, runs):
    recs, dflt = runs["both"][0], runs["dflt"][0]
    for b in range(len(SEEDS_CALL)):   # TEXT is on the list: the record is K13's
        r = recs[recs["frame"] == b]
        assert len(r) == 1 and r[0]["decoded"] == 1 and r[0]["osd"] == 2 and G.unpack_message(r[0]["message"]) == (0, TEXT)
        x, y = r[0].copy(), dflt[dflt["frame"] == b][0].copy()
        x["osd"] = y["osd"]
        assert x.tobytes() == y.tobytes()
    assert not (recs["osd"] == 3).any() or all(int(f) >= len(SEEDS_CALL) for f in recs["frame"][recs["osd"] == 3])


def test_osd_takes_only_what_the_call_search_left(runs):
    recs, dflt, base = runs["osd"][0], runs["dflt"][0], runs["base"][0]
    assert len(recs) == len(dflt)
    for r, d, r0 in zip(recs, dflt, base):
        if d["osd"] == 3:
            assert r.tobytes() == d.tobytes()   # K14 took it: K9 never saw it
        else:
            assert r["osd"] in (0, 1)
            if r["osd"] == 0:
                assert r.tobytes() == r0.tobytes()


def test_two_passes_run_and_keep_the_frame_order(runs):
    recs = runs["two"][0]
    assert (np.diff(recs["frame"]) >= 0).all() and set(recs["frame"].tolist()) <= set(range(runs["n"]))
    first = recs[recs["pass"] == 0]
    assert first.tobytes() == runs["dflt"][0].tobytes()   # the first pass is the one-pass run


def test_options_and_set_rules_through_the_pipe(G):
    pipe = G.Pipe(hop=45000, batch_frames=2, lanes=1)
    try:
        for name in ("call_min", "call_gap"):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_option(name, -1)
            assert e.value.status == -6
            pipe.set_option(name, 0)
        for bad in (["K1ABC", "K1ABC"], ["PJ4/K1ABC"], CX.random_calls(np.random.Generator(np.random.Philox(3)), 65)):
            with pytest.raises(G.UwsprError) as e:
                pipe.set_calls(bad)
            assert e.value.status == -6
        pipe.set_calls(CALLS_WITH, grids=["FN"], powers=[37])
        pipe.set_calls(["K1ABC"])
        pipe.set_calls([])
    finally:
        pipe.close()


def test_decode_wav_dicts_carry_call(G, tmp_path):
    p = str(tmp_path / "mono.wav")
    G.encode_wav(p, [(TEXT, 0, 0, 2.0)])
    plain = G.decode_wav(p, batch_frames=8)
    out = G.decode_wav(p, batch_frames=8, calls=CALLS_WITH)
    assert out and all(d["call"] in (0, 1) and d["deep"] in (0, 1) and d["osd"] in (0, 1) for d in out)
    assert all("call" in d and d["call"] == 0 for d in plain)
    assert [d for d in out if not d["call"]] == plain   # what Fano decodes is not the call search's to take


def test_python_record_split_marks_the_call_records(G, runs):
    # decode_wav's split of a record (context.record_dict), on the records of the default run and of the run with a list
    recs = runs["dflt"][0]
    for b in range(len(SEEDS_CALL)):
        d = G.context.record_dict(recs[recs["frame"] == b][0])
        assert (d["call"], d["deep"], d["osd"], d["text"], d["frame"]) == (1, 0, 0, TEXT, b)
        d = G.context.record_dict(runs["both"][0][runs["both"][0]["frame"] == b][0])
        assert (d["call"], d["deep"], d["osd"], d["text"]) == (0, 1, 0, TEXT)
    for r in recs[(recs["decoded"] == 1) & (recs["osd"] == 0)]:
        d = G.context.record_dict(r)
        assert (d["call"], d["deep"], d["osd"]) == (0, 0, 0)
