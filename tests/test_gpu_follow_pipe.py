"""K16 in the pipe (uwspr_pipe_set_follow): the moving sources that the fine search loses, through Pipe(follow=grid).

One stream of nine 120 s frames (hop = 45000, so no frame sees its neighbour's signal): frames 0 .. 3 carry TEXT from the
receiver's grid trajectories 21 and 1 -- V = (2, -2) and (-2, -2) from p = (0, 250): closest point of approach in
mid-transmission, profiles/moving_source.txt's lost passes -- each in the "doppler" and the "delay" model, rendered by
tx_render at -20 dB as one 122 s s16 recording each (its first 120 s are the frame); frame 4 a static -20 dB signal; frames
5 .. 8 noise of the recordings' level and no signal.  The follow grid is the true pass among the five separated decoys of
tests/follow_cases.py, qf = 16, two lags, the default "doppler" model for all four recordings."""
import ctypes as C

import numpy as np
import pytest

import follow_cases as FC
import track_exact as TX

pytestmark = pytest.mark.gpu
TEXT = FC.TEXT
NREC = 120 * 12000
MOVING = [(21, "doppler"), (21, "delay"), (1, "doppler"), (1, "delay")]
SEED0 = 31                           # recording m is rendered with seed SEED0 + m
NMOV, STATIC, NFRAMES = 4, 4, 9


@pytest.fixture(scope="module")
def runs(G):
    ctx = G.Context()
    sigma = G.tx_sigma(-20.0)
    parts = []
    for m, (k, model) in enumerate(MOVING):
        sig = [{"text": TEXT, "start": FC.START, "f0": FC.F0, "motion": {"v": FC.SLM[k][:2], "p": FC.SLM[k][2:], "model": model}}]
        parts.append(ctx.tx_render(sig, 122 * 12000, sigma=sigma, seed=SEED0 + m, format="s16")[:NREC, 0])
    parts.append(ctx.tx_render([{"text": TEXT, "start": FC.START, "f0": FC.F0}], 122 * 12000, sigma=sigma, seed=SEED0 + 4, format="s16")[:NREC, 0])
    ctx.close()
    level = float(np.std(parts[0].astype(np.float64)))
    rng = np.random.Generator(np.random.Philox(0xF0110E))
    parts.append(np.rint(level * rng.standard_normal(4 * NREC + 2 * 12000)).astype(np.int16))   # (2 s more: the front-end's tail)
    x = np.concatenate(parts)
    grid, ti = FC.grid(G, 21)
    assert tuple(grid[ti]) == tuple(FC.grid(G, 1)[0][ti])          # the two passes differ in bearing alone

    def run(bad_sets=False, **kw):
        pipe = G.Pipe(hop=45000, batch_frames=NFRAMES, lanes=1, **kw)
        try:
            refused = []
            if bad_sets:   # none of these may change the set the pipe has
                N, L = G.native, G.native.lib()
                gp = C.c_void_p(grid.ctypes.data)
                fast = G.track_trajs([tuple(grid[ti]), (10.5, 100.0, 0.0)])
                for args in ((gp, 0, 99, 1, N.TX_DOPPLER), (gp, 0, 4, 7, N.TX_DOPPLER), (gp, 0, 4, 1, 9), (gp, -1, 4, 1, N.TX_DOPPLER),
                             (gp, len(grid), 17, 1, N.TX_DOPPLER), (gp, len(grid), 4, 5, N.TX_DOPPLER), (gp, len(grid), 4, 1, N.TX_STATIC),
                             (None, 3, 4, 1, N.TX_DOPPLER), (C.c_void_p(fast.ctypes.data), 2, 4, 1, N.TX_DOPPLER)):
                    refused.append(L.uwspr_pipe_set_follow(pipe.h, *args))
            pipe.push_audio(x)
            pipe.flush()
            recs = pipe.collect()
            fits = pipe.follows()
            tracks = pipe.tracks() if pipe.track_trajs is not None else None
            return {"recs": recs, "fits": fits, "stats": pipe.stats(), "of": [pipe.follow_of(t) for t in fits], "tracks": tracks, "refused": refused}
        finally:
            pipe.close()

    fkw = {"follow": grid, "follow_qf": FC.QF, "follow_lags": FC.NL}
    return {"plain": run(), "follow": run(bad_sets=True, **fkw), "combo": run(block=3, osd=2, **fkw),
            "tracks": run(tracks=grid, track_qf=8, track_model="doppler", **fkw), "grid": grid, "ti": ti}


def _text(G, r):
    return G.unpack_message(r["message"])[1]


def test_a_plain_pipe_decodes_none_of_the_moving_recordings(G, runs):
    recs = runs["plain"]["recs"]
    assert len(runs["plain"]["fits"]) == 0 and not (recs["osd"] == 4).any()
    for m in range(NMOV):
        r = recs[recs["frame"] == m]
        assert len(r) >= 1 and r["worth_a_try"].any(), m          # the signal is found ...
        assert not [1 for q in r if q["decoded"] and _text(G, q) == TEXT], m   # ... and lost
    st = recs[recs["frame"] == STATIC]
    assert [1 for q in st if q["decoded"] and _text(G, q) == TEXT and q["osd"] == 0]   # a static signal at this level never fails


def test_follow_decodes_each_recording(G, runs):
    f = runs["follow"]
    recs, fits, of = f["recs"], f["fits"], f["of"]
    truth = tuple(float(v) for v in runs["grid"][runs["ti"]])
    hit = recs[recs["osd"] == 4]
    assert len(fits) == len(hit)
    for r, t in zip(hit, fits):   # K15's door: in the order of the records that follow decoded
        assert (t["frame"], t["cand"], t["channel"], t["pass"]) == (r["frame"], r["cand"], r["channel"], r["pass"])
    for m in range(NMOV):
        mine = [(r, d) for r, d in zip(hit, of) if r["frame"] == m]
        assert len(mine) == 1, m
        r, d = mine[0]
        print("recording %d (%s): pass (%.3f, %.1f, %.1f), f %.3f Hz, lag %d, s_best %.3f, s_ref %.3f" % (
            (m, MOVING[m]) + (d["v"], d["d"], d["tc"], d["f"], d["lag"], d["s_best"], d["s_ref"])))
        assert r["decoded"] == 1 and _text(G, r) == TEXT and r["block"] == 0
        assert (d["v"], d["d"], d["tc"]) == truth and d["s_best"] > d["s_ref"] and d["s_best"] > 0.12
        assert abs(d["lag"]) <= 32 * FC.NL
    # nothing decodes on the noise frames, and the extra Fano calls are counted
    assert not recs["decoded"][recs["frame"] > STATIC].any()
    assert f["stats"]["fano_calls"] >= runs["plain"]["stats"]["fano_calls"] + NMOV
    assert f["stats"]["decoded"] == runs["plain"]["stats"]["decoded"] + len(hit)
    assert f["stats"]["resume_s"] > 0.0


def test_records_against_the_run_without_follow(runs):
    base, recs = runs["plain"]["recs"], runs["follow"]["recs"]
    assert len(base) == len(recs)
    for r0, r in zip(base, recs):
        if r0["decoded"]:      # (the static signal among them)
            assert r.tobytes() == r0.tobytes()
            continue
        x, y = r.copy(), r0.copy()
        for k in ("decoded", "idt", "message", "osd"):
            x[k] = y[k]
        assert x.tobytes() == y.tobytes()
        assert r.tobytes() == r0.tobytes() or (r["decoded"] == 1 and r["osd"] == 4)
    st = recs[recs["frame"] == STATIC]
    assert st.tobytes() == base[base["frame"] == STATIC].tobytes() and st["decoded"].any()


def test_refused_sets_change_nothing(runs):
    assert runs["follow"]["refused"] == [-6] * 9
    # (the run that met them is the one test_follow_decodes_each_recording reads: the set it was opened with decoded)


def test_follow_block_and_osd_never_share_a_record(G, runs):
    recs = runs["combo"]["recs"]
    assert not ((recs["block"] != 0) & (recs["osd"] != 0)).any()
    assert set(recs["osd"].tolist()) <= {0, 1, 4}
    # "block" comes first: what it leaves, follow takes; every moving recording is decoded by one of the two, to the text
    for m in range(NMOV):
        r = [q for q in recs[recs["frame"] == m] if q["decoded"] and _text(G, q) == TEXT]
        assert len(r) == 1 and (r[0]["block"] in (2, 3)) != (r[0]["osd"] == 4), m
    assert len(runs["combo"]["fits"]) == int((recs["osd"] == 4).sum())


def test_a_track_item_carries_the_followers_shift_and_frequency(runs):
    """K15's f_hz is its item's f plus 0.0125 q, |q| <= 8: within 0.1 Hz of the follower's f, which lies more than 0.5 Hz
    from the f the fine search held the record at (the follower's own offset says so)"""
    t = runs["tracks"]
    recs, tracks, fits = t["recs"], t["tracks"], t["fits"]
    assert recs.tobytes() == runs["follow"]["recs"].tobytes()
    dec = recs[recs["decoded"] == 1]
    assert len(tracks) == len(dec) and len(fits) == int((dec["osd"] == 4).sum()) == NMOV
    nf, nlg = 2 * FC.QF + 1, 2 * FC.NL + 1
    k = 0
    for r, tr in zip(dec, tracks):
        assert (tr["frame"], tr["cand"]) == (r["frame"], r["cand"])
        if r["osd"] != 4:
            continue
        fol = fits[k]["result"]
        k += 1
        q = (int(fol["best"]) // nlg) % nf - FC.QF
        assert abs(q) * 375.0 / 2048.0 > 0.5
        assert abs(float(tr["result"]["f_hz"]) - float(fol["f_hz"])) <= 0.0125 * 8 + 1e-6
        assert tr["result"]["t_best"] > tr["result"]["t_ref"]
