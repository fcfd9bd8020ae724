"""K15 (uwspr_track_set, uwspr_track_batch) on the GPU against tests/track_exact.py's binary64 restatement: the whole surface
at three shifts (windows off the front, inside, past fl), 1 and 70 trajectories, qf 0 and 2, both models; the pick; the
bit-equal identities; the refusals.

TOL: the largest relative distance |T_kernel - T_restated| / T_restated measured over every hypothesis of the 8 surface cases
(2 models x n in {1, 70} x qf in {0, 2}, three items each; per case 2.3e-7 .. 6.9e-7) was 6.87e-7 (profiles/track.txt);
4 x that is asserted -- the factor covers other seeds of the same binary32 accumulation -- and may not exceed 1e-4 of T: a
window off by one sample in every symbol moves T by about 4e-3 and a wrong dfreq sign by far more."""
import ctypes as C

import numpy as np
import pytest

import track_exact as TX

pytestmark = pytest.mark.gpu
TEXT = "K1ABC FN42 37"
MEASURED = 6.87e-7
TOL = 4 * MEASURED
F0, FL, HOP = 1.25, TX.FL, 3375
SHIFTS = (-300, 380, 4200)          # 4200 + 41472 > 45000: the last three symbols pass fl
MODELS = ("delay", "doppler")
# the transmission starts where a decoder's shift for it -- aligned at mid-transmission -- is SHIFTS[1]
START = {m: 2 * SHIFTS[1] - TX.truth_item(TX.TRUTH, m, SHIFTS[1])[0] for m in MODELS}


def test_tolerance_condition():
    assert TOL <= 1e-4


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sym(G):
    return G.wspr_symbols(TEXT)


@pytest.fixture(scope="module")
def grid70(G):
    g = G.track_grid(v=(0.0, 1.5, 2.5, 3.5), d=(50.0, 100.0, 200.0, 400.0), tc=(15.0, 35.0, 55.0, 75.0, 95.0, 115.0))[:70]
    assert len(g) == 70 and (2.5, 100.0, 55.0) in [tuple(r) for r in g]
    return g


@pytest.fixture(scope="module")
def frames(G, ctx):
    """frame m: the TRUTH pass rendered by the transmitter in MODELS[m] at unit gain, plus Gaussian noise of sigma 2 per
    component (seeded); frame 2: noise alone"""
    rng = np.random.Generator(np.random.Philox(0x7AC15))
    out = []
    for model in MODELS:
        sig = {"text": TEXT, "start": START[model], "f0": F0, "motion": G.track_motion(TX.TRUTH, bearing=0.4, model=model)}
        out.append(ctx.tx_baseband([sig], n=FL) + (2.0 * rng.standard_normal((FL, 2))).astype(np.float32))
    out.append((2.0 * rng.standard_normal((FL, 2))).astype(np.float32))
    return np.stack(out).astype(np.float32)


def _items(sym, model, frame=None, drift=0.0):
    m = MODELS.index(model) if frame is None else frame
    shift, f = TX.truth_item(TX.TRUTH, model, START[model], f0=F0)
    assert shift == SHIFTS[1]
    return [{"frame": m, "shift": s, "f": f, "drift": drift, "symbols": sym} for s in SHIFTS]


_cases = {}


def _case(G, ctx, frames, sym, grid70, n, qf, model):
    """-> (results, kernel surface [3, n, nf], restated surface [3, n, nf]); computed once per case"""
    key = (n, qf, model)
    if key not in _cases:
        trajs = grid70 if n == 70 else G.track_trajs([TX.TRUTH])
        items = _items(sym, model)
        ctx.track_set(trajs, qf=qf, model=model)
        res, surf = ctx.track(frames, items, surface=True)
        df, ta = TX.design(trajs, model)
        want = np.stack([TX.surface(frames[it["frame"]], it["shift"], it["f"], sym, df, ta, qf) for it in items])
        _cases[key] = (res, surf, want)
    return _cases[key]


CASES = [(n, qf, model) for model in MODELS for n in (1, 70) for qf in (0, 2)]


@pytest.mark.parametrize("n,qf,model", CASES)
def test_surface_against_the_restatement(G, ctx, frames, sym, grid70, n, qf, model):
    res, surf, want = _case(G, ctx, frames, sym, grid70, n, qf, model)
    assert surf.shape == want.shape == (3, n, 2 * qf + 1) and surf.dtype == np.float32
    assert (want > 0).all() and np.isfinite(surf).all()
    rel = np.abs(surf.astype(np.float64) - want) / want
    print("K15 surface n %d qf %d %s: largest relative distance %.3g" % (n, qf, model, rel.max()))
    assert rel.max() <= TOL, (float(rel.max()), np.unravel_index(rel.argmax(), rel.shape))
    # the things the tolerance is there to see: one sample of misalignment, the other sign of dfreq
    trajs = grid70 if n == 70 else G.track_trajs([TX.TRUTH])
    df, ta = TX.design(trajs, model)
    it = _items(sym, model)[1]
    j = [tuple(r) for r in trajs].index(TX.TRUTH)
    for wdf, wta in ((df[j:j + 1], ta[j:j + 1] + 1), (-df[j:j + 1], ta[j:j + 1])):
        wrong = TX.surface(frames[it["frame"]], it["shift"], it["f"], sym, wdf, wta, 0)[0, 0]
        assert abs(wrong - want[1, j, qf]) / want[1, j, qf] > 10 * TOL


@pytest.mark.parametrize("n,qf,model", CASES)
def test_pick_is_the_first_maximum_of_the_kernels_own_surface(G, ctx, frames, sym, grid70, n, qf, model):
    res, surf, want = _case(G, ctx, frames, sym, grid70, n, qf, model)
    nf = 2 * qf + 1
    for k in range(3):
        flat = surf[k].reshape(-1)
        assert res["best"][k] == TX.first_max(flat) == int(flat.argmax())
        assert res["t_best"][k].tobytes() == flat[res["best"][k]].tobytes()
        f = np.float32(np.float64(np.float32(_items(sym, model)[k]["f"])) + 0.0125 * (int(res["best"][k]) % nf - qf))
        assert res["f_hz"][k].tobytes() == f.tobytes()
        assert abs(want[k].max() - float(res["t_best"][k])) <= TOL * want[k].max()
        wref = TX.t_ref(frames[MODELS.index(model)], SHIFTS[k], _items(sym, model)[k]["f"], 0.0, sym)
        assert abs(wref - float(res["t_ref"][k])) <= TOL * wref
    if n == 70:   # the item that sits on the signal names the true pass, and the pass explains more than the record's line
        truth = [tuple(r) for r in grid70].index(TX.TRUTH)
        assert res["best"][1] // nf == truth and res["t_best"][1] > res["t_ref"][1]


def test_pick_ties_zero_and_nan(G, ctx, frames, sym):
    other = (3.5, 100.0, 55.0)
    items = _items(sym, "delay")[1:2]
    # a duplicated trajectory: equal bytes, the smaller index wins
    ctx.track_set([other, TX.TRUTH, TX.TRUTH, other], qf=1, model="delay")
    res, surf = ctx.track(frames, items, surface=True)
    assert surf[0, 1].tobytes() == surf[0, 2].tobytes() and surf[0, 0].tobytes() == surf[0, 3].tobytes()
    assert res["best"][0] // 3 == 1 and res["best"][0] == int(surf[0].reshape(-1).argmax())
    # an all-zero frame
    res, surf = ctx.track(np.zeros((1, FL, 2), np.float32), [dict(items[0], frame=0)], surface=True)
    assert not surf.any() and res["best"][0] == 0 and res["t_best"][0] == 0.0 and res["t_ref"][0] == 0.0
    # a NaN sample that the static trajectory reads (tau = 0: sample 10 of symbol 0) and the pass does not (its first
    # window starts tau[0] = 17 samples later): the static row is NaN, the others are what they were
    df, ta = TX.design([TX.TRUTH], "delay")
    assert ta[0, 0] > 10 and TX.design([other], "delay")[1][0, 0] > 10
    bad = frames[:1].copy()
    bad[0, SHIFTS[1] + 10] = (np.nan, 0.0)
    static = (0.0, 100.0, 0.0)
    clean_items = [dict(items[0], frame=0)]
    ctx.track_set([TX.TRUTH, static, other], qf=1, model="delay")
    clean, csurf = ctx.track(frames[:1], clean_items, surface=True)
    res, surf = ctx.track(bad, clean_items, surface=True)
    assert np.isnan(surf[0, 1]).all() and surf[0, 0].tobytes() == csurf[0, 0].tobytes() and surf[0, 2].tobytes() == csurf[0, 2].tobytes()
    assert res["best"][0] == clean["best"][0] == TX.first_max(surf[0]) and res["best"][0] // 3 == 0   # a NaN T is never moved to
    assert np.isnan(res["t_ref"][0])                                                                 # (the record's line reads it too)
    ctx.track_set([static, TX.TRUTH, other], qf=1, model="delay")
    res, surf = ctx.track(bad, clean_items, surface=True)
    assert np.isnan(surf[0, 0]).all() and not np.isnan(surf[0, 1:]).any()
    assert res["best"][0] == 0 == TX.first_max(surf[0]) and np.isnan(res["t_best"][0])                # a NaN T(0) is never left


def test_static_trajectory_is_t_ref(G, ctx, frames, sym):
    ctx.track_set([(0.0, 100.0, 0.0), TX.TRUTH], qf=2, model="delay")
    items = _items(sym, "delay") + _items(sym, "doppler")
    res, surf = ctx.track(frames, items, surface=True)
    for k in range(len(items)):
        assert surf[k, 0, 2].tobytes() == res["t_ref"][k].tobytes(), k
    # with a drift the record's line is another sum (and the hypotheses do not read drift_hz at all)
    res2, surf2 = ctx.track(frames, [dict(it, drift=1.0) for it in items], surface=True)
    assert surf2.tobytes() == surf.tobytes() and (res2["t_ref"] != res["t_ref"]).all()
    assert np.array_equal(res2["best"], res["best"])


def test_an_items_bytes_do_not_depend_on_the_batch(G, ctx, frames, sym, grid70):
    ctx.track_set(grid70[:33], qf=1, model="delay")
    items = [_items(sym, "delay")[1], _items(sym, "delay")[0], _items(sym, "doppler")[2], _items(sym, "doppler")[1],
             dict(_items(sym, "doppler")[1], shift=1000, drift=-0.5)]
    assert [it["frame"] for it in items] == [0, 0, 1, 1, 1]
    res, surf = ctx.track(frames[:2], items, surface=True)
    for k, it in enumerate(items):
        r1, s1 = ctx.track(frames[it["frame"]:it["frame"] + 1], [dict(it, frame=0)], surface=True)
        assert r1.tobytes() == res[k:k + 1].tobytes() and s1.tobytes() == surf[k:k + 1].tobytes(), k
    assert ctx.track(frames[:2], items).tobytes() == res.tobytes()      # without the surface: the same records


def test_host_device_and_in_place_frames_give_the_same_bytes(G, ctx, frames, sym, grid70):
    import torch
    ctx.track_set(grid70[:20], qf=1, model="delay")
    stream = np.concatenate([frames[0], frames[2][:HOP]])                # two frames a hop apart, read where they lie
    cut = np.stack([stream[:FL], stream[HOP:HOP + FL]])
    items = [_items(sym, "delay")[1], _items(sym, "delay", frame=1)[0], dict(_items(sym, "delay", frame=1)[2], shift=1000)]
    res, surf = ctx.track(cut, items, surface=True)
    dres, dsurf = ctx.track(torch.from_numpy(cut).to("cuda:0"), items, surface=True)
    assert dres.tobytes() == res.tobytes() and dsurf.tobytes() == surf.tobytes()
    sdev = torch.from_numpy(stream).to("cuda:0")
    torch.cuda.synchronize()
    ctx.set_frame_stride(HOP)
    try:
        for view in (G.FrameView(2, host=stream), G.FrameView(2, ptr=sdev.data_ptr())):
            vres, vsurf = ctx.track(view, items, surface=True)
            assert vres.tobytes() == res.tobytes() and vsurf.tobytes() == surf.tobytes()
    finally:
        ctx.set_frame_stride(0)


def _raw(G, c, frames, where, items, res, surf):
    arr = G.sub_items(items)
    fp = frames.data_ptr() if hasattr(frames, "data_ptr") else frames.ctypes.data
    B = frames.shape[0]
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)   # noqa: E731
    return G.native.lib().uwspr_track_batch(c.h, C.c_void_p(fp), B, where, C.c_void_p(arr.ctypes.data) if len(arr) else None, len(arr),
                                            ptr(res), ptr(surf))


def test_refusals_leave_the_outputs_alone(G, frames, sym):
    import torch
    N = G.native
    L = N.lib()
    c = G.Context()
    try:
        good = _items(sym, "delay")[:2]
        res = np.full(2, 0x55, np.uint8).repeat(16).view(N.TRACK_RESULT_DTYPE)[:2].copy()
        surf = np.full((2, 3, 3), 7.0, np.float32)
        untouched = lambda: (res.view(np.uint8) == 0x55).all() and (surf == 7.0).all()   # noqa: E731
        assert _raw(G, c, frames, N.HOST, good, res, surf) == -6 and "no trajectory set" in L.uwspr_last_error(c.h).decode()
        assert untouched()
        # sets that are refused leave no set behind, and later leave the set before in place
        tr = G.track_trajs([TX.TRUTH, (0.0, 100.0, 0.0), (1.5, 200.0, 35.0)])
        tp = C.c_void_p(tr.ctypes.data)
        badtr = G.track_trajs([TX.TRUTH, (1.0, 0.5, 0.0)])
        for args in ((tp, 0, 1, N.TX_DELAY), (tp, 4097, 1, N.TX_DELAY), (None, 3, 1, N.TX_DELAY), (tp, 3, 17, N.TX_DELAY), (tp, 3, -1, N.TX_DELAY),
                     (tp, 3, 1, N.TX_STATIC), (tp, 3, 1, 3), (C.c_void_p(badtr.ctypes.data), 2, 1, N.TX_DELAY)):
            assert L.uwspr_track_set(c.h, *args) == -6, args[1:]
        assert _raw(G, c, frames, N.HOST, good, res, surf) == -6 and untouched()
        c.track_set(tr, qf=1, model="delay")
        want, wsurf = c.track(frames, good, surface=True)
        assert L.uwspr_track_set(c.h, C.c_void_p(badtr.ctypes.data), 2, 1, N.TX_DELAY) == -6
        again, asurf = c.track(frames, good, surface=True)
        assert again.tobytes() == want.tobytes() and asurf.tobytes() == wsurf.tobytes()
        # items uwspr_subtract_batch would refuse
        s4 = sym.copy()
        s4[100] = 4
        for bad in ([dict(good[0], symbols=s4)], [dict(good[0], frame=3)], [dict(good[0], frame=-1)], [dict(good[0], frame=1), good[1]],
                    [dict(good[0], f=float("nan"))], [dict(good[0], f=2e4)], [dict(good[0], drift=float("inf"))], [dict(good[0], shift=(1 << 20) + 1)]):
            assert _raw(G, c, frames, N.HOST, bad, res, surf) == -6 and untouched()
        assert _raw(G, c, frames, 7, good, res, surf) == -6 and untouched()
        assert _raw(G, c, frames, N.HOST, good, None, surf) == -6 and untouched()
        assert L.uwspr_track_batch(c.h, None, 3, N.HOST, None, 0, None, None) == -6
        assert _raw(G, c, frames, N.HOST, [], None, None) == 0            # nothing to do is fine
        # device outputs that are no device memory, or end past their allocation
        dev = torch.from_numpy(frames).to("cuda:0")
        dres = torch.full((2 * 16,), 0x55, dtype=torch.uint8, device="cuda:0")
        dsurf = torch.full((2 * 9,), 7.0, dtype=torch.float32, device="cuda:0")
        small = C.c_void_p()   # one float short, and an allocation of its own: a tensor may lie inside a larger block of the caching allocator
        assert L.uwspr_device_alloc(4 * (2 * 9 - 1), C.byref(small)) == 0
        torch.cuda.synchronize()
        garr = G.sub_items(good)
        for where in (N.DEVICE, N.DEVICE_FRAMES):
            assert _raw(G, c, dev, where, good, res, dsurf) == -6
            assert _raw(G, c, dev, where, good, dres, surf) == -6
            assert L.uwspr_track_batch(c.h, C.c_void_p(dev.data_ptr()), 1, where, C.c_void_p(garr.ctypes.data), 2, C.c_void_p(dres.data_ptr()), small) == -6
            assert b"inside device allocations" in L.uwspr_last_error(c.h)
        c.synchronize()
        assert untouched() and (dres.cpu().numpy() == 0x55).all() and (dsurf.cpu().numpy() == 7.0).all()
        L.uwspr_device_free(small)
        # and the asynchronous form gives the host form's bytes
        assert _raw(G, c, dev, N.DEVICE, good, dres, dsurf) == 0
        c.synchronize()
        assert dres.cpu().numpy().tobytes() == want.tobytes() and dsurf.cpu().numpy().tobytes() == wsurf.tobytes()
    finally:
        c.close()


def test_closed_loop_through_the_pipe(G, ctx):
    """One DELAY-model pass at -20 dB through a Pipe(tracks=grid): the record decodes, pipe.tracks() names the true pass with
    t_best > t_ref, and the decode records are the bytes of the same pipe without tracks.  The pass, the grid and the offset
    reach were chosen without a GPU (tests/test_track.py: the restatement alone picks the truth at -20 dB)."""
    nf = 2 * TX.LOOP_QF + 1
    grid = G.track_grid(v=TX.LOOP_V, d=TX.LOOP_D, tc=TX.LOOP_TC)
    truth = [tuple(r) for r in grid].index(TX.LOOP_TRUTH)
    sig = [{"text": TEXT, "start": 375, "f0": 1.0, "motion": {"v": TX.LOOP_SLM[:2], "p": TX.LOOP_SLM[2:], "model": "delay"}}]
    x = ctx.tx_render(sig, 122 * 12000, sigma=G.tx_sigma(-20.0), seed=12, format="s16")[:, 0]

    def run(**kw):
        pipe = G.Pipe(batch_frames=8, **kw)
        try:
            pipe.push_audio(x)
            pipe.flush()
            return pipe.collect(), pipe.tracks(), pipe.stats(), pipe
        finally:
            pipe.close()
    plain, nofits, _, _ = run()
    recs, fits, st, pipe = run(tracks=grid, track_qf=TX.LOOP_QF)
    assert len(nofits) == 0 and recs.tobytes() == plain.tobytes()
    dec = [r for r in recs if r["decoded"]]
    assert len(dec) >= 1 and len(fits) == len(dec)
    for r, t in zip(dec, fits):
        assert (t["frame"], t["cand"], t["channel"], t["pass"]) == (r["frame"], r["cand"], r["channel"], r["pass"])
    hit = [t for r, t in zip(dec, fits) if G.unpack_message(r["message"])[1] == TEXT]
    assert len(hit) >= 1
    for t in hit:
        res = t["result"]
        print("closed loop: best %d (trajectory %d, truth %d), t_best %.1f, t_ref %.1f, f %.4f" % (
            res["best"], res["best"] // nf, truth, res["t_best"], res["t_ref"], res["f_hz"]))
        assert res["best"] // nf == truth and res["t_best"] > res["t_ref"]
        d = pipe.track_of(t)
        assert (d["v"], d["d"], d["tc"]) == TX.LOOP_TRUTH
    assert st["resume_s"] > 0.0
