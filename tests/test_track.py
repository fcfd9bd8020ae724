"""K15 without a GPU: the host-side design against its binary64 restatement (tests/track_exact.py), the (v, d, tc) model
against the receiver's straight-line model, the restated score on a transmission synthesised in numpy from the header's
transmit formulas, the grid helper, the refusals that need no device and the ABI bookkeeping."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_exact as TX

TEXT = "K1ABC FN42 37"


def _grid(G):
    return G.track_grid(v=TX.GRID_V, d=TX.GRID_D, tc=TX.GRID_TC)


def test_design_equals_the_restatement(G):
    """tau exactly, dfreq to the bit: every operation of the stated order is a correctly rounded binary64 one on both sides"""
    rng = np.random.Generator(np.random.Philox(0x715))
    extra = [(0.0, 1.0, 0.0), (10.0, 1.0, 55.296), (10.0, 1e6, -1e4), (10.0, 1.0, 0.0), (10.0, 1.0, 110.592), (0.3, 7.5, 1e4)]
    extra += [(float(rng.uniform(0, 10)), float(10 ** rng.uniform(0, 6)), float(rng.uniform(-200, 300))) for _ in range(200)]
    trajs = np.concatenate([_grid(G), G.track_trajs(extra)])
    for model in ("delay", "doppler"):
        for cf in (1500.0, 1234.0):
            df, ta = G.track_design(trajs, model=model, cf=cf)
            wdf, wta = TX.design(trajs, model, cf)
            assert ta.dtype == np.int32 and np.array_equal(ta, wta), model
            assert np.array_equal(df.view(np.int64), wdf.view(np.int64)), (model, cf, float(np.abs(df - wdf).max()))
            assert np.abs(ta).max() <= 139
            if model == "doppler":
                assert not ta.any()
    assert np.abs(G.track_design([(10.0, 1.0, 0.0)])[1]).max() == 138      # the bound the kernel's window is made for
    df, ta = G.track_design([(0.0, 30.0, 0.0)])
    assert not df.any() and not ta.any()


def test_model_is_the_straight_line_model(G):
    """Over the receiver's 125 trajectories and the 111 whole seconds K3 evaluates plus the 162 symbol centres,
    track_doppler(track_from_slm(.)) against slm_drift: the largest difference measured is 8.9e-16 Hz (a few ulp of
    binary64 at 2 Hz -- both sides are binary64; the reference's own float arithmetic rounds at 1.2e-7 relative); 4 x that
    is asserted.  The radial passes of the grid (V1 = 0) have d = 0, which from_slm returns and the set refuses."""
    slm = G.slm_trajectories()
    tr = G.track_from_slm(slm)
    t = np.concatenate([np.arange(111, dtype=np.float64), TX.T_SYM])
    got = G.track_doppler(tr, t)
    want = G.slm_drift(slm[:, None, :], t[None, :])
    worst = float(np.abs(got - want).max())
    print("track_doppler vs slm_drift: largest difference %.3g Hz" % worst)
    assert worst <= 4 * 8.9e-16
    assert np.allclose(tr["v"], np.hypot(slm[:, 0], slm[:, 1]))
    moving = tr["v"] > 0
    assert np.allclose(tr["d"][moving], np.abs(slm[moving, 0] * slm[moving, 3] - slm[moving, 1] * slm[moving, 2]) / tr["v"][moving])
    assert (tr["d"][~moving] == np.hypot(slm[~moving, 2], slm[~moving, 3])).all() and not tr["tc"][~moving].any()
    # t_first moves the CPA time and nothing else
    later = G.track_from_slm(slm, t_first=20.0)
    assert np.array_equal(later["v"], tr["v"]) and np.array_equal(later["d"], tr["d"])
    assert np.allclose(later["tc"][moving], tr["tc"][moving] - 20.0)
    # and the motion dict closes the loop: its SLM parameters are the trajectory again
    for bearing in (0.0, 0.7, -2.0):
        m = G.track_motion(TX.TRUTH, bearing=bearing)
        back = G.track_from_slm(m["v"] + m["p"])[0]
        assert np.allclose([back["v"], back["d"], back["tc"]], TX.TRUTH, rtol=1e-12), bearing
        assert m["model"] == "delay" and m["t"] == 0.0


@pytest.fixture(scope="module")
def synth_case(G):
    sym = G.wspr_symbols(TEXT)
    grid = _grid(G)
    truth = int(np.flatnonzero((grid["v"] == TX.TRUTH[0]) & (grid["d"] == TX.TRUTH[1]) & (grid["tc"] == TX.TRUTH[2]))[0])
    return sym, grid, truth


@pytest.mark.parametrize("model", ["doppler", "delay"])
def test_restatement_finds_the_truth_on_a_numpy_synthesis(G, synth_case, model):
    sym, grid, truth = synth_case
    start, f0, qf = 380, 1.25, 2
    frame = TX.synth(sym, TX.TRUTH, model, start, f0=f0)
    shift, f = TX.truth_item(TX.TRUTH, model, start, f0=f0)
    df, ta = TX.design(grid, model)
    T = TX.surface(frame, shift, f, sym, df, ta, qf)
    best = TX.first_max(T)
    assert best == truth * (2 * qf + 1) + qf, (best, truth, T[truth], T.max())
    others = np.delete(T.max(axis=1), truth)
    assert T[truth, qf] > 1.02 * others.max()                       # the decoys are separated, not near ties
    assert T[truth, qf] > 0.9 * TX.N                                # nearly the whole energy is collected
    assert T[truth, qf] > TX.t_ref(frame, shift, f, 0.0, sym)       # and the linear model of the record collects less
    if model == "delay":   # a DELAY signal scored with Doppler alone: the windows slide off at both ends
        dfd, tad = TX.design(grid, "doppler")
        assert T[truth, qf] > TX.surface(frame, shift, f, sym, dfd[truth:truth + 1], tad[truth:truth + 1], 0)[0, 0]


def test_pick_rule_of_the_restatement():
    nan = float("nan")
    assert TX.first_max([1.0, 3.0, 3.0, 2.0]) == 1
    assert TX.first_max([nan, 3.0, 5.0]) == 0
    assert TX.first_max([1.0, nan, 5.0, nan, 5.0]) == 2
    assert TX.first_max([0.0, 0.0]) == 0


def test_track_grid(G):
    g = _grid(G)
    assert len(g) == 1 + 3 * 3 * 3 and g.dtype == G.native.TRACK_TRAJ_DTYPE
    assert tuple(g[0]) == (0.0, 50.0, 0.0) and tuple(g[1]) == (1.5, 50.0, 35.0) and tuple(g[2]) == (1.5, 50.0, 55.0)
    assert tuple(g[-1]) == (3.5, 200.0, 75.0)
    assert len(G.track_grid(v=[0.0], d=[10.0, 20.0], tc=[0.0, 1.0, 2.0])) == 1
    assert len(G.track_grid(v=2.0, d=100.0, tc=[0.0, 1.0])) == 2
    assert len(G.track_grid(v=np.linspace(1, 8, 16), d=np.linspace(10, 1000, 16), tc=np.linspace(0, 110, 16))) == 4096
    with pytest.raises(ValueError):
        G.track_grid(v=np.linspace(0, 8, 17), d=np.linspace(10, 1000, 16), tc=np.linspace(0, 110, 16))   # 1 + 4096
    with pytest.raises(ValueError):
        G.track_grid(v=[1.0], d=[], tc=[0.0])


def test_refusals_that_need_no_device(G):
    N = G.native
    L = N.lib()
    for bad in [(-0.1, 100.0, 0.0), (10.5, 100.0, 0.0), (1.0, 0.5, 0.0), (1.0, 2e6, 0.0), (1.0, 100.0, 1.1e4), (float("nan"), 100.0, 0.0),
                (1.0, float("inf"), 0.0), (1.0, 100.0, float("nan"))]:
        with pytest.raises(N.UwsprError) as e:
            G.track_design([TX.TRUTH, bad])
        assert e.value.status == -6, bad
    for kw in ({"model": "static"}, {"model": 7}, {"cf": 0.0}, {"cf": float("nan")}):
        with pytest.raises(N.UwsprError):
            G.track_design([TX.TRUTH], **kw)
    with pytest.raises(N.UwsprError):
        G.track_design([])
    # a refused design writes nothing
    tr = G.track_trajs([TX.TRUTH, (11.0, 100.0, 0.0)])
    df, ta = np.full((2, 162), 7.0), np.full((2, 162), 7, np.int32)
    assert L.uwspr_track_design(C.c_void_p(tr.ctypes.data), 2, N.TX_DELAY, 1500.0, C.c_void_p(df.ctypes.data), C.c_void_p(ta.ctypes.data)) == -6
    assert (df == 7.0).all() and (ta == 7).all()
    assert L.uwspr_track_design(C.c_void_p(tr.ctypes.data), 1, N.TX_DELAY, 1500.0, None, C.c_void_p(ta.ctypes.data)) == -6
    with pytest.raises(N.UwsprError):
        G.track_from_slm((1.0, float("nan"), 0.0, 50.0))
    assert L.uwspr_track_from_slm(1.0, 0.0, 0.0, 50.0, 0.0, None) == -6
    # no context, no set, no batch
    assert L.uwspr_track_set(None, C.c_void_p(tr.ctypes.data), 1, 4, N.TX_DELAY) == -6
    assert L.uwspr_track_batch(None, None, 1, N.HOST, None, 0, None, None) == -6


def test_abi_bookkeeping(G):
    N = G.native
    hdr = open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read()
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert int(m.group(1)) == 6
    for name in ("uwspr_track_design", "uwspr_track_from_slm", "uwspr_track_set", "uwspr_track_batch"):
        assert name in m.group(2), name
        assert name in N.ABI_SYMBOLS and hasattr(N.lib(), name)
    assert "k15_track.hip" in N.SOURCES
    assert N.TRACK_TRAJ_DTYPE.itemsize == 24 and N.TRACK_RESULT_DTYPE.itemsize == 16 and N.SUB_ITEM_DTYPE.itemsize == 180


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_finds_the_loop_pass_at_minus_20_db(G, seed):
    """The pass, the grid and the offset reach of tests/test_gpu_track.py's closed loop, chosen here: at -20 dB, from an item
    a decoder might hand over (0.06 Hz and 3 samples off), the restatement alone picks the truth."""
    sym = G.wspr_symbols(TEXT)
    grid = G.track_grid(v=TX.LOOP_V, d=TX.LOOP_D, tc=TX.LOOP_TC)
    tr = G.track_from_slm(TX.LOOP_SLM)[0]
    assert np.allclose([tr["v"], tr["d"], tr["tc"]], TX.LOOP_TRUTH, rtol=1e-14)
    truth = int(np.flatnonzero((grid["v"] == TX.LOOP_TRUTH[0]) & (grid["d"] == TX.LOOP_TRUTH[1]) & (grid["tc"] == TX.LOOP_TRUTH[2]))[0])
    rng = np.random.Generator(np.random.Philox(seed))
    frame = TX.synth(sym, TX.LOOP_TRUTH, "delay", 375, f0=1.0) + (TX.SIGMA_M20 * rng.standard_normal((TX.FL, 2))).astype(np.float32)
    shift, f = TX.truth_item(TX.LOOP_TRUTH, "delay", 375, f0=1.0)
    df, ta = TX.design(grid, "delay")
    T = TX.surface(frame, shift + 3, f + 0.06, sym, df, ta, TX.LOOP_QF)
    assert TX.first_max(T) // (2 * TX.LOOP_QF + 1) == truth, (TX.first_max(T), truth)
    assert T.max() > TX.t_ref(frame, shift + 3, f + 0.06, 0.0, sym)
