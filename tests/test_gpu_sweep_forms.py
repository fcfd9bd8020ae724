"""Every instantiation the sweep launchers can choose -- k4_tonecorr<1|2|4>, the wave and the lanes fold, k4_grid<NL>
at every NL and every wavefronts-per-workgroup value, and the grid's fall-back to the flat kernel -- against the CPU
oracle at sizes the oracle covers in full.  Context.launch_forms() (host-side counters where the launchers choose)
proves that the form a test forces is the one that ran: an option that were ignored could not pass.

Comparisons with the oracle are exact: `sync` by its four bytes, soft symbols by bytes.  One case needs a rule of its
own.  uwspr_sync_sweep returns the metric ss / totp of each hypothesis (cc:226); the oracle's call returns the best-of
value of cc:227-231, which starts at -1e30 and moves on `>` alone.  Where the metric is NaN (a NaN sample in a window,
or no sample inside the frame: 0 / 0) the comparison is false and the oracle keeps -1e30 -- so for a live hypothesis
"the GPU's metric is NaN" must hold exactly where the oracle answers -1e30, whatever the NaN's sign and payload (x86
and the GPU differ in those); the symbol bytes (all zero there, on both sides) are still compared.
"""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

NSYM = 162
NP = 45000            # the fine search's sample bound (cc:92)
DEAD = np.float32(-1e30)

# 3528 is the last lag with every window inside np; 0 excludes sample 0; 45000 and -41500 lie wholly outside
EDGE_LAGS = (-300, -255, -1, 0, 1, 368, 3527, 3528, 3529, 3600, 5000, 45000, -41500)
EDGE_DEAD = (0, 40, 81, 82, 83, 120, 162)          # frame = -1: both ends, a run of three, singles between live ones
EDGE_NONLINEAR = (5, 20, 33, 57, 90, 130, 150)
EDGE_DEN0 = 57                                     # p1 = p2 = 0: the den == 0 branch of slmFrequencyDrift
NAN_FRAME = 4
NAN_SAMPLE = 368 + 256 * 80 + 100                  # inside symbol 80 of a hypothesis at lag 368
EDGE_ON_NAN_FRAME = {25: 368, 26: 0, 60: 3600, 100: 45000, 141: 1}
DRIFTS = (0.0, 0.5, -0.5, 2.0, -2.0)


def hyp_dtype():
    from gr_uwspr_amd import native
    return native.HYP_DTYPE


def edge_hyps():
    """The edge list: H = 163 (163 * 162 = 26 406 pairs: a multiple of neither 16, 32 nor 64), fixed seed."""
    rng = np.random.default_rng(0xED6E)
    H = 163
    hy = np.zeros(H, hyp_dtype())
    hy["frame"] = rng.integers(0, 4, H)
    lag = rng.integers(-300, 3701, H)
    pick = rng.random(H) < 0.4
    lag[pick] = rng.choice(EDGE_LAGS, int(pick.sum()))
    lag[1:1 + len(EDGE_LAGS)] = EDGE_LAGS            # every edge lag at least once, on a frame without NaN
    hy["lag"] = lag
    hy["f0"] = rng.uniform(-8.0, 8.0, H).astype(np.float32)
    hy["drift"] = rng.choice(DRIFTS, H).astype(np.float32)
    for q in EDGE_NONLINEAR:
        hy[q]["m_type"] = 1
        hy[q]["drift"] = 0.0
        hy[q]["V1"] = float(rng.integers(-2, 3)); hy[q]["V2"] = float(rng.integers(-2, 3))
        hy[q]["p1"] = 0; hy[q]["p2"] = int(rng.choice([50, 250, 450, 650, 850]))
    hy[EDGE_DEN0]["V1"] = 1.0; hy[EDGE_DEN0]["V2"] = -2.0; hy[EDGE_DEN0]["p1"] = 0; hy[EDGE_DEN0]["p2"] = 0
    for q, lg in EDGE_ON_NAN_FRAME.items():
        hy[q]["frame"] = NAN_FRAME; hy[q]["lag"] = lg
    hy["frame"][list(EDGE_DEAD)] = -1
    return hy


def wave_classes(hy, T):
    """The flat kernel's mapping, restated from the header comment of k4_tonecorr.hip: pairs g = 162 h + i are
    flattened, wavefront w covers pairs [16 T w, 16 T (w + 1)) and hypothesis = pair // 162.  -> Counter of the classes
    of wavefront the list contains."""
    ppw = 16 * T
    total = hy.size * NSYM
    live = hy["frame"] >= 0
    out = collections.Counter()
    for w in range((total + ppw - 1) // ppw):
        g = np.arange(w * ppw, min((w + 1) * ppw, total))
        h, i = g // NSYM, g % NSYM
        nb = hy["lag"][h].astype(np.int64) + 256 * i
        inside = (nb > 0) & (nb + 255 < NP)            # cc:205: every sample of the window is used
        if g.size < ppw:
            out["partial last wavefront"] += 1
        if live[h].all() and inside.all():
            out["every window interior"] += 1
        if (live[h] & ~inside).any():
            out["an edge window"] += 1
        if h[0] != h[-1]:
            assert h[-1] == h[0] + 1                   # 162 > 64 >= pairs per wavefront: at most two hypotheses
            out[("live" if live[h[0]] else "dead") + " then " + ("live" if live[h[-1]] else "dead")] += 1
            # `interior` is one vote of the wavefront: here one hypothesis' windows lose it for the other's
            if live[h].all() and inside[h == h[0]].all() != inside[h == h[-1]].all():
                out["interior beside edge"] += 1
    return out


WAVE_CLASSES = ("every window interior", "an edge window", "live then live", "dead then live", "live then dead",
                "dead then dead", "partial last wavefront", "interior beside edge")


def test_edge_list_holds_every_class_of_wavefront():
    """No GPU: the edge list is what the GPU tests below assume, for every T the flat kernel has."""
    hy = edge_hyps()
    assert hy.size == 163 and all((hy.size * NSYM) % n for n in (16, 32, 64))
    live = hy["frame"] >= 0
    clean = live & (hy["frame"] != NAN_FRAME)
    assert set(EDGE_LAGS) <= set(hy["lag"][clean].tolist())
    assert set(np.flatnonzero(~live).tolist()) == set(EDGE_DEAD)
    assert {0, 162} <= set(EDGE_DEAD) and {81, 82, 83} <= set(EDGE_DEAD)
    assert live[39] and live[41] and live[119] and live[121]           # single dead entries between live ones
    assert set(hy["drift"][clean & (hy["m_type"] == 0)].tolist()) == set(DRIFTS)
    assert np.abs(hy["f0"]).max() <= 8 and hy["f0"].min() < -6 and hy["f0"].max() > 6
    nl = hy[live & (hy["m_type"] == 1)]
    assert nl.size >= 5 and ((nl["p1"] == 0) & (nl["p2"] == 0)).sum() == 1 and ((nl["p2"] != 0).sum() >= 4)
    on_nan = hy[hy["frame"] == NAN_FRAME]
    assert on_nan.size == len(EDGE_ON_NAN_FRAME) and 368 in on_nan["lag"]
    assert 368 + 256 * 80 <= NAN_SAMPLE < 368 + 256 * 81
    for T in (1, 2, 4):
        got = wave_classes(hy, T)
        for k in WAVE_CLASSES:
            assert got[k] >= 1, (T, k, dict(got))
    # the prefix of 162 (test a) ends in a LIVE partial wavefront for every T; the lanes-fold prefixes (test b) cover
    # nh = 1, 2, 63 (clamped tail), 64, 64 + 1, 128 + 1 and 128 + 35, with nh * 162 = 2 mod 4 for the odd ones
    assert live[161] and all((162 * NSYM) % n for n in (16, 32, 64))
    assert [(n % 64 or 64) for n in PREFIXES] == [1, 2, 63, 64, 1, 1, 35]
    assert all(clean[n] for n in PREFIXES if n < hy.size)      # the row behind each prefix holds symbols of its own
    assert all((nh * NSYM) % 4 == (2 if nh % 2 else 0) for nh in (1, 2, 63, 64, 35))


PREFIXES = (1, 2, 63, 64, 65, 129, 163)

# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def frames(G):
    """the parity file's four frames, and a fifth: frame 0 with one NaN sample"""
    f = G.synth.make_frames(4, seed=0xC0FFEE, snr_db=-20.0)
    f = np.concatenate([f, f[:1]])
    f[NAN_FRAME, NAN_SAMPLE, 0] = np.nan
    return f


@pytest.fixture(scope="module")
def vec():
    return np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))


def oracle_entry(oracle, frames, h):
    """(sync as float32, symbols[162]) of one live hypothesis: the call test_sync_sweep_edges makes"""
    cand = np.zeros(1, oracle.CAND_DTYPE)[0]
    cand["m_type"] = h["m_type"]; cand["V1"] = h["V1"]; cand["V2"] = h["V2"]
    cand["p1"] = h["p1"]; cand["p2"] = h["p2"]
    s, _, _, y = oracle.sync_and_demodulate(cand, 1500, frames[h["frame"]], float(h["f0"]), 0, 0,
                                            0.0, int(h["lag"]), 0, 0, 1, float(h["drift"]), 50, 2)
    return np.float32(s), y


def assert_equals_oracle(oracle, frames, hy, sync, sym, idx=None, ref=None):
    """Entries idx (default: all) of a sweep's output against the oracle, exactly; ref: {index: oracle_entry} made
    earlier.  -> the number of entries whose metric is NaN."""
    nnan = 0
    for q in (range(hy.size) if idx is None else idx):
        h = hy[q]
        if h["frame"] < 0:
            assert sync[q].tobytes() == DEAD.tobytes() and not sym[q].any(), q
            continue
        s, y = ref[q] if ref is not None else oracle_entry(oracle, frames, h)
        if np.isnan(sync[q]) or s.tobytes() == DEAD.tobytes():
            assert np.isnan(sync[q]) and s.tobytes() == DEAD.tobytes(), (q, sync[q], s)   # (module docstring)
            nnan += 1
        else:
            assert sync[q].tobytes() == s.tobytes(), (q, sync[q], s)
        assert (sym[q] == y).all(), q
    return nnan


@pytest.fixture(scope="module")
def edge_ref(oracle, frames):
    hy = edge_hyps()
    return {q: oracle_entry(oracle, frames, hy[q]) for q in range(hy.size) if hy[q]["frame"] >= 0}


def nonzero(forms):
    return {k: v for k, v in forms.items() if v}


def delta(after, before):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("k4_t", [1, 2, 3, 4])
def test_flat_and_fold_forms_on_the_edge_list(G, oracle, frames, edge_ref, k4_t, lanes):
    """a. k4_tonecorr<T> x fold form, all 163 entries against the oracle ("k4_t" = 3 is `by size`: T = 1 here)."""
    hy = edge_hyps()
    c = G.Context(options={"k4_t": k4_t, "k5_lanes": lanes})
    try:
        assert nonzero(c.launch_forms()) == {}
        sync, sym = c.sync_sweep(frames, hy, soft=True)
        hard, none = c.sync_sweep(frames, hy, soft=False)
        s162, y162 = c.sync_sweep(frames, hy[:162], soft=True)     # ends in a live, partial wavefront
        forms = nonzero(c.launch_forms())
    finally:
        c.close()
    nnan = assert_equals_oracle(oracle, frames, hy, sync, sym, ref=edge_ref)
    # wholly outside (0 / 0) or on the NaN sample; lag 3600 on the NaN frame still reads the sample
    expect_nan = [q for q in range(163) if hy[q]["frame"] >= 0 and
                  (hy[q]["lag"] in (45000, -41500) or hy[q]["frame"] == NAN_FRAME)]
    assert nnan == len(expect_nan) >= 7 and all(np.isnan(sync[q]) for q in expect_nan)
    dead = hy["frame"] < 0
    assert dead.sum() == 7 and (sync[dead].view(np.uint32) == DEAD.view(np.uint32)).all() and not sym[dead].any()
    assert none is None and hard.tobytes() == sync.tobytes()
    assert s162.tobytes() == sync[:162].tobytes() and y162.tobytes() == sym[:162].tobytes()
    fold = "fold_lanes" if lanes else "fold_wave"
    assert forms == {"flat_t%d" % (1 if k4_t == 3 else k4_t): 3, fold: 3, fold + "_soft": 2}


@pytest.mark.gpu
def test_lanes_fold_tails(G, oracle, frames, edge_ref):
    """b. Prefixes of the edge list whose last workgroup of the lanes fold holds 1, 2, 63, 64, 1, 1 and 35 hypotheses
    (the clamped tail; nh * 162 = 2 mod 4 for odd nh: the byte tail of the 4-byte store path): lanes form = wave form
    = oracle, and nothing beyond the call's H is touched: neither in the caller's arrays (0xAA before the call) nor in
    the context's own buffers, which the fold writes and the results are copied from (uwspr_debug_sweep_outputs: the
    rows behind H still hold, byte for byte, what the call over all 163 left there)."""
    hy = edge_hyps()
    L = G.native.lib()
    L.uwspr_debug_sweep_outputs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.uwspr_debug_sweep_outputs.restype = C.c_int
    fr = np.ascontiguousarray(frames, np.float32)
    outs = {}
    for lanes in (1, 0):
        c = G.Context(options={"k5_lanes": lanes})
        try:
            full_sync, full_sym = c.sync_sweep(frames, hy, soft=True)      # sizes the context's buffers for 163 rows
            # (a store past a tail would bring zeros -- the bytes of a lane without a hypothesis -- or stale LDS)
            assert all(full_sym[n, :2].all() for n in PREFIXES if n < hy.size)
            for n in PREFIXES:
                for soft in (True, False):
                    sync = np.full(n + 3, 0xAAAAAAAA, np.uint32).view(np.float32)
                    sym = np.full((n + 3, NSYM), 0xAA, np.uint8)
                    h = np.ascontiguousarray(hy[:n])
                    rc = L.uwspr_sync_sweep(c.h, C.c_void_p(fr.ctypes.data), fr.shape[0], C.c_void_p(h.ctypes.data), n,
                                            G.native.HOST, C.c_void_p(sync.ctypes.data),
                                            C.c_void_p(sym.ctypes.data) if soft else None)
                    assert rc == 0, (lanes, n, soft)
                    assert (sync[n:].view(np.uint32) == 0xAAAAAAAA).all() and (sym[n if soft else 0:] == 0xAA).all(), (lanes, n)
                    outs[lanes, n, soft] = (sync[:n].copy(), sym[:n].copy())
                    if n < hy.size:
                        behind_sync = np.zeros(hy.size - n, np.float32)
                        behind_sym = np.zeros((hy.size - n, NSYM), np.uint8)
                        assert L.uwspr_debug_sweep_outputs(c.h, n, hy.size - n, C.c_void_p(behind_sync.ctypes.data),
                                                           C.c_void_p(behind_sym.ctypes.data)) == 0
                        assert behind_sync.tobytes() == full_sync[n:].tobytes(), (lanes, n, soft)
                        assert behind_sym.tobytes() == full_sym[n:].tobytes(), (lanes, n, soft)
            scratch = np.zeros((hy.size + 1, NSYM), np.uint8)
            assert L.uwspr_debug_sweep_outputs(c.h, 0, hy.size + 1, None, C.c_void_p(scratch.ctypes.data)) != 0   # past the buffer
            forms = nonzero(c.launch_forms())
        finally:
            c.close()
        fold = "fold_lanes" if lanes else "fold_wave"
        assert forms == {"flat_t1": 2 * len(PREFIXES) + 1, fold: 2 * len(PREFIXES) + 1, fold + "_soft": len(PREFIXES) + 1}
    for n in PREFIXES:
        sync, sym = outs[1, n, True]
        assert_equals_oracle(oracle, frames, hy[:n], sync, sym, ref=edge_ref)
        for lanes, soft in ((0, True), (1, False), (0, False)):
            assert outs[lanes, n, soft][0].tobytes() == sync.tobytes(), (lanes, n, soft)
        assert outs[0, n, True][1].tobytes() == sym.tobytes(), n


FORCED_SCHEDULES = (
    {"sched": 0, "stage_kernels": 0, "k4_t": 2},
    {"sched": 0, "stage_kernels": 0, "k4_t": 4},
    {"sched": 0, "k4_t": 4},
    {"sched": 0, "k5_lanes": 1},
    {"sched": 0, "stage_kernels": 0, "reuse": 0, "phasor_tables": 0, "k4_t": 4, "k5_lanes": 1},
)


def check_schedule_forms(opts, forms):
    """what a staged demod_batch under `opts` must have launched, and must not have"""
    t = opts.get("k4_t", 1)
    for k in (1, 2, 4):
        assert (forms["flat_t%d" % k] > 0) == (k == t), (opts, forms)
    if opts.get("stage_kernels", 1) == 0:
        assert forms["flat_t%d" % t] == 6                       # the flat kernel for every stage
    lanes = opts.get("k5_lanes", 0) == 1
    assert forms["fold_lanes"] == forms["fold_lanes_soft"] == forms["fold_lanes_pwin"] == (1 if lanes else 0), (opts, forms)
    assert forms["fold_wave"] == forms["fold_wave_soft"] == forms["fold_wave_pwin"] == (0 if lanes else 1), (opts, forms)


@pytest.mark.gpu
def test_schedule_through_the_forced_forms(G, oracle, frames, vec):
    """c. The staged schedule with T = 2 / 4 and with the lanes fold (stage 5: `pwin`, per_slot = 17) on the parity
    vectors' candidates and on test_schedule_forms_on_random_candidates' set (its drifting linear candidates send S0
    and S2 of the default staged form through the flat kernel with `taken` and `skip_pairs`): the fused kernel's
    bytes; a sample of the records against the oracle."""
    from test_gpu_parity import RANDOM_CANDIDATE_SAMPLE, random_candidates
    vcands = [vec["cands"][b, :int(vec["npk"][b])] for b in range(4)]
    rframes, rcands, rper = random_candidates(G, oracle)
    sets = ((frames[:4], vcands, max(len(c) for c in vcands)), (rframes, rcands, rper))
    base = G.Context(options={"sched": 1})
    try:
        want = [base.demod_batch(f, c, max_per_frame=per) for f, c, per in sets]
        assert nonzero(base.launch_forms()) == {}               # the fused kernel goes through none of the launchers
    finally:
        base.close()
    for opts in FORCED_SCHEDULES:
        for (f, c, per), w in zip(sets, want):
            ctx = G.Context(options=opts)
            try:
                got = ctx.demod_batch(f, c, max_per_frame=per)
                forms = ctx.launch_forms()
            finally:
                ctx.close()
            assert got.tobytes() == w.tobytes(), opts
            check_schedule_forms(opts, forms)
    assert (want[0][:, 0]["symbols"] == vec["demod_symbols"]).all()
    for b, j in RANDOM_CANDIDATE_SAMPLE:
        d = oracle.demod_candidate(rcands[b][j], 1500, rframes[b])
        o = want[1][b, j]
        assert int(o["shift1"]) == d["shift1"] and int(o["worth_a_try"]) == d["worth_a_try"], (b, j)
        for k in ("f1", "drift1", "sync1"):
            assert np.float32(o[k]).tobytes() == np.float32(d[k]).tobytes(), (b, j, k)
        if d["worth_a_try"]:
            assert (o["symbols"] == d["symbols"]).all(), (b, j)
    # the default staged form on the random set: its flat launches are the ones with `taken` (S0) and `skip_pairs` (S2)
    ctx = G.Context(options={"sched": 0, "k4_t": 4})
    try:
        ctx.demod_batch(rframes, rcands, max_per_frame=rper)
        assert nonzero(ctx.launch_forms()) == {"flat_t4": 2, "fold_wave": 1, "fold_wave_soft": 1, "fold_wave_pwin": 1}
    finally:
        ctx.close()


@pytest.mark.gpu
def test_lazy_tries_through_t4_and_the_lanes_fold(G, frames, vec):
    """c, lazy: stage 5 on the k wanted tries only (k4_tonecorr<4> on few, unrelated lags; the lanes fold with
    per_slot = k < 17), then uwspr_demod_resume -- test_lazy_tries_and_resume_equal_the_eager_schedule's checks."""
    cands = [vec["cands"][b, :int(vec["npk"][b])] for b in range(4)]
    per = max(len(c) for c in cands)
    base = G.Context(options={"sched": 1})
    try:
        fused = base.demod_batch(frames[:4], cands, max_per_frame=per)
    finally:
        base.close()
    c = G.Context(options={"sched": 0, "k4_t": 4, "k5_lanes": 1})
    try:
        eager = c.demod_batch(frames[:4], cands, max_per_frame=per)
        assert eager.tobytes() == fused.tobytes()
        for k in (1, 3):
            c.set_tries(k)
            before = c.launch_forms()
            lazy = c.demod_batch(frames[:4], cands, max_per_frame=per)
            # S0 and S2 (`taken`, `skip_pairs`) and the lazy S5 through the flat kernel; the final fold in lanes form
            assert delta(c.launch_forms(), before) == {"flat_t4": 3, "fold_lanes": 1, "fold_lanes_soft": 1, "fold_lanes_pwin": 1}
            for f in ("f1", "drift1", "sync1", "shift1", "worth_a_try"):
                assert lazy[f].tobytes() == eager[f].tobytes()
            assert lazy["symbols"][:, :, :k].tobytes() == eager["symbols"][:, :, :k].tobytes()
            assert lazy["jig_sync"][:, :, :k].tobytes() == eager["jig_sync"][:, :, :k].tobytes()
            assert lazy["jig_rms"][:, :, :k].tobytes() == eager["jig_rms"][:, :, :k].tobytes()
            assert not lazy["symbols"][:, :, k:].any() and not lazy["jig_sync"][:, :, k:].any()
            need = np.zeros((4, per), np.uint8)
            need[1, :] = 1
            need[3, 0] = 1
            res = c.demod_resume(frames[:4], need, None, max_per_frame=per)
            for b in range(4):
                for j in range(per):
                    want = eager[b, j] if need[b, j] else lazy[b, j]
                    assert res[b, j].tobytes() == want.tobytes(), (k, b, j)
    finally:
        c.close()


def size_hyps():
    """32 768 + 37 seeded hypotheses on frames 0..3, every 50th skipped"""
    rng = np.random.default_rng(32805)
    H = 32768 + 37
    hy = np.zeros(H, hyp_dtype())
    hy["frame"] = rng.integers(0, 4, H)
    hy["lag"] = rng.integers(-300, 3701, H)
    hy["f0"] = rng.uniform(-8.0, 8.0, H).astype(np.float32)
    hy["drift"] = rng.choice(DRIFTS, H).astype(np.float32)
    hy["frame"][7::50] = -1
    return hy


@pytest.mark.gpu
def test_dispatch_by_size(G, oracle, frames):
    """d. The thresholds of launch_tonecorr (2^20 pairs: H = 6473) and launch_fold (H = 32 768) on a default context,
    and one call past both against T = 1 with the wave fold, and against the oracle."""
    hy = size_hyps()
    assert 6472 * NSYM < 1024 * 1024 <= 6473 * NSYM
    c = G.Context()
    try:
        for n, flat, fold in ((6472, "flat_t1", "fold_wave"), (6473, "flat_t2", "fold_wave"),
                              (32767, "flat_t2", "fold_wave"), (32768, "flat_t2", "fold_lanes")):
            before = c.launch_forms()
            c.sync_sweep(frames, hy[:n], soft=False)
            assert delta(c.launch_forms(), before) == {flat: 1, fold: 1}, n
        before = c.launch_forms()
        sync, sym = c.sync_sweep(frames, hy, soft=True)
        assert delta(c.launch_forms(), before) == {"flat_t2": 1, "fold_lanes": 1, "fold_lanes_soft": 1}
    finally:
        c.close()
    c = G.Context(options={"k4_t": 1, "k5_lanes": 0})
    try:
        sync1, sym1 = c.sync_sweep(frames, hy, soft=True)
        assert nonzero(c.launch_forms()) == {"flat_t1": 1, "fold_wave": 1, "fold_wave_soft": 1}
    finally:
        c.close()
    assert sync.tobytes() == sync1.tobytes() and sym.tobytes() == sym1.tobytes()
    idx = range(0, hy.size, 257)
    assert len(idx) == 128
    assert_equals_oracle(oracle, frames, hy, sync, sym, idx=idx)
    dead = hy["frame"] < 0
    assert dead.sum() == 656 and (sync[dead].view(np.uint32) == DEAD.view(np.uint32)).all() and not sym[dead].any()


# ------------------------------------------------------------------------------------------------------------- grid
def grid_wmax(ncombo):
    return min(16, (15 + ncombo - 1) // ncombo + 1)          # symbol windows a wavefront of 16 pairs can span


def grid_waves_per_wg(ncombo, span):
    """the rule of grid_waves_per_wg (k4_grid.hip): the most wavefronts (4, 2, 1) whose windows -- wmax per wavefront,
    256 + span samples each at an odd stride, 8 bytes a sample -- fit 64 KB of LDS; 0: none"""
    wstride = (256 + span) | 1
    return next((w for w in (4, 2, 1) if w * grid_wmax(ncombo) * wstride * 8 <= 64 * 1024), 0)


def grid_forms(ncombo, dl):
    """the counters one uwspr_sync_grid call moves: per lag block of 8 its NL and wavefronts per workgroup, up to the
    first block that does not fit"""
    out = collections.Counter()
    for base in range(0, len(dl), 8):
        blk = [int(x) for x in dl[base:base + 8]]
        wpw = grid_waves_per_wg(ncombo, max(blk) - min(blk))
        if wpw == 0:
            out["grid_fallback"] += 1
            break
        out["grid_nl%d" % next(n for n in (1, 2, 4, 5, 6, 8) if len(blk) <= n)] += 1
        out["grid_wpw%d" % wpw] += 1
    return out


def expand_grid(N, cents, df, dd, dl):
    """the grid's hypotheses as a flat uwspr_sync_sweep list, [centre][f][drift][lag] (include/uwspr_hip.h)"""
    hy = np.zeros((len(cents), df.size, dd.size, dl.size), N.HYP_DTYPE)
    for b, ce in enumerate(cents):
        nonlinear = int(ce["m_type"]) == 1
        hy["frame"][b] = b
        hy["m_type"][b] = ce["m_type"]
        hy["f0"][b] = (np.float32(ce["freq"]) + df.astype(np.float32))[:, None, None]
        lin = np.frombuffer(ce.tobytes()[24:28], np.float32)[0]
        hy["drift"][b] = 0.0 if nonlinear else (np.float32(lin) + dd.astype(np.float32))[None, :, None]
        hy["lag"][b] = (int(ce["shift"]) + dl.astype(np.int64))[None, None, :]
        if nonlinear:
            for key in ("V1", "V2", "p1", "p2"):
                hy[key][b] = ce[key]
    return hy.reshape(-1)


@pytest.mark.gpu
def test_grid_instantiations(G, oracle, frames, vec):
    """e. k4_grid<NL> at every NL (lag blocks of 1, 2, 3, 5, 6, 7 and 8 lags, alone and behind a block of 8), with 1, 2
    and 4 wavefronts per workgroup (ncombo = 1, 2, 16 and 32 x 32), at the largest window that fits LDS, and the
    fall-back to the flat kernel after a first block was launched: the flat sweep's bytes on the expanded list; the
    cases with a block of 2, 5 and 6 lags against the oracle directly."""
    N = G.native
    fr = np.concatenate([frames[:4], frames[1:2]])
    cents = np.zeros(5, N.CAND_DTYPE)
    cents[:4] = vec["cands"][:, 0]
    cents[4] = vec["cands"][1, 0]
    cents[1]["shift"] = 3500        # lags reach past np
    cents[2]["m_type"] = 1; cents[2]["V1"] = -1.0; cents[2]["V2"] = 2.0; cents[2]["p1"] = 0; cents[2]["p2"] = 450
    cents[3]["shift"] = 40          # lags reach before sample 0 -> cc:205 skipping
    cents[4]["m_type"] = 1; cents[4]["V1"] = 1.0; cents[4]["V2"] = -2.0; cents[4]["p1"] = 0; cents[4]["p2"] = 0
    rng = np.random.default_rng(61)
    f32 = lambda *v: np.array(v, np.float32)   # noqa: E731
    combos = {1: (f32(0.1), f32(0.0)),
              2: (f32(0.0, -0.3), f32(0.5)),
              16: (f32(-0.2, 0.0, 0.05, 0.3), f32(-1.0, 0.0, 0.25, 2.0))}
    cases = []
    for nlag in (2, 5, 6, 7, 10, 13, 14, 9, 3):      # 9 and 3: blocks of 1 and of 3 lags (NL = 1, 4), so every NL runs here
        dl = rng.choice(np.arange(-90, 91), nlag, replace=False).astype(np.int32)     # unsorted, both signs
        for nc in (1, 2, 16):
            cases.append((combos[nc][0], combos[nc][1], dl))
    cases.append(((np.arange(32) * 0.05 - 0.8).astype(np.float32), np.linspace(-1, 1, 32).astype(np.float32),
                  np.array([24, -40], np.int32)))
    # ncombo = 3: the largest span whose windows still fit (one wavefront per workgroup) behind a block of 8, and the
    # smallest that does not: the first block is launched, the second sends the whole call to the flat kernel
    fits = max(s for s in range(4096) if grid_waves_per_wg(3, s))
    assert grid_waves_per_wg(3, fits) == 1 and grid_waves_per_wg(3, fits + 1) == 0 and grid_waves_per_wg(3, 56) == 4
    first = np.arange(8, dtype=np.int32) * 8
    for span in (fits, fits + 1):
        second = np.array([0, span, 7, 100, span // 2, 33, span - 1, 64], np.int32) - 20
        cases.append((f32(0.0, 0.05, -0.05), f32(0.0), np.concatenate([first, second])))
    expect = collections.Counter()
    flat = G.Context()
    grid = G.Context()
    try:
        for df, dd, dl in cases:
            expect += grid_forms(df.size * dd.size, dl)
            sync, sym = grid.sync_grid(fr, cents, df, dd, dl, soft=True)
            hy = expand_grid(N, cents, df, dd, dl)
            fsync, fsym = flat.sync_sweep(fr, hy, soft=True)
            assert sync.reshape(-1).tobytes() == fsync.tobytes(), (df.size, dd.size, dl)
            assert sym.reshape(-1).tobytes() == fsym.tobytes(), (df.size, dd.size, dl)
            if df.size * dd.size == 2 and dl.size in (2, 5, 6):
                assert hy.size == 10 * dl.size
                assert_equals_oracle(oracle, fr, hy, sync.reshape(-1), sym.reshape(-1, NSYM))
        forms = grid.launch_forms()
        assert nonzero(flat.launch_forms()).keys() <= {"flat_t1", "flat_t2", "fold_wave", "fold_wave_soft"}
    finally:
        flat.close()
        grid.close()
    assert {k: v for k, v in forms.items() if k.startswith("grid_") and v} == dict(expect)
    assert all(expect[k] >= 1 for k in N_GRID_FORMS) and expect["grid_fallback"] == 1
    assert forms["flat_t1"] == 1 and forms["flat_t2"] == 0 and forms["flat_t4"] == 0      # the fall-back, and only it
    assert forms["fold_wave"] + forms["fold_lanes"] == len(cases)


N_GRID_FORMS = ("grid_nl1", "grid_nl2", "grid_nl4", "grid_nl5", "grid_nl6", "grid_nl8",
                "grid_wpw1", "grid_wpw2", "grid_wpw4", "grid_fallback")
