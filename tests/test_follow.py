"""K16 without a GPU: the binary64 restatement (tests/follow_exact.py) decodes the moving sources that the fine search loses
(tests/follow_cases.py: the oracle's FDR + schedule, the host Fano decoder, the restated follower); the hypothesis index, the
pick, the s_ref identity and the normalisation on designed inputs; the pipe's acceptance gates as a stand-alone host
program; the refusals that need no device and the ABI bookkeeping."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import follow_cases as FC
import follow_exact as FX
import track_exact as TX

MINRMS = np.float32(52.0 * (50 / 64.0))


def _decodes(G, sym):
    rc, msg, _, cycles = G.fano_decode(G.deinterleave(sym))
    return rc == 0 and G.unpack_message(msg[:7].astype(np.int8)) == (0, FC.TEXT), cycles // 81


@pytest.mark.parametrize("model", FC.MODELS)
@pytest.mark.parametrize("k", sorted(FC.SLM))
def test_restatement_decodes_what_the_fine_search_loses(G, oracle, k, model):
    """Per case: the oracle's strongest record is an item under the fallbacks' common rule (worth a try, a gated try); Fano
    decodes none of its gated tries; the restated follower over the true pass among five decoys, qf = 16, nl = 2, picks the
    true pass and its bytes decode to the sent text -- also in 16 copies with a random 2 % of the bytes moved by +-1, twice the
    share of bytes in which the kernel may differ from the restatement.  Measured: 15 to 17 gated tries, largest jig_sync
    0.17 to 0.31, S(best) 0.45 to 0.52 at q = -7 (trajectories 1, 21: -1.28 Hz) and q = -13 (trajectory 35: -2.38 Hz, hence a
    reach of 16), lags -1 .. 1, Fano at 1 cycle per bit."""
    fr = FC.frame(G, k, model)
    cands = oracle.FDR().transform(fr)
    assert len(cands) >= 1
    d = oracle.demod_candidate(cands[0], 1500, fr)
    gated = [t for t in range(17) if d["jig_sync"][t] > np.float32(0.12) and d["jig_rms"][t] > MINRMS]
    assert d["worth_a_try"] and gated
    assert not any(G.fano_decode(G.deinterleave(d["symbols"][t]))[0] == 0 for t in gated)
    t = max(gated, key=lambda kk: (d["jig_sync"][kk], -kk))
    f, drift = np.float32(d["f1"]), np.float32(d["drift1"])
    if int(cands[0]["m_type"]) == G.native.NONLINEAR:
        from test_gpu_blockdemod import slm_at_zero
        f, drift = np.float32(f + slm_at_zero(cands[0])), np.float32(0.0)
    shift = int(d["jig_shift"][t])
    grid, ti = FC.grid(G, k)
    assert len(grid) >= 6
    df, ta = TX.design(grid, model)
    best, S, sym = FX.follow(fr, shift, f, df, ta, FC.QF, FC.NL)
    j, q, l = FX.unhyp(best, FC.QF, FC.NL)
    sref = FX.s_ref(fr, shift, f, drift)
    ok, cycles = _decodes(G, sym)
    print("trajectory %d %s: %d gated tries, largest jig_sync %.3f, item (%d, %.4f, %.2f); best j %d q %d l %d, S %.3f, s_ref %.3f, rms %.1f, %d cycles / bit"
          % (k, model, len(gated), max(d["jig_sync"]), shift, f, drift, j, q, l, S.reshape(-1)[best], sref, FX.rms(sym), cycles))
    assert j == ti and S.reshape(-1)[best] > sref and S.reshape(-1)[best] > 0.12 and FX.rms(sym) > MINRMS
    assert abs(sref - float(d["jig_sync"][t])) < 1e-5        # S is the fine search's own metric: the record's line gives its jig_sync
    assert ok
    rng = np.random.Generator(np.random.Philox(0xF0110 + k))
    for _ in range(16):
        step = np.where(rng.random(162) < 0.02, rng.choice([-1, 1], 162), 0)
        assert _decodes(G, np.clip(sym.astype(np.int32) + step, 0, 255).astype(np.uint8))[0]


def test_hypothesis_index():
    seen = set()
    qf, nl = 3, 2
    for j in range(4):
        for q in range(-qf, qf + 1):
            for l in range(-nl, nl + 1):
                h = FX.hyp(j, q, l, qf, nl)
                assert FX.unhyp(h, qf, nl) == (j, q, l)
                seen.add(h)
    assert seen == set(range(4 * 7 * 5))
    assert FX.hyp(0, -qf, -nl, qf, nl) == 0 and FX.hyp(0, -qf, -nl + 1, qf, nl) == 1 and FX.hyp(0, -qf + 1, -nl, qf, nl) == 5
    assert FX.hyp(1, -qf, -nl, qf, nl) == 35


def test_pick_rule_of_the_restatement():
    nan = float("nan")
    assert FX.first_max([0.1, 0.3, 0.3, 0.2]) == 1
    assert FX.first_max([nan, 0.3, 0.5]) == 0
    assert FX.first_max([0.1, nan, 0.5, nan, 0.5]) == 2
    assert FX.first_max([0.0, 0.0]) == 0
    assert FX.first_max([-0.2, -0.1, -0.1]) == 1


def _tone_frame(G, f0, shift):
    """a clean static transmission of TEXT at f0 from sample `shift`"""
    return TX.synth(G.wspr_symbols(FC.TEXT), (0.0, 100.0, 0.0), "doppler", shift, f0=f0)


def test_surface_on_a_designed_frame(G):
    """A clean static transmission: S is 1 at the static pass, the true offset and lag 0 (every symbol's energy sits on its
    sync-consistent tones: (p1 + p3) - (p0 + p2) = +- the sum, up to the other tones' leakage), smaller at every other
    hypothesis, and a pass that moves scores less.  An item 3 steps of Q off tune finds q = -3."""
    fr = _tone_frame(G, 1.0, 400)
    trajs = G.track_trajs([(0.0, 100.0, 0.0), (2.5, 50.0, 55.0)])
    df, ta = TX.design(trajs, "delay")
    S = FX.surface(fr, 400, 1.0, df, ta, 2, 1)
    assert S.shape == (2, 5, 3)
    assert FX.first_max(S) == FX.hyp(0, 0, 0, 2, 1) and S[0, 2, 1] > 0.95
    assert S[1].max() < S[0, 2, 1]
    off = np.float32(1.0 + 3 * FX.Q)
    S3 = FX.surface(fr, 400, off, df[:1], ta[:1], 4, 0)
    assert FX.unhyp(FX.first_max(S3), 4, 0) == (0, -3, 0)
    assert abs(S3[0, 1, 0] - S[0, 2, 1]) < 1e-6
    # an all-zero frame: the denominator is 0, S is 0 everywhere, the pick stays at 0 and the bytes are 128
    z = np.zeros((TX.FL, 2), np.float32)
    best, S0, sym = FX.follow(z, 400, 1.0, df, ta, 1, 1)
    assert best == 0 and not S0.any() and (sym == 128).all()


def test_s_ref_identity(G):
    """a v = 0 pass at q = 0, l = 0 of an item without drift is the record's own line; with a drift it is another sum"""
    rng = np.random.Generator(np.random.Philox(5))
    fr = _tone_frame(G, 1.0, 400) + rng.standard_normal((TX.FL, 2)).astype(np.float32)
    df, ta = TX.design([(0.0, 100.0, 0.0)], "delay")
    S = FX.surface(fr, 380, 1.1, df, ta, 0, 1)              # (the same grid width as s_ref's: the same matrix product)
    assert S[0, 0, 1] == FX.s_ref(fr, 380, 1.1, 0.0)
    assert S[0, 0, 1] != FX.s_ref(fr, 380, 1.1, 1.0)
    assert abs(FX.surface(fr, 380, 1.1, df, ta, 2, 0)[0, 2, 0] - S[0, 0, 1]) < 1e-12


def test_normalisation(G):
    """K10's text on designed values: soft = +-1, +-2 in equal shares has fsum 0 and fac sqrt(2.5), so v = +-31.62, +-63.25
    and the bytes are (uint8)(v + 128) = 159, 96, 191, 64; the clip; a NaN or a constant vector (fac 0) gives 128 everywhere; and on a clean frame the data bits come back"""
    s = np.tile([1.0, -1.0, 2.0, -2.0], 41)[:162]            # (162 = 40 x 4 + 2: one more +-1 pair, fac 1.5753: v = +-31.74, +-63.48)
    assert list(FX.normalise(s)[:4]) == [159, 96, 191, 64] and set(FX.normalise(s)) == {159, 96, 191, 64}
    big = s.copy()
    big[0], big[1] = 1e3, -1e3
    b = FX.normalise(big)
    assert b[0] == 255 and b[1] == 0
    assert (FX.normalise(np.full(162, 2.5)) == 128).all()
    bad = s.copy()
    bad[7] = np.nan
    assert (FX.normalise(bad) == 128).all()
    assert (FX.normalise(np.zeros(162)) == 128).all()
    v = np.zeros(162)
    v[0], v[1] = 1.0, -1.0                      # fac = sqrt(2 / 162): 50 / fac = 450, clipped
    assert FX.normalise(v)[0] == 255 and FX.normalise(v)[1] == 0 and FX.normalise(v)[2] == 128
    sym = G.wspr_symbols(FC.TEXT)
    fr = _tone_frame(G, 1.0, 400)
    df, ta = TX.design([(0.0, 100.0, 0.0)], "delay")
    by = FX.symbols(fr, 400, 1.0, df[0], ta[0], 0, 0)
    assert np.array_equal(by > 128, (np.asarray(sym) >> 1) == 1)
    assert _decodes(G, by)[0]


def test_follow_gates_host_program():
    """rules::follow_gates and rules::bytes_rms (gr-uwspr_amd/csrc/pipe_rules.h) against values written by hand in
    tests/host/follow_rules_main.cc, as a stand-alone CPU program under ASan + UBSan"""
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "host", "_follow_rules")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "gr-uwspr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "follow_rules_main.cc"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "follow rules ok" in r.stdout and "runtime error" not in r.stderr


def test_refusals_that_need_no_device(G):
    N = G.native
    L = N.lib()
    tr = G.track_trajs([TX.TRUTH])
    assert L.uwspr_follow_set(None, C.c_void_p(tr.ctypes.data), 1, 4, 1, N.TX_DELAY) == -6
    assert L.uwspr_follow_batch(None, None, 1, N.HOST, None, 0, None, None, None) == -6
    assert L.uwspr_pipe_set_follow(None, C.c_void_p(tr.ctypes.data), 1, 4, 1, N.TX_DELAY) == -6
    assert L.uwspr_pipe_collect_follows(None, None, 0) == -6


def test_abi_bookkeeping(G):
    N = G.native
    hdr = open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read()
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert int(m.group(1)) == 6
    for name in ("uwspr_follow_result", "uwspr_follow_set", "uwspr_follow_batch", "uwspr_follow_record", "uwspr_pipe_set_follow",
                 "uwspr_pipe_collect_follows"):
        assert name in m.group(2), name
    for name in ("uwspr_follow_set", "uwspr_follow_batch", "uwspr_pipe_set_follow", "uwspr_pipe_collect_follows"):
        assert name in N.ABI_SYMBOLS and hasattr(N.lib(), name)
    assert "k16_follow.hip" in N.SOURCES
    assert N.FOLLOW_RESULT_DTYPE.itemsize == 16 and N.FOLLOW_RECORD_DTYPE.itemsize == 32 and N.BLOCK_ITEM_DTYPE.itemsize == 16
    assert N.FOLLOW_Q == FX.Q and N.FOLLOW_LSTEP == FX.LSTEP
    assert re.search(r"4: Fano timed\s+out on every gated try and decoded K16", hdr)      # uwspr_decode.osd documents 4
