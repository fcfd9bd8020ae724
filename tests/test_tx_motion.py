"""Moving sources on the transmit side, the parts a machine without a GPU can check: uwspr_tx_motion's layout in C and
ctypes, the two entry points declared, exported and bound, the signal dicts' "motion", and the receiver's
straight-line-model grid and Doppler (slm_trajectories, slm_drift) against lib/slm.cc restated."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")
FIELDS = [("v1", 0), ("v2", 8), ("p1", 16), ("p2", 24), ("t_first", 32), ("model", 40), ("flags", 44)]


def test_motion_layout_in_c_and_ctypes(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n' +
                   "".join('static_assert(offsetof(uwspr_tx_motion, %s) == %d, "%s");\n' % (f, o, f) for f, o in FIELDS) +
                   'static_assert(sizeof(uwspr_tx_motion) == 48, "size");\n'
                   'static_assert(sizeof(uwspr_tx_signal) == 208 && sizeof(uwspr_tx_channel) == 40, "static records");\n'
                   'static_assert(UWSPR_TX_STATIC == 0 && UWSPR_TX_DOPPLER == 1 && UWSPR_TX_DELAY == 2, "models");\n'
                   'static_assert(UWSPR_TX_ABSOLUTE == 1 && UWSPR_TX_SPREADING == 2, "flags");\n'
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    M = G.native.TxMotion
    assert C.sizeof(M) == 48
    assert [(f, getattr(M, f).offset) for f, _ in FIELDS] == FIELDS
    N = G.native
    assert (N.TX_STATIC, N.TX_DOPPLER, N.TX_DELAY, N.TX_ABSOLUTE, N.TX_SPREADING) == (0, 1, 2, 1, 2)


def test_entry_points_are_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    assert re.search(r"int uwspr_tx_baseband_moving\(uwspr_ctx \*ctx, const uwspr_tx_signal \*sig, "
                     r"const uwspr_tx_motion \*motion, int nsig,\s+int channel, long long t0, int n, float \*iq, int where\);", hdr)
    assert re.search(r"int uwspr_tx_render_moving\(uwspr_ctx \*ctx, const uwspr_tx_signal \*sig, "
                     r"const uwspr_tx_motion \*motion, int nsig,\s+const uwspr_tx_channel \*chan, int C, long long t0, "
                     r"long long nframes, int format, void \*out,\s+int where\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m and int(m.group(1)) == 6
    entry6 = m.group(2).split("6:")[1]
    L = G.native.lib()
    for name, nargs in (("uwspr_tx_baseband_moving", 9), ("uwspr_tx_render_moving", 11)):
        assert name in entry6 and name in G.native.ABI_SYMBOLS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs


def test_signal_dicts_carry_their_motion(G):
    N = G.native
    s = [{"text": "K1ABC FN42 37"},
         {"text": "K1ABC FN42 37", "motion": {"v": (1.0, -2.0), "p": (3.0, 450.0), "t": 9.5, "model": "delay",
                                              "absolute": True, "spreading": True}},
         {"text": "K1ABC FN42 37", "motion": {"v": (0.5, 0.0), "p": (0.0, 50.0)}}]
    assert G.tx_motions(s[:1]) is None and G.tx_motions([]) is None
    m = G.tx_motions(s)
    assert len(m) == 3
    assert (m[0].model, m[0].flags, m[0].v1, m[0].p2) == (N.TX_STATIC, 0, 0.0, 0.0)
    assert (m[1].v1, m[1].v2, m[1].p1, m[1].p2, m[1].t_first) == (1.0, -2.0, 3.0, 450.0, 9.5)
    assert (m[1].model, m[1].flags) == (N.TX_DELAY, N.TX_ABSOLUTE | N.TX_SPREADING)
    assert (m[2].model, m[2].flags, m[2].t_first) == (N.TX_DOPPLER, 0, 0.0)
    assert len(G.tx_signals(s)) == 3
    with pytest.raises(ValueError):
        G.tx_motions([{"text": "K1ABC FN42 37", "motion": {"speed": 3}}])
    with pytest.raises(KeyError):
        G.tx_motions([{"text": "K1ABC FN42 37", "motion": {"model": "warp"}}])


def _generator():
    """lib/slm.cc:76-116 as written: the static indices and their wrap-around, one instance per call"""
    V1_min, V1_max, V1_step = -2, 2, 1
    V2_min, V2_max, V2_step = -2, 2, 1
    p2_min, p2_max, p2_step = 50, 850, 200
    nV1 = (V1_max - V1_min) // V1_step + 1
    np2 = (p2_max - p2_min) // p2_step + 1
    last = nV1 * ((V2_max - V2_min) // V2_step + 1) * np2
    ip2 = iV1 = iV2 = 0
    for _ in range(last):
        if ip2 >= np2:
            ip2 = 0
            iV1 += 1
            if iV1 >= nV1:
                iV1 = 0
                iV2 += 1
        yield (iV1 * V1_step + V1_min, iV2 * V2_step + V2_min, 0, ip2 * p2_step + p2_min)
        ip2 += 1


def test_slm_trajectories_are_the_generator_order(G):
    t = G.slm_trajectories()
    assert t.shape == (125, 4) and t.dtype == np.float64
    assert np.array_equal(t, np.array(list(_generator()), np.float64))
    assert tuple(t[0]) == (-2, -2, 0, 50) and tuple(t[1]) == (-2, -2, 0, 250) and tuple(t[5]) == (-1, -2, 0, 50)
    assert tuple(t[25]) == (-2, -1, 0, 50) and tuple(t[124]) == (2, 2, 0, 850)


def _slm_sign_form(tr, t, cf=1500.0):
    """slmFrequencyDrift as slm.cc writes it: -Sign |V.q| / |q| cf / c, Sign = 2 (V.q > 0) - 1, 0 where |q| = 0"""
    V1, V2, p1, p2 = tr
    q1, q2 = V1 * t + p1, V2 * t + p2
    sign = ((q1 * V1 + q2 * V2) > 0) * 2.0 - 1.0
    num = np.abs(V1 * q1 + V2 * q2)
    den = np.sqrt(q1 ** 2 + q2 ** 2)
    return np.where(den == 0, 0.0, -sign * num / np.where(den == 0, 1.0, den) * cf / 1500.0)


def test_slm_drift_is_slm_cc_and_minus_dr_dt(G):
    grid = G.slm_trajectories()
    t = np.arange(111, dtype=np.float64)
    got = G.slm_drift(grid[:, None, :], t[None, :])
    assert got.shape == (125, 111) and got.dtype == np.float64
    for i, tr in enumerate(grid):
        ref = _slm_sign_form(tr, t)
        assert np.allclose(got[i], ref, rtol=1e-13, atol=1e-13), i
        # -(fc / c) dR/dt, fc = c: central differences of R
        h = 1e-3
        R = lambda s: np.hypot(tr[0] * s + tr[2], tr[1] * s + tr[3])   # noqa: E731
        fd = -(R(t + h) - R(t - h)) / (2 * h)
        assert np.abs(got[i] - fd).max() < 1e-6, i
    assert np.abs(got).max() > 2.5   # |V| = 2 sqrt 2 moving away / towards: up to 2.83 Hz
    # scalar forms, the carrier, and R = 0
    assert G.slm_drift((1.0, 0.0, 0.0, 0.0), 0.0) == 0.0
    assert G.slm_drift((0.0, 2.0, 0.0, 50.0), 3.0) == -2.0
    assert G.slm_drift((0.0, 2.0, 0.0, 50.0), 3.0, cf=750.0) == -1.0
    assert G.slm_drift((0.0, -2.0, 0.0, 50.0), 3.0) == 2.0
