"""The list search, the parts a machine without a GPU can check: the restatement (tests/deep_exact.py) against the
definition's own words -- its table from the generator matrix equals wspr_symbols(m) >> 1, a noiseless vector scores
sum |s - 128| and wins, ties go to the smaller index, M = 1 has no runner-up -- and the C ABI: the entry points are
declared, exported and bound, uwspr_deep_result has the layout the header gives it, and a list that breaks the rules is
UWSPR_ERR_ARG before any device is asked for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import deep_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")
ERR_ARG = -6


def test_table_from_the_generator_is_the_symbols_code_bit(G):
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE90001)), 200)
    tab = X.code_table(G, msgs)
    assert tab.dtype == np.int64 and tab.shape == (200, 162)
    for m, row in zip(msgs, tab):
        assert np.array_equal(G.wspr_symbols(m) >> 1, row)
    text = G.wspr_pack("K1ABC FN42 37")
    assert text[6] & 0x3f == 0
    assert np.array_equal(X.code_table(G, text[None])[0], G.wspr_symbols("K1ABC FN42 37") >> 1)


def test_noiseless_vector_scores_the_sum_of_magnitudes_and_wins(G):
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE90002)), 300)
    tab = X.code_table(G, msgs)
    for m in (0, 17, 299):
        s = (255 * tab[m]).astype(np.uint8)   # 255 where the code bit is 1, 0 where it is 0
        r = X.deep_restate(tab, s)[0]
        want = int(np.abs(s.astype(np.int64) - 128).sum())
        assert (int(r["best"]), int(r["sbest"]), int(r["reserved"])) == (m, want, 0)
        assert 162 * 127 <= want <= 162 * 128 and r["snext"] < r["sbest"]
        assert X.scores(tab, s)[0].max() == want and abs(int(X.scores(tab, s)[0].min())) <= 20736


def test_ties_go_to_the_smaller_index_and_one_message_has_no_runner_up(G):
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE90003)), 8)
    tab = X.code_table(G, msgs)
    # 128 wherever messages 2 and 5 differ, noiseless for both elsewhere: they score the same
    agree = tab[2] == tab[5]
    s = np.full(162, 128, np.uint8)
    s[agree] = (255 * tab[2][agree]).astype(np.uint8)
    S = X.scores(tab, s)[0]
    assert S[2] == S[5] == S.max()
    r = X.deep_restate(tab, s)[0]
    assert (int(r["best"]), int(r["sbest"]), int(r["snext"])) == (2, int(S[2]), int(S[2]))
    # all-128: every score is 0
    r = X.deep_restate(tab, np.full(162, 128, np.uint8))[0]
    assert (int(r["best"]), int(r["sbest"]), int(r["snext"])) == (0, 0, 0)
    # M = 1
    r = X.deep_restate(tab[:1], s)[0]
    assert (int(r["best"]), int(r["sbest"]), int(r["snext"])) == (0, int(S[0]), -2 ** 31)
    assert X.accepted(r, 1, int(S[0]), 10 ** 9) and not X.accepted(r, 1, int(S[0]) + 1, 0)
    r2 = X.deep_restate(tab[:2], s)[0]
    assert X.accepted(r2, 2, 0, int(r2["sbest"]) - int(r2["snext"])) and not X.accepted(r2, 2, 0, int(r2["sbest"]) - int(r2["snext"]) + 1)


def test_entry_points_are_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    assert re.search(r"int uwspr_deep_set_list\(uwspr_ctx \*ctx, const int8_t \*messages7 /\*\[M\]\[7\]\*/, int M\);", hdr)
    assert re.search(r"int uwspr_deep_batch\(uwspr_ctx \*ctx, const uint8_t \*symbols /\*\[n\]\[162\]\*/, int n, int where, "
                     r"uwspr_deep_result \*res\);", hdr)
    assert re.search(r"int uwspr_pipe_set_list\(uwspr_pipe \*pipe, const int8_t \*messages7 /\*\[M\]\[7\]\*/, int M\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m and int(m.group(1)) == 6
    entry6 = m.group(2).split("6:")[1]
    for name in ("uwspr_deep_result", "uwspr_deep_set_list", "uwspr_deep_batch", "uwspr_pipe_set_list", '"deep_min"', '"deep_gap"',
                 "uwspr_decode.osd = 2"):
        assert name in entry6, name
    N = G.native
    for macro, value in (("UWSPR_DEEP_MAX", N.DEEP_MAX), ("UWSPR_DEEP_MIN_DEFAULT", N.DEEP_MIN_DEFAULT),
                         ("UWSPR_DEEP_GAP_DEFAULT", N.DEEP_GAP_DEFAULT)):
        d = re.search(r"#define %s (\d+)" % macro, hdr)
        assert d and int(d.group(1)) == value, macro
    assert N.DEEP_MAX == 65536
    L = N.lib()
    for name, nargs in (("uwspr_deep_set_list", 3), ("uwspr_deep_batch", 5), ("uwspr_pipe_set_list", 3)):
        assert name in N.ABI_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert callable(G.Context.deep) and callable(G.Context.deep_set_list) and callable(G.Pipe.set_list)
    assert "1: ordered-statistics decoding, 2: list search" in hdr


def test_result_layout_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(sizeof(uwspr_deep_result) == 16, \"result\");\n"
                   "static_assert(offsetof(uwspr_deep_result, best) == 0 && offsetof(uwspr_deep_result, sbest) == 4, \"result\");\n"
                   "static_assert(offsetof(uwspr_deep_result, snext) == 8 && offsetof(uwspr_deep_result, reserved) == 12, \"result\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112 && offsetof(uwspr_decode, osd) == 111, \"decode\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    R = G.native.DEEP_RESULT_DTYPE
    assert R == X.DEEP_DTYPE and R.itemsize == 16
    assert [R.fields[k][1] for k in ("best", "sbest", "snext", "reserved")] == [0, 4, 8, 12]


def test_list_rules_are_checked_before_any_device(G):
    N = G.native
    L = N.lib()
    params = N.Params(375, 45000, 256, 0, 200, 10, 1500, 10)
    h = C.c_void_p()
    L.uwspr_ctx_create(C.byref(params), 0, C.byref(h))   # without a device the call fails and still hands the context back
    assert h.value
    try:
        good = X.random_messages(np.random.Generator(np.random.Philox(0xDEE90004)), 5)

        def call(a, M=None):
            a = np.ascontiguousarray(a, np.int8)
            return L.uwspr_deep_set_list(h, C.c_void_p(a.ctypes.data), len(a) if M is None else M)

        dup = good.copy()
        dup[4] = dup[1]
        assert call(dup) == ERR_ARG and b"twice" in L.uwspr_last_error(h)
        dirty = good.copy()
        dirty[3, 6] |= 1
        assert call(dirty) == ERR_ARG and b"byte 6" in L.uwspr_last_error(h)
        assert call(good, N.DEEP_MAX + 1) == ERR_ARG   # (M is refused before a byte is read)
        assert call(good, -1) == ERR_ARG
        assert L.uwspr_deep_set_list(h, None, 3) == ERR_ARG
        assert L.uwspr_deep_set_list(None, C.c_void_p(good.ctypes.data), 5) == ERR_ARG
        # no list: the batch call is an argument error, with or without items
        sym = np.full((2, 162), 128, np.uint8)
        res = np.zeros(2, N.DEEP_RESULT_DTYPE)
        assert L.uwspr_deep_batch(h, C.c_void_p(sym.ctypes.data), 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_deep_batch(h, None, 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_deep_batch(h, C.c_void_p(sym.ctypes.data), 2, N.HOST, None) == ERR_ARG
        assert L.uwspr_deep_batch(h, C.c_void_p(sym.ctypes.data), -1, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_deep_batch(None, C.c_void_p(sym.ctypes.data), 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert not res.view(np.uint8).any()
        assert L.uwspr_pipe_set_list(None, C.c_void_p(good.ctypes.data), 5) == ERR_ARG
    finally:
        L.uwspr_ctx_destroy(h)


def test_python_list_helper_packs_texts(G):
    m = G.context.deep_list(["K1ABC FN42 37", "W1AW EM10 30"])
    assert m.dtype == np.int8 and m.shape == (2, 7)
    assert np.array_equal(m[0], G.wspr_pack("K1ABC FN42 37")) and np.array_equal(m[1], G.wspr_pack("W1AW EM10 30"))
    assert G.context.deep_list([]).shape == (0, 7) and G.context.deep_list(None).shape == (0, 7)
    assert G.context.deep_list(m) is m or np.array_equal(G.context.deep_list(m), m)
    with pytest.raises(TypeError):
        G.context.deep_list(np.zeros((2, 8), np.int8))
