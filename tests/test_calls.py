"""The call search, the parts a machine without a GPU can check: the decomposition the kernel rests on -- the code bits of
"CALL GRID dBm" are the XOR of those of the callsign alone, the locator alone and the power alone -- against wspr_symbols
of the packed text; call_message against wspr_pack and unpack_message; the hypothesis index; the "grids" spec; the
restatement (tests/call_exact.py) against the list search's (tests/deep_exact.py) on explicit lists; and the C ABI: the
entry points are declared, exported and bound, uwspr_call_result has the layout the header gives it, and a call set that
breaks the rules is UWSPR_ERR_ARG with a message before any device is asked for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import call_exact as CX
import deep_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")
ERR_ARG = -6
CORNER_CALLS = ["K1ABC", "W1AW", "A1B", "G4ABC", "9A1AA", "1A2BCD", "AB1CDE", "R30O", "C0R", "N0T"]   # 3 to 6 characters; a leading
# blank in the packed form (the digit second), a leading digit, the digit third


def triples():
    rng = np.random.Generator(np.random.Philox(0xCA110001))
    calls = CX.random_calls(rng, 300)
    out = [(c, int(rng.integers(CX.NGRID)), int(rng.integers(CX.NPOW))) for c in calls]
    out += [(c, g, d) for c in CORNER_CALLS for g in (0, CX.NGRID - 1) for d in (0, CX.NPOW - 1)]
    return out


def test_code_bits_are_the_xor_of_the_three_partial_codewords(G):
    gb, pb = CX.grid_bits(G), CX.power_bits(G)
    assert gb.shape == (CX.NGRID, 162) and pb.shape == (CX.NPOW, 162)
    for call, g, d in triples():
        text = "%s %s %d" % (call, CX.ngrid_grid(g), CX.P19[d])
        want = G.wspr_symbols(G.wspr_pack(text)) >> 1
        assert np.array_equal(want, CX.call_bits(G, [call])[0] ^ gb[g] ^ pb[d]), text


def test_call_message_is_wspr_pack_and_unpacks_to_the_text(G):
    for call, g, d in triples():
        grid, dbm = CX.ngrid_grid(g), CX.P19[d]
        assert CX.grid_ngrid(grid) == g and G.grid_ngrid(grid) == g
        text = "%s %s %d" % (call, grid, dbm)
        m = G.call_message(call, grid, dbm)
        assert m.dtype == np.int8 and np.array_equal(m, G.wspr_pack(text)), text
        assert np.array_equal(m, G.call_message(call.lower(), g, dbm)) and np.array_equal(m, CX.message(G, call, g, dbm))
        assert G.unpack_message(m) == (0, "%s %s %2d" % (call, grid, dbm)), text
    for bad in (("K1ABC", 32400, 37), ("K1ABC", -1, 37), ("K1ABC", 0, 36), ("K1ABC", 0, 63), ("PJ4/K1ABC", 0, 37), ("<K1ABC>", 0, 37),
                ("K1", 0, 37), ("K1ABCDE", 0, 37), ("K1 AB", 0, 37), ("KABC", 0, 37)):
        with pytest.raises(G.UwsprError) as e:
            G.call_message(*bad)
        assert e.value.status == ERR_ARG, bad


def test_hypothesis_index_maps_both_ways():
    rng = np.random.Generator(np.random.Philox(0xCA110002))
    for a, g, d in [(0, 0, 0), (63, 32399, 18), (1, 0, 0), (0, 1, 0), (0, 0, 1)] + [tuple(int(v) for v in (rng.integers(64), rng.integers(32400), rng.integers(19))) for _ in range(200)]:
        h = CX.join_h(a, g, d)
        assert 0 <= h < 64 * 615600 < 2 ** 31 and CX.split_h(h) == (a, g, d)
    assert CX.join_h(0, 0, 1) == 1 and CX.join_h(0, 1, 0) == 19 and CX.join_h(1, 0, 0) == 615600
    assert len(CX.P19) == 19 and all(p % 10 in (0, 3, 7) for p in CX.P19) and CX.P19 == tuple(sorted(CX.P19))


def test_grids_spec_makes_the_bitmap(G):
    assert G.grids_bitmap(None) is None
    fn = G.grids_bitmap(["FN"])
    assert fn.dtype == np.uint8 and fn.shape == (4050,) and int(np.unpackbits(fn).sum()) == 100
    assert np.array_equal(fn, CX.grids_bitmap(["FN"])) and np.array_equal(fn, G.grids_bitmap("fn"))
    cells = CX.bitmap_list(fn)
    assert all(CX.ngrid_grid(int(g))[:2] == "FN" for g in cells) and len(set(cells.tolist())) == 100
    one = G.grids_bitmap(["FN42"])
    g = CX.grid_ngrid("FN42")
    assert CX.bitmap_list(one).tolist() == [g] and one[g >> 3] == 1 << (g & 7)
    both = G.grids_bitmap(["FN", "FN42", "JO22", "AA00", "RR99"])
    assert int(np.unpackbits(both).sum()) == 103
    assert CX.bitmap_list(G.grids_bitmap(["RR99"])).tolist() == [179] and CX.bitmap_list(G.grids_bitmap(["AA00"])).tolist() == [32220]
    assert CX.bitmap_list(G.grids_bitmap(["RA90"])).tolist() == [0] and CX.bitmap_list(G.grids_bitmap(["AR09"])).tolist() == [32399]
    for bad in (["F"], ["FN4"], ["SN42"], ["FNAB"]):
        with pytest.raises(ValueError):
            G.grids_bitmap(bad)
    assert G.powers_mask(None) == 0 and G.powers_mask([0]) == 1 and G.powers_mask([60, 0, 37]) == (1 << 18) | 1 | (1 << 11)
    assert CX.power_list(0).tolist() == list(range(19)) and CX.power_list(G.powers_mask([3, 60])).tolist() == [1, 18]


def test_restatement_agrees_with_the_list_search_on_explicit_lists(G):
    rng = np.random.Generator(np.random.Philox(0xCA110003))
    calls = CX.random_calls(rng, 4)
    bm = CX.grids_bitmap(["FN", "JO22"])
    gl, dl = CX.bitmap_list(bm), CX.power_list(CX.powers_mask((0, 37, 60)))
    pm = CX.powers_mask((0, 37, 60))
    # every allowed hypothesis, in the order of h: the list search's index is the rank of h
    hs = np.array([CX.join_h(a, g, d) for a in range(4) for g in gl for d in dl])
    assert (np.diff(hs) > 0).all()
    sym = rng.integers(0, 256, (12, 162), dtype=np.uint8)
    tie = np.full(162, 128, np.uint8)
    sym = np.concatenate([sym, tie[None]])
    r = CX.call_restate(G, calls, bm, pm, sym)
    # 64 messages drawn from the set, the winner among them
    for i in range(len(sym)):
        pick = np.sort(np.unique(np.concatenate([rng.choice(len(hs), 63, replace=False), [int(np.searchsorted(hs, r[i]["best"]))]])))[:64]
        if int(np.searchsorted(hs, r[i]["best"])) not in pick:
            pick[-1] = int(np.searchsorted(hs, r[i]["best"]))
            pick = np.sort(pick)
        msgs = np.stack([CX.message(G, calls[a], g, CX.P19[d]) for a, g, d in (CX.split_h(int(h)) for h in hs[pick])])
        S = X.scores(X.code_table(G, msgs), sym[i])[0]
        full = CX.scores(G, calls, gl, dl, sym[i])[0].reshape(-1)
        assert np.array_equal(S, full[pick])                       # the same S, message by message
        d = X.deep_restate(X.code_table(G, msgs), sym[i])[0]
        assert int(hs[pick][int(d["best"])]) == int(r[i]["best"]) and int(d["sbest"]) == int(r[i]["sbest"])
        assert int(d["snext"]) <= int(r[i]["snext"])
    # the whole set as a list: the same winner under the order of h, the same runner-up
    msgs = np.stack([CX.message(G, calls[a], g, CX.P19[d]) for a, g, d in (CX.split_h(int(h)) for h in hs)])
    d = X.deep_restate(X.code_table(G, msgs), sym)
    assert hs[d["best"]].tolist() == r["best"].tolist()
    assert d["sbest"].tolist() == r["sbest"].tolist() and d["snext"].tolist() == r["snext"].tolist()
    assert (int(r[-1]["best"]), int(r[-1]["sbest"]), int(r[-1]["snext"])) == (int(hs[0]), 0, 0)
    a, g, dd = CX.split_h(int(r[0]["best"]))
    assert (int(r[0]["call"]), int(r[0]["ngrid"]), int(r[0]["dbm"])) == (a, g, CX.P19[dd]) and not r["reserved"].any()
    one = CX.call_restate(G, calls[:1], CX.grids_bitmap(["FN42"]), CX.powers_mask((37,)), sym[:2])
    assert (one["snext"] == CX.INT32_MIN).all() and CX.accepted(one[0], 1, int(one[0]["sbest"]), 10 ** 9)
    assert not CX.accepted(r[0], len(hs), int(r[0]["sbest"]) + 1, 0)
    assert CX.accepted(r[0], len(hs), 0, int(r[0]["sbest"]) - int(r[0]["snext"])) and not CX.accepted(r[0], len(hs), 0, int(r[0]["sbest"]) - int(r[0]["snext"]) + 1)


def test_entry_points_are_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    assert re.search(r"int uwspr_calls_set\(uwspr_ctx \*ctx, const char \*const \*calls, int A, const uint8_t \*grid_bitmap /\*\[4050\] or NULL\*/,\s+uint32_t power_mask\);", hdr)
    assert re.search(r"int uwspr_calls_batch\(uwspr_ctx \*ctx, const uint8_t \*symbols /\*\[n\]\[162\]\*/, int n, int where, uwspr_call_result \*res\);", hdr)
    assert re.search(r"int uwspr_call_message\(const char \*call, int ngrid, int dbm, int8_t \*message7\);", hdr)
    assert re.search(r"int uwspr_pipe_set_calls\(uwspr_pipe \*pipe, const char \*const \*calls, int A, const uint8_t \*grid_bitmap /\*\[4050\] or NULL\*/,\s+uint32_t power_mask\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    last = m.group(2).split("%s:" % m.group(1))[1]
    for name in ("uwspr_call_result", "uwspr_calls_set", "uwspr_calls_batch", "uwspr_call_message", "uwspr_pipe_set_calls",
                 '"call_min"', '"call_gap"', "uwspr_decode.osd = 3"):
        assert name in last, name
    N = G.native
    for macro, value in (("UWSPR_CALLS_MAX", N.CALLS_MAX), ("UWSPR_CALL_NGRID", N.CALL_NGRID), ("UWSPR_CALL_NPOW", len(N.P19)),
                         ("UWSPR_CALL_MIN_DEFAULT", N.CALL_MIN_DEFAULT), ("UWSPR_CALL_GAP_DEFAULT", N.CALL_GAP_DEFAULT)):
        d = re.search(r"#define %s (\d+)" % macro, hdr)
        assert d and int(d.group(1)) == value, macro
    assert (N.CALLS_MAX, N.CALL_NGRID, N.P19) == (64, 32400, CX.P19)
    assert N.CALL_MIN_DEFAULT > N.DEEP_MIN_DEFAULT   # (more hypotheses: the largest noise score is larger)
    L = N.lib()
    for name, nargs in (("uwspr_calls_set", 5), ("uwspr_calls_batch", 5), ("uwspr_call_message", 4), ("uwspr_pipe_set_calls", 5)):
        assert name in N.ABI_SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert hasattr(L, "uwspr_debug_calls_time") and "uwspr_debug_calls_time" not in N.ABI_SYMBOLS
    assert callable(G.Context.calls) and callable(G.Context.calls_set) and callable(G.Pipe.set_calls) and callable(G.call_message)
    assert "2: list search, 3: call search" in hdr


def test_result_layout_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(sizeof(uwspr_call_result) == 32, \"result\");\n"
                   "static_assert(offsetof(uwspr_call_result, best) == 0 && offsetof(uwspr_call_result, call) == 4, \"result\");\n"
                   "static_assert(offsetof(uwspr_call_result, ngrid) == 8 && offsetof(uwspr_call_result, dbm) == 12, \"result\");\n"
                   "static_assert(offsetof(uwspr_call_result, sbest) == 16 && offsetof(uwspr_call_result, snext) == 20, \"result\");\n"
                   "static_assert(offsetof(uwspr_call_result, reserved) == 24, \"result\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112 && offsetof(uwspr_decode, osd) == 111, \"decode\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    R = G.native.CALL_RESULT_DTYPE
    assert R == CX.CALL_DTYPE and R.itemsize == 32
    assert [R.fields[k][1] for k in ("best", "call", "ngrid", "dbm", "sbest", "snext", "reserved")] == [0, 4, 8, 12, 16, 20, 24]


def test_set_rules_are_checked_before_any_device(G):
    N = G.native
    L = N.lib()
    params = N.Params(375, 45000, 256, 0, 200, 10, 1500, 10)
    h = C.c_void_p()
    L.uwspr_ctx_create(C.byref(params), 0, C.byref(h))   # without a device the call fails and still hands the context back
    assert h.value
    try:
        def call(calls, bitmap=None, pm=0, A=None):
            arr = (C.c_char_p * max(len(calls), 1))(*[c.encode() for c in calls])
            return L.uwspr_calls_set(h, arr, len(calls) if A is None else A, C.c_void_p(bitmap.ctypes.data) if bitmap is not None else None, pm)

        def err():
            return L.uwspr_last_error(h)

        assert call(["K1ABC", "W1AW", "k1abc"]) == ERR_ARG and b"twice" in err()
        assert call(["K1ABC", " K1ABC"]) == ERR_ARG
        assert call(["PJ4/K1ABC"]) == ERR_ARG and b"type-1" in err()
        assert call(["K1ABC/P"]) == ERR_ARG and b"type-1" in err()
        assert call(["<K1ABC>"]) == ERR_ARG and b"type-1" in err()
        assert call(["K1ABC", "NOCALL"]) == ERR_ARG and b"callsign 1" in err()
        many = CX.random_calls(np.random.Generator(np.random.Philox(0xCA110004)), 65)
        assert call(many) == ERR_ARG and b"1..64" in err()
        assert call(["K1ABC"], A=-1) == ERR_ARG
        assert L.uwspr_calls_set(h, None, 2, None, 0) == ERR_ARG
        assert call(["K1ABC"], bitmap=np.zeros(4050, np.uint8)) == ERR_ARG and b"empty" in err()
        assert call(["K1ABC"], pm=1 << 19) == ERR_ARG and b"power_mask" in err()
        assert L.uwspr_calls_set(None, None, 0, None, 0) == ERR_ARG
        # no set: the batch call is an argument error, with or without items; a clear of nothing is fine
        assert call([], A=0) == 0
        sym = np.full((2, 162), 128, np.uint8)
        res = np.zeros(2, N.CALL_RESULT_DTYPE)
        assert L.uwspr_calls_batch(h, C.c_void_p(sym.ctypes.data), 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG and b"no call set" in err()
        assert L.uwspr_calls_batch(h, None, 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_calls_batch(h, C.c_void_p(sym.ctypes.data), 2, N.HOST, None) == ERR_ARG
        assert L.uwspr_calls_batch(h, C.c_void_p(sym.ctypes.data), -1, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_calls_batch(h, C.c_void_p(sym.ctypes.data), 2, 7, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert L.uwspr_calls_batch(None, C.c_void_p(sym.ctypes.data), 2, N.HOST, C.c_void_p(res.ctypes.data)) == ERR_ARG
        assert not res.view(np.uint8).any()
        arr = (C.c_char_p * 1)(b"K1ABC")
        assert L.uwspr_pipe_set_calls(None, arr, 1, None, 0) == ERR_ARG
    finally:
        L.uwspr_ctx_destroy(h)


def test_a_power_outside_the_19_is_refused_in_python(G):
    for bad in ([36], [0, 61], [-3], [3.5]):
        with pytest.raises(G.UwsprError) as e:
            G.powers_mask(bad)
        assert e.value.status == ERR_ARG and "19" in str(e.value)
    with pytest.raises(G.UwsprError) as e:
        G.powers_mask([])
    assert e.value.status == ERR_ARG and "empty" in str(e.value)
