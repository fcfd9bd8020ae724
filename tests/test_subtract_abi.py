"""Known-symbol subtraction, the parts a machine without a GPU can check: uwspr_subtract_batch is declared, exported and
bound; uwspr_sub_item / uwspr_sub_result have the layout the header gives them in C and in numpy; uwspr_decode is still
112 bytes with `pass` where the second byte-pair of padding began (offset 110).

The issue's struct (two int32, two float, 162 symbols, 2 bytes of padding) is 180 bytes, not the 176 its test list
names (176 is uwspr_sync_result, which has one field fewer): the layout of the struct as written is what is pinned."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")


def test_entry_point_is_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    assert re.search(r"int uwspr_subtract_batch\(uwspr_ctx \*ctx, const float \*frames, int B, int where, "
                     r"const uwspr_sub_item \*items, int nitems,\s+int refine, float \*frames_out, uwspr_sub_result \*res\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m and int(m.group(1)) == 6
    entry6 = m.group(2).split("6:")[1]
    for name in ("uwspr_subtract_batch", "uwspr_sub_item", "uwspr_sub_result", "uwspr_decode.pass", '"passes"'):
        assert name in entry6, name
    assert "uwspr_subtract_batch" in G.native.ABI_SYMBOLS
    L = G.native.lib()
    assert hasattr(L, "uwspr_subtract_batch") and len(L.uwspr_subtract_batch.argtypes) == 9
    assert callable(G.Context.subtract) and callable(G.sub_items)


def test_record_layouts_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(sizeof(uwspr_sub_item) == 180, \"item\");\n"
                   "static_assert(offsetof(uwspr_sub_item, shift) == 4 && offsetof(uwspr_sub_item, f_hz) == 8, \"item\");\n"
                   "static_assert(offsetof(uwspr_sub_item, drift_hz) == 12 && offsetof(uwspr_sub_item, symbols) == 16, \"item\");\n"
                   "static_assert(sizeof(uwspr_sub_result) == 16, \"result\");\n"
                   "static_assert(offsetof(uwspr_sub_result, shift) == 4 && offsetof(uwspr_sub_result, metric) == 8, \"result\");\n"
                   "static_assert(offsetof(uwspr_sub_result, removed) == 12, \"result\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112, \"decode\");\n"
                   "static_assert(offsetof(uwspr_decode, channel) == 108, \"channel\");\n"
                   "static_assert(offsetof(uwspr_decode, pass) == 110, \"pass\");\n"
                   "static_assert(sizeof(((uwspr_decode *)0)->pass) == 1, \"uint8\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N = G.native
    assert N.SUB_ITEM_DTYPE.itemsize == 180 and N.SUB_RESULT_DTYPE.itemsize == 16
    assert [N.SUB_ITEM_DTYPE.fields[k][1] for k in ("frame", "shift", "f_hz", "drift_hz", "symbols")] == [0, 4, 8, 12, 16]
    assert [N.SUB_RESULT_DTYPE.fields[k][1] for k in ("f_hz", "shift", "metric", "removed")] == [0, 4, 8, 12]
    D = N.DECODE_DTYPE
    assert D.itemsize == 112 and D.fields["channel"][1] == 108
    assert D.fields["pass"][1] == 110 and D.fields["pass"][0] == np.dtype("u1")
    rec = np.zeros(1, D)
    rec["pass"] = 1
    assert rec.tobytes()[110] == 1 and sum(rec.tobytes()) == 1


def test_items_from_dicts(G):
    sym = G.wspr_symbols("K1ABC FN42 37")
    it = G.sub_items([{"frame": 2, "shift": -40, "f": 1.25, "text": "K1ABC FN42 37"},
                      {"frame": 3, "shift": 7, "f": -2.0, "drift": 0.5, "symbols": sym[::-1]}])
    assert it.dtype == G.native.SUB_ITEM_DTYPE and len(it) == 2
    assert (it["frame"].tolist(), it["shift"].tolist(), it["f_hz"].tolist(), it["drift_hz"].tolist()) == \
        ([2, 3], [-40, 7], [1.25, -2.0], [0.0, 0.5])
    assert np.array_equal(it[0]["symbols"], sym) and np.array_equal(it[1]["symbols"], sym[::-1])
    assert G.sub_items(it) is it or np.array_equal(G.sub_items(it), it)
