"""Block demodulation, the parts a machine without a GPU can check: uwspr_blockdemod_batch is declared, exported and bound;
uwspr_block_item has the layout the header gives it in C and in numpy; uwspr_decode is still 112 bytes with `block` in the
byte that was _pad0 (offset 107)."""
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
    assert re.search(r"int uwspr_blockdemod_batch\(uwspr_ctx \*ctx, const float \*frames, int B, int where, "
                     r"const uwspr_block_item \*items, int nitems,\s+uint8_t \*symbols /\*\[nitems\]\[3\]\[162\]\*/\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m and int(m.group(1)) == 6
    entry6 = m.group(2).split("6:")[1]
    for name in ("uwspr_blockdemod_batch", "uwspr_block_item", "uwspr_decode.block", '"block"'):
        assert name in entry6, name
    assert "uwspr_blockdemod_batch" in G.native.ABI_SYMBOLS
    L = G.native.lib()
    assert hasattr(L, "uwspr_blockdemod_batch") and len(L.uwspr_blockdemod_batch.argtypes) == 7
    assert callable(G.Context.blockdemod)


def test_record_layouts_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(sizeof(uwspr_block_item) == 16, \"item\");\n"
                   "static_assert(offsetof(uwspr_block_item, frame) == 0 && offsetof(uwspr_block_item, shift) == 4, \"item\");\n"
                   "static_assert(offsetof(uwspr_block_item, f_hz) == 8 && offsetof(uwspr_block_item, drift_hz) == 12, \"item\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112, \"decode\");\n"
                   "static_assert(offsetof(uwspr_decode, block) == 107, \"block\");\n"
                   "static_assert(sizeof(((uwspr_decode *)0)->block) == 1, \"uint8\");\n"
                   "static_assert(offsetof(uwspr_decode, message) == 100 && offsetof(uwspr_decode, channel) == 108, \"decode\");\n"
                   "static_assert(offsetof(uwspr_decode, pass) == 110 && offsetof(uwspr_decode, osd) == 111, \"decode\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N = G.native
    I = N.BLOCK_ITEM_DTYPE
    assert I.itemsize == 16 and [I.fields[k][1] for k in ("frame", "shift", "f_hz", "drift_hz")] == [0, 4, 8, 12]
    D = N.DECODE_DTYPE
    assert D.itemsize == 112 and D.fields["block"][1] == 107 and D.fields["block"][0] == np.dtype("u1")
    assert D.fields["message"][1] == 100 and D.fields["channel"][1] == 108 and D.fields["osd"][1] == 111
    rec = np.zeros(1, D)
    rec["block"] = 3
    assert rec.tobytes()[107] == 3 and sum(rec.tobytes()) == 3


def test_items_from_dicts(G):
    arr = G.block_items([{"frame": 2, "shift": -7, "f": 1.5, "drift": -2.0}, {"frame": 3, "shift": 375, "f": 0.25}])
    assert arr.dtype == G.native.BLOCK_ITEM_DTYPE and arr.tobytes() == np.array(
        [(2, -7, 1.5, -2.0), (3, 375, 0.25, 0.0)], G.native.BLOCK_ITEM_DTYPE).tobytes()
    assert G.block_items(arr) is not None and len(G.block_items([])) == 0
