"""Ordered-statistics decoding, the parts a machine without a GPU can check: uwspr_osd_batch is declared, exported and
bound; uwspr_osd_result has the layout the header gives it in C and in numpy; uwspr_decode is still 112 bytes with `osd`
in its last byte (offset 111); the restatement's generator matrix is 50 calls of uwspr_fano_encode."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_osd import GEN, SRC, K, NSYM, OSD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")


def test_entry_point_is_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    assert re.search(r"int uwspr_osd_batch\(uwspr_ctx \*ctx, const uint8_t \*symbols /\*\[n\]\[162\]\*/, int n, int where, "
                     r"int order, uwspr_osd_result \*res\);", hdr)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m and int(m.group(1)) == 6
    entry6 = m.group(2).split("6:")[1]
    for name in ("uwspr_osd_batch", "uwspr_osd_result", "uwspr_decode.osd", '"osd"', '"osd_gap"'):
        assert name in entry6, name
    d = re.search(r"#define UWSPR_OSD_GAP_DEFAULT (\d+)", hdr)
    assert d and int(d.group(1)) == G.native.OSD_GAP_DEFAULT
    assert "uwspr_osd_batch" in G.native.ABI_SYMBOLS
    L = G.native.lib()
    assert hasattr(L, "uwspr_osd_batch") and len(L.uwspr_osd_batch.argtypes) == 6
    assert callable(G.Context.osd)


def test_record_layouts_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(sizeof(uwspr_osd_result) == 20, \"result\");\n"
                   "static_assert(offsetof(uwspr_osd_result, dmin) == 0 && offsetof(uwspr_osd_result, dnext) == 4, \"result\");\n"
                   "static_assert(offsetof(uwspr_osd_result, nhard) == 8 && offsetof(uwspr_osd_result, nflip) == 12, \"result\");\n"
                   "static_assert(offsetof(uwspr_osd_result, message) == 13, \"result\");\n"
                   "static_assert(sizeof(((uwspr_osd_result *)0)->message) == 7, \"message\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112, \"decode\");\n"
                   "static_assert(offsetof(uwspr_decode, channel) == 108 && offsetof(uwspr_decode, pass) == 110, \"decode\");\n"
                   "static_assert(offsetof(uwspr_decode, osd) == 111, \"osd\");\n"
                   "static_assert(sizeof(((uwspr_decode *)0)->osd) == 1, \"uint8\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    N = G.native
    R = N.OSD_RESULT_DTYPE
    assert R == OSD_DTYPE and R.itemsize == 20
    assert [R.fields[k][1] for k in ("dmin", "dnext", "nhard", "nflip", "message")] == [0, 4, 8, 12, 13]
    D = N.DECODE_DTYPE
    assert D.itemsize == 112 and D.fields["channel"][1] == 108 and D.fields["pass"][1] == 110
    assert D.fields["osd"][1] == 111 and D.fields["osd"][0] == np.dtype("u1")
    rec = np.zeros(1, D)
    rec["osd"] = 1
    assert rec.tobytes()[111] == 1 and sum(rec.tobytes()) == 1


def test_generator_is_fifty_calls_of_the_encoder(G):
    for j in range(K):
        data = np.zeros(11, np.uint8)
        data[j >> 3] = 0x80 >> (j & 7)
        assert np.array_equal(G.fano_encode(data)[:NSYM], GEN[j]), j
    assert np.linalg.matrix_rank(GEN.astype(float)) == K   # (rank over the reals bounds the GF(2) rank from above only; the elimination asserts 50)
    idx = np.arange(NSYM, dtype=np.uint8)
    assert np.array_equal(G.deinterleave(idx), SRC)
