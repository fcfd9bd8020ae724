"""The transmit side's host half (no GPU): WSPR message packing, the type 3 hash, wsprsim's channel symbols and the
.c2 writer.  uwspr_unpack_message -- pinned against the reference's unpk_ -- is the specification of the packer."""
import ctypes as C
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POWERS = [p for p in range(61) if p % 10 in (0, 3, 7)]
CALLS = ["K1A", "K1AB", "K1ABC", "KA1A", "KA1AB", "VE3EMB", "G4X", "2E0AB", "4X1ABC", "W9ZZZ"]
GRIDS = ["AA00", "RR99", "FN25", "JO01"]
COMPOUND = ["PJ4/K1ABC", "Q/K1A", "AB3/G4XYZ", "4X/VE3EMB", "K1ABC/7", "K1ABC/P", "VE3EMB/Z", "K1ABC/12", "G4XYZ/99"]


def _corpus():
    out = []
    for i, p in enumerate(POWERS):
        for j, call in enumerate(CALLS):
            grid = GRIDS[(i + j) % len(GRIDS)]
            out.append(("%s %s %d" % (call, grid, p), "%s %s %2d" % (call, grid, p), 1))
        for call in COMPOUND:
            out.append(("%s %d" % (call, p), "%s %2d" % (call, p), 2))
        out.append(("<PJ4/K1ABC> FN42AX %d" % p, "<...> FN42AX %2d" % p, 3))
    return out


def test_pack_round_trip_over_the_corpus(G, oracle):
    have_ref = oracle.ref() is not None
    for text, want, kind in _corpus():
        m = G.wspr_pack(text)
        rc, got = G.unpack_message(m)
        assert rc == 0 and got == want, (text, got)
        if have_ref and kind in (1, 2):
            assert oracle.ref_unpk(m) == want, (text, oracle.ref_unpk(m))
        assert (G.wspr_pack(text.lower()) == m).all()


def test_pack_rejects_bad_text_without_partial_output(G):
    bad = ["K1ABC FN42 38", "K1ABC FN42 63", "K1ABC FN42 -3", "K1ABC SS42 30", "K1ABC FN4 30", "KABC FN42 30",
           "K1ABCDE FN42 30", "K1 FN42 30", "", "K1ABC FN42", "K1ABC FN42 30 X", "<K1ABC> FN42 30", "<K1ABC> FN42AZ 30",
           "K1ABC/123 30", "K1ABC/05 30", "ABCD/K1ABC 30", "K1ABC/7 31", "K1-BC FN42 30", "<> FN42AA 30"]
    L = G.native.lib()
    for t in bad:
        with pytest.raises(G.UwsprError) as e:
            G.wspr_pack(t)
        assert e.value.status == -6, t
        m = np.full(7, 0x55, np.int8)
        assert L.uwspr_wspr_pack(t.encode(), C.c_void_p(m.ctypes.data)) == -6
        assert (m == 0x55).all(), t


def test_type3_hash_is_lookup3(G):
    # the self-test values lookup3.c's driver5() prints for hashlittle()
    assert G.nhash(b"", 0) == 0xDEADBEEF
    assert G.nhash(b"", 0xDEADBEEF) == 0xBD5B7DDE
    assert G.nhash(b"Four score and seven years ago", 0) == 0x17770551
    assert G.nhash(b"Four score and seven years ago", 1) == 0xCD628161
    # and it is what a type 3 message carries: n2 = 128 (hash & 32767) - (dBm + 1) + 64
    for call, p in (("PJ4/K1ABC", 37), ("VE3EMB", 30), ("K1A", 0)):
        d = G.wspr_pack("<%s> FN25AB %d" % (call, p)).view(np.uint8).astype(np.int64)
        n2 = ((d[3] & 15) << 18) | (d[4] << 10) | (d[5] << 2) | (d[6] >> 6)
        assert (n2 + p + 1 - 64) % 128 == 0
        assert (n2 + p + 1 - 64) // 128 == G.nhash(call, 146) & 32767


def _symbols_of_c2(G, path):
    iq, _, _ = G.c2_read(path)
    x = iq[:, 0].astype(np.float64) + 1j * iq[:, 1]
    seg = x[375:375 + 162 * 256]
    dphi = np.angle(seg[1:] * np.conj(seg[:-1]))
    dphi = np.concatenate([dphi, [0.0]]).reshape(162, 256)[:, :255].mean(axis=1)
    return np.rint(dphi / (2 * np.pi / 256) + 1.5).astype(np.uint8)


def test_ve3emb_symbols_are_the_recorded_transmission(G):
    sym = G.wspr_symbols("VE3EMB FN25 30")
    assert sym.shape == (162,) and sym.max() <= 3
    assert (sym == _symbols_of_c2(G, os.path.join(GOLDEN, "VE3EMB.c2"))).all()
    assert (G.wspr_symbols(G.wspr_pack("VE3EMB FN25 30")) == sym).all()
    soft = G.deinterleave(((sym >> 1) * 255).astype(np.uint8))
    rc, data, _, _ = G.fano_decode(soft)
    assert rc == 0 and (data[:7].view(np.int8) == G.wspr_pack("VE3EMB FN25 30")).all()
    assert G.unpack_message(data[:7].view(np.int8))[1] == "VE3EMB FN25 30"
    assert ((sym & 1) == G.synth.PR3).all()


def test_c2_write_is_the_inverse_of_c2_read(G, tmp_path):
    iq, freq, typ = G.c2_read(os.path.join(GOLDEN, "VE3EMB.c2"))
    p = str(tmp_path / "VE3EMB.c2")
    G.write_c2(p, iq, dial_freq=freq, type=typ)
    iq2, freq2, typ2 = G.c2_read(p)
    assert (iq2 == iq).all() and freq2 == freq and typ2 == typ
    # the bytes after the name are the reference file's
    assert open(p, "rb").read()[14:] == open(os.path.join(GOLDEN, "VE3EMB.c2"), "rb").read()[14:]
    assert open(p, "rb").read()[:14] == b"VE3EMB.c2" + b"\0" * 5
    rng = np.random.default_rng(7)
    r = rng.standard_normal((45000, 2)).astype(np.float32)
    G.write_c2(p, r, dial_freq=14.0956, type=7)
    r2, f2, t2 = G.c2_read(p)
    assert (r2 == r).all() and f2 == 14.0956 and t2 == 7
    with pytest.raises(G.UwsprError):
        G.write_c2(p, r[:100])
