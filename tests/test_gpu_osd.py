"""Ordered-statistics decoding (K9, uwspr_osd_batch) against the binary restatement of its definition.

The definition (include/uwspr_hip.h, "ordered-statistics decoding") is all integers, so every comparison here is exact:
dmin, dnext, nhard, nflip and the 7 message bytes of every item, at orders 0, 1 and 2.  The restatement below is numpy
and nothing else: its own convolutional encoder (tests/test_osd_abi.py compares its generator matrix with 50 calls of
uwspr_fano_encode), its own de-interleave table, Gauss-Jordan on a 50 x 212 bit matrix and a full enumeration of the
flip sets.  tests/golden/osd_vectors.npz (tests/golden/make_osd_vectors.py) holds noisy encodings of packed messages
on which the host Fano decoder times out and the restated order 2 returns the transmitted message -- won with 0, 1
and 2 flips -- and as many noise-only vectors."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT32_MAX = 2 ** 31 - 1
NSYM, K = 162, 50
POLY1, POLY2 = 0xF2D05351, 0xE4613C47   # the code's two polynomials (Fano.cc:54-55)

OSD_DTYPE = np.dtype([("dmin", "<i4"), ("dnext", "<i4"), ("nhard", "<i4"), ("nflip", "u1"), ("message", "i1", (7,))])


# ---- the restatement --------------------------------------------------------------------------------------------------
def deint_src():
    """destination p of the de-interleaved vector takes source j: the bit-reversed 8-bit counter, values >= 162 skipped"""
    src, i = [], 0
    while len(src) < NSYM:
        j = int("{:08b}".format(i)[::-1], 2)
        if j < NSYM:
            src.append(j)
        i += 1
    return np.array(src)


def conv_encode(bits81):
    """the rate-1/2, K = 32 convolutional code: per input bit the parities of the shift register under the two polynomials"""
    state, out = 0, []
    for b in bits81:
        state = ((state << 1) | int(b)) & 0xFFFFFFFF
        out += [bin(state & POLY1).count("1") & 1, bin(state & POLY2).count("1") & 1]
    return np.array(out, np.uint8)


def generator():
    """G, 50 x 162 over GF(2): row j = the encoding of the 81-bit input with only bit j set"""
    g = np.zeros((K, NSYM), np.uint8)
    for j in range(K):
        b = np.zeros(81, np.uint8)
        b[j] = 1
        g[j] = conv_encode(b)
    return g


SRC = deint_src()
GEN = generator()
_IA, _IB = np.triu_indices(K, 1)   # the pairs (a, b), a < b, in lexicographic order


def pack_bits(bits50):
    """50 message bits -> the 7 bytes uwspr_fano_decode fills: bit j in byte j // 8, most significant bit first"""
    b = np.zeros(56, np.uint8)
    b[:K] = bits50
    return np.packbits(b).view(np.int8)


def osd_restate(symbols, order=2, parts=None):
    """One 162-byte soft-symbol vector as uwspr_demod_out.symbols[idt] holds it -> (dmin, dnext, nhard, nflip, message7).
    parts (a dict) receives the information set ("pivcol") and the de-interleaved hard bits / reliabilities."""
    s = np.asarray(symbols, np.uint8)[SRC].astype(np.int64)
    h = (s >= 128).astype(np.uint8)
    r = np.abs(2 * s - 255)
    perm = np.argsort(-r, kind="stable")           # reliability descending, ties by ascending index
    A = np.concatenate([GEN, np.eye(K, dtype=np.uint8)], axis=1)
    pivoted = np.zeros(K, bool)
    pivrow, pivcol = [], []
    for col in perm:
        rows = np.nonzero((A[:, col] == 1) & ~pivoted)[0]
        if rows.size == 0:
            continue                               # dependent on the columns taken so far
        p = rows[0]
        pivoted[p] = True
        others = np.nonzero(A[:, col])[0]
        A[others[others != p]] ^= A[p]
        pivrow.append(p)
        pivcol.append(col)
        if len(pivrow) == K:
            break
    assert len(pivrow) == K
    T, M = A[pivrow, :NSYM], A[pivrow, NSYM:]      # reduced rows in pivot order: code bits, and the message bits they stand for
    u = h[pivcol]
    c0 = (u.astype(np.int64) @ T) & 1
    m0 = (u.astype(np.int64) @ M) & 1
    z = (c0 ^ h).astype(np.uint8)
    E = [np.zeros((1, NSYM), np.uint8)]
    F = [np.zeros((1, K), np.uint8)]
    if order >= 1:
        E.append(T)
        F.append(M)
    if order >= 2:
        E.append(T[_IA] ^ T[_IB])
        F.append(M[_IA] ^ M[_IB])
    E, F = np.concatenate(E), np.concatenate(F)
    D = (E ^ z).astype(np.int64) @ r
    n = int(np.argmin(D))                          # the first minimum: fewer flips, then the lexicographically smaller set
    rest = np.delete(D, n)
    if parts is not None:
        parts.update(pivcol=np.array(pivcol), h=h, r=r, perm=perm)
    return (int(D[n]), int(rest.min()) if rest.size else INT32_MAX, int((E[n] ^ z).sum()),
            0 if n == 0 else (1 if n <= K else 2), pack_bits(m0.astype(np.uint8) ^ F[n]))


def restate_batch(symbols, order):
    out = np.zeros(len(symbols), OSD_DTYPE)
    for i, s in enumerate(symbols):
        out[i] = osd_restate(s, order)
    return out


def codeword_bytes(bits50, lo=0, hi=255):
    """an exact codeword as soft symbols (interleaved, as the demodulator writes them): lo for a 0, hi for a 1"""
    b = np.zeros(81, np.uint8)
    b[:K] = bits50
    c = conv_encode(b)
    sym = np.zeros(NSYM, np.uint8)
    sym[SRC] = np.where(c == 1, hi, lo)
    return sym


# ---- the inputs -------------------------------------------------------------------------------------------------------
def _message_bits(seed):
    return np.random.default_rng(seed).integers(0, 2, K).astype(np.uint8)


def _flip(sym, depos):
    """soft symbols with the bytes at the given DE-INTERLEAVED positions inverted"""
    out = sym.copy()
    for p in depos:
        out[SRC[p]] = 255 - out[SRC[p]]
    return out


def edge_vectors():
    """name -> (vector, expectation) for the constructed cases"""
    cases = {}
    bits = _message_bits(11)
    cw = codeword_bytes(bits)
    parts = {}
    osd_restate(cw, 0, parts)
    info = parts["pivcol"]   # all reliabilities equal: the information set is decided by the index alone
    cases["codeword"] = cw
    cases["one_flip"] = _flip(cw, [info[7]])
    cases["two_flips"] = _flip(cw, [info[3], info[31]])
    # dependent columns: the most reliable positions are 50 columns of rank < 50 -- the information set of the plain
    # codeword with its last member swapped for a column in the span of the first 49 -- so the elimination has to skip
    dep = None
    sub = GEN[:, info[:49]].astype(np.int64)
    for cnd in range(NSYM):
        if cnd in info:
            continue
        if _rank(np.concatenate([sub, GEN[:, [cnd]]], axis=1)) == 49:
            dep = cnd
            break
    assert dep is not None
    v = codeword_bytes(bits, 100, 155)
    for p in list(info[:49]) + [dep]:
        v[SRC[p]] = 255 if v[SRC[p]] >= 128 else 0
    cases["dependent"] = v
    # a value straddling 127 / 128: the least reliable pair, hard bits 0 and 1, reliability 1 both
    st = codeword_bytes(_message_bits(12), 40, 215)
    st[SRC[5]], st[SRC[6]], st[SRC[100]], st[SRC[101]] = 127, 128, 128, 127
    cases["straddle"] = st
    return cases, bits, info, dep


def _rank(m):
    m = m.copy() % 2
    rk = 0
    for c in range(m.shape[1]):
        rows = np.nonzero(m[rk:, c])[0]
        if rows.size == 0:
            continue
        p = rk + rows[0]
        m[[rk, p]] = m[[p, rk]]
        for q in np.nonzero(m[:, c])[0]:
            if q != rk:
                m[q] ^= m[rk]
        rk += 1
        if rk == m.shape[0]:
            break
    return rk


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "osd_vectors.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def pool(golden):
    """every vector of this file once, with its restated results at the three orders (computed once, never changed)"""
    cases, _, _, _ = edge_vectors()
    rng = np.random.default_rng(2026)
    rnd = np.clip(np.rint(128 + 40 * rng.standard_normal((12, NSYM))), 0, 255).astype(np.uint8)
    ties = (rng.integers(0, 4, (6, NSYM)) * 85).astype(np.uint8)   # four levels only: equal reliabilities and equal distances everywhere
    sym = np.concatenate([golden["signal"], golden["noise"], np.stack(list(cases.values())), rnd, ties])
    sym = np.ascontiguousarray(sym, np.uint8)
    ref = {o: restate_batch(sym, o) for o in (0, 1, 2)}
    for o in ref:
        ref[o].setflags(write=False)
    sym.setflags(write=False)
    return sym, ref, {k: len(golden["signal"]) + len(golden["noise"]) + i for i, k in enumerate(cases)}


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


def _same(got, exp):
    assert got.dtype == exp.dtype
    for k in exp.dtype.names:
        assert np.array_equal(got[k], exp[k]), (k, np.nonzero(np.any(np.atleast_2d(got[k] != exp[k]), axis=0))[0][:8] if got[k].ndim > 1
                                                 else np.nonzero(got[k] != exp[k])[0][:8])
    assert got.tobytes() == exp.tobytes()


# ---- the restatement's own sanity (no device) -------------------------------------------------------------------------
def test_restatement_constructed_cases():
    cases, bits, info, dep = edge_vectors()
    msg = pack_bits(bits).tobytes()
    d = osd_restate(cases["codeword"], 2)
    assert (d[0], d[2], d[3], d[4].tobytes()) == (0, 0, 0, msg) and d[1] > 0
    assert len(set(info)) == K
    d = osd_restate(cases["one_flip"], 1)
    assert (d[0], d[2], d[3], d[4].tobytes()) == (255, 1, 1, msg)
    assert osd_restate(cases["one_flip"], 0)[0] > 255
    d1, d2 = osd_restate(cases["two_flips"], 1), osd_restate(cases["two_flips"], 2)
    assert (d2[0], d2[2], d2[3], d2[4].tobytes()) == (510, 2, 2, msg)
    assert d1[0] > 510 and d1[4].tobytes() != msg          # order 2 wins, order 1 does not
    parts = {}
    d = osd_restate(cases["dependent"], 2, parts)
    assert dep in parts["perm"][:K] and len(set(parts["perm"][:K]) - set(parts["pivcol"])) == 1   # one of the first 50 columns was skipped
    assert (d[0], d[3], d[4].tobytes()) == (0, 0, msg)
    parts = {}
    osd_restate(cases["straddle"], 2, parts)
    assert parts["r"][5] == 1 and parts["r"][6] == 1 and parts["h"][5] == 0 and parts["h"][6] == 1
    assert list(parts["perm"][-4:]) == [5, 6, 100, 101]


def test_golden_vectors_are_what_they_claim(G, golden):
    """Fano times out on every signal vector; restated order 2 returns its message with 0 / 1 / 2 flips"""
    sig, msg, nf = golden["signal"], golden["message"], golden["nflip"]
    assert sig.shape[1] == NSYM and len(sig) == len(golden["noise"]) <= 32 and sig.dtype == np.uint8
    assert (nf == 2).sum() >= 8 and (nf == 1).sum() >= 8 and (nf == 0).sum() >= 4
    gap = int(golden["gap"])
    for s, m, f in zip(sig, msg, nf):
        assert G.fano_decode(G.deinterleave(s))[0] == -1
        d = osd_restate(s, 2)
        assert d[4].tobytes() == m.tobytes() and d[3] == f and d[1] - d[0] >= gap
        assert G.unpack_message(m)[0] == 0


# ---- the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1, 2])
def test_kernel_equals_restatement(ctx, pool, order):
    sym, ref, _ = pool
    _same(ctx.osd(sym, order=order), ref[order])


@pytest.mark.gpu
def test_constructed_cases_on_the_device(ctx, pool):
    sym, ref, at = pool
    got = {o: ctx.osd(sym, order=o) for o in (0, 1, 2)}
    cw, one, two = at["codeword"], at["one_flip"], at["two_flips"]
    for o in (0, 1, 2):
        assert got[o][cw]["dmin"] == 0 and got[o][cw]["nflip"] == 0 and got[o][cw]["nhard"] == 0
    assert got[0][cw]["dnext"] == INT32_MAX
    assert got[1][one]["dmin"] == 255 and got[1][one]["nflip"] == 1
    assert got[2][two]["dmin"] == 510 and got[2][two]["nflip"] == 2 and got[1][two]["dmin"] > 510
    assert got[2][two]["message"].tobytes() == got[2][cw]["message"].tobytes() != got[1][two]["message"].tobytes()
    assert got[2][at["dependent"]]["dmin"] == 0


@pytest.mark.gpu
def test_batches_are_independent(ctx, pool):
    sym, ref, _ = pool
    rng = np.random.default_rng(5)
    for n in (1, 63, 65, 300):
        idx = rng.integers(0, len(sym), n)
        _same(ctx.osd(sym[idx], order=2), ref[2][idx])
    assert len(ctx.osd(np.zeros((0, NSYM), np.uint8), order=2)) == 0


@pytest.mark.gpu
def test_host_and_device_pointers(ctx, pool):
    import torch
    sym, ref, _ = pool
    dev = torch.from_numpy(np.array(sym)).to("cuda:0")
    for o in (0, 1, 2):
        _same(ctx.osd(dev, order=o), ref[o])


@pytest.mark.gpu
def test_argument_errors(G, ctx, pool):
    import ctypes as C
    N = G.native
    sym = np.array(pool[0][:4])
    res = np.zeros(4, OSD_DTYPE)
    sp, rp = C.c_void_p(sym.ctypes.data), C.c_void_p(res.ctypes.data)
    L = ctx.L
    assert L.uwspr_osd_batch(None, sp, 4, N.HOST, 2, rp) == -6
    for order in (-1, 3):
        assert L.uwspr_osd_batch(ctx.h, sp, 4, N.HOST, order, rp) == -6
    assert L.uwspr_osd_batch(ctx.h, sp, -1, N.HOST, 2, rp) == -6
    assert L.uwspr_osd_batch(ctx.h, None, 4, N.HOST, 2, rp) == -6
    assert L.uwspr_osd_batch(ctx.h, sp, 4, N.HOST, 2, None) == -6
    assert L.uwspr_osd_batch(ctx.h, sp, 4, N.DEVICE_FRAMES, 2, rp) == -6
    assert L.uwspr_osd_batch(ctx.h, sp, 4, N.DEVICE, 2, rp) == -6      # host pointers called device memory: refused before any launch
    assert L.uwspr_osd_batch(ctx.h, None, 0, N.HOST, 2, None) == 0     # nothing to do is fine
    assert not res.tobytes().strip(b"\0")
    with pytest.raises(G.UwsprError):
        ctx.osd(sym, order=3)
    _same(ctx.osd(sym, order=2), pool[1][2][:4])                        # the context is unharmed
