"""The numpy restatement of the call search (K14, uwspr_calls_batch; include/uwspr_hip.h states the definition).

A type-1 message is n1 (28 bits, the callsign) and n2 = 128 ngrid + dBm + 64 (22 bits); ngrid < 2^15 and dBm + 64 < 128, so
callsign, locator and power sit in disjoint bits of the 50, and the code is linear: the code bits of "CALL GRID dBm" are
the XOR of those of the callsign alone, the locator alone and the power alone.  With signs 2 c - 1 the XOR is a product, so
    S[a, g, d] = sum_p call_sign[a][p] power_sign[d][p] grid_sign[g][p] (s[p] - 128):
one [32400, 162] table for every callsign and power.  The partial tables come from tests/deep_exact.py's generator matrix
(wspr_symbols of the single-bit messages).  The products run through a float64 matrix product -- every term and sum is an
integer below 2^15, far inside 2^53, so it is exact -- and everything after it is int64."""
import numpy as np

import deep_exact as X

NSYM, NGRID, NPOW, CALLS_MAX = 162, 32400, 19, 64
P19 = (0, 3, 7, 10, 13, 17, 20, 23, 27, 30, 33, 37, 40, 43, 47, 50, 53, 57, 60)
ALL_POWERS = (1 << NPOW) - 1
CALL_DTYPE = np.dtype([("best", "<i4"), ("call", "<i4"), ("ngrid", "<i4"), ("dbm", "<i4"), ("sbest", "<i4"), ("snext", "<i4"),
                       ("reserved", "<i4", (2,))])
INT32_MIN = -2 ** 31
_GRID = None


def put50(n1, n2):
    """(n1, n2) -> the 7 message bytes [.., 7] int8, as uwspr_wspr_pack lays them out"""
    n1, n2 = np.asarray(n1, np.int64), np.asarray(n2, np.int64)
    m = np.stack([n1 >> 20, n1 >> 12, n1 >> 4, ((n1 & 15) << 4) | ((n2 >> 18) & 15), n2 >> 10, n2 >> 2, (n2 & 3) << 6], axis=-1)
    return np.ascontiguousarray((m & 255).astype(np.uint8)).view(np.int8)


def call_n1(G, call):
    """the 28 callsign bits of a type-1 message with this callsign"""
    b = G.wspr_pack("%s AA00 0" % call).view(np.uint8).astype(np.int64)
    return int((b[0] << 20) | (b[1] << 12) | (b[2] << 4) | (b[3] >> 4))


def grid_ngrid(grid4):
    g = grid4.upper()
    return 180 * (179 - 10 * (ord(g[0]) - 65) - (ord(g[2]) - 48)) + 10 * (ord(g[1]) - 65) + (ord(g[3]) - 48)


def ngrid_grid(ngrid):
    lon, lat = 179 - ngrid // 180, ngrid % 180
    return "%c%c%d%d" % (65 + lon // 10, 65 + lat // 10, lon % 10, lat % 10)


def grid_bits(G):
    """[32400, 162] int8 of 0 / 1: the code bits of the messages with only ngrid = g set"""
    global _GRID
    if _GRID is None:
        _GRID = X.code_table(G, put50(np.zeros(NGRID, np.int64), 128 * np.arange(NGRID))).astype(np.int8)
    return _GRID


def power_bits(G):
    """[19, 162] of 0 / 1: the messages with only dBm + 64 set"""
    return X.code_table(G, put50(np.zeros(NPOW, np.int64), np.asarray(P19) + 64))


def call_bits(G, calls):
    """[A, 162] of 0 / 1: the messages with only the callsign set"""
    return X.code_table(G, put50(np.array([call_n1(G, c) for c in calls], np.int64), np.zeros(len(calls), np.int64)))


def split_h(h):
    """h -> (call index, ngrid, index into P19)"""
    return h // (NGRID * NPOW), (h // NPOW) % NGRID, h % NPOW


def join_h(a, g, d):
    return (a * NGRID + g) * NPOW + d


def message(G, call, ngrid, dbm):
    """message(h) composed from its numbers"""
    return put50(call_n1(G, call), 128 * ngrid + dbm + 64)


def grids_bitmap(grids):
    """the "grids" spec -> the [4050] uint8 bitmap over ngrid (bit g: byte g >> 3, bit g & 7); None: all"""
    bm = np.zeros(NGRID // 8, np.uint8)
    if grids is None:
        bm[:] = 255
        return bm
    for s in grids:
        s = s.upper()
        cells = [s] if len(s) == 4 else ["%s%d%d" % (s, i, j) for i in range(10) for j in range(10)]
        for c in cells:
            g = grid_ngrid(c)
            bm[g >> 3] |= 1 << (g & 7)
    return bm


def bitmap_list(bitmap):
    bm = np.full(NGRID // 8, 255, np.uint8) if bitmap is None else np.asarray(bitmap, np.uint8)
    return np.flatnonzero(np.unpackbits(bm, bitorder="little")[:NGRID])


def power_list(power_mask):
    pm = ALL_POWERS if not power_mask else int(power_mask)
    return np.array([d for d in range(NPOW) if pm >> d & 1], np.int64)


def powers_mask(powers):
    return ALL_POWERS if powers is None else sum(1 << P19.index(int(p)) for p in set(powers))


def scores(G, calls, gl, dl, symbols):
    """S[i, a, g, d] over the allowed locators gl and power indices dl: [n, A, len(gl), len(dl)] int64"""
    s = np.ascontiguousarray(symbols, np.uint8).reshape(-1, NSYM).astype(np.float64) - 128.0
    sg = 2.0 * grid_bits(G)[gl].astype(np.float64) - 1.0                                   # [g, 162]
    sa, sd = 2.0 * call_bits(G, calls) - 1.0, 2.0 * power_bits(G)[dl] - 1.0                # [A, 162], [d, 162]
    x = s[:, None, None, :] * sa[None, :, None, :] * sd[None, None, :, :]                  # [n, A, d, 162]
    S = x.reshape(-1, NSYM) @ sg.T                                                         # [n A d, g]
    return np.rint(S).astype(np.int64).reshape(len(s), len(calls), len(dl), len(gl)).transpose(0, 1, 3, 2)


def call_restate(G, calls, grid_bitmap, power_mask, symbols):
    """-> CALL_DTYPE [n]: best = the allowed h with the largest S (the smallest h on ties), its parts, sbest, snext = the
    largest S over the other allowed h (INT32_MIN with a single hypothesis), reserved = 0"""
    gl, dl = bitmap_list(grid_bitmap), power_list(power_mask)
    sym = np.ascontiguousarray(symbols, np.uint8).reshape(-1, NSYM)
    res = np.zeros(len(sym), CALL_DTYPE)
    step = max(1, (1 << 25) // (len(calls) * len(gl) * len(dl)))
    for i0 in range(0, len(sym), step):
        S = scores(G, calls, gl, dl, sym[i0:i0 + step])
        n = len(S)
        flat = S.reshape(n, -1)                       # (a, g, d) in the order of h: the first maximum is the smallest h
        k = flat.argmax(axis=1)
        a, gi, di = np.unravel_index(k, S.shape[1:])
        r = res[i0:i0 + n]
        r["call"], r["ngrid"], r["dbm"] = a, gl[gi], np.asarray(P19)[dl[di]]
        r["best"] = join_h(a, gl[gi], dl[di])
        r["sbest"] = flat[np.arange(n), k]
        if flat.shape[1] == 1:
            r["snext"] = INT32_MIN
        else:
            flat[np.arange(n), k] = np.iinfo(np.int64).min
            r["snext"] = flat.max(axis=1)
    return res


def accepted(res, nhyp, call_min, call_gap):
    """the pipe's rule for one result (nhyp: the number of allowed hypotheses)"""
    return int(res["sbest"]) >= call_min and (nhyp == 1 or int(res["sbest"]) - int(res["snext"]) >= call_gap)


def random_calls(rng, A):
    """A distinct random callsigns of 3 to 6 characters that uwspr_wspr_pack takes"""
    L, D = "ABCDEFGHIJKLMNOPQRSTUVWXYZ", "0123456789"
    out = []
    while len(out) < A:
        pre = rng.choice(list(L)) + (rng.choice(list(L + D)) if rng.integers(2) else "")
        c = pre + rng.choice(list(D)) + "".join(rng.choice(list(L)) for _ in range(int(rng.integers(1, 4))))
        if c not in out:
            out.append(c)
    return out
