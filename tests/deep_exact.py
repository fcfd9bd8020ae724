"""The numpy restatement of the list search (K13, uwspr_deep_batch; include/uwspr_hip.h states the definition), int64
throughout.  The code table comes from the generator matrix -- 50 rows, wspr_symbols of the single-bit messages -- and
not from one wspr_symbols call per message, which is how the library builds its table."""
import numpy as np

NSYM, K = 162, 50
DEEP_DTYPE = np.dtype([("best", "<i4"), ("sbest", "<i4"), ("snext", "<i4"), ("reserved", "<i4")])
INT32_MIN = -2 ** 31
_GEN = None


def generator(G):
    """[50, 162] uint8: row j = the code bits of the message with only bit j set (bit j: byte j // 8, most significant first)"""
    global _GEN
    if _GEN is None:
        assert not (G.wspr_symbols(np.zeros(7, np.int8)) >> 1).any()   # the code is linear: the zero message has no code bit set
        rows = []
        for j in range(K):
            m = np.zeros(7, np.uint8)
            m[j >> 3] = 0x80 >> (j & 7)
            rows.append(G.wspr_symbols(m.view(np.int8)) >> 1)
        _GEN = np.stack(rows).astype(np.uint8)
    return _GEN


def code_table(G, messages):
    """messages [M, 7] int8 -> [M, 162] int64 of 0 / 1: the XOR of the generator's rows at the set message bits (per message
    byte, a 256-entry table of row combinations)"""
    gen = generator(G)
    msgs = np.ascontiguousarray(messages, np.int8).reshape(-1, 7).view(np.uint8)
    out = np.zeros((len(msgs), NSYM), np.uint8)
    for byte in range(7):
        lut = np.zeros((256, NSYM), np.uint8)
        for bit in range(8):
            j = 8 * byte + bit
            if j >= K:
                break
            on = ((np.arange(256) >> (7 - bit)) & 1).astype(bool)
            lut[on] ^= gen[j]
        out ^= lut[msgs[:, byte]]
    return out.astype(np.int64)


def scores(table, symbols):
    """S[i, m] = sum_p (2 c[m][p] - 1) (s[i][p] - 128): [n, M] int64"""
    s = np.ascontiguousarray(symbols, np.uint8).reshape(-1, NSYM).astype(np.int64) - 128
    return s @ (2 * np.asarray(table, np.int64) - 1).T


def deep_restate(table, symbols):
    """-> DEEP_DTYPE [n]: best = the m with the largest S (the smallest m on ties), sbest, snext = the largest S over
    m != best (INT32_MIN when M = 1), reserved = 0"""
    S = scores(table, symbols)
    n, M = S.shape
    res = np.zeros(n, DEEP_DTYPE)
    best = S.argmax(axis=1)               # (the first maximum)
    res["best"] = best
    res["sbest"] = S[np.arange(n), best]
    if M == 1:
        res["snext"] = INT32_MIN
    else:
        S[np.arange(n), best] = np.iinfo(np.int64).min
        res["snext"] = S.max(axis=1)
    return res


def random_messages(rng, M):
    """M distinct random 50-bit messages as [M, 7] int8 (the low 6 bits of byte 6 zero)"""
    out = np.zeros((0, 7), np.uint8)
    while len(out) < M:
        m = rng.integers(0, 256, (M - len(out) + 16, 7), dtype=np.uint8)
        m[:, 6] &= 0xC0
        out = np.concatenate([out, m])
        _, first = np.unique(out, axis=0, return_index=True)
        out = out[np.sort(first)]
    return np.ascontiguousarray(out[:M]).view(np.int8)


def accepted(res, M, deep_min, deep_gap):
    """the pipe's rule for one result"""
    return int(res["sbest"]) >= deep_min and (M == 1 or int(res["sbest"]) - int(res["snext"]) >= deep_gap)
