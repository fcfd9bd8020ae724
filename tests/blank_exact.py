"""The noise blanker K12 restated in numpy from the text of include/uwspr_hip.h ("impulsive noise"), on the uint32 views
of the samples: what tests/test_gpu_blank*.py compare the device's bytes with.  No GPU, no library.

    u(i)   = bits(x[i]) & 0x7fffffff
    med(b) = rank N/2 - 1 of the u of block b (complete blocks)
    thr(b) = fl32(fl32((float) blank * med(b - 1)) * 0.25f)     none for b = 0, med(b - 1) = 0, >= 0x7f800000
    flag(i) = u(i) > bits(thr(block(i)))                        y[i] = +0 if a flag in [i - G, i + G] else x[i]

The keyword arguments of `blank` other than blank and guard are MUTATIONS for tests/test_blank.py: each restates a
plausible misreading of the text, and the tests show that the inputs they use tell it from the definition.
"""
import numpy as np

N = 4096
ABS = np.uint32(0x7fffffff)
INF = np.uint32(0x7f800000)


def as_float(x):
    """the float32 value of every sample: int16 counts as s / 32768, exactly"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(1.0 / 32768)
    assert x.dtype == np.float32, x.dtype
    return x


def patterns(xf):
    return np.ascontiguousarray(xf).view(np.uint32) & ABS


def levels(x, rank=N // 2 - 1):
    """-> med [nblocks, C] as uint32 patterns: the level of every complete block, 0 for a trailing partial one"""
    xf = as_float(x)
    xf = xf.reshape(xf.shape[0], -1)
    u = patterns(xf)
    n, nb = u.shape[0], -(-u.shape[0] // N)
    med = np.zeros((nb, u.shape[1]), np.uint32)
    for b in range(n // N):
        med[b] = np.partition(u[b * N:(b + 1) * N], rank, axis=0)[rank]
    return med


def thresholds(med, blank, own_block=False):
    """-> (thr [nblocks, C] uint32 patterns, has [nblocks, C] bool): the threshold of the samples OF block b"""
    src = med if own_block else np.concatenate([np.zeros((1,) + med.shape[1:], np.uint32), med[:-1]])
    has = (src != 0) & (src < INF)
    if not own_block and med.shape[0]:
        has[0] = False
    with np.errstate(over="ignore", invalid="ignore"):
        t = (np.float32(blank) * src.view(np.float32)).astype(np.float32)
        t = (t * np.float32(0.25)).astype(np.float32)
    return t.view(np.uint32), has


def flags(x, blank, rank=N // 2 - 1, own_block=False, ge=False):
    xf = as_float(x)
    xf = xf.reshape(xf.shape[0], -1)
    u = patterns(xf)
    thr, has = thresholds(levels(xf, rank), blank, own_block)
    blk = np.arange(u.shape[0]) // N
    t, h = thr[blk], has[blk]
    return h & ((u >= t) if ge else (u > t))


def dilate(f, guard, guard_stops=False):
    """f [n, C] bool -> whether any j with |j - i| <= guard, 0 <= j < n, has f[j]"""
    n, C = f.shape
    c = np.concatenate([np.zeros((1, C), np.int64), np.cumsum(f, axis=0, dtype=np.int64)])
    i = np.arange(n)
    lo, hi = np.maximum(i - guard, 0), np.minimum(i + guard, n - 1)
    if guard_stops:   # (mutation: the guard ends at the edge of the sample's block)
        lo, hi = np.maximum(lo, i // N * N), np.minimum(hi, i // N * N + N - 1)
    return (c[hi + 1] - c[lo]) > 0


def blank(x, blank=24, guard=2, rank=N // 2 - 1, own_block=False, guard_stops=False, ge=False):
    """-> (y float32 like x, med float32 [nblocks(, C)], nzero int32 [nblocks(, C)]): uwspr_blank_batch"""
    x = np.asarray(x)
    xf = as_float(x)
    x2 = xf.reshape(xf.shape[0], -1)
    n, C = x2.shape
    hit = dilate(flags(x2, blank, rank, own_block, ge), guard, guard_stops)
    y = np.where(hit, np.float32(0.0), x2).astype(np.float32)
    nb = -(-n // N)
    nz = np.zeros((nb, C), np.int32)
    for b in range(nb):
        nz[b] = hit[b * N:(b + 1) * N].sum(axis=0)
    med = levels(x2, N // 2 - 1).view(np.float32)   # (the level the call reports is the definition's, whatever rank the flags used)
    tail = x.shape[1:]
    return y.reshape(x.shape), med.reshape((nb,) + tail), nz.reshape((nb,) + tail)


def stream(x, blank_=24, guard=2):
    """what a stream that was pushed x has output: the batch call's y without its last `guard` samples"""
    y = blank(x, blank_, guard)[0]
    return y[:max(0, y.shape[0] - guard)]


def brute(x, blank_=24, guard=2):
    """the same text by a second route, one channel: a full sort per block, Python floats for the threshold's two
    roundings, and the guard as an explicit loop over j -> (y, med, nzero)"""
    xf = as_float(np.asarray(x)).reshape(-1)
    u = patterns(xf)
    n, nb = len(u), -(-len(u) // N)
    med = np.zeros(nb, np.uint32)
    for b in range(n // N):
        med[b] = np.sort(u[b * N:(b + 1) * N])[N // 2 - 1]
    flag = np.zeros(n, bool)
    for b in range(1, nb):
        m = med[b - 1]
        if m == 0 or m >= INF or b - 1 >= n // N:
            continue
        with np.errstate(over="ignore"):
            t = np.float32(np.float32(np.float32(blank_) * np.array([m], np.uint32).view(np.float32)[0]) * np.float32(0.25))
        tb = np.array([t], np.float32).view(np.uint32)[0]
        for i in range(b * N, min(n, (b + 1) * N)):
            flag[i] = int(u[i]) > int(tb)
    hit = np.zeros(n, bool)
    for i in np.nonzero(flag)[0]:
        for j in range(max(0, i - guard), min(n - 1, i + guard) + 1):
            hit[j] = True
    y = xf.copy()
    y[hit] = np.float32(0.0)
    nz = np.array([hit[b * N:(b + 1) * N].sum() for b in range(nb)], np.int32)
    return y, med.view(np.float32), nz


# ---- inputs shared by tests/test_blank.py (no GPU) and the GPU tests: what the former shows about them -- the special
# cases they meet, the mutations they tell apart -- holds for the bytes the latter compare
def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def make_input(seed=0, nblocks=7, extra=321):
    """one channel, `nblocks` blocks and a ragged tail: noise whose level moves from block to block, spikes at and
    around block edges, and the special blocks the definition names"""
    r = np.random.Generator(np.random.Philox(seed))
    n = nblocks * N + extra
    x = r.standard_normal(n).astype(np.float32) * np.float32(0.01)
    x[2 * N:3 * N] *= np.float32(100.0)                      # a level step up: block 2 is judged by block 1
    x[3 * N:4 * N] = np.float32(0.25)                        # an all-equal block (every rank is 0.25)
    x[3 * N + 5] = np.float32(-0.25)
    x[4 * N:5 * N] = 0.0                                     # a zero block: block 5 has no threshold
    x[5 * N + 17] = np.float32(1e30)
    x[6 * N:7 * N] = f32(r.integers(1, 1 << 20, N))          # subnormals: block 7's threshold is subnormal
    for i in (N - 1, N, N + 1, 2 * N - 3, 2 * N + 2, n - 1, N + 700, N + 701):
        x[i] = np.float32(7.0) * (-1) ** i
    x[N + 2000] = np.inf
    x[N + 2100] = -np.inf
    x[N + 2200] = np.nan
    x[100] = np.nan                                          # block 0: no threshold, a NaN passes
    return x


def tie_input():
    """medians with 2048-way ties: half a block at one magnitude, half at another, in every order the rank can meet"""
    x = np.empty(4 * N, np.float32)
    x[0:N] = np.where(np.arange(N) % 2 == 0, np.float32(0.5), np.float32(-0.125))      # rank 2047 is 0.125, rank 2048 is 0.5
    x[N:2 * N] = np.float32(0.3)
    x[N + 9] = np.float32(0.75)                                                          # 0.75 = 24/4 * 0.125: NOT above it
    x[N + 11] = f32(np.array(0.75, np.float32).view(np.uint32) + 1)                      # one ulp more: flagged
    x[2 * N:3 * N] = np.float32(0.01)
    x[3 * N:] = np.float32(0.01)
    x[3 * N + 1] = np.float32(1.0)
    x[4 * N - 1] = np.float32(-1.0)                                                      # a spike on the record's last sample
    return x
