"""K13, the list search (uwspr_deep_set_list / uwspr_deep_batch): Context.deep equals the numpy restatement
(tests/deep_exact.py) byte for byte, over the host and the device form.

Random asymmetric bytes against numpy are the lane-map check of the int8 MFMA: a transposed or permuted operand or
accumulator map changes `best` or the scores.  The shapes walk the 16-item and 16-message tiles (1 below, at and 1 above a
tile, several tiles, several message chunks: a chunk is at least 64 messages); the special vectors are the int8 edges (bytes
0 and 255, that is -128 and 127), a non-zero pad of K (all 255 / all 0 would show it), all scores equal, exact ties, and
winner / runner-up pairs in one message tile and in the first and the last one."""
import numpy as np
import pytest

import deep_exact as X

pytestmark = pytest.mark.gpu
NS = (1, 15, 16, 17, 33)
MS = (1, 2, 15, 16, 17, 63, 65, 1000)
ERR_ARG = -6


@pytest.fixture(scope="module")
def lists(G):
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE91000)), 1000)
    return msgs, X.code_table(G, msgs)


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context()
    yield c
    c.close()


def random_vectors(n, seed):
    rng = np.random.Generator(np.random.Philox(0xDEE92000 + seed))
    s = rng.integers(0, 256, (n, 162), dtype=np.uint8)
    s[:, 0], s[:, 161], s[:, 64], s[:, 63] = 0, 255, 0, 255   # the int8 edges at the ends and across a k-step
    return s


def pair_vector(tab, a, b):
    """message a strongly and message b less so: a wins, and b's score stands clear of a random codeword's"""
    return (128 + 80 * (2 * tab[a] - 1) + 47 * (2 * tab[b] - 1)).astype(np.uint8)


def special_vectors(tab):
    M = len(tab)
    v = [np.full(162, 128, np.uint8), np.full(162, 255, np.uint8), np.zeros(162, np.uint8),
         (255 * tab[M - 1]).astype(np.uint8)]                  # the winner in the last (partial) tile
    if M >= 2:
        for a, b in ((0, M - 1), (M - 2, M - 1), (M // 2, M // 2 - 1)):
            t = np.full(162, 128, np.uint8)                    # 128 where a and b differ: they tie
            agree = tab[a] == tab[b]
            t[agree] = (255 * tab[a][agree]).astype(np.uint8)
            v.append(t)
        for a, b in ((M - 2, M - 1), (M - 1, M - 2), (0, M - 1), (M - 1, 0)):   # one tile; the first and the last chunk
            v.append(pair_vector(tab, a, b))
    return np.stack(v)


def both_forms(ctx, sym):
    import torch
    host = ctx.deep(sym)
    dev = ctx.deep(torch.from_numpy(np.ascontiguousarray(sym)).to("cuda:0"))
    return host, dev


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_shapes_equal_the_restatement(ctx, lists, n, M):
    msgs, tab = lists
    sym = random_vectors(n, 100 * n + M)
    sp = special_vectors(tab[:M])
    if n >= 15:
        sym[1:1 + len(sp)] = sp[:n - 1]
    else:
        sym[0] = sp[M % len(sp)]
    ctx.deep_set_list(msgs[:M])
    want = X.deep_restate(tab[:M], sym)
    host, dev = both_forms(ctx, sym)
    assert host.dtype == X.DEEP_DTYPE and host.tobytes() == want.tobytes()
    assert dev.tobytes() == want.tobytes()
    if M == 1:
        assert (host["best"] == 0).all() and (host["snext"] == -2 ** 31).all()


@pytest.mark.parametrize("M", MS)
def test_special_vectors(ctx, lists, M):
    msgs, tab = lists
    sym = special_vectors(tab[:M])
    ctx.deep_set_list(msgs[:M])
    want = X.deep_restate(tab[:M], sym)
    host, dev = both_forms(ctx, sym)
    assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    # what the vectors were built for, said of the restatement (the kernel equals it)
    assert (int(want[0]["best"]), int(want[0]["sbest"])) == (0, 0)
    assert int(want[0]["snext"]) == (0 if M > 1 else -2 ** 31)
    assert int(want[3]["best"]) == M - 1 and int(want[3]["sbest"]) == int(np.abs(sym[3].astype(np.int64) - 128).sum())
    if M >= 3:
        for row, (a, b) in zip((4, 5, 6), ((0, M - 1), (M - 2, M - 1), (M // 2, M // 2 - 1))):
            assert int(want[row]["best"]) == min(a, b) and int(want[row]["sbest"]) == int(want[row]["snext"])
    if M >= 15:
        S = X.scores(tab[:M], sym)
        for row, (a, b) in zip((7, 8, 9, 10), ((M - 2, M - 1), (M - 1, M - 2), (0, M - 1), (M - 1, 0))):
            assert int(want[row]["best"]) == a and int(want[row]["snext"]) == int(S[row, b])


def test_the_largest_list(G, ctx):
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE93000)), 65536)
    tab = X.code_table(G, msgs)
    sym = random_vectors(33, 65536)
    sym[1] = 128
    sym[2] = (255 * tab[65535]).astype(np.uint8)
    sym[3] = pair_vector(tab, 65535, 0)
    sym[4] = pair_vector(tab, 40000, 40001)
    ctx.deep_set_list(msgs)
    want = X.deep_restate(tab, sym)
    host, dev = both_forms(ctx, sym)
    assert host.tobytes() == want.tobytes() and dev.tobytes() == want.tobytes()
    assert int(want[2]["best"]) == 65535 and int(want[3]["best"]) == 65535 and int(want[4]["best"]) == 40000
    # fewer items make more, smaller message chunks (1024 for one item): the bytes do not depend on the split
    assert ctx.deep(sym[:1]).tobytes() == want[:1].tobytes()
    assert ctx.deep(sym[2:19]).tobytes() == want[2:19].tobytes()


def test_replacing_and_clearing_the_list(G, ctx, lists):
    msgs, tab = lists
    sym = random_vectors(5, 7)
    ctx.deep_set_list(msgs[:100])
    a = ctx.deep(sym)
    ctx.deep_set_list(msgs[100:300])
    b = ctx.deep(sym)
    assert a.tobytes() == X.deep_restate(tab[:100], sym).tobytes()
    assert b.tobytes() == X.deep_restate(tab[100:300], sym).tobytes() and a.tobytes() != b.tobytes()
    # texts go through wspr_pack
    texts = ["K1ABC FN42 37", "W1AW EM10 30", "G4XYZ IO91 10"]
    ctx.deep_set_list(texts)
    s = (255 * (G.wspr_symbols(texts[1]) >> 1)).astype(np.uint8)
    r = ctx.deep(s)[0]
    assert int(r["best"]) == 1 and int(r["sbest"]) == int(np.abs(s.astype(np.int64) - 128).sum())
    assert len(ctx.deep(np.zeros((0, 162), np.uint8))) == 0
    # a list that breaks the rules leaves the one in force
    bad = msgs[:4].copy()
    bad[3] = bad[0]
    with pytest.raises(G.UwsprError) as e:
        ctx.deep_set_list(bad)
    assert e.value.status == ERR_ARG
    assert int(ctx.deep(s)[0]["best"]) == 1
    ctx.deep_set_list([])
    with pytest.raises(G.UwsprError) as e:
        ctx.deep(sym)
    assert e.value.status == ERR_ARG


def test_device_pointers_are_checked_before_any_launch(G, ctx, lists):
    import ctypes as C
    import torch
    msgs, _ = lists
    ctx.deep_set_list(msgs[:20])
    sym = torch.zeros(3 * 162, dtype=torch.uint8, device="cuda:0")
    res = torch.zeros(3 * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    N = G.native
    # host pointers called device memory, on either side: refused before any launch
    host, hres = np.zeros(3 * 162, np.uint8), np.zeros(3, N.DEEP_RESULT_DTYPE)
    assert ctx.L.uwspr_deep_batch(ctx.h, C.c_void_p(host.ctypes.data), 3, N.DEVICE, C.c_void_p(res.data_ptr())) == ERR_ARG
    assert ctx.L.uwspr_deep_batch(ctx.h, C.c_void_p(sym.data_ptr()), 3, N.DEVICE, C.c_void_p(hres.ctypes.data)) == ERR_ARG
    assert ctx.L.uwspr_deep_batch(ctx.h, C.c_void_p(sym.data_ptr()), 3, N.DEVICE_FRAMES, C.c_void_p(res.data_ptr())) == ERR_ARG
    ctx.synchronize()
    assert not res.cpu().numpy().any() and not hres.view(np.uint8).any()
    assert ctx.L.uwspr_deep_batch(ctx.h, C.c_void_p(sym.data_ptr()), 3, N.DEVICE, C.c_void_p(res.data_ptr())) == 0
    ctx.synchronize()
    got = res.cpu().numpy().view(N.DEEP_RESULT_DTYPE)
    assert not got["reserved"].any() and (got["sbest"] >= got["snext"]).all()
