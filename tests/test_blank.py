"""The noise blanker's definition (include/uwspr_hip.h, "impulsive noise") without a GPU: the numpy restatement the GPU
tests compare bytes with (tests/blank_exact.py) against a second, brute-force route, the int16 and float32 paths against
each other, four misreadings of the text that the test inputs must tell from it, and the new symbols' declarations."""
import os
import re

import numpy as np
import pytest

import blank_exact as BX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = BX.N


f32, make_input, tie_input = BX.f32, BX.make_input, BX.tie_input


INPUTS = [make_input(0), make_input(1, nblocks=8, extra=0), tie_input()]


@pytest.mark.parametrize("k", range(len(INPUTS)))
@pytest.mark.parametrize("blank,guard", [(24, 2), (4, 0), (1024, 64), (24, 1)])
def test_restatement_against_brute_force(k, blank, guard):
    x = INPUTS[k]
    y, med, nz = BX.blank(x, blank, guard)
    yb, mb, nb = BX.brute(x, blank, guard)
    assert y.dtype == np.float32 and med.dtype == np.float32 and nz.dtype == np.int32
    assert (y.view(np.uint32) == yb.view(np.uint32)).all()
    assert (med.view(np.uint32) == mb.view(np.uint32)).all()
    assert (nz == nb).all()


def test_the_inputs_meet_the_special_cases():
    x = INPUTS[0]
    y, med, nz = BX.blank(x, 24, 2)
    m = med.view(np.uint32)
    assert m[3] == np.array(0.25, np.float32).view(np.uint32) and m[4] == 0 and 0 < m[6] < 0x00800000 and med[-1] == 0
    # block 0 passes untouched (its own spike at N - 1 and its NaN too), but for the guard of the spike at N
    assert nz[0] == 2 and np.isnan(y[100]) and (y[:N - 2].view(np.uint32) == x[:N - 2].view(np.uint32)).all()
    assert nz[5] == 0 and y[5 * N + 17] == np.float32(1e30)   # a zero block, then signal: nothing is blanked
    assert nz[2] > N // 2                                     # the level step is blanked (the design's stated cost)
    assert (y[N + 2198:N + 2203] == 0).all() and (y[N + 1998:N + 2003] == 0).all()   # NaN and inf in a block with a threshold
    assert (y[N - 2:N + 4] == 0).all() and y[N - 3] != 0                     # the guard crosses the block edge, block 0 included
    assert nz[-1] == 321                                      # noise after a block of subnormals: a level step again
    t = INPUTS[2]
    yt, mt, nzt = BX.blank(t, 24, 0)
    assert mt[0] == np.float32(0.125)
    assert yt[N + 9] == np.float32(0.75) and yt[N + 11] == 0 and nzt[1] == 1   # strictly above the threshold only
    y2, _, nz2 = BX.blank(t, 24, 2)
    assert (y2[-3:] == 0).all() and y2[-4] == np.float32(0.01) and nz2[3] == 4 + 3   # no j behind the record's end


def test_int16_and_float_paths_agree():
    r = np.random.Generator(np.random.Philox(5))
    s = (r.standard_normal((3 * N + 77, 2)) * 300).astype(np.int16)
    s[N + 5, 0] = 32767
    s[2 * N, 1] = -32768
    s[2 * N + 1, 0] = 20000
    f = s.astype(np.float32) / np.float32(32768)
    a, b = BX.blank(s, 24, 2), BX.blank(f, 24, 2)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and p.shape == q.shape and (p.view(np.uint32) == q.view(np.uint32)).all()
    assert a[2].sum() > 0
    # channels are treated on their own
    for c in range(2):
        one = BX.blank(np.ascontiguousarray(s[:, c]), 24, 2)
        for p, q in zip(one, a):
            assert (p.view(np.uint32) == np.ascontiguousarray(q[:, c]).view(np.uint32)).all()


def test_stream_is_the_batch_without_its_last_guard_samples():
    x = INPUTS[0]
    for g in (0, 2, 64):
        assert (BX.stream(x, 24, g).view(np.uint32) == BX.blank(x, 24, g)[0][:len(x) - g].view(np.uint32)).all()


@pytest.mark.parametrize("mutation", [dict(rank=N // 2), dict(own_block=True), dict(guard_stops=True), dict(ge=True)])
def test_mutations_change_the_expectations(mutation):
    """rank N/2 instead of N/2 - 1; the block's own level instead of the previous block's; a guard that stops at a
    block edge; >= instead of >: each is seen by the inputs the GPU tests use the same constructions of"""
    changed = 0
    for x in INPUTS:
        y = BX.blank(x, 24, 2)[0]
        ym = BX.blank(x, 24, 2, **mutation)[0]
        changed += int((y.view(np.uint32) != ym.view(np.uint32)).sum())
    assert changed > 0, mutation


def test_symbols_declared_and_bound():
    import gr_uwspr_amd as G
    hdr = open(os.path.join(ROOT, "include", "uwspr_hip.h")).read()
    for name in ("uwspr_blank_batch", "uwspr_stream_blank_stats", "uwspr_pipe_blank_stats"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in G.native.ABI_SYMBOLS
    assert re.search(r"^#define UWSPR_BLANK_BLOCK 4096$", hdr, re.M) and G.BLANK_BLOCK == 4096 == N
    assert re.search(r"^#define UWSPR_ABI_VERSION 6\b", hdr, re.M)
    for name in ("blank", "stream_blank_stats", "debug_blank_launch"):
        assert callable(getattr(G.Context, name))
    assert callable(G.Pipe.blank_stats) and callable(G.blank_launch_counts)
    import inspect
    sig = inspect.signature(G.Pipe.__init__).parameters
    assert sig["blank"].default == 0 and "blank_guard" in sig
