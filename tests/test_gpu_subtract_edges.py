"""K8 over its whole refine surface, at the frame's edges, beyond rank 1 and at the limits of its parameters.

tests/test_gpu_subtract.py sees the winner of k8_refine in six look-alike cases and the cancellation on four items.  Here
all 441 values M(l, q) that k8_pick chooses from are read back (uwspr_debug_subtract_surface: the nine per-workgroup
partial rows added as the pick adds them) and held to the binary64 restatement of that file, with the truth in the
corners of the grid, items clipped at either end of the frame or wholly outside it, a drift of 40 Hz, |f| = 1e4 Hz and
|drift| = 1e3 Hz; k8_cancel / k8_apply run with lo / hi on and beside tile (4608) and symbol (256) edges, with windows
that are never full, with one sample and with none; a NaN sample; 70 items in up to five ranks after a small call.

Everything at fl = 45000, unit-amplitude signals of random symbols 0..3 in AWGN of sigma 0.5 per component.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_subtract import (CANCEL_BOUND, FL, FS, N, NSYM, SPB, add_signal, cancel_ref, f_sym, first_max, item, refine_ref,
                               to_c, to_frame)

SIGMA = 0.5
DFQ = 0.0125
# max over the cases below of max_(q, l) |M_gpu - M_restated| / S_l, S_l = sum_i sum_k |x[shift + l + 256 i + k]|, measured on
# an MI355X: SURFACE_MEASURED (profiles/subtract.txt, "refine surface": the line of the worst case).  The bytes are
# deterministic; the factor 4 is the room CANCEL_BOUND keeps for another compiler's instruction order.  The ceiling is what
# a 256-term binary32 FMA sum with two rounded phasor factors can be off by at worst (2e-5 S): a bad measurement cannot
# hide behind the factor.  test_the_surface_bound_can_tell_neighbours_apart is what shows the bound means something.
SURFACE_MEASURED = 1.835e-07
SURFACE_BOUND = 4 * SURFACE_MEASURED
assert SURFACE_BOUND <= 2e-5

F_WIDE = 9999.7


# ---- helpers -----------------------------------------------------------------------------------------------------------
def surface_ref(x, sym, f, shift, drift):
    """refine_ref, and all zeros for an item none of whose 49 lags reaches the frame (refine_ref pads by 2^16 only)"""
    if shift - 24 >= len(x) or shift + 24 + N <= 0:
        return np.zeros((9, 49))
    return refine_ref(x, sym, f, shift, drift)


def lag_mass(x, shift):
    """S_l, l = -24..24: the sum of the magnitudes lag l's 162 windows hold (they tile [shift + l, shift + l + N))"""
    cs = np.concatenate(([0.0], np.cumsum(np.abs(x))))
    start = shift + np.arange(-24, 25)
    lo, hi = np.clip(start, 0, len(x)), np.clip(start + N, 0, len(x))
    return np.where(hi > lo, cs[hi] - cs[lo], 0.0)


def surface_error(M, Mref, S):
    """|M - Mref| / S_l per cell, 0 / 0 = 0"""
    d = np.abs(np.asarray(M, np.float64) - Mref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0.0, 0.0, d / S[None, :])


def f32(v):
    return float(np.float32(v))


def refined_f(f, q):
    """f' of the header: formed in binary64, rounded to the binary32 of the result record"""
    return np.float32(np.float64(np.float32(f)) + DFQ * q)


def q_of(res_f, f):
    """the q behind a result's f_hz (the nine candidates are distinct binary32 numbers up to |f| = 1e4: 0.0125 against an
    ulp of 0.001)"""
    hits = [q for q in range(-4, 5) if refined_f(f, q) == np.float32(res_f)]
    assert len(hits) == 1, (res_f, f, hits)
    return hits[0]


def noise(rng):
    return SIGMA * (rng.standard_normal(FL) + 1j * rng.standard_normal(FL))


def place(sig, rng, sym, f, start, drift=0.0, amp=1.0):
    """the item model (f, start, drift) added to sig; f is taken to its alias in [-187.5, 187.5) Hz: the same samples, and
    add_signal's running phase sum stays short"""
    f = np.float64(f)
    add_signal(sig, sym, f - FS * np.round(f / FS), int(start), rng.uniform(0.0, 2.0 * np.pi), amp, drift)


def one_item_frame(seed, shift, f, drift=0.0, truth=(0, 0), signal=True, awgn=True):
    """-> (frame [fl, 2] float32, item dict): a unit signal whose start is truth[0] samples and whose frequency is
    0.0125 truth[1] Hz from the item's (shift, f), in AWGN"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, NSYM).astype(np.uint8)
    sig = np.zeros(FL, np.complex128)
    if signal:
        place(sig, rng, sym, np.float64(np.float32(f)) + DFQ * truth[1], shift + truth[0], f32(drift))
    if awgn:
        sig += noise(rng)
    return to_frame(sig), item(0, int(shift), f32(f), sym, f32(drift))


# name, kind, arguments of one_item_frame.  kind: "signal" (the restatement has a peak to find), "flat" (noise only, or
# only some lags inside), "zero" (the surface is exactly 0)
SURFACE_CASES = [
    ("a nominal", "signal", dict(shift=375, f=1.3, truth=(-13, -2))),
    ("b corner (-24, -4)", "signal", dict(shift=390, f=-2.2, truth=(-24, -4))),
    ("b corner (+24, +4)", "signal", dict(shift=350, f=0.6, truth=(24, 4))),
    ("b corner (-24, +4)", "signal", dict(shift=401, f=2.9, truth=(-24, 4))),
    ("b corner (+24, -4)", "signal", dict(shift=333, f=-0.9, truth=(24, -4))),
    ("c drift 40", "signal", dict(shift=375, f=-1.7, drift=40.0, truth=(0, 0))),
    ("d shift -3000", "signal", dict(shift=-3000, f=0.8, truth=(7, 2))),
    ("e shift fl - N + 5000", "signal", dict(shift=FL - N + 5000, f=-2.6, truth=(-9, -1))),
    ("f shift -24", "signal", dict(shift=-24, f=1.9, truth=(-20, 1))),
    ("g shift fl - N + 24", "signal", dict(shift=FL - N + 24, f=-0.4, truth=(20, -1))),
    ("h noise only", "flat", dict(shift=375, f=0.7, signal=False)),
    ("i all zero", "zero", dict(shift=375, f=0.7, signal=False, awgn=False)),
    ("j shift 2^20", "zero", dict(shift=1 << 20, f=1.1, truth=(0, 0))),
    ("j shift -2^20", "zero", dict(shift=-(1 << 20), f=1.1, truth=(0, 0))),
    ("j shift fl + 24", "zero", dict(shift=FL + 24, f=1.1, signal=False)),
    ("j shift fl", "flat", dict(shift=FL, f=1.1, signal=False)),          # lags < 0 are inside
    ("k f +9999.7", "signal", dict(shift=375, f=F_WIDE, truth=(-13, -2))),
    ("k f -9999.7", "signal", dict(shift=380, f=-F_WIDE, truth=(11, 3))),
    ("k drift +1000", "signal", dict(shift=370, f=1.5, drift=1000.0, truth=(-6, 2))),
    ("k drift -1000", "signal", dict(shift=365, f=-1.5, drift=-1000.0, truth=(5, -3))),
]
# l: three items in one frame, (shift, f, drift, truth, amplitude); items 2 and 3 are refined on the residual
CHAIN = [(375, 1.3, 0.0, (-13, -2), 1.0), (700, -2.1, 0.5, (9, 3), 0.8), (100, 0.45, 0.0, (-4, 1), 0.6)]


def build_surface_cases():
    """frames [21, fl, 2], the 23 items, and per item the restated surface and S_l.  The chain's second and third surface
    are restated on cancel_ref's residual at the restatement's own first maximum of the one before."""
    frames, items, names, kinds = [], [], [], []
    for n, (name, kind, kw) in enumerate(SURFACE_CASES):
        fr, it = one_item_frame(2000 + n, **kw)
        it["frame"] = len(frames)
        frames.append(fr)
        items.append(it)
        names.append(name)
        kinds.append(kind)
    rng = np.random.default_rng(2100)
    sig = np.zeros(FL, np.complex128)
    chain_frame = len(frames)
    for j, (sh, f, dr, tr, amp) in enumerate(CHAIN):
        sym = rng.integers(0, 4, NSYM).astype(np.uint8)
        place(sig, rng, sym, np.float64(np.float32(f)) + DFQ * tr[1], sh + tr[0], f32(dr), amp)
        items.append(item(chain_frame, sh, f32(f), sym, f32(dr)))
        names.append("l item %d of 3" % (j + 1))
        kinds.append("signal")
    sig += noise(rng)
    frames.append(to_frame(sig))
    frames = np.stack(frames)
    Mref, S, chain_pick = [], [], []
    x, x_of = None, -1
    for n, it in enumerate(items):
        if it["frame"] != x_of:
            x, x_of = to_c(frames[it["frame"]]), it["frame"]
        M = surface_ref(x, it["symbols"], it["f"], it["shift"], it["drift"])
        Mref.append(M)
        S.append(lag_mass(x, it["shift"]))
        if it["frame"] == chain_frame:
            q, l = first_max(M)
            chain_pick.append((q, l))
            x, _ = cancel_ref(x, it["symbols"], refined_f(it["f"], q), it["shift"] + l, np.float32(it["drift"]))
    return {"frames": frames, "items": items, "names": names, "kinds": kinds, "Mref": np.stack(Mref), "S": np.stack(S),
            "chain_first": len(SURFACE_CASES), "chain_pick": chain_pick}


@pytest.fixture(scope="module")
def surf():
    return build_surface_cases()


def bind_surface(G):
    L = G.native.lib()
    L.uwspr_debug_subtract_surface.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.uwspr_debug_subtract_surface.restype = C.c_int
    return L


def read_surface(G, ctx, i):
    M = np.full((9, 49), -1.0, np.float32)
    rc = bind_surface(G).uwspr_debug_subtract_surface(ctx.h, int(i), C.c_void_p(M.ctypes.data))
    assert rc == 0, (i, rc)
    return M


@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_surf(G, ctx, surf):
    """the one refining call over the surface cases, and every item's surface"""
    out, res = ctx.subtract(surf["frames"], surf["items"], refine=True)
    M = np.stack([read_surface(G, ctx, i) for i in range(len(surf["items"]))])
    L = bind_surface(G)
    scratch = np.zeros(441, np.float32)
    assert L.uwspr_debug_subtract_surface(ctx.h, len(surf["items"]), C.c_void_p(scratch.ctypes.data)) == -6   # no such item
    assert L.uwspr_debug_subtract_surface(ctx.h, -1, C.c_void_p(scratch.ctypes.data)) == -6
    return {"out": out, "res": res, "M": M}


# ---- the refine surface --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refine_surface_equals_the_restatement(G, ctx, surf, gpu_surf):
    worst = 0.0
    first = surf["chain_first"]
    for n, (name, kind, it) in enumerate(zip(surf["names"], surf["kinds"], surf["items"])):
        M, Mref, S = gpu_surf["M"][n], surf["Mref"][n], surf["S"][n]
        if n > first:   # the residual this item was refined on is the restatement's only if the item before went the same way
            prev, (q, l) = gpu_surf["res"][n - 1], surf["chain_pick"][n - 1 - first]
            assert int(prev["shift"]) == surf["items"][n - 1]["shift"] + l and prev["f_hz"] == refined_f(surf["items"][n - 1]["f"], q), name
        e = surface_error(M, Mref, S)
        h = int(np.argmax(e))
        print("surface %-22s max |M_gpu - M_ref| / S_l = %.3e at (q, l) = (%d, %d); M there %.6f against %.6f, S_l %.1f"
              % (name, e.max(), h // 49 - 4, h % 49 - 24, float(M.reshape(-1)[h]), Mref.reshape(-1)[h], S[h % 49]))
        assert np.isfinite(M).all(), name
        if kind == "zero":
            assert not Mref.any() and M.tobytes() == np.zeros((9, 49), np.float32).tobytes(), name
        assert e.max() <= SURFACE_BOUND, (name, e.max())
        worst = max(worst, e.max())
    print("refine surface: worst case %.3e (SURFACE_MEASURED %.3e, bound %.3e)" % (worst, SURFACE_MEASURED, SURFACE_BOUND))
    # the read-out belongs to a refining call
    ctx.subtract(surf["frames"][:1], surf["items"][:1], refine=False)
    scratch = np.zeros(441, np.float32)
    assert bind_surface(G).uwspr_debug_subtract_surface(ctx.h, 0, C.c_void_p(scratch.ctypes.data)) == -6


def test_the_surface_bound_can_tell_neighbours_apart(surf):
    """What makes the bound a test: a kernel that put every value one lag, or one offset, beside its place would fail the
    comparison above in at least 90 % of its cells, in every case with a signal (a..g, k).  The restatement alone, no GPU."""
    checked = 0
    for n, (name, kind) in enumerate(zip(surf["names"], surf["kinds"])):
        if kind != "signal" or n >= surf["chain_first"]:
            continue
        M, S = surf["Mref"][n], surf["S"][n]
        moved = {"lag + 1": (M[:, 1:], M[:, :-1], S[:-1]), "lag - 1": (M[:, :-1], M[:, 1:], S[1:]),
                 "offset + 1": (M[1:, :], M[:-1, :], S), "offset - 1": (M[:-1, :], M[1:, :], S)}
        for what, (got, want, s) in moved.items():
            caught = float((surface_error(got, want, s) > SURFACE_BOUND).mean())
            print("sensitivity %-22s %-10s caught in %5.1f %% of the cells" % (name, what, 100.0 * caught))
            assert caught >= 0.9, (name, what, caught)
        checked += 1
    assert checked == 14


@pytest.mark.gpu
def test_pick_is_the_first_maximum_of_the_surface(G, ctx, surf, gpu_surf):
    decided = 0
    for n, (name, kind, it) in enumerate(zip(surf["names"], surf["kinds"], surf["items"])):
        M, Mref, S, res = gpu_surf["M"][n], surf["Mref"][n], surf["S"][n], gpu_surf["res"][n]
        q, l = first_max(M)                                        # of the GPU's own surface: the pick's input
        got_l, got_q = int(res["shift"]) - it["shift"], q_of(res["f_hz"], it["f"])
        assert (got_q, got_l) == (q, l), (name, (got_q, got_l), (q, l))
        assert np.float32(res["metric"]).tobytes() == M[q + 4, l + 24].tobytes(), name
        assert res["f_hz"] == refined_f(it["f"], q), name
        if kind == "zero":
            assert (q, l) == (-4, -24) and res["metric"] == 0.0 and res["removed"] == 0.0, name
        # where no other cell of the restatement comes within the bound of its best, the GPU's maximum is the restatement's
        rq, rl = first_max(Mref)
        gap = Mref[rq + 4, rl + 24] - Mref - SURFACE_BOUND * (S[rl + 24] + S[None, :])
        gap[rq + 4, rl + 24] = np.inf
        if (gap > 0).all():
            decided += 1
            assert (q, l) == (rq, rl), (name, (q, l), (rq, rl))
        print("pick %-22s GPU (q, l) = (%d, %d), restatement (%d, %d)%s" % (name, q, l, rq, rl, "" if (gap > 0).all() else "  (within the bound of another cell)"))
    # (the top of a peak is flat: neighbouring offsets differ by 1e-6 .. 3e-5 of S there, so not every case is decisive)
    print("pick: the restatement's maximum was decisive in %d of %d items" % (decided, len(surf["items"])))


# ---- cancel at the edges -------------------------------------------------------------------------------------------------
BIG = 1 << 20
# name, shift, f, drift, what is expected beyond the bound: "in" some samples inside, "out" none
CANCEL_CASES = [("lo on a tile edge", -4608, 1.3, 0.0, "in"), ("lo one before a tile edge", -4607, -0.7, 0.0, "in"),
                ("lo one past a tile edge", -4609, 2.2, 0.3, "in"), ("lo on a symbol edge", -256, -1.9, 0.0, "in"),
                ("lo one before a symbol edge", -255, 0.4, 0.0, "in"),
                ("hi on a tile edge", FL - 4608, 1.1, 0.0, "in"), ("hi one before a tile edge", FL - 4607, -2.4, 0.0, "in"),
                ("hi one past two tiles", FL - 9216 - 1, 0.9, -0.4, "in"),
                ("700 samples at the end", FL - 700, -1.2, 0.0, "in"), ("700 samples at the start", -N + 700, 2.6, 0.0, "in"),
                ("one sample at the end", FL - 1, 0.3, 0.0, "in"), ("one sample at the start", -N + 1, -0.3, 0.0, "in"),
                ("shift fl", FL, 1.0, 0.0, "out"), ("shift -N", -N, 1.0, 0.0, "out"),
                ("shift 2^20", BIG, 1.0, 0.0, "out"), ("shift -2^20", -BIG, 1.0, 0.0, "out"),
                ("f +9999.7", 375, F_WIDE, 0.0, "in"), ("f -9999.7", 380, -F_WIDE, 0.0, "in"),
                ("drift +1000", 370, 1.5, 1000.0, "in"), ("drift -1000", 365, -1.5, -1000.0, "in")]
WIDE_TRUTH = {"f +9999.7": (-13, -2), "f -9999.7": (11, 3), "drift +1000": (-6, 2), "drift -1000": (5, -3)}   # as in SURFACE_CASES


def build_cancel_cases():
    frames, items, ref, removed = [], [], [], []
    for n, (name, shift, f, drift, _) in enumerate(CANCEL_CASES):
        rng = np.random.default_rng(3000 + n)
        sym = rng.integers(0, 4, NSYM).astype(np.uint8)
        sig = noise(rng)
        if name in WIDE_TRUTH:     # the surface list's items: off the truth by a few lags and offsets
            l, q = WIDE_TRUTH[name]
            place(sig, rng, sym, np.float64(np.float32(f)) + DFQ * q, shift + l, f32(drift))
        else:                      # a model that is slightly off, as in tests/test_gpu_subtract.py
            place(sig, rng, sym, np.float64(np.float32(f)) + 0.004, shift + 1, f32(drift))
        fr = to_frame(sig)
        it = item(n, shift, f32(f), sym, f32(drift))
        r, rm = cancel_ref(to_c(fr), sym, np.float32(f), shift, np.float32(drift), reduced=name in WIDE_TRUTH)
        frames.append(fr)
        items.append(it)
        ref.append(r)
        removed.append(rm)
    return {"frames": np.stack(frames), "items": items, "ref": np.stack(ref), "removed": np.array(removed)}


@pytest.fixture(scope="module")
def cancel_cases():
    return build_cancel_cases()


def test_the_reduced_phase_is_the_running_sum_where_both_are_good(cancel_cases):
    """cancel_ref's two forms of theta on an item at 1.3 Hz, and the reduced one against exact rational arithmetic at
    9999.7 Hz: the restatement's own phase is good to 1e-9 turns over the whole range"""
    from fractions import Fraction
    it = cancel_cases["items"][0]
    x = to_c(cancel_cases["frames"][0])
    a, _ = cancel_ref(x, it["symbols"], np.float32(it["f"]), it["shift"], np.float32(0.0))
    b, _ = cancel_ref(x, it["symbols"], np.float32(it["f"]), it["shift"], np.float32(0.0), reduced=True)
    assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(x))
    # the turns the reduced form arrives at, against the header's sum in exact arithmetic
    sym = cancel_cases["items"][16]["symbols"]
    f = Fraction(float(np.float32(F_WIDE)))
    fi = [(f + (int(s) * 2 - 3) * Fraction(375, 512)) / 375 for s in sym]
    w = f_sym(np.float32(F_WIDE), np.float32(0.0), sym) / FS      # cancel_ref's own turns per sample
    ph, worst = 0.0, 0.0
    exact = Fraction(0)
    for i in range(NSYM):
        for r in (0, 255):
            t = (ph + r * w[i]) % 1.0
            d = abs(float(((exact + r * fi[i]) % 1) - Fraction(t)))
            worst = max(worst, min(d, 1.0 - d))
        ph = (ph + SPB * w[i]) % 1.0
        exact += SPB * fi[i]
    print("reduced phase at %.1f Hz: off by at most %.2e turns over 162 symbols" % (F_WIDE, worst))
    assert worst <= 1e-9


@pytest.mark.gpu
def test_cancel_at_tile_symbol_and_frame_edges(G, ctx, cancel_cases):
    frames, items = cancel_cases["frames"], cancel_cases["items"]
    out, res = ctx.subtract(frames, items, refine=False)
    scale = np.max(np.abs(to_c(frames)))
    for n, (name, shift, f, drift, where) in enumerate(CANCEL_CASES):
        err = np.max(np.abs(to_c(out[n]) - cancel_cases["ref"][n])) / scale
        print("cancel %-28s shift %8d: max |GPU - restatement| / max |x| = %.3e (bound %.3e), removed %.6g against %.6g"
              % (name, shift, err, CANCEL_BOUND, float(res[n]["removed"]), cancel_cases["removed"][n]))
        assert err <= CANCEL_BOUND, name
        assert res[n]["shift"] == shift and res[n]["f_hz"] == np.float32(f) and res[n]["metric"] == 0.0, name
        if where == "out":
            assert out[n].tobytes() == frames[n].tobytes() and res[n]["removed"] == 0.0, name
        else:
            assert out[n].tobytes() != frames[n].tobytes(), name
            assert np.allclose(res[n]["removed"], cancel_cases["removed"][n], rtol=1e-4, atol=0.0), name
            k = np.arange(FL)          # nothing outside [shift, shift + N) is touched
            outside = (k < shift) | (k >= shift + N)
            assert out[n][outside].tobytes() == frames[n][outside].tobytes(), name


@pytest.mark.gpu
def test_a_refined_shift_moves_the_first_sample(G, ctx):
    """an item given at shift 10 whose signal starts at -5: given, lo = 0; refined, lo = 5"""
    fr, it = one_item_frame(3100, shift=10, f=-1.4, truth=(-15, 1))
    out, res = ctx.subtract(fr[None], [it], refine=True)
    x = to_c(fr)
    Mref = refine_ref(x, it["symbols"], it["f"], it["shift"], it["drift"])
    assert first_max(Mref) == (1, -15)
    assert int(res[0]["shift"]) == -5 and res[0]["f_hz"] == refined_f(it["f"], 1)
    ref, rm = cancel_ref(x, it["symbols"], res[0]["f_hz"], int(res[0]["shift"]), np.float32(it["drift"]))
    err = np.max(np.abs(to_c(out[0]) - ref)) / np.max(np.abs(x))
    print("cancel after a refinement that moves lo: %.3e (bound %.3e)" % (err, CANCEL_BOUND))
    assert err <= CANCEL_BOUND
    assert np.allclose(res[0]["removed"], rm, rtol=1e-4, atol=0.0)
    assert out[0][0].tobytes() != fr[0].tobytes()         # sample 0 is k = 5 of the refined item


# ---- a NaN sample ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_nan_sample_stays_local(G, ctx):
    fa, ia = one_item_frame(3200, shift=375, f=0.9, truth=(1, 0))
    fb, ib = one_item_frame(3201, shift=-1200, f=-1.6, drift=0.4, truth=(-1, 0))
    knan = 20000 + 77                                       # k of the NaN within item a: no tile or symbol edge near
    fa = fa.copy()
    fa[375 + knan] = np.nan
    frames = np.stack([fa, fb])
    ib = dict(ib, frame=1)
    alone, ralone = ctx.subtract(fb[None], [dict(ib, frame=0)], refine=False)
    out, res = ctx.subtract(frames, [ia, ib], refine=False)
    assert out[1].tobytes() == alone[0].tobytes() and res[1].tobytes() == ralone[0].tobytes()
    k = np.arange(FL) - 375
    want_nan = np.abs(k - knan) <= 511                      # the 1023 outputs whose window holds the sample
    got_nan = np.isnan(out[0])
    assert np.array_equal(got_nan[:, 0], want_nan) and np.array_equal(got_nan[:, 1], want_nan), \
        (np.flatnonzero(got_nan.any(axis=1))[[0, -1]] - 375, knan)
    ref, _ = cancel_ref(to_c(fa), ia["symbols"], np.float32(ia["f"]), 375, np.float32(0.0))
    assert np.array_equal(np.isnan(ref), want_nan)
    err = np.max(np.abs(to_c(out[0]) - ref)[~want_nan]) / np.nanmax(np.abs(to_c(fa)))
    print("cancel beside a NaN sample: %.3e (bound %.3e)" % (err, CANCEL_BOUND))
    assert err <= CANCEL_BOUND
    # refining: an accepted call; every lag's windows hold the sample, M is NaN throughout and the pick stays where it starts
    alone, ralone = ctx.subtract(fb[None], [dict(ib, frame=0)], refine=True)
    out, res = ctx.subtract(frames, [ia, ib], refine=True)
    assert -24 <= int(res[0]["shift"]) - 375 <= 24 and -4 <= q_of(res[0]["f_hz"], ia["f"]) <= 4
    assert out[1].tobytes() == alone[0].tobytes() and res[1].tobytes() == ralone[0].tobytes()


# ---- ranks, growth, and the batch ----------------------------------------------------------------------------------------
COUNTS = [3, 1, 0, 2, 5, 3, 4, 2, 3, 0, 4, 3, 2, 4, 3, 2, 4, 3, 2, 4, 4, 4, 4, 4]
assert sum(COUNTS) == 70 and len(COUNTS) == 24 and COUNTS.count(5) == 1


@pytest.mark.gpu
def test_ranks_growth_and_batch_independence(G):
    rng = np.random.default_rng(3300)
    frames, items = [], []
    for b, cnt in enumerate(COUNTS):
        sig = noise(rng)
        for _ in range(cnt):
            sym = rng.integers(0, 4, NSYM).astype(np.uint8)
            shift, f, drift = int(rng.integers(-2000, FL - N + 2001)), f32(rng.uniform(-150.0, 150.0)), f32(rng.choice([0.0, 0.0, 1.0, -2.0]))
            l, q = int(rng.integers(-24, 25)), int(rng.integers(-4, 5))
            place(sig, rng, sym, np.float64(f) + DFQ * q, shift + l, drift, rng.uniform(0.4, 1.0))
            items.append(item(b, shift, f, sym, drift))
        frames.append(to_frame(sig))
    frames = np.stack(frames)
    ctx = G.Context(device=0)     # its own: the scratch starts empty, a small call sizes it, the large one regrows all of it
    try:
        ctx.subtract(frames[:1], items[:1], refine=True)
        out, res = ctx.subtract(frames, items, refine=True)
        M = [read_surface(G, ctx, i) for i in range(70)]
        five = COUNTS.index(5)
        n = 0
        for b, cnt in enumerate(COUNTS):
            cur = frames[b:b + 1]
            for j in range(cnt):
                it = items[n]
                nxt, r1 = ctx.subtract(cur, [dict(it, frame=0)], refine=True)
                assert r1[0].tobytes() == res[n].tobytes(), (b, j, r1[0], res[n])
                assert read_surface(G, ctx, 0).tobytes() == M[n].tobytes(), (b, j)
                if b == five:     # the restatement, stage by stage, on the bytes each stage started from
                    x = to_c(cur[0])
                    Mref = refine_ref(x, it["symbols"], it["f"], it["shift"], it["drift"])
                    e = surface_error(M[n], Mref, lag_mass(x, it["shift"])).max()
                    ref, rm = cancel_ref(x, it["symbols"], r1[0]["f_hz"], int(r1[0]["shift"]), np.float32(it["drift"]))
                    err = np.max(np.abs(to_c(nxt[0]) - ref)) / np.max(np.abs(to_c(frames[b])))
                    print("rank %d of the 5-item frame: surface %.3e (bound %.3e), cancel %.3e (bound %.3e)" % (j, e, SURFACE_BOUND, err, CANCEL_BOUND))
                    assert e <= SURFACE_BOUND and err <= CANCEL_BOUND
                    q, l = first_max(M[n])
                    assert int(r1[0]["shift"]) == it["shift"] + l and r1[0]["f_hz"] == refined_f(it["f"], q)
                    assert np.allclose(r1[0]["removed"], rm, rtol=1e-4, atol=0.0)
                cur = nxt
                n += 1
            assert out[b].tobytes() == cur[0].tobytes(), b      # (a frame without items: the input's bytes)
            if cnt == 0:
                assert out[b].tobytes() == frames[b].tobytes()
        assert n == 70
    finally:
        ctx.close()
