"""Designed spectrograms for the spectrum kernel (K2) and the coarse search (K3) -- numpy and the CPU oracle only, no device.

Noise plus a signal through K1 never reaches large parts of K2 and K3: the cut at `maxfreqs`, ties in `snr` and in the
percentile, plateaus, the first and last eligible bin, a zero noise level; a running best that stays negative, that is
exactly zero, NaN metrics inside a searched candidate.  The builders here hand over a spectrogram directly.  Each case
comes with a CONDITION that is checked on the oracle alone (tests/test_spectrum_cases.py): it says that the oracle, fed
this input, really goes where the case is meant to go.  tests/test_gpu_spectrum_edges.py then compares the library with
the oracle on the same input; it asserts nothing about the device with the replay below, the replay only classifies.

Column numbering: pass-band bin j is spectrum column m - hpbm + j (FDR_impl.cc:265-275); a candidate found on bin j has
if0 = m - hpbm + j (cc:341) and its 130 cells are ifr = if0 - 2 .. if0 + 2 times k0 = 0 .. 25.
"""
import numpy as np

import oracle_py as O

NK0, NIFR, NSYM, NSLM = O.NK0, O.NIFR, O.NSYM, O.NSLM
NCELL = NIFR * NK0
POISON = np.float32(3e30)      # finite, and 348 * 7 of them still are: what the library must never need


class Geom:
    """The constants of one FDR geometry, from the oracle's own constructor (raises ValueError where it refuses)."""

    def __init__(self, **kw):
        self.kw = dict(kw)
        self.fdr = O.FDR(**kw)
        f = self.fdr.f
        self.size, self.m, self.hpbm, self.n, self.finpb, self.noiseidx = f.size, f.m, f.hpbm, f.n, f.finpb, f.noiseidx
        self.df = np.float32(f.df)
        self.maxdrift, self.cf, self.maxfreqs = f.maxdrift, f.cf, f.maxfreqs
        self.nlin = 2 * f.maxdrift + 1
        self.hc = self.nlin + NSLM
        self.threshold = np.float32(f.threshold)
        self._band = None

    def col(self, j):
        return self.m - self.hpbm + j

    def offsets(self):
        """(omin, omax) of ifd - ifr over every tuned bin, hypothesis and symbol (cc:353 in binary64, cc:382-385 in binary32)"""
        ifr = np.arange(self.m - self.hpbm - 1, self.m + self.hpbm + 1)
        k = np.arange(NSYM)
        omin, omax = 0, 0
        for d in range(-self.maxdrift, self.maxdrift + 1):
            v = ifr[:, None].astype(np.float64) + (k.astype(np.float32).astype(np.float64) - 81.0) / 81.0 * \
                float(np.float32(d)) / (2.0 * float(self.df))
            o = v.astype(np.int64) - ifr[:, None]
            omin, omax = min(omin, int(o.min())), max(omax, int(o.max()))
        slm = np.array([[O.slm_frequency_drift(V1, V2, p1, p2, float(self.cf), float(t)) for t in range(111)]
                        for (V1, V2, p1, p2) in O.slm_instances()], np.float32)
        t = k * 111 // 162
        q = (slm[:, t] / self.df).astype(np.float32)                                # [125][162]
        o = (ifr.astype(np.float32)[:, None, None] + q[None]).astype(np.float32).astype(np.int64) - ifr[:, None, None]
        return min(omin, int(o.min())), max(omax, int(o.max()))

    def band(self):
        """(band_lo, band_w): the columns the smoothing (cc:268-275) and the search (cc:188-210) can read"""
        if self._band is None:
            omin, omax = self.offsets()
            lo = min(self.m - self.hpbm - 3, self.m - self.hpbm - 1 + omin - 3)
            hi = max(self.m + self.hpbm - 1 + 3, self.m + self.hpbm + omax + 3)
            self._band = (lo, hi - lo + 1)
        return self._band


def embed(tile, lo, size=512, poison=POISON):
    """band tile [..., n, band_w] -> full [..., n, size] spectrogram, POISON outside the band: the oracle then reads what
    the library was never given, and a band that is too narrow shows in the oracle's result"""
    tile = np.asarray(tile, np.float32)
    full = np.full(tile.shape[:-1] + (size,), poison, np.float32)
    full[..., lo:lo + tile.shape[-1]] = tile
    return full


def cut(full, lo, w):
    return np.ascontiguousarray(np.asarray(full, np.float32)[..., lo:lo + w])


# ----------------------------------------------------------------------------------------------- the oracle's side
def k2_oracle(g, full):
    """-> dict(psavg[size], smraw, smspec, noise, peaks) of one full spectrogram"""
    psavg, smraw, smspec, noise = g.fdr.stats(full)
    return {"psavg": psavg, "smraw": smraw, "smspec": smspec, "noise": np.float32(noise), "peaks": g.fdr.peaks(smspec)}


def maxima(smspec):
    """bins 1 .. finpb-2 that are strict local maxima of smspec (before the cut at maxfreqs)"""
    s = np.asarray(smspec)
    with np.errstate(invalid="ignore"):
        return [j for j in range(1, len(s) - 1) if s[j] > s[j - 1] and s[j] > s[j + 1]]


def replay(grid, nlin, threshold):
    """FDR_impl.cc:339-409 over an oracle grid [5][26][hc] in reference order (cell-major, linear hypotheses first).
    -> (winner, accepts): winner = (sync, entry index or -1); accepts = [(entry, best before it, is_linear)]."""
    flat = np.asarray(grid, np.float32).reshape(-1)
    hc = flat.size // NCELL
    thr = np.float32(threshold)
    best, gbest, acc = np.float32(-1e30), -1, []
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(flat.size):
            v = flat[e]
            lin = (e % hc) < nlin
            if (v > best) if lin else (np.float32(v / best) > thr):
                acc.append((e, best, lin))
                best, gbest = v, e
    return (best, gbest), acc


def winner_record(g, j, gbest, sync):
    """the fields cc:360-366 / cc:392-401 write for the winning entry of a candidate found on bin j"""
    cell, h = divmod(gbest, g.hc)
    ifr_i, k0 = divmod(cell, NK0)
    return {"sync": np.float32(sync), "shift": 128 * k0, "freq": np.float32(np.float32(g.col(j) - 2 + ifr_i - g.m) * g.df),
            "m_type": 0 if h < g.nlin else 1}


def classify(g, grid, acc):
    """the figures the conditions speak of"""
    flat = np.asarray(grid, np.float32).reshape(NCELL, g.hc)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero((flat[:, :g.nlin] >= np.float32(1.001) / g.threshold).any(axis=1))[0]
    return {"nl_neg": sum(1 for (e, b, lin) in acc if not lin and b < 0),
            "nl_zero": sum(1 for (e, b, lin) in acc if not lin and b == 0),
            "nl_pos": sum(1 for (e, b, lin) in acc if not lin and b > 0),
            "lin": sum(1 for (e, b, lin) in acc if lin),
            "zeros": int((flat == 0).sum()), "nans": int(np.isnan(flat).sum()),
            "cstar": int(hit[0]) if hit.size else NCELL,
            "neg_cells_before_cstar": int((flat[:int(hit[0]) if hit.size else NCELL, :g.nlin] < 0).all(axis=1).sum())}


def same_float(a, e):
    """binary32 arrays: NaN by position, everything else by bytes (the payload and sign of a NaN are nobody's contract)"""
    a, e = np.asarray(a, np.float32), np.asarray(e, np.float32)
    if a.shape != e.shape:
        return False
    na, ne = np.isnan(a), np.isnan(e)
    return bool((na == ne).all()) and a[~na].tobytes() == e[~ne].tobytes()


def record_diff(a, e):
    """fields of a library candidate `a` that differ from the oracle's `e` after the search: bytes (sync: or both NaN)"""
    bad = [k for k in ("m_type", "shift") if int(a[k]) != int(e[k])]
    bad += [k for k in ("freq", "snr") if np.float32(a[k]).tobytes() != np.float32(e[k]).tobytes()]
    if not same_float(a["sync"], e["sync"]):
        bad.append("sync")
    if int(e["m_type"]) == 1:
        bad += [k for k in ("V1", "V2", "p1", "p2") if a[k] != e[k]]
    elif a.tobytes()[24:28] != e.tobytes()[24:28]:      # m_linear.drift
        bad.append("drift")
    return bad


# ------------------------------------------------------------------------------------------------------ K2 inputs
# Rows are identical and column values are small integers: every sum of cc:257-275 is exact in binary32
# (n * 7 * value < 2^24), so smraw = n * (7-tap sum of the profile) whatever the order of the additions.
def rows_of(g, profile):
    p = np.asarray(profile, np.float32)
    assert p.shape == (g.size,) and (p == np.round(p)).all() and p.min() >= 0 and g.n * 7 * p.max() < 2 ** 24
    return np.tile(p, (g.n, 1))


def profile(g, base, spikes):
    """column profile: `base` everywhere, base + h on pass-band bin i for (i, h) in spikes (i may be -3 .. finpb + 2)"""
    p = np.full(g.size, base, np.float32)
    for i, h in spikes:
        assert -3 <= i <= g.finpb + 2
        p[g.col(i)] += h
    return p


def comb(g, parity=1, hi=40, lo=1):
    """period-2 comb over ALL columns: the 7-tap sums alternate 3*hi + 4*lo / 4*hi + 3*lo, the high ones on bins of
    `parity`: every other bin a peak, (finpb - 1) // 2 of them with parity 1, all with the same snr"""
    c = np.arange(g.size)
    return rows_of(g, np.where((c - g.col(0)) % 2 == (1 - parity), hi, lo))


def flat(g, v=5):
    return rows_of(g, np.full(g.size, v))


def pair(j, h):
    """two spikes six bins apart: the 7-tap sum holds both on bin j only -- one strict maximum with equal neighbours"""
    return [(j - 3, h), (j + 3, h)]


def five_peaks(g, heights=(100, 110, 120, 130, 300)):
    """five maxima five bins apart, on bins 4, 9, 14, 19, 24, rising: the highest is the LAST (cut away by maxfreqs < 5)"""
    sp = []
    for q, h in enumerate(heights):
        sp += pair(4 + 5 * q, h)
    return rows_of(g, profile(g, 1, sp)), [4 + 5 * q for q in range(len(heights))]


def plateaus(g, h=50):
    """two equal adjacent bins (2, 3: spikes five apart), three (13, 14, 15: four apart), and one peak with equal
    neighbours on bin finpb - 2"""
    j = g.finpb - 2
    return rows_of(g, profile(g, 1, [(0, h), (5, h), (12, h), (16, h)] + pair(j, h)))


def edges_in(g, h=50):
    """maxima on the first and the last eligible bin, j = 1 and j = finpb - 2"""
    return rows_of(g, profile(g, 1, pair(1, h) + pair(g.finpb - 2, h + 10)))


def edges_out(g, h=50):
    """maxima on j = 0 and j = finpb - 1: no candidate"""
    return rows_of(g, profile(g, 1, pair(0, h) + pair(g.finpb - 1, h + 10)))


def ties(g, h=50):
    """one peak on bin 20; every bin it does not reach holds the same 7-tap sum, the percentile among them"""
    return rows_of(g, profile(g, 1, pair(20, h)))


def zero_noise(g, h=50):
    """all-zero columns under bins 0 .. noiseidx + 4: the percentile is 0, smspec holds NaN (0/0) and +inf"""
    p = profile(g, 1, pair(g.finpb - 6, h))
    p[:g.col(g.noiseidx + 4) + 4] = 0
    return rows_of(g, p)


# ------------------------------------------------------------------------------------------------------ K3 inputs
def _sign():
    return 2.0 * O.pr3().astype(np.float64) - 1.0


def cell_gradients(g, j, halo=5):
    """d ss / d x of the drift-0 linear numerator of every cell (cc:207 with ifd = ifr), x = sqrt(ps):
    +-(2*pr3[k] - 1) on rows k0 + 2k at columns ifr - 3, ifr - 1, ifr + 1, ifr + 3.  -> [130][n][2*halo + 1], column 0 of
    the window = if0 - halo"""
    s = _sign()
    G = np.zeros((NCELL, g.n, 2 * halo + 1))
    rows2 = 2 * np.arange(NSYM)
    for ifr_i in range(NIFR):
        c = halo - 2 + ifr_i                                  # window column of ifr
        for k0 in range(NK0):
            a = G[ifr_i * NK0 + k0]
            a[k0 + rows2, c - 3] -= s
            a[k0 + rows2, c - 1] += s
            a[k0 + rows2, c + 1] -= s
            a[k0 + rows2, c + 3] += s
    return G


def bump(g, j, base=10.0, height=20.0, halfwidth=4):
    """x0: `base` plus a triangular column bump centred on the candidate's column (identical rows).  Seven columns wide
    at half-width 4: narrower than the 7-tap window it would smooth into a plateau, not a peak."""
    c = np.arange(g.size)
    x = base + height * np.maximum(0.0, 1.0 - np.abs(c - g.col(j)) / float(halfwidth))
    return np.tile(x, (g.n, 1))


def bump_skew(g, j):
    """x0 for the `zero` and `nan` cases: a bump with its peak on the candidate's column whose rise from if0 - 5 to
    if0 - 3 equals its fall from if0 - 1 to if0 + 1, so that (x[if0-3] + x[if0+1]) - (x[if0-5] + x[if0-1]) = 0 exactly"""
    x = np.full(g.size, 10.0)
    x[g.col(j) - 4:g.col(j) + 5] = [10, 15, 20, 25, 30, 20, 15, 12, 10]
    return np.tile(x, (g.n, 1))


def design(g, j, target, x0=None, hold=(), halo=5):
    """Least squares: x = x0 + sum a_c g_c with g_c . x = target[c] for the 130 cells of a candidate on bin j; columns in
    `hold` (offsets from if0) keep x0 and the cells that lose their whole gradient to them drop out.  -> ps = float32(x)^2"""
    x0 = bump(g, j) if x0 is None else np.array(x0, np.float64)
    G = cell_gradients(g, j, halo)
    win = slice(g.col(j) - halo, g.col(j) + halo + 1)
    ss0 = G.reshape(NCELL, -1) @ x0[:, win].reshape(-1)        # the numerators of x0, held columns included
    for o in hold:
        G[:, :, halo + o] = 0.0
    Gf = G.reshape(NCELL, -1)
    live = np.nonzero(np.abs(Gf).sum(axis=1) > 0)[0]
    rhs = np.asarray(target, np.float64)[live] - ss0[live]
    a = np.linalg.solve(Gf[live] @ Gf[live].T, rhs)
    x = x0.copy()
    x[:, win] += (a @ Gf[live]).reshape(g.n, -1)
    assert x.min() > 0, "the design left the positive quadrant"
    x32 = x.astype(np.float32)
    return x32 * x32


T_FLAT = np.full(NCELL, -50.0)
T_RAMP = np.linspace(-100.0, -1.0, NCELL)
T_TAIL = np.r_[np.full(NCELL - 1, -50.0), -0.5]      # the last cell's numerator next to zero: see _k_tail
T_HELD = np.full(NCELL, -10.0)      # with four columns held the system is stiffer: smaller numerators keep x > 0


PRUNED_PEAK = 1600.0    # ss of cell 60: with pw of about 13 000 there the metric passes 1.001 / 10


def t_pruned(seed=7):
    t = np.random.default_rng(seed).uniform(-50.0, 50.0, NCELL)
    t[:60] = -50.0
    t[60] = PRUNED_PEAK
    return t


HOLD = (-5, -3, -1, 1)      # the four columns of the first tuned bin's drift-0 path (ifr = if0 - 2)


def allneg(g, j, target=T_FLAT):
    return design(g, j, target)


def pruned(g, j):
    return design(g, j, t_pruned())


def zero(g, j):
    """the first tuned bin's linear path sees four row-constant columns, pairwise equal: its 26 metrics are exactly 0"""
    return design(g, j, T_HELD, x0=bump_skew(g, j), hold=HOLD)


def nan(g, j):
    """those columns zero on even rows and x0 * sqrt 2 on odd rows (same column sums): 0/0 for every even k0 there"""
    x0 = bump_skew(g, j)
    ps = design(g, j, T_HELD, x0=x0, hold=HOLD)
    for o in HOLD:
        c = g.col(j) + o
        v = x0[0, c].astype(np.float32)
        ps[0::2, c] = 0.0
        ps[1::2, c] = np.float32(2.0) * (v * v)
    return ps


def seeded(g, j, seed=11):
    """the ordinary case: exponential noise (positive, seed fixed) under the same bump"""
    x0 = bump(g, j).astype(np.float32)
    e = np.random.default_rng(seed).exponential(1.0, x0.shape).astype(np.float32)
    return (x0 * x0) * e


def k3_oracle(g, full, limit=None):
    """peaks of `full`, then the search with its grid for the first `limit` of them -> (peaks, [(cand, grid)])"""
    k2 = k2_oracle(g, full)
    pk = k2["peaks"]
    return pk, [g.fdr.search(full, pk[q:q + 1], want_grid=True) for q in range(len(pk) if limit is None else min(limit, len(pk)))]


# ------------------------------------------------------------------------------ the cases and what must hold for each
WIDEST_HALFBANDWIDTH = 181     # the widest pass band the oracle and the library both accept (182: both refuse)
ODD_GEOMETRY = dict(fl=45056, halfbandwidth=8, cf=3000)     # n = 349, band_w = 43: n * band_w is no multiple of 4
EVEN_GEOMETRY = dict(fl=45056, halfbandwidth=8)             # n = 349, band_w = 36: a multiple of 4


def bin_of(g, freq):
    return int(round(float(freq) / float(g.df))) + g.hpbm


def _c_comb(g, k2):
    """(finpb - 1) // 2 maxima, every snr equal, so the stable order is by ascending bin; cut to maxfreqs"""
    mx = maxima(k2["smspec"])
    assert mx == list(range(1, g.finpb - 1, 2)) and len(mx) == (g.finpb - 1) // 2
    pk = k2["peaks"]
    assert len(pk) == min(len(mx), g.maxfreqs)
    assert len(set(pk["snr"].tobytes()[4 * q:4 * q + 4] for q in range(len(pk)))) == 1
    assert [bin_of(g, f) for f in pk["freq"]] == mx[:len(pk)]
    low = k2["smraw"][0::2]                                 # half the bins share the low sum: the percentile sits in a tie
    assert (low == k2["noise"]).all() and low.size >= g.noiseidx + 1
    return {"maxima": len(mx), "peaks": len(pk)}


def _c_comb_cut(g, k2):
    r = _c_comb(g, k2)
    assert r["maxima"] > g.maxfreqs == r["peaks"] == 200
    return r


def _c_cut(g, k2):
    """the list holds the first maxfreqs maxima by position, and not the highest"""
    mx = maxima(k2["smspec"])
    assert mx == [4, 9, 14, 19, 24]
    h = k2["smspec"][mx]
    assert (np.diff(h) > 0).all()                                   # distinct, rising: the highest is the last
    pk = k2["peaks"]
    assert len(pk) == g.maxfreqs < len(mx)
    assert sorted(bin_of(g, f) for f in pk["freq"]) == mx[:g.maxfreqs]
    assert [bin_of(g, f) for f in pk["freq"]] == mx[:g.maxfreqs][::-1]      # and in descending snr
    assert mx[-1] not in [bin_of(g, f) for f in pk["freq"]]
    return {"maxima": len(mx), "peaks": len(pk)}


def _c_plateaus(g, k2):
    s = k2["smspec"]
    assert s[2] == s[3] and s[2] > s[1] and s[3] > s[4]
    assert s[13] == s[14] == s[15] and s[13] > s[12] and s[15] > s[16]
    j = g.finpb - 2
    assert s[j - 1] == s[j + 1] < s[j]
    assert [bin_of(g, f) for f in k2["peaks"]["freq"]] == [j]
    return {"peaks": 1}


def _c_edges_in(g, k2):
    assert sorted(bin_of(g, f) for f in k2["peaks"]["freq"]) == [1, g.finpb - 2]
    return {"peaks": 2}


def _c_edges_out(g, k2):
    s = k2["smspec"]
    assert s[0] > s[1] and s[-1] > s[-2] and len(k2["peaks"]) == 0 and maxima(s) == []
    return {"peaks": 0}


def _c_ties(g, k2):
    assert int((k2["smraw"] == k2["noise"]).sum()) >= g.noiseidx + 2
    assert [bin_of(g, f) for f in k2["peaks"]["freq"]] == [20]
    return {"tied": int((k2["smraw"] == k2["noise"]).sum())}


def _c_zero_noise(g, k2):
    assert int((k2["smraw"] == 0).sum()) > g.noiseidx and k2["noise"] == 0
    s = k2["smspec"]
    assert np.isnan(s).any() and np.isposinf(s).any()
    return {"zeros": int((k2["smraw"] == 0).sum()), "nan": int(np.isnan(s).sum()), "inf": int(np.isposinf(s).sum()),
            "peaks": len(k2["peaks"])}


def _c_flat(g, k2):
    assert len(k2["peaks"]) == 0 and len(set(k2["smraw"].tolist())) == 1
    return {"peaks": 0}


# name -> (constructor arguments, builder(g) -> full spectrogram [n][512], condition(g, k2_oracle) -> figures)
K2_CASES = {
    "comb_hb1": (dict(halfbandwidth=1), comb, _c_comb),
    "comb_hb2": (dict(halfbandwidth=2), comb, _c_comb),
    "comb_hb10": (dict(), comb, _c_comb),
    "comb_hb60_unstaged": (dict(halfbandwidth=60), comb, _c_comb),
    "comb_widest": (dict(halfbandwidth=WIDEST_HALFBANDWIDTH), comb, _c_comb_cut),
    "cut1": (dict(maxfreqs=1), lambda g: five_peaks(g)[0], _c_cut),
    "cut2": (dict(maxfreqs=2), lambda g: five_peaks(g)[0], _c_cut),
    "cut3": (dict(maxfreqs=3), lambda g: five_peaks(g)[0], _c_cut),
    "plateaus": (dict(), plateaus, _c_plateaus),
    "edges_in": (dict(), edges_in, _c_edges_in),
    "edges_out": (dict(), edges_out, _c_edges_out),
    "ties": (dict(), ties, _c_ties),
    "zero_noise": (dict(), zero_noise, _c_zero_noise),
    "flat": (dict(), flat, _c_flat),
    "comb_scalar_copy": (ODD_GEOMETRY, comb, _c_comb),
    "comb_vector_copy": (EVEN_GEOMETRY, comb, _c_comb),
}
BATCH_K2 = ("flat", "comb_hb10", "flat", "comb_hb10")      # frames without a peak beside frames with peaks


def k3_figures(g, full, j):
    """search the candidate(s) of `full` on the oracle, replay the rule over each grid and check that the replay IS the
    oracle's search (sync, shift, m_type, freq).  -> (peaks, [(cand, grid)], [figures])"""
    pk, res = k3_oracle(g, full)
    figs = []
    for q, (c, grid) in enumerate(res):
        (best, gb), acc = replay(grid, g.nlin, g.threshold)
        w = winner_record(g, bin_of(g, pk[q]["freq"]), gb, best)
        assert same_float(c["sync"], w["sync"]) and int(c["shift"]) == w["shift"] and int(c["m_type"]) == w["m_type"]
        assert np.float32(c["freq"]).tobytes() == w["freq"].tobytes()
        fg = classify(g, grid, acc)
        fg.update(sync=float(c["sync"]), winner_cell=gb // g.hc, winner_entry=gb, bin=bin_of(g, pk[q]["freq"]))
        figs.append(fg)
    return pk, res, figs


def _k_allneg(g, j, figs):
    """every linear numerator negative: nonlinear acceptances under a negative running best, a negative final sync"""
    f, = figs
    assert f["bin"] == j and f["neg_cells_before_cstar"] == NCELL == f["cstar"]
    assert f["nl_neg"] >= (100 if g.threshold == 1 else 10) and f["nl_pos"] == 0 and f["nl_zero"] == 0
    assert f["sync"] < 0


def _k_tail(g, j, figs):
    """threshold 10: a nonlinear acceptance under a negative best is undone by the next linear hypothesis (any of them
    is greater), so it shows in the record only after the LAST linear one.  Here the last cell's linear metric is next to
    zero, one of its nonlinear metrics is ten times below it, and the winner lies in a 64-entry slice of the replay that
    holds no linear hypothesis: a slice only its minimum over the nonlinear metrics can keep from being skipped."""
    _k_allneg(g, j, figs)
    e = figs[0]["winner_entry"]
    assert e // g.hc == NCELL - 1 and all((q % g.hc) >= g.nlin for q in range(e // 64 * 64, min(e // 64 * 64 + 64, NCELL * g.hc)))


def _k_pruned(g, j, figs):
    f, = figs
    assert f["bin"] == j and f["cstar"] == 60 == f["winner_cell"] and f["neg_cells_before_cstar"] == 60


def _k_zero(g, j, figs):
    f, = figs
    assert f["bin"] == j and f["zeros"] >= 26 and f["nl_zero"] >= 1


def _k_nan(g, j, figs):
    f, = figs
    assert f["bin"] == j and f["nans"] >= 1 and f["nans"] < NCELL * g.hc


def _k_seeded(g, j, figs):
    assert len(figs) >= 1 and j in [f["bin"] for f in figs]


# name -> (threshold, bin, builder(g, j), condition); all at the default geometry
def _k3_cases():
    c = {}
    for thr in (1, 10):
        for tag, j in (("first", 1), ("last", -2), ("mid", 13)):
            c["allneg_flat_%s_t%d" % (tag, thr)] = (thr, j, allneg, _k_allneg)
        c["allneg_ramp_mid_t%d" % thr] = (thr, 13, lambda g, j: allneg(g, j, T_RAMP), _k_allneg)
        c["seeded_t%d" % thr] = (thr, 13, seeded, _k_seeded)
    c["allneg_tail_t10"] = (10, 13, lambda g, j: allneg(g, j, T_TAIL), _k_tail)
    c["pruned_t10"] = (10, 13, pruned, _k_pruned)
    c["zero_t10"] = (10, 13, zero, _k_zero)
    c["nan_t10"] = (10, 13, nan, _k_nan)
    return c


K3_CASES = _k3_cases()


def k3_build(g, name):
    """-> (full spectrogram, bin) of a K3 case in geometry g (bin -2 = the last eligible one, finpb - 2)"""
    thr, j, build, cond = K3_CASES[name]
    j = j if j >= 0 else g.finpb + j
    return build(g, j), j


_GEOMS = {}


def geom(**kw):
    """one Geom (and one oracle FDR) per set of constructor arguments, shared by the tests of a session"""
    key = tuple(sorted(kw.items()))
    if key not in _GEOMS:
        _GEOMS[key] = Geom(**kw)
    return _GEOMS[key]
