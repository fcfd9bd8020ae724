"""TEST INFRASTRUCTURE ONLY -- K0's carrier form (gr-uwspr_amd/csrc/k0_frontend.hip, template flag CAR) restated to the
bit in numpy, no GPU needed, on top of tests/frontend_exact.py.

The carrier form is K0's sum with other taps, then the rotator (include/uwspr_hip.h, "The rotator"):

  s        the sum K0 forms at any carrier: frontend_exact.restate_many with carrier k's binary32 taps
  index    ((fc mod 375) (m mod 375)) mod 375 for the 64-bit stream index m
  (c, d)   = rot[index], the library's table (uwspr_frontend_rotator): ((float)cos, (float)(-sin))(2 pi index / 375)
  y.re     = fmaf(s.re, c, -(s.im d))
  y.im     = fmaf(s.re, d, s.im c)            one order; not applied at all when 375 divides fc

and plane q = c NC + k holds audio channel c at carrier k.

  rot_index, rotate     the rotator on sums that are already there (a restatement's, or the kernel's own from the door
                        of the forms without a rotator)
  restate_planes        the planes of one launch, [nch NC][len(ms), 2]
  MUTATIONS, mutated    the mistakes the tests must be able to see, as changed expectations
  shift_band            the numpy side of the decode test: a band of a recording moved to another carrier"""
import numpy as np

import frontend_exact as X
from frontend_exact import fma32, restate_many, taps_J  # noqa: F401  (taps_J: re-exported for the tests)

NROT = 375


def rot_index(fc, ms):
    """the table row of outputs ms (int64 stream indices) at carrier fc"""
    ms = np.asarray(ms, np.int64)
    return ((int(fc) % NROT) * (ms % NROT)) % NROT


def _mul32(a, b):
    """the correctly rounded binary32 product (exact in binary64, one cast)"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def rotate(s, fc, ms, table, index=None, conj=False):
    """s: float32 [n, 2] sums of outputs ms -> the carrier form's bytes.  index / conj: the mutations' way in."""
    s = np.asarray(s, np.float32)
    if int(fc) % NROT == 0 and index is None:
        return s.copy()
    idx = rot_index(fc, ms) if index is None else np.asarray(index, np.int64)
    c, d = table[idx, 0], table[idx, 1]
    if conj:
        d = -d
    out = np.empty_like(s)
    out[:, 0] = fma32(s[:, 0], c, -_mul32(s[:, 1], d))
    out[:, 1] = fma32(s[:, 0], d, _mul32(s[:, 1], c))
    return out


def restate_planes(taps32, D, table, carriers, x, x_origin, ms, mutation=None):
    """taps32: per carrier the binary32 composite taps; x: float32 [nin, nch] frames [x_origin, x_origin + nin); ms:
    absolute output indices -> list of nch * NC float32 [len(ms), 2] arrays in the kernel's plane order."""
    x = np.asarray(x, np.float32)
    nch, NC = x.shape[1], len(carriers)
    ms = np.asarray(ms, np.int64)
    planes = [None] * (nch * NC)
    for k, fc in enumerate(carriers):
        sums = restate_many(taps32[k], D, [(np.ascontiguousarray(x[:, c]), x_origin, ms) for c in range(nch)])
        for c in range(nch):
            q, kr = c * NC + k, k
            if mutation == "plane_k_nch_plus_c":
                q = k * nch + c
            if mutation == "other_carriers_rotator":
                kr = (k + 1) % NC
            fr = carriers[kr]
            if mutation == "plus_sin":
                y = rotate(sums[c], fr, ms, table, conj=True)
            elif mutation == "index_from_32m":
                y = rotate(sums[c], fr, ms, table, index=((int(fr) % NROT) * ((32 * ms) % NROT)) % NROT)
            elif mutation == "fc_not_reduced":
                # the product fc (m mod 375) taken in 16 bits before the reduction (what an unreduced fc overflows first)
                y = rotate(sums[c], fr, ms, table, index=((int(fr) * (ms % NROT)) % 65536) % NROT)
            else:
                y = rotate(sums[c], fr, ms, table)
            planes[q] = y
    return planes


MUTATIONS = ("plus_sin", "index_from_32m", "fc_not_reduced", "other_carriers_rotator", "plane_k_nch_plus_c")


def shift_band(x, lo, hi, df, fs=12000.0):
    """x (real) masked to [lo, hi] Hz with an FFT and moved up by df Hz through its analytic signal -> float64, real"""
    x = np.asarray(x, np.float64)
    n = len(x)
    F = np.fft.fft(x)
    f = np.fft.fftfreq(n, 1.0 / fs)
    A = np.where((f >= lo) & (f <= hi), 2.0 * F, 0.0)          # the band's analytic signal
    a = np.fft.ifft(A)
    t = np.arange(n, dtype=np.float64)
    ph = 2.0 * np.pi * ((int(df) * (t % fs)) % fs) / fs if float(df).is_integer() else 2.0 * np.pi * df * t / fs
    return (a * np.exp(1j * ph)).real
