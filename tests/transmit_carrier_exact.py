"""TEST INFRASTRUCTURE ONLY -- K7's carrier form (gr-uwspr_amd/csrc/k7_transmit.hip, template flag CARRIER) restated to
the bit in numpy, no GPU needed, on top of tests/transmit_exact.py (the chain) and tests/carrier_exact.py (the rotator).

Channel c's audio sample n before noise, background and quantiser (include/uwspr_hip.h, "Transmit at another carrier"):

  groups   the channel's signals by carrier, the distinct carriers ascending in Hz: f_1 < ... < f_G
  x_f[j]   the group's baseband in the file orientation (given: the device's own, from tx_baseband on that group's signals)
  xr_f[j]  carrier_exact.rotate(x_f, f, j, table): x_f's bytes when 375 divides f, else one product in K0's order with
           rot[((f mod 375)(j mod 375)) mod 375], j mod 375 in 0 .. 374 for negative j as well
  chain_f  transmit_exact.chain(image_f, xr_f, n, x0)
  a        chain_{f_1}, then a = fl32(a + chain_{f_g}) for g = 2 .. G

  expect               that, from per-group basebands
  MUTATIONS, mutated   the mistakes the byte comparison must see, as changed expectations
  per_signal_rotation  the rotator applied to every signal after its gain, the rotated signals then added
  two_stage            the flowgraph's chain in float64 at a carrier (no claim about order): the independent check
  response             a tap set's frequency response"""
import numpy as np

import carrier_exact as CX
import transmit_exact as X

NROT = CX.NROT


def rotated(x, fc, j, table, **kw):
    """x = (re, im) float32 of baseband samples j (int64, absolute) -> (re, im) after carrier fc's rotator"""
    s = np.stack([np.asarray(x[0], np.float32), np.asarray(x[1], np.float32)], axis=1)
    y = CX.rotate(s, fc, j, table, **kw)
    return np.ascontiguousarray(y[:, 0]), np.ascontiguousarray(y[:, 1])


def expect(groups, n, x0, table, mutation=None):
    """groups: {carrier Hz: (image [32, 104, 2] float32, (re, im) float32 of baseband samples [x0, x0 + len))} of one
    channel; n: absolute audio indices -> float32 audio before noise, background and quantiser."""
    n = np.asarray(n, np.int64).reshape(-1)
    fcs = sorted(groups)
    j = int(x0) + np.arange(len(groups[fcs[0]][1][0]), dtype=np.int64)
    order = list(fcs)
    if mutation == "groups_in_given_order":
        order = list(groups)                                   # (the dict's own order: the order the signals came in)
    a = None
    for k, f in enumerate(order):
        image, x = groups[f]
        fr = f
        if mutation == "other_groups_rotator":
            fr = order[(k + 1) % len(order)]
        if mutation == "plus_sin":
            xr = rotated(x, fr, j, table, conj=True)
        elif mutation == "index_from_n":
            xr = rotated(x, fr, j, table, index=((int(fr) % NROT) * ((32 * j) % NROT)) % NROT)
        elif mutation == "c_remainder":
            # C's %: the dividend's sign, so a negative j gives a negative row; a kernel that then drops the sign reads
            # row (f |j mod 375|) mod 375 -- the same row as the right one for every j >= 0
            jm = np.abs(np.fmod(j, NROT))
            xr = rotated(x, fr, j, table, index=((int(fr) % NROT) * jm) % NROT)
        elif mutation == "fc_not_reduced":
            # the product fc (j mod 375) taken in 16 bits before the reduction (what an unreduced fc overflows first)
            xr = rotated(x, fr, j, table, index=((int(fr) * (j % NROT)) % 65536) % NROT)
        else:
            xr = rotated(x, fr, j, table)
        c = X.chain(image, xr, n, x0=x0)
        a = c if a is None else (a + c)
        assert a.dtype == np.float32
    return a


MUTATIONS = ("plus_sin", "index_from_n", "c_remainder", "fc_not_reduced", "other_groups_rotator", "groups_in_given_order")


def per_signal_rotation(image, xs, fc, n, x0, table):
    """one group whose signals are rotated one by one (after their gain) and then added in index order; xs: the (re, im)
    of every signal alone"""
    j = int(x0) + np.arange(len(xs[0][0]), dtype=np.int64)
    re = np.zeros(len(j), np.float32)
    im = np.zeros(len(j), np.float32)
    for x in xs:
        r, i = rotated(x, fc, j, table)
        re, im = re + r, im + i
    return X.chain(image, (re, im), n, x0=x0)


# ---- the independent restatement --------------------------------------------------------------------------------------
def two_stage(x_file, nout, fc, cutoff=2500):
    """c2ToWaveFile.grc in float64 at Center_Frequency fc on the baseband as the .c2 FILE holds it, from sample 0:
    zero-stuff x32, h1, freq_xlating_fir_filter's rotated h2, the mixer, the real part"""
    import scipy.signal as ss
    import frontend_grc as F
    h1 = F.low_pass(1, 12000, 200, 10).astype(np.float64)
    h2r = F.xlating_taps(F.low_pass(1, 12000, cutoff, 100), float(fc)).astype(np.complex128)
    u = np.zeros(len(x_file) * 32, np.complex128)
    u[::32] = x_file
    v = ss.oaconvolve(ss.oaconvolve(u, h1)[:len(u)], h2r)[:nout]
    k = np.arange(nout, dtype=np.int64)
    return (v * np.exp(-2j * np.pi * ((int(fc) * (k % 12000)) % 12000) / 12000.0)).real


def response(g, f_hz):
    """sum_q g[q] e^{-j 2 pi f q / 12000} at the frequencies f_hz"""
    q = np.arange(len(g), dtype=np.float64)
    return np.array([(g * np.exp(-2j * np.pi * f * q / 12000.0)).sum() for f in np.atleast_1d(f_hz)])
