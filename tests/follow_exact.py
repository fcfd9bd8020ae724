"""K16 (uwspr_follow_set, uwspr_follow_batch) restated in numpy binary64 from include/uwspr_hip.h: the grid powers P_i(j, l)[g]
along a pass, the sync metric S of every hypothesis h = (j nf + (q + qf)) nlg + (l + nl), s_ref, the pick, and the soft
symbols of one hypothesis with K10's normalisation.  The tables are tests/track_exact.py's design.  Shared by
tests/test_follow.py (no GPU), tests/test_gpu_follow.py and tests/test_gpu_follow_pipe.py."""
import numpy as np

import track_exact as TX

NSYM, SPB, MID, FS = TX.NSYM, TX.SPB, TX.MID, TX.FS
Q = 375.0 / 2048.0            # df / 8
LSTEP = 32
# the sync bit of symbol i (the LSB of any uwspr_wspr_symbols): include/uwspr_hip.h's pr3, as gr-uwspr_amd/synth.py holds it
_PR3 = None


def pr3():
    global _PR3
    if _PR3 is None:
        import gr_uwspr_amd as G
        _PR3 = np.asarray(G.synth.PR3, np.int64).copy()
    return _PR3


def hyp(j, q, l, qf, nl):
    return (j * (2 * qf + 1) + (q + qf)) * (2 * nl + 1) + (l + nl)


def unhyp(h, qf, nl):
    nf, nlg = 2 * qf + 1, 2 * nl + 1
    return h // (nf * nlg), (h // nlg) % nf - qf, h % nlg - nl


def powers(x, shift, f_sym, tau_row, lag, gmax):
    """P [162, 2 gmax + 1] of one (trajectory, lag): x complex128 [fl]; f_sym [162] = f_hz + dfreq[j] in binary64;
    grid index g = -gmax .. gmax at f_sym + g Q.  The rotator of (g, k) is e^{-j 2 pi (g k mod 2048) / 2048}: Q / 375 = 1 / 2048."""
    X = TX._windows(x, int(shift) + LSTEP * int(lag), tau_row)
    k = np.arange(SPB)
    Y = X * np.exp(-2j * np.pi * (np.asarray(f_sym, np.float64)[:, None] / FS) * k[None, :])
    g = np.arange(-gmax, gmax + 1)
    E = np.exp(-2j * np.pi * ((k[:, None] * g[None, :]) % 2048) / 2048.0)
    return np.abs(Y @ E)


def sync_of(P, qf):
    """P [162, 2 qf + 25] -> S [nf]: tone t of offset q is grid index q + 8 t - 12, slot (q + qf) + 8 t"""
    nf = 2 * qf + 1
    sg = (2.0 * pr3() - 1.0)[:, None]
    p = [P[:, 8 * t:8 * t + nf] for t in range(4)]
    num = (sg * ((p[1] + p[3]) - (p[0] + p[2]))).sum(axis=0)
    den = (((p[0] + p[1]) + p[2]) + p[3]).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))


def surface(frame, shift, f_hz, dfreq, tau, qf, nl):
    """S [n, nf, nlg] of one item; f_hz is taken as the binary32 the item holds"""
    x = TX.as_complex(frame)
    f0 = float(np.float32(f_hz))
    out = np.empty((len(dfreq), 2 * qf + 1, 2 * nl + 1))
    for j in range(len(dfreq)):
        for l in range(-nl, nl + 1):
            out[j, :, l + nl] = sync_of(powers(x, shift, f0 + dfreq[j], tau[j], l, qf + 12), qf)
    return out


def line(f_hz, drift_hz):
    f0, dr = float(np.float32(f_hz)), float(np.float32(drift_hz))
    return f0 + 0.5 * dr * ((np.arange(NSYM) - MID) / 81.0)


def s_ref(frame, shift, f_hz, drift_hz):
    return float(sync_of(powers(TX.as_complex(frame), shift, line(f_hz, drift_hz), np.zeros(NSYM, np.int64), 0, 12), 0)[0])


first_max = TX.first_max


def normalise(soft):
    """K10's text: fsum, f2sum the means of the 162 values and their squares, fac = sqrt(f2sum - fsum^2), v = 50 soft / fac
    clipped to [-128, 127], byte = (uint8)(v + 128); 128 everywhere when fac is no positive finite number"""
    soft = np.asarray(soft, np.float64)
    fsum, f2sum = 0.0, 0.0
    for v in soft:
        fsum += v / 162.0
        f2sum += v * v / 162.0
    with np.errstate(invalid="ignore"):
        fac = np.sqrt(f2sum - fsum * fsum)
    if not (fac > 0.0 and np.isfinite(fac)):
        return np.full(NSYM, 128, np.uint8)
    v = np.clip(50.0 * soft / fac, -128.0, 127.0)
    return np.where(np.isnan(v), 128, np.trunc(np.nan_to_num(v) + 128.0)).astype(np.uint8)


def soft_values(frame, shift, f_hz, dfreq_row, tau_row, q, lag):
    """soft[i] = p_i[pr3[i] + 2] - p_i[pr3[i]] of one hypothesis, binary64"""
    f0 = float(np.float32(f_hz))
    P = powers(TX.as_complex(frame), shift, f0 + dfreq_row, tau_row, lag, abs(q) + 12)
    c = abs(q) + 12 + q - 12                      # slot of grid index q - 12
    i, b = np.arange(NSYM), pr3()
    return P[i, c + 8 * (b + 2)] - P[i, c + 8 * b]


def symbols(frame, shift, f_hz, dfreq_row, tau_row, q, lag):
    return normalise(soft_values(frame, shift, f_hz, dfreq_row, tau_row, q, lag))


def follow(frame, shift, f_hz, dfreq, tau, qf, nl):
    """-> (best, S [n, nf, nlg], the 162 bytes at best)"""
    S = surface(frame, shift, f_hz, dfreq, tau, qf, nl)
    best = first_max(S)
    j, q, l = unhyp(best, qf, nl)
    return best, S, symbols(frame, shift, f_hz, dfreq[j], tau[j], q, l)


def rms(sym):
    """the fine search's rms of 162 bytes about 128 (cc:469-474)"""
    y = np.asarray(sym).astype(np.float32) - np.float32(128.0)
    sq = np.float32(0.0)
    for v in y:
        sq = np.float32(sq + v * v)
    return np.float32(np.sqrt(np.float64(sq) / 162.0))
