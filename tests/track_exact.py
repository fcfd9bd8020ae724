"""K15 (uwspr_track_design, uwspr_track_batch) restated in numpy binary64 from include/uwspr_hip.h: the per-symbol Doppler
and delay tables in the header's one operation order, the score T of every hypothesis, T_ref, the pick -- and a moving
transmission synthesised from the header's UWSPR_TX_DOPPLER / UWSPR_TX_DELAY formulas, without the library.  Shared by
tests/test_track.py (no GPU) and tests/test_gpu_track.py."""
import numpy as np

NSYM, SPB, MID = 162, 256, 81
N = NSYM * SPB
FS, DF, DFQ, C_SOUND = 375.0, 375.0 / 256.0, 0.0125, 1500.0
T_SYM = (SPB * np.arange(NSYM) + 128).astype(np.float64) / FS      # symbol centres, s from the item's first sample
FL = 45000


def _cols(trajs):
    a = np.asarray(trajs)
    if a.dtype.names:
        return (a[k].astype(np.float64).reshape(-1, 1) for k in ("v", "d", "tc"))
    a = np.asarray(trajs, np.float64).reshape(-1, 3)
    return (a[:, k:k + 1] for k in range(3))


def ranges(trajs, t):
    """R(t), Rdot(t) [n, len(t)] in the header's order: a = v (t - tc), R = sqrt(d d + a a), Rdot = (v a) / R"""
    v, d, tc = _cols(trajs)
    a = v * (np.asarray(t, np.float64)[None, :] - tc)
    R = np.sqrt(d * d + a * a)
    return R, (v * a) / R


def design(trajs, model, cf=1500.0):
    """-> dfreq [n, 162] float64, tau [n, 162] int32"""
    R, D = ranges(trajs, T_SYM)
    dfreq = -((float(cf) / C_SOUND) * (D - D[:, MID:MID + 1]))
    tau = np.rint((FS * (R - R[:, MID:MID + 1])) / C_SOUND).astype(np.int32)
    return dfreq, (tau if model == "delay" else np.zeros_like(tau))


def _windows(x, shift, tau_row):
    """x [fl] complex128 -> [162, 256]: x[shift + 256 i + tau[i] + k], 0 outside [0, fl)"""
    idx = int(shift) + SPB * np.arange(NSYM)[:, None] + np.asarray(tau_row, np.int64)[:, None] + np.arange(SPB)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], 0.0)


def _score(X, f_sym):
    """X [162, 256], f_sym [..., 162] Hz -> T [...]"""
    ph = np.exp(-2j * np.pi * (f_sym[..., None] / FS) * np.arange(SPB))
    return np.abs((X * ph).sum(axis=-1)).sum(axis=-1)


def as_complex(frame):
    f = np.asarray(frame)
    return f[:, 0].astype(np.float64) + 1j * f[:, 1].astype(np.float64)


def surface(frame, shift, f_hz, symbols, dfreq, tau, qf):
    """T [n, nf] of one item; f_hz is taken as the binary32 the item holds"""
    x = as_complex(frame)
    f0 = float(np.float32(f_hz))
    tone = (np.asarray(symbols, np.float64) - 1.5) * DF
    q = np.arange(-qf, qf + 1, dtype=np.float64)
    out = np.empty((len(dfreq), len(q)))
    for j in range(len(dfreq)):
        f_sym = ((f0 + DFQ * q)[:, None] + dfreq[j][None, :]) + tone[None, :]
        out[j] = _score(_windows(x, shift, tau[j]), f_sym)
    return out


def t_ref(frame, shift, f_hz, drift_hz, symbols):
    f0, dr = float(np.float32(f_hz)), float(np.float32(drift_hz))
    f_sym = (f0 + 0.5 * dr * ((np.arange(NSYM) - MID) / 81.0)) + (np.asarray(symbols, np.float64) - 1.5) * DF
    return float(_score(_windows(as_complex(frame), shift, np.zeros(NSYM, np.int64)), f_sym))


def first_max(T):
    """the header's pick over T flattened in ascending h: moves on `>` alone"""
    T = np.asarray(T).reshape(-1)
    best, bm = 0, T[0]
    for h in range(1, len(T)):
        if T[h] > bm:
            best, bm = h, T[h]
    return best


def synth(symbols, traj, model, start, f0=0.0, cf=1500.0, fl=FL, gain=1.0):
    """A moving transmission in a frame of fl complex samples, from the header's formulas alone (phase0 = 0, no drift):
    t = k / 375 from the first sample, D(t) = (R(t) - R(0)) / c; "doppler": y(k) = e^{j [theta(k) - 2 pi fc D]};
    "delay": k' = k - 375 D, y(k) = e^{j [theta(k') - 2 pi fc D]} for 0 <= k' < N, theta the per-symbol phase at a fractional
    index."""
    fsym = f0 + (np.asarray(symbols, np.float64) - 1.5) * DF
    cum = np.concatenate([[0.0], np.cumsum(SPB * fsym)])
    k = np.arange(-400, N + 400, dtype=np.float64)
    R, _ = ranges([traj], k / FS)
    R0, _ = ranges([traj], np.zeros(1))
    D = (R[0] - R0[0, 0]) / C_SOUND
    kp = k - FS * D if model == "delay" else k
    ok = (kp >= 0) & (kp < N)
    i = np.clip(np.floor(kp / SPB).astype(np.int64), 0, NSYM - 1)
    theta = 2.0 * np.pi / FS * (cum[i] + (kp - SPB * i) * fsym[i])
    y = np.where(ok, gain * np.exp(1j * (theta - 2.0 * np.pi * cf * D)), 0.0)
    out = np.zeros(fl, np.complex128)
    at = start + k.astype(np.int64)
    m = (at >= 0) & (at < fl)
    out[at[m]] = y[m]
    return np.stack([out.real, out.imag], axis=1).astype(np.float32)


def truth_item(traj, model, start, f0=0.0, cf=1500.0):
    """the (shift, f) a perfect decoder would hand over for synth()'s signal: aligned and tuned at mid-transmission"""
    R, D = ranges([traj], np.array([0.0, T_SYM[MID]]))
    shift = start + (int(np.rint(FS * (R[0, 1] - R[0, 0]) / C_SOUND)) if model == "delay" else 0)
    return shift, float(np.float32(f0 - (cf / C_SOUND) * D[0, 1]))


# the pass the tests share: CPA at 100 m in mid-transmission at 2.5 m/s, and a grid that holds it among separated decoys
TRUTH = (2.5, 100.0, 55.0)
GRID_V, GRID_D, GRID_TC = (0.0, 1.5, 2.5, 3.5), (50.0, 100.0, 200.0), (35.0, 55.0, 75.0)

# the pass of the closed loop through the pipe: the receiver's grid trajectory V = (-2, -2), p = (0, 50) -- 2.83 m/s past a
# CPA at 35.4 m, 12.5 s into the transmission --, which the pipe decodes at -20 dB in either model (profiles/moving_source.txt)
LOOP_SLM = (-2.0, -2.0, 0.0, 50.0)
LOOP_TRUTH = (float(np.sqrt(8.0)), 100.0 / float(np.sqrt(8.0)), 12.5)
LOOP_V, LOOP_D, LOOP_TC = (0.0, 2.0, LOOP_TRUTH[0], 3.6), (LOOP_TRUTH[1], 100.0, 250.0), (2.5, 12.5, 22.5)
LOOP_QF = 16
SIGMA_M20 = float(np.sqrt(7.5))    # per component at 375 S/s: a unit-amplitude signal at -20 dB in 2500 Hz
