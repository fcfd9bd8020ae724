"""How the seeds of the two closed loops of tests/test_gpu_medium.py were chosen -- on the CPU, without the transmitter.

    python tools/medium_cpu_seeds.py [--seeds 6] [--workers 8]

Impulses.  Signal: tests/golden/closed_loop_int16.npz `tx` (`VE3EMB FN25 30`).  Noise: sigma x the restated AWGN of seed s
(tests/transmit_exact.py: Philox blocks with counter word 3 = 0, Box-Muller in binary64) at -22 dB in 2500 Hz, then the
restated impulses of the same seed (tests/medium_exact.py: probability 1 / 250, 60 sigma, length 1).  Chain: the numpy
blanker of tests/blank_exact.py (blank = 24, guard = 2; or none), oracle/frontend_grc.py's float64 chain, the oracle's
FDR and schedule on the first 2 candidates, the library's host tail (Fano + unpack, CPU code).  A seed is good when the
message decodes with the blanker and not without.

Fading.  At baseband: the unit transmission (f0 = 2 Hz, the first symbol at sample 375) times the restated gain
h(k) of {"spread": 0.1, "k": 10, "seed": s, "paths": 16}, plus noise of synth.sigma_for_snr(-18) from Philox(100 + s),
through the oracle and the real Fano.  A seed is good when the message decodes."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

WANT = "VE3EMB FN25 30"
SNR_DB, RATE, AMP = -22.0, 1.0 / 250, 60.0
FADE_SNR_DB = -18.0


def decode(frame):
    import gr_uwspr_amd as G
    import oracle_py as O
    out = set()
    for c in O.FDR().transform(frame)[:2]:
        d = O.demod_candidate(c, 1500, frame)
        rec = np.zeros(1, G.native.DEMOD_DTYPE)[0]
        for k in ("f1", "drift1", "sync1", "shift1", "worth_a_try", "jig_sync", "jig_rms", "jig_shift", "symbols"):
            rec[k] = d[k]
        dec = G.decode_candidate(rec)
        if dec is not None:
            out.add(G.unpack_message(dec[0])[1])
    return out


def impulsive_audio(seed):
    import medium_exact as MX
    import transmit_exact as X
    tx = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop_int16.npz"))["tx"].astype(np.float64) / 32768.0
    sigma = np.sqrt(tx.var() * 6000.0 / (2500.0 * 10.0 ** (SNR_DB / 10.0)))
    n = np.arange(len(tx), dtype=np.int64)
    x = tx + sigma * X.gauss_ref(*X.gauss_inputs(seed, 0, n))
    imp = {"rate": RATE, "sigma": AMP * sigma, "seed": seed, "length": 1}
    ev = MX.impulse_events(imp, 0, 0, len(tx))
    x[ev] += AMP * sigma * MX.impulse_ref(*MX.impulse_inputs(imp, 0, ev, 0))
    return x.astype(np.float32), len(ev)


def impulse_cell(job):
    import blank_exact as BX
    import frontend_grc as FE
    seed, blanked = job
    x, nev = impulsive_audio(seed)
    if blanked:
        x = BX.blank(x, 24, 2)[0]
    y = FE.chain(x)
    return job, WANT in decode(np.stack([y.real, y.imag], axis=1).astype(np.float32)), nev


def fading_cell(seed):
    import gr_uwspr_amd as G
    import medium_exact as MX
    from gr_uwspr_amd import synth
    sym = G.wspr_symbols(WANT).astype(np.float64)
    ftone = np.repeat((sym - 1.5) * 375.0 / 256, 256) + 2.0
    phase = 2.0 * np.pi * np.concatenate([[0.0], np.cumsum(ftone)[:-1]]) / 375.0
    h = MX.fade_gain(MX.fade_design({"spread": 0.1, "k": 10.0, "seed": seed, "paths": 16}), np.arange(len(phase)))
    y = np.zeros(45000, np.complex128)
    y[375:375 + len(phase)] = np.exp(1j * phase) * h
    rng = np.random.Generator(np.random.Philox(100 + seed))
    fr = np.stack([y.real, y.imag], axis=1) + synth.sigma_for_snr(FADE_SNR_DB) * rng.standard_normal((45000, 2))
    return seed, WANT in decode(fr.astype(np.float32)), float(np.mean(np.abs(h) ** 2)), float(np.abs(h).min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    with ProcessPoolExecutor(a.workers) as ex:
        res = dict((job, (ok, nev)) for job, ok, nev in ex.map(impulse_cell, [(s, b) for s in range(a.seeds) for b in (False, True)]))
        fades = list(ex.map(fading_cell, range(a.seeds)))
    print("impulses: %.0f dB in 2500 Hz, probability 1/%d, %.0f sigma, blank = 24, guard = 2" % (SNR_DB, round(1 / RATE), AMP))
    for s in range(a.seeds):
        off, on = res[(s, False)][0], res[(s, True)][0]
        print("  seed %d: %d events; blank=0 %s, blank=24 %s -> %s" %
              (s, res[(s, True)][1], "decodes" if off else "lost", "decodes" if on else "lost", "good" if on and not off else "REPLACE"))
    print("fading: Rician K = 10, spread 0.1 Hz, 16 paths, %.0f dB in 2500 Hz, at baseband" % FADE_SNR_DB)
    for s, ok, p, lo in fades:
        print("  seed %d: mean |h|^2 %.3f, min |h| %.3f -> %s" % (s, p, lo, "decodes: good" if ok else "lost: REPLACE"))


if __name__ == "__main__":
    main()
