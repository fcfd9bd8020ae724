"""The CPU table of profiles/blanker.txt: what impulsive noise does to the receiver, and what a blanker ahead of the
front-end gives back -- without a GPU.

    python tools/blanker_cpu_table.py [--seeds 16] [--workers 8]

Signal: tests/golden/closed_loop_int16.npz `tx` (the closed-loop demo's transmission, `VE3EMB FN25 30`).  Noise: sigma
N(0, 1) at the row's SNR in 2500 Hz (sigma^2 = var(tx) 6000 / (2500 10^(SNR/10))), then impulses: a sample gets one with
probability p, normally distributed with amp sigma.  The three draws come in that order from Philox(1000 + seed).
Chain: the numpy blanker of tests/blank_exact.py (blank = 24, guard = 2; or none), oracle/frontend_grc.py's float64
chain, the oracle's FDR and schedule on the first 2 candidates, the library's host tail (Fano + unpack, CPU code).
A cell is the number of seeds whose decode set holds the message."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

WANT = "VE3EMB FN25 30"
ROWS = ((-22.0, 1.0 / 250, 60.0), (-26.0, 1.0 / 250, 60.0), (-24.0, 1.0 / 500, 40.0))
BLANK, GUARD = 24, 2


def audio(seed, snr_db, p, amp, impulses):
    tx = np.load(os.path.join(ROOT, "tests", "golden", "closed_loop_int16.npz"))["tx"].astype(np.float64) / 32768.0
    sigma = np.sqrt(tx.var() * 6000.0 / (2500.0 * 10.0 ** (snr_db / 10.0)))
    r = np.random.Generator(np.random.Philox(1000 + seed))
    gauss = r.standard_normal(len(tx))
    where = r.random(len(tx)) < p
    imp = r.standard_normal(len(tx))
    x = tx + sigma * gauss
    if impulses:
        x = x + np.where(where, amp * sigma * imp, 0.0)
    return x.astype(np.float32), sigma


def decode(x):
    import gr_uwspr_amd as G
    import oracle_py as O
    import frontend_grc as FE
    y = FE.chain(x)
    frame = np.stack([y.real, y.imag], axis=1).astype(np.float32)
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


def cell(job):
    import blank_exact as BX
    row, seed, impulses, blanked = job
    x, sigma = audio(seed, *ROWS[row], impulses)
    zeroed = 0
    if blanked:
        x, _, nz = BX.blank(x, BLANK, GUARD)
        zeroed = int(nz.sum())
    power = float(np.mean((x.astype(np.float64) - audio(seed, *ROWS[row], False)[0]) ** 2)) if impulses and not blanked else 0.0
    return job, WANT in decode(x), zeroed, power / (sigma * sigma) if power else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    jobs = [(row, s, imp, bl) for row in range(len(ROWS)) for s in range(a.seeds) for imp in (False, True) for bl in (False, True)]
    with ProcessPoolExecutor(a.workers) as ex:
        res = list(ex.map(cell, jobs))
    n = 1440000
    print("CPU chain, %d seeds, blank = %d, guard = %d (tools/blanker_cpu_table.py)" % (a.seeds, BLANK, GUARD))
    print("SNR, p, amp            | Gaussian only | + impulses | + impulses, blanked | Gaussian only, blanked | impulses add | zeroed (impulses / Gaussian)")
    for row, (snr, p, amp) in enumerate(ROWS):
        def count(imp, bl):
            return sum(ok for (r, s, i, b), ok, z, pw in res if r == row and i == imp and b == bl)
        zi = np.mean([z for (r, s, i, b), ok, z, pw in res if r == row and i and b]) / n
        zg = np.mean([z for (r, s, i, b), ok, z, pw in res if r == row and not i and b]) / n
        add = np.mean([pw for (r, s, i, b), ok, z, pw in res if r == row and i and not b])
        print("%5.0f dB, 1/%d, %2.0f    | %13d | %10d | %19d | %22d | %9.1f dB | %.2f %% / %.3f %%" %
              (snr, round(1 / p), amp, count(False, False), count(True, False), count(True, True), count(False, True),
               10 * np.log10(1.0 + add), 100 * zi, 100 * zg))


if __name__ == "__main__":
    main()
