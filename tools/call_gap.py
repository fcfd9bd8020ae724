"""The defaults "call_min" and "call_gap" (UWSPR_CALL_MIN_DEFAULT, UWSPR_CALL_GAP_DEFAULT), measured on the CPU against
the restatement of the definition (tests/call_exact.py: the kernel equals it byte for byte), never against the kernel.

tools/deep_gap.py's frame model and levels, with random type-1 messages (a random callsign, locator and power): frames of
tests/test_gpu_osd_pipe.py's text_frame go through the CPU oracle's FDR + refinement schedule, the strongest candidate's
gated tries (cc:470) through the host Fano decoder.  A frame on which every gated try times out is one sample: its vector
is the pipe's item (the gated try with the largest jig_sync, the first on ties).  The vector is scored against the worst
case of a call set -- 64 callsigns, all 32400 locators, all 19 powers, 39.4 M hypotheses -- that does NOT hold the
transmitted callsign: what matters is the largest sbest and the largest sbest - snext over all samples; each default is
that maximum plus a quarter (a hedge for the tail beyond the sample, not a derived bound).  The same maxima are printed
for the first 16 and the first 1 of those callsigns and for the 64 with the locators of one field (100 locators: the field
of the transmitted locator).  With the transmitted callsign in the set -- beside the first 63, 15 and 0 of the others --
the share of the samples that the defaults accept as the transmitted message is printed per level, and how many other
messages they accepted; then the same for thresholds a narrower set would allow -- the maxima of that narrower set plus a
quarter: 16 callsigns, one callsign, and 64 callsigns within one field.

The scores are float32 matrix products, exact because every sum is an integer below 2^24.

python tools/call_gap.py [--frames 1600] [--snr -30 -31 -32] [--procs 8]"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

MINSYNC2, MINRMS = np.float32(0.12), np.float32(52.0 * (50 / 64.0))
NWRONG, SIZES = 64, (1, 16, 64)
GBLOCK = 3240
_TAB = None


def tables(G):
    """once per worker: the 64 other callsigns, their signs [64, 162], the powers' [19, 162], the locators' [32400, 162]
    (float32)"""
    global _TAB
    if _TAB is None:
        import call_exact as CX
        calls = CX.random_calls(np.random.Generator(np.random.Philox(0xCA1150000)), NWRONG)
        _TAB = (calls, (2 * CX.call_bits(G, calls) - 1).astype(np.float32), (2 * CX.power_bits(G) - 1).astype(np.float32),
                np.ascontiguousarray(2 * CX.grid_bits(G).astype(np.float32) - 1))
    return _TAB


def top2_rows(S):
    """S [g, c]: per column the largest and second largest over the rows (equal when the maximum appears twice)"""
    k = S.argmax(axis=0)
    cols = np.arange(S.shape[1])
    t1 = S[k, cols].copy()
    S[k, cols] = -np.inf
    return t1, S.max(axis=0)


def merge2(t1, t2, axis):
    """the two largest of the union of (t1, t2) pairs along an axis"""
    both = np.sort(np.concatenate([t1, t2], axis=axis), axis=axis)
    return np.take(both, -1, axis=axis), np.take(both, -2, axis=axis)


def score_item(G, s, true_call, g_true, d_true):
    """-> st, top [65, 2] (per callsign the two largest scores over all locators and powers; row 64 = the transmitted callsign
    without the transmitted message), field [65, 2] (the same over the 100 locators of the transmitted locator's field)"""
    import call_exact as CX
    calls, sa, sd, sg = tables(G)
    fl = CX.bitmap_list(CX.grids_bitmap([CX.ngrid_grid(g_true)[:2]]))
    sa = np.concatenate([sa, (2 * CX.call_bits(G, [true_call]) - 1).astype(np.float32)])
    x = (sa[:, None, :] * sd[None, :, :] * s.astype(np.float32)[None, None, :]).reshape(-1, CX.NSYM)   # [65 * 19, 162]
    col_true = NWRONG * CX.NPOW + d_true
    t1s, t2s, st = [], [], None
    for g0 in range(0, CX.NGRID, GBLOCK):
        S = sg[g0:g0 + GBLOCK] @ x.T
        if g0 <= g_true < g0 + GBLOCK:
            st = int(S[g_true - g0, col_true])
            S[g_true - g0, col_true] = -np.inf
        a, b = top2_rows(S)
        t1s.append(a); t2s.append(b)
    t1, t2 = merge2(np.stack(t1s), np.stack(t2s), 0)                                  # [65 * 19]
    t1, t2 = merge2(t1.reshape(-1, CX.NPOW), t2.reshape(-1, CX.NPOW), 1)              # [65]
    F = sg[fl] @ x.T
    F[int(np.searchsorted(fl, g_true)), col_true] = -np.inf
    f1, f2 = top2_rows(F)
    f1, f2 = merge2(f1.reshape(-1, CX.NPOW), f2.reshape(-1, CX.NPOW), 1)
    return st, np.stack([t1, t2], 1).astype(np.int64), np.stack([f1, f2], 1).astype(np.int64)


def frames_job(args):
    import gr_uwspr_amd as G
    import oracle_py as O
    import call_exact as CX
    from test_gpu_osd_pipe import text_frame
    first, count, snr = args
    f = O.FDR()
    calls = tables(G)[0]
    out = []   # (seed, kind, st, top [65, 2], field [65, 2]) flattened; kind 0: no gated try, 1: Fano decoded, 2: timed out
    width = 3 + 4 * (NWRONG + 1)
    for seed in range(first, first + count):
        rng = np.random.Generator(np.random.Philox(0xCA115EED + seed))
        call = CX.random_calls(rng, 1)[0]
        g, d = int(rng.integers(CX.NGRID)), int(rng.integers(CX.NPOW))
        if call in calls:
            continue   # (the set must not hold the transmitted callsign)
        frame = text_frame(G, CX.message(G, call, g, CX.P19[d]), seed, snr)
        cands = f.transform(frame)
        row = np.zeros(width, np.int64)
        row[0] = seed
        if len(cands):
            dm = O.demod_candidate(cands[0], 1500, frame)
            gt = [t for t in range(17) if dm["jig_sync"][t] > MINSYNC2 and dm["jig_rms"][t] > MINRMS] if dm["worth_a_try"] else []
            if gt:
                if any(G.fano_decode(G.deinterleave(dm["symbols"][t]))[0] == 0 for t in gt):
                    row[1] = 1
                else:
                    t = max(gt, key=lambda k: (dm["jig_sync"][k], -k))
                    st, top, fld = score_item(G, dm["symbols"][t].astype(np.int64) - 128, call, g, d)
                    row[1], row[2] = 2, st
                    row[3:3 + 2 * (NWRONG + 1)] = top.ravel()
                    row[3 + 2 * (NWRONG + 1):] = fld.ravel()
        out.append(row)
    return out


def set_top2(pairs):
    """pairs [n, k, 2] -> the two largest of each sample's union: [n], [n]"""
    flat = np.sort(pairs.reshape(len(pairs), -1), axis=1)
    return flat[:, -1], flat[:, -2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1600)
    ap.add_argument("--snr", type=float, nargs="+", default=[-30.0, -31.0, -32.0])
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=10)
    a = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"   # (the workers are the parallelism)
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()   # (built before the workers start; they are spawned, not forked: each loads the library itself)
    per = {}
    nt = 2 * (NWRONG + 1)
    with multiprocessing.get_context("spawn").Pool(a.procs) as pool:
        for snr in a.snr:
            jobs = [(k, min(a.chunk, a.frames - k), snr) for k in range(0, a.frames, a.chunk)]
            rows = np.array([r for out in pool.map(frames_job, jobs) for r in out], np.int64).reshape(-1, 3 + 2 * nt)
            per[snr] = rows
            t = rows[rows[:, 1] == 2]
            print("snr %g dB: %d frames, %d with a gated try, Fano decoded %d, timed out %d" %
                  (snr, len(rows), (rows[:, 1] > 0).sum(), (rows[:, 1] == 1).sum(), len(t)), flush=True)
            if len(t):
                q = np.percentile(t[:, 2], [5, 50])
                print("  S of the transmitted message: 5%% %d, median %d" % (q[0], q[1]))
                top = t[:, 3:3 + nt].reshape(len(t), NWRONG + 1, 2)
                for A in SIZES:
                    sb, sn = set_top2(top[:, :A])
                    print("  %2d callsigns without it, all locators and powers: sbest median %d, max %d; sbest - snext median %d, max %d"
                          % (A, np.median(sb), sb.max(), np.median(sb - sn), (sb - sn).max()), flush=True)
                sb, sn = set_top2(t[:, 3 + nt:].reshape(len(t), NWRONG + 1, 2)[:, :NWRONG])
                print("  64 callsigns without it, the 100 locators of one field: sbest median %d, max %d; sbest - snext median %d, max %d"
                      % (np.median(sb), sb.max(), np.median(sb - sn), (sb - sn).max()), flush=True)
                own = top[:, NWRONG, 0]
                print("  the transmitted callsign's other locators and powers: largest score median %d, max %d; the transmitted "
                      "message's lead over them median %d, min %d" % (np.median(own), own.max(), np.median(t[:, 2] - own), (t[:, 2] - own).min()))
    allt = np.concatenate([r[r[:, 1] == 2] for r in per.values()])
    if not len(allt):
        return
    sb, sn = set_top2(allt[:, 3:3 + nt].reshape(len(allt), NWRONG + 1, 2)[:, :NWRONG])
    smax, gmax = int(sb.max()), int((sb - sn).max())
    cmin, cgap = smax + (smax + 3) // 4, gmax + (gmax + 3) // 4
    print("%d time-outs in all; 64 callsigns without the transmitted one: largest sbest %d, largest sbest - snext %d" % (len(allt), smax, gmax))
    print("defaults (each maximum plus a quarter): call_min %d, call_gap %d" % (cmin, cgap))
    def report(label, cmin, cgap, pick):
        for snr, rows in per.items():
            t = rows[rows[:, 1] == 2]
            # the transmitted callsign joins the others of the set; everything but the transmitted message is "the others"
            o1, o2 = set_top2(pick(t))
            st = t[:, 2]
            ok = (st > o1) & (st >= cmin) & (st - o1 >= cgap)
            wrong = (st <= o1) & (o1 >= cmin) & (o1 - np.maximum(o2, st) >= cgap)
            print("snr %g dB, %s with it, call_min %d, call_gap %d: accepted %d of %d time-outs (%.0f %%), another message accepted %d; "
                  "Fano alone %d of %d frames" % (snr, label, cmin, cgap, ok.sum(), len(t), 100.0 * ok.mean() if len(t) else 0.0,
                                                  wrong.sum(), (rows[:, 1] == 1).sum(), len(rows)))

    def tops(t, lo, A):
        top = t[:, lo:lo + nt].reshape(len(t), NWRONG + 1, 2)
        return np.concatenate([top[:, :A - 1], top[:, NWRONG:]], axis=1)

    print("at the defaults:")
    for A in SIZES:
        report("%2d callsigns" % A, cmin, cgap, lambda t, A=A: tops(t, 3, A))
    print("at the thresholds a narrower set would allow (its own maxima plus a quarter):")
    for A in SIZES[:-1]:
        sb, sn = set_top2(allt[:, 3:3 + nt].reshape(len(allt), NWRONG + 1, 2)[:, :A])
        smax, gmax = int(sb.max()), int((sb - sn).max())
        report("%2d callsigns" % A, smax + (smax + 3) // 4, gmax + (gmax + 3) // 4, lambda t, A=A: tops(t, 3, A))
    sb, sn = set_top2(allt[:, 3 + nt:].reshape(len(allt), NWRONG + 1, 2)[:, :NWRONG])
    smax, gmax = int(sb.max()), int((sb - sn).max())
    report("64 callsigns, one field", smax + (smax + 3) // 4, gmax + (gmax + 3) // 4, lambda t: tops(t, 3 + nt, NWRONG))


if __name__ == "__main__":
    main()
