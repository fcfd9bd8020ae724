"""The defaults "deep_min" and "deep_gap" (UWSPR_DEEP_MIN_DEFAULT, UWSPR_DEEP_GAP_DEFAULT), measured on the CPU against
the restatement of the definition (tests/deep_exact.py: the kernel equals it byte for byte), never against the kernel.

Frames of tests/test_gpu_osd_pipe.py's text_frame model carrying random 50-bit messages go through the CPU oracle's FDR +
refinement schedule; the strongest candidate's gated tries (cc:470) go through the host Fano decoder.  A frame on which
every gated try times out is one sample: its vector is the pipe's item (the gated try with the largest jig_sync, the first
on ties).  The vector is scored against a list of 65536 random messages that does NOT hold the transmitted one (the
largest list is the worst case for both numbers): what matters is the largest sbest and the largest sbest - snext over
all samples.  Each default is that maximum plus a quarter (a hedge for the tail beyond the sample, not a derived bound).
With the transmitted message added to the list -- 65536, 4096 and 16 messages, the first of the same list -- the share of
the samples accepted at those defaults is printed per level.

python tools/deep_gap.py [--frames 1500] [--snr -30 -31 -32] [--procs 8]"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

MINSYNC2, MINRMS = np.float32(0.12), np.float32(52.0 * (50 / 64.0))
SIZES = (16, 4096, 65536)
_SIGNS = None


def list_signs(G):
    """the list's +-1 table [65536, 162] (int64), once per worker"""
    global _SIGNS
    if _SIGNS is None:
        import deep_exact as X
        msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE90000)), SIZES[-1])
        _SIGNS = (msgs, 2 * X.code_table(G, msgs) - 1)
    return _SIGNS


def frames_job(args):
    import gr_uwspr_amd as G
    import oracle_py as O
    import deep_exact as X
    from test_gpu_osd_pipe import text_frame
    first, count, snr = args
    f = O.FDR()
    msgs, signs = list_signs(G)
    out = []   # (seed, kind, S of the transmitted message, then per list size: sbest, snext); kind 0: no gated try, 1: Fano decoded, 2: timed out
    for seed in range(first, first + count):
        msg = X.random_messages(np.random.Generator(np.random.Philox(0xDEE95EED + seed)), 1)[0]
        if (msgs == msg).all(axis=1).any():
            continue   # (the list must not hold the transmitted message)
        frame = text_frame(G, msg, seed, snr)
        cands = f.transform(frame)
        row = [seed, 0, 0] + [0, 0] * len(SIZES)
        if len(cands):
            d = O.demod_candidate(cands[0], 1500, frame)
            g = [t for t in range(17) if d["jig_sync"][t] > MINSYNC2 and d["jig_rms"][t] > MINRMS] if d["worth_a_try"] else []
            if g:
                if any(G.fano_decode(G.deinterleave(d["symbols"][t]))[0] == 0 for t in g):
                    row[1] = 1
                else:
                    t = max(g, key=lambda k: (d["jig_sync"][k], -k))
                    s = d["symbols"][t].astype(np.int64) - 128
                    S = signs @ s
                    row[1] = 2
                    row[2] = int((2 * X.code_table(G, msg[None])[0] - 1) @ s)
                    for q, M in enumerate(SIZES):
                        top = np.sort(S[:M])[-2:]
                        row[3 + 2 * q], row[4 + 2 * q] = int(top[1]), int(top[0])
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--snr", type=float, nargs="+", default=[-30.0, -31.0, -32.0])
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=10)
    a = ap.parse_args()
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()   # (built before the workers start; they are spawned, not forked: each loads the library itself)
    per = {}
    with multiprocessing.get_context("spawn").Pool(a.procs) as pool:
        for snr in a.snr:
            jobs = [(k, min(a.chunk, a.frames - k), snr) for k in range(0, a.frames, a.chunk)]
            rows = np.array([r for out in pool.map(frames_job, jobs) for r in out], np.int64).reshape(-1, 3 + 2 * len(SIZES))
            per[snr] = rows
            t = rows[rows[:, 1] == 2]
            print("snr %g dB: %d frames, %d with a gated try, Fano decoded %d, timed out %d" %
                  (snr, len(rows), (rows[:, 1] > 0).sum(), (rows[:, 1] == 1).sum(), len(t)), flush=True)
            if len(t):
                q = np.percentile(t[:, 2], [5, 50])
                print("  S of the transmitted message: 5%% %d, median %d" % (q[0], q[1]))
                for k, M in enumerate(SIZES):
                    sb, gp = t[:, 3 + 2 * k], t[:, 3 + 2 * k] - t[:, 4 + 2 * k]
                    print("  list of %5d without it: sbest median %d, max %d; sbest - snext median %d, max %d" %
                          (M, np.median(sb), sb.max(), np.median(gp), gp.max()), flush=True)
    allt = np.concatenate([r[r[:, 1] == 2] for r in per.values()])
    if not len(allt):
        return
    k = len(SIZES) - 1
    smax, gmax = int(allt[:, 3 + 2 * k].max()), int((allt[:, 3 + 2 * k] - allt[:, 4 + 2 * k]).max())
    dmin, dgap = smax + (smax + 3) // 4, gmax + (gmax + 3) // 4
    print("%d time-outs in all; list of 65536 without the transmitted message: largest sbest %d, largest sbest - snext %d"
          % (len(allt), smax, gmax))
    print("defaults (each maximum plus a quarter): deep_min %d, deep_gap %d" % (dmin, dgap))
    for snr, rows in per.items():
        t = rows[rows[:, 1] == 2]
        for k, M in enumerate(SIZES):
            # the transmitted message joins the list (behind the others: it loses ties)
            st, sb, sn = t[:, 2], t[:, 3 + 2 * k], t[:, 4 + 2 * k]
            ok = (st > sb) & (st >= dmin) & (st - sb >= dgap)
            wrong = (st <= sb) & (sb >= dmin) & (sb - np.maximum(sn, st) >= dgap)
            print("snr %g dB, list of %5d with it: accepted %d of %d time-outs (%.0f %%), another message accepted %d"
                  % (snr, M, ok.sum(), len(t), 100.0 * ok.mean() if len(t) else 0.0, wrong.sum()))


if __name__ == "__main__":
    main()
