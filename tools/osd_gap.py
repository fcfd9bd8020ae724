"""The default "osd_gap" (UWSPR_OSD_GAP_DEFAULT), measured on the CPU against the restatement of the definition
(tests/test_gpu_osd.py: the kernel equals it byte for byte), never against the kernel:

  noise   signal-free frames (complex white noise) through the CPU oracle's FDR + refinement schedule; every gated try
          (cc:470) of every record that is worth a try goes through restated order-2 OSD.  What matters is the largest
          dnext - dmin among the vectors whose bytes uwspr_unpack_message accepts: a gap above it would have refused every
          false decode of the sample.  The default is that maximum plus a quarter (a hedge for the tail beyond the
          sample, not a derived bound).
  signal  synth frames with packable messages at --snr: the records Fano times out on whose restated order-2 message is
          the transmitted one -- the share of them whose gap survives the default.

python tools/osd_gap.py noise --records 20000 [--procs 8]
python tools/osd_gap.py signal --frames 400 --snr -29 --gap N"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

MINSYNC2, MINRMS = np.float32(0.12), np.float32(52.0 * (50 / 64.0))


def gated(d):
    return [t for t in range(17) if d["jig_sync"][t] > MINSYNC2 and d["jig_rms"][t] > MINRMS]


def noise_frames(args):
    import gr_uwspr_amd as G
    import oracle_py as O
    from test_gpu_osd import osd_restate
    first, count, per = args
    f = O.FDR()
    out = []   # (frame, cand, try, dmin, dnext, unpacks)
    nrec = 0
    for b in range(first, first + count):
        rng = np.random.Generator(np.random.Philox(0x05D0000 + b))
        frame = rng.standard_normal((45000, 2)).astype(np.float32)
        for j, c in enumerate(f.transform(frame)[:per]):
            d = O.demod_candidate(c, 1500, frame)
            nrec += 1
            if not d["worth_a_try"]:
                continue
            for t in gated(d):
                r = osd_restate(d["symbols"][t], 2)
                out.append((b, j, t, r[0], r[1], int(G.unpack_message(r[4])[0] == 0)))
    return nrec, out


def signal_frames(args):
    import gr_uwspr_amd as G
    import oracle_py as O
    from test_gpu_osd import osd_restate
    first, count, snr = args
    f = O.FDR()
    out = []   # (frame, fano decoded, osd true, gap)
    for b in range(first, first + count):
        frames, meta = G.synth.make_frames(1, seed=0x05D5EED, snr_db=snr, first=b, return_meta=True)
        bits = np.zeros(56, np.uint8)
        bits[:50] = meta[0]["bits"]
        want = np.packbits(bits).view(np.int8).tobytes()
        cands = f.transform(frames[0])
        if not len(cands):
            continue
        d = O.demod_candidate(cands[0], 1500, frames[0])
        if not d["worth_a_try"]:
            continue
        g = gated(d)
        if not g:
            continue
        if any(G.fano_decode(G.deinterleave(d["symbols"][t]))[0] == 0 for t in g):
            out.append((b, 1, 0, 0))
            continue
        t = max(g, key=lambda k: (d["jig_sync"][k], -k))   # the pipe's item: the gated try with the largest jig_sync, the first on ties
        r = osd_restate(d["symbols"][t], 2)
        out.append((b, 0, int(r[4].tobytes() == want), r[1] - r[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("noise", "signal"))
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--per", type=int, default=200, help="candidates refined per frame")
    ap.add_argument("--snr", type=float, default=-29.0)
    ap.add_argument("--gap", type=int, default=0)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=8)
    a = ap.parse_args()
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()   # (built before the workers start; they are spawned, not forked: each loads the library itself)
    with multiprocessing.get_context("spawn").Pool(a.procs) as pool:
        if a.what == "noise":
            nrec, rows, first = 0, [], 0
            while nrec < a.records:
                jobs = [(first + k * a.chunk, a.chunk, a.per) for k in range(a.procs)]
                first += a.procs * a.chunk
                for n, out in pool.map(noise_frames, jobs):
                    nrec += n
                    rows += out
                print("frames %d records %d vectors %d" % (first, nrec, len(rows)), file=sys.stderr, flush=True)
            rows = np.array(rows, np.int64).reshape(-1, 6)
            gap = rows[:, 4] - rows[:, 3]
            ok = rows[:, 5] == 1
            print("signal-free frames %d, records %d, gated tries (vectors) %d, of which unpack %d" % (first, nrec, len(rows), ok.sum()))
            for name, g in (("all vectors", gap), ("vectors that unpack", gap[ok])):
                if len(g):
                    q = np.percentile(g, [50, 90, 99, 99.9, 100])
                    print("dnext - dmin, %s: median %d, 90%% %d, 99%% %d, 99.9%% %d, max %d" % ((name,) + tuple(int(v) for v in q)))
            if ok.any():
                m = int(gap[ok].max())
                print("largest gap among vectors that unpack: %d; plus a quarter: %d" % (m, m + (m + 3) // 4))
        else:
            jobs = [(k, a.chunk, a.snr) for k in range(0, a.frames, a.chunk)]
            rows = np.array([r for out in pool.map(signal_frames, jobs) for r in out], np.int64).reshape(-1, 4)
            fano = rows[:, 1] == 1
            true = (rows[:, 1] == 0) & (rows[:, 2] == 1)
            wrong = (rows[:, 1] == 0) & (rows[:, 2] == 0)
            print("snr %g dB: %d frames with a gated try; Fano decoded %d; timed out %d, of which restated order 2 gives the "
                  "transmitted message for %d" % (a.snr, len(rows), fano.sum(), (~fano).sum(), true.sum()))
            if true.any():
                g = rows[true, 3]
                print("gap of those true messages: min %d, median %d, max %d; >= %d for %d of %d (%.0f %%)"
                      % (g.min(), np.median(g), g.max(), a.gap, (g >= a.gap).sum(), len(g), 100.0 * (g >= a.gap).mean()))
            if wrong.any():
                g = rows[wrong, 3]
                print("gap of the wrong ones: median %d, max %d; >= %d for %d of %d" % (np.median(g), g.max(), a.gap, (g >= a.gap).sum(), len(g)))


if __name__ == "__main__":
    main()
