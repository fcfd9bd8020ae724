"""What the noise blanker ahead of the front-end (K12, options "blank" / "blank_guard") gives and costs on the device --
the GPU figures of profiles/blanker.txt.

    python tools/blanker_probe.py [--seeds 16] [--sweep-seeds 8] [--minutes 60] [--reps 3] [--out FILE]

  rows:    the three rows of tools/blanker_cpu_table.py (same audio, same seeds) through the whole pipe
           (Pipe(max_per_frame=2), blank = 0 and 24): seeds whose records hold `VE3EMB FN25 30`.
  sweep:   tools/snr_sweep.py's Gaussian sweep (the recording + AWGN, its seeds, 4 candidates per frame) through the pipe
           with blank = 0 and 24: decodes of `VE3EMB FN42 33`, other texts, and whether the decode sets are equal.
  kernels: k12_level and k12_apply alone on device memory (uwspr_debug_blank_launch on a torch stream, bracketed by HIP
           events): one hour of 12 kS/s audio, int16 and float32, 1, 8 and 64 interleaved channels (64: timed on
           --minutes / 6 and scaled), per channel-hour.
  hour:    one hour of 12 kS/s int16 noise through the pipe as tools/audio_stream_probe.py pushes it (10-s and 5-min
           pieces, pageable), blank = 0 and 24."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOP, FL, RATE, N = 3375, 45000, 12000, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--sweep-seeds", type=int, default=8)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    import blanker_cpu_table as T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def texts(x, per, **opts):
        pipe = G.Pipe(hop=HOP, batch_frames=3, max_per_frame=per, lanes=3, **opts)
        try:
            for k in range(0, len(x), 250000):
                pipe.push_audio(x[k: k + 250000])
            pipe.flush()
            recs = pipe.collect(cap=1 << 16)
            s, z = pipe.blank_stats(1)
        finally:
            pipe.close()
        return sorted(G.unpack_message(r["message"])[1] for r in recs if r["decoded"]), int(z[0])

    say("device: %s" % torch.cuda.get_device_name(0))

    # ---- the table's rows through the pipe
    say("pipe (K12 -> K0 -> FDR + schedule -> Fano), %d seeds, blank = %d, guard = %d: seeds that decode %s" %
        (a.seeds, T.BLANK, T.GUARD, T.WANT))
    say("SNR, p, amp            | Gaussian only | + impulses | + impulses, blanked | Gaussian only, blanked | zeroed (impulses / Gaussian)")
    for snr, p, amp in T.ROWS:
        cnt = {}
        zs = {True: [], False: []}
        for s in range(a.seeds):
            for imp in (False, True):
                x, _ = T.audio(s, snr, p, amp, imp)
                for bl in (False, True):
                    t, z = texts(x, 2, blank=T.BLANK if bl else 0, blank_guard=T.GUARD)
                    cnt[(imp, bl)] = cnt.get((imp, bl), 0) + (T.WANT in t)
                    if bl:
                        zs[imp].append(z / len(x))
        say("%5.0f dB, 1/%d, %2.0f    | %13d | %10d | %19d | %22d | %.2f %% / %.3f %%" %
            (snr, round(1 / p), amp, cnt[(False, False)], cnt[(True, False)], cnt[(True, True)], cnt[(False, True)],
             100 * np.mean(zs[True]), 100 * np.mean(zs[False])))

    # ---- the Gaussian sweep of tools/snr_sweep.py
    import snr_sweep as S
    x = np.load(os.path.join(ROOT, "tests", "golden", "150613_1920_int16.npz"))["x"].astype(np.float32) / 32768.0
    wide = G.Context(options={"frontend": G.FRONTEND_COMPACT})
    clean = wide.frontend(x[None])
    cands, out = wide.pipeline_batch(clean, max_per_frame=S.PER)
    wide.close()
    f1 = [float(out[0, j]["f1"]) for j in range(min(S.PER, len(cands[0]))) if S.decode_texts(out[0, j]) == S.WANT][0]
    ps, n0 = S.estimate_native(clean[0], f1)
    say("Gaussian sweep (tools/snr_sweep.py's audio and seeds, %d per SNR, %d candidates per frame) through the pipe: frames with %s / other texts" %
        (a.sweep_seeds, S.PER, S.WANT))
    for snr in S.SNRS:
        sigma = np.sqrt(max(ps / (2500.0 * 10 ** (snr / 10.0)) - n0, 0.0) * 12000.0)
        ok, other, same, zz = [0, 0], [0, 0], 0, []
        for s in range(a.sweep_seeds):
            rng = np.random.Generator(np.random.Philox(int(1000 * -snr) + s))
            au = (x + sigma * rng.standard_normal(x.size).astype(np.float32)).astype(np.float32)   # (as snr_sweep.run stores it)
            t0, _ = texts(au, S.PER)
            t1, z = texts(au, S.PER, blank=24)
            for k, t in enumerate((t0, t1)):
                ok[k] += S.WANT in t
                other[k] += len([u for u in t if u != S.WANT])
            same += t0 == t1
            zz.append(z / len(au))
        say("SNR %5.1f dB: blank=0 %2d/%d, %d other | blank=24 %2d/%d, %d other | decode sets equal for %d of %d seeds | zeroed %.3f %%" %
            (snr, ok[0], a.sweep_seeds, other[0], ok[1], a.sweep_seeds, other[1], same, a.sweep_seeds, 100 * np.mean(zz)))

    # ---- the kernels alone
    ctx = G.Context()
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    try:
        for dtype, name in ((torch.int16, "int16"), (torch.float32, "float32")):
            for nch in (1, 8, 64):
                minutes = a.minutes / 6.0 if nch == 64 else a.minutes
                n = int(minutes * 60 * RATE) // N * N
                nb = n // N
                with torch.cuda.stream(st):
                    g = torch.Generator(device="cuda:0").manual_seed(nch)
                    xd = torch.randint(-9000, 9000, (n, nch), dtype=torch.int16, device="cuda:0", generator=g)
                    if dtype == torch.float32:
                        xd = xd.to(torch.float32) / 32768.0
                    lev = torch.zeros((nb, nch), dtype=torch.float32, device="cuda:0")
                    yd = torch.empty((n, nch), dtype=torch.float32, device="cuda:0")
                    nz = torch.empty((nb, nch), dtype=torch.int32, device="cuda:0")
                    ms = {"level": [], "apply": []}
                    for r in range(a.reps + 1):
                        for which in ("level", "apply"):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            if which == "level":
                                ctx.debug_blank_launch(xd, 0, lev, 0, 0, nb, 24, 2, None, 0, None, nch=nch)
                            else:
                                ctx.debug_blank_launch(xd, 0, lev, 0, 0, 0, 24, 2, yd, 0, nz, nch=nch)
                            e1.record(st)
                            e1.synchronize()
                            if r:
                                ms[which].append(e0.elapsed_time(e1))
                es = 2 if dtype == torch.int16 else 4
                for which, byt in (("level", es), ("apply", es + 4)):
                    v = sorted(ms[which])
                    t = v[len(v) // 2]
                    say("k12_%-5s %-7s C=%-2d %8.3f ms per %g min of %d channels = %7.3f ms per channel-hour (%.0f GB/s)%s" %
                        (which, name, nch, t, minutes, nch, t / nch * 60.0 / minutes, n * nch * byt / 1e9 / (t / 1e3),
                         "  [timed on 1/6]" if nch == 64 else ""))
                del xd, yd, lev, nz
                torch.cuda.empty_cache()
    finally:
        ctx.close()

    # ---- one hour through the pipe
    n = int(a.minutes * 60 * RATE)
    xs = np.clip(np.rint(np.random.default_rng(0).standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16)
    for label, piece in (("pipe push_audio 10 s, pageable", 10 * RATE), ("pipe push_audio 5 min, pageable", 300 * RATE)):
        for blank in (0, 24):
            ts = []
            for r in range(a.reps + 1):
                pipe = G.Pipe(hop=HOP, batch_frames=256, blank=blank)
                try:
                    t0 = time.perf_counter()
                    for k in range(0, n, piece):
                        pipe.push_audio(xs[k: k + piece])
                    pipe.flush()
                    dt = time.perf_counter() - t0
                    frames = pipe.stats()["frames"]
                finally:
                    pipe.close()
                if r:
                    ts.append(dt)
            ts.sort()
            t = ts[len(ts) // 2]
            say("%-32s blank=%-2d median %.3f s (min %.3f, max %.3f)  %d frames  %8.0f x real time" %
                (label, blank, t, ts[0], ts[-1], frames, a.minutes * 60 / t))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
