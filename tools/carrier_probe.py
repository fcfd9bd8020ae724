#!/usr/bin/env python3
"""What K0's carrier form costs (profiles/carriers.txt).  One MI355X.
  * one launch over a channel-hour of 12 kS/s int16 audio, by HIP events (median of --reps after one untimed run): the
    form there was at 1500 Hz against the carrier form with (nch, NC) = (1, 1) at 2203 Hz, then NC = 2, 8 and 64
    carriers on one channel (64: a sixth of the hour, scaled);
  * an hour of int16 noise through a pipe with 1 and with 8 carriers, 5-minute pushes, wall time from the first push
    to flush.
usage: tools/carrier_probe.py [--minutes 60] [--reps 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gr_uwspr_amd as G  # noqa: E402

J = 216


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("device: %s" % torch.cuda.get_device_name(0))
    n = a.minutes * 60 * 12000
    x = np.clip(np.rint(np.random.default_rng(1).standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16)
    pool = [2203, 497, 1501, 1100, 2600, 3001, 3400, 3800] + [600 + 37 * i for i in range(56)]

    ctx = G.Context()
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    try:
        for label, fc, NC in (("form there was, 1500 Hz", 1500, 0), ("carrier form, 1500 Hz (identity)", 1500, 1),
                              ("carrier form, 2203 Hz", 2203, 1), ("carrier form", None, 2), ("carrier form", None, 8),
                              ("carrier form", None, 64)):
            part = 6 if NC == 64 else 1
            nin = n // part
            nout = nin // 32
            xd = torch.from_numpy(x[:nin]).to("cuda:0")
            out = torch.empty((max(NC, 1) * nout, 2), dtype=torch.float32, device="cuda:0")
            car = [fc] if NC == 1 else pool[:NC]
            ms = []
            for r in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                if NC == 0:
                    ctx.debug_frontend_launch(xd, 0, out, 0, nout=nout, nin=nin)
                else:
                    ctx.debug_frontend_carrier_launch(xd, 0, out, 0, car, nch=1, plane=nout, nout=nout, nin=nin)
                e1.record(st)
                e1.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            ms.sort()
            t = ms[len(ms) // 2] * part
            npl = max(NC, 1)
            say("%-34s NC=%-2d %8.3f ms per channel-hour, %7.3f ms per plane-hour%s" %
                (label, NC, t * 60 / a.minutes, t * 60 / a.minutes / npl, "  [timed on 1/6]" if part > 1 else ""))
            del xd, out
    finally:
        ctx.close()

    frames = (n // 32 - 45000) // 3375 + 1
    for carriers in (None, [1500], [2203], pool[:8]):
        ts = []
        for r in range(a.reps + 1):
            pipe = G.Pipe(carriers=carriers)
            try:
                t0 = time.perf_counter()
                for k in range(0, n, 5 * 60 * 12000):
                    pipe.push_audio(x[k: k + 5 * 60 * 12000])
                pipe.flush()
                dt = time.perf_counter() - t0
                nrec = len(pipe.collect(cap=1 << 20))
            finally:
                pipe.close()
            if r:
                ts.append(dt)
        ts.sort()
        t = ts[len(ts) // 2]
        say("pipe push_audio 5 min, carriers %-28s median %.3f s (min %.3f, max %.3f)  %d frames x %d planes, %d records" %
            ("default" if carriers is None else str(carriers), t, ts[0], ts[-1], frames, len(carriers or [0]), nrec))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
