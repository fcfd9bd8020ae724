"""What the resampler ahead of K0 (K11, option "audio_rate") costs -- the figures of profiles/resample.txt.

    python tools/resample_probe.py [--minutes 60] [--reps 3] [--out profiles/resample.txt]

  kernel: K11 alone on device memory (uwspr_resample_batch with device pointers, on a torch stream, bracketed by HIP
          events): one hour of int16 audio at 48 000 and 44 100 S/s with 1, 8 and 64 interleaved channels, reported per
          channel-hour.  64 channels are timed on --minutes / 6 and scaled (an hour of them is 22 GB of input).
  pipe:   one hour of 48 kS/s int16 audio through the whole pipe (Pipe(audio_rate=48000), 5-minute pieces) beside the
          same hour at 12 kS/s through the default pipe -- the path that existed before the option, whose bytes the
          default still gives -- and the ratio of the two.
The audio is seeded white noise at -21 dBFS (no frame decodes; the rates do not depend on it)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, FL = 3375, 45000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; --minutes %g --reps %d (median of the reps after one untimed run)" %
        (torch.cuda.get_device_name(0), a.minutes, a.reps))

    # ---- K11 alone
    ctx = G.Context()
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    try:
        for rate in (48000, 44100):
            taps, L, M, T, D = G.resample_design(rate)
            for nch in (1, 8, 64):
                minutes = a.minutes / 6.0 if nch == 64 else a.minutes
                n = int(minutes * 60 * rate)
                with torch.cuda.stream(st):
                    g = torch.Generator(device="cuda:0").manual_seed(rate + nch)
                    x = torch.randint(-9000, 9000, (n, nch), dtype=torch.int16, device="cuda:0", generator=g)
                    ms = []
                    for r in range(a.reps + 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        y = ctx.resample(x, rate)
                        e1.record(st)
                        e1.synchronize()
                        if r:
                            ms.append(e0.elapsed_time(e1))
                        nout = y.shape[0]
                        del y
                ms.sort()
                t = ms[len(ms) // 2] * (a.minutes / minutes)
                gb = (n * nch * 2 + nout * nch * 4) * (a.minutes / minutes) / 1e9
                say("K11 %6d S/s int16 C=%-2d  L/M %d/%d T %3d  %8.3f ms per %g min of %d channels = %7.3f ms per channel-hour "
                    "(%.0f GB/s in + out)%s" % (rate, nch, L, M, T, t, a.minutes, nch, t / nch * 60.0 / a.minutes, gb / (t / 1e3),
                                                "  [timed on 1/6, scaled]" if nch == 64 else ""))
                del x
                torch.cuda.empty_cache()
    finally:
        ctx.close()

    # ---- the whole pipe
    def pipe_hour(rate):
        n = int(a.minutes * 60 * rate)
        x = np.clip(np.rint(np.random.default_rng(rate).standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16)
        nframes = (n * 12000 // rate // 32 - FL) // HOP + 1
        ts = []
        for r in range(a.reps + 1):
            pipe = G.Pipe(hop=HOP, batch_frames=256, audio_rate=rate)
            try:
                t0 = time.perf_counter()
                for k in range(0, n, 300 * rate):
                    pipe.push_audio(x[k: k + 300 * rate])
                pipe.flush()
                dt = time.perf_counter() - t0
                stt = pipe.stats()
            finally:
                pipe.close()
            assert abs(stt["frames"] - nframes) <= 1, (stt, nframes)
            if r:
                ts.append(dt)
        ts.sort()
        t = ts[len(ts) // 2]
        say("pipe %6d S/s int16, 5-min pieces: median %.3f s (min %.3f, max %.3f) per %g min, %d frames, %8.0f x real time" %
            (rate, t, ts[0], ts[-1], a.minutes, stt["frames"], a.minutes * 60 / t))
        return t

    t12 = pipe_hour(12000)
    t48 = pipe_hour(48000)
    say("ratio: the 48 kS/s hour takes %.2f x the 12 kS/s hour (4 x the bytes over the link, K11, then the same K0 + search)" %
        (t48 / t12))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
