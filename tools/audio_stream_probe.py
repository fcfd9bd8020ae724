"""One hour of 12 kS/s int16 audio through the audio stream -- the rate of profiles/audio_stream.txt.

    python tools/audio_stream_probe.py [--minutes 60] [--reps 3]

  pipe:   uwspr_pipe_push_audio in 10-s and 5-min pieces, then uwspr_pipe_flush: audio -> staging -> K0 on the copy stream ->
          ring -> FDR + schedule + Fano, every frame decoded.  From pageable numpy memory and from page-locked memory
          (uwspr_host_alloc).
  ingest: uwspr_stream_push_audio in 1-min and 10-min pieces with the frames taken as views (no search): the upload and K0 alone.
          Pageable (staged), page-locked (one DMA per piece, the call waits for it) and page-locked asynchronous.
Each push runs K0 once per 4 Mi samples it brings, so short pushes are launch-bound.  Frames are 2-minute frames
every 9 s (hop 3375 at 375 S/s); "x real time" = audio seconds per wall-clock second.
The audio is seeded white noise at -21 dBFS (the rate does not depend on it: no frame decodes, few candidates)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, FL, RATE = 3375, 45000, 12000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    n = int(a.minutes * 60 * RATE)
    x = np.clip(np.rint(np.random.default_rng(0).standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16)
    buf = G.host_alloc(x.nbytes)
    pinned = np.frombuffer(buf, np.int16)
    pinned[:] = x
    nframes = (n // 32 - FL) // HOP + 1
    secs = n / RATE
    print("audio: %.0f s = %d int16 samples (%.1f MB), %d frames of %d samples every %d" %
          (secs, n, x.nbytes / 1e6, nframes, FL, HOP))
    print("device: %s" % torch.cuda.get_device_name(0))

    def report(name, ts):
        ts = sorted(ts)
        t = ts[len(ts) // 2]
        print("%-34s median %.3f s (min %.3f, max %.3f)  %8.0f frames/s  %8.0f x real time" %
              (name, t, ts[0], ts[-1], nframes / t, secs / t))

    # the pipe, end to end
    for label, src, piece in (("pipe push_audio 10 s, pageable", x, 10 * RATE),
                              ("pipe push_audio 10 s, page-locked", pinned, 10 * RATE),
                              ("pipe push_audio 5 min, pageable", x, 300 * RATE),
                              ("pipe push_audio 5 min, page-locked", pinned, 300 * RATE)):
        ts = []
        for r in range(a.reps + 1):
            pipe = G.Pipe(hop=HOP, batch_frames=256)
            try:
                t0 = time.perf_counter()
                for k in range(0, n, piece):
                    pipe.push_audio(src[k: k + piece])
                pipe.flush()
                dt = time.perf_counter() - t0
                recs = pipe.collect(cap=1 << 20)
                st = pipe.stats()
            finally:
                pipe.close()
            assert st["frames"] == nframes, st
            if r:
                ts.append(dt)     # (the first run pays the allocations)
        report(label, ts)
        print("    %d records, %d decoded" % (len(recs), int(recs["decoded"].sum())))

    # ingest alone: upload + K0 into the ring, frames taken as views
    for label, src, where, piece in (("ingest 1 min, pageable", x, "host", 60 * RATE),
                                     ("ingest 1 min, page-locked", pinned, "host", 60 * RATE),
                                     ("ingest 1 min, page-locked async", pinned, "async", 60 * RATE),
                                     ("ingest 10 min, pageable", x, "host", 600 * RATE),
                                     ("ingest 10 min, page-locked", pinned, "host", 600 * RATE),
                                     ("ingest 10 min, page-locked async", pinned, "async", 600 * RATE)):
        ts = []
        for r in range(a.reps + 1):
            ctx = G.Context()
            try:
                ctx.stream_open(HOP, 256)
                got = 0
                t0 = time.perf_counter()
                for k in range(0, n, piece):
                    nr = ctx.stream_push_audio(src[k: k + piece], where=where)
                    if nr:
                        ctx.stream_take_view(nr)
                        got += nr
                ctx.stream_wait_uploads()
                nr = ctx.stream_push_audio(np.zeros(0, np.int16))
                if nr:
                    ctx.stream_take_view(nr)
                    got += nr
                ctx.synchronize()
                dt = time.perf_counter() - t0
            finally:
                ctx.close()
            assert got == nframes, (got, nframes)
            if r:
                ts.append(dt)
        report(label, ts)
    G.host_free(buf)


if __name__ == "__main__":
    main()
