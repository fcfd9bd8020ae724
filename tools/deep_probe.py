#!/usr/bin/env python3
"""K13 (the list search) on the GPU:
  * the time of one uwspr_deep_batch call's two launches (HIP events around them: uwspr_debug_deep_time) for --items
    vectors against lists of 16, 4096 and 65536 random messages;
  * pipe frames/s with a list of 4096 messages against no list, on the same stream of frames nothing decodes on (synth
    frames at -34 dB, the stream tools/osd_probe.py uses).
Each GPU step runs in a child process of its own under a time limit; a step that fails ends the probe.

usage: deep_probe.py [--items 256] [--frames 2048] [--reps 5] [--out profiles/deep_probe.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    import deep_exact as X
    rng = np.random.default_rng(13)
    sym = np.clip(np.rint(128 + 32 * rng.standard_normal((a.items, 162))), 0, 255).astype(np.uint8)
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE95000)), 65536)
    ctx = G.Context()
    L = ctx.L
    L.uwspr_debug_deep_time.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.from_numpy(sym).to("cuda:0")
    for M in (16, 4096, 65536):
        ctx.deep_set_list(msgs[:M])
        L.uwspr_debug_deep_time(ctx.h, 0, None)
        ctx.deep(dev)   # warm-up: the call's scratch
        L.uwspr_debug_deep_time(ctx.h, 1, None)
        ms = []
        for _ in range(a.reps):
            ctx.deep(dev)
            t = C.c_double(0)
            L.uwspr_debug_deep_time(ctx.h, -1, C.byref(t))
            ms.append(t.value)
        print("k13 score + reduce, %d items x %d messages: median %.3f ms (%.1f G int8 multiply-adds per s), min %.3f" %
              (a.items, M, np.median(ms), 1e-9 * a.items * M * 192 / (1e-3 * np.median(ms)), min(ms)), flush=True)
    ctx.close()


def step_pipe(a):
    import torch
    import gr_uwspr_amd as G
    import deep_exact as X
    frames = G.synth.make_frames_torch(a.frames, "cuda:0", seed=77, snr_db=-34.0)
    torch.cuda.synchronize()
    msgs = X.random_messages(np.random.Generator(np.random.Philox(0xDEE95000)), 4096)
    for known in (None, msgs, None, msgs):
        pipe = G.Pipe(hop=45000, known=known)
        t0 = time.perf_counter()
        for k in range(0, a.frames, 256):
            pipe.submit_device(frames[k:k + 256])
        pipe.flush()
        dt = time.perf_counter() - t0
        recs, st = pipe.collect(cap=1 << 20), pipe.stats()
        pipe.close()
        print("pipe list of %d: %d frames in %.3f s = %.1f k frames/s; decoded %d (list search %d), fano time-outs %d" %
              (0 if known is None else len(known), a.frames, dt, 1e-3 * a.frames / dt, st["decoded"],
               int((recs["osd"] == 2).sum()), st["fano_timeouts"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        {"kernel": step_kernel, "pipe": step_pipe}[a.step](a)
        return 0
    lines = []
    for step, limit in (("kernel", 120), ("pipe", 300)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--items", str(a.items), "--frames", str(a.frames), "--reps", str(a.reps)],
                           capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            print("step %s ended with status %d: the probe stops here" % (step, r.returncode))
            return r.returncode
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
