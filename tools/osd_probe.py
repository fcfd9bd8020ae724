#!/usr/bin/env python3
"""K9 (ordered-statistics decoding) on the GPU:
  * the time of one uwspr_osd_batch launch of --items vectors per order (HIP events around the launch:
    uwspr_debug_osd_time), on noisy codewords;
  * pipe frames/s with osd = 2 against osd = 0 on the same stream of frames nothing decodes on (synth frames at -34 dB).
Each GPU step runs in a child process of its own under a time limit; a step that fails ends the probe.

usage: osd_probe.py [--items 4096] [--frames 2048] [--reps 5] [--out profiles/osd_probe.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    rng = np.random.default_rng(9)
    sym = np.clip(np.rint(128 + 32 * rng.standard_normal((a.items, 162))), 0, 255).astype(np.uint8)
    ctx = G.Context()
    L = ctx.L
    L.uwspr_debug_osd_time.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.from_numpy(sym).to("cuda:0")
    ctx.osd(dev, order=2)   # warm-up: the context's table
    L.uwspr_debug_osd_time(ctx.h, 1, None)
    for order in (0, 1, 2):
        ms = []
        for _ in range(a.reps):
            ctx.osd(dev, order=order)
            t = C.c_double(0)
            L.uwspr_debug_osd_time(ctx.h, -1, C.byref(t))
            ms.append(t.value)
        print("k9_osd order %d, %d items: median %.3f ms (%.2f us per item), min %.3f" %
              (order, a.items, np.median(ms), 1e3 * np.median(ms) / a.items, min(ms)), flush=True)
    ctx.close()


def step_pipe(a):
    import torch
    import gr_uwspr_amd as G
    frames = G.synth.make_frames_torch(a.frames, "cuda:0", seed=77, snr_db=-34.0)
    torch.cuda.synchronize()
    for osd in (0, 2, 0, 2):
        pipe = G.Pipe(hop=45000, osd=osd)
        t0 = time.perf_counter()
        for k in range(0, a.frames, 256):
            pipe.submit_device(frames[k:k + 256])
        pipe.flush()
        dt = time.perf_counter() - t0
        recs, st = pipe.collect(cap=1 << 20), pipe.stats()
        pipe.close()
        print("pipe osd=%d: %d frames in %.3f s = %.1f k frames/s; decoded %d (osd %d), fano time-outs %d" %
              (osd, a.frames, dt, 1e-3 * a.frames / dt, st["decoded"], int(recs["osd"].sum()), st["fano_timeouts"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
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
