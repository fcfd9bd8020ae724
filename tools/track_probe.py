#!/usr/bin/env python3
"""K15 (trajectory fit of a decoded source) on the GPU:
  * the time of one uwspr_track_batch call's launches (HIP events around them: uwspr_debug_track_time) for 1 and 64 items x
    256 and 4096 trajectories x 9 frequency offsets (qf = 4), and its rate: n nf hypotheses x 41 472 samples x 8 FMAs per
    item -- the correlation alone, as the issue of this kernel counts it -- at 2 flops per FMA, as a share of the 157.3
    TFLOPS FP32 peak;
  * the distance of the 4096 x 9 surface of one item to the binary64 restatement (tests/track_exact.py) on --check
    trajectories spread over the set;
  * pipe frames/s with tracks (256 trajectories x 9) against the same stream without, on frames that decode
    (tests/test_gpu_osd_pipe.py's text_frame model at -20 dB).
Each GPU step runs in a child process of its own under a time limit; a step that fails ends the probe.

usage: track_probe.py [--frames 256] [--reps 5] [--check 32] [--out FILE]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TEXT = "K1ABC FN42 37"
PEAK = 157.3e12


def _grid(G, n):
    k = {256: (4, 8, 8), 4096: (16, 16, 16)}[n]
    return G.track_grid(v=np.linspace(0.5, 8.0, k[0]), d=np.geomspace(20.0, 2000.0, k[1]), tc=np.linspace(-20.0, 130.0, k[2]))


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    import track_exact as TX
    sym = G.wspr_symbols(TEXT)
    ctx = G.Context()
    rng = np.random.Generator(np.random.Philox(0x7AC16))
    sig = {"text": TEXT, "start": 380, "f0": 1.25, "motion": G.track_motion(TX.TRUTH, model="delay")}
    frames = np.stack([ctx.tx_baseband([sig], n=TX.FL) + (2.0 * rng.standard_normal((TX.FL, 2))).astype(np.float32) for _ in range(4)])
    dev = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    shift, f = TX.truth_item(TX.TRUTH, "delay", 380, f0=1.25)
    L = ctx.L
    for n in (256, 4096):
        grid = _grid(G, n)
        assert len(grid) == n
        ctx.track_set(grid, qf=4, model="delay")
        for nitems in (1, 64):
            items = [{"frame": (4 * q) // nitems, "shift": shift + (q % 7) - 3, "f": f, "symbols": sym} for q in range(nitems)]
            ctx.track(dev, items)   # warm-up: the context's buffers, the code object
            L.uwspr_debug_track_time(ctx.h, 1, None)
            ms = []
            for _ in range(a.reps):
                ctx.track(dev, items)
                t = C.c_double(0)
                L.uwspr_debug_track_time(ctx.h, -1, C.byref(t))
                ms.append(t.value)
            L.uwspr_debug_track_time(ctx.h, 0, None)
            flops = 2.0 * 8.0 * n * 9 * TX.N * nitems
            med = float(np.median(ms))
            print("k15_track + k15_pick, %2d items x %4d trajectories x 9: median %.3f ms, min %.3f (%.3f ms per item); "
                  "%.1f TFLOPS of correlation = %.1f %% of the FP32 peak" % (nitems, n, med, min(ms), med / nitems,
                                                                          1e-12 * flops / (1e-3 * med), 100.0 * flops / (1e-3 * med) / PEAK), flush=True)
    pick = np.unique(np.linspace(0, 4095, max(a.check, 1)).astype(int))
    item = {"frame": 0, "shift": shift, "f": f, "symbols": sym}
    _, surf = ctx.track(dev, [item], surface=True)
    df, ta = TX.design(grid[pick], "delay")
    want = TX.surface(frames[0], shift, f, sym, df, ta, 4)
    rel = np.abs(surf[0][pick].astype(np.float64) - want) / want
    print("distance to the binary64 restatement, %d of the 4096 trajectories x 9: largest relative distance %.3g" % (len(pick), rel.max()), flush=True)
    ctx.close()


def step_pipe(a):
    import torch
    import gr_uwspr_amd as G
    from test_gpu_osd_pipe import text_frame
    frames = torch.from_numpy(np.stack([text_frame(G, TEXT, s, -20.0) for s in range(a.frames)])).to("cuda:0")
    torch.cuda.synchronize()
    grid = _grid(G, 256)
    for tracks in (None, grid, None, grid):
        pipe = G.Pipe(hop=45000, tracks=tracks, track_qf=4)
        t0 = time.perf_counter()
        for k in range(0, a.frames, 256):
            pipe.submit_device(frames[k:k + 256])
        pipe.flush()
        dt = time.perf_counter() - t0
        fits, st = pipe.tracks(cap=1 << 20), pipe.stats()
        pipe.close()
        print("pipe tracks=%s: %d frames in %.3f s = %.2f k frames/s; decoded %d, track records %d, resume_s %.3f" %
              ("256 x 9" if tracks is not None else "none", a.frames, dt, 1e-3 * a.frames / dt, st["decoded"], len(fits), st["resume_s"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        {"kernel": step_kernel, "pipe": step_pipe}[a.step](a)
        return 0
    lines = []
    for step, limit in (("kernel", 240), ("pipe", 240)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--frames", str(a.frames), "--reps", str(a.reps), "--check", str(a.check)],
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
