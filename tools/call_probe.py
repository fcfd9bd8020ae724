#!/usr/bin/env python3
"""K14 (the call search) on the GPU: the time of one uwspr_calls_batch call's launches (HIP events around the score and the
reduce launch: uwspr_debug_calls_time) for --items vectors against call sets of 1, 16 and 64 callsigns, every locator and
power (615 600 hypotheses per callsign), median of --reps after a warm-up, beside the multiply-add count (K = 192 counted).
The GPU step runs in a child process of its own under a time limit.

usage: call_probe.py [--items 256] [--reps 5] [--out profiles/call_probe.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    import call_exact as CX
    rng = np.random.default_rng(14)
    sym = np.clip(np.rint(128 + 32 * rng.standard_normal((a.items, 162))), 0, 255).astype(np.uint8)
    calls = CX.random_calls(np.random.Generator(np.random.Philox(0xCA116000)), 64)
    ctx = G.Context()
    L = ctx.L
    L.uwspr_debug_calls_time.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.from_numpy(sym).to("cuda:0")
    for A in (1, 16, 64):
        ctx.calls_set(calls[:A])
        L.uwspr_debug_calls_time(ctx.h, 0, None)
        ctx.calls(dev)   # warm-up: the call's scratch
        L.uwspr_debug_calls_time(ctx.h, 1, None)
        ms = []
        for _ in range(a.reps):
            ctx.calls(dev)
            t = C.c_double(0)
            L.uwspr_debug_calls_time(ctx.h, -1, C.byref(t))
            ms.append(t.value)
        macs = a.items * A * CX.NGRID * CX.NPOW * 192
        print("k14 score + reduce, %d items x %d callsigns (%.1f M hypotheses, %.2f T multiply-adds): median %.3f ms (%.1f T int8 "
              "multiply-adds per s), min %.3f" % (a.items, A, 1e-6 * A * CX.NGRID * CX.NPOW, 1e-12 * macs, np.median(ms),
                                                  1e-12 * macs / (1e-3 * np.median(ms)), min(ms)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        step_kernel(a)
        return 0
    r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--step", "kernel",
                        "--items", str(a.items), "--reps", str(a.reps)], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        print("the kernel step ended with status %d" % r.returncode)
        return r.returncode
    if a.out:
        with open(a.out, "w") as f:
            f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
