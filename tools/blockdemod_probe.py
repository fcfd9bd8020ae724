#!/usr/bin/env python3
"""K10 (block demodulation) on the GPU:
  * the time of one uwspr_blockdemod_batch launch of 1, 64 and 512 items (HIP events around the launch:
    uwspr_debug_blockdemod_time), items spread over 8 frames of tests/test_gpu_osd_pipe.py's text_frame model;
  * the distance of the 512-item call to the binary64 restatement (tests/blockdemod_exact.py: block_restate), on its
    first --check items (default: all): the share of bytes that differ and the largest difference;
  * pipe frames/s with block = 3 against block = 0 on the same stream of frames nothing decodes on (synth frames at -34 dB).
Each GPU step runs in a child process of its own under a time limit; a step that fails ends the probe.

usage: blockdemod_probe.py [--frames 1024] [--reps 5] [--check 512] [--out FILE]
(--out: the steps' output is also written to FILE; by default it only goes to standard output)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _items(n, offs):
    rng = np.random.Generator(np.random.Philox(0xB10C0))
    fr = np.sort(rng.integers(0, len(offs), n))
    return [{"frame": int(b), "shift": int(rng.integers(-300, 4300)), "f": offs[b] + float(rng.uniform(-1.0, 1.0)),
             "drift": float(rng.choice([0.0, 2.0, -2.0]))} for b in fr]


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    from blockdemod_exact import block_restate, frame_offset
    from test_gpu_osd_pipe import text_frame
    seeds = list(range(100, 108))
    frames = np.stack([text_frame(G, "K1ABC FN42 37", s, -28.0) for s in seeds])
    offs = [frame_offset(s) for s in seeds]
    ctx = G.Context()
    L = ctx.L
    L.uwspr_debug_blockdemod_time.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    ctx.blockdemod(dev, _items(8, offs))   # warm-up: the context's buffers, the code object
    L.uwspr_debug_blockdemod_time(ctx.h, 1, None)
    for n in (1, 64, 512):
        items, ms = _items(n, offs), []
        for _ in range(a.reps):
            got = ctx.blockdemod(dev, items)
            t = C.c_double(0)
            L.uwspr_debug_blockdemod_time(ctx.h, -1, C.byref(t))
            ms.append(t.value)
        print("k10_blockdemod, %d items: median %.3f ms (%.2f us per item), min %.3f" %
              (n, np.median(ms), 1e3 * np.median(ms) / n, min(ms)), flush=True)
    pick = list(range(min(max(a.check, 1), 512)))
    want = np.stack([block_restate(frames[items[q]["frame"]], items[q]["shift"], items[q]["f"], items[q]["drift"], G.synth.PR3)
                     for q in pick])
    d = np.abs(got[pick].astype(np.int32) - want.astype(np.int32))
    print("distance to the binary64 restatement, %d items of the 512: %d of %d bytes differ (%.4f %%), largest difference %d" %
          (len(pick), int((d > 0).sum()), d.size, 100.0 * (d > 0).mean(), int(d.max())), flush=True)
    ctx.close()


def step_pipe(a):
    import torch
    import gr_uwspr_amd as G
    frames = G.synth.make_frames_torch(a.frames, "cuda:0", seed=77, snr_db=-34.0)
    torch.cuda.synchronize()
    for block in (0, 3, 0, 3):
        pipe = G.Pipe(hop=45000, block=block)
        t0 = time.perf_counter()
        for k in range(0, a.frames, 256):
            pipe.submit_device(frames[k:k + 256])
        pipe.flush()
        dt = time.perf_counter() - t0
        recs, st = pipe.collect(cap=1 << 20), pipe.stats()
        pipe.close()
        print("pipe block=%d: %d frames in %.3f s = %.1f k frames/s; decoded %d (block %d), fano calls %d, time-outs %d" %
              (block, a.frames, dt, 1e-3 * a.frames / dt, st["decoded"], int((recs["block"] != 0).sum()), st["fano_calls"],
               st["fano_timeouts"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        {"kernel": step_kernel, "pipe": step_pipe}[a.step](a)
        return 0
    lines = []
    for step, limit in (("kernel", 120), ("pipe", 300)):
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
