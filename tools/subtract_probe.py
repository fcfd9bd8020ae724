#!/usr/bin/env python
"""K8 (known-symbol subtraction) on the GPU box -> profiles/subtract.txt (or the path given):
  * k8_refine and k8_cancel time for 256 items (HIP events around each launch, one stream: uwspr_debug_subtract_times) and
    the host wall time of the whole call, best of --reps;
  * the cancel test's max |GPU - restatement| / max |x| (tests/test_gpu_subtract.py's case and restatement);
  * pipe frames/s with passes = 2 against passes = 1 on a stream where every frame decodes.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "subtract.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2048)
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    import test_gpu_subtract as T
    ctx = G.Context(device=0)
    lines = ["K8 known-symbol subtraction on %s" % ctx.info.device_name.decode(), ""]

    B = 256
    frames, meta = G.synth.make_frames(B, seed=8100, snr_db=-12.0, return_meta=True)
    sym = G.synth.encode_messages(np.array([m["bits"] for m in meta]))
    items = G.sub_items([{"frame": b, "shift": 375 + 9, "f": meta[b]["f_off"] + 0.02, "symbols": sym[b]} for b in range(B)])
    dev = torch.from_numpy(frames).to("cuda:0")
    out = torch.empty_like(dev)
    import ctypes as C
    L = G.native.lib()
    L.uwspr_debug_subtract_times.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.uwspr_debug_subtract_times(ctx.h, 1, None, None)
    best = {}
    for refine in (0, 1):
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            ctx.subtract(dev, items, refine=bool(refine), out=out)
            wall = 1e3 * (time.perf_counter() - t0)
            r, c = C.c_double(), C.c_double()
            L.uwspr_debug_subtract_times(ctx.h, -1, C.byref(r), C.byref(c))
            b = best.setdefault(refine, [1e9, 1e9, 1e9])
            b[0], b[1], b[2] = min(b[0], r.value), min(b[1], c.value), min(b[2], wall)
    L.uwspr_debug_subtract_times(ctx.h, 0, None, None)
    tr, tc = best[1][0], min(best[0][1], best[1][1])
    lines += ["uwspr_subtract_batch, 256 items in 256 frames, device memory, one stream, best of %d (ms)" % a.reps,
              "HIP events around the launch itself:",
              "  k8_refine   %8.3f   (146 MFLOP per item: %.1f TFLOP/s)" % (tr, 256 * 146e6 / (tr * 1e-3) / 1e12),
              "  k8_cancel   %8.3f   (41472 x 1023 x 2 FMA = 170 MFLOP per item: %.1f TFLOP/s)" % (tc, 256 * 170e6 / (tc * 1e-3) / 1e12),
              "host wall time of the whole call (item upload, two stream synchronisations, k8_copy / k8_pick / k8_apply, results back):",
              "  refine = 0  %8.3f" % best[0][2],
              "  refine = 1  %8.3f" % best[1][2], ""]

    case = T.make_cancel_case(G)
    got, _ = ctx.subtract(case["frames"], case["items"], refine=False)
    err = np.max(np.abs(T.to_c(got) - case["ref"])) / np.max(np.abs(T.to_c(case["frames"])))
    lines += ["cancel, refine = 0, the test's 3 frames / 4 items: max |GPU - binary64 restatement| / max |x| = %.3e" % err,
              "(tests/test_gpu_subtract.py bounds it by 4 x this value)", ""]

    import test_gpu_subtract_edges as E
    s = E.build_surface_cases()
    ctx.subtract(s["frames"], s["items"], refine=True)
    lines.append("refine surface, tests/test_gpu_subtract_edges.py's cases: max over (q, l) of |M_gpu - binary64 restatement| / S_l")
    worst = 0.0
    for n, name in enumerate(s["names"]):
        e = float(E.surface_error(E.read_surface(G, ctx, n), s["Mref"][n], s["S"][n]).max())
        worst = max(worst, e)
        lines.append("  %-24s %.3e" % (name, e))
    lines += ["worst case %.3e (the test bounds every case by 4 x SURFACE_MEASURED)" % worst, ""]
    ctx.close()

    nf = a.frames
    big = G.synth.make_frames_torch(nf, "cuda:0", seed=8200, snr_db=-12.0)
    torch.cuda.synchronize()
    lines.append("pipe, %d frames at -12 dB in HBM (every frame decodes), batches of 256, max_per_frame 1, best of 3 (frames/s)" % nf)
    for passes in (1, 2, 1, 2):
        best, extra = 0.0, 0
        for _ in range(3):
            pipe = G.Pipe(batch_frames=256, max_per_frame=1, passes=passes)
            try:
                t0 = time.perf_counter()
                for k in range(0, nf, 256):
                    pipe.submit_device(big[k:k + 256])
                pipe.flush()
                dt = time.perf_counter() - t0
                recs = pipe.collect(cap=1 << 20)
            finally:
                pipe.close()
            best = max(best, nf / dt)
            extra = int((recs["pass"] == 1).sum())
            dec = int((recs["decoded"] == 1).sum())
        lines.append("  passes = %d   %10.0f   (%d decoded records, %d from the second pass)" % (passes, best, dec, extra))
    lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
