#!/usr/bin/env python3
"""K16 (blind demodulation along straight-line passes) on the GPU:
  * the time of one uwspr_follow_batch call's launches (HIP events around them: uwspr_debug_follow_time) for 1 and 64 items
    at a few (n, qf, nl), and its rate counted as the grid sums alone: n nlg (nf + 24) sums x 41 472 samples x 4 FMAs per
    item, at 2 flops per FMA, as a share of the 157.3 TFLOPS FP32 peak;
  * pipe frames/s on a stream of Fano time-outs (tests/test_gpu_block_pipe.py's "lost" frames, repeated) with a follow set
    (64 passes, qf 8, 1 lag) and without;
  * the table of profiles/moving_source.txt part 3 again -- the receiver's own 125 grid trajectories, 64-channel recordings
    at flowgraph defaults, both models at -20 and -26 dB -- without follow and with follow = a product grid that does NOT
    hold the true passes (7 speeds x 7 CPA ranges x 12 CPA times = 588 passes, qf 16, 2 lags).
Each GPU step runs in a child process of its own under a time limit; a step that fails ends the probe.

usage: follow_probe.py [--frames 64] [--reps 5] [--out FILE] [--skip kernel,pipe,table]"""
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


def product_grid(G):
    return G.track_grid(v=np.linspace(0.75, 3.0, 7), d=(1.0, 40.0, 100.0, 200.0, 350.0, 550.0, 850.0), tc=np.linspace(-40.0, 150.0, 12))


def step_kernel(a):
    import torch
    import gr_uwspr_amd as G
    import follow_cases as FC
    import track_exact as TX
    ctx = G.Context()
    truth = FC.truth(G, 21)
    frames = np.stack([FC.frame(G, 21, "delay", seed=s) for s in range(1, 5)])
    dev = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    shift, f = TX.truth_item(truth, "delay", FC.START, f0=FC.F0)
    L = ctx.L
    big = G.track_grid(v=np.linspace(0.5, 8.0, 16), d=np.geomspace(20.0, 2000.0, 16), tc=np.linspace(-20.0, 130.0, 16))
    for n, qf, nl in ((64, 8, 1), (588, 16, 2), (4096, 4, 0), (4096, 16, 2)):
        grid = product_grid(G) if n == 588 else big[:n]
        assert len(grid) == n
        ctx.follow_set(grid, qf=qf, lags=nl, model="delay")
        for nitems in (1, 64):
            items = [{"frame": (4 * q) // nitems, "shift": shift + (q % 7) - 3, "f": f} for q in range(nitems)]
            ctx.follow(dev, items)   # warm-up: the context's buffers, the code object
            L.uwspr_debug_follow_time(ctx.h, 1, None)
            ms = []
            for _ in range(a.reps):
                ctx.follow(dev, items)
                t = C.c_double(0)
                L.uwspr_debug_follow_time(ctx.h, -1, C.byref(t))
                ms.append(t.value)
            L.uwspr_debug_follow_time(ctx.h, 0, None)
            flops = 2.0 * 4.0 * n * (2 * nl + 1) * (2 * qf + 25) * TX.N * nitems
            med = float(np.median(ms))
            print("k16_follow + k16_pick + k16_soft, %2d items x %4d passes, qf %2d, nl %d (%7d hypotheses): median %8.3f ms, min %8.3f "
                  "(%7.3f ms per item); %5.1f TFLOPS of grid sums = %4.1f %% of the FP32 peak" % (
                      nitems, n, qf, nl, n * (2 * qf + 1) * (2 * nl + 1), med, min(ms), med / nitems, 1e-12 * flops / (1e-3 * med),
                      100.0 * flops / (1e-3 * med) / PEAK), flush=True)
    ctx.close()


def step_pipe(a):
    import torch
    import gr_uwspr_amd as G
    from test_gpu_block_pipe import SEEDS_LOST, SNR_DB
    from test_gpu_osd_pipe import text_frame
    lost = [text_frame(G, TEXT, s, SNR_DB) for s in SEEDS_LOST]
    frames = torch.from_numpy(np.stack([lost[k % len(lost)] for k in range(a.frames)])).to("cuda:0")
    torch.cuda.synchronize()
    grid = G.track_grid(v=(1.0, 2.0, 3.0, 4.0), d=(50.0, 100.0, 200.0, 400.0), tc=(15.0, 45.0, 75.0, 105.0))
    for follow in (None, grid, None, grid):
        pipe = G.Pipe(hop=45000, batch_frames=min(a.frames, 256), follow=follow, follow_qf=8, follow_lags=1)
        t0 = time.perf_counter()
        for k in range(0, a.frames, 256):
            pipe.submit_device(frames[k:k + 256])
        pipe.flush()
        dt = time.perf_counter() - t0
        recs, st = pipe.collect(cap=1 << 20), pipe.stats()
        pipe.close()
        print("pipe on Fano time-outs, follow=%s: %d frames in %.3f s = %.1f frames/s; decoded %d (by follow %d), fano_calls %d, resume_s %.3f" %
              ("64 x 17 x 3" if follow is not None else "none", a.frames, dt, a.frames / dt, st["decoded"], int((recs["osd"] == 4).sum()),
               st["fano_calls"], st["resume_s"]), flush=True)


def _text(i):
    L = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    return "K%d%s%s FN%02d 37" % (i % 10, L[(i // 10) % 26], L[(i * 7) % 26] + L[(i * 3 + 1) % 26], i % 100)


def decode_table(G, model, snr, **pipe_kw):
    """tools/moving_source_probe.py's decode_table through a pipe with pipe_kw -> (decoded per trajectory, decoded by follow per
    trajectory, other decodes, follow's items that decoded)"""
    trajs = G.slm_trajectories()
    Cn, slots, slot_s = 64, 2, 126
    sig, want = [], {}
    for i, tr in enumerate(trajs):
        c, s = i % Cn, i // Cn
        sig.append({"text": _text(i), "channel": c, "start": 375 * slot_s * s + 375,
                    "motion": {"v": (tr[0], tr[1]), "p": (tr[2], tr[3]), "model": model}})
        want[(c, s)] = (i, G.unpack_message(G.wspr_pack(_text(i)))[1])
    n = (slot_s * (slots - 1) + 122) * 12000
    tx = G.Context()
    pipe = G.Pipe(batch_frames=64, **pipe_kw)
    try:
        step = 500_000
        for k in range(0, n, step):
            pipe.push_audio(tx.tx_render(sig, min(step, n - k), t0=k, channels=Cn, sigma=G.tx_sigma(snr),
                                         seed=[1000 + c for c in range(Cn)], format="s16"))
        pipe.flush()
        recs = pipe.collect(cap=1 << 18)
        st = pipe.stats()
    finally:
        pipe.close()
        tx.close()
    ok, by = np.zeros(len(trajs), bool), np.zeros(len(trajs), bool)
    extra = 0
    for r in recs[recs["decoded"] == 1]:
        c, s = int(r["channel"]), int(round(int(r["stream_pos"]) / 375.0 / slot_s))
        text = G.unpack_message(r["message"])[1]
        if (c, s) in want and want[(c, s)][1] == text:
            ok[want[(c, s)][0]] = True
            by[want[(c, s)][0]] |= bool(r["osd"] == 4)
        else:
            extra += 1
    return ok, by, extra, st


def step_table(a):
    import gr_uwspr_amd as G
    grid = product_grid(G)
    print("moving sources, profiles/moving_source.txt part 3 again: follow = %d passes (v %s m/s x d %s m x tc %s s), qf 16, 2 lags, "
          "the model of the recording" % (len(grid), np.round(np.unique(grid["v"]), 3).tolist(), np.unique(grid["d"]).tolist(),
                                          np.round(np.unique(grid["tc"]), 1).tolist()))
    for model in ("doppler", "delay"):
        for snr in (-20.0, -26.0):
            t0 = time.perf_counter()
            ok0, _, extra0, st0 = decode_table(G, model, snr)
            t1 = time.perf_counter()
            ok, by, extra, st = decode_table(G, model, snr, follow=grid, follow_qf=16, follow_lags=2, follow_model=model)
            t2 = time.perf_counter()
            print("   %-7s %4.0f dB: plain %3d / 125 decoded, %d other decodes (%.1f s); follow %3d / 125, %d other decodes (%.1f s, fano_calls "
                  "%d -> %d); recovered %s; lost with follow %s; still lost %s" % (
                      model, snr, int(ok0.sum()), extra0, t1 - t0, int(ok.sum()), extra, t2 - t1, st0["fano_calls"], st["fano_calls"],
                      np.flatnonzero(ok & ~ok0).tolist(), np.flatnonzero(ok0 & ~ok).tolist(), np.flatnonzero(~ok).tolist()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip", default="")
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        {"kernel": step_kernel, "pipe": step_pipe, "table": step_table}[a.step](a)
        return 0
    skip = set(a.skip.split(",")) - {""}
    lines = []
    for step, limit in (("kernel", 240), ("pipe", 240), ("table", 500)):
        if step in skip:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--frames", str(a.frames), "--reps", str(a.reps)], capture_output=True, text=True)
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
