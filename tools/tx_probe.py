#!/usr/bin/env python3
"""K7 (the transmitter) on the GPU box -> profiles/transmit.txt (or the path given):

  1. render time per channel-hour: one hour of int16 audio per channel rendered into device memory with C = 1, 8, 64
     channels (uwspr_tx_render, where = UWSPR_DEVICE), best of --reps, wall time around the call;
  2. the closed loop at -20 and -28 dB: --slots transmissions of random messages rendered, pushed through
     uwspr_stream_push_audio (front-end K0), searched (uwspr_pipeline_batch) and Fano-decoded -- once with the audio
     left in HBM (a torch CUDA tensor handed to stream_push_audio: no PCIe crossing) and once through host memory.

usage: python tools/tx_probe.py [--reps 3] [--slots 12] [--out profiles/transmit.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render_rates(G, ctx, reps, lines):
    import torch
    n = 3600 * 12000
    lines.append("render: one hour of int16 audio per channel into device memory (best of %d)" % reps)
    lines.append("%8s %12s %16s %14s" % ("C", "wall ms", "ms/channel-hour", "GFLOP/s"))
    for Cn in (1, 8, 64):
        sig = [{"text": "K1ABC FN42 37", "channel": c, "start": 375 + 45000 * k, "f0": 0.1 * c}
               for c in range(Cn) for k in range(0, 3600 * 375 // 45000, 4)]
        out = torch.empty((n, Cn), dtype=torch.int16, device="cuda:0")
        ctx.tx_render(sig, 12000, channels=Cn, sigma=0.01, format="s16", out=out)   # warm-up (taps, LDS attribute)
        best = 1e30
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctx.tx_render(sig, n, channels=Cn, sigma=0.01, format="s16", out=out)
            best = min(best, time.perf_counter() - t)
        flop = 2.0 * 2 * 100 * n * Cn
        lines.append("%8d %12.2f %16.3f %14.0f" % (Cn, best * 1e3, best * 1e3 / Cn, flop / best / 1e9))
        del out
        torch.cuda.empty_cache()


def closed_loop(G, slots, snr, device_resident):
    import torch
    rng = np.random.default_rng(int(abs(snr)) * 100 + slots)
    L = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    sig, want = [], set()
    for s in range(slots):
        call = "".join(rng.choice(list(L), 2)) + str(int(rng.integers(0, 10))) + "".join(rng.choice(list(L), 3))
        grid = "".join(rng.choice(list(L[:18]), 2)) + "%02d" % int(rng.integers(0, 100))
        text = "%s %s %d" % (call, grid, int(rng.choice([0, 10, 20, 30, 37])))
        sig.append({"text": text, "start": 375 * 126 * s + 375, "f0": float(rng.uniform(-6, 6)), "gain": 0.5})
        want.add(G.unpack_message(G.wspr_pack(text))[1])
    n = (126 * (slots - 1) + 122) * 12000
    sigma = G.tx_sigma(snr, 0.5)
    tx, rx = G.Context(), G.Context()
    rx.stream_open(hop=3375, max_frames=256)
    torch.cuda.synchronize()
    t = time.perf_counter()
    if device_resident:
        x = torch.empty((n, 1), dtype=torch.float32, device="cuda:0")
        tx.tx_render(sig, n, sigma=sigma, seed=1, out=x)
        nready = rx.stream_push_audio(x.view(-1))
    else:
        x = tx.tx_render(sig, n, sigma=sigma, seed=1)[:, 0]
        nready = rx.stream_push_audio(x)
    frames = torch.empty((nready, 45000, 2), dtype=torch.float32, device="cuda:0")
    rx.stream_take(nready, frames)
    rx.synchronize()
    _, out = rx.pipeline_batch(frames, max_per_frame=4)
    msg, _, ok = G.decode_batch(out)
    wall = time.perf_counter() - t
    got = {G.unpack_message(m)[1] for m, k in zip(msg, ok) if k}
    tx.close()
    rx.close()
    return wall, len(want & got), len(want), len(got - want), nready


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmit.txt"))
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    ctx = G.Context()
    lines = ["K7 transmitter on %s" % ctx.info.device_name.decode(), ""]
    render_rates(G, ctx, a.reps, lines)
    ctx.close()
    lines += ["", "closed loop: %d two-minute transmissions (126-s slots), render -> stream_push_audio -> "
              "pipeline_batch (4 candidates per frame) -> Fano" % a.slots,
              "%8s %10s %10s %10s %10s %8s" % ("SNR dB", "audio in", "wall s", "decoded", "expected", "extra")]
    closed_loop(G, 2, -20.0, True)   # warm-up
    for snr in (-20.0, -28.0):
        for dev in (True, False):
            w, d, e, x, nf = closed_loop(G, a.slots, snr, dev)
            lines.append("%8.0f %10s %10.3f %10d %10d %8d   (%d frames)" % (snr, "HBM" if dev else "host", w, d, e, x, nf))
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    del torch


if __name__ == "__main__":
    main()
