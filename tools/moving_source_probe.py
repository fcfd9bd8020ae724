#!/usr/bin/env python3
"""K7 with moving sources (uwspr_tx_*_moving) on the GPU box -> profiles/moving_source.txt (or the path given):

  1. render time per channel-hour: tx_probe.py's load (one hour of int16 audio per channel into device memory, eight
     transmissions per channel, C = 1, 8, 64, best of --reps), static through uwspr_tx_render, then through
     uwspr_tx_render_moving with 0, 1 and 8 of each channel's transmissions moving, DOPPLER and DELAY;
  2. the coarse search (K3) on the receiver's own hypotheses: each of the 125 grid trajectories rendered noise-free in
     DOPPLER mode (t_first = 0, f0 on a bin centre) as one frame, through K0 (uwspr_frontend_batch) into uwspr_fdr_batch
     with threshold = 1 and with the flowgraph's threshold = 10: is some candidate of the frame nonlinear, is one at
     freq == f0 nonlinear, and does a nonlinear candidate at f0 have the transmitted trajectory's bin-offset sequence
     (FDR_impl.cc:382-385's quantisation; trajectories that share a sequence cannot be told apart);
  3. decoding: the same 125 trajectories, DOPPLER and DELAY, at -20 and -26 dB, 64-channel recordings (two 126-s slots
     per channel, a different message per trajectory) through one multichannel pipe at flowgraph defaults: is the text
     decoded on its channel in its slot.

usage: python tools/moving_source_probe.py [--reps 3] [--out profiles/moving_source.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID_MOTION = {"v": (2.0, 2.0), "p": (0.0, 50.0)}   # the most strongly nonlinear grid trajectory


def render_rates(G, ctx, reps, lines):
    import torch
    n = 3600 * 12000
    lines.append("1. render: one hour of int16 audio per channel into device memory, 8 transmissions per channel "
                 "(best of %d)" % reps)
    lines.append("   ms per channel-hour; 'moving k': k of each channel's 8 transmissions on the trajectory V = (2, 2), "
                 "p = (0, 50)")
    cols = [("static", None, 0), ("moving 0", "doppler", 0), ("doppler 1", "doppler", 1), ("doppler 8", "doppler", 8),
            ("delay 1", "delay", 1), ("delay 8", "delay", 8)]
    lines.append("%6s" % "C" + "".join("%12s" % c[0] for c in cols))
    for Cn in (1, 8, 64):
        out = torch.empty((n, Cn), dtype=torch.int16, device="cuda:0")
        row = "%6d" % Cn
        for name, model, k in cols:
            sig = []
            for c in range(Cn):
                for i, slot in enumerate(range(0, 3600 * 375 // 45000, 4)):
                    s = {"text": "K1ABC FN42 37", "channel": c, "start": 375 + 45000 * slot, "f0": 0.1 * c}
                    if model is not None:
                        s["motion"] = dict(GRID_MOTION, model=model) if i < k else {"model": "static"}
                    sig.append(s)
            ctx.tx_render(sig, 12000, channels=Cn, sigma=0.01, format="s16", out=out)   # warm-up
            best = 1e30
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ctx.tx_render(sig, n, channels=Cn, sigma=0.01, format="s16", out=out)
                best = min(best, time.perf_counter() - t)
            row += "%12.3f" % (best * 1e3 / Cn)
        lines.append(row)
        del out
        torch.cuda.empty_cache()


def offset_sequence(info, traj, ifr, cf=1500.0):
    """ifd - ifr for k = 0..161 as K3 quantises a trajectory (FDR_impl.cc:382-385: t = k*111/162 in integers,
    slmFrequencyDrift in binary64 returned as binary32, (int)((float)ifr + drift / df) in binary32)"""
    V1, V2, p1, p2 = (float(x) for x in traj)
    df = np.float32(info.df)
    out = np.zeros(162, np.int64)
    for k in range(162):
        t = float(np.float32(k * 111 // 162))
        q1, q2 = V1 * t + p1, V2 * t + p2
        sign = 1.0 if (q1 * V1 + q2 * V2) > 0 else -1.0
        den = np.sqrt(q1 * q1 + q2 * q2)
        d = np.float32(0.0) if den == 0 else np.float32(-sign * abs(V1 * q1 + V2 * q2) / den * float(np.float32(cf)) / 1500.0)
        out[k] = int(np.float32(np.float32(ifr) + np.float32(d / df))) - ifr
    return out


def coarse_table(G, f0_bins=4):
    import torch
    N = G.native
    trajs = G.slm_trajectories()
    f0 = f0_bins * 375.0 / 512
    nin = 45000 * 32
    audio = torch.zeros((len(trajs), nin), dtype=torch.float32, device="cuda:0")
    tx = G.Context()
    for i, tr in enumerate(trajs):
        sig = [{"text": "K1ABC FN42 37", "start": 375, "f0": f0,
                "motion": {"v": (tr[0], tr[1]), "p": (tr[2], tr[3]), "model": "doppler"}}]
        tx.tx_render(sig, nin, out=audio[i])
    tx.close()
    res = {}
    for thr in (1, 10):
        rx = G.Context(threshold=thr)
        frames = rx.frontend(audio)
        cands = rx.fdr_batch(frames)
        info = rx.info
        rows = []
        for i, tr in enumerate(trajs):
            cs = cands[i]
            nl = cs[cs["m_type"] == N.NONLINEAR]
            at = nl[nl["freq"] == np.float32(f0)]
            match = False
            for c in at:
                ifr = info.m + int(round(float(c["freq"]) / float(info.df)))
                got = offset_sequence(info, (c["V1"], c["V2"], c["p1"], c["p2"]), ifr)
                match = match or bool((got == offset_sequence(info, tr, ifr)).all())
            rows.append((len(nl) > 0, len(at) > 0, match, len(cs)))
        res[thr] = rows
        rx.close()
    return f0, res


def _text(i):
    L = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    return "K%d%s%s FN%02d 37" % (i % 10, L[(i // 10) % 26], L[(i * 7) % 26] + L[(i * 3 + 1) % 26], i % 100)


def decode_table(G, model, snr):
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
    pipe = G.Pipe(batch_frames=64)
    try:
        step = 500_000
        for k in range(0, n, step):
            pipe.push_audio(tx.tx_render(sig, min(step, n - k), t0=k, channels=Cn, sigma=G.tx_sigma(snr),
                                         seed=[1000 + c for c in range(Cn)], format="s16"))
        pipe.flush()
        recs = pipe.collect(cap=1 << 18)
    finally:
        pipe.close()
        tx.close()
    ok = np.zeros(len(trajs), bool)
    extra = 0
    for r in recs[recs["decoded"] == 1]:
        c, s = int(r["channel"]), int(round(int(r["stream_pos"]) / 375.0 / slot_s))
        text = G.unpack_message(r["message"])[1]
        if (c, s) in want and want[(c, s)][1] == text:
            ok[want[(c, s)][0]] = True
        else:
            extra += 1
    return ok, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moving_source.txt"))
    ap.add_argument("--skip", default="", help="comma-separated parts to skip (1, 2, 3)")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) - {""}
    import gr_uwspr_amd as G
    ctx = G.Context()
    lines = ["K7 moving sources on %s" % ctx.info.device_name.decode(), ""]
    if "1" not in skip:
        render_rates(G, ctx, a.reps, lines)
        lines.append("")
    ctx.close()
    trajs = G.slm_trajectories()
    cols = []
    if "2" not in skip:
        f0, res = coarse_table(G)
        lines.append("2. coarse search (K0 -> K3), DOPPLER, noise-free, t_first = 0, f0 = %.6f Hz (4 bins): per threshold, "
                     "nl = some candidate nonlinear, f0nl = a nonlinear candidate at freq == f0, seq = one of those has "
                     "the transmitted bin-offset sequence" % f0)
        for thr in (1, 10):
            r = res[thr]
            lines.append("   threshold %2d: nl %3d / 125, f0nl %3d / 125, seq %3d / 125" %
                         (thr, sum(x[0] for x in r), sum(x[1] for x in r), sum(x[2] for x in r)))
        cols.append(("thr1 nl f0nl seq", [" %d %d %d" % x[:3] for x in res[1]]))
        cols.append(("thr10 nl f0nl seq", [" %d %d %d" % x[:3] for x in res[10]]))
        lines.append("")
    if "3" not in skip:
        lines.append("3. decode: 64-channel recordings through one pipe at flowgraph defaults (threshold 10), t_first = 0, "
                     "f0 = 0, a different message per trajectory; 1 = decoded on its channel in its slot")
        for model in ("doppler", "delay"):
            for snr in (-20.0, -26.0):
                t = time.perf_counter()
                ok, extra = decode_table(G, model, snr)
                lines.append("   %-7s %4.0f dB: %3d / 125 decoded, %d other decodes (%.1f s)" %
                             (model, snr, int(ok.sum()), extra, time.perf_counter() - t))
                cols.append(("%s%d" % (model[:3], int(snr)), [" %d" % v for v in ok]))
        lines.append("")
    if cols:
        lines.append("per trajectory (slmGenerator order: p2 fastest, then V1, then V2; p1 = 0)")
        lines.append("%4s %4s %4s %4s  " % ("i", "V1", "V2", "p2") + "  ".join(c[0] for c in cols))
        for i, tr in enumerate(trajs):
            lines.append("%4d %4.0f %4.0f %4.0f  " % (i, tr[0], tr[1], tr[3]) +
                         "  ".join(c[1][i].rjust(len(c[0])) for c in cols))
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
