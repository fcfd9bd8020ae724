#!/usr/bin/env python3
"""K7's medium form on the GPU box -> profiles/medium.txt (or the path given).  Device time between two HIP events on
the context's stream around the render into device memory (where = UWSPR_DEVICE), one hour of int16 audio of one channel,
after a warm-up of the same shape; per row the median and the spread (min .. max) of --reps renders:

  (a) a channel-hour at 1500 Hz through the 1500 Hz kernels -- on this build and, with --parent-lib, on the library of the
      parent commit loaded beside it, the two interleaved render by render.  The margin is the run-to-run spread of the
      session itself: the two tie when their medians differ by no more than the larger of the two (max - min);
  (b) the medium form, interleaved with the 1500 Hz kernels: the carrier form alone (tx_form = 1: what the medium form is
      built on), one faded signal with 16 paths, impulses of length 1 and of length 8, both together;
  (c) the compiler's resource report for the render instances (--resources-from: a file made where the library is built
      with --resources-only, which compiles k7_transmit.hip alone with -Rpass-analysis=kernel-resource-usage);
  (d) with --decode: the decode rate over 16 seeds at -24 dB in 2500 Hz, Rayleigh fading of spread 0, 0.05, 0.2 and 1 Hz,
      with block = 0 and block = 3 (16 channels of one render, each with its own fade and noise seed, into one pipe).

usage: python tools/medium_probe.py [--reps 7] [--parent-lib lib.so] [--resources-from file] [--decode] [--out profiles/medium.txt]
       python tools/medium_probe.py --resources-only > file"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOUR = 3600 * 12000
TEXT = "VE3EMB FN25 30"


def hour_of_signals(fading=None):
    """back-to-back two-minute transmissions for an hour (the whole hour is signal), every one faded when asked"""
    sig = [{"text": "K1ABC FN42 37", "start": 375 + 45000 * k, "f0": 0.1, "gain": 0.5} for k in range(3600 * 375 // 45000)]
    return [dict(s, fading=dict(fading, seed=i)) for i, s in enumerate(sig)] if fading else sig


class Case:
    def __init__(self, name, ctx, sig, torch, impulses=None):
        self.name, self.ctx, self.sig, self.impulses, self.ms = name, ctx, sig, impulses, []
        self.out = torch.empty((HOUR, 1), dtype=torch.int16, device="cuda:0")
        self.stream = torch.cuda.Stream()
        self.torch = torch

    def render(self, timed=True):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        self.ctx.set_stream(self.stream.cuda_stream)
        a.record(self.stream)
        kw = {} if self.impulses is None else {"impulses": self.impulses}     # (the parent's tx_render has no such argument)
        self.ctx.tx_render(self.sig, HOUR, channels=1, sigma=0.01, format="s16", out=self.out, **kw)
        b.record(self.stream)
        b.synchronize()
        self.ctx.set_stream(None)
        if timed:
            self.ms.append(a.elapsed_time(b))

    def row(self):
        m = np.array(self.ms)
        return "%-52s %10.3f %10.3f %10.3f" % (self.name, np.median(m), m.min(), m.max())

    def free(self):
        del self.out
        self.torch.cuda.empty_cache()


def run(cases, reps, lines):
    """warm every case, then time them interleaved: A B C A B C ..."""
    for _ in range(3):
        for c in cases:
            c.render(timed=False)
    for _ in range(reps):
        for c in cases:
            c.render()
    for c in cases:
        lines.append(c.row())
        c.free()


def resources():
    """the compiler's report for k7_render's instances: k7_transmit.hip compiled alone with the library's flags"""
    import gr_uwspr_amd as G
    N = G.native
    cmd = [N._hipcc()] + [f for f in N.HIPFLAGS if f != "-fPIC"] + ["-I" + os.path.join(ROOT, "include"), "-c",
                                                                   os.path.join(N.CSRC, "k7_transmit.hip"), "-o", os.devnull,
                                                                   "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|TotalSGPRs|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    out = ["%-34s %6s %6s %8s %11s %11s %10s" % ("k7_render<S16, MOVING, CARRIER, MEDIUM>", "VGPRs", "AGPRs", "SGPRs", "VGPR spill", "SGPR spill", "scratch B")]
    for r in rows:
        m = re.match(r"_ZN5uwspr9k7_renderILb(\d)ELb(\d)ELb(\d)ELb(\d)EEE", r["name"])
        if m:
            out.append("%-34s %6s %6s %8s %11s %11s %10s" % ("<%s, %s, %s, %s>" % m.groups(), r["VGPRs"], r["AGPRs"], r["TotalSGPRs"],
                                                             r["VGPRs Spill"], r["SGPRs Spill"], r["ScratchSize [bytes/lane]"]))
    return "\n".join(out)


def decode_table(G, lines, seeds=16, snr_db=-24.0):
    ctx = G.Context()
    n = 1440000 + 64
    lines.append("decodes of %d seeds, one Rayleigh transmission (16 paths) at %.0f dB in 2500 Hz, 120 s, max_per_frame 2" % (seeds, snr_db))
    lines.append("%-14s %10s %10s" % ("spread Hz", "block = 0", "block = 3"))
    want = G.unpack_message(G.wspr_pack(TEXT))[1]
    for spread in (0.0, 0.05, 0.2, 1.0):
        sig = [{"text": TEXT, "start": 375, "f0": 2.0, "channel": c, "fading": {"spread": spread, "k": 0.0, "seed": c, "paths": 16}}
               for c in range(seeds)]
        x = ctx.tx_render(sig, n, channels=seeds, sigma=G.tx_sigma(snr_db), seed=[500 + c for c in range(seeds)])
        got = []
        for block in (0, 3):
            pipe = G.Pipe(batch_frames=4, max_per_frame=2, block=block)
            try:
                for k in range(0, n, 250000):
                    pipe.push_audio(x[k:k + 250000])
                pipe.flush()
                recs = pipe.collect(cap=1 << 16)
            finally:
                pipe.close()
            ok = {int(r["channel"]) for r in recs if r["decoded"] and G.unpack_message(r["message"])[1] == want}
            got.append(len(ok))
        lines.append("%-14g %7d/%d %7d/%d" % (spread, got[0], seeds, got[1], seeds))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--resources-from", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "medium.txt"))
    a = ap.parse_args()
    if a.resources_only:
        print(resources())
        return
    import torch
    import gr_uwspr_amd as G
    from tx_carrier_probe import context_on
    ctx = G.Context()
    forced = G.Context(options={"tx_form": 1})
    lines = ["K7 medium form on %s" % ctx.info.device_name.decode(),
             "one hour of int16 audio of one channel into device memory, signal throughout, sigma 0.01; device time between two",
             "HIP events on the context's stream around the render; median (min .. max) of %d renders, the rows of a block" % a.reps,
             "interleaved render by render", "",
             "(a) the 1500 Hz kernels, this build against the parent commit's",
             "%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    plain = hour_of_signals()
    before = (G.tx_medium_launch_counts(), G.tx_carrier_launch_counts())
    block = [Case("1500 Hz kernels, this build", ctx, plain, torch)]
    parent = None
    if a.parent_lib:
        parent = context_on(G, os.path.abspath(a.parent_lib))
        block.append(Case("1500 Hz kernels, parent commit", parent, plain, torch))
    run(block, a.reps, lines)
    assert (G.tx_medium_launch_counts(), G.tx_carrier_launch_counts()) == before, "the 1500 Hz rows ran another form"
    if parent is None:
        lines.append("%-52s %s" % ("1500 Hz kernels, parent commit", "not measured (no --parent-lib)"))
    else:
        m = [np.array(c.ms) for c in block]
        spread = max(x.max() - x.min() for x in m)
        diff = abs(np.median(m[0]) - np.median(m[1]))
        lines.append("difference of the medians %.3f ms, run-to-run spread (the larger max - min) %.3f ms: %s"
                     % (diff, spread, "a tie" if diff <= spread else "NOT a tie"))
        parent.close()
    fade = {"spread": 1.0, "k": 0.0, "paths": 16}
    short, long_ = {"rate": 1.0 / 250, "sigma": 0.6, "seed": 5, "length": 1}, {"rate": 1.0 / 250, "sigma": 0.6, "seed": 5, "length": 8}
    lines += ["", "(b) the medium form (impulses: probability 1/250 per sample)",
              "%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    block = [Case("1500 Hz kernels", ctx, plain, torch),
             Case("carrier form alone (tx_form = 1)", forced, plain, torch),
             Case("medium: every transmission faded, 16 paths", ctx, hour_of_signals(fade), torch),
             Case("medium: impulses of length 1", ctx, plain, torch, short),
             Case("medium: impulses of length 8", ctx, plain, torch, long_),
             Case("medium: faded, 16 paths, and impulses of length 8", ctx, hour_of_signals(fade), torch, long_)]
    run(block, a.reps, lines)
    after = G.tx_medium_launch_counts()
    lines += ["medium-form launches during the block: %d (int16 output)" % (after[1] - before[0][1]), "",
              "(c) the compiler's resource report (1024-thread workgroups: 128 VGPRs per lane)"]
    lines.append(open(a.resources_from).read().rstrip() if a.resources_from else "not measured (no --resources-from)")
    lines += ["", "(d) decoding under fading"]
    if a.decode:
        decode_table(G, lines)
    else:
        lines.append("not measured (no --decode)")
    ctx.close()
    forced.close()
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
