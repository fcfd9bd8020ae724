#!/usr/bin/env python3
"""K7's carrier form on the GPU box -> profiles/transmit_carrier.txt (or the path given).  Device time between two HIP
events on the context's stream around uwspr_tx_render into device memory (where = UWSPR_DEVICE), one hour of int16 audio
per channel, after a warm-up of the same shape; per row the median and the spread (min .. max) of --reps renders:

  1. a channel-hour at 1500 Hz through the 1500 Hz kernels -- on this build and, with --parent-lib, on the library of the
     parent commit loaded beside it, the two interleaved render by render (expect a tie within the spread);
  2. one block, interleaved: the 1500 Hz kernels again; the same hour through the carrier form with "tx_form" = 1, with one
     group at 2203 Hz (rotator) and at 1875 Hz (none); 3 and 8 carrier groups in the one channel (expect linear growth);
  3. 64 channels, one group each, at 1500 Hz (1500 Hz kernels) and at 2203 Hz, interleaved.

usage: python tools/tx_carrier_probe.py [--reps 7] [--parent-lib libuwspr_hip_parent.so] [--out profiles/transmit_carrier.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOUR = 3600 * 12000


def hour_of_signals(channels, carriers):
    """back-to-back two-minute transmissions for an hour on every channel and carrier (the whole hour is signal)"""
    return [{"text": "K1ABC FN42 37", "channel": c, "start": 375 + 45000 * k, "f0": 0.1 * c, "gain": 0.5, "carrier": fc}
            for c in range(channels) for fc in carriers for k in range(3600 * 375 // 45000)]


def context_on(G, libpath, options=None):
    """a Context on another build of the library (the parent commit's), loaded beside this one's"""
    N = G.native
    mine = N.lib()
    other = C.CDLL(libpath)
    for name in N.ABI_SYMBOLS:
        if hasattr(other, name) and hasattr(mine, name):
            getattr(other, name).argtypes = getattr(mine, name).argtypes
            getattr(other, name).restype = getattr(mine, name).restype
    saved, N._lib = N._lib, other
    try:
        return G.Context(options=options)
    finally:
        N._lib = saved


class Case:
    def __init__(self, name, ctx, sig, channels, torch):
        self.name, self.ctx, self.sig, self.channels, self.ms = name, ctx, sig, channels, []
        self.out = torch.empty((HOUR, channels), dtype=torch.int16, device="cuda:0")
        self.stream = torch.cuda.Stream()
        self.torch = torch

    def render(self, timed=True):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        self.ctx.set_stream(self.stream.cuda_stream)           # (cases may share a context: each renders on its own stream)
        a.record(self.stream)
        self.ctx.tx_render(self.sig, HOUR, channels=self.channels, sigma=0.01, format="s16", out=self.out)
        b.record(self.stream)
        b.synchronize()
        self.ctx.set_stream(None)
        if timed:
            self.ms.append(a.elapsed_time(b))

    def row(self):
        m = np.array(self.ms)
        per = np.median(m) / self.channels
        return "%-44s %10.3f %10.3f %10.3f %16.3f" % (self.name, np.median(m), m.min(), m.max(), per)

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


def strip(sig):
    return [{k: v for k, v in s.items() if k != "carrier"} for s in sig]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmit_carrier.txt"))
    a = ap.parse_args()
    import torch
    import gr_uwspr_amd as G
    ctx = G.Context()
    forced = G.Context(options={"tx_form": 1})
    lines = ["K7 carrier form on %s" % ctx.info.device_name.decode(),
             "one hour of int16 audio per channel into device memory, signal throughout, sigma 0.01; device time between two",
             "HIP events on the context's stream around uwspr_tx_render; median (min .. max) of %d renders, the rows of a" % a.reps,
             "block interleaved render by render", "",
             "%-44s %10s %10s %10s %16s" % ("", "median ms", "min ms", "max ms", "ms/channel-hour")]
    h1500 = hour_of_signals(1, [1500])
    before = G.tx_carrier_launch_counts()
    block = [Case("1500 Hz, 1500 Hz kernels, this build", ctx, strip(h1500), 1, torch)]
    parent = None
    if a.parent_lib:
        parent = context_on(G, os.path.abspath(a.parent_lib))
        block.append(Case("1500 Hz, 1500 Hz kernels, parent commit", parent, strip(h1500), 1, torch))
    run(block, a.reps, lines)
    assert G.tx_carrier_launch_counts() == before, "the 1500 Hz rows ran the carrier form"
    if parent is None:
        lines.append("%-44s %s" % ("1500 Hz, 1500 Hz kernels, parent commit", "not measured (no --parent-lib)"))
    else:
        parent.close()
    lines.append("")
    block = [Case("1500 Hz, 1500 Hz kernels", ctx, strip(h1500), 1, torch),
             Case("1500 Hz, carrier form (tx_form = 1)", forced, strip(h1500), 1, torch),
             Case("2203 Hz, one group (rotator)", ctx, hour_of_signals(1, [2203]), 1, torch),
             Case("1875 Hz, one group (no rotator)", ctx, hour_of_signals(1, [1875]), 1, torch),
             Case("3 groups in one channel (497, 1500, 2203)", ctx, hour_of_signals(1, [497, 1500, 2203]), 1, torch),
             Case("8 groups in one channel (300 .. 2050 by 250)", ctx, hour_of_signals(1, list(range(300, 2051, 250))), 1, torch)]
    run(block, a.reps, lines)
    lines.append("")
    block = [Case("64 channels at 1500 Hz, 1500 Hz kernels", ctx, strip(hour_of_signals(64, [1500])), 64, torch),
             Case("64 channels at 2203 Hz, one group each", ctx, hour_of_signals(64, [2203]), 64, torch)]
    run(block, a.reps, lines)
    after = G.tx_carrier_launch_counts()
    lines += ["", "carrier-form launches during the probe: %d (int16 output)" % (after[1] - before[1])]
    ctx.close()
    forced.close()
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
