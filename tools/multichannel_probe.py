"""C channels of 12 kS/s int16 audio through ONE pipe (uwspr_pipe_push_audio_channels) against the same audio through C
one-channel pipes, one after another -- profiles/multichannel_audio.txt.

    python tools/multichannel_probe.py [--minutes 60] [--channels 1,8,32] [--reps 3] [--out FILE] [--no-rocprof]

For each C: one hour of audio per channel, pushed in 5-minute pieces ([n, C] interleaved for the one pipe, channel c
alone for pipe c), then flush.  Wall time from the first push to the last record (median of --reps after one untimed
run), frames, decodes, and the device memory each pipe holds (free device memory before open minus after the run).
K0's total time comes from a run of its own under `rocprofv3 --kernel-trace --stats` (a child process per form:
`--one C --form multi|single`), reported per channel-hour.
Channel c is the seeded noise of channel 0 rotated by c * 1234567 samples: distinct content, no decodes."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, FL, RATE = 3375, 45000, 12000
PIECE = 5 * 60 * RATE


def audio(minutes, nch):
    n = int(minutes * 60 * RATE)
    x = np.clip(np.rint(np.random.default_rng(0).standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16)
    X = np.empty((n, nch), np.int16)
    for c in range(nch):
        X[:, c] = np.roll(x, c * 1234567)
    return X


def run_multi(G, X):
    nch = X.shape[1] if X.ndim == 2 else 1
    cap = nch * (X.shape[0] // (32 * HOP) + 2)   # >= the records (one per frame): no large buffer inside the timing
    pipe = G.Pipe(hop=HOP)
    try:
        t0 = time.perf_counter()
        for k in range(0, X.shape[0], PIECE):
            pipe.push_audio(X[k: k + PIECE])
        pipe.flush()
        recs = pipe.collect(cap=cap)
        return time.perf_counter() - t0, recs, pipe.stats()["frames"]
    finally:
        pipe.close()


def run_single(G, cols):
    t, recs, frames = 0.0, [], 0
    for x in cols:
        dt, r, f = run_multi(G, x)
        t += dt
        recs.append(r)
        frames += f
    return t, np.concatenate(recs), frames


def device_bytes(G, X):
    """device memory a pipe holds after taking X (one pipe: the lanes' contexts, the ring, K0's buffers)"""
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    pipe = G.Pipe(hop=HOP)
    try:
        for k in range(0, X.shape[0], PIECE):
            pipe.push_audio(X[k: k + PIECE])
        pipe.flush()
        pipe.collect(cap=1 << 22)
        torch.cuda.synchronize()
        return free0 - torch.cuda.mem_get_info(0)[0]
    finally:
        pipe.close()


def k0_profile(nch, form, minutes, timeout):
    """K0's total ns and launches from rocprofv3 --kernel-trace --stats over one run of the form"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="mcprobe_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--one", str(nch), "--form", form, "--minutes", str(minutes)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 exited %d: %s" % (r.returncode, (r.stderr or r.stdout)[-800:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel_stats.csv under %s" % d)
        ns, calls = 0, 0
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                if "k0_frontend" in row["Name"]:
                    ns += int(float(row["TotalDurationNs"]))
                    calls += int(row["Calls"])
        return ns, calls
    finally:
        shutil.rmtree(d, ignore_errors=True)


def one(nch, form, minutes):
    import gr_uwspr_amd as G
    X = audio(minutes, nch)
    if form == "multi":
        run_multi(G, X)
    else:
        run_single(G, [np.ascontiguousarray(X[:, c]) for c in range(nch)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--channels", default="1,8,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multichannel_audio.txt"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--prof-timeout", type=float, default=300.0)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--form", default="multi", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.form, a.minutes)
        return
    import torch
    import gr_uwspr_amd as G
    chans = [int(c) for c in a.channels.split(",")]
    hours = a.minutes / 60.0
    lines = ["audio: %.0f min of int16 noise per channel, %d-minute pushes; device: %s" %
             (a.minutes, PIECE // (60 * RATE), torch.cuda.get_device_name(0)),
             "%-4s %-22s %9s %9s %8s %8s %12s %14s" % ("C", "form", "wall s", "ms/ch-h", "frames", "decoded",
                                                       "device MB", "K0 ms/ch-h")]
    k0 = {}
    for nch in chans:
        X = audio(a.minutes, nch)
        cols = [np.ascontiguousarray(X[:, c]) for c in range(nch)]
        res = {}
        for form, fn in (("multi", lambda: run_multi(G, X)), ("single", lambda: run_single(G, cols))):
            fn()   # untimed: code objects, the host pool, first-touch of pages
            ts, last = [], None
            for _ in range(a.reps):
                dt, recs, frames = fn()
                ts.append(dt)
                last = (recs, frames)
            res[form] = (float(np.median(ts)), last)
        # the one pipe's records of channel c are pipe c's (the single run concatenates the pipes in channel order)
        rm = res["multi"][1][0]
        rm = rm[np.argsort(rm["channel"], kind="stable")].copy()
        rm["channel"] = 0
        same = rm.tobytes() == res["single"][1][0].tobytes()
        mem_multi = device_bytes(G, X)
        mem_single = device_bytes(G, cols[0]) if nch > 1 else mem_multi
        for form in ("multi", "single"):
            if nch == 1 and form == "single":
                continue
            if not a.no_rocprof:
                ns, calls = k0_profile(nch, form, a.minutes, a.prof_timeout)
                k0[(nch, form)] = (ns, calls)
            wall, (recs, frames) = res[form]
            name = ("one pipe, %d channel%s" % (nch, "s" if nch > 1 else "")) if form == "multi" else "%d one-channel pipes" % nch
            mem = mem_multi if form == "multi" else mem_single * nch
            kcol = "%9.2f (%d)" % (k0[(nch, form)][0] / 1e6 / (nch * hours), k0[(nch, form)][1]) if (nch, form) in k0 else "-"
            lines.append("%-4d %-22s %9.3f %9.2f %8d %8d %12.0f %14s" % (
                nch, name, wall, 1e3 * wall / (nch * hours), frames, int(recs["decoded"].sum()), mem / 1e6, kcol))
        lines.append("     records of the one pipe, channel by channel, %s those of the one-channel pipes" %
                     ("equal" if same else "DIFFER FROM"))
        print("\n".join(lines[-3:]), flush=True)
    if k0 and (1, "multi") in k0:
        base = k0[(1, "multi")][0]
        for nch in chans:
            if nch > 1 and (nch, "multi") in k0:
                lines.append("K0 per channel-hour, one pipe of %d channels against one channel: %.3f x" %
                             (nch, k0[(nch, "multi")][0] / nch / base))
    lines.append("(device MB: free device memory before the pipe opened minus after its run, for C one-channel pipes "
                 "C x one pipe's; K0 ms/ch-h: K0's total rocprofv3 time per channel-hour, (launches))")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
