"""How the seeds and the level of tests/test_gpu_calls_pipe.py were picked, on the CPU: frames of that test's model
(text_frame of tests/test_gpu_osd_pipe.py) carrying TEXT through the oracle's FDR + schedule, the host Fano decoder on
every gated try, and the numpy restatement of the call search (tests/call_exact.py) under the pipe's item rule at the
default thresholds, against that test's two call sets of 8 callsigns, all locators and powers: CALLS_WITH holds TEXT's
callsign, CALLS_OTHER does not.  Prints per level the seeds whose strongest candidate Fano decodes on no try and the
restatement accepts as TEXT with CALLS_WITH while it accepts nothing with CALLS_OTHER ("call"); those it accepts with
neither ("lost"); those Fano decodes ("fano"); and those on which another message was accepted ("wrong").

python tests/golden/make_call_pipe_seeds.py [first] [count] [snr ...]"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]


def classify(args):
    import gr_uwspr_amd as G
    import oracle_py as O
    import call_exact as CX
    from test_gpu_calls_pipe import TEXT, CALLS_WITH, CALLS_OTHER
    from test_gpu_osd_pipe import text_frame
    seed, snr = args
    N = G.native
    frame = text_frame(G, TEXT, seed, snr)
    cands = O.FDR().transform(frame)
    if not len(cands):
        return seed, "none"
    d = O.demod_candidate(cands[0], 1500, frame)
    g = [t for t in range(17) if d["jig_sync"][t] > np.float32(0.12) and d["jig_rms"][t] > np.float32(52.0 * (50 / 64.0))]
    if not d["worth_a_try"] or not g:
        return seed, "none"
    if any(G.fano_decode(G.deinterleave(d["symbols"][t]))[0] == 0 for t in g):
        return seed, "fano"
    t = max(g, key=lambda k: (d["jig_sync"][k], -k))
    nhyp = 8 * CX.NGRID * CX.NPOW
    r = CX.call_restate(G, CALLS_WITH, None, 0, d["symbols"][t])[0]
    ro = CX.call_restate(G, CALLS_OTHER, None, 0, d["symbols"][t])[0]
    if CX.accepted(ro, nhyp, N.CALL_MIN_DEFAULT, N.CALL_GAP_DEFAULT):
        return seed, "wrong"
    if not CX.accepted(r, nhyp, N.CALL_MIN_DEFAULT, N.CALL_GAP_DEFAULT):
        return seed, "lost"
    a, gg, dd = CX.split_h(int(r["best"]))
    same = np.array_equal(CX.message(G, CALLS_WITH[a], gg, CX.P19[dd]), G.wspr_pack(TEXT))
    return seed, "call" if same else "wrong"


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    levels = [float(v) for v in sys.argv[3:]] or [-29.0, -30.0, -31.0, -32.0]
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()
    with multiprocessing.get_context("spawn").Pool(8) as pool:
        for snr in levels:
            res = pool.map(classify, [(s, snr) for s in range(first, first + count)], chunksize=4)
            print("snr %g dB" % snr)
            for kind in ("call", "lost", "fano", "wrong", "none"):
                seeds = [s for s, k in res if k == kind]
                print(" ", kind, len(seeds), seeds[:40], flush=True)
