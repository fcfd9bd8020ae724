"""How the seeds of tests/test_gpu_osd_pipe.py were picked, on the CPU: frames of that test's model (its text_frame) through
the oracle's FDR + schedule, the host Fano decoder on every gated try, and the numpy restatement of ordered-statistics
decoding under the pipe's item rule.  Prints the seeds whose strongest candidate Fano decodes on no try and restated
order 2 recovers with dnext - dmin >= the default gap ("osd"), and those it does not recover ("lost").

python tests/golden/make_osd_pipe_seeds.py [first] [count]"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]


def classify(seed):
    import gr_uwspr_amd as G
    import oracle_py as O
    from test_gpu_osd import osd_restate
    from test_gpu_osd_pipe import SNR_DB, TEXT, text_frame
    frame = text_frame(G, TEXT, seed, SNR_DB)
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
    r = osd_restate(d["symbols"][t], 2)
    ok = r[4].tobytes() == G.wspr_pack(TEXT).tobytes() and r[1] - r[0] >= G.native.OSD_GAP_DEFAULT
    return seed, "osd" if ok else "lost"


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 320
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()
    with multiprocessing.get_context("spawn").Pool(8) as pool:
        res = pool.map(classify, range(first, first + count), chunksize=8)
    for kind in ("osd", "lost", "fano", "none"):
        print(kind, [s for s, k in res if k == kind][:40])
