"""How the seeds of tests/test_gpu_deep_pipe.py were picked, on the CPU: frames of that test's model (text_frame of
tests/test_gpu_osd_pipe.py, at -31 dB) through the oracle's FDR + schedule, the host Fano decoder on every gated try, and the
numpy restatement of the list search (tests/deep_exact.py) under the pipe's item rule, against that test's list of 1024
messages of which TEXT is one.  Prints the seeds whose strongest candidate Fano decodes on no try and the restatement
accepts as TEXT at the default thresholds, while the same list without TEXT is not accepted ("deep"); those neither list
is accepted for ("lost"); and those Fano decodes ("fano").

python tests/golden/make_deep_pipe_seeds.py [first] [count]"""
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
    import deep_exact as X
    from test_gpu_deep_pipe import SNR_DB, TEXT, TEXT_AT, known_list
    from test_gpu_osd_pipe import text_frame
    N = G.native
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
    msgs = known_list(G)
    tab = X.code_table(G, msgs)
    r = X.deep_restate(tab, d["symbols"][t])[0]
    rm = X.deep_restate(np.delete(tab, TEXT_AT, axis=0), d["symbols"][t])[0]
    if X.accepted(rm, len(msgs) - 1, N.DEEP_MIN_DEFAULT, N.DEEP_GAP_DEFAULT):
        return seed, "wrong"
    ok = int(r["best"]) == TEXT_AT and X.accepted(r, len(msgs), N.DEEP_MIN_DEFAULT, N.DEEP_GAP_DEFAULT)
    return seed, "deep" if ok else "lost"


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()
    with multiprocessing.get_context("spawn").Pool(8) as pool:
        res = pool.map(classify, range(first, first + count), chunksize=4)
    for kind in ("deep", "lost", "fano", "wrong", "none"):
        print(kind, [s for s, k in res if k == kind][:40])
