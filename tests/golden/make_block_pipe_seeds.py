"""How the seeds of tests/test_gpu_block_pipe.py were picked, on the CPU: frames of that test's model (test_gpu_osd_pipe's
text_frame at the test's SNR) through the oracle's FDR + schedule, the host Fano decoder on every gated try, and the
binary64 restatement of block demodulation (tests/test_gpu_blockdemod.py) under the pipe's item rule -- the gated try with
the largest jig_sync, the first one on ties; its jig_shift, the record's f1 and drift1 (a NONLINEAR candidate: f1 +
slmFrequencyDrift at t = 0, no drift).  Prints the seeds whose strongest candidate Fano decodes on no try and whose
restated n = 2 or n = 3 vector passes the rms gate and decodes to the sent text ("block", with the block length the pipe
would report and each vector's Fano cycles per bit), those on which every vector times out ("lost"), those that decode
as always ("fano"), and the rest.  A "lost" seed is "far" from decoding when its n = 2 and n = 3 vectors also time out with
ten times the cycle limit (100 000 per bit), and at the pipe's limit in each of 16 copies in which a random 2 % of the
bytes are moved by +-1 -- ten times the share of bytes by which the kernel may differ from the restatement.

python tests/golden/make_block_pipe_seeds.py [first] [count] [snr_db]"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]


def classify(arg):
    seed, snr_db = arg
    import gr_uwspr_amd as G
    import oracle_py as O
    from test_gpu_blockdemod import block_restate, slm_at_zero
    from test_gpu_block_pipe import TEXT
    from test_gpu_osd_pipe import text_frame
    frame = text_frame(G, TEXT, seed, snr_db)
    cands = O.FDR().transform(frame)
    if not len(cands):
        return seed, "none", None
    d = O.demod_candidate(cands[0], 1500, frame)
    minrms = np.float32(52.0 * (50 / 64.0))
    g = [t for t in range(17) if d["jig_sync"][t] > np.float32(0.12) and d["jig_rms"][t] > minrms]
    if not d["worth_a_try"] or not g:
        return seed, "none", None
    if any(G.fano_decode(G.deinterleave(d["symbols"][t]))[0] == 0 for t in g):
        return seed, "fano", None
    t = max(g, key=lambda k: (d["jig_sync"][k], -k))
    f, drift = np.float32(d["f1"]), np.float32(d["drift1"])
    if int(cands[0]["m_type"]) == G.native.NONLINEAR:
        f, drift = np.float32(f + slm_at_zero(cands[0])), np.float32(0.0)
    vec = block_restate(frame, int(d["jig_shift"][t]), f, drift, G.synth.PR3)
    first, info = 0, []
    for nb in (2, 3):
        v = vec[nb - 1]
        y = (v.astype(np.float32) - np.float32(128.0))
        rms = np.float32(np.sqrt(np.float64((y * y).sum(dtype=np.float32)) / 162.0))
        if not rms > minrms:
            info.append((nb, "rms"))
            continue
        rc, msg, _, cycles = G.fano_decode(G.deinterleave(v))
        ok = rc == 0 and G.unpack_message(msg[:7].astype(np.int8)) == (0, TEXT)
        wrong = rc == 0 and not ok
        info.append((nb, "ok" if ok else ("WRONG" if wrong else "timeout"), cycles // 81))
        if ok and not first:
            first = nb
        if wrong and not first:
            return seed, "wrong", info
    far = False
    if not first:
        far = True
        rng = np.random.Generator(np.random.Philox(0xFA2 + seed))
        for nb in (2, 3):
            v = vec[nb - 1]
            if G.fano_decode(G.deinterleave(v), maxcycles=100000)[0] == 0:
                far = False
            for _ in range(16):
                step = np.where(rng.random(162) < 0.02, rng.choice([-1, 1], 162), 0)
                w = np.clip(v.astype(np.int32) + step, 0, 255).astype(np.uint8)
                if G.fano_decode(G.deinterleave(w))[0] == 0:
                    far = False
    return seed, ("block" if first else "lost"), (first, info, far)


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    import oracle_py as O
    O.build(ref=False)
    import gr_uwspr_amd as G
    G.native.build()
    from test_gpu_block_pipe import SNR_DB
    snr = float(sys.argv[3]) if len(sys.argv) > 3 else SNR_DB
    with multiprocessing.get_context("spawn").Pool(8) as pool:
        res = pool.map(classify, [(s, snr) for s in range(first, first + count)], chunksize=4)
    print("snr_db", snr, "seeds", first, "..", first + count - 1)
    for kind in ("block", "lost", "fano", "none", "wrong"):
        print(kind, len([1 for _, k, _ in res if k == kind]), [s for s, k, _ in res if k == kind][:40])
    print("lost and far from decoding", [s for s, k, info in res if k == "lost" and info[2]][:40])
    for s, k, info in res:
        if k == "block":
            print("  seed", s, "first block length", info[0], info[1])
