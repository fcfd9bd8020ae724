"""tests/golden/osd_vectors.npz: soft-symbol vectors for tests/test_gpu_osd.py, found on the CPU with the host
uwspr_fano_decode and the numpy restatement of ordered-statistics decoding.

signal  [20, 162] uint8: noisy encodings, clip(round(128 +- amp + sigma N(0, 1))), of packed messages for which Fano
        returns -1 and restated order 2 returns the transmitted message with dnext - dmin >= UWSPR_OSD_GAP_DEFAULT:
        8 won with two flips, 8 with one, 4 with none
message [20, 7] int8, nflip [20], text [20]
noise   [20, 162] uint8: clip(round(128 + sigma N(0, 1)))
gap     the default gap the signal vectors were chosen against

python tests/golden/make_osd_vectors.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gr_uwspr_amd as G   # noqa: E402
from test_gpu_osd import NSYM, SRC, conv_encode, osd_restate   # noqa: E402

WANT = {2: 8, 1: 8, 0: 4}
LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def random_text(rng):
    call = "".join(rng.choice(list(LETTERS), 2)) + str(rng.integers(0, 10)) + "".join(rng.choice(list(LETTERS), 3))
    grid = "".join(rng.choice(list(LETTERS[:18]), 2)) + "%02d" % rng.integers(0, 100)
    return "%s %s %d" % (call, grid, rng.choice([0, 3, 7, 10, 13, 17, 20, 23, 27, 30, 33, 37]))


def main():
    gap = G.native.OSD_GAP_DEFAULT
    rng = np.random.default_rng(20261018)
    got = {0: [], 1: [], 2: []}
    trials = 0
    while any(len(got[k]) < WANT[k] for k in WANT):
        trials += 1
        text = random_text(rng)
        msg = G.wspr_pack(text)
        bits = np.zeros(81, np.uint8)
        bits[:56] = np.unpackbits(msg.view(np.uint8))
        c = conv_encode(bits)
        amp, sigma = rng.choice([24.0, 27.0, 30.0, 34.0]), rng.choice([28.0, 32.0, 36.0])
        de = np.clip(np.rint(128 + amp * (2.0 * c - 1) + sigma * rng.standard_normal(NSYM)), 0, 255).astype(np.uint8)
        sym = np.zeros(NSYM, np.uint8)
        sym[SRC] = de
        if G.fano_decode(G.deinterleave(sym))[0] != -1:
            continue
        d = osd_restate(sym, 2)
        if d[4].tobytes() != msg.tobytes() or d[1] - d[0] < gap or len(got[d[3]]) >= WANT[d[3]]:
            continue
        got[d[3]].append((sym, msg, d[3], text))
        print("trial %d: %d flips, gap %d, %s (amp %g sigma %g); have %s" % (trials, d[3], d[1] - d[0], text, amp, sigma,
                                                                          {k: len(v) for k, v in got.items()}), flush=True)
    rows = got[2] + got[1] + got[0]
    noise = np.clip(np.rint(128 + 32.0 * rng.standard_normal((len(rows), NSYM))), 0, 255).astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "osd_vectors.npz"), signal=np.stack([r[0] for r in rows]),
                        message=np.stack([r[1] for r in rows]), nflip=np.array([r[2] for r in rows], np.uint8),
                        text=np.array([r[3] for r in rows]), noise=noise, gap=np.int32(gap))


if __name__ == "__main__":
    main()
