"""The moving-source cases that tests/test_follow.py (no GPU) and tests/test_gpu_follow.py share: the three trajectories of the receiver's own grid that profiles/moving_source.txt lists as decoding in no model at
either level -- closest point of approach in mid-transmission, a Doppler S-curve of 2 to 3.7 Hz --, rendered by
tests/track_exact.py's synth at f0 = 1 Hz from sample 375 with noise of SIGMA_M20 per component, and the follow grid: the
true pass among five separated decoys."""
import numpy as np

import track_exact as TX

TEXT = "K1ABC FN42 37"
START, F0 = 375, 1.0
QF, NL = 16, 2
# index in the receiver's grid (slm_trajectories' order) -> (V1, V2, p1, p2)
SLM = {1: (-2.0, -2.0, 0.0, 250.0), 21: (2.0, -2.0, 0.0, 250.0), 35: (0.0, -1.0, 0.0, 50.0)}
MODELS = ("doppler", "delay")
DECOYS = ((0.0, 100.0, 0.0), (1.0, 300.0, 20.0), (2.0, 150.0, 90.0), (3.5, 60.0, 30.0), (1.5, 500.0, 55.0))
# the noise seed of every case: the first one tried (seed 2 gives the same outcomes), so no seed was picked
SEED = {(k, m): 1 for k in SLM for m in MODELS}


def truth(G, k):
    """(v, d, tc) of grid trajectory k by uwspr_track_from_slm; the radial pass (d = 0) is approximated by d = 1"""
    t = G.track_from_slm(SLM[k])[0]
    return (float(t["v"]), max(float(t["d"]), 1.0), float(t["tc"]))


def grid(G, k):
    """the true pass at index 2 among the decoys"""
    rows = list(DECOYS[:2]) + [truth(G, k)] + list(DECOYS[2:])
    return G.track_trajs(rows), 2


def frame(G, k, model, seed=None):
    sym = G.wspr_symbols(TEXT)
    rng = np.random.Generator(np.random.Philox(SEED[(k, model)] if seed is None else seed))
    return TX.synth(sym, truth(G, k), model, START, f0=F0) + (TX.SIGMA_M20 * rng.standard_normal((TX.FL, 2))).astype(np.float32)
