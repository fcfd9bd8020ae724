#!/usr/bin/env python3
"""Writes tests/golden/live_ref.npz: what the REAL reference objects (oracle/_ref, built by oracle/Makefile `ref`
where the reference sources are) return on the inputs of the three "live reference" tests, so that those tests run
against the stored answers where oracle/_ref cannot be built.  DATA only; the inputs are re-derived by the tests from
the same seeds, in the same order:

  slm_out         test_oracle_pins.test_slm_against_live_reference: lib/slm.cc on 2000 seeded (V1, V2, p1, p2, t)
  ve3emb_*        test_oracle_pins.test_ve3emb_decodes_through_real_reference_fano: lib/Fano.cc on the 17
                  deinterleaved soft-symbol vectors of the oracle's top VE3EMB candidate (inputs stored too), and
                  lib/helpers.cc unpk_ on the message it decoded
  fano_*          test_host_tail.test_fano_against_live_reference: lib/Fano.cc on 12 seeded noisy encodings
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle_py as O  # noqa: E402
import gr_uwspr_amd as G  # noqa: E402


def main():
    O.build(ref=True)
    R = O.ref()
    assert R is not None, "oracle/_ref not built: run where the reference sources are"
    out = {}
    rng = np.random.default_rng(3)
    slm = np.zeros(2000, np.float32)
    for i in range(2000):
        V1, V2 = rng.uniform(-3, 3, 2)
        p1, p2 = int(rng.integers(-50, 50)), int(rng.integers(0, 900))
        t = float(rng.integers(0, 120))
        slm[i] = np.float32(R.ref_slm_frequency_drift(V1, V2, p1, p2, 1500.0, t))
    out["slm_out"] = slm

    ve = O.read_c2(os.path.join(HERE, "VE3EMB.c2"))
    c = O.FDR().transform(ve)[0]
    d = O.demod_candidate(c, 1500, ve)
    syms = np.array([O.deinterleave(d["symbols"][idt]) for idt in range(17)], np.uint8)
    res = [O.ref_fano_decode(s) for s in syms]
    out["ve3emb_symbols"] = syms
    out["ve3emb_rc"] = np.array([r[0] for r in res], np.int32)
    out["ve3emb_data"] = np.array([r[1] for r in res], np.uint8)
    idt = next(i for i in range(17) if d["jig_sync"][i] > 0.12 and d["jig_rms"][i] > 40.625 and res[i][0] == 0)
    out["ve3emb_message"] = np.array(O.ref_unpk([int(x) - 256 if x > 127 else int(x) for x in res[idt][1][:7]]))

    rng = np.random.default_rng(11)
    soft_all, res = [], []
    for k in range(12):
        bits = rng.integers(0, 2, 50).astype(np.uint8)
        data = np.zeros(11, np.uint8)
        data[:7] = np.packbits(np.concatenate([bits, np.zeros(6, np.uint8)]))
        enc = G.fano_encode(data)[:162].astype(np.float64)
        soft = np.clip(128 + 40 * (2 * enc - 1) + (20 + 6 * k) * rng.standard_normal(162), 0, 255).astype(np.uint8)
        soft_all.append(soft)
        res.append(O.ref_fano_decode(soft))
    out["fano_soft"] = np.array(soft_all, np.uint8)
    out["fano_rc"] = np.array([r[0] for r in res], np.int32)
    out["fano_data"] = np.array([r[1] for r in res], np.uint8)
    out["fano_metric"] = np.array([r[2] for r in res], np.int64)
    out["fano_cycles"] = np.array([r[3] for r in res], np.int64)
    np.savez_compressed(os.path.join(HERE, "live_ref.npz"), **out)
    print("wrote", os.path.join(HERE, "live_ref.npz"))


if __name__ == "__main__":
    main()
