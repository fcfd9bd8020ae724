"""The line `bench.py` prints is a contract with the driver (one JSON object on stdout, rank 0): the keys it reads, their
types, and what this round added (the spot check, the trial scalars).  A short run with the driver's own flag set; the
legs beside the headline (roofline, CPU baseline, spot check) need --full."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_bench_line_has_the_contract_keys():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "UWSPR_OPTIONS"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                        "--no-sweep", "--no-lazy", "--no-host-legs", "--trial-steps", "12", "--full"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]                      # ONE line on stdout
    d = json.loads(lines[0])
    assert d["metric"].startswith("2-min WSPR frames decoded/sec") and d["unit"] == "frames/s"
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic"
    assert isinstance(d["value"], float) and d["value"] > 0
    assert abs(d["value"] - 256 * 6 / (d["ms_per_step"] * 1e-3 * 6)) < 1e-6 * d["value"]      # value = frames / time
    cfg = d["config"]
    assert "configs[1]" in cfg["workload"] and "model" not in cfg and cfg["frames_per_gpu"] == 256
    rf = d["roofline"]
    assert rf["bound"] == "valu_fp32_nofma" and rf["unit"] == "Top/s" and rf["peak"] == 78.6
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0.2 < rf["frac"] < 1.0
    assert "traffic" in rf and rf["kernel_ms_per_step"] > 0 and rf["launches_per_step"] >= 1
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "frames/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    sc = d["parity_spot_check"]
    assert sc["equal"] is True and sc["frames"] == 8 and sc["mismatches"] == []
    # the (form, streams) trial: its table and the choice as top-level scalars, its length independent of --steps
    assert d["trial_steps"] == 12 and d["chosen_sched"] in ("staged", "fused") and d["chosen_streams"] in (1, 2, 3)
    for f in ("staged", "fused"):
        for n in (1, 2, 3):
            assert d["trial_%s_x%d_ms" % (f, n)] > 0
    best = min(d["trial_%s_x%d_ms" % (f, n)] for f in ("staged", "fused") for n in (1, 2, 3))
    assert d["trial_%s_x%d_ms" % (d["chosen_sched"], d["chosen_streams"])] <= 1.02 * best


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps once and carries the headline keys only; --dump-outputs writes
    what its last timed step computed, and that is what the library computes on the same seeded batch."""
    import numpy as np
    import torch
    import gr_uwspr_amd as G
    from gr_uwspr_amd import dist as D
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "UWSPR_OPTIONS"):
        env.pop(k, None)
    out_dir = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", out_dir], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:3]
    d = json.loads(lines[0])
    assert d["metric"].startswith("2-min WSPR frames decoded/sec") and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 2
    assert d["repeats"]["n"] == 1 and abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "kernels", "cpu_baseline", "parity_spot_check", "sweep", "configs4_n1", "lazy_s5",
              "fast_search", "end_to_end_decoded"):
        assert k not in d, k
    files = sorted(os.listdir(out_dir))
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 * 10 ** 6
    # the last timed step (i = 6) read batch 6 mod 5 of rank 0
    frames = G.synth.make_frames_torch(256, "cuda:0", seed=0xC0FFEE + 104729 * 1, snr_db=-20.0)
    ctx = G.Context(device=0, options={"sched": 0})
    try:
        cands, out = ctx.pipeline_batch(frames, max_per_frame=1)
    finally:
        ctx.close()
    def same(a, b):
        return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)
    npk = np.array([len(c) for c in cands])
    assert same(arrays["npk"], npk) and npk.sum() > 0
    for f in G.native.CAND_DTYPE.names:
        got = arrays["cand_" + f]
        for b in range(256):
            assert same(got[b, :npk[b]], cands[b][f]) and (got[b, npk[b]:] == 0).all(), (f, b)
    for f in G.native.DEMOD_DTYPE.names:
        if not f.startswith("_"):
            assert same(arrays["rec_" + f], out[:, 0][f]), f
    slab = arrays["slab"].astype(np.uint8)
    for b in (0, 101, 255):
        n, sc, f1, shift1, drift1, sync1 = D.unpack_slab(slab[b], G.native.CAND_DTYPE)
        assert n == npk[b] and sc.tobytes() == cands[b][:D.SLAB_K].tobytes()
        assert same([f1, shift1, drift1, sync1], [out[b, 0][k] for k in ("f1", "shift1", "drift1", "sync1")])
    torch.cuda.synchronize()
