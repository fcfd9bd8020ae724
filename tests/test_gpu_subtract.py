"""K8, known-symbol subtraction (uwspr_subtract_batch, the pipe's second pass) on the device.

The reference has no subtraction, so the definitions of include/uwspr_hip.h are restated here in numpy binary64
(refine_ref, cancel_ref) and the kernels are held to that.

The scenario (one frame per case, default_rng(1000 + case), cases 0..5): transmission A at f_A in U(-3, 3) Hz with unit
amplitude, another message B at f_A + 0.3 Hz and 12 dB weaker, both starting at 375 +- 100 samples with random phases,
AWGN of synth.sigma_for_snr(-12).  Alone B would decode; under A a single search never sees it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, FL, NSYM, SPB = 375.0, 45000, 162, 256
N = NSYM * SPB
DF = FS / SPB
HOP = 3375
# max |GPU - restatement| / max |x| of the cancel test, measured on an MI355X: CANCEL_MEASURED (profiles/subtract.txt).
# The bytes are deterministic; the factor 4 is room for another compiler's instruction order in the 1023-term binary32
# sums, and the bound stays under the issue's ceiling of 1e-4.
CANCEL_MEASURED = 6.879e-07
CANCEL_BOUND = 4 * CANCEL_MEASURED
assert CANCEL_BOUND <= 1e-4


# ---- the restatement (binary64) --------------------------------------------------------------------------------------
def f_sym(f, drift, sym):
    i = np.arange(NSYM, dtype=np.float64)
    return np.float64(f) + (np.float64(drift) / 2.0) * (i - 81.0) / 81.0 + (np.asarray(sym, np.float64) - 1.5) * DF


def refine_ref(x, sym, f, shift, drift):
    """M[q + 4, l + 24] of the header, x complex128 [fl]."""
    fi = f_sym(f, drift, sym)
    pad = 1 << 16
    xp = np.zeros(len(x) + 2 * pad, np.complex128)
    xp[pad:pad + len(x)] = x
    seg = np.stack([xp[pad + shift - 24 + SPB * i: pad + shift - 24 + SPB * i + SPB + 48] for i in range(NSYM)])
    W = np.lib.stride_tricks.sliding_window_view(seg, SPB, axis=1)      # [162, 49, 256]
    k = np.arange(SPB, dtype=np.float64)
    M = np.zeros((9, 49))
    for q in range(-4, 5):
        ph = np.exp(-2j * np.pi * (fi[:, None] + 0.0125 * q) * k[None, :] / FS)
        M[q + 4] = np.abs(np.einsum("ilk,ik->il", W, ph)).sum(axis=0)
    return M


def first_max(M):
    h = int(np.argmax(M.reshape(-1)))   # (numpy returns the first maximum; rows are q, columns l)
    return h // 49 - 4, h % 49 - 24


def cancel_ref(x, sym, f, shift, drift, reduced=False):
    """-> (frame with the item taken out, removed), x complex128 [fl]; f, drift as the binary32 values of the call.
    reduced: the phase from per-symbol prefix sums taken mod 1 turn (tests/test_gpu_subtract_edges.py: at |f| = 1e4 Hz the
    running sum over 41472 samples reaches 1e6 turns and loses what this form keeps -- good to 1e-9 turns)"""
    if reduced:
        w = f_sym(f, drift, sym) / FS                      # turns per sample
        ph = np.zeros(NSYM)
        for i in range(1, NSYM):
            ph[i] = (ph[i - 1] + SPB * w[i - 1]) % 1.0
        theta = 2.0 * np.pi * ((ph[:, None] + np.arange(SPB, dtype=np.float64)[None, :] * w[:, None]) % 1.0).reshape(N)
    else:
        fi = np.repeat(f_sym(f, drift, sym), SPB)
        theta = 2.0 * np.pi * np.concatenate(([0.0], np.cumsum(fi / FS)[:-1]))
    r = np.exp(1j * theta)
    idx = shift + np.arange(N)
    ok = (idx >= 0) & (idx < len(x))
    c = np.zeros(N, np.complex128)
    c[ok] = x[idx[ok]] * np.conj(r[ok])
    w = np.hanning(1025)[1:-1]
    a = np.zeros(N, np.complex128)
    a[ok] = (np.convolve(c, w, mode="same") / np.maximum(np.convolve(ok.astype(np.float64), w, mode="same"), 1e-300))[ok]
    out = x.copy()
    out[idx[ok]] -= (a * r)[ok]
    return out, float(np.sum(np.abs((a * r)[ok]) ** 2))


def to_c(frame):
    return frame[..., 0].astype(np.float64) + 1j * frame[..., 1].astype(np.float64)


def add_signal(sig, sym, f, start, phase, amp, drift=0.0):
    """amp e^{j (phase + theta)} of the item model (f, start, drift) added to complex128 sig, clipped to it"""
    fi = np.repeat(f_sym(f, drift, sym), SPB)
    theta = phase + 2.0 * np.pi * np.concatenate(([0.0], np.cumsum(fi / FS)[:-1]))
    idx = start + np.arange(N)
    ok = (idx >= 0) & (idx < len(sig))
    sig[idx[ok]] += amp * np.exp(1j * theta[ok])


def to_frame(sig):
    return np.stack([sig.real, sig.imag], axis=-1).astype(np.float32)


def message_of(bits50):
    return np.packbits(np.concatenate([bits50, np.zeros(6, np.uint8)]).astype(np.uint8)).astype(np.int8)


def item(frame, shift, f, sym, drift=0.0):
    return {"frame": frame, "shift": shift, "f": f, "drift": drift, "symbols": sym}


def model_of(G, cand, rec):
    """(f, drift) the fine search correlated a record with: (f1, drift1) of a LINEAR candidate; a NONLINEAR one has the
    constant f1 + slmFrequencyDrift(t = 0) and no drift (the pipe's second pass forms its items the same way)"""
    if int(cand["m_type"]) == G.native.NONLINEAR:
        slm = np.float32(G.slm_drift((cand["V1"], cand["V2"], cand["p1"], cand["p2"]), 0.0))
        return float(np.float32(rec["f1"]) + slm), 0.0
    return float(rec["f1"]), float(rec["drift1"])


# ---- shared inputs, made once -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(G):
    c = G.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenario(G):
    """the six frames: dict of frames [6, fl, 2], and per case the messages, symbols and true (f, start) of A and B"""
    S = G.synth
    frames = np.zeros((6, FL, 2), np.float32)
    meta = []
    for case in range(6):
        rng = np.random.default_rng(1000 + case)
        bits = rng.integers(0, 2, size=(2, 50)).astype(np.uint8)
        sym = S.encode_messages(bits)
        fa = rng.uniform(-3.0, 3.0)
        start = rng.integers(375 - 100, 375 + 101, size=2)
        phase = rng.uniform(0.0, 2.0 * np.pi, size=2)
        sig = np.zeros(FL, np.complex128)
        add_signal(sig, sym[0], fa, int(start[0]), phase[0], 1.0)
        add_signal(sig, sym[1], fa + 0.3, int(start[1]), phase[1], 10.0 ** (-12.0 / 20.0))
        noise = S.sigma_for_snr(-12.0) * rng.standard_normal((FL, 2))
        frames[case] = (np.stack([sig.real, sig.imag], axis=-1) + noise).astype(np.float32)
        msg = [message_of(bits[0]), message_of(bits[1])]
        for m, s in zip(msg, sym):   # (the library's encoder and the generator's agree on what these bytes transmit)
            assert np.array_equal(G.wspr_symbols(m), s)
        meta.append({"msg": msg, "sym": sym, "f": (fa, fa + 0.3), "start": start})
    return {"frames": frames, "meta": meta}


def make_cancel_case(G):
    """B = 3 frames, 4 items: frame 0 an item clipped at the frame's start (shift -40, with drift) and a second one under it
    (order matters), frame 1 nothing, frame 2 an item clipped at the end (shift fl - N + 300) and one more"""
    rng = np.random.default_rng(77)
    sym = G.synth.encode_messages(rng.integers(0, 2, size=(4, 50)))
    spec = [(0, -40, 1.30, 0.5), (0, 380, 1.75, 0.0), (2, FL - N + 300, -2.40, 0.0), (2, 300, -2.05, -0.3)]
    sig = np.zeros((3, FL), np.complex128)
    for (b, sh, f, dr), s, amp in zip(spec, sym, (1.0, 0.4, 0.8, 0.5)):
        add_signal(sig[b], s, f + 0.004, sh + 1, rng.uniform(0, 2 * np.pi), amp, dr)   # (a model that is slightly off)
    sig += 0.5 * (rng.standard_normal((3, FL)) + 1j * rng.standard_normal((3, FL)))
    frames = to_frame(sig)
    items = [item(b, sh, f, s, dr) for (b, sh, f, dr), s in zip(spec, sym)]
    ref = to_c(frames)
    removed = []
    for it in G.sub_items(items):
        ref[it["frame"]], rm = cancel_ref(ref[it["frame"]], it["symbols"], it["f_hz"], int(it["shift"]), it["drift_hz"])
        removed.append(rm)
    return {"frames": frames, "items": items, "ref": ref, "removed": removed}


@pytest.fixture(scope="module")
def cancel_case(G):
    return make_cancel_case(G)


# ---- cancel -------------------------------------------------------------------------------------------------------------
def test_cancel_matches_the_restatement(G, ctx, cancel_case):
    import torch
    frames, items = cancel_case["frames"], cancel_case["items"]
    out, res = ctx.subtract(frames, items, refine=False)
    err = np.max(np.abs(to_c(out) - cancel_case["ref"])) / np.max(np.abs(to_c(frames)))
    print("cancel: max |GPU - restatement| / max |x| = %.3e (bound %.3e)" % (err, CANCEL_BOUND))
    assert err <= CANCEL_BOUND
    assert out[1].tobytes() == frames[1].tobytes()                       # the frame without items: copied bytes
    assert not np.array_equal(out[0], frames[0]) and not np.array_equal(out[2], frames[2])
    # two items in one frame: the second is fitted on what the first left -- the other order gives other bytes
    swapped, _ = ctx.subtract(frames, [items[1], items[0]] + items[2:], refine=False)
    assert swapped[0].tobytes() != out[0].tobytes() and swapped[2].tobytes() == out[2].tobytes()
    it = G.sub_items(items)
    assert np.array_equal(res["f_hz"], it["f_hz"]) and np.array_equal(res["shift"], it["shift"]) and not res["metric"].any()
    # removed = sum |a r|^2: a binary32 sum of <= 41472 terms in blocks of 8 / 64 / 9 / 9, terms good to the bound above
    assert np.allclose(res["removed"], cancel_case["removed"], rtol=1e-4, atol=0.0), (res["removed"], cancel_case["removed"])
    # device pointers: the same bytes, results included; and in place
    dev = torch.from_numpy(frames).to("cuda:0")
    dout, dres = ctx.subtract(dev, items, refine=False)
    assert dout.cpu().numpy().tobytes() == out.tobytes() and dres.tobytes() == res.tobytes()
    assert dev.cpu().numpy().tobytes() == frames.tobytes()
    same, _ = ctx.subtract(dev, items, refine=False, out=dev)
    assert same.data_ptr() == dev.data_ptr() and dev.cpu().numpy().tobytes() == out.tobytes()


def test_strided_input_equals_contiguous_input(G, ctx):
    """frames in place in a stretch of stream at hop 3375 (uwspr_set_frame_stride) against the same frames cut out"""
    rng = np.random.default_rng(78)
    sym = G.synth.encode_messages(rng.integers(0, 2, size=(2, 50)))
    sig = 0.5 * (rng.standard_normal(2 * HOP + FL) + 1j * rng.standard_normal(2 * HOP + FL))
    add_signal(sig, sym[0], 0.8, 375, 0.3, 1.0)
    add_signal(sig, sym[1], -1.1, 2 * HOP + 200, 1.3, 0.7)
    stream = to_frame(sig)
    cut = np.stack([stream[b * HOP: b * HOP + FL] for b in range(3)])
    items = [item(0, 375, 0.8, sym[0]), item(1, 375 - HOP, 0.8, sym[0]), item(2, 200, -1.1, sym[1])]
    want, wres = ctx.subtract(cut, items, refine=True)
    ctx.set_frame_stride(HOP)
    try:
        got, gres = ctx.subtract(G.FrameView(3, host=stream), items, refine=True)
    finally:
        ctx.set_frame_stride(0)
    assert got.tobytes() == want.tobytes() and gres.tobytes() == wres.tobytes()
    assert np.array_equal(stream, to_frame(sig))    # the stream is read, never written


# ---- refine -------------------------------------------------------------------------------------------------------------
def test_refine_returns_the_restatements_maximum(G, ctx, scenario):
    """A's (f1, shift1) as the receiver estimates them, pushed off by +13 samples and +0.03 Hz: the kernel returns the
    (q, l) of the restatement.  Where the restatement's two best M differ by < 1e-5 relative either is accepted; the
    number of cases that needed it is printed and must be <= 1 of 6."""
    frames, meta = scenario["frames"], scenario["meta"]
    cands, out = ctx.pipeline_batch(frames, max_per_frame=1)
    items = []
    for b in range(6):
        o = out[b, 0]
        assert len(cands[b]) > 0
        f1, drift1 = model_of(G, cands[b][0], o)
        assert abs(f1 - meta[b]["f"][0]) < 0.2 and abs(int(o["shift1"]) - int(meta[b]["start"][0])) < 40
        items.append(item(b, int(o["shift1"]) + 13, float(np.float32(f1) + np.float32(0.03)), meta[b]["sym"][0], drift1))
    it = G.sub_items(items)
    res_frames, res = ctx.subtract(frames, items, refine=True)
    allowed = 0
    for b in range(6):
        M = refine_ref(to_c(frames[b]), it[b]["symbols"], it[b]["f_hz"], int(it[b]["shift"]), it[b]["drift_hz"])
        q, l = first_max(M)
        got_q = int(round((float(res[b]["f_hz"]) - float(it[b]["f_hz"])) / 0.0125))
        got_l = int(res[b]["shift"]) - int(it[b]["shift"])
        top = np.sort(M.reshape(-1))[::-1]
        print("refine case %d: restatement (q, l) = (%d, %d), M %.6f, runner-up %.3e below; GPU (%d, %d), M %.6f"
              % (b, q, l, top[0], (top[0] - top[1]) / top[0], got_q, got_l, float(res[b]["metric"])))
        assert -4 <= got_q <= 4 and -24 <= got_l <= 24
        assert res[b]["f_hz"] == np.float32(np.float64(it[b]["f_hz"]) + 0.0125 * got_q)
        if (got_q, got_l) != (q, l):
            assert (top[0] - top[1]) < 1e-5 * top[0] and M[got_q + 4, got_l + 24] == top[1], (b, (q, l), (got_q, got_l))
            allowed += 1
        assert abs(float(res[b]["metric"]) - M[got_q + 4, got_l + 24]) <= 1e-5 * M[got_q + 4, got_l + 24]
        print("    refined shift %d, f %.4f; transmitted start %d, f %.4f" % (int(res[b]["shift"]), float(res[b]["f_hz"]), int(meta[b]["start"][0]), meta[b]["f"][0]))
    print("refine: %d of 6 cases used the near-tie allowance" % allowed)
    assert allowed <= 1
    # a call without refinement on the refined values removes what the refining call removed
    again = [item(b, int(res[b]["shift"]), float(res[b]["f_hz"]), meta[b]["sym"][0], float(it[b]["drift_hz"])) for b in range(6)]
    plain, _ = ctx.subtract(frames, again, refine=False)
    assert plain.tobytes() == res_frames.tobytes()


# ---- the point of the feature ---------------------------------------------------------------------------------------------
def run_pipe(G, frames, passes):
    import torch
    dev = torch.from_numpy(frames).to("cuda:0")
    torch.cuda.synchronize()
    pipe = G.Pipe(batch_frames=8, max_per_frame=2, lanes=2, passes=passes)
    try:
        pipe.submit_device(dev)
        pipe.flush()
        return pipe.collect(), pipe.stats()
    finally:
        pipe.close()


def test_second_pass_decodes_the_signal_under_the_decoded_one(G, scenario):
    frames, meta = scenario["frames"], scenario["meta"]
    one, st1 = run_pipe(G, frames, 1)
    two, st2 = run_pipe(G, frames, 2)
    assert not one["pass"].any()
    for b in range(6):   # one pass: exactly the A messages
        got = {bytes(r["message"]) for r in one[(one["frame"] == b) & (one["decoded"] == 1)]}
        assert got == {bytes(meta[b]["msg"][0])}, (b, got)
    # The receiver takes some of these A's as NONLINEAR candidates (a straight-line trajectory whose Doppler at t = 0 is a
    # whole Hz: f1 is then that far from the tone the fine search correlated with).  Those frames are where the item's
    # frequency has to be f1 + slmFrequencyDrift(t = 0): with f1 alone the fit misses A by 1 Hz and B stays buried.
    nonlinear = {int(r["frame"]) for r in one if r["decoded"] and int(r["coarse"]["m_type"]) == G.native.NONLINEAR
                 and abs(float(r["f1"]) - meta[int(r["frame"])]["f"][0]) > 0.5}
    print("first pass: A decoded through a NONLINEAR candidate with f1 off the tone in frames", sorted(nonlinear))
    assert nonlinear, "the scenario no longer exercises the nonlinear item model"
    first = two[two["pass"] == 0]
    assert first.tobytes() == one.tobytes()           # the first-pass records: byte for byte
    found = 0
    for b in range(6):
        recs = two[two["frame"] == b]
        k = int((recs["pass"] == 0).sum())
        assert not recs["pass"][:k].any() and recs["pass"][k:].all()        # directly behind the frame's first-pass records
        extra = recs[k:]
        assert extra["decoded"].all() and extra["cand"].tolist() == list(range(k, k + len(extra)))
        assert (extra["npk"] == recs["npk"][0]).all()
        msgs = [bytes(m) for m in extra["message"]]
        assert all(m == bytes(meta[b]["msg"][1]) for m in msgs), (b, msgs)   # nothing but A or B anywhere
        assert len(msgs) <= 1                                                # a new message is emitted once
        found += bool(msgs)
        if b in nonlinear:
            print("    frame %d (nonlinear A): B %s" % (b, "decoded" if msgs else "missed"))
    print("second pass: B decoded in %d of 6 frames" % found)
    assert any(len(two[(two["frame"] == b) & (two["pass"] == 1)]) for b in nonlinear)   # the nonlinear model works
    assert found >= 5
    assert np.array_equal(np.sort(two["frame"]), two["frame"])              # frame order stays
    assert st2["frames"] == st1["frames"] == 6 and st2["decoded"] == st1["decoded"] + int((two["pass"] == 1).sum())


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_anything_is_written(G, ctx, cancel_case):
    import torch
    frames, items = cancel_case["frames"], cancel_case["items"]
    out = np.full((3, FL, 2), 7.0, np.float32)
    with pytest.raises(G.UwsprError) as e:                       # unsorted
        ctx.subtract(frames, [items[2], items[0]], refine=False, out=out)
    assert e.value.status == -6 and (out == 7.0).all()
    bad = G.sub_items(items).copy()
    bad[3]["symbols"][161] = 4
    with pytest.raises(G.UwsprError) as e:                       # a symbol > 3
        ctx.subtract(frames, bad, refine=True, out=out)
    assert e.value.status == -6 and (out == 7.0).all()
    bad = G.sub_items(items).copy()
    bad[3]["frame"] = 3
    with pytest.raises(G.UwsprError) as e:                       # a frame outside [0, B)
        ctx.subtract(frames, bad, refine=True, out=out)
    assert e.value.status == -6 and (out == 7.0).all()
    # in place over frames that overlap in memory
    stream = torch.from_numpy(np.random.default_rng(5).standard_normal((3 * FL, 2)).astype(np.float32)).to("cuda:0")
    before = stream.cpu().numpy().tobytes()
    ctx.set_frame_stride(HOP)
    try:
        with pytest.raises(G.UwsprError) as e:
            ctx.subtract(G.FrameView(3, ptr=stream.data_ptr()), items, refine=False, out=stream)
    finally:
        ctx.set_frame_stride(0)
    assert e.value.status == -6 and stream.cpu().numpy().tobytes() == before
    with pytest.raises(G.UwsprError) as e:
        G.Pipe(batch_frames=4, lanes=1, passes=3)
    assert e.value.status == -6
    pipe = G.Pipe(batch_frames=4, lanes=1)
    try:
        with pytest.raises(G.UwsprError) as e:
            pipe.set_option("passes", 0)
        assert e.value.status == -6
        pipe.set_option("passes", 2)
        pipe.set_option("passes", 1)
    finally:
        pipe.close()
