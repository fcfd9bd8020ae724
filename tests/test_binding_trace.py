"""The Python binding issues the C calls it always issued.

native._lib is replaced by a stub whose every function records (name, arguments) and returns 0 -- no library, no
device.  Every Context / Pipe method that has a host (numpy) form and every module-level function is then driven with
small fixed inputs, and the trace -- the calls in order, and the type, dtype and shape of what each method returned --
must equal tests/test_binding_trace.json.  That file was written by this file run as a script
(`python tests/test_binding_trace.py --write`) on the binding as it stood before its idioms were folded; the file uses
the public API only, so it runs unchanged on either.

Arguments are normalised: ints, floats and bytes by value; None as "None"; a c_void_p as "null" / "ptr"; a byref() as
what it points to; structures by their fields (pointer fields as "null" / "ptr"); other ctypes objects by type name.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

FIXTURE = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
RETURNS = {"uwspr_debug_tx_taps": 3179, "uwspr_tx_design_at": 3179, "uwspr_debug_launch_forms": 20,
           "uwspr_frontend_rotator": 375, "uwspr_frontend_design_at": 8, "uwspr_resample_design": 8,
           "uwspr_tx_fade_design": 4}
INFO = {"n": 4, "band_w": 3, "finpb": 5, "cell_hyps": 2}   # what uwspr_get_info leaves in the stub's contexts


def norm(a):
    if a is None:
        return "None"
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, (float, np.floating)):
        return float(a)
    if isinstance(a, bytes):
        return a.decode("latin-1")
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else "null"
    if type(a).__name__ == "CArgObject":                 # byref(x)
        return {"byref": norm(a._obj)}
    if isinstance(a, C.Structure):
        out = {}
        for k, t in a._fields_:
            v = getattr(a, k)
            out[k] = ("ptr" if v else "null") if t is C.c_void_p else norm(v)
        return {type(a).__name__: out}
    if isinstance(a, C.Array):
        if issubclass(a._type_, C.Structure) or a._type_ is C.c_char_p:
            return [norm(v) for v in a]
        return type(a).__name__
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, norm(a.value)]
    return type(a).__name__


def shape_of(r):
    if isinstance(r, np.ndarray):
        return ["ndarray", str(r.dtype), list(r.shape)]
    if isinstance(r, tuple):
        return ["tuple"] + [shape_of(v) for v in r]
    if isinstance(r, list):
        return ["list"] + [shape_of(v) for v in r]
    if isinstance(r, dict):
        return ["dict", {str(k): shape_of(v) for k, v in r.items()}]
    if r is None or isinstance(r, (bool, int, float, str, np.integer, np.floating)):
        return norm(r) if not isinstance(r, str) else r
    return type(r).__name__


class Stub:
    def __init__(self):
        self.trace = []
        self._page = (C.c_uint8 * 65536)()               # where uwspr_pipe_acquire / uwspr_host_alloc point

    def __getattr__(self, name):
        if not name.startswith("uwspr_"):
            raise AttributeError(name)

        def f(*args):
            self.trace.append(["call", name, [norm(a) for a in args]])
            if name == "uwspr_get_info":
                for k, v in INFO.items():
                    setattr(args[1]._obj, k, v)
            if name in ("uwspr_pipe_acquire", "uwspr_host_alloc"):
                args[-1]._obj.value = C.addressof(self._page)
            if name.endswith("_last_error") or name == "uwspr_status_string":
                return b""
            return RETURNS.get(name, 0)
        self.__dict__[name] = f                          # one function object per name (callers may set attributes on it)
        return f


def drive(G, tmp):
    """-> the trace of one fixed tour through the binding"""
    N, X = G.native, G.context
    stub = Stub()
    saved, N._lib = N._lib, stub
    T = stub.trace

    def do(label, fn, *a, **kw):
        T.append(["enter", label])
        T.append(["return", label, shape_of(fn(*a, **kw))])
    try:
        rng = np.random.default_rng(7)
        FL = 64
        frames = rng.standard_normal((2, FL, 2)).astype(np.float32)
        sym3 = rng.integers(0, 256, (3, 162)).astype(np.uint8)
        a48 = (1000 * rng.standard_normal(4800)).astype(np.int16)
        ctx = None

        def make():
            nonlocal ctx
            ctx = G.Context(fl=FL, maxfreqs=4, options={"sched": 0})
        do("Context", make)
        do("set_option", ctx.set_option, "reuse", 1)
        do("get_option", ctx.get_option, "reuse")
        do("set_stream", ctx.set_stream, 0)
        do("synchronize", ctx.synchronize)
        do("launch_forms", ctx.launch_forms)
        do("frontend 1-D", ctx.frontend, np.zeros(640, np.float32))
        do("frontend 2-D", ctx.frontend, np.zeros((2, 640), np.float64))
        do("resample s16", ctx.resample, a48, 48000)
        do("resample f32 [n, 2]", ctx.resample, np.zeros((441, 2), np.float32), 44100, nout=100)
        do("blank f32 [n, 2]", ctx.blank, np.zeros((5000, 2), np.float32))
        do("blank s16", ctx.blank, a48, blank=16, guard=3)
        do("stream_blank_stats", ctx.stream_blank_stats, 2)
        do("fdr_batch", ctx.fdr_batch, frames)
        do("fdr_batch FrameView", ctx.fdr_batch, G.FrameView(2, host=frames))
        do("fdr_from_ps", ctx.fdr_from_ps, np.zeros((2, INFO["n"], INFO["band_w"]), np.float32))
        do("fdr_spectrum", ctx.fdr_spectrum, 2)
        do("keep_syncgrid", ctx.keep_syncgrid, 3)
        do("fdr_syncgrid", ctx.fdr_syncgrid, 2)
        hyps = np.zeros(5, N.HYP_DTYPE)
        do("sync_sweep soft", ctx.sync_sweep, frames, hyps)
        do("sync_sweep sync only", ctx.sync_sweep, frames, hyps, soft=False)
        cent = np.zeros(2, N.CAND_DTYPE)
        do("sync_grid", ctx.sync_grid, frames, cent, [0.0, 0.5], [0.0], [-1, 0, 1])
        do("sync_grid sync only", ctx.sync_grid, frames, cent, [0.0], [0.0, 1.0], [0], soft=False)
        do("sync_and_demodulate", ctx.sync_and_demodulate, frames, np.zeros(3, N.CALL_DTYPE))
        do("demod_batch", ctx.demod_batch, frames, [np.zeros(2, N.CAND_DTYPE), np.zeros(1, N.CAND_DTYPE)], max_per_frame=2)
        do("stream_open", ctx.stream_open, hop=16, max_frames=8)
        do("stream_push", ctx.stream_push, np.zeros((100, 2), np.float32))
        do("stream_push_audio f32", ctx.stream_push_audio, np.zeros(320, np.float32))
        do("stream_push_audio s16 async", ctx.stream_push_audio, a48, where="async")
        do("stream_wait_uploads", ctx.stream_wait_uploads)
        do("stream_reset", ctx.stream_reset, 5)
        do("stream_take_view", ctx.stream_take_view, 2)
        do("set_frame_stride", ctx.set_frame_stride, 16)
        do("set_tries", ctx.set_tries, 1)
        do("demod_resume", ctx.demod_resume, frames, np.ones((2, 1), np.uint8), None)
        do("pipeline_batch", ctx.pipeline_batch, frames, max_per_frame=2)
        do("pipeline_slabs None", ctx.pipeline_slabs, 3, None)
        do("pack_slabs_into", ctx.pack_slabs_into, 2, 3, np.zeros((2, 32 + 48 * 3), np.uint8))
        items = [{"frame": 0, "shift": 3, "f": 1.5, "symbols": np.zeros(162, np.uint8)},
                 {"frame": 1, "shift": -2, "f": -0.5, "drift": 0.25, "text": "K1ABC FN42 37"}]
        do("subtract", ctx.subtract, frames, items)
        do("subtract nothing", ctx.subtract, frames, [], refine=False, out=np.empty((2, FL, 2), np.float32))
        do("osd", ctx.osd, sym3)
        do("osd order 1, nothing", ctx.osd, np.zeros((0, 162), np.uint8), order=1)
        do("deep_set_list", ctx.deep_set_list, ["K1ABC FN42 37", np.arange(7, dtype=np.int8)])
        do("deep_set_list empty", ctx.deep_set_list, [])
        do("deep", ctx.deep, sym3)
        do("deep nothing", ctx.deep, np.zeros((0, 162), np.uint8))
        do("calls_set", ctx.calls_set, ["K1ABC"], grids=["FN42"], powers=[37])
        do("calls_set any", ctx.calls_set, ["K1ABC", "W1AW"])
        do("calls", ctx.calls, sym3)
        do("calls nothing", ctx.calls, np.zeros((0, 162), np.uint8))
        do("blockdemod", ctx.blockdemod, frames, [{"frame": 0, "shift": 1, "f": 0.5}, {"frame": 1, "shift": 0, "f": 0.0, "drift": 1.0}])
        do("blockdemod nothing", ctx.blockdemod, frames, [])
        # the four transmit routes, baseband and audio: plain, moving, at a carrier, through a medium
        s0 = {"symbols": np.arange(162) % 4, "f0": 1.0, "gain": 0.5}
        mot = {"v": (1.0, -1.0), "p": (0.0, 300.0), "model": "delay", "spreading": True}
        fad = {"spread": 1.0, "k": 2.0, "seed": 5, "paths": 8}
        do("tx_baseband plain", ctx.tx_baseband, [s0], n=128)
        do("tx_baseband nothing", ctx.tx_baseband, [], n=64, t0=10, channel=1)
        do("tx_baseband moving", ctx.tx_baseband, [dict(s0, motion=mot)], n=128)
        do("tx_baseband at", ctx.tx_baseband, [dict(s0, carrier=1800), dict(s0, motion=mot)], n=128)
        do("tx_baseband medium", ctx.tx_baseband, [dict(s0, fading=fad, carrier=900), s0], n=128)
        do("tx_render plain", ctx.tx_render, [s0], 256)
        do("tx_render moving s16", ctx.tx_render, [dict(s0, motion=mot, channel=1)], 256, t0=12, channels=2, sigma=[0.1, 0.2], seed=[3, -1],
           background=[None, a48], background_gain=0.5, format="s16")
        do("tx_render at", ctx.tx_render, [dict(s0, carrier=2000)], 256, background=np.zeros(100, np.float32))
        do("tx_render medium", ctx.tx_render, [dict(s0, carrier=1200, fading=fad), dict(s0, channel=1)], 256, channels=2, sigma=0.01, seed=9,
           impulses=[None, {"rate": 0.001, "sigma": 2.0, "seed": 4, "length": 3}])
        do("tx_render impulses only", ctx.tx_render, [s0], 256, impulses={"rate": 0.01, "sigma": 1.0})
        do("dist_unique_id", G.Context.dist_unique_id)
        do("dist_init", ctx.dist_init, 0, 1, b"\x01" * 128)
        do("dist_finalize", ctx.dist_finalize)
        do("prof_enable all", ctx.prof_enable, True)
        do("prof_enable some", ctx.prof_enable, ("tonecorr", "sched"))
        do("prof_enable off", ctx.prof_enable, False)
        do("prof_intervals", ctx.prof_intervals, "coarse", 0, cap=16)
        do("prof_read", ctx.prof_read)
        do("close", ctx.close)

        # ---- module-level functions
        do("deinterleave", G.deinterleave, np.arange(162) % 256)
        do("fano_decode", G.fano_decode, sym3[0], delta=30, maxcycles=100)
        do("fano_encode", G.fano_encode, np.arange(11, dtype=np.uint8))
        do("decode_candidate", G.decode_candidate, np.zeros((), N.DEMOD_DTYPE))
        do("host_threads", G.host_threads)
        do("host_set_ranks", G.host_set_ranks, 2)
        do("decode_batch", G.decode_batch, np.zeros((2, 2), N.DEMOD_DTYPE), nthreads=3)
        do("unpack_message", G.unpack_message, np.zeros(7, np.int8))
        buf = None

        def alloc():
            nonlocal buf
            buf = G.host_alloc(1024)
            return len(buf)
        do("host_alloc", alloc)
        do("host_free", lambda: G.host_free(buf))
        do("frontend_design", G.frontend_design)
        do("frontend_design stage 2", G.frontend_design, G.FRONTEND_COMPACT, stage=2, centre=1800, half_bw=25)
        do("tx_taps", G.tx_taps)
        do("tx_design", G.tx_design, carrier=1800, cutoff=3000)
        do("tx_carrier_launch_counts", G.tx_carrier_launch_counts)
        do("tx_medium_launch_counts", G.tx_medium_launch_counts)
        do("tx_fade_design", G.tx_fade_design, fad)
        do("frontend_rotator", G.frontend_rotator)
        do("frontend_carrier_launch_counts", G.frontend_carrier_launch_counts)
        do("resample_design", G.resample_design, 48000)
        do("resample_launch_counts", G.resample_launch_counts)
        do("blank_launch_counts", G.blank_launch_counts)
        do("c2_read", G.c2_read, "a.c2")
        do("wspr_pack", G.wspr_pack, "K1ABC FN42 37")
        do("call_message", G.call_message, "K1ABC", "FN42", 37)
        do("call_message ngrid", G.call_message, "K1ABC", 1234, 0)
        do("nhash", G.nhash, "K1ABC")
        do("wspr_symbols", G.wspr_symbols, "K1ABC FN42 37")
        do("write_c2", G.write_c2, "b.c2", np.zeros((45000, 2), np.float32), dial_freq=7.0386, type=1)
        do("tx_sigma", G.tx_sigma, -20.0, gain=2.0)
        do("supported_rate", lambda: [G.supported_rate(r) for r in (12000, 44100, 48000, 7999, 11025 * 17)])
        wav = os.path.join(str(tmp), "t.wav")
        do("encode_wav", G.encode_wav, wav, [("K1ABC FN42 37", 1, 0.0, 10.0), dict(s0, carrier=1800)], channels=2, snr_db=-10.0, seed=2,
           seconds=0.5, piece_s=0.2, impulses={"rate": 0.001, "sigma": 1.0})
        do("read_wav", G.read_wav, wav, channels="all")
        do("decode_wav", G.decode_wav, wav, channels="all", carriers=[1500, 1800], osd=2)

        # ---- the pipe, every keyword set
        pipe = None

        def open_pipe():
            nonlocal pipe
            pipe = G.Pipe(fs=375, fl=FL, spb=256, maxdrift=1, maxfreqs=4, halfbandwidth=10, cf=1500, threshold=9, device=0, hop=16,
                          batch_frames=4, max_per_frame=2, lanes=2, host_threads=3, eager=True, sched="staged", spare_after_us=50,
                          passes=2, osd=2, osd_gap=400, block=3, audio_rate=48000, blank=24, blank_guard=2, carriers=[1500, 1800],
                          frontend_hbw=25, known=["K1ABC FN42 37"], deep_min=4000, deep_gap=1000, calls=["K1ABC"],
                          call_grids=["FN"], call_powers=[37, 30], call_min=5000, call_gap=700)
        do("Pipe", open_pipe)
        do("Pipe defaults", lambda: G.Pipe(audio_rate=12000, known=[], calls=[]).close())
        do("pipe.push", pipe.push, np.zeros((50, 2), np.float32))
        do("pipe.push_audio 1-D", pipe.push_audio, a48)
        do("pipe.push_audio [n, 2]", pipe.push_audio, np.zeros((300, 2), np.float32))
        do("pipe.acquire", pipe.acquire, 100)
        do("pipe.commit", pipe.commit, 100)
        do("pipe.submit_device", pipe.submit_device, 4096, B=2, stride=80)
        do("pipe.flush", pipe.flush)
        do("pipe.collect", pipe.collect, cap=8, wait=True)
        do("pipe.inject_failure", pipe.inject_failure, 3, 1)
        do("pipe.set_option", pipe.set_option, "fast_search", 1)
        do("pipe.set_list", pipe.set_list, np.zeros((2, 7), np.int8))
        do("pipe.set_calls", pipe.set_calls, "W1AW", powers=[0])
        do("pipe.set_carriers", pipe.set_carriers, [1400, 1500, 1600])
        do("pipe.split_plane", pipe.split_plane, 4)
        do("pipe.blank_stats", pipe.blank_stats, 2)
        do("pipe.stats", pipe.stats)
        do("pipe.close", pipe.close)
    finally:
        N._lib = saved
    return T


def test_binding_issues_the_recorded_calls(G, tmp_path):
    got = json.loads(json.dumps(drive(G, tmp_path)))
    want = json.load(open(FIXTURE))
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "trace entry %d: %r, recorded %r" % (k, g, w)


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gr_uwspr_amd
    with tempfile.TemporaryDirectory() as d:
        trace = drive(gr_uwspr_amd, d)
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(e) for e in trace) + "\n]\n")
    print("%d entries, %d C calls" % (len(trace), sum(e[0] == "call" for e in trace)))
