"""A context on a caller's stream (Context.set_stream) gives the bytes a context on its own stream gives.

With a caller's stream the binding waits for nothing: the inputs are made on that stream by the work queued just
before the call, the library's kernels are queued behind them, and the caller synchronizes its stream before reading
device results.  The other context owns its stream and goes through the binding's waits.  Same kernels, same inputs:
equality, no tolerance.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FL = 45000
RNG = np.random.default_rng(20240611)
AUDIO48 = (3000 * RNG.standard_normal(4800)).astype(np.int16)
BLANK_IN = RNG.standard_normal((2 * 4096 + 17, 2)).astype(np.float32)
BLANK_IN[[100, 5000, 8200], [0, 1, 0]] = 60.0                                 # impulses for the blanker to find
SYM3 = RNG.integers(0, 256, (3, 162)).astype(np.uint8)
AUDIO12 = RNG.standard_normal((1, 32 * FL)).astype(np.float32)                # one frame's worth at 12 kS/s
KNOWN = ["K1ABC FN42 37", "W1AW FN31 30"]
TX = [{"text": "K1ABC FN42 37", "start": 0, "f0": 12.5}]


@pytest.fixture(scope="module")
def pair(G):
    """(context on its own stream, context on the caller's stream, that stream)"""
    import torch
    s = torch.cuda.Stream()
    own, cal = G.Context(device=0), G.Context(device=0)
    cal.set_stream(s.cuda_stream)
    for c in (own, cal):
        c.deep_set_list(KNOWN)
        c.calls_set(["K1ABC"], grids=["FN42"], powers=[37])
    yield own, cal, s
    torch.cuda.synchronize()
    own.close()
    cal.close()


@pytest.fixture(scope="module")
def frames2(G):
    return G.synth.make_frames(2, seed=4242, snr_db=-18.0)


def _dev(x):
    """a device copy made by a kernel on the current stream: the call that follows depends on queued work"""
    import torch
    return torch.from_numpy(x).to("cuda:0").clone()


def _resample(c, _):
    return [c.resample(_dev(AUDIO48), 48000)]


def _blank(c, _):
    return list(c.blank(_dev(BLANK_IN)))


def _osd(c, _):
    return [c.osd(_dev(SYM3))]


def _deep(c, _):
    return [c.deep(_dev(SYM3))]


def _calls(c, _):
    return [c.calls(_dev(SYM3))]


def _tx_render(c, _):
    import torch
    out = torch.zeros((4096, 1), dtype=torch.float32, device="cuda:0")
    return [c.tx_render(TX, 4096, sigma=0.05, seed=77, out=out)]


def _frontend(c, _):
    return [c.frontend(_dev(AUDIO12))]


def _pipeline_batch(c, frames):
    cands, out = c.pipeline_batch(_dev(frames), max_per_frame=1)
    return list(cands) + [out]


CASES = {"resample": _resample, "blank": _blank, "osd": _osd, "deep": _deep, "calls": _calls, "tx_render": _tx_render,
         "frontend": _frontend, "pipeline_batch": _pipeline_batch}


def _bytes(v):
    return (v if isinstance(v, np.ndarray) else v.cpu().numpy()).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_caller_stream_gives_the_own_stream_bytes(pair, frames2, name):
    import torch
    own, cal, s = pair
    want = [_bytes(v) for v in CASES[name](own, frames2)]
    with torch.cuda.stream(s):
        got = CASES[name](cal, frames2)
    s.synchronize()
    got = [_bytes(v) for v in got]
    assert len(got) == len(want) and all(len(w) > 0 for w in want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: result %d differs between the caller's stream and the context's own" % (name, k)
