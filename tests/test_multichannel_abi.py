"""Multichannel audio into one pipe, the parts a machine without a GPU can check: the entry point is declared, exported
and bound; uwspr_decode's channel sits where the header and DECODE_DTYPE both say (offset 108, the record still 112
bytes); read_wav(channels="all") returns every channel as scipy.io.wavfile does, and the default call is unchanged."""
import os
import re
import shutil
import subprocess
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uwspr_hip.h")


def test_entry_point_is_declared_exported_and_bound(G):
    hdr = open(HEADER).read()
    name = "uwspr_pipe_push_audio_channels"
    assert re.search(r"\bint %s\(uwspr_pipe \*pipe, const void \*audio, int nframes, int nchannels, int format\);" % name, hdr)
    assert re.search(r"#define UWSPR_PIPE_MAX_CHANNELS 64\b", hdr)
    assert name in G.native.ABI_SYMBOLS
    L = G.native.lib()
    assert hasattr(L, name) and len(getattr(L, name).argtypes) == 5
    assert G.native.PIPE_MAX_CHANNELS == 64


def test_decode_record_layout_in_c_and_numpy(G, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a C++ compiler is needed to check the header's layout")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include "uwspr_hip.h"\n'
                   "static_assert(offsetof(uwspr_decode, message) == 100, \"message\");\n"
                   "static_assert(offsetof(uwspr_decode, channel) == 108, \"channel\");\n"
                   "static_assert(sizeof(((uwspr_decode *)0)->channel) == 2, \"int16\");\n"
                   "static_assert(sizeof(uwspr_decode) == 112, \"size\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    D = G.native.DECODE_DTYPE
    assert D.itemsize == 112
    assert D.fields["message"][1] == 100 and D.fields["channel"][1] == 108
    assert D.fields["channel"][0] == np.dtype("<i2")
    rec = np.zeros(1, D)
    rec["channel"] = 5
    assert rec.tobytes()[108:110] == (5).to_bytes(2, "little")


def _write(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(2)
        w.setframerate(12000)
        w.writeframes(np.ascontiguousarray(x).tobytes())


@pytest.mark.parametrize("channels", [2, 5])
def test_read_wav_all_channels_matches_scipy(G, tmp_path, channels):
    from scipy.io import wavfile
    x = np.random.default_rng(100 + channels).integers(-32768, 32768, size=(12000 * 2 + 13, channels), dtype=np.int16)
    path = tmp_path / "m.wav"
    _write(path, x)
    rate_ref, ref = wavfile.read(str(path))
    y, rate = G.read_wav(path, channels="all")
    assert rate == rate_ref == 12000
    assert y.dtype == np.int16 and y.shape == ref.shape == (x.shape[0], channels) and y.flags.c_contiguous
    assert np.array_equal(y, ref)
    y0, _ = G.read_wav(path)   # the default: channel 0, 1-D, as before
    assert y0.ndim == 1 and y0.flags.c_contiguous and np.array_equal(y0, ref[:, 0])


def test_read_wav_all_channels_of_a_mono_file(G, tmp_path):
    x = np.arange(-500, 500, dtype=np.int16)[:, None]
    path = tmp_path / "mono.wav"
    _write(path, x)
    y, _ = G.read_wav(path, channels="all")
    assert y.shape == (1000, 1) and np.array_equal(y, x)


def test_read_wav_refuses_an_unknown_channel_selection(G, tmp_path):
    path = tmp_path / "s.wav"
    _write(path, np.zeros((10, 2), np.int16))
    with pytest.raises(ValueError, match="channels"):
        G.read_wav(path, channels=1)
