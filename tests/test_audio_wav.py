"""read_wav: the 16-bit PCM WAV reader in front of the audio stream (decode_wav) -- channel 0 as int16 and the rate,
against scipy.io.wavfile on the same files; anything the 12 kS/s front-end cannot take is a clear error."""
import struct
import wave

import numpy as np
import pytest


def _write(path, x, rate=12000, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x).tobytes())


@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_matches_scipy(G, tmp_path, channels):
    from scipy.io import wavfile
    rng = np.random.default_rng(channels)
    x = rng.integers(-32768, 32768, size=(12000 * 3 + 7, channels), dtype=np.int16)
    x = x[:, 0] if channels == 1 else x
    path = tmp_path / "a.wav"
    _write(path, x)
    y, rate = G.read_wav(path)
    rate_ref, ref = wavfile.read(str(path))
    ref0 = ref if ref.ndim == 1 else ref[:, 0]
    assert rate == rate_ref == 12000
    assert y.dtype == np.int16 and y.ndim == 1 and y.flags.c_contiguous
    assert np.array_equal(y, ref0)


def test_read_wav_refuses_another_rate(G, tmp_path):
    path = tmp_path / "r.wav"
    _write(path, np.zeros(100, np.int16), rate=48000)
    with pytest.raises(ValueError, match="48000"):
        G.read_wav(path)


@pytest.mark.parametrize("width", [1, 3, 4])
def test_read_wav_refuses_another_width(G, tmp_path, width):
    path = tmp_path / "w.wav"
    _write(path, np.zeros(100 * width, np.uint8), width=width)
    with pytest.raises(ValueError, match="16-bit PCM only"):
        G.read_wav(path)


def test_read_wav_refuses_float(G, tmp_path):
    from scipy.io import wavfile
    path = tmp_path / "f.wav"
    wavfile.write(str(path), 12000, np.zeros(100, np.float32))
    with open(path, "rb") as f:
        assert struct.unpack("<H", f.read(22)[20:22])[0] == 3   # WAVE_FORMAT_IEEE_FLOAT
    with pytest.raises(ValueError, match="16-bit PCM"):
        G.read_wav(path)
