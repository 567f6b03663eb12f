"""leaxer-tts --out-rate R: the WAV at the sink's rate.  With --stream-chunk the scheduler's streams carry the sink, without it the whole
decode goes through one push + finish of the same resampler; both write ceil(n24 / 3) samples at 8 kHz, within 1 LSB of each other
(the streamed and the one-shot vocoder already differ by fp32 rounding).  --out-rate 24000 is the file written without the flag."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def read_wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    fmt, ch, rate, bps, align, bits = struct.unpack("<HHIIHH", b[20:36])
    assert (fmt, ch, align, bits) == (1, 1, 2, 16) and bps == 2 * rate
    n = struct.unpack("<I", b[40:44])[0]
    assert struct.unpack("<I", b[4:8])[0] == 36 + n and len(b) == 44 + n
    return rate, np.frombuffer(b[44:], np.int16)


def test_out_rate(tmp_path):
    common = ["-m", "synthetic:0", "--tokens", "11,22,33,44,55", "--max-tokens", "12", "--seed", "3"]
    files = {}
    for name, extra in (("plain", []), ("r24", ["--out-rate", "24000"]), ("r8", ["--out-rate", "8000"]),
                        ("r8s", ["--out-rate", "8000", "--stream-chunk", "5"])):
        out = str(tmp_path / (name + ".wav"))
        r = subprocess.run([CLI, "-o", out] + common + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        files[name] = out
    assert open(files["plain"], "rb").read() == open(files["r24"], "rb").read()
    rate24, w24 = read_wav(files["plain"])
    rate_a, a = read_wav(files["r8"])
    rate_b, b = read_wav(files["r8s"])
    assert rate24 == 24000 and rate_a == 8000 and rate_b == 8000
    assert w24.size > 0 and a.size == b.size == -(-w24.size // 3)
    assert np.abs(a.astype(int) - b.astype(int)).max() <= 1
    assert np.abs(a.astype(int)).max() > 0


def test_out_rate_refused(tmp_path):
    r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22", "--max-tokens", "2", "--out-rate", "3999", "-o", str(tmp_path / "x.wav")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "3999" in r.stderr
