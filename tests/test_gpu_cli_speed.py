"""leaxer-tts --speed X: the WAV X times as fast.  Without --stream-chunk the whole clip passes the standalone stage, with it the
chunks pass a stretcher while they are generated; the stage's output does not depend on the cuts and --stream-chunk gives the one-shot
decode's samples, so the files are the same bytes, ceil(1000 n24 / S) samples long.  With --feed the stretcher sits inside the
scheduler's streams, whose vocoder pushes round differently from the one-shot decode: the same length is asserted, not the same bytes.
--speed 1.0 is the file written without the flag; --speed 3 is refused with the range in the message."""
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


def test_speed(tmp_path):
    common = ["-m", "synthetic:0", "--tokens", "11,22,33,44,55", "--max-tokens", "12", "--seed", "3"]
    files = {}
    for name, extra in (("plain", []), ("s1", ["--speed", "1.0"]), ("fast", ["--speed", "1.25"]),
                        ("fast_s", ["--speed", "1.25", "--stream-chunk", "5"]),
                        ("fast_8k", ["--speed", "1.25", "--out-rate", "8000"]),
                        ("fast_feed", ["--speed", "1.25", "--stream-chunk", "5", "--feed", "2"])):
        out = str(tmp_path / (name + ".wav"))
        r = subprocess.run([CLI, "-o", out] + common + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        files[name] = out
    assert open(files["plain"], "rb").read() == open(files["s1"], "rb").read()
    rate24, w24 = read_wav(files["plain"])
    rate_a, a = read_wav(files["fast"])
    rate_b, b = read_wav(files["fast_s"])
    rate_c, c = read_wav(files["fast_8k"])
    assert rate24 == 24000 and rate_a == 24000 and rate_b == 24000 and rate_c == 8000
    n_fast = -(-1000 * w24.size // 1250)
    assert w24.size > 0 and a.size == b.size == n_fast
    assert open(files["fast"], "rb").read() == open(files["fast_s"], "rb").read()
    assert c.size == -(-n_fast // 3)                       # composes with --out-rate: the stretched clip, resampled
    assert np.abs(a.astype(int)).max() > 0 and np.abs(c.astype(int)).max() > 0
    rate_d, d = read_wav(files["fast_feed"])               # through the scheduler's float callback
    assert rate_d == 24000 and d.size == n_fast and np.abs(d.astype(int)).max() > 0


def test_speed_refused(tmp_path):
    r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22", "--max-tokens", "2", "--speed", "3", "-o", str(tmp_path / "x.wav")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "0.5 .. 2.0" in r.stderr and "3" in r.stderr
