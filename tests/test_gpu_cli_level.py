"""leaxer-tts --gain DB --limit X: the WAV through the output-level stage.  The plain run's float samples are recovered exactly — the
run's --save-codes frames through the same weights' one-shot decode, checked against the plain WAV under save_wav16's rule — and the
flagged runs' files must be the numpy restatement (tests/level_ref.py) of those samples, then save_wav16, byte for byte; with --speed
and --out-rate the file is the composed standalone stages (stretcher -> level -> sink).  The gain is chosen from the plain run's peak
so that the limiter has overs to work on.  Out-of-range values are refused with the range in the message."""
import os
import struct
import subprocess

import numpy as np
import pytest

import q3tts
from level_ref import level32
from util import tiny_pair

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


def wav16(x):
    """save_wav16's rule: clip to [-1, 1], (int16_t)(v * 32767.0f), truncating"""
    return (np.clip(x.astype(np.float32), np.float32(-1), np.float32(1)) * np.float32(32767.0)).astype(np.int16)


def read_codes(path):
    return np.array([[int(v) for v in line.split()] for line in open(path) if line.strip()], np.int64)


def test_gain_and_limit(tmp_path):
    eng, orc, _ = tiny_pair(seed=4, max_batch=1, max_ctx=96)
    orc.close()
    mdir = tmp_path / "model"
    mdir.mkdir()
    eng.save_weights(str(mdir / "model.q3w"))
    common = ["-m", str(mdir), "--tokens", "11,22,33,44,55", "--max-tokens", "12", "--seed", "3"]

    def cli(name, extra):
        out = str(tmp_path / (name + ".wav"))
        r = subprocess.run([CLI, "-o", out] + common + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return out
    codes_file = str(tmp_path / "plain.codes")
    plain = cli("plain", ["--save-codes", codes_file])
    x = eng.codec_decode(read_codes(codes_file))
    rate, w = read_wav(plain)
    assert rate == 24000 and np.array_equal(w, wav16(x))            # the plain run's float samples, exactly
    T = 0.5
    cb = int(np.clip(round(200.0 * np.log10(3.0 * T / float(np.abs(x).max()))), -600, 400)) or 10
    flags = ["--gain", "%.1f" % (cb / 10.0), "--limit", "0.5"]
    y, s = level32(x, cb, 500, want_s=True)
    assert np.count_nonzero(s < 1.0) > 0                             # the limiter has work
    rate_a, a = read_wav(cli("level", flags))
    rate_b, b = read_wav(cli("level_s", flags + ["--stream-chunk", "5"]))
    assert rate_a == rate_b == 24000
    assert np.array_equal(a, wav16(y)) and np.array_equal(b, wav16(y))
    assert np.abs(a.astype(int)).max() <= int(0.5 * 32767)
    rate_g, g = read_wav(cli("gain", ["--gain", "%.1f" % (cb / 10.0)]))
    assert rate_g == 24000 and np.array_equal(g, wav16(level32(x, cb, 0)))
    # composed with --speed and --out-rate: stretcher -> level -> sink, the standalone stages
    rate_c, c = read_wav(cli("all", flags + ["--speed", "1.25", "--out-rate", "8000"]))
    ids = eng.speed_begin(1250), eng.level_begin(cb, 500), eng.pcm_sink_begin(8000, "int16")
    mid = eng.speed_push_batch([ids[0]], [x], [True])[0]
    mid = eng.level_push_batch([ids[1]], [mid], [True])[0]
    ref = eng.pcm_sink_push_batch([ids[2]], [mid], [True])[0]
    eng.speed_end(ids[0]), eng.level_end(ids[1]), eng.pcm_sink_end(ids[2])
    eng.close()
    assert rate_c == 8000 and ref.dtype == np.int16 and np.array_equal(c, ref)


def test_level_refused(tmp_path):
    for flags, word in ((["--gain", "41"], "-60 .. +40"), (["--limit", "1.5"], "0.001 .. 1.0")):
        r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22", "--max-tokens", "2", "-o", str(tmp_path / "x.wav")] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and word in r.stderr, r.stderr
