"""leaxer-tts --loudness LUFS: the WAV through the loudness stage.  Without the flag the file is the one written before the stage
existed: the run's --save-codes frames through the same weights' one-shot decode, converted by save_wav16's rule.  With it the file must
be the standalone stages over those samples — loudness alone, one-shot and with --stream-chunk, and loudness -> sink with --out-rate,
the Python path's samples — byte for byte.  A value out of range is refused with the range in the message."""
import os
import struct
import subprocess

import numpy as np
import pytest

import q3tts
from util import tiny_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def read_wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and b[36:40] == b"data"
    fmt, ch, rate, bps, align, bits = struct.unpack("<HHIIHH", b[20:36])
    assert (fmt, ch, align, bits) == (1, 1, 2, 16) and bps == 2 * rate
    return rate, np.frombuffer(b[44:], np.int16)


def wav16(x):
    """save_wav16's rule: clip to [-1, 1], (int16_t)(v * 32767.0f), truncating"""
    return (np.clip(x.astype(np.float32), np.float32(-1), np.float32(1)) * np.float32(32767.0)).astype(np.int16)


def read_codes(path):
    return np.array([[int(v) for v in line.split()] for line in open(path) if line.strip()], np.int64)


def test_loudness(tmp_path):
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
    assert rate == 24000 and np.array_equal(w, wav16(x))            # without the flag: the file written before the stage existed
    ids = eng.loudness_begin(*q3tts.loudness_params(-16)), eng.loudness_begin(*q3tts.loudness_params(-16, 6)), eng.pcm_sink_begin(8000, "int16")
    even = eng.loudness_push_batch([ids[0]], [x], [True])[0]
    rate_a, a = read_wav(cli("l16", ["--loudness", "-16"]))
    rate_b, b = read_wav(cli("l16_s", ["--loudness", "-16", "--stream-chunk", "5"]))
    assert rate_a == rate_b == 24000 and even.size == x.size
    assert np.array_equal(a, wav16(even)) and np.array_equal(b, wav16(even))
    # composed with --loudness-range and --out-rate: loudness -> sink, the Python path's samples
    narrow = eng.loudness_push_batch([ids[1]], [x], [True])[0]
    ref = eng.pcm_sink_push_batch([ids[2]], [narrow], [True])[0]
    eng.loudness_end(ids[0]), eng.loudness_end(ids[1]), eng.pcm_sink_end(ids[2])
    rate_c, c = read_wav(cli("l16_8k", ["--loudness", "-16", "--loudness-range", "6", "--out-rate", "8000"]))
    eng.close()
    assert rate_c == 8000 and ref.dtype == np.int16 and np.array_equal(c, ref)


def test_loudness_refused(tmp_path):
    for flags, word in ((["--loudness", "-4"], "-40 .. -5"), (["--loudness", "-16", "--loudness-range", "41"], "0 .. 40")):
        r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22", "--max-tokens", "2", "-o", str(tmp_path / "x.wav")] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and word in r.stderr, r.stderr
