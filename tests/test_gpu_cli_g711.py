"""leaxer-tts --out-format mulaw / alaw: the G.711 WAV a PBX plays (format tag 7 / 6, 18-byte fmt chunk, fact chunk, data padded to an
even length), whose bytes are the numpy restatement (tests/g711_ref.py) of the law applied to the int16 samples the same command line
writes with --out-format pcm16 — byte for byte, at 24 kHz (the format-only sink) and at --out-rate 8000, with and without
--stream-chunk.  And back: --encode of such a file gives the codes of the 16-bit WAV that holds its decode."""
import os
import struct
import subprocess

import numpy as np
import pytest

import g711_ref
from test_gpu_cli_out_rate import read_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
COMMON = ["-m", "synthetic:0", "--tokens", "11,22,33,44,55", "--max-tokens", "12", "--seed", "3"]
SHAPES = {"r24": [], "r24s": ["--stream-chunk", "5"], "r8": ["--out-rate", "8000"], "r8s": ["--out-rate", "8000", "--stream-chunk", "5"]}
TAGS = {"mulaw": 7, "alaw": 6}


def cli(out, extra):
    r = subprocess.run([CLI, "-o", out] + COMMON + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def read_wav_g711(path):
    """-> (format tag, rate, data bytes); asserts the whole layout"""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and struct.unpack("<I", b[16:20])[0] == 18
    tag, ch, rate, bps, align, bits, cb = struct.unpack("<HHIIHHH", b[20:38])
    assert (ch, align, bits, cb) == (1, 1, 8, 0) and bps == rate
    assert b[38:42] == b"fact" and struct.unpack("<I", b[42:46])[0] == 4
    n_fact = struct.unpack("<I", b[46:50])[0]
    assert b[50:54] == b"data"
    n = struct.unpack("<I", b[54:58])[0]
    pad = n & 1
    assert n_fact == n and len(b) == 58 + n + pad and struct.unpack("<I", b[4:8])[0] == len(b) - 8
    return tag, rate, np.frombuffer(b[58:58 + n], np.uint8)


@pytest.fixture(scope="module")
def pcm16(tmp_path_factory):
    """each shape of command line with --out-format pcm16: written once, shared"""
    d = tmp_path_factory.mktemp("pcm16")
    return {name: cli(str(d / (name + ".wav")), extra + ["--out-format", "pcm16"]) for name, extra in SHAPES.items()}


@pytest.mark.parametrize("law", list(TAGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bytes_are_the_law_of_the_pcm16_file(tmp_path, pcm16, shape, law):
    out = cli(str(tmp_path / "g.wav"), SHAPES[shape] + ["--out-format", law])
    tag, rate, data = read_wav_g711(out)
    rate16, s = read_wav(pcm16[shape])
    assert tag == TAGS[law] and rate == rate16 == (8000 if "r8" in shape else 24000)
    assert s.size > 0 and np.abs(s.astype(int)).max() > 0
    assert data.size == s.size and np.array_equal(data, g711_ref.ENC[law](s))


def test_pcm16_is_the_file_written_without_the_flag(tmp_path, pcm16):
    for shape in ("r24", "r8s"):
        plain = cli(str(tmp_path / (shape + ".wav")), SHAPES[shape])
        assert open(plain, "rb").read() == open(pcm16[shape], "rb").read(), shape


def test_unknown_format_is_refused_by_name(tmp_path):
    r = subprocess.run([CLI, "-o", str(tmp_path / "x.wav")] + COMMON + ["--out-format", "gsm610"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "gsm610" in r.stderr and not os.path.exists(str(tmp_path / "x.wav"))


def test_encode_reads_the_file_back(tmp_path):
    g = cli(str(tmp_path / "line.wav"), SHAPES["r8"] + ["--out-format", "mulaw"])
    tag, rate, data = read_wav_g711(g)
    assert tag == 7 and rate == 8000
    s = g711_ref.mu_dec(data).astype("<i2").tobytes()
    lin = str(tmp_path / "lin.wav")
    with open(lin, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(s)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 8000, 16000, 2, 16) + b"data" + struct.pack("<I", len(s)) + s)
    codes = {}
    for name, wav, extra in (("g711", g, []), ("lin", lin, []), ("g711_chunked", g, ["--encode-chunk", "100"])):
        out = str(tmp_path / (name + ".codes"))
        r = subprocess.run([CLI, "-m", "synthetic:0", "--encode", wav, "--save-codes", out] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Encoded" in r.stdout, r.stdout + r.stderr
        codes[name] = open(out).read()
    assert codes["g711"] == codes["lin"] == codes["g711_chunked"] and len(codes["lin"].split("\n")) > 4
