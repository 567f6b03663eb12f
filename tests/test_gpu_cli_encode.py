"""leaxer-tts --encode / --ref-text: audio -> codes through the CLI, and the in-context clone that consumes them."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import mimi_ref
import q3_oracle as qo
import q3tts
from util import calibrate_codec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def write_wav16(path, x, rate=24000):
    s = (np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(s)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * 2, 2, 16) + b"data" + struct.pack("<I", len(s)) + s)


def read_codes(path):
    return np.array([[int(v) for v in line.split()] for line in open(path) if line.strip()], np.int64)


def test_encode_then_continue_round_trips_through_the_files(tmp_path):
    z = np.load(os.path.join(ROOT, "tests", "golden", "hf_mimi_encoder.npz"))
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)
    w.update({k[2:]: z[k] for k in z.files if k.startswith("w:enc.")})
    eng = q3tts.Engine(q3tts.Config.from_dict(dict(ocfg.to_dict(), **json.loads(str(z["cfg"])))), device=0, max_batch=1, max_ctx=96)
    eng.load(w)
    mdir = tmp_path / "model"
    mdir.mkdir()
    eng.save_weights(str(mdir / "model.q3w"))
    wav, c0, c1 = str(tmp_path / "ref.wav"), str(tmp_path / "ref.codes"), str(tmp_path / "all.codes")
    write_wav16(wav, mimi_ref.clip(4 * 1920 + 100, 40))
    r = subprocess.run([CLI, "-m", str(mdir), "--encode", wav, "--save-codes", c0], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Encoded 5 frames" in r.stdout, r.stdout + r.stderr
    pcm, rate = q3tts.read_wav(wav)
    want = eng.audio_encode(pcm)
    eng.close()
    assert rate == 24000 and np.array_equal(read_codes(c0), want)
    r = subprocess.run([CLI, "-m", str(mdir), "--tokens", "11,22,33,44,55,66,77", "--continue-codes", c0, "--save-codes", c1, "--max-tokens", "4",
                        "-o", str(tmp_path / "o.wav"), "--seed", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "5 recorded + " in r.stdout, r.stdout + r.stderr
    allc = read_codes(c1)
    assert allc.shape[0] > 5 and np.array_equal(allc[:5], want)


def test_ref_tokens_in_context_clone_on_synthetic(tmp_path):
    wav, out, c1 = str(tmp_path / "ref.wav"), str(tmp_path / "o.wav"), str(tmp_path / "all.codes")
    write_wav16(wav, mimi_ref.clip(2 * 1920, 41))
    r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22,33", "--ref", wav, "--ref-tokens", "101,102", "--max-tokens", "3", "-o", out,
                        "--save-codes", c1], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "In-context clone: 2 reference text tokens" in r.stdout, r.stdout + r.stderr
    allc = read_codes(c1)
    assert allc.shape[1] == 16 and 2 < allc.shape[0] <= 5 and (allc >= 0).all() and (allc[:, 0] < 2048).all()
    n = (os.path.getsize(out) - 44) // 2
    assert 0 < n <= 3 * 1920          # the target's samples only: at most the new frames' worth
