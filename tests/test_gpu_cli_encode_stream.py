"""leaxer-tts --encode WAV --encode-chunk MS: the file pushed MS milliseconds at a time through one encoder stream
(TTSEngine::audio_stream_push) gives the codes file --encode alone gives, byte for byte."""
import os
import subprocess

import pytest

import mimi_ref
from test_gpu_cli_encode import write_wav16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_encode_chunk_writes_the_same_codes_file(tmp_path):
    wav, c0, c1 = str(tmp_path / "in.wav"), str(tmp_path / "oneshot.codes"), str(tmp_path / "stream.codes")
    write_wav16(wav, mimi_ref.clip(16 * 1920 + 480, 42))          # 1.3 s at 24 kHz: 17 frames, 200 ms pushes cut inside frames
    r = subprocess.run([CLI, "-m", "synthetic:0", "--encode", wav, "--save-codes", c0], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Encoded 17 frames" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([CLI, "-m", "synthetic:0", "--encode", wav, "--encode-chunk", "200", "--save-codes", c1], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Encoded 17 frames" in r.stdout, r.stdout + r.stderr
    a, b = open(c0, "rb").read(), open(c1, "rb").read()
    assert len(a) > 0 and a == b
