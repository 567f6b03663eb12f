"""leaxer-tts --encode WAV --encode-chunk MS on a file that is not at 24 kHz: the encoder stream is opened at the file's own rate, so the
codes file is byte for byte what --encode alone writes, whatever MS."""
import os
import subprocess

import pytest

import mimi_ref
from test_gpu_cli_encode import write_wav16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_encode_chunk_of_a_16k_file_writes_the_same_codes_file(tmp_path):
    wav = str(tmp_path / "in16k.wav")
    write_wav16(wav, mimi_ref.clip(16123, 43), rate=16000)          # 1.0 s at 16 kHz: 24 184 samples at 24 kHz, 13 frames
    outs = []
    for extra in ([], ["--encode-chunk", "200"], ["--encode-chunk", "7"]):
        out = str(tmp_path / ("codes%d" % len(outs)))
        r = subprocess.run([CLI, "-m", "synthetic:0", "--encode", wav, "--save-codes", out] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Encoded 13 frames" in r.stdout, r.stdout + r.stderr
        outs.append(open(out, "rb").read())
    assert len(outs[0]) > 0 and outs[0] == outs[1] == outs[2]
