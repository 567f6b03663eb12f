"""leaxer-tts --eq SPEC: the WAV through the tone stage.  `--eq telephone --out-rate 8000 --out-format mulaw`, a narrow-band telephone
leg, must write the bytes the Python path delivers for the same settings: the run's --save-codes frames through the same weights'
one-shot decode, the standalone tone stage and the standalone mu-law sink — one-shot and with --stream-chunk, byte for byte.  A spec
that cannot be read or is out of range is refused with the field named, and nothing is written."""
import os
import subprocess

import numpy as np
import pytest

import q3tts
from test_gpu_cli_g711 import read_wav_g711
from test_gpu_cli_loudness import read_codes, read_wav, wav16
from util import tiny_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_eq_telephone_line(tmp_path):
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
    cli("plain", ["--save-codes", codes_file])
    x = eng.codec_decode(read_codes(codes_file))
    tone, sink = eng.tone_begin("telephone"), eng.pcm_sink_begin(8000, "mulaw")
    shaped = eng.tone_push_batch([tone], [x], [True])[0]
    ref = eng.pcm_sink_push_batch([sink], [shaped], [True])[0]
    eng.tone_end(tone), eng.pcm_sink_end(sink)
    line = ["--eq", "telephone", "--out-rate", "8000", "--out-format", "mulaw"]
    for name, extra in (("line", line), ("line_s", line + ["--stream-chunk", "5"])):
        tag, rate, data = read_wav_g711(cli(name, extra))
        assert (tag, rate) == (7, 8000) and ref.dtype == np.uint8 and data.size == ref.size > 0, name
        assert data.tobytes() == ref.tobytes(), name
    assert len(set(ref.tolist())) > 8                                # not silence
    # the stage alone, as sections: the 24 kHz file is the shaped clip by save_wav16's rule
    rate, w = read_wav(cli("sections", ["--eq", "hp:300:0.707,hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707,lp:3400:0.707"]))
    eng.close()
    assert rate == 24000 and np.array_equal(w, wav16(shaped)) and not np.array_equal(w, wav16(x))


def test_eq_refused(tmp_path):
    for spec, word in (("hp:5:0.707", "section 0 freq_hz 5"), ("peak:1000:+30:1", "section 0 gain_cb 300"), ("hp:300:0.7,lp:3400:20", "section 1 q_permille 20000"),
                       ("treble:300:1", "kind 'treble'")):
        out = str(tmp_path / "x.wav")
        r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22", "--max-tokens", "2", "-o", out, "--eq", spec], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and word in r.stderr and "--eq" in r.stderr, r.stderr
        assert not os.path.exists(out)
