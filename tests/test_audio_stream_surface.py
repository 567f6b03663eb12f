"""The surface of streamed audio-to-codes, checkable without a GPU: the six C-ABI entry points in include/q3tts.h, q3tts.EXPORTS and the
built library, the Python wrappers' argument checks, TTSEngine's methods and the CLI flag.  What the entry points compute is checked on
the GPU: tests/test_gpu_audio_stream.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_audio_stream_begin", "q3tts_audio_stream_push_len", "q3tts_audio_stream_push_host", "q3tts_audio_stream_push_batch_host",
       "q3tts_audio_stream_info", "q3tts_audio_stream_end")
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_audio_stream_begin\(q3tts_engine\* e, int64_t max_samples, int\* stream_id\);", hdr)
    assert re.search(r"int q3tts_audio_stream_push_len\(q3tts_engine\* e, int stream_id, int64_t n_samples, int finish\);", hdr)
    assert re.search(r"int q3tts_audio_stream_push_host\(q3tts_engine\* e, int stream_id, const float\* pcm24k, int64_t n_samples, int finish,\s*"
                     r"int64_t\* codes_out, int cap_frames, int32_t\* n_frames\);", hdr)
    assert re.search(r"int q3tts_audio_stream_info\(q3tts_engine\* e, int stream_id, int64_t\* n_samples, int32_t\* n_frames, int\* finished, int64_t\* bytes\);", hdr)
    assert re.search(r"int q3tts_audio_stream_end\(q3tts_engine\* e, int stream_id\);", hdr)
    # the section states the promise, the 24 kHz contract and the reference lines it stands beside
    sec = hdr[hdr.index("carried-state pushes"):hdr.index("int q3tts_audio_stream_end(")]
    assert "bit-identical" in sec and "24 kHz" in sec and "resample first" in sec and "tts_onnx.cpp:331-365" in sec
    # no engine: refused like every other entry point
    i64 = ctypes.c_int64
    assert L.q3tts_audio_stream_begin(None, i64(0), None) == -1
    assert L.q3tts_audio_stream_push_len(None, 0, i64(1920), 0) == -1
    assert L.q3tts_audio_stream_push_host(None, 0, None, i64(0), 0, None, 0, None) == -1
    assert L.q3tts_audio_stream_push_batch_host(None, 1, None, None, None, None, None, None, None, None) == -1
    assert L.q3tts_audio_stream_info(None, 0, None, None, None, None) == -1
    assert L.q3tts_audio_stream_end(None, 0) == -1


def test_python_callers_exist():
    import q3tts
    E = q3tts.Engine
    for name in ("audio_stream_begin", "audio_stream_push", "audio_stream_push_batch", "audio_stream_push_len", "audio_stream_info", "audio_stream_end",
                 "audio_encode_long"):
        assert callable(getattr(E, name)), name
    assert list(inspect.signature(E.audio_stream_begin).parameters) == ["self", "max_samples"]
    assert list(inspect.signature(E.audio_stream_push).parameters) == ["self", "sid", "pcm", "finish", "want_latents"]
    assert list(inspect.signature(E.audio_stream_push_batch).parameters) == ["self", "sids", "pcms", "finish", "want_latents"]
    sig = inspect.signature(E.audio_encode_long).parameters
    assert list(sig) == ["self", "pcm24k", "chunk_samples"] and sig["chunk_samples"].default == 96000
    S = q3tts.AudioEncodeStream
    for name in ("push", "finish", "close", "__enter__", "__exit__"):
        assert callable(getattr(S, name)), name
    assert isinstance(S.codes, property)
    assert list(inspect.signature(E.audio_encode).parameters) == ["self", "pcm24k", "want_latents"]      # the one-shot stays as it is


class _Shell:
    """an Engine that never reaches the library: the wrappers' own argument checks run before any call"""

    def __init__(self):
        import q3tts
        self.cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))

    def __getattr__(self, name):
        raise AssertionError("the wrapper went on to the library (%s)" % name)


def test_python_wrappers_check_their_arguments():
    import q3tts
    sh = _Shell()
    E = q3tts.Engine
    with pytest.raises(ValueError, match="one sample array per stream"):
        E.audio_stream_push_batch(sh, [0, 1], [np.zeros(10, np.float32)])
    with pytest.raises(ValueError, match="finish: one flag per stream"):
        E.audio_stream_push_batch(sh, [0, 1], [np.zeros(10, np.float32)] * 2, finish=[True])
    with pytest.raises(ValueError, match="once per push"):
        E.audio_stream_push_batch(sh, [3, 3], [np.zeros(10, np.float32)] * 2)
    with pytest.raises(ValueError, match="expected float samples"):
        E.audio_stream_push_batch(sh, [0], [np.zeros(10, np.int16)])
    with pytest.raises(ValueError, match="expected mono samples"):
        E.audio_stream_push_batch(sh, [0], [np.zeros((2, 10), np.float32)])
    assert E.audio_stream_push_batch(sh, [], []) == []                                      # nothing to do: no call
    assert E.audio_stream_push_batch(sh, [], [], want_latents=True) == ([], [])
    with pytest.raises(ValueError, match="max_samples"):
        E.audio_stream_begin(sh, -1)
    with pytest.raises(ValueError, match="n_samples must not be negative"):
        E.audio_stream_push_len(sh, 0, -5)
    with pytest.raises(ValueError, match="chunk_samples must be at least 1"):
        E.audio_encode_long(sh, np.zeros(10, np.float32), chunk_samples=0)
    with pytest.raises(ValueError, match="no samples"):
        E.audio_encode_long(sh, np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="expected float samples"):
        E.audio_encode_long(sh, np.zeros(10, np.int32))


def test_tts_engine_declares_the_stream_methods():
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"int audio_stream_begin\(int64_t max_samples = 0\);", h)
    assert re.search(r"std::vector<int64_t> audio_stream_push\(int id, const float\* pcm, size_t n, bool finish = false", h)
    assert re.search(r"void audio_stream_end\(int id\);", h)
    assert h.index("encode_audio(") < h.index("audio_stream_begin(") < h.index("audio_stream_push(") < h.index("audio_stream_end(")


def test_cli_encode_chunk(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert re.search(r"^\s+--encode-chunk MS ", r.stdout, re.M), r.stdout
    # refused before any model is looked for (no GPU is touched here)
    base = [CLI, "-m", str(tmp_path / "no-such-model"), "--save-codes", str(tmp_path / "codes.txt")]
    r = subprocess.run(base + ["--encode", str(tmp_path / "a.wav"), "--encode-chunk", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--encode-chunk MS (MS >= 1) goes with --encode" in r.stderr and "Usage:" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--tokens", "1,2,3", "--encode-chunk", "200"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--encode-chunk MS (MS >= 1) goes with --encode" in r.stderr and "Usage:" in r.stderr, r.stdout + r.stderr
