"""The surface of encoder streams at the source's own rate, checkable without a GPU: the new C-ABI entry points in include/q3tts.h,
q3tts.EXPORTS and the built library, their ctypes signatures, the Python keyword arguments, TTSEngine's overloads and the CLI's help.
What they compute is checked on the GPU: tests/test_gpu_audio_stream_rate.py; the host rule in tests/test_cpu_resample_stream.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_audio_stream_begin_rate", "q3tts_audio_stream_format", "q3tts_audio_stream_push_any_host", "q3tts_audio_stream_push_batch_any_host")
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert "q3tts_resample_stream_emitted" in q3tts.EXPORTS and hasattr(L, "q3tts_resample_stream_emitted")
    assert re.search(r"int64_t q3tts_resample_stream_emitted\(int32_t src_rate, int32_t dst_rate, int64_t n_received, int finish\);", hdr)
    assert re.search(r"int q3tts_audio_stream_begin_rate\(q3tts_engine\* e, int32_t sample_rate, int format, int64_t max_samples, int\* stream_id\);", hdr)
    assert re.search(r"int q3tts_audio_stream_format\(q3tts_engine\* e, int stream_id, int32_t\* sample_rate, int\* format\);", hdr)
    assert re.search(r"int q3tts_audio_stream_push_any_host\(q3tts_engine\* e, int stream_id, const void\* pcm, int64_t n_samples, int finish,", hdr)
    assert re.search(r"int q3tts_audio_stream_push_batch_any_host\(q3tts_engine\* e, int n_streams, const int32_t\* stream_ids, const void\* const\* pcm,", hdr)
    assert re.search(r"#define Q3TTS_PCM_F32 0\b", hdr) and re.search(r"#define Q3TTS_PCM_S16 1\b", hdr)
    assert (q3tts.PCM_F32, q3tts.PCM_S16) == (0, 1)
    # the section states the new promise and both emission conditions, and no longer sends the caller away to resample
    sec = hdr[hdr.index("carried-state pushes"):hdr.index("int q3tts_audio_stream_end(")]
    assert "is the caller's to resample" not in hdr and "serves whole clips only" not in hdr
    assert "bit-identical to q3tts_audio_encode_batch_host" in sec and "v / 32768.0f" in sec
    assert "floor(i / ratio) + 1 <= N - 1" in sec and "i < floor(N * ratio)" in sec and "Latency" in sec
    # no engine: refused like every other entry point; the host rule needs none
    i64 = ctypes.c_int64
    assert L.q3tts_audio_stream_begin_rate(None, 16000, 1, i64(0), None) == -1
    assert L.q3tts_audio_stream_format(None, 0, None, None) == -1
    assert L.q3tts_audio_stream_push_any_host(None, 0, None, i64(0), 0, None, 0, None) == -1
    assert L.q3tts_audio_stream_push_batch_any_host(None, 1, None, None, None, None, None, None, None, None) == -1
    L.q3tts_resample_stream_emitted.restype = i64
    assert L.q3tts_resample_stream_emitted(16000, 24000, i64(1000), 1) == 1500
    assert L.q3tts_resample_stream_emitted(0, 24000, i64(1000), 1) == -1


def test_ctypes_signatures():
    import q3tts
    L = q3tts.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.q3tts_audio_stream_begin_rate.argtypes == [vp, i32, i32, i64, ctypes.POINTER(ctypes.c_int)]
    assert L.q3tts_audio_stream_format.argtypes == [vp, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]
    assert L.q3tts_audio_stream_push_any_host.argtypes == [vp, i32, vp, i64, i32, vp, i32, ctypes.POINTER(ctypes.c_int32)]
    assert len(L.q3tts_audio_stream_push_batch_any_host.argtypes) == 10
    assert L.q3tts_resample_stream_emitted.argtypes == [i32, i32, i64, i32] and L.q3tts_resample_stream_emitted.restype == i64


def test_python_keyword_arguments():
    import q3tts
    E = q3tts.Engine
    # the 24 kHz callers keep their signatures (tests/test_audio_stream_surface.py pins them); rate and sample format have callers of their own
    sig = inspect.signature(E.audio_stream_begin_rate).parameters
    assert list(sig) == ["self", "sample_rate", "dtype", "max_samples"]
    assert (sig["dtype"].default, sig["max_samples"].default) == ("float32", 0)
    sig = inspect.signature(E.audio_encode_long_rate).parameters
    assert list(sig) == ["self", "pcm", "sample_rate", "chunk_samples"]
    sig = inspect.signature(q3tts.AudioEncodeStream.__init__).parameters
    assert list(sig) == ["self", "engine", "max_samples", "sample_rate", "dtype"]
    assert (sig["sample_rate"].default, sig["dtype"].default) == (24000, "float32")
    assert callable(E.audio_stream_format)
    assert list(inspect.signature(q3tts.resample_stream_emitted).parameters) == ["src_rate", "dst_rate", "n_received", "finish"]
    assert q3tts.resample_stream_emitted(96000, 24000, 2) == 0 and q3tts.resample_stream_emitted(96000, 24000, 3, True) == 0
    with pytest.raises(ValueError, match="dtype must be float32 or int16"):
        q3tts._pcm_format("int32")
    assert q3tts._pcm_format(np.int16) == q3tts.PCM_S16 and q3tts._pcm_format("float32") == q3tts.PCM_F32


def test_tts_engine_declares_rate_and_int16():
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"int audio_stream_begin\(int64_t max_samples, int sample_rate", h)
    assert re.search(r"std::vector<int64_t> audio_stream_push\(int id, const int16_t\* pcm, size_t n, bool finish = false", h)


def test_cli_help_and_source_no_longer_resample_on_the_host():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if "--encode-chunk MS" in l]
    assert line and "own rate" in line[0] and "24 kHz file" not in line[0], r.stdout
    src = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "main.cpp")).read()
    assert "read_wav_24k" not in src and "q3tts_resample_host" not in src
