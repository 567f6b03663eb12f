"""The surface of the output-level stage, checkable without a GPU: every new symbol is declared in the header, exported by the library,
listed in q3tts.EXPORTS and bound by a Python wrapper; an entry point without an engine is refused like every other; the header holds
the arithmetic in full; TTSEngine and the CLI name the stage."""
import ctypes
import inspect
import os
import re
import subprocess

import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_level_gain", "q3tts_level_emitted", "q3tts_level_last_error", "q3tts_level_begin", "q3tts_level_push_batch_host",
       "q3tts_level_end", "q3tts_codec_stream_set_level", "q3tts_engine_set_level")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"float q3tts_level_gain\(int32_t gain_cb\);", hdr)
    assert re.search(r"int64_t q3tts_level_emitted\(int32_t gain_cb, int32_t ceiling_permille, int64_t n_received, int finished\);", hdr)
    assert re.search(r"int q3tts_level_begin\(q3tts_engine\* e, int32_t gain_cb, int32_t ceiling_permille, int\* id\);", hdr)
    assert re.search(r"int q3tts_codec_stream_set_level\(q3tts_engine\* e, int stream_id, int32_t gain_cb, int32_t ceiling_permille\);", hdr)
    assert re.search(r"int q3tts_engine_set_level\(q3tts_engine\* e, int32_t gain_cb, int32_t ceiling_permille\);", hdr)


def test_header_holds_the_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for formula in ("g = 10^(gain_cb / 200)", "r[k] = (a[k] > T) ? T / a[k] : 1.0f", "m[k] = min(r[k], .., r[k + 127])",
                    "q[k] = (int32)floor(m[k] * 65536.0f)", "S[k] = q[k] + q[k - 1] + .. + q[k - 127]", "s[k] = (float)S[k] * 2^-23",
                    "y[k] = min(max(v[k] * s[k], -T), T)", "E(R) = max(0, R - 127)", "r = 1 history", "overshoot"):
        assert formula in hdr, formula


def test_no_engine_is_refused():
    L = ctypes.CDLL(q3tts.LIB_PATH)
    i64 = ctypes.c_int64
    assert L.q3tts_level_begin(None, 60, 900, None) == -1
    assert L.q3tts_level_push_batch_host(None, 1, None, None, None, None, None, i64(0), None) == -1
    assert L.q3tts_level_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_level(None, 0, 60, 900) == -1
    assert L.q3tts_engine_set_level(None, 60, 900) == -1


def test_python_wrappers():
    q3tts.level_gain(60)
    q3tts.level_emitted(60, 900, 10)
    Lb = q3tts.lib()
    assert Lb.q3tts_level_gain.argtypes == [ctypes.c_int32] and Lb.q3tts_level_gain.restype == ctypes.c_float
    assert Lb.q3tts_level_emitted.argtypes == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int]
    assert Lb.q3tts_level_emitted.restype == ctypes.c_int64
    for name in ("level_begin", "level_push_batch", "level_end", "codec_stream_set_level", "set_level"):
        assert callable(getattr(q3tts.Engine, name)), name
    for fn in (q3tts.Engine.codec_stream_begin, q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        par = inspect.signature(fn).parameters
        assert "gain_db" in par and "ceiling" in par, fn
    assert callable(q3tts.level_params)


def test_tts_engine_and_cli_name_the_stage():
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_level\(float gain_db, float ceiling\);", th)
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--gain" in r.stdout and "--limit" in r.stdout
