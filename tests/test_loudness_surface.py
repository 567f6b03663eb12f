"""The surface of the loudness stage, checkable without a GPU: every new symbol is declared in the header, exported by the library,
listed in q3tts.EXPORTS and bound by a Python wrapper; an entry point without an engine is refused like every other; out-of-range
parameters are refused with the value named; the header holds the arithmetic; the kernel is in the code object without scratch;
TTSEngine and the CLI name the stage."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_loudness_coeffs", "q3tts_loudness_emitted", "q3tts_loudness_lufs", "q3tts_loudness_last_error", "q3tts_loudness_begin",
       "q3tts_loudness_push_batch_host", "q3tts_loudness_end", "q3tts_codec_stream_set_loudness", "q3tts_engine_set_loudness")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_loudness_coeffs\(int32_t rate, double out\[10\]\);", hdr)
    assert re.search(r"int64_t q3tts_loudness_emitted\(int32_t target_dlufs, int64_t n_received, int finished\);", hdr)
    assert re.search(r"double q3tts_loudness_lufs\(const int64_t\* E, int64_t n, int mode\);", hdr)
    assert re.search(r"int q3tts_loudness_begin\(q3tts_engine\* e, int32_t target_dlufs, int32_t range_cb, int32_t start_cb, int\* id\);", hdr)


def test_header_holds_the_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for formula in ("f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196", "Vb = Vh^0.4996667741545416",
                    "f0 = 38.13547087602444, Q = 0.5003270373238773", "ff = (b0 x[k] + b1 x[k-1]) + b2 x[k-2], u[k] = (ff - a2 u[k-2]) - a1 u[k-1]",
                    "q[k] = (int64)floor((z < 4.0 ? z : 4.0) 2^32)", "W_b >= 4834272", "P = (double)A / ((double)N 41231686041600.0)",
                    "G_b = min(max(T, G_{b-1} DN), G_{b-1} UP)", "y[k] = x[k] (G_{b-1} + (G_b - G_{b-1}) ((float)i / 2400.0f))",
                    "E(R) = 2400 floor(R / 2400)", "vocoder -> pitch -> stretcher -> loudness -> level -> sink", "The latency is 100 ms"):
        assert formula in hdr, formula


def test_no_engine_is_refused():
    L = ctypes.CDLL(q3tts.LIB_PATH)
    i64 = ctypes.c_int64
    assert L.q3tts_loudness_begin(None, -160, 200, 0, None) == -1
    assert L.q3tts_loudness_push_batch_host(None, 1, None, None, None, None, None, i64(0), None, None, None, None) == -1
    assert L.q3tts_loudness_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_loudness(None, 0, -160, 200, 0) == -1
    assert L.q3tts_engine_set_loudness(None, 1, -160, 200, 0) == -1


def test_out_of_range_parameters_are_refused_with_the_value_named():
    """the host helpers run the stage's own parameter check (q3tts_loudness_emitted on its target); range and start gain need an engine:
    tests/test_gpu_loudness.py"""
    for bad in (-401, -49, 5, -1000):
        with pytest.raises(ValueError, match="target %d " % bad):
            q3tts.loudness_emitted(bad, 2400)
    for ok in (-400, -50, 0):
        assert q3tts.loudness_emitted(ok, 2400) == 2400
    with pytest.raises(ValueError, match="-7"):
        q3tts.loudness_emitted(-160, -7)
    with pytest.raises(ValueError, match="7999"):
        q3tts.loudness_coeffs(7999)
    with pytest.raises(ValueError, match="mode 5"):
        q3tts.loudness_lufs([1, 2, 3, 4], 5)


def test_python_wrappers():
    assert q3tts.loudness_emitted(-160, 5000) == 4800 and q3tts.loudness_emitted(-160, 5000, True) == 5000 and q3tts.loudness_emitted(0, 5000) == 5000
    Lb = q3tts.lib()
    assert Lb.q3tts_loudness_emitted.argtypes == [ctypes.c_int32, ctypes.c_int64, ctypes.c_int] and Lb.q3tts_loudness_emitted.restype == ctypes.c_int64
    assert Lb.q3tts_loudness_lufs.restype == ctypes.c_double
    for name in ("loudness_begin", "loudness_push_batch", "loudness_end", "codec_stream_set_loudness", "set_loudness"):
        assert callable(getattr(q3tts.Engine, name)), name
    for fn in (q3tts.Engine.codec_stream_begin, q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        assert "loudness" in inspect.signature(fn).parameters, fn
    assert {"loudness_range", "loudness_start"} <= set(inspect.signature(q3tts.Engine.codec_stream_begin).parameters)


def test_kernel_is_in_the_code_object_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_table
    rows = {name.split("(")[0]: (scratch, lds) for name, vgpr, agpr, sgpr, scratch, lds in kernel_table(q3tts.LIB_PATH)}
    hit = [k for k in rows if "k_loudness" in k]
    assert len(hit) == 1, sorted(rows)
    scratch, lds = rows[hit[0]]
    assert scratch == 0 and 0 < lds <= 65536, (scratch, lds)


def test_tts_engine_and_cli_name_the_stage():
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_loudness\(float lufs", th)
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--loudness LUFS" in r.stdout and "--loudness-range DB" in r.stdout
