"""The surface of the pitch stage, checkable without a GPU: every new symbol is declared in the header, exported by the library, listed
in q3tts.EXPORTS and bound by a Python wrapper; an entry point without an engine is refused like every other; the header holds the
arithmetic in full; the new keywords come last; TTSEngine and the CLI name the stage."""
import ctypes
import inspect
import os
import re
import subprocess

import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_pitch_ratio", "q3tts_pitch_emitted", "q3tts_pitch_last_error", "q3tts_pitch_begin", "q3tts_pitch_push_batch_host",
       "q3tts_pitch_end", "q3tts_codec_stream_set_pitch", "q3tts_engine_set_pitch")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int32_t q3tts_pitch_ratio\(double cents\);", hdr)
    assert re.search(r"int64_t q3tts_pitch_emitted\(int64_t n_received, int finished\);", hdr)
    assert re.search(r"int q3tts_pitch_begin\(q3tts_engine\* e, int32_t ratio_permille, int\* id\);", hdr)
    assert re.search(r"int q3tts_codec_stream_set_pitch\(q3tts_engine\* e, int stream_id, int32_t ratio_permille\);", hdr)
    assert re.search(r"int q3tts_engine_set_pitch\(q3tts_engine\* e, int32_t ratio_permille\);", hdr)


def test_header_holds_the_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for formula in ("Pmin = 48, Pmax = 400, Pu = 120, W = 240", "VOICED2 = 0.25f, OCTAVE2 = 0.81f", "FLOOR = 0.0625f", "F = 20 fraction bits",
                    "a_0 = 0, a_{j+1} = a_j + P_j", "score(L) = den > 0 ? (num * |num|) / den : 0", "score(L) >= score(L - 1) and score(L) >= score(L + 1)",
                    "the SMALLEST candidate with score >= OCTAVE2 * best", "s_{i+1} = s_i + ((P_j * 1000) << F) / r", "the later of two",
                    "h[m] = (float)(0.5 - 0.5 cos(pi m / P_j))", "y[k] = acc[k] / (wsum[k] > FLOOR ? wsum[k] : FLOOR)",
                    "E(R) = max(0, R - LA), LA = Pmax + GATE - 1 = 1240", "vocoder -> pitch -> stretcher -> level -> sink", "like the other stages"):
        assert formula in hdr, formula


def test_no_engine_is_refused():
    L = ctypes.CDLL(q3tts.LIB_PATH)
    i64 = ctypes.c_int64
    assert L.q3tts_pitch_begin(None, 1260, None) == -1
    assert L.q3tts_pitch_push_batch_host(None, 1, None, None, None, None, None, i64(0), None) == -1
    assert L.q3tts_pitch_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_pitch(None, 0, 1260) == -1
    assert L.q3tts_engine_set_pitch(None, 1260) == -1


def test_python_wrappers():
    assert q3tts.pitch_ratio(-200) == 891 and q3tts.pitch_emitted(5000) == 3760 and q3tts.pitch_emitted(5000, True) == 5000
    Lb = q3tts.lib()
    assert Lb.q3tts_pitch_ratio.argtypes == [ctypes.c_double] and Lb.q3tts_pitch_ratio.restype == ctypes.c_int32
    assert Lb.q3tts_pitch_emitted.argtypes == [ctypes.c_int64, ctypes.c_int] and Lb.q3tts_pitch_emitted.restype == ctypes.c_int64
    for name in ("pitch_begin", "pitch_push_batch", "pitch_end", "codec_stream_set_pitch", "set_pitch"):
        assert callable(getattr(q3tts.Engine, name)), name
    for fn in (q3tts.Engine.codec_stream_begin, q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        par = list(inspect.signature(fn).parameters)
        assert par[-1] == "pitch", fn                       # new keywords go last: existing calls are unchanged


def test_tts_engine_and_cli_name_the_stage():
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_pitch\(float semitones\);", th)
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pitch ST" in r.stdout
