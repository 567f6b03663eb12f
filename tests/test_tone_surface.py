"""The surface of the tone stage, checkable without a GPU: every new symbol is declared in the header, exported by the library, listed
in q3tts.EXPORTS and bound by a Python wrapper; an entry point without an engine is refused like every other; the header holds the
arithmetic and the six-stage order; the kernel is in the code object without scratch; TTSEngine and the CLI name the stage."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_tone_coeffs", "q3tts_tone_parse", "q3tts_tone_last_error", "q3tts_tone_begin", "q3tts_tone_push_batch_host", "q3tts_tone_end",
       "q3tts_codec_stream_set_tone", "q3tts_engine_set_tone")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert "typedef struct { int32_t kind, freq_hz, gain_cb, q_permille; } q3tts_tone_section;" in hdr
    for kind, v in (("HIGHPASS", 1), ("LOWPASS", 2), ("LOWSHELF", 3), ("HIGHSHELF", 4), ("PEAK", 5)):
        assert re.search(r"#define Q3TTS_TONE_%s %d\b" % (kind, v), hdr), kind
    assert re.search(r"int q3tts_tone_coeffs\(int32_t n, const q3tts_tone_section\* sections, double \(\*out\)\[5\]\);", hdr)
    assert re.search(r"int q3tts_tone_begin\(q3tts_engine\* e, int32_t n, const q3tts_tone_section\* sections, int\* id\);", hdr)
    assert re.search(r"int q3tts_codec_stream_set_tone\(q3tts_engine\* e, int stream_id, int32_t n, const q3tts_tone_section\* sections\);", hdr)


def test_header_holds_the_arithmetic_and_the_order():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for formula in ("vocoder -> pitch -> stretcher -> tone -> loudness -> level -> sink", "alpha = sin(w0) / (2 Q)", "A = 10^(gain_dB / 40)",
                    "s_0[k] = (double)x[k]", "ff = (b0 s_{j-1}[k] + b1 s_{j-1}[k-1]) + b2 s_{j-1}[k-2], s_j[k] = (ff - a2 s_j[k-2]) - a1 s_j[k-1]",
                    "y[k] = (float)s_n[k]", "nothing is rounded\n *    to float between sections", "all history is zero before sample 0", "subnormals are kept",
                    "a stage that has received N samples has emitted N", "finish flushes nothing", "(n + 1) * 2 in all",
                    "b = (1 + alpha A, -2 c, 1 - alpha A), a = (1 + alpha / A, -2 c, 1 - alpha / A)", "starts from\n * zero history"):
        assert formula in hdr, formula
    # the older sections keep their sentences
    assert "vocoder -> pitch -> stretcher -> loudness -> level -> sink" in hdr


def test_no_engine_is_refused():
    L = ctypes.CDLL(q3tts.LIB_PATH)
    i64 = ctypes.c_int64
    sec = (ctypes.c_int32 * 4)(1, 300, 0, 707)
    assert L.q3tts_tone_begin(None, 1, sec, None) == -1
    assert L.q3tts_tone_push_batch_host(None, 1, None, None, None, None, None, i64(0), None) == -1
    assert L.q3tts_tone_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_tone(None, 0, 1, sec) == -1
    assert L.q3tts_engine_set_tone(None, 1, sec) == -1
    L.q3tts_tone_last_error.restype = ctypes.c_char_p
    assert L.q3tts_tone_coeffs(1, sec, None) == -1 and b"NULL" in L.q3tts_tone_last_error()
    assert L.q3tts_tone_parse(None, None, None) == -1 and b"NULL" in L.q3tts_tone_last_error()


def test_python_wrappers():
    assert q3tts.tone_coeffs("rumble").shape == (1, 5) and q3tts.tone_sections("rumble").shape == (1, 4)
    assert q3tts.TONE_KINDS == {"highpass": 1, "lowpass": 2, "lowshelf": 3, "highshelf": 4, "peak": 5}
    for name in ("tone_begin", "tone_push_batch", "tone_end", "codec_stream_set_tone", "set_tone"):
        assert callable(getattr(q3tts.Engine, name)), name
    for fn in (q3tts.Engine.codec_stream_begin, q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        assert "tone" in inspect.signature(fn).parameters, fn


def test_kernel_is_in_the_code_object_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_table
    rows = {name.split("(")[0]: (scratch, lds) for name, vgpr, agpr, sgpr, scratch, lds in kernel_table(q3tts.LIB_PATH)}
    hit = [k for k in rows if "k_tone" in k]
    assert len(hit) == 1, sorted(rows)
    scratch, lds = rows[hit[0]]
    assert scratch == 0 and 0 < lds <= 65536, (scratch, lds)


def test_tts_engine_and_cli_name_the_stage():
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_tone\(const char\* spec\)", th)
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--eq SPEC" in r.stdout and "telephone" in r.stdout
