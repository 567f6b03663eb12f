"""The surface of live text input, checkable without a GPU: the C-ABI entry points in include/q3tts.h, q3tts.EXPORTS and the built
library, SlotState's size (text_open took the place of its padding word), the Python wrappers' parameters, TTSEngine's method and the CLI
flag.  What they compute is checked on the GPU: tests/test_gpu_live_text.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc")
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
NEW = ("q3tts_slot_text_open", "q3tts_slot_text_append_host", "q3tts_slots_text_append_ids", "q3tts_slot_text_status",
       "q3tts_build_prompt_open_host", "q3tts_synthesize_live_host")


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_slot_text_open\(q3tts_engine\* e, int slot\);", hdr)
    assert re.search(r"int q3tts_slot_text_append_host\(q3tts_engine\* e, int slot, const float\* rows, int n_rows, int close\);", hdr)
    assert re.search(r"int q3tts_slots_text_append_ids\(q3tts_engine\* e, int n, const int32_t\* slots, const int64_t\* ids, const int32_t\* offsets, "
                     r"const uint8_t\* close\);", hdr)
    assert re.search(r"int q3tts_slot_text_status\(q3tts_engine\* e, int slot, int\* n_text_rows, int\* open, int\* starved\);", hdr)
    assert re.search(r"int q3tts_build_prompt_open_host\(q3tts_engine\* e, const int64_t\* ids, int n_ids, int lang, const float\* speaker,\s*"
                     r"float\* prompt, int\* S, float\* trailing, int cap_rows, int\* n_trailing\);", hdr)
    assert re.search(r"typedef int \(\*q3tts_text_cb\)\(void\* user, int utt, int64_t\* ids, int cap, int32_t\* n, int32_t\* closed\);", hdr)
    assert re.search(r"int q3tts_synthesize_live_host\(q3tts_engine\* e, int n_utt, q3tts_text_cb text_cb, void\* text_user, int lang,", hdr)
    # each entry's comment cites the reference lines it rests on
    assert hdr.count("tts_onnx.cpp:531-536") >= 5 and hdr.count(":833-842") >= 6
    assert "q3tts_slot_text_status" in hdr[hdr.index("a stalled slot never reaches max_frames"):][:200]
    # no engine: refused like every other entry point
    assert L.q3tts_slot_text_open(None, 0) == -1
    assert L.q3tts_slot_text_append_host(None, 0, None, 0, 1) == -1
    assert L.q3tts_slots_text_append_ids(None, 0, None, None, None, None) == -1
    assert L.q3tts_slot_text_status(None, 0, None, None, None) == -1
    assert L.q3tts_build_prompt_open_host(None, None, 4, 0, None, None, None, None, 0, None) == -1
    assert L.q3tts_synthesize_live_host(None, 1, None, None, 0, None, None, None, ctypes.c_uint64(0), 0, None, ctypes.c_int64(0), None, None, None,
                                        1, None, None) == -1


def test_slot_state_keeps_its_size_and_names_the_flag():
    """text_open replaced the padding word: the sampler still reads the struct as four 16-byte loads (the build's static_assert)"""
    src = open(os.path.join(CSRC, "q3_common.h")).read()
    body = src[src.index("struct SlotState {"):]
    body = body[: body.index("};")]
    assert "uint32_t text_open;" in body and "pad1" not in body
    assert 'static_assert(sizeof(SlotState) == 64, "SlotState must be 64 bytes");' in src
    words = {"int32_t": 4, "uint32_t": 4, "float": 4, "uint64_t": 8}
    size = 0
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*(int32_t|uint32_t|uint64_t|float)\s+([^;]+);", line)
        if m:
            size += words[m.group(1)] * len(m.group(2).split(","))
    assert size == 64


def test_python_wrappers_and_cli():
    import q3tts
    E = q3tts.Engine
    assert list(inspect.signature(E.slot_text_open).parameters) == ["self", "slot"]
    ps = inspect.signature(E.slot_text_append).parameters
    assert list(ps) == ["self", "slot", "rows", "ids", "close"] and ps["rows"].default is None and ps["ids"].default is None and ps["close"].default is False
    assert list(inspect.signature(E.slots_text_append_ids).parameters)[:3] == ["self", "slots", "id_lists"]
    assert list(inspect.signature(E.slot_text_status).parameters) == ["self", "slot"]
    assert list(inspect.signature(E.build_prompt_open).parameters)[:2] == ["self", "ids"]
    ps = inspect.signature(E.synthesize_live).parameters
    assert list(ps)[:6] == ["self", "n_utt", "text_source", "sp", "chunk_frames", "on_audio"]
    with pytest.raises(ValueError, match="rows or ids"):
        E.slot_text_append(object(), 0, rows=np.zeros((1, 4)), ids=[1])
    with pytest.raises(ValueError, match="one entry per slot"):
        E.slots_text_append_ids(object(), [0, 1], [[1]])
    h = open(os.path.join(CSRC, "tts_engine.h")).read()
    assert re.search(r"std::vector<int> synthesize_tokens_live\(int n_utt,", h)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and re.search(r"^\s+--feed K", r.stdout, re.M), r.stdout
    # --feed needs --stream-chunk: refused before the model is looked for
    r = subprocess.run([CLI, "-m", "x", "--tokens", "1,2,3", "--feed", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--feed K (K >= 1) needs --stream-chunk" in r.stderr
