"""The surface of voice instructions (the reference README's roadmap row "Voice instructions (--instruct)"), checkable without a GPU:
the chat-turn framing of an instruction, the three C-ABI entry points in include/q3tts.h, q3tts.EXPORTS and the built library, the
Python callers, TTSEngine's methods and the CLI flags.  (What they compute is checked on the GPU: tests/test_gpu_long_prefill.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_build_prompt_instruct_host", "q3tts_frame_instruct_ids", "q3tts_synthesize_instruct_host")
HEAD, TAIL = [151644, 872, 198], [151645, 198]   # <|im_start|> user \n ... <|im_end|> \n


def test_frame_instruct_ids():
    import q3tts
    L = ctypes.CDLL(q3tts.LIB_PATH)
    L.q3tts_frame_instruct_ids.restype = ctypes.c_int64
    L.q3tts_frame_instruct_ids.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    text = np.array([11, 22, 33, 44, 55], np.int32)
    for ids in (text[:0], text):
        want = HEAD + [int(v) for v in ids] + TAIL
        ptr = ids.ctypes.data_as(ctypes.c_void_p) if ids.size else None
        assert L.q3tts_frame_instruct_ids(ptr, ids.size, None, 0) == len(want)          # cap = 0 sizes
        out = np.full(len(want) + 2, -7, np.int64)
        assert L.q3tts_frame_instruct_ids(ptr, ids.size, out.ctypes.data_as(ctypes.c_void_p), len(want)) == len(want)
        assert out[: len(want)].tolist() == want and out[len(want):].tolist() == [-7, -7]
        short = np.full(4, -7, np.int64)                                                   # a short buffer is filled, never overrun
        assert L.q3tts_frame_instruct_ids(ptr, ids.size, short.ctypes.data_as(ctypes.c_void_p), 3) == len(want)
        assert short.tolist() == want[:3] + [-7]
        assert q3tts.frame_instruct_ids(ids).tolist() == want
    assert q3tts.frame_instruct_ids(text).dtype == np.int64
    assert L.q3tts_frame_instruct_ids(None, 3, None, 0) == -1 and L.q3tts_frame_instruct_ids(None, -1, None, 0) == -1


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_build_prompt_instruct_host\(q3tts_engine\* e, const int64_t\* ids, int n_ids, int lang, const float\* speaker,\s*"
                     r"const int64_t\* instruct_ids, int n_instruct,\s*float\* prompt, int cap_prompt_rows, int\* S, float\* trailing, int cap_rows, int\* n_trailing\);", hdr)
    assert re.search(r"int64_t q3tts_frame_instruct_ids\(const int32_t\* text_ids, int64_t n, int64_t\* out, int64_t cap\);", hdr)
    assert re.search(r"q3tts_audio_cb cb, void\* user,\s*const int64_t\* instruct_ids, const int32_t\* instruct_offsets\);", hdr)
    assert "[HINT], unpinned" in hdr and "1 <= S <= max_ctx" in hdr
    # no engine: refused like every other entry point
    s = ctypes.c_int(5)
    assert L.q3tts_build_prompt_instruct_host(None, None, 0, 0, None, None, 0, None, 0, ctypes.byref(s), None, 0, None) == -1 and s.value == 5
    assert L.q3tts_synthesize_instruct_host(None, 1, None, None, 0, None, None, None, ctypes.c_uint64(0), 0, None, ctypes.c_int64(0), None, None, None,
                                            0, None, None, None, None) == -1
    # the Python callers
    import inspect
    assert "instruct_ids" in inspect.signature(q3tts.Engine.build_prompt).parameters
    assert "instructs" in inspect.signature(q3tts.Engine.synthesize_batch).parameters
    assert "instructs" in inspect.signature(q3tts.Engine.synthesize_stream).parameters
    assert callable(q3tts.frame_instruct_ids)
    # TTSEngine: beside the reference's methods, which stay
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"synthesize_instruct\(const std::string& text, const std::string& instruct, Language lang", h)
    assert re.search(r"synthesize_instruct\(const std::string& text, const std::string& instruct, const std::vector<float>& speaker_embed,", h)
    assert "synthesize_clone(const std::string& text, const std::string& ref_audio_path," in h
    # the command line names both flags
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert re.search(r"^\s+--instruct TEXT", r.stdout, re.M) and re.search(r"^\s+--instruct-tokens IDS", r.stdout, re.M), r.stdout
