"""The surface of the shared prompt prefix (run_prefill, reference src/tts_onnx.cpp:615-665, once for rows many utterances have in
front of their prompts), checkable without a GPU: the C-ABI entries in include/q3tts.h, the built library, q3tts.EXPORTS, the Python
callers and TTSEngine's method.  (What they compute is checked on the GPU: tests/test_gpu_prefix.py.)"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_prefix_create", "q3tts_prefix_create_instruct", "q3tts_prefix_info", "q3tts_prefix_release",
       "q3tts_slot_begin_prefixed", "q3tts_slots_begin_prefixed", "q3tts_synthesize_prefixed_host")


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(q3tts_engine\* e," % name, hdr), name
    assert re.search(r"int q3tts_prefix_create\(q3tts_engine\* e, const float\* rows, int n_rows, int\* prefix_id\);", hdr)
    assert re.search(r"int q3tts_prefix_create_instruct\(q3tts_engine\* e, const int64_t\* framed_ids, int n, int\* prefix_id\);", hdr)
    assert re.search(r"int q3tts_prefix_info\(q3tts_engine\* e, int prefix_id, int\* n_rows, int64_t\* bytes\);", hdr)
    assert re.search(r"int q3tts_prefix_release\(q3tts_engine\* e, int prefix_id\);", hdr)
    assert re.search(r"int q3tts_slot_begin_prefixed\(q3tts_engine\* e, int slot, int prefix_id, const float\* prompt, int S, const float\* trailing, int n_trailing,\s*"
                     r"const int64_t\* prefix_codes, int n_prefix_frames, const q3tts_sampling\* p, uint64_t seed, uint32_t stream_id, int ignore_eos\);", hdr)
    assert re.search(r"int q3tts_slots_begin_prefixed\(q3tts_engine\* e, int n, const int32_t\* slots, const int32_t\* prefix_ids, const float\* const\* prompts, "
                     r"const int32_t\* S,", hdr)
    assert re.search(r"int chunk_frames, q3tts_audio_cb cb, void\* user, const int32_t\* prefix_ids\);", hdr)
    assert hdr.count("tts_onnx.cpp:615-665") >= 7          # every new entry cites run_prefill


def test_library_exports_and_refuses_a_null_engine():
    import q3tts
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    pid = ctypes.c_int(7)
    assert L.q3tts_prefix_create(None, None, 4, ctypes.byref(pid)) == -1 and pid.value == 7
    assert L.q3tts_prefix_create_instruct(None, None, 4, ctypes.byref(pid)) == -1 and pid.value == 7
    assert L.q3tts_prefix_info(None, 0, None, None) == -1
    assert L.q3tts_prefix_release(None, 0) == -1
    assert L.q3tts_slots_begin_prefixed(None, 1, None, None, None, None, None, None, None, ctypes.c_uint64(0), None, 0) == -1


def test_python_surface():
    import q3tts
    for name in NEW:
        assert name in q3tts.EXPORTS, name
    for m in ("prefix_create", "prefix_create_instruct", "prefix_info", "prefix_release", "slots_begin_prefixed", "synthesize_prefixed"):
        assert callable(getattr(q3tts.Engine, m)), m
    assert "prefix_id" in inspect.signature(q3tts.Engine.slot_begin).parameters
    sb = inspect.signature(q3tts.Engine.synthesize_batch).parameters
    assert "share_instructs" in sb and sb["share_instructs"].default is False


def test_tts_engine_method():
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"synthesize_tokens_batch_instruct_shared\(", h)
