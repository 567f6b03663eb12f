"""The surface of the ragged prefill (q3tts_slots_begin_ragged, Q3TTS_FLAG_RAGGED_PREFILL; run_prefill, reference
src/tts_onnx.cpp:615-665, and the frame loop's rows, :824-842), checkable without a GPU: the C-ABI entry, the built library, the Python
binding, and the segment instantiations of the chunk attention in the code object.  (What they compute: tests/test_gpu_ragged_prefill.py.)"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_header_declares_the_entry_and_the_flag():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    assert re.search(r"int q3tts_slots_begin_ragged\(q3tts_engine\* e, int n, const int32_t\* slots, const int32_t\* prefix_ids, const float\* const\* prompts, "
                     r"const int32_t\* S,\s*const float\* const\* trailing, const int32_t\* n_trailing,\s*const int64_t\* const\* prefix_codes /\* entries may be NULL \*/, "
                     r"const int32_t\* n_prefix_frames,\s*const q3tts_sampling\* p, uint64_t seed, const uint32_t\* stream_ids, int ignore_eos\);", hdr)
    assert re.search(r"#define Q3TTS_FLAG_RAGGED_PREFILL 64u", hdr)
    comment = hdr[hdr.index("/* Ragged begin"):hdr.index("int q3tts_slots_begin_ragged")]
    for text in ("tts_onnx.cpp:615-665", ":824-842", "bit for bit", "2e-4", "4e-3", "all or nothing"):
        assert text in comment, text


def test_library_exports_and_argument_errors():
    import q3tts
    L = ctypes.CDLL(q3tts.LIB_PATH)
    assert hasattr(L, "q3tts_slots_begin_ragged")
    assert L.q3tts_slots_begin_ragged(None, 2, None, None, None, None, None, None, None, None, None, ctypes.c_uint64(0), None, 0) == -1


def test_python_surface():
    import q3tts
    C = ctypes
    assert "q3tts_slots_begin_ragged" in q3tts.EXPORTS
    assert q3tts.FLAG_RAGGED_PREFILL == 64
    assert callable(q3tts.Engine.slots_begin_ragged)
    L = q3tts.lib() if hasattr(q3tts, "lib") else None
    if L is not None:
        vp, i32 = C.c_void_p, C.c_int32
        at = list(L.q3tts_slots_begin_ragged.argtypes)
        assert len(at) == 14 and at[0] is vp and at[1] in (i32, C.c_int) and at[11] is C.c_uint64 and at[10] == C.POINTER(q3tts.Sampling)
        assert all(a is vp for a in at[2:10]) and at[12] is vp


def test_segment_kernels_are_in_the_code_object_without_scratch():
    import q3tts
    from kernel_resources import kernel_table
    rows = kernel_table(q3tts.LIB_PATH)
    att = [r for r in rows if "k_attn_prefill" in r[0]]
    app = [r for r in rows if "k_prefill_append" in r[0]]
    # the one-slot / group forms: (16, 64, 128) x (1, 2, 4) x (fp32, bf16) = 18 and 6; the segment forms: 64 x (1, 2, 4) + 128 x 2, x 2 caches = 8 and 4
    assert len(att) == 18 + 8, [r[0] for r in att]
    assert sum(r[0].endswith(", true>") for r in att) == 8 and sum(r[0].endswith(", true>") for r in app) == 4
    assert len(app) == 6 + 4, [r[0] for r in app]
    for name, vgpr, agpr, sgpr, scratch, lds in att + app:
        assert scratch == 0, (name, scratch)
        assert lds <= 57600 + 1024, (name, lds)          # the existing kernel's LDS at head_dim 128
    assert max(r[1] for r in att) <= 176, max(r[1] for r in att)   # the existing kernel's 169 VGPRs, not meaningfully more
