"""The surface of batched vocoder streaming, checkable without a GPU: the three C-ABI entry points are declared in include/q3tts.h,
listed in q3tts.EXPORTS and exported by the built library; the Python binding and TTSEngine carry their callers; the library's device
code holds the new kernels.  (What they compute is checked on the GPU: tests/test_gpu_stream_batch.py.)"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW = ("q3tts_codec_stream_push_batch_host", "q3tts_slots_codec_decode_new_host", "q3tts_synthesize_stream_host")


def test_entry_points_declared_listed_and_exported():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(q3tts_engine\* e," % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"typedef int \(\*q3tts_audio_cb\)\(void\* user, int utt, int frame_begin, int frame_end, const float\* pcm, int64_t n_samples, int finished\);", hdr)
    # no engine: refused like every other entry point, nothing is touched
    n = ctypes.c_int64(7)
    assert L.q3tts_codec_stream_push_batch_host(None, 1, None, None, None, None, ctypes.c_int64(0), ctypes.byref(n)) == -1 and n.value == 7
    assert L.q3tts_slots_codec_decode_new_host(None, 1, None, None, ctypes.c_int64(0), None, None, None) == -1


def test_callers_exist():
    import q3tts
    for m in ("codec_stream_push_batch", "slots_codec_decode_new", "synthesize_stream"):
        assert callable(getattr(q3tts.Engine, m)), m
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"synthesize_tokens_batch_streaming\(const std::vector<std::vector<int64_t>>& token_ids, Language lang, const SamplingParams& params,\s*int chunk_frames,", h)
    assert "synthesize_tokens_streaming(" in h   # the single-utterance method stays


def test_library_holds_the_stream_kernels():
    """The windowed attention's sibling and the four descriptor-driven row kernels are in the gfx950 code object, none with a scratch
    segment; the sibling asks for k_attn_win's LDS (it is the same tile)."""
    import q3tts
    from kernel_resources import kernel_table
    rows = {name.split("(")[0]: (scratch, lds) for name, vgpr, agpr, sgpr, scratch, lds in kernel_table(q3tts.LIB_PATH)}
    for k in ("k_attn_win_streams", "k_code_embed_mean_streams", "k_rope_store_streams", "k_rmsnorm_rows_streams",
              "k_gather_stream_rows"):
        hit = [v for name, v in rows.items() if k in name]
        assert len(hit) == 1, (k, hit)
        assert hit[0][0] == 0, (k, hit)
    win = [v for name, v in rows.items() if "k_attn_win<" in name or name.endswith("k_attn_win")]
    sib = [v for name, v in rows.items() if "k_attn_win_streams" in name]
    assert len(win) == 1 and win[0][1] == sib[0][1], (win, sib)
