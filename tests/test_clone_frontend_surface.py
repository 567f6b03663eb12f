"""The surface of the GPU voice-clone front end, checkable without a GPU: the three C-ABI entry points are declared in
include/q3tts.h, listed in q3tts.EXPORTS and exported by the built library, the Python binding and TTSEngine carry their callers, and
the library's device code holds the two new kernels.  (What they compute is checked on the GPU: tests/test_gpu_clone_frontend.py.)"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW = ("q3tts_resample_gpu_host", "q3tts_mel_gpu_host", "q3tts_speaker_embed_pcm_batch_host")


def test_entry_points_declared_listed_and_exported():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(q3tts_engine\* e," % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    # no engine: refused like every other entry point, nothing is touched
    L.q3tts_resample_gpu_host.restype = ctypes.c_int64
    assert L.q3tts_resample_gpu_host(None, None, ctypes.c_int64(0), 16000, 24000, None, ctypes.c_int64(0)) == -1
    fr = ctypes.c_int32(5)
    assert L.q3tts_mel_gpu_host(None, None, ctypes.c_int64(0), 24000, None, ctypes.c_int64(0), ctypes.byref(fr)) == -1 and fr.value == 5
    assert L.q3tts_speaker_embed_pcm_batch_host(None, 1, None, None, None, None) == -1


def test_callers_exist():
    import q3tts
    for m in ("resample_gpu", "log_mel_gpu", "speaker_embeddings"):
        assert callable(getattr(q3tts.Engine, m)), m
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"extract_speaker_embedding\(const std::vector<float>& pcm, int sample_rate\)", h)
    assert re.search(r"extract_speaker_embedding\(const std::string& audio_path\)", h)


def test_library_holds_the_front_end_kernels():
    """k_resample_linear and k_logmel are in the gfx950 code object, without a scratch segment; the log-mel frame (padded complex
    frame + twiddles) is the LDS it asks for."""
    import q3tts
    from kernel_resources import kernel_table
    rows = {name.split("(")[0]: (scratch, lds) for name, vgpr, agpr, sgpr, scratch, lds in kernel_table(q3tts.LIB_PATH)}
    rs = [v for k, v in rows.items() if "k_resample_linear" in k]
    lm = [v for k, v in rows.items() if "k_logmel" in k]
    assert len(rs) == 1 and len(lm) == 1, (rs, lm)
    assert rs[0][0] == 0 and lm[0][0] == 0
    assert lm[0][1] == (2 * (1024 + 32) + 2 * 512) * 4


def test_host_length_formulas_match_the_host_front_end():
    """The sizes the GPU path computes on the host are q3_audio.cpp's: checked through the host entry points, which share them."""
    import numpy as np
    import q3tts
    for n, src in ((1366, 16000), (1365, 16000), (12345, 44100), (3, 48000), (2048, 24000)):
        a = np.zeros(n, np.float32)
        r = q3tts.resample(a, src, 24000)
        assert r.size == (n if src == 24000 else int(float(n) * (24000.0 / src)))
        assert q3tts.log_mel(r).shape[1] == (0 if r.size == 0 else 1 if r.size < 1024 else (r.size - 1024) // 256 + 1)
