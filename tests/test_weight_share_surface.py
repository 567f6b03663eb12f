"""The surface of weight sharing between engines on a GPU ("weights immutable & shareable across handles"), checkable
without a GPU: the C-ABI entries in include/q3tts.h, the built library, q3tts.EXPORTS, the Python callers and TTSEngine's method.
(What a sharing engine computes is checked on the GPU: tests/test_gpu_weight_share.py.)"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_create_sharing", "q3tts_weights_info")


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    assert re.search(r"q3tts_engine\* q3tts_create_sharing\(q3tts_engine\* donor, int max_batch, int max_ctx, int64_t kv_pool_tokens, uint32_t flags\);", hdr)
    assert re.search(r"int q3tts_weights_info\(q3tts_engine\* e, int64_t\* shared_bytes, int\* holders, int64_t\* private_weight_bytes\);", hdr)
    assert "weights are shared by N engines" in hdr     # the refusal's wording is part of the contract


def test_library_exports_and_refuses_a_null_engine():
    import q3tts
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
    L.q3tts_create_sharing.restype = ctypes.c_void_p
    L.q3tts_create_sharing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32]
    L.q3tts_last_error.restype = ctypes.c_char_p
    L.q3tts_last_error.argtypes = [ctypes.c_void_p]
    assert L.q3tts_create_sharing(None, 1, 128, 0, 0) is None
    msg = L.q3tts_last_error(None).decode()
    assert "donor" in msg, msg
    b, n, p = ctypes.c_int64(7), ctypes.c_int(7), ctypes.c_int64(7)
    assert L.q3tts_weights_info(None, ctypes.byref(b), ctypes.byref(n), ctypes.byref(p)) == -1
    assert (b.value, n.value, p.value) == (7, 7, 7)


def test_python_surface():
    import q3tts
    for name in NEW:
        assert name in q3tts.EXPORTS, name
    assert callable(q3tts.Engine.share) and callable(q3tts.Engine.weights_info)
    sh = inspect.signature(q3tts.Engine.share).parameters
    assert sh["max_batch"].default == 1 and sh["max_ctx"].default is None and sh["flags"].default is None and sh["kv_pool_tokens"].default == 0


def test_tts_engine_method():
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"static std::unique_ptr<TTSEngine> share_weights\(const TTSEngine& donor\);", h)
    assert re.search(r"TTSEngine\(const TTSEngine&\) = delete;", h)     # the copy constructor stays deleted
