"""The surface of streaming behind a prefix, checkable without a GPU: the four C-ABI entry points in include/q3tts.h, q3tts.EXPORTS and
the built library, the Python wrappers' argument checks, TTSEngine's method and the CLI flags.  What the entry points compute is checked
on the GPU: tests/test_gpu_continue_stream.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_codec_stream_prime_batch_host", "q3tts_slots_codec_prime", "q3tts_codec_stream_info", "q3tts_synthesize_continue_stream_host")
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_codec_stream_prime_batch_host\(q3tts_engine\* e, int n_streams, const int32_t\* stream_ids, const int64_t\* codes, "
                     r"const int32_t\* frame_offsets\);", hdr)
    assert re.search(r"int q3tts_slots_codec_prime\(q3tts_engine\* e, int n_slots, const int32_t\* slots, const int32_t\* n_frames\);", hdr)
    assert re.search(r"int q3tts_codec_stream_info\(q3tts_engine\* e, int stream_id, int\* n_done, int\* kv_capacity_rows, int64_t\* bytes\);", hdr)
    assert re.search(r"int q3tts_synthesize_continue_stream_host\(q3tts_engine\* e, int n_utt, const int64_t\* ids, const int32_t\* offsets, int lang,\s*"
                     r"const float\* const\* speakers, const q3tts_sampling\* p, const int32_t\* max_new_per_utt, uint64_t seed, int ignore_eos,\s*"
                     r"float\* const\* pcm_out, int64_t pcm_cap, int64_t\* pcm_len, int32_t\* n_frames, int64_t\* codes_out,\s*"
                     r"const int64_t\* prefix_codes, const int32_t\* prefix_offsets,\s*int chunk_frames, q3tts_audio_cb cb, void\* user\);", hdr)
    # the continue entry keeps its wording and points to the streaming one; every new entry cites the reference lines it stands for
    assert "Non-streaming only" in hdr and re.search(r"Non-streaming only[^/]*q3tts_synthesize_continue_stream_host", hdr)
    for name in NEW:
        decl = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, decl):decl]
        assert "tts_onnx.cpp:" in comment, name
    # no engine: refused like every other entry point
    assert L.q3tts_codec_stream_prime_batch_host(None, 1, None, None, None) == -1
    assert L.q3tts_slots_codec_prime(None, 1, None, None) == -1
    assert L.q3tts_codec_stream_info(None, 0, None, None, None) == -1
    assert L.q3tts_synthesize_continue_stream_host(None, 1, None, None, 0, None, None, None, ctypes.c_uint64(0), 0, None, ctypes.c_int64(0), None, None, None,
                                                   None, None, 1, None, None) == -1
    # the Python callers
    for name in ("codec_stream_prime_batch", "slots_codec_prime", "codec_stream_info", "synthesize_icl_batch"):
        assert callable(getattr(q3tts.Engine, name)), name
    sig = inspect.signature(q3tts.Engine.synthesize_continue).parameters
    assert list(sig)[-2:] == ["chunk_frames", "on_audio"] and sig["chunk_frames"].default == 0 and sig["on_audio"].default is None
    assert list(inspect.signature(q3tts.Engine.synthesize_icl_batch).parameters) == [
        "self", "ref_pcms", "ref_ids_list", "token_lists", "sp", "lang", "seed", "ignore_eos", "speakers", "ref_rates", "max_new_per_utt", "chunk_frames", "on_audio"]
    assert list(inspect.signature(q3tts.Engine.synthesize_icl).parameters)[:5] == ["self", "ref_pcm", "ref_ids", "ids", "sp"]      # stays as it is
    # TTSEngine: next to synthesize_tokens_continue
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"int synthesize_tokens_continue_streaming\(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes,", h)
    assert h.index("synthesize_tokens_continue(") < h.index("synthesize_tokens_continue_streaming(") < h.index("encode_audio(")


class _Shell:
    """an Engine that never reaches the library: the wrappers' own argument checks run before any call"""

    def __init__(self):
        import q3tts
        self.cfg = q3tts.default_config("0.6b")

    def __getattr__(self, name):
        raise AssertionError("the wrapper went on to the library (%s)" % name)


def test_python_wrappers_check_their_arguments():
    import q3tts
    sh = _Shell()
    G = sh.cfg.n_groups
    E = q3tts.Engine
    sh._frames = lambda c, what: E._frames(sh, c, what)
    with pytest.raises(ValueError, match="one code array per stream"):
        E.codec_stream_prime_batch(sh, [0, 1], [np.zeros((2, G))])
    assert E.codec_stream_prime_batch(sh, [], []) is None                                   # nothing to do: no call
    with pytest.raises(ValueError, match="one frame count per slot"):
        E.slots_codec_prime(sh, [0, 1], [3])
    assert E.slots_codec_prime(sh, [], []) is None
    sp = q3tts.Sampling()
    with pytest.raises(ValueError, match="one entry"):
        E.synthesize_continue(sh, [[1, 2]], [None, None], sp, chunk_frames=4, on_audio=lambda *a: 0)
    with pytest.raises(ValueError, match="on_audio needs chunk_frames >= 1"):
        E.synthesize_continue(sh, [[1, 2]], [None], sp, on_audio=lambda *a: 0)
    with pytest.raises(ValueError, match="chunk_frames without on_audio"):
        E.synthesize_continue(sh, [[1, 2]], [None], sp, chunk_frames=4)
    with pytest.raises(ValueError, match=r"expected \[frames\]"):
        E.synthesize_continue(sh, [[1, 2]], [np.zeros((2, 3))], sp, chunk_frames=4, on_audio=lambda *a: 0)
    with pytest.raises(ValueError, match="one reference clip and one reference id list per utterance"):
        E.synthesize_icl_batch(sh, [np.zeros(10)], [[1], [2]], [[1, 2, 3, 4, 5]], sp)
    with pytest.raises(ValueError, match="on_audio needs chunk_frames >= 1"):
        E.synthesize_icl_batch(sh, [np.zeros(10)], [[1]], [[1, 2, 3, 4, 5]], sp, on_audio=lambda *a: 0)
    with pytest.raises(ValueError, match="chunk_frames without on_audio"):
        E.synthesize_icl_batch(sh, [np.zeros(10)], [[1]], [[1, 2, 3, 4, 5]], sp, chunk_frames=2)


def test_cli_flags_combine(tmp_path):
    import q3tts
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert re.search(r"^\s+--stream-chunk N .*\n\s+combines with --continue-codes and with --ref \+ --ref-text / --ref-tokens", r.stdout, re.M), r.stdout
    good = tmp_path / "codes.txt"
    q3tts.save_codes(good, np.random.default_rng(0).integers(0, 2048, (5, 16)).astype(np.int64))
    # the CLI reads the codes file and then looks for the model (no GPU is touched here: the model directory does not exist)
    base = [CLI, "-m", str(tmp_path / "no-such-model"), "--tokens", "1,2,3"]
    r = subprocess.run(base + ["--continue-codes", str(good), "--stream-chunk", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "(5 frames of 16 codes)" in r.stdout and "model directory not found" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--ref", str(tmp_path / "ref.wav"), "--ref-tokens", "7,8", "--stream-chunk", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "model directory not found" in r.stderr, r.stdout + r.stderr
    # live text behind a prefix stays refused
    r = subprocess.run(base + ["--continue-codes", str(good), "--stream-chunk", "5", "--feed", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--feed K (K >= 1) needs --stream-chunk (without --ref, --instruct, --continue-codes)" in r.stderr
    r = subprocess.run(base + ["--ref", str(tmp_path / "ref.wav"), "--ref-tokens", "7,8", "--stream-chunk", "5", "--feed", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--feed K (K >= 1) needs --stream-chunk" in r.stderr
