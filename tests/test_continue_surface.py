"""The surface of "continue from codes", checkable without a GPU: the three C-ABI entry points in include/q3tts.h, q3tts.EXPORTS and the
built library, the Python wrappers' argument checks, TTSEngine's method, the CLI flags and the codes file format — and, with the oracle
alone, that the prefixes tests/test_gpu_continue.py continues from hold distinct code0 ids (otherwise its penalty-bitmap check would be
vacuous).  What the entry points compute is checked on the GPU: tests/test_gpu_continue.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_frame_rows_host", "q3tts_slot_begin_codes", "q3tts_synthesize_continue_host")
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def test_entry_points_declared_listed_exported_and_reachable():
    import q3tts
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_frame_rows_host\(q3tts_engine\* e, const int64_t\* codes, int n, int frame0, const float\* trailing, int n_trailing, float\* out\);", hdr)
    assert re.search(r"int q3tts_slot_begin_codes\(q3tts_engine\* e, int slot, const float\* prompt, int S, const float\* trailing, int n_trailing,\s*"
                     r"const int64_t\* prefix_codes, int n_prefix,\s*const q3tts_sampling\* p, uint64_t seed, uint32_t stream_id, int ignore_eos\);", hdr)
    assert re.search(r"int q3tts_synthesize_continue_host\(q3tts_engine\* e, int n_utt, const int64_t\* ids, const int32_t\* offsets, int lang,\s*"
                     r"const float\* const\* speakers, const q3tts_sampling\* p, const int32_t\* max_new_per_utt, uint64_t seed, int ignore_eos,\s*"
                     r"float\* const\* pcm_out, int64_t pcm_cap, int64_t\* pcm_len, int32_t\* n_frames, int64_t\* codes_out,\s*"
                     r"const int64_t\* prefix_codes, const int32_t\* prefix_offsets\);", hdr)
    assert hdr.count("tts_onnx.cpp:824-842") >= 3                     # each entry cites the row arithmetic it restates
    assert "Non-streaming only" in hdr and "left_context >= n_prefix" in hdr
    # no engine: refused like every other entry point
    assert L.q3tts_frame_rows_host(None, None, 1, 0, None, 0, None) == -1
    assert L.q3tts_slot_begin_codes(None, 0, None, 1, None, 0, None, 0, None, ctypes.c_uint64(0), 0, 0) == -1
    assert L.q3tts_synthesize_continue_host(None, 1, None, None, 0, None, None, None, ctypes.c_uint64(0), 0, None, ctypes.c_int64(0), None, None, None,
                                            None, None) == -1
    # the Python callers
    assert list(inspect.signature(q3tts.Engine.frame_rows).parameters)[:4] == ["self", "codes", "frame0", "trailing"]
    assert inspect.signature(q3tts.Engine.slot_begin).parameters["prefix_codes"].default is None
    assert list(inspect.signature(q3tts.Engine.synthesize_continue).parameters)[:4] == ["self", "token_lists", "prefix_codes", "sp"]
    # TTSEngine: beside the instruct methods
    h = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"synthesize_tokens_continue\(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes,", h)
    assert h.index("synthesize_tokens_instruct(") < h.index("synthesize_tokens_continue(")


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
    G, H = sh.cfg.n_groups, sh.cfg.hidden
    frames = q3tts.Engine._frames
    assert frames(sh, np.zeros((3, G), np.int32), "x").dtype == np.int64
    assert frames(sh, [], "x").shape == (0, G)
    for bad in (np.zeros((3, G - 1)), np.zeros(G), np.zeros((2, 2, G))):
        with pytest.raises(ValueError, match=r"expected \[frames\]\[%d\]" % G):
            frames(sh, bad, "x")
    sh._frames = lambda c, what: frames(sh, c, what)
    with pytest.raises(ValueError, match="frame0"):
        q3tts.Engine.frame_rows(sh, np.zeros((1, G)), frame0=-1)
    with pytest.raises(ValueError, match="trailing must be"):
        q3tts.Engine.frame_rows(sh, np.zeros((1, G)), 0, np.zeros((2, H + 1), np.float32))
    assert q3tts.Engine.frame_rows(sh, np.zeros((0, G)), 0).shape == (0, H)          # no frame: no call
    with pytest.raises(ValueError, match=r"expected \[frames\]"):
        q3tts.Engine.slot_begin(sh, 0, np.zeros((8, H)), np.zeros((1, H)), q3tts.Sampling(), prefix_codes=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="one entry"):
        q3tts.Engine.synthesize_continue(sh, [[1, 2]], [None, None], q3tts.Sampling())
    with pytest.raises(ValueError, match=r"expected \[frames\]"):
        q3tts.Engine.synthesize_continue(sh, [[1, 2]], [np.zeros((2, 3))], q3tts.Sampling())


def test_codes_file_format_and_cli_flags(tmp_path):
    import q3tts
    codes = np.random.default_rng(0).integers(0, 2048, (5, 16)).astype(np.int64)
    good = tmp_path / "codes.txt"
    q3tts.save_codes(good, codes)
    lines = open(good).read().splitlines()
    assert len(lines) == 5 and all(len(ln.split()) == 16 for ln in lines)             # one frame per line, n_groups integers
    back = q3tts.load_codes(good)
    assert back.dtype == np.int64 and np.array_equal(back, codes)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert re.search(r"^\s+--save-codes FILE", r.stdout, re.M) and re.search(r"^\s+--continue-codes FILE", r.stdout, re.M), r.stdout
    # the CLI reads the file before it looks for the model (no GPU is touched here: the model directory does not exist)
    base = [CLI, "-m", str(tmp_path / "no-such-model"), "--tokens", "1,2,3"]
    r = subprocess.run(base + ["--continue-codes", str(good)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "(5 frames of 16 codes)" in r.stdout and "model directory not found" in r.stderr
    ragged = tmp_path / "ragged.txt"
    ragged.write_text("1 2 3\n4 5\n")
    r = subprocess.run(base + ["--continue-codes", str(ragged)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "line 2: 2 codes, the lines before have 3" in r.stderr
    with pytest.raises(ValueError):
        q3tts.load_codes(ragged)
    words = tmp_path / "words.txt"
    words.write_text("1 2 x\n")
    r = subprocess.run(base + ["--continue-codes", str(words)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "line 1: not an integer" in r.stderr
    r = subprocess.run(base + ["--continue-codes", str(tmp_path / "absent.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot read codes file" in r.stderr
    r = subprocess.run([CLI, "-m", "x", "-p", "text", "--save-codes", str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "go with --tokens" in r.stderr


def test_prefixes_of_the_gpu_tests_hold_distinct_code0_ids():
    """the checker run tests/test_gpu_continue.py continues from (oracle alone): with the penalty the code0 ids of the first 7 and 31
    frames are not all one id, so a forced begin that left the bitmap empty would be penalising nothing where the checker penalises
    (F0 = 1 holds one id by construction).  Also: the penalty acts inside the frames behind each join."""
    import q3_oracle as qo
    from continue_ref import GREEDY, JOINS, N_FRAMES, PENALTY, PROMPT_SEED, SAMPLED, SEED, STREAM, WEIGHT_SEED, checker, prompt_ids
    ocfg = qo.config_tiny()
    orc = qo.Oracle(ocfg, max_ctx=128, weights=qo.random_weights(ocfg, WEIGHT_SEED))
    try:
        for kw in (GREEDY, SAMPLED):
            so = qo.Sampling(kw["temperature"], kw["top_p"], kw["top_k"], PENALTY, N_FRAMES)
            ref, _ = checker(orc, prompt_ids(PROMPT_SEED), so)
            assert ref.shape == (N_FRAMES, ocfg.n_groups)
            for F0 in JOINS:
                if F0 > 1:
                    assert len(set(ref[:F0, 0].tolist())) >= 2, (kw, F0)
            if kw is GREEDY:
                plain = orc.generate(orc.build_prompt(prompt_ids(PROMPT_SEED), 0), qo.Sampling(1.0, 1.0, 1, 1.0, N_FRAMES), seed=SEED, stream=STREAM,
                                     cp_cached=True, ignore_eos=True)
                diff = np.nonzero(plain[:, 0] != ref[:, 0])[0]
                assert diff.size and all((diff >= F0).any() for F0 in JOINS)
    finally:
        orc.close()
