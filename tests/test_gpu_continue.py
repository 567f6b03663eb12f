"""Continue from codes on the GPU (q3tts_frame_rows_host, q3tts_slot_begin_codes, q3tts_synthesize_continue_host; the row arithmetic is
reference src/tts_onnx.cpp:824-842): the rows bit for bit against a numpy fold, the forced begin against the host-built emulation and
against the CPU oracle walked through the same rows, self-continuation of a checker run (which pins the RNG frame index, the text-row
index and the penalty bitmap at once), the vocoder join, limits.  NOISE = 2e-4 on logits as everywhere else; no new tolerance.
tests/test_continue_surface.py confirms on the CPU that the prefixes used here hold distinct code0 ids."""
import os
import subprocess

import numpy as np
import pytest

import q3_oracle as qo
from continue_ref import (GREEDY, JOINS, N_FRAMES, NOISE, PENALTY, PROMPT_SEED, PROMPT_SEEDS, SAMPLED, SEED, STREAM, WEIGHT_SEED, checker, fold_rows,
                          oracle_after_forced, prompt_ids, verdict)
from util import calibrate_codec, frame_tokens, tiny_pair, to_ocfg, to_osampling, to_q3cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")


def _codes(cfg, seed, n):
    """n valid recorded frames: code0 below the suppressed range, sub-codes anywhere in their vocabulary"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, cfg.sub_vocab, (n, cfg.n_groups)).astype(np.int64)
    c[:, 0] = rng.integers(0, min(cfg.vocab, cfg.suppress_begin), n)
    return c


def _rows(seed, n, H):
    return (np.random.default_rng(seed).standard_normal((n, H)) * 0.1).astype(np.float32)


@pytest.fixture(scope="module")
def tiny():
    eng, orc, w = tiny_pair(seed=WEIGHT_SEED, max_batch=4, max_ctx=128)
    yield eng, orc, w
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def medium():
    eng, orc, w = tiny_pair(seed=5, max_batch=2, max_ctx=256, ocfg=qo.config_medium())
    yield eng, orc, w
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def big06():
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=256)
    eng.fill_synthetic(seed=0)
    yield eng
    eng.close()


def _pad_row(eng):
    """the tts_pad row: text_project(TTS_PAD), which is where the engine takes it from (zeros for a text vocabulary without the id)"""
    return eng.text_project([151671])[0] if 151671 < eng.cfg.text_vocab else np.zeros(eng.cfg.hidden, np.float32)


# ---- 1. rows are exact ----
def _check_rows(eng, codes, frame0, trailing):
    got = eng.frame_rows(codes, frame0, trailing)
    want = fold_rows(eng.codec_embed, eng.cp_embed, codes, frame0, [] if trailing is None else trailing, _pad_row(eng))
    assert got.shape == want.shape == (len(codes), eng.cfg.hidden)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    return got


def test_rows_exact_tiny(tiny):
    eng, _, _ = tiny
    H = eng.cfg.hidden
    codes, tr = _codes(eng.cfg, 1, 5), _rows(2, 3, H)
    a = _check_rows(eng, codes, 0, tr)                       # frames 0..2 take text rows, 3..4 the pad row
    b = _check_rows(eng, codes, 2, tr)                       # the index is absolute: only frame 2 has a text row
    assert np.array_equal(a[3:], b[3:]) and not np.array_equal(a[1], b[1])   # frames 3..4 carry the pad row either way, frame 1 does not
    _check_rows(eng, codes[:1], 7, None)                     # no trailing rows at all


def test_rows_exact_medium(medium):
    eng, _, _ = medium
    _check_rows(eng, _codes(eng.cfg, 3, 4), 1, _rows(4, 3, eng.cfg.hidden))


def test_rows_exact_06b_dims(big06):
    _check_rows(big06, _codes(big06.cfg, 5, 1), 0, _rows(6, 1, big06.cfg.hidden))


def test_rows_exact_17b_dims():
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("1.7b"), device=0, max_batch=1, max_ctx=128)
    try:
        eng.fill_synthetic(seed=1)
        assert eng.cfg.hidden == 2048
        _check_rows(eng, _codes(eng.cfg, 7, 1), 0, _rows(8, 1, eng.cfg.hidden))
    finally:
        eng.close()


# ---- 2. forced begin == the host-built emulation, where the emulation is right (the KV rows, hence logits and last_hidden) ----
def _forced_vs_emulation(eng, F0, sp):
    p, t = eng.build_prompt(prompt_ids(PROMPT_SEED), 0)
    codes = _codes(eng.cfg, 10 + F0, F0)
    eng.slot_begin(0, p, t, sp, seed=SEED, stream_id=STREAM, ignore_eos=True, prefix_codes=codes)
    assert eng.slot_status(0) == (F0, False)
    assert np.array_equal(eng.slot_codes(0), codes)
    a = eng.slot_logits(0)
    eng.slot_release(0)
    rows = eng.frame_rows(codes, 0, t)
    eng.slot_begin(0, np.concatenate([p, rows]), t[F0:], sp, seed=SEED, stream_id=STREAM, ignore_eos=True)
    b = eng.slot_logits(0)
    eng.slot_release(0)
    assert np.isfinite(a[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return p.shape[0]


def test_forced_begin_equals_emulation_short_path(tiny):
    import q3tts
    S = _forced_vs_emulation(tiny[0], 5, q3tts.Sampling(max_new_tokens=8, **GREEDY))
    assert S + 5 <= 16


def test_forced_begin_equals_emulation_mfma_chunk(medium):
    import q3tts
    eng = medium[0]
    S = eng.build_prompt(prompt_ids(PROMPT_SEED), 0)[0].shape[0]
    assert _forced_vs_emulation(eng, 40 - S, q3tts.Sampling(max_new_tokens=8, **GREEDY)) == S


# ---- 3. against the oracle: prefill(prompt), then one decode per forced row ----
def _oracle_case(orc, ocfg, F0):
    ids = prompt_ids(PROMPT_SEED)
    prompt = orc.build_prompt(ids, 0)
    rows_t, pad = orc.trailing()
    codes = _codes(ocfg, 20 + F0, F0)
    rows = fold_rows(orc.codec_embed, orc.cp_embed, codes, 0, rows_t, pad)
    return ids, codes, oracle_after_forced(orc, prompt, rows)


def _forced_logits(eng, ids, codes):
    import q3tts
    p, t = eng.build_prompt(ids, 0)
    eng.slot_begin(0, p, t, q3tts.Sampling(max_new_tokens=8, **GREEDY), seed=SEED, stream_id=STREAM, ignore_eos=True, prefix_codes=codes)
    out = eng.slot_logits(0)
    eng.slot_release(0)
    return out


def test_forced_begin_vs_oracle_gemv_family(tiny):
    eng, orc, _ = tiny
    ids, codes, (lo, ho) = _oracle_case(orc, qo.config_tiny(), 30)
    lg, lh = _forced_logits(eng, ids, codes)
    d = float(np.abs(lg - lo).max()), float(np.abs(lh - ho).max())
    print("tiny, F0 = 30: max |logit - oracle| %.3g, last_hidden %.3g" % d)
    assert d[0] < NOISE and d[1] < NOISE, d


@pytest.fixture(scope="module")
def medium_ref(medium):
    _, orc, _ = medium
    return _oracle_case(orc, qo.config_medium(), 70)       # S + 70 rows: past a 64-token KV page


def test_forced_begin_vs_oracle_mfma(medium, medium_ref):
    eng = medium[0]
    ids, codes, (lo, ho) = medium_ref
    lg, lh = _forced_logits(eng, ids, codes)
    d = float(np.abs(lg - lo).max()), float(np.abs(lh - ho).max())
    print("medium, F0 = 70: max |logit - oracle| %.3g, last_hidden %.3g" % d)
    assert d[0] < NOISE and d[1] < NOISE, d


def test_forced_begin_vs_oracle_chunk16(medium, medium_ref):
    """Q3TTS_PREFILL_CHUNK=16 on a hooks engine (read at creation): the forced rows straddle chunk boundaries"""
    import q3tts
    _, _, w = medium
    ids, codes, (lo, ho) = medium_ref
    os.environ["Q3TTS_PREFILL_CHUNK"] = "16"
    try:
        eng = q3tts.Engine(to_q3cfg(qo.config_medium()), device=0, max_batch=1, max_ctx=256, flags=q3tts.FLAG_TEST_HOOKS)
    finally:
        del os.environ["Q3TTS_PREFILL_CHUNK"]
    try:
        eng.load(w)
        lg, lh = _forced_logits(eng, ids, codes)
        d = float(np.abs(lg - lo).max()), float(np.abs(lh - ho).max())
        print("medium, F0 = 70, 16-row chunks: max |logit - oracle| %.3g, last_hidden %.3g" % d)
        assert d[0] < NOISE and d[1] < NOISE, d
    finally:
        eng.close()


def test_forced_begin_vs_oracle_kv_bf16(medium):
    """Q3TTS_FLAG_KV_BF16 against the oracle's kv_bf16, at that mode's existing bound of 4e-3 (include/q3tts.h)"""
    import q3tts
    _, _, w = medium
    ocfg = qo.config_medium()
    orc = qo.Oracle(ocfg, max_ctx=256, weights=w, kv_bf16=True)
    eng = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=1, max_ctx=256, flags=q3tts.FLAG_KV_BF16)
    try:
        eng.load(w)
        ids, codes, (lo, ho) = _oracle_case(orc, ocfg, 70)
        lg, lh = _forced_logits(eng, ids, codes)
        d = float(np.abs(lg - lo).max()), float(np.abs(lh - ho).max())
        print("medium, F0 = 70, bf16 KV: max |logit - oracle| %.3g, last_hidden %.3g" % d)
        assert d[0] < 4e-3 and d[1] < 4e-3, d
    finally:
        eng.close()
        orc.close()


# ---- 4. self-continuation ----
@pytest.fixture(scope="module")
def refs(tiny):
    """the checker's N_FRAMES frames of the shared prompt: greedy + penalty and sampled + penalty, with decision margins"""
    import q3tts
    _, orc, _ = tiny
    out = {}
    for name, kw in (("greedy", GREEDY), ("sampled", SAMPLED)):
        sp = q3tts.Sampling(repetition_penalty=PENALTY, max_new_tokens=N_FRAMES, **kw)
        out[name] = checker(orc, prompt_ids(PROMPT_SEED), to_osampling(sp))
        assert out[name][0].shape == (N_FRAMES, qo.config_tiny().n_groups)
    return out


def _continue(eng, ref, F0, kw, slot=0, neighbours=()):
    """forced begin with ref[:F0] in `slot` (ordinary slots beside it: (slot, prompt seed) pairs), run to N_FRAMES frames"""
    import q3tts
    sp = q3tts.Sampling(repetition_penalty=PENALTY, max_new_tokens=N_FRAMES - F0, **kw)
    p, t = eng.build_prompt(prompt_ids(PROMPT_SEED), 0)
    eng.slot_begin(slot, p, t, sp, seed=SEED, stream_id=STREAM, ignore_eos=True, prefix_codes=ref[:F0])
    for b, ps in neighbours:
        pn, tn = eng.build_prompt(prompt_ids(ps), 0)
        eng.slot_begin(b, pn, tn, sp, seed=SEED, stream_id=STREAM + b, ignore_eos=True)
    left = N_FRAMES - F0
    while left > 0 and eng.decode_steps(min(16, left)) > 0:
        left -= 16
    assert eng.slot_status(slot) == (N_FRAMES, True)
    out = eng.slot_codes(slot), [eng.slot_codes(b) for b, _ in neighbours]
    for b in [slot] + [b for b, _ in neighbours]:
        eng.slot_release(b)
    return out


def _judge(codes, ref, mg, F0, label, sampled):
    assert np.array_equal(codes[:F0], ref[:F0]), label                            # the prefix itself, exactly
    n = verdict(codes[F0:], ref[F0:], mg[F0:], label)                             # the tail: exact, or stops at a sub-noise margin
    if sampled:
        assert n >= min(5, N_FRAMES - F0), (label, n)                             # the floor of the existing sampled tests
    return n


@pytest.mark.parametrize("no_graph", [False, True])
def test_self_continuation(tiny, refs, no_graph):
    """b = 1 and a forced slot beside two ordinary slots, hipGraph replay and Q3TTS_FLAG_NO_GRAPH.  An empty bitmap or n_frames = 0
    behind the join would re-emit a penalised id / redraw frame 0's uniforms / read text row 0 again: the asserts at the end show
    that both the penalty and the frame index matter for these prompts."""
    import q3tts
    eng, orc, w = tiny
    if no_graph:
        eng = q3tts.Engine(to_q3cfg(qo.config_tiny()), device=0, max_batch=4, max_ctx=128, flags=q3tts.FLAG_NO_GRAPH)
        eng.load(w)
    try:
        tag = " eager" if no_graph else ""
        for name, kw in (("greedy", GREEDY), ("sampled", SAMPLED)):
            ref, mg = refs[name]
            for F0 in JOINS:
                codes, _ = _continue(eng, ref, F0, kw)
                _judge(codes, ref, mg, F0, "%s b=1 F0=%d%s" % (name, F0, tag), name == "sampled")
        # a forced slot (slot 1) between two ordinary ones: their codes equal the same batch without the forced begin's prefix state
        ref, mg = refs["greedy"]
        codes, others = _continue(eng, ref, 7, GREEDY, slot=1, neighbours=((0, PROMPT_SEEDS[1]), (2, PROMPT_SEEDS[2])))
        _judge(codes, ref, mg, 7, "greedy batch F0=7%s" % tag, False)
        sp = q3tts.Sampling(repetition_penalty=PENALTY, max_new_tokens=N_FRAMES - 7, **GREEDY)
        for k, (b, ps) in enumerate(((0, PROMPT_SEEDS[1]), (2, PROMPT_SEEDS[2]))):
            want, mgn = checker(orc, prompt_ids(ps), to_osampling(sp), stream=STREAM + b)
            verdict(others[k], want, mgn, "ordinary slot %d beside the forced one%s" % (b, tag))
        # the penalty acts behind the join: the unpenalised oracle run differs from the checker inside the frames judged above
        plain = orc.generate(orc.build_prompt(prompt_ids(PROMPT_SEED), 0), qo.Sampling(1.0, 1.0, 1, 1.0, N_FRAMES), seed=SEED, stream=STREAM, cp_cached=True, ignore_eos=True)
        assert (plain[:, 0] != refs["greedy"][0][:, 0]).any()
    finally:
        if no_graph:
            eng.close()


def test_self_continuation_06b_dims(big06):
    """0.6B dims (the shipped sampler / MFMA prefill instantiations): F0 = 8 of 24 greedy frames with a penalty that acts"""
    import q3tts
    eng = big06
    orc = qo.Oracle(to_ocfg(eng.cfg), max_ctx=64)
    try:
        for name, shape in eng.tensor_infos():
            if not name.startswith(("cd.", "spk.")):
                orc.set_tensor(name, eng.get_tensor(name, shape))
        ids = frame_tokens(np.random.default_rng(4).integers(0, 151643, 16))
        F, F0 = 24, 8
        sp = q3tts.Sampling(repetition_penalty=2.0, max_new_tokens=F, **GREEDY)
        ref, mg = checker(orc, ids, to_osampling(sp))
        assert len(set(ref[:F0, 0].tolist())) >= 2
        p, t = eng.build_prompt(ids, 0)
        eng.slot_begin(0, p, t, q3tts.Sampling(repetition_penalty=2.0, max_new_tokens=F - F0, **GREEDY), seed=SEED, stream_id=STREAM, ignore_eos=True,
                       prefix_codes=ref[:F0])
        eng.decode_steps(F - F0)
        codes = eng.slot_codes(0)
        eng.slot_release(0)
        _judge(codes, ref, mg, F0, "0.6B dims F0=8", False)
    finally:
        orc.close()


# ---- 5. vocoder join, and the scheduler entry ----
def test_vocoder_join_and_synthesize_continue(tiny, refs):
    import q3tts
    eng, _, _ = tiny
    ref, _ = refs["sampled"]
    F0, NEW = 31, 17
    toks = [prompt_ids(PROMPT_SEED), prompt_ids(PROMPT_SEEDS[1])]
    sp = q3tts.Sampling(repetition_penalty=PENALTY, max_new_tokens=NEW, **SAMPLED)
    # slot level, in the batch shape the job below has: slot 0 forced (RNG stream 0), slot 1 ordinary (stream 1), NEW steps
    for b in range(2):
        p, t = eng.build_prompt(toks[b], 0)
        eng.slot_begin(b, p, t, sp, seed=SEED, stream_id=b, ignore_eos=True, prefix_codes=ref[:F0] if b == 0 else None)
    assert eng.decode_steps(NEW) == 0
    codes0 = eng.slot_codes(0)
    assert codes0.shape[0] == F0 + NEW and np.array_equal(codes0[:F0], ref[:F0])
    tail = eng.slot_codec_decode_range(0, F0, F0 + NEW, left_context=F0)
    whole_slot = eng.slot_codec_decode(0)
    eng.slot_release(0)
    eng.slot_release(1)
    whole = eng.codec_decode(codes0)
    L0 = eng.codec_decode_len(F0)
    assert tail.shape == whole[L0:].shape and tail.size > 0
    d = float(np.abs(tail - whole[L0:]).max())
    print("vocoder join: new frames' samples with the prefix as history vs the tail of the whole decode: max |diff| %.3g" % d)
    assert d <= 2e-5 and float(np.abs(whole_slot - whole).max()) <= 2e-5
    # the job: utterance 0 continues the same prefix, utterance 1 has none
    pcm, codes, nfr = eng.synthesize_continue(toks, [ref[:F0], None], sp, seed=SEED, ignore_eos=True)
    assert list(nfr) == [F0 + NEW, NEW]
    assert np.array_equal(codes[0], codes0)
    assert pcm[0].shape == tail.shape and float(np.abs(pcm[0] - whole[L0:]).max()) <= 2e-5
    # utterance 1 equals q3tts_synthesize_schedule_host's utterance 1, bit for bit (utterance 0 there: the same number of frames, no prefix)
    pcm_s, codes_s, nfr_s = eng.synthesize_batch(toks, q3tts.Sampling(repetition_penalty=PENALTY, max_new_tokens=F0 + NEW, **SAMPLED), seed=SEED, ignore_eos=True,
                                                 max_new_per_utt=[F0 + NEW, NEW])
    assert list(nfr_s) == [F0 + NEW, NEW]
    assert np.array_equal(codes[1], codes_s[1]) and np.array_equal(pcm[1], pcm_s[1])
    # no prefix anywhere: the schedule entry itself
    pcm_n, codes_n, nfr_n = eng.synthesize_continue(toks, [None, None], sp, seed=SEED, ignore_eos=True)
    pcm_b, codes_b, nfr_b = eng.synthesize_batch(toks, sp, seed=SEED, ignore_eos=True)
    for u in range(2):
        assert np.array_equal(codes_n[u], codes_b[u]) and np.array_equal(pcm_n[u], pcm_b[u])


# ---- 6. limits ----
def test_validation_arms_nothing_and_keeps_the_pool():
    import ctypes as C
    import q3tts
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 3), ocfg)
    eng = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=2, max_ctx=256, kv_pool_tokens=2 * 64)
    try:
        eng.load(w)
        cfg = eng.cfg
        p, t = eng.build_prompt(prompt_ids(PROMPT_SEED), 0)
        S = p.shape[0]
        sp = q3tts.Sampling(max_new_tokens=8, **GREEDY)
        before = eng.kv_pool_info()
        good = _codes(cfg, 1, 6)

        def refused(codes, match, sampling=sp):
            with pytest.raises(RuntimeError, match=match):
                eng.slot_begin(0, p, t, sampling, seed=1, stream_id=0, ignore_eos=True, prefix_codes=codes)
            assert eng.decode_steps(1) == 0 and eng.kv_pool_info() == before

        for f, g, v in ((3, 0, cfg.vocab), (3, 0, -1), (2, 0, cfg.suppress_begin), (5, 0, cfg.codec_eos), (4, 9, cfg.sub_vocab), (0, 15, -2)):
            bad = good.copy()
            bad[f, g] = v
            refused(bad, "frame %d group %d holds %d" % (f, g, v))
        refused(_codes(cfg, 2, 256 - S - 8 + 1), "exceeds max_ctx")                         # S + F0 + max_new = max_ctx + 1
        refused(_codes(cfg, 2, 100), "KV page pool exhausted", q3tts.Sampling(max_new_tokens=30, **GREEDY))   # 138 tokens: 3 pages > 2
        c = np.ascontiguousarray(good)
        rc = eng.L.q3tts_slot_begin_codes(eng.h, 0, p.ctypes.data_as(C.c_void_p), S, t.ctypes.data_as(C.c_void_p), t.shape[0],
                                          c.ctypes.data_as(C.c_void_p), -1, C.byref(sp), 1, 0, 1)
        assert rc == -1 and b"n_prefix must be >= 0" in eng.L.q3tts_last_error(eng.h)
        assert eng.decode_steps(1) == 0 and eng.kv_pool_info() == before
        with pytest.raises(ValueError):
            eng.slot_begin(0, p, t, sp, prefix_codes=good[:, :5])                               # not [frames][n_groups]
        with pytest.raises(RuntimeError, match="frame 1 group 0"):
            eng.synthesize_continue([prompt_ids(1)], [np.array([good[0], [cfg.codec_eos] + [0] * 15])], sp, ignore_eos=True)
        assert eng.kv_pool_info() == before
        # n_prefix = 0 is q3tts_slot_begin, bit for bit
        outs = []
        for prefix in (None, np.zeros((0, cfg.n_groups), np.int64)):
            eng.slot_begin(0, p, t, sp, seed=SEED, stream_id=STREAM, ignore_eos=True, prefix_codes=prefix)
            lg = eng.slot_logits(0)
            eng.decode_steps(8)
            outs.append((lg, eng.slot_codes(0)))
            eng.slot_release(0)
            assert eng.kv_pool_info() == before
        assert np.array_equal(outs[0][0][0], outs[1][0][0]) and np.array_equal(outs[0][0][1], outs[1][0][1]) and np.array_equal(outs[0][1], outs[1][1])
        # and a prefix that fits is armed: 8 + 100 + 8 tokens = 2 pages
        eng.slot_begin(0, p, t, sp, seed=1, stream_id=0, ignore_eos=True, prefix_codes=_codes(cfg, 2, 100))
        assert eng.slot_status(0) == (100, False) and eng.kv_pool_info()[2] == before[2] - 2
        assert eng.decode_steps(8) == 0 and eng.slot_status(0) == (108, True)
        eng.slot_release(0)
        assert eng.kv_pool_info() == before
    finally:
        eng.close()


def test_cli_save_and_continue_codes(tmp_path):
    """leaxer-tts --save-codes / --continue-codes: the second run's frames start with the first run's, its WAV holds the new frames only"""
    import q3tts

    def run(extra, out):
        r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22,33,44,55,66", "-o", str(out), "--top-k", "1", "--rep-penalty", "1.5",
                            "--seed", "3"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    run(["--max-tokens", "12", "--save-codes", str(a)], tmp_path / "a.wav")
    ca = q3tts.load_codes(a)
    assert ca.shape[1] == 16 and 1 <= ca.shape[0] <= 12
    out = run(["--max-tokens", "8", "--continue-codes", str(a), "--save-codes", str(b)], tmp_path / "b.wav")
    cb = q3tts.load_codes(b)
    assert ca.shape[0] < cb.shape[0] <= ca.shape[0] + 8 and np.array_equal(cb[: ca.shape[0]], ca)
    assert "Frames: %d recorded + %d new" % (ca.shape[0], cb.shape[0] - ca.shape[0]) in out
    cfg = q3tts.default_config("0.6b")
    L = lambda n: int(q3tts.lib().q3tts_codec_decode_len(cfg, n))   # noqa: E731
    n_samples = (os.path.getsize(tmp_path / "b.wav") - 44) // 2
    assert n_samples == L(cb.shape[0]) - L(ca.shape[0])
