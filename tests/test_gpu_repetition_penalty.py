"""q3tts_sampling::repetition_penalty on the GPU, through the C-ABI: the sampler with an explicit history against the oracle's sampler
on a penalised row (every trial), the fused generation loop against the checker of tests/penalty_ref.py (the oracle's step functions
in the reference's frame loop, reference src/tts_onnx.cpp:782-872, plus the penalty), per-slot / per-utterance state, preemption,
validation and the CLI flag.  tests/test_cpu_repetition_penalty.py shows on the CPU that the checker equals the oracle with the penalty
off and that the prompts / penalty / frame count used here make the penalty change the codes."""
import math
import os
import subprocess

import numpy as np
import pytest

import q3_oracle as qo
from penalty_ref import FRAMES, PENALTY, PROMPT_SEEDS, SEED, STREAM, WEIGHT_SEED, generate_with_penalty, penalise, prompt_ids, suppress
from util import Hip, calibrate_codec, frame_tokens, tiny_pair, to_ocfg, to_osampling, to_q3cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
NOISE = 2e-4    # bound asserted on |HIP logit - oracle logit| by the teacher-forced tests (tests/test_gpu_full.py)

SAMPLER_PARAMS = [   # the nine parameter sets of test_sampler_vs_oracle
    dict(temperature=0.8, top_p=0.95, top_k=50),
    dict(temperature=1.0, top_p=1.0, top_k=1),
    dict(temperature=0.0, top_p=1.0, top_k=0),
    dict(temperature=1.3, top_p=0.5, top_k=10),
    dict(temperature=0.7, top_p=0.9, top_k=0),
    dict(temperature=0.8, top_p=1.0, top_k=200),
    dict(temperature=0.9, top_p=0.9, top_k=64),
    dict(temperature=0.9, top_p=0.9, top_k=65),
    dict(temperature=1.0, top_p=0.8, top_k=2),
]


@pytest.fixture(scope="module")
def pair():
    eng, orc, w = tiny_pair(seed=WEIGHT_SEED, max_batch=8, max_ctx=128)
    yield eng, orc, w
    eng.close()
    orc.close()


def _trial(rng, t, params):
    """logits row, uniform, history, penalty, suppress flag of trial t: the rows and tie constructions of test_sampler_vs_oracle, history
    lengths 0 / 1 / 7 / 300 / 2048 (with duplicates) that hold the current argmax and the top-k threshold element"""
    n = (96, 3072, 2048, 2176)[t % 4]
    lg = (rng.standard_normal(n) * 2.0).astype(np.float32)
    if t % 5 == 0:
        lg[rng.integers(0, n, 4)] = lg.max()
    if t % 7 == 3:
        lg[rng.integers(0, n, 6)] = np.sort(lg)[-min(params["top_k"] or 5, n - 1)]
    if t % 11 == 5:
        lg[:] = np.round(lg * 4) / 4
    u = float(rng.random()) if t % 13 else (0.0, 0.99999994)[t % 2]
    hl = (0, 1, 7, 300, 2048)[(t // 4) % 5]
    pen = (1.05, 1.3, 2.0, 0.8)[(t // 2) % 4]
    sup = n in (2176, 3072)
    vis = suppress(qo.config_tiny(), lg, False) if sup else lg
    order = np.argsort(-vis, kind="stable")
    k = params["top_k"] or 5
    hist = rng.integers(0, n, hl).astype(np.int64)          # with replacement: duplicates from 300 up are certain
    if hl >= 1:
        hist[0] = order[0]                                   # the argmax
    if hl >= 7:
        hist[1] = order[min(k, n) - 1]                       # the top-k threshold element
        hist[2] = order[min(k, n - 1)]                       # and the first one below it
        hist[3] = hist[0]                                    # a duplicate of the argmax
    return lg, u, hist, pen, sup


@pytest.mark.parametrize("params", SAMPLER_PARAMS)
def test_sampler_with_history_vs_oracle(pair, params):
    """q3tts_sample_hist_host == q3o_sample on the penalised row, on EVERY trial (200 per parameter set): ids are integers, the penalty is
    one IEEE fp32 divide or multiply on both sides, so nothing is tolerated.  Suppression is on for the 2176 / 3072-wide rows: the
    kernel penalises the raw row and suppresses afterwards, the checker does the same (the oracle's sampler itself does not suppress)."""
    import q3tts
    eng, orc, _ = pair
    cfg = qo.config_tiny()
    rng = np.random.default_rng(7)
    bad, moved = [], 0
    for t in range(200):
        lg, u, hist, pen, sup = _trial(rng, t, params)
        sp = q3tts.Sampling(max_new_tokens=8, repetition_penalty=pen, **params)
        a = eng.sample_hist(lg, sp, u, hist, suppress=sup)
        row = penalise(lg, hist, pen)
        plain = lg
        if sup:
            row, plain = suppress(cfg, row, False), suppress(cfg, lg, False)
        b = orc.sample(row, to_osampling(sp), u)
        moved += int(b != orc.sample(plain, to_osampling(sp), u))
        if a != b:
            bad.append((t, lg.size, u, hist.size, pen, a, b))
    print("params %s: the penalty moved the oracle's decision in %d of 200 trials" % (params, moved))
    assert not bad, bad[:5]
    assert moved > 0


def test_penalty_moves_the_greedy_decision(pair):
    """top_k = 1, history = {argmax}, p = 2: the argmax is not returned when the runner-up is within a factor 2 (and is when it is not)"""
    import q3tts
    eng, orc, _ = pair
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=2.0, max_new_tokens=1)
    rng = np.random.default_rng(3)
    for n in (96, 2048, 2176, 3072):
        lg = (rng.standard_normal(n) * 0.1).astype(np.float32)
        lg[17], lg[40] = 3.0, 2.0                            # runner-up within a factor 2
        assert eng.sample(lg, sp, 0.5) == 17
        assert eng.sample_hist(lg, sp, 0.5, [17]) == 40
        assert eng.sample_hist(lg, sp, 0.5, [17, 40]) == 17  # both halved: 1.5 > 1.0
        lg[40] = 1.0                                         # 3 / 2 > 1: the argmax stays
        assert eng.sample_hist(lg, sp, 0.5, [17]) == 17
        lg[:] = -np.abs(lg) - 2.5                            # negative logits are multiplied: -1 * 2 = -2 falls behind -1.5, the rest is below -2.5
        lg[5], lg[9] = -1.0, -1.5
        assert eng.sample(lg, sp, 0.5) == 5 and eng.sample_hist(lg, sp, 0.5, [5]) == 9


def test_sample_hist_dev_equals_the_host_entry_row_by_row(pair):
    import q3tts
    eng, orc, _ = pair
    hip = Hip()
    try:
        rng = np.random.default_rng(9)
        for V, sup in ((eng.cfg.vocab, True), (eng.cfg.sub_vocab, False), (3072, True)):
            for kw in (dict(temperature=1.0, top_p=1.0, top_k=1), dict(temperature=0.8, top_p=0.95, top_k=50), dict(temperature=1.3, top_p=0.7, top_k=0)):
                sp = q3tts.Sampling(max_new_tokens=1, repetition_penalty=1.3, **kw)
                B, ld = 24, 320
                lg = (rng.standard_normal((B, V)) * 2.0).astype(np.float32)
                u = rng.random(B).astype(np.float32)
                hist = rng.integers(0, V, (B, ld)).astype(np.int64)
                hist[:, 0] = np.argmax(lg, axis=1)
                lens = (rng.integers(0, ld + 1, B)).astype(np.int32)
                lens[:4] = (0, 1, ld, 7)
                ids_d = hip.alloc(B * 8)
                eng.sample_hist_dev(hip.put(lg), B, V, sp, hip.put(u), sup, hip.put(hist), ld, hip.put(lens), ids_d)
                hip.rt.hipStreamSynchronize(eng.stream)
                got = hip.get(ids_d, (B,), np.int64)
                want = np.array([eng.sample_hist(lg[b], sp, float(u[b]), hist[b, :lens[b]], suppress=sup) for b in range(B)], np.int64)
                assert np.array_equal(got, want), (V, kw)
    finally:
        hip.free()


@pytest.mark.parametrize("params", SAMPLER_PARAMS[:3] + SAMPLER_PARAMS[4:5])
def test_off_is_off_in_the_sampler(pair, params):
    """p in {0, 1} with any history, and any p with an empty history: the ids of q3tts_sample_host on the same trials"""
    import q3tts
    eng, _, _ = pair
    rng = np.random.default_rng(7)
    for t in range(60):
        lg, u, hist, pen, sup = _trial(rng, t, params)
        want = eng.sample(lg, q3tts.Sampling(max_new_tokens=8, **params), u, sup)
        full = np.concatenate([hist, [int(np.argmax(lg))]])
        for p, h in ((0.0, full), (1.0, full), (pen, [])):
            sp = q3tts.Sampling(max_new_tokens=8, repetition_penalty=p, **params)
            assert eng.sample_hist(lg, sp, u, h, suppress=sup) == want, (t, p)


def _gen_batch(eng, seeds, sp, ignore_eos=True, penalties=None):
    """arm slot i with prompt seeds[i] (stream STREAM + i), run to the cap, return the codes per slot"""
    import q3tts
    for i, ps in enumerate(seeds):
        p, t = eng.build_prompt(prompt_ids(ps), 0)
        spi = sp if penalties is None else q3tts.Sampling(sp.temperature, sp.top_p, sp.top_k, penalties[i], sp.max_new_tokens)
        eng.slot_begin(i, p, t, spi, seed=SEED, stream_id=STREAM + i, ignore_eos=ignore_eos)
    left = sp.max_new_tokens
    while left > 0 and eng.decode_steps(min(16, left)) > 0:
        left -= 16
    out = [eng.slot_codes(i) for i in range(len(seeds))]
    for i in range(len(seeds)):
        eng.slot_release(i)
    return out


@pytest.mark.parametrize("params", [dict(temperature=1.0, top_p=1.0, top_k=1), dict(temperature=0.8, top_p=0.95, top_k=50)])
def test_off_is_off_in_the_fused_loop(pair, params):
    """repetition_penalty 0.0 and 1.0: identical codes, at b = 1 and in a batch, and equal to the oracle (which has no penalty)"""
    import q3tts
    eng, orc, _ = pair
    outs = []
    for p in (0.0, 1.0):
        sp = q3tts.Sampling(max_new_tokens=FRAMES, repetition_penalty=p, **params)
        outs.append((_gen_batch(eng, PROMPT_SEEDS[:1], sp), _gen_batch(eng, PROMPT_SEEDS, sp)))
    assert np.array_equal(outs[0][0][0], outs[1][0][0])
    for i in range(len(PROMPT_SEEDS)):
        assert np.array_equal(outs[0][1][i], outs[1][1][i]), i
    if params["top_k"] == 1:
        sp = q3tts.Sampling(max_new_tokens=FRAMES, repetition_penalty=0.0, **params)
        ref = orc.generate(orc.build_prompt(prompt_ids(PROMPT_SEEDS[0]), 0), to_osampling(sp), seed=SEED, stream=STREAM, cp_cached=True, ignore_eos=True)
        assert np.array_equal(outs[0][0][0], ref)


def _verdict(codes, ref, mg, label, noise=NOISE):
    """the margin-aware acceptance of tests/test_gpu_full.py (check_free_running): bit-exact up to the first differing decision, which
    must have a checker margin (on the PENALISED row for code0) under the logit noise; returns the number of bit-exact frames"""
    assert codes.shape == ref.shape, (label, codes.shape, ref.shape)
    bad = np.argwhere(codes != ref)
    if bad.size == 0:
        print("penalty free-running %s: %d frames bit-exact; smallest decision margin %.3g" % (label, ref.shape[0], float(mg.min())))
        return ref.shape[0]
    f, g = int(bad[0][0]), int(bad[0][1])
    print("penalty free-running %s: first divergence at frame %d group %d, checker margin %.3g (noise bound %.0e)" % (label, f, g, float(mg[f, g]), noise))
    assert float(mg[f, g]) < noise, "%s: ids differ at frame %d group %d although the checker's margin there is %g" % (label, f, g, float(mg[f, g]))
    assert np.array_equal(codes[:f], ref[:f]) and np.array_equal(codes[f, :g], ref[f, :g])
    return f


def _checker(orc, ps, sp, stream, penalty=None):
    so = to_osampling(sp)
    if penalty is not None:
        so.repetition_penalty = penalty
    return generate_with_penalty(orc, orc.build_prompt(prompt_ids(ps), 0), so, seed=SEED, stream=stream, ignore_eos=True, margins=True)


@pytest.mark.parametrize("no_graph", [False, True])
def test_fused_loop_greedy_vs_checker(no_graph):
    """greedy with the penalty: b = 1 (three prompts) and a batch of 8 with a different prompt per slot, hipGraph replay and
    Q3TTS_FLAG_NO_GRAPH, FRAMES frames each, against the checker; every run must also differ from the unpenalised oracle"""
    import q3tts
    eng, orc, _ = tiny_pair(seed=WEIGHT_SEED, max_batch=8, max_ctx=128, flags=q3tts.FLAG_NO_GRAPH if no_graph else 0)
    try:
        sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=PENALTY, max_new_tokens=FRAMES)
        sp_off = qo.Sampling(1.0, 1.0, 1, 1.0, FRAMES)
        for ps in PROMPT_SEEDS[:3]:
            codes = _gen_batch(eng, [ps], sp)[0]
            ref, mg = _checker(orc, ps, sp, STREAM)
            n = _verdict(codes, ref, mg, "b=1 prompt %d%s" % (ps, " eager" if no_graph else ""))
            plain = orc.generate(orc.build_prompt(prompt_ids(ps), 0), sp_off, seed=SEED, stream=STREAM, cp_cached=True, ignore_eos=True)
            first = np.nonzero(plain[:, 0] != ref[:, 0])[0]
            assert first.size and first[0] < n, "the exact prefix does not reach the first frame the penalty changes"
        batch = _gen_batch(eng, PROMPT_SEEDS, sp)
        for i, ps in enumerate(PROMPT_SEEDS):
            ref, mg = _checker(orc, ps, sp, STREAM + i)
            n = _verdict(batch[i], ref, mg, "b=8 slot %d%s" % (i, " eager" if no_graph else ""))
            plain = orc.generate(orc.build_prompt(prompt_ids(ps), 0), sp_off, seed=SEED, stream=STREAM + i, cp_cached=True, ignore_eos=True)
            first = np.nonzero(plain[:, 0] != ref[:, 0])[0]
            assert first.size and first[0] < n, i
    finally:
        eng.close()
        orc.close()


def test_fused_loop_sampled_vs_checker(pair):
    """0.8 / 50 / 0.95 with the penalty: equal to the checker up to the first decision under the logit noise (README: what sampled
    parity means).  Floor on the exact prefix: 5 frames, the lowest floor of the existing free-running tests."""
    import q3tts
    eng, orc, _ = pair
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, repetition_penalty=PENALTY, max_new_tokens=FRAMES)
    for ps in PROMPT_SEEDS[:3]:
        codes = _gen_batch(eng, [ps], sp)[0]
        ref, mg = _checker(orc, ps, sp, STREAM)
        assert _verdict(codes, ref, mg, "sampled prompt %d" % ps) >= 5


def test_fused_loop_greedy_vs_checker_full_size():
    """0.6B dims (code0 row 3072 wide: the PW = 12 instantiation of k_sample that ships), synthetic weights, greedy, 24 frames with a
    penalty: the bitmap path against the checker.  The penalty is chosen on the unpenalised oracle run so that it acts (see the assert)."""
    import q3tts
    cfg = q3tts.default_config("0.6b")
    eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=256)
    eng.fill_synthetic(seed=0)
    orc = qo.Oracle(to_ocfg(cfg), max_ctx=64)
    try:
        for name, shape in eng.tensor_infos():
            if not name.startswith(("cd.", "spk.")):
                orc.set_tensor(name, eng.get_tensor(name, shape))
        ids = frame_tokens(np.random.default_rng(4).integers(0, 151643, 16))
        F = 24
        sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=2.0, max_new_tokens=F)
        p, t = eng.build_prompt(ids, 0)
        codes = eng.generate(p, t, sp, seed=SEED, stream_id=STREAM, ignore_eos=True)
        ref, mg = generate_with_penalty(orc, orc.build_prompt(ids, 0), to_osampling(sp), seed=SEED, stream=STREAM, ignore_eos=True, margins=True)
        n = _verdict(codes, ref, mg, "0.6B dims")
        plain = orc.generate(orc.build_prompt(ids, 0), qo.Sampling(1.0, 1.0, 1, 1.0, F), seed=SEED, stream=STREAM, cp_cached=True, ignore_eos=True)
        first = np.nonzero(plain[:, 0] != ref[:, 0])[0]
        print("0.6B dims: the penalty first changes code0 at frame %s, %d of %d code0 differ" % (first[:1], first.size, F))
        assert first.size and first[0] < n, "the exact prefix does not reach the first frame the penalty changes"
    finally:
        eng.close()
        orc.close()


def test_bitmap_is_per_slot_and_per_utterance(pair):
    import q3tts
    eng, orc, w = pair
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=PENALTY, max_new_tokens=40)
    # a slot that ran one utterance with a penalty, then another: the second equals a fresh engine's
    _gen_batch(eng, PROMPT_SEEDS[:1], sp)
    second = _gen_batch(eng, PROMPT_SEEDS[1:2], sp)[0]
    fresh, forc, _ = tiny_pair(seed=WEIGHT_SEED, max_batch=8, max_ctx=128)
    try:
        assert np.array_equal(second, _gen_batch(fresh, PROMPT_SEEDS[1:2], sp)[0])
        # two slots with different penalties in one batch (one off): each equals its solo run in slot 0 of a fresh engine
        # (stream ids differ per slot in _gen_batch; greedy draws do not depend on them)
        pens = [PENALTY, 1.0, 1.2]
        both = _gen_batch(eng, PROMPT_SEEDS[:3], sp, penalties=pens)
        for i in range(3):
            solo = _gen_batch(fresh, [PROMPT_SEEDS[i]], q3tts.Sampling(1.0, 1.0, 1, pens[i], 40))[0]
            assert np.array_equal(both[i], solo), i
        assert not np.array_equal(both[0][:, 0], _gen_batch(fresh, [PROMPT_SEEDS[0]], q3tts.Sampling(1.0, 1.0, 1, 1.0, 40))[0][:, 0])
    finally:
        fresh.close()
        forc.close()


def test_preempted_utterances_regenerate_the_same_codes_with_a_penalty():
    """a pool small enough to preempt (asserted), penalty on, EOS-terminated sampled generation: every utterance's codes equal the run
    with an ample pool — the re-admitted utterance starts from an empty history"""
    import q3tts
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 31), ocfg)

    def engine(pool):
        e = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=4, max_ctx=320, kv_pool_tokens=pool)
        e.load(w)
        return e
    rng = np.random.default_rng(4)
    toks = [frame_tokens(rng.integers(0, 1000, n)) for n in (5, 2, 12, 7, 3, 9)]
    sp = q3tts.Sampling(temperature=0.9, top_p=0.95, top_k=30, repetition_penalty=1.3, max_new_tokens=150)
    full = engine(0)
    try:
        _, codes_full, nfr_full = full.synthesize_batch(toks, sp, lang=2, seed=13)
        assert full.sched_stats()[1] == 0
        sp_off = q3tts.Sampling(temperature=0.9, top_p=0.95, top_k=30, repetition_penalty=1.0, max_new_tokens=150)
        _, codes_off, nfr_off = full.synthesize_batch(toks, sp_off, lang=2, seed=13)
        assert any(nfr_off[u] != nfr_full[u] or not np.array_equal(codes_off[u][:nfr_off[u]], codes_full[u][:nfr_full[u]]) for u in range(len(toks)))
    finally:
        full.close()
    small = engine(5 * 64)
    try:
        _, codes, nfr = small.synthesize_batch(toks, sp, lang=2, seed=13)
        admitted, preempted, peak = small.sched_stats()
        print("penalty 1.3, 5-page pool: admitted %d, preempted %d, peak live %d, frames %s" % (admitted, preempted, peak, list(nfr)))
        assert preempted > 0
        assert list(nfr) == list(nfr_full)
        for u in range(len(toks)):
            assert np.array_equal(codes[u][:nfr[u]], codes_full[u][:nfr[u]]), u
    finally:
        small.close()


@pytest.mark.parametrize("bad", [-1.0, math.nan, math.inf, -math.inf])
def test_bad_penalties_are_refused_and_arm_nothing(pair, bad):
    import q3tts
    eng, _, _ = pair
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=bad, max_new_tokens=8)
    p, t = eng.build_prompt(prompt_ids(1), 0)
    with pytest.raises(RuntimeError, match="repetition_penalty must be positive"):
        eng.slot_begin(0, p, t, sp, seed=1, stream_id=0, ignore_eos=True)
    assert eng.decode_steps(1) == 0                      # nothing armed
    with pytest.raises(RuntimeError, match="repetition_penalty must be positive"):
        eng.synthesize_batch([prompt_ids(1), prompt_ids(2)], sp, seed=1, ignore_eos=True)
    assert eng.decode_steps(1) == 0
    with pytest.raises(RuntimeError, match="repetition_penalty must be positive"):
        eng.sample_hist(np.zeros(96, np.float32), sp, 0.5, [1])


def test_cli_rep_penalty(tmp_path):
    """leaxer-tts --rep-penalty: the WAV differs from the run without the flag and equals a second run with it"""
    def run(name, extra):
        out = tmp_path / name
        r = subprocess.run([CLI, "-m", "synthetic:0", "--tokens", "11,22,33,44,55,66", "-o", str(out), "--top-k", "1", "--max-tokens", "24",
                            "--seed", "3"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(out, "rb").read()
    plain = run("a.wav", [])
    pen = run("b.wav", ["--rep-penalty", "1.5"])
    again = run("c.wav", ["--rep-penalty", "1.5"])
    assert pen == again
    assert pen != plain
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "--rep-penalty" in r.stdout
