"""Primed vocoder streams (q3tts_codec_stream_prime_batch_host, q3tts_slots_codec_prime, q3tts_codec_stream_info) and the streaming
scheduler behind prefix codes (q3tts_synthesize_continue_stream_host).  Tolerances are the project's own (tests/test_gpu_codec.py,
tests/test_gpu_stream_batch.py): codes bit-exact, PCM 2e-5 max-abs against the one-shot decode of the same codes, 1e-4 RMS against the
CPU oracle.

The control "a stream that PUSHED the frames reports a larger capacity" needs a push that outgrows what q3tts_codec_stream_begin
allocates (64 K / V rows at the tiny config, 256 at 0.6B dims).  40 frames at the tiny config and 150 at 0.6B dims do not, so the
controls use 90 and 300 frames, primed on one stream and pushed on another."""
import statistics

import numpy as np
import pytest

import q3_oracle as qo
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

ABS, RMS = 2e-5, 1e-4


def stage_b_context(cfg):
    """Engine::codec_stage_b_context() from the config: frames the stages behind the pre-transformer look back"""
    frames, rate = 0.0, 1.0
    for s in range(cfg.cd_n_up):
        rate *= cfg.cd_up_ratios[s]
        frames += 6.0 / rate
    frames += 6.0 / rate
    for i in range(cfg.cd_n_blocks):
        frames += 1.0 / rate
        rate *= cfg.cd_up_rates[i]
        frames += 6.0 * (1 + 3 + 9) / rate
    frames += 6.0 / rate
    return int(frames) + 3


@pytest.fixture(scope="module")
def pair():
    eng, orc, w = tiny_pair(seed=2, max_batch=3, max_ctx=512, flags=32)   # Q3TTS_FLAG_TEST_HOOKS: poison_workspace below
    yield eng, orc, w
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def full():
    """ONE 0.6B-dims engine (synthetic fill) for the full-size tests of this file."""
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=512)
    eng.fill_synthetic(seed=0)
    yield eng
    eng.close()


def rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def tail_of(eng, whole, n):
    return whole[(eng.codec_decode_len(n) if n else 0):]


# ---- 1. priming equals pushing, tiny config (head size 16: k_attn) ----
REST = (3, 6)


def tiny_cases(eng):
    ctx = stage_b_context(eng.cfg)
    assert ctx > 6
    return [0, 1, 2, 3, 4, 5, ctx - 1, ctx, ctx + 1, 40, 90]


@pytest.fixture(scope="module")
def tiny_codes(pair):
    eng, orc, _ = pair
    rng = np.random.default_rng(17)
    ns = tiny_cases(eng)
    codes = [rng.integers(0, eng.cfg.cd_codebook, (n + sum(REST), eng.cfg.n_groups)).astype(np.int64) for n in ns]
    return ns, codes


@pytest.fixture(scope="module")
def tiny_wholes(pair, tiny_codes):
    """one-shot decodes of the GPU and of the oracle, computed once"""
    eng, orc, _ = pair
    _, codes = tiny_codes
    return [eng.codec_decode(c) for c in codes], [orc.vocoder(c) for c in codes]


def prime_then_push(eng, ns, codes, poison=False, check_info=False):
    sids = [eng.codec_stream_begin(c.shape[0]) for c in codes]
    fresh = [eng.codec_stream_info(s) for s in sids]
    if poison:
        eng.poison_workspace()
    eng.codec_stream_prime_batch(sids, [c[:n] for n, c in zip(ns, codes)])
    if check_info:
        for n, s, f in zip(ns, sids, fresh):
            assert f[0] == 0
            assert eng.codec_stream_info(s) == (n, f[1], f[2]), (n, eng.codec_stream_info(s), f)
    parts, at = [[] for _ in ns], list(ns)
    for r in REST:
        if poison:
            eng.poison_workspace()
        out = eng.codec_stream_push_batch(sids, [c[a:a + r] for a, c in zip(at, codes)])
        for i, p in enumerate(out):
            parts[i].append(p)
        at = [a + r for a in at]
    for s in sids:
        eng.codec_stream_end(s)
    return [np.concatenate(p) for p in parts]


def test_priming_equals_pushing_tiny(pair, tiny_codes, tiny_wholes):
    eng, orc, _ = pair
    ns, codes = tiny_codes
    wholes, owholes = tiny_wholes
    got = prime_then_push(eng, ns, codes, check_info=True)
    for n, g, w, ow in zip(ns, got, wholes, owholes):
        want, owant = tail_of(eng, w, n), tail_of(eng, ow, n)
        assert g.shape == want.shape and g.size > 0, n
        d, r = float(np.abs(g - want).max()), rms(g, owant)
        print("tiny, primed with %d frames: max-abs vs one-shot tail %.3g, rms vs oracle tail %.3g" % (n, d, r))
        assert d < ABS, n
        assert r < RMS, n
    again = prime_then_push(eng, ns, codes)
    for n, a, g in zip(ns, again, got):
        assert np.array_equal(a, g), n                       # same calls, same bits
    poisoned = prime_then_push(eng, ns, codes, poison=True)
    for n, a, g in zip(ns, poisoned, got):
        assert np.isfinite(a).all(), n                       # nothing read that the calls did not write
        assert np.array_equal(a, g), n
    # control: the parent's only way to this state — pushing the frames — grows the stream's buffers; priming does not
    c90 = codes[ns.index(90)]
    sp, sq = eng.codec_stream_begin(c90.shape[0]), eng.codec_stream_begin(c90.shape[0])
    fresh = eng.codec_stream_info(sp)
    eng.codec_stream_prime_batch([sp], [c90[:90]])
    eng.codec_stream_push_batch([sq], [c90[:90]])
    primed, pushed = eng.codec_stream_info(sp), eng.codec_stream_info(sq)
    eng.codec_stream_end(sp)
    eng.codec_stream_end(sq)
    print("tiny, 90 frames: fresh %s, primed %s, pushed %s" % (fresh, primed, pushed))
    assert primed == (90, fresh[1], fresh[2]) and pushed[0] == 90
    assert pushed[1] > primed[1] and pushed[2] > primed[2]


# ---- 2. the same at 0.6B codec dims (window 72, head size 64: k_attn_win) ----
def test_priming_equals_pushing_06b_dims(full):
    eng = full
    rng = np.random.default_rng(29)
    ns, NEW = [1, 70, 71, 72, 73, 150], 20
    codes = [rng.integers(0, eng.cfg.cd_codebook, (n + NEW, eng.cfg.n_groups)).astype(np.int64) for n in ns]
    sids = [eng.codec_stream_begin(c.shape[0]) for c in codes]
    fresh = [eng.codec_stream_info(s) for s in sids]
    eng.codec_stream_prime_batch(sids, [c[:n] for n, c in zip(ns, codes)])
    for n, s, f in zip(ns, sids, fresh):
        assert eng.codec_stream_info(s) == (n, f[1], f[2]), n
    out = eng.codec_stream_push_batch(sids, [c[n:] for n, c in zip(ns, codes)])
    for s in sids:
        eng.codec_stream_end(s)
    for n, g, c in zip(ns, out, codes):
        want = tail_of(eng, eng.codec_decode(c), n)
        assert g.shape == want.shape, n
        d = float(np.abs(g - want).max())
        print("0.6B dims, primed with %d frames: max-abs vs one-shot tail %.3g" % (n, d))
        assert d < ABS, n
    # control: a push that outgrows the begun buffer (more than its 256 rows) grows it for good, priming the same frames does not
    c300 = rng.integers(0, eng.cfg.cd_codebook, (300, eng.cfg.n_groups)).astype(np.int64)
    sp, sq = eng.codec_stream_begin(300), eng.codec_stream_begin(300)
    begun = eng.codec_stream_info(sp)
    assert eng.codec_stream_info(sq) == begun
    eng.codec_stream_prime_batch([sp], [c300])
    eng.codec_stream_push_batch([sq], [c300])
    primed, pushed = eng.codec_stream_info(sp), eng.codec_stream_info(sq)
    eng.codec_stream_end(sp)
    eng.codec_stream_end(sq)
    print("0.6B dims, 300 frames: begun %s, primed %s, pushed %s" % (begun, primed, pushed))
    assert primed == (300, begun[1], begun[2]) and pushed[0] == 300
    assert pushed[1] > primed[1] and pushed[2] > primed[2]


# ---- 3. validation moves nothing ----
def test_validation_moves_nothing(pair, tiny_codes, tiny_wholes):
    eng, _, _ = pair
    ns, codes = tiny_codes
    want = prime_then_push(eng, ns, codes)
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    ca, cb = codes[ns.index(5)], codes[ns.index(40)]
    sa, sb, sc, sd = (eng.codec_stream_begin(49) for _ in range(4))
    eng.codec_stream_end(sc)
    eng.codec_stream_push_batch([sd], [cb[:2]])
    bad = ca[:5].copy()
    bad[3, 1] = CB
    ids32 = np.array([sa, sb], np.int32)
    flat = np.ascontiguousarray(np.concatenate([ca[:5], cb[:40]]))

    def raw(offs):
        return eng._ck(eng.L.q3tts_codec_stream_prime_batch_host(eng.h, 2, ids32.ctypes.data, flat.ctypes.data, np.ascontiguousarray(offs, np.int32).ctypes.data))
    before = [eng.codec_stream_info(s) for s in (sa, sb, sd)]
    for match, call in (
        ("stream listed twice", lambda: eng.codec_stream_prime_batch([sa, sa], [ca[:5], cb[:40]])),
        ("no such stream", lambda: eng.codec_stream_prime_batch([sa, sc], [ca[:5], cb[:40]])),
        ("stream already has frames", lambda: eng.codec_stream_prime_batch([sa, sd], [ca[:5], cb[:40]])),
        ("code out of range", lambda: eng.codec_stream_prime_batch([sa, sb], [bad, cb[:40]])),
        ("more frames than the stream was opened for", lambda: eng.codec_stream_prime_batch([sa, sb], [ca[:5], np.concatenate([cb, cb])[:50]])),
        ("frame_offsets must start at 0", lambda: raw([1, 5, 45])),
        ("frame_offsets must not decrease", lambda: raw([0, 5, 3])),
    ):
        with pytest.raises(RuntimeError, match=match):
            call()
        assert [eng.codec_stream_info(s) for s in (sa, sb, sd)] == before, match
    for s in (sa, sb, sd):
        eng.codec_stream_end(s)
    got = prime_then_push(eng, ns, codes)
    for n, a, g in zip(ns, got, want):
        assert np.array_equal(a, g), n


# ---- 4. slots_codec_prime ----
def test_slots_codec_prime(pair):
    import q3tts
    eng, _, _ = pair
    F0, NEW = 7, 10
    ids = frame_tokens([9, 8, 7, 6, 5])
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=NEW)
    _, plain, _ = eng.synthesize_batch([ids], q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=F0), seed=3, ignore_eos=True)
    prefix = plain[0]
    assert prefix.shape[0] == F0
    for b in range(3):
        eng.slot_release(b)
    prompt, trailing = eng.build_prompt(ids, 0)
    for b in range(2):
        eng.slot_begin(b, prompt, trailing, sp, seed=5, stream_id=0, ignore_eos=True, prefix_codes=prefix)
    eng.decode_steps(NEW)
    assert eng.slot_status(0)[0] == F0 + NEW and np.array_equal(eng.slot_codes(0), eng.slot_codes(1))
    with pytest.raises(RuntimeError, match="more frames than the slot holds"):
        eng.slots_codec_prime([0], [F0 + NEW + 1])
    with pytest.raises(RuntimeError, match="slot listed twice"):
        eng.slots_codec_prime([0, 0], [F0, F0])
    eng.slots_codec_prime([0], [F0])
    fb, fe, pcm = eng.slots_codec_decode_new([0])[0]
    assert (fb, fe) == (F0, F0 + NEW)
    want = eng.slot_codec_decode_range(1, F0, F0 + NEW, F0)
    assert pcm.shape == want.shape and pcm.size > 0
    d = float(np.abs(pcm - want).max())
    print("slots_codec_prime: new frames behind a primed prefix vs the windowed range decode: max-abs %.3g" % d)
    assert d < ABS
    for b in range(2):
        eng.slot_release(b)


# ---- 5. the scheduler ----
PREFIX = (0, 1, 7, 31, 0)
NEW_FRAMES = 17


def _job(eng, kw_s, seed):
    import q3tts
    rng = np.random.default_rng(3)
    toks = [frame_tokens(rng.integers(0, 1000, 2 + u % 4)) for u in range(len(PREFIX))]
    _, plain, _ = eng.synthesize_batch(toks, q3tts.Sampling(max_new_tokens=max(PREFIX), **kw_s), seed=seed, ignore_eos=True)
    pre = [plain[u][:n] if n else None for u, n in enumerate(PREFIX)]
    return toks, pre, q3tts.Sampling(max_new_tokens=NEW_FRAMES, **kw_s)


def _check_stream_job(eng, kw_s, ignore_eos, seed):
    toks, pre, sp = _job(eng, kw_s, seed)
    kw = dict(seed=seed, ignore_eos=ignore_eos)
    ref_pcm, ref_codes, ref_nf = eng.synthesize_continue(toks, pre, sp, **kw)
    log = [[] for _ in toks]

    def on_audio(utt, fb, fe, pcm, fin):
        log[utt].append((fb, fe, pcm, fin))
        return 0
    pcm, codes, nf = eng.synthesize_continue(toks, pre, sp, chunk_frames=5, on_audio=on_audio, **kw)
    assert np.array_equal(nf, ref_nf)
    if ignore_eos:
        assert list(nf) == [n + NEW_FRAMES for n in PREFIX]
    for u, n0 in enumerate(PREFIX):
        assert np.array_equal(codes[u], ref_codes[u]), u
        calls = log[u]
        assert calls and [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u
        assert calls[0][0] == n0, u
        at = n0
        for fb, fe, p, fin in calls:
            assert fb == at and fe >= fb and (fe > fb or fin), (u, fb, fe, at)
            assert p.size == (eng.codec_decode_len(fe) if fe else 0) - (eng.codec_decode_len(fb) if fb else 0)
            at = fe
        assert at == nf[u], u
        cat = np.concatenate([c[2] for c in calls])
        assert cat.shape == ref_pcm[u].shape and np.array_equal(cat, pcm[u]), u
        if cat.size:
            d = float(np.abs(cat - ref_pcm[u]).max())
            assert d < ABS, (u, d)
    return toks, sp, kw, log


@pytest.mark.parametrize("ignore_eos", [True, False])
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_streaming_scheduler_behind_prefixes(pair, mode, ignore_eos):
    eng, _, _ = pair
    kw_s = dict(temperature=1.0, top_p=1.0, top_k=1) if mode == "greedy" else dict(temperature=0.8, top_p=0.95, top_k=50)
    toks, sp, kw, log = _check_stream_job(eng, kw_s, ignore_eos, seed=11)
    # the two prefix-less utterances: q3tts_synthesize_stream_host's chunks, bit for bit
    plain = [[] for _ in toks]
    eng.synthesize_stream(toks, sp, 5, lambda utt, fb, fe, pcm, fin: plain[utt].append((fb, fe, pcm, fin)) and 0, **kw)
    for u, n0 in enumerate(PREFIX):
        if n0 == 0:
            assert len(plain[u]) == len(log[u]), u
            for a, b in zip(plain[u], log[u]):
                assert a[:2] == b[:2] and a[3] == b[3] and np.array_equal(a[2], b[2]), u


def test_streaming_scheduler_behind_prefixes_ragged(pair):
    import q3tts
    from util import to_q3cfg
    _, _, w = pair
    eng = q3tts.Engine(to_q3cfg(qo.config_tiny()), device=0, max_batch=3, max_ctx=512, flags=q3tts.FLAG_RAGGED_PREFILL)
    eng.load(w)
    try:
        _check_stream_job(eng, dict(temperature=0.8, top_p=0.95, top_k=50), True, seed=11)
    finally:
        eng.close()


def test_streaming_scheduler_cancel_and_limits(pair):
    import q3tts
    eng, _, _ = pair
    toks, pre, sp = _job(eng, dict(temperature=0.8, top_p=0.95, top_k=50), 4)
    n = [0]

    def third(utt, fb, fe, pcm, fin):
        n[0] += 1
        return 1 if n[0] == 3 else 0
    with pytest.raises(RuntimeError, match="cancelled by callback"):
        eng.synthesize_continue(toks, pre, sp, seed=4, ignore_eos=True, chunk_frames=5, on_audio=third)
    assert n[0] == 3
    assert eng.decode_steps(1) == 0                                                  # every slot is free: nothing is armed
    ref = eng.synthesize_continue(toks, pre, sp, seed=4, ignore_eos=True)
    got = eng.synthesize_continue(toks, pre, sp, seed=4, ignore_eos=True, chunk_frames=5, on_audio=lambda *a: 0)
    for u in range(len(toks)):
        assert np.array_equal(got[1][u], ref[1][u]) and float(np.abs(got[0][u] - ref[0][u]).max()) < ABS
    # prefix + prompt + cap beyond max_ctx (512): refused before anything runs
    called = []
    long_pre = [np.concatenate([pre[3]] * 16)[:480], None, None, None, None]
    with pytest.raises(RuntimeError, match="exceeds"):
        eng.synthesize_continue(toks, long_pre, q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=30), seed=4, ignore_eos=True,
                                chunk_frames=5, on_audio=lambda *a: called.append(a) and 0)
    assert not called


# ---- 8. cost guard ----
def test_priming_is_cheaper_than_the_discarded_push(full):
    """Device time (last_codec_ms) of priming 16 fresh streams x 125 frames against the batched push of the same frames on 16 other fresh
    streams (the parent's only way to the state, audio dropped): medians of 5 alternating rounds after one warm-up round.  The margin is
    1.0: priming omits the conv decoder and the upsampling stages, the larger part of the push."""
    eng = full
    rng = np.random.default_rng(41)
    NS, F, ROUNDS = 16, 125, 5
    codes = [rng.integers(0, eng.cfg.cd_codebook, (F, eng.cfg.n_groups)).astype(np.int64) for _ in range(NS)]
    A, Bt = [], []
    for r in range(ROUNDS + 1):
        sp = [eng.codec_stream_begin(F) for _ in range(NS)]
        sq = [eng.codec_stream_begin(F) for _ in range(NS)]
        eng.codec_stream_prime_batch(sp, codes)
        a = eng.last_codec_ms()
        eng.codec_stream_push_batch(sq, codes)
        b = eng.last_codec_ms()
        for s in sp + sq:
            eng.codec_stream_end(s)
        if r > 0:
            A.append(a); Bt.append(b)
    a, b = statistics.median(A), statistics.median(Bt)
    print("16 streams x 125 frames: priming %.3f ms (min %.3f max %.3f), discarded push %.3f ms (min %.3f max %.3f), ratio %.3f"
          % (a, min(A), max(A), b, min(Bt), max(Bt), a / b))
    assert a < b


# ---- 6. synthesize_icl_batch ----
def test_synthesize_icl_batch(tmp_path):
    import json
    import os
    import mimi_ref
    import q3tts
    from util import calibrate_codec
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hf_mimi_encoder.npz"))
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)
    w.update({k[2:]: z[k] for k in z.files if k.startswith("w:enc.")})
    eng = q3tts.Engine(q3tts.Config.from_dict(dict(ocfg.to_dict(), **json.loads(str(z["cfg"])))), device=0, max_batch=2, max_ctx=192)
    eng.load(w)
    try:
        clips, rates = [mimi_ref.clip(3 * 1920, 30), mimi_ref.clip(2 * 1280 + 200, 31)], [24000, 16000]
        ref_ids, toks = [[101, 102, 103, 104], [105, 106]], [frame_tokens([11, 22, 33]), frame_tokens([44, 55, 66, 77])]
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=20, max_new_tokens=7)
        alone = [eng.synthesize_icl(clips[u], ref_ids[u], toks[u], sp, seed=4, stream_id=u, ignore_eos=True, ref_rate=rates[u]) for u in range(2)]
        pcm, codes, nref = eng.synthesize_icl_batch(clips, ref_ids, toks, sp, seed=4, ignore_eos=True, ref_rates=rates)
        log = [[], []]
        spcm, scodes, snref = eng.synthesize_icl_batch(clips, ref_ids, toks, sp, seed=4, ignore_eos=True, ref_rates=rates, chunk_frames=3,
                                                       on_audio=lambda utt, fb, fe, p, fin: log[utt].append((fb, fe, p, fin)) and 0)
        for u in range(2):
            a_pcm, a_codes, a_f0 = alone[u]
            assert a_f0 >= 2 and nref[u] == a_f0 and snref[u] == a_f0
            assert np.array_equal(codes[u], a_codes) and np.array_equal(scodes[u], a_codes), u
            assert pcm[u].shape == a_pcm.shape and float(np.abs(pcm[u] - a_pcm).max()) < ABS, u
            assert log[u][0][0] == a_f0 and log[u][-1][3], u
            cat = np.concatenate([c[2] for c in log[u]])
            assert np.array_equal(cat, spcm[u]) and float(np.abs(cat - a_pcm).max()) < ABS, u
    finally:
        eng.close()


# ---- 7. the CLI ----
def _read_wav16(path):
    raw = open(path, "rb").read()
    return np.frombuffer(raw[44:], "<i2").astype(np.int32)


def test_cli_stream_chunk_behind_a_prefix(tmp_path):
    import os
    import subprocess
    import mimi_ref
    from test_gpu_cli_encode import CLI, read_codes, write_wav16
    t = lambda name: str(tmp_path / name)
    base = [CLI, "-m", "synthetic:0", "--tokens", "11,22,33,44,55", "--seed", "3"]
    r = subprocess.run(base + ["--max-tokens", "6", "--save-codes", t("a.txt"), "-o", t("a.wav")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cont = base + ["--max-tokens", "9", "--continue-codes", t("a.txt")]
    r = subprocess.run(cont + ["--save-codes", t("b0.txt"), "-o", t("b0.wav")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(cont + ["--save-codes", t("b.txt"), "-o", t("b.wav"), "--stream-chunk", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "streamed in" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(read_codes(t("b.txt")), read_codes(t("b0.txt")))
    x, y = _read_wav16(t("b.wav")), _read_wav16(t("b0.wav"))
    assert x.shape == y.shape and x.size > 0 and int(np.abs(x - y).max()) <= 1
    write_wav16(t("ref.wav"), mimi_ref.clip(2 * 1920, 41))
    icl = [CLI, "-m", "synthetic:0", "--tokens", "11,22,33", "--ref", t("ref.wav"), "--ref-tokens", "101,102", "--max-tokens", "5", "--seed", "3"]
    r = subprocess.run(icl + ["--save-codes", t("c0.txt"), "-o", t("c0.wav")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(icl + ["--save-codes", t("c.txt"), "-o", t("c.wav"), "--stream-chunk", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "new frames in" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(read_codes(t("c.txt")), read_codes(t("c0.txt")))
    x, y = _read_wav16(t("c.wav")), _read_wav16(t("c0.wav"))
    assert x.shape == y.shape and x.size > 0 and int(np.abs(x - y).max()) <= 1
