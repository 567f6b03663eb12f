"""Batched carried-state vocoder pushes (q3tts_codec_stream_push_batch_host, q3tts_slots_codec_decode_new_host) and the streaming
scheduler on top of them (q3tts_synthesize_stream_host).  Tolerances are the project's own (tests/test_gpu_codec.py): 2e-5 max-abs
against the one-shot decode of the same codes, 1e-4 RMS against the CPU oracle."""
import statistics

import numpy as np
import pytest

import q3_oracle as qo
from util import frame_tokens, tiny_pair, to_ocfg

pytestmark = pytest.mark.gpu

ABS, RMS = 2e-5, 1e-4


@pytest.fixture(scope="module")
def pair():
    eng, orc, w = tiny_pair(seed=2, max_batch=3, max_ctx=512, flags=32)   # Q3TTS_FLAG_TEST_HOOKS: q3tts_test_poison_workspace below
    yield eng, orc, w
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def full():
    """ONE 0.6B-dims engine (synthetic fill) for every full-size test of this file."""
    import q3tts
    cfg = q3tts.default_config("0.6b")
    eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=512)
    eng.fill_synthetic(seed=0)
    yield eng
    eng.close()


def rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


# 5 streams, ragged: stream 1 sits out some calls, stream 3 starts three calls late, stream 4 five calls late (fresh streams beside
# old ones: two left-context groups in one call); sizes from 1 to 130 frames — a tiny stream's K / V buffer holds 128 rows and its row
# buffer 2 x context + 64, so the larger pushes grow both and the sequence slides them several times
PATTERN = [
    (1, 4, 2, None, None),
    (13, 0, 1, None, None),
    (2, 9, 40, None, None),
    (7, 0, 3, 5, None),
    (18, 13, 64, 1, None),
    (130, 1, 7, 30, 2),
    (3, 0, 90, 66, 1),
    (64, 25, 1, 125, 33),
    (9, 70, 11, 2, 128),
]


def run_pattern(eng, codes, poison):
    sids, pos, parts = [None] * 5, [0] * 5, [[] for _ in range(5)]
    for call in PATTERN:
        ids, chunks, who = [], [], []
        for s, n in enumerate(call):
            if n is None:
                continue
            if sids[s] is None:
                sids[s] = eng.codec_stream_begin(codes[s].shape[0])
            ids.append(sids[s]); chunks.append(codes[s][pos[s]:pos[s] + n]); who.append(s)
            pos[s] += n
        if poison:
            eng.poison_workspace()
        out = eng.codec_stream_push_batch(ids, chunks)
        for s, n, pcm in zip(who, [c.shape[0] for c in chunks], out):
            if n == 0:
                assert pcm.size == 0
            parts[s].append(pcm)
    for s in range(5):
        assert pos[s] == codes[s].shape[0]
        eng.codec_stream_end(sids[s])
    return [np.concatenate(p) for p in parts]


def test_tiny_ragged_streams_equal_the_one_shot_decode(pair):
    """Tiny config: head size 16, so attention keeps k_attn stream by stream between the batched launches, and the conv decoder runs
    sequence by sequence behind the batched front (the batched conv kernels do not cover these widths)."""
    eng, orc, _ = pair
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(71)
    totals = [sum(c[s] or 0 for c in PATTERN) for s in range(5)]
    codes = [rng.integers(0, CB, (t, G)).astype(np.int64) for t in totals]
    got = run_pattern(eng, codes, poison=False)
    for s in range(5):
        whole = eng.codec_decode(codes[s])
        d = float(np.abs(got[s] - whole).max()) if got[s].shape == whole.shape else None
        r = rms(got[s], orc.vocoder(codes[s]))
        print("tiny stream %d: %d frames, max-abs vs one-shot %s, rms vs oracle %.3g" % (s, totals[s], d, r))
        assert got[s].shape == whole.shape
        assert d < ABS
        assert r < RMS
    again = run_pattern(eng, codes, poison=False)
    for s in range(5):
        assert np.array_equal(got[s], again[s]), s          # same calls, same bits
    poisoned = run_pattern(eng, codes, poison=True)
    for s in range(5):
        assert np.isfinite(poisoned[s]).all(), s            # nothing read that the call did not write
        assert np.array_equal(got[s], poisoned[s]), s


def test_validation_moves_no_stream(pair):
    eng, _, _ = pair
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(5)
    ca, cb = rng.integers(0, CB, (20, G)).astype(np.int64), rng.integers(0, CB, (14, G)).astype(np.int64)
    wa, wb = eng.codec_decode(ca), eng.codec_decode(cb)
    sa, sb, sc = eng.codec_stream_begin(20), eng.codec_stream_begin(14), eng.codec_stream_begin(8)
    eng.codec_stream_end(sc)
    pa, pb = [], []
    first = eng.codec_stream_push_batch([sa, sb], [ca[:5], cb[:3]])
    pa.append(first[0]); pb.append(first[1])
    bad = ca[5:9].copy()
    bad[2, 1] = CB
    ids32 = np.array([sa, sb], np.int32)
    for match, call in (
        ("stream listed twice", lambda: eng.codec_stream_push_batch([sa, sa], [ca[5:9], ca[9:11]])),
        ("no such stream", lambda: eng.codec_stream_push_batch([sa, sc], [ca[5:9], cb[3:5]])),
        ("frame_offsets must not decrease", lambda: eng._push_batch(ids32, [ca[5:9], cb[3:5]], np.array([0, 4, 2], np.int32))),
        ("code out of range", lambda: eng.codec_stream_push_batch([sa, sb], [bad, cb[3:5]])),
        ("more frames than the stream was opened for", lambda: eng.codec_stream_push_batch([sa, sb], [ca[5:9], cb])),
    ):
        with pytest.raises(RuntimeError, match=match):
            call()
        nxt = eng.codec_stream_push_batch([sa, sb], [ca[_done(pa, eng):][:3], cb[_done(pb, eng):][:2]])
        pa.append(nxt[0]); pb.append(nxt[1])
    last = eng.codec_stream_push_batch([sa, sb], [ca[_done(pa, eng):], cb[_done(pb, eng):]])
    pa.append(last[0]); pb.append(last[1])
    ga, gb = np.concatenate(pa), np.concatenate(pb)
    assert ga.shape == wa.shape and gb.shape == wb.shape
    assert float(np.abs(ga - wa).max()) < ABS and float(np.abs(gb - wb).max()) < ABS
    eng.codec_stream_end(sa)
    eng.codec_stream_end(sb)


def _done(parts, eng):
    """frames behind the samples delivered so far (the decoder's length formula is strictly increasing)"""
    n, f = sum(p.size for p in parts), 0
    while f < 4096 and (eng.codec_decode_len(f) if f else 0) < n:
        f += 1
    assert (eng.codec_decode_len(f) if f else 0) == n
    return f


def test_single_and_batched_pushes_interleave(pair):
    eng, _, _ = pair
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(9)
    ca, cb = rng.integers(0, CB, (60, G)).astype(np.int64), rng.integers(0, CB, (60, G)).astype(np.int64)
    sa, sb = eng.codec_stream_begin(60), eng.codec_stream_begin(60)
    pa, pb, i = [], [], 0
    for k, n in enumerate((3, 11, 1, 20, 6, 19)):
        if k % 2 == 0:
            pa.append(eng.codec_stream_push(sa, ca[i:i + n])); pb.append(eng.codec_stream_push(sb, cb[i:i + n]))
        else:
            out = eng.codec_stream_push_batch([sb, sa], [cb[i:i + n], ca[i:i + n]])
            pa.append(out[1]); pb.append(out[0])
        i += n
    assert i == 60
    for got, c in ((np.concatenate(pa), ca), (np.concatenate(pb), cb)):
        whole = eng.codec_decode(c)
        assert got.shape == whole.shape and float(np.abs(got - whole).max()) < ABS
    eng.codec_stream_end(sa)
    eng.codec_stream_end(sb)


def test_slots_decode_new_alternates_with_the_range_decode(pair):
    import q3tts
    eng, orc, _ = pair
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=40)
    for b in range(3):
        eng.slot_release(b)
    for b, text in enumerate(([9, 8, 7, 6, 5], [4, 3, 2])):
        prompt, trailing = eng.build_prompt(frame_tokens(text), 0)
        eng.slot_begin(b, prompt, trailing, sp, seed=5, stream_id=b, ignore_eos=True)
    parts, done = [[], []], [0, 0]
    for k, step in enumerate((3, 8, 1, 12, 5, 11)):
        eng.decode_steps(step)
        nf = eng.slot_status(0)[0]
        if k % 2 == 0:
            for b, (fb, fe, pcm) in enumerate(eng.slots_codec_decode_new([0, 1])):
                assert (fb, fe) == (done[b], nf)
                parts[b].append(pcm)
        else:
            out = eng.slots_codec_decode_new([1])
            assert out[0][:2] == (done[1], nf)
            parts[1].append(out[0][2])
            parts[0].append(eng.slot_codec_decode_range(0, done[0], nf, left_context=nf))
        done = [nf, nf]
    fb, fe, pcm = eng.slots_codec_decode_new([0])[0]
    assert (fb, fe) == (40, 40) and pcm.size == 0          # nothing new: the stream is left where it is
    for b in range(2):
        whole = eng.slot_codec_decode(b)
        got = np.concatenate(parts[b])
        assert got.shape == whole.shape and float(np.abs(got - whole).max()) < ABS
        assert rms(got, orc.vocoder(eng.slot_codes(b))) < RMS
    for b in range(2):
        eng.slot_release(b)


def _job(eng, ignore_eos, seed):
    import q3tts
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=30)
    rng = np.random.default_rng(3)
    toks = [frame_tokens(rng.integers(0, 1000, 2 + u % 5)) for u in range(11)]
    caps = [30, 7, 19, 1, 26, 12, 30, 5, 22, 9, 16] if ignore_eos else None
    return sp, toks, caps, dict(seed=seed, ignore_eos=ignore_eos, max_new_per_utt=caps)


@pytest.mark.parametrize("ignore_eos", [True, False])
def test_streaming_scheduler(pair, ignore_eos):
    """11 utterances over 3 slots: chunks contiguous from frame 0, `finished` once and last, codes bit-equal to the schedule entry's,
    concatenated chunks within 2e-5 of its PCM (and the entry's own concatenation equal to the chunks)."""
    eng, _, _ = pair
    sp, toks, caps, kw = _job(eng, ignore_eos, seed=11)
    ref_pcm, ref_codes, ref_nf = eng.synthesize_batch(toks, sp, **kw)
    log = [[] for _ in toks]

    def on_audio(utt, fb, fe, pcm, fin):
        log[utt].append((fb, fe, pcm, fin))
        return 0
    pcm, codes, nf = eng.synthesize_stream(toks, sp, 4, on_audio, **kw)
    assert np.array_equal(nf, ref_nf)
    if ignore_eos:
        assert list(nf) == caps
    for u in range(len(toks)):
        assert np.array_equal(codes[u], ref_codes[u]), u
        calls = log[u]
        assert calls and [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u
        at = 0
        for fb, fe, p, fin in calls:
            assert fb == at and fe >= fb and (fe > fb or fin), (u, fb, fe, at)
            assert p.size == (eng.codec_decode_len(fe) if fe else 0) - (eng.codec_decode_len(fb) if fb else 0)
            at = fe
        assert at == nf[u], u
        cat = np.concatenate([c[2] for c in calls])
        assert cat.shape == ref_pcm[u].shape and np.array_equal(cat, pcm[u]), u
        if cat.size:
            assert float(np.abs(cat - ref_pcm[u]).max()) < ABS, u


def test_streaming_scheduler_cancel(pair):
    eng, _, _ = pair
    sp, toks, caps, kw = _job(eng, True, seed=4)
    n = [0]

    def third(utt, fb, fe, pcm, fin):
        n[0] += 1
        return 1 if n[0] == 3 else 0
    with pytest.raises(RuntimeError, match="cancelled by callback"):
        eng.synthesize_stream(toks, sp, 4, third, **kw)
    assert n[0] == 3
    ref_pcm, ref_codes, ref_nf = eng.synthesize_batch(toks[:4], sp, seed=4, ignore_eos=True, max_new_per_utt=caps[:4])
    pcm, codes, nf = eng.synthesize_stream(toks[:4], sp, 5, lambda *a: 0, seed=4, ignore_eos=True, max_new_per_utt=caps[:4])
    for u in range(4):
        assert np.array_equal(codes[u], ref_codes[u]) and float(np.abs(pcm[u] - ref_pcm[u]).max()) < ABS


def test_full_size_16_streams(full):
    """0.6B dims: k_attn_win's sibling across the 72-frame window and several buffer slides, the conv decoder as one batch per push.
    16 streams x 300 frames in pushes of 25; stream 3 in pushes of 7, stream 11 in pushes of 40 (ragged rows, different slide times)."""
    import q3tts
    eng = full
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(123)
    F, NS = 300, 16
    codes = [rng.integers(0, CB, (F, G)).astype(np.int64) for _ in range(NS)]
    step = [25] * NS
    step[3], step[11] = 7, 40
    sids = [eng.codec_stream_begin(F) for _ in range(NS)]
    pos, parts = [0] * NS, [[] for _ in range(NS)]
    while any(p < F for p in pos):
        chunks = [codes[s][pos[s]:pos[s] + step[s]] for s in range(NS)]
        out = eng.codec_stream_push_batch(sids, chunks)
        for s in range(NS):
            parts[s].append(out[s]); pos[s] += chunks[s].shape[0]
    worst = 0.0
    for s in range(NS):
        eng.codec_stream_end(sids[s])
        whole = eng.codec_decode(codes[s])
        got = np.concatenate(parts[s])
        assert got.shape == whole.shape
        d = float(np.abs(got - whole).max())
        worst = max(worst, d)
        assert d < ABS, (s, d)
    print("0.6B dims, 16 streams x 300 frames: worst max-abs vs one-shot %.3g" % worst)
    orc = qo.Oracle(to_ocfg(eng.cfg), max_ctx=16)
    for name, shape in eng.tensor_infos():
        if name.startswith("cd."):
            orc.set_tensor(name, eng.get_tensor(name, shape))
    r = rms(np.concatenate(parts[3]), orc.vocoder(codes[3]))
    orc.close()
    print("stream 3 (pushes of 7): rms vs oracle %.3g" % r)
    assert r < RMS


def test_batched_push_is_not_slower_than_single_pushes(full):
    """(A) 64 single 25-frame pushes against (B) one batched push of the same frames, same engine, medians of five alternating rounds by
    last_codec_ms (device events).  B < A is the weakest claim the feature makes: a loop over streams would land at the ratio 1."""
    eng = full
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(7)
    NS, HIST, N, ROUNDS = 64, 100, 25, 5
    F = HIST + 2 * N + 2 * N * ROUNDS
    sids = [eng.codec_stream_begin(F) for _ in range(NS)]
    eng.codec_stream_push_batch(sids, [rng.integers(0, CB, (HIST, G)).astype(np.int64) for _ in range(NS)])   # warm history
    eng.codec_stream_push_batch(sids, [rng.integers(0, CB, (N, G)).astype(np.int64) for _ in range(NS)])      # both paths' buffers sized
    eng.codec_stream_push(sids[0], rng.integers(0, CB, (N, G)).astype(np.int64))
    eng.codec_stream_push_batch(sids[1:], [rng.integers(0, CB, (N, G)).astype(np.int64) for _ in range(NS - 1)])
    A, Bt = [], []
    for _ in range(ROUNDS):
        chunks = [rng.integers(0, CB, (N, G)).astype(np.int64) for _ in range(NS)]
        a = 0.0
        for s in range(NS):
            eng.codec_stream_push(sids[s], chunks[s])
            a += eng.last_codec_ms()
        A.append(a)
        chunks = [rng.integers(0, CB, (N, G)).astype(np.int64) for _ in range(NS)]
        eng.codec_stream_push_batch(sids, chunks)
        Bt.append(eng.last_codec_ms())
    for s in sids:
        eng.codec_stream_end(s)
    a, b = statistics.median(A), statistics.median(Bt)
    print("64 streams x 25 frames: (A) single pushes %.2f ms, (B) one batched push %.2f ms, B / A = %.3f" % (a, b, b / a))
    assert b < a
