"""Vocoder streams and the streaming scheduler delivering through a PCM sink (q3tts_codec_stream_set_sink,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_sink).  Reference: the standalone sink (tests/test_gpu_pcm_sink.py) fed the
24 kHz PCM that the same sequence of calls returns from streams without a sink: bit-identical, so np.array_equal.  Against the fp64
fold of that PCM the tolerance is the push bound the project already
asserts (2e-5, tests/test_gpu_stream_batch.py) times sum|h|, plus the fp32 summation bound gamma_T * sum|h| * max|x| — both from the
library's own table.  Tiny synthetic config: two streams and three pushes are the smallest at which carry, finish and mixed formats
can go wrong."""
import numpy as np
import pytest

import q3tts
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

ABS = 2e-5


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=256)
    orc.close()
    yield e
    e.close()


def tolerance(rate, x):
    L, M, half, taps, tab = q3tts.sink_plan(rate)
    sum_h = float(np.abs(tab.astype(np.float64)).sum(axis=1).max())
    u = 2.0 ** -24
    return ABS * sum_h + taps * u / (1 - taps * u) * sum_h * max(float(np.abs(x).max()), ABS)


def fold64(x, rate, n_out):
    L, M, half, taps, tab = q3tts.sink_plan(rate)
    j = np.arange(n_out, dtype=np.int64)
    kc, p = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(half, np.float64), x.astype(np.float64), np.zeros(half + 1, np.float64)])
    idx = (kc + 1)[:, None] + np.arange(taps)[None, :]
    return (tab.astype(np.float64)[p] * xp[idx]).sum(axis=1)


PUSHES = [3, 5, 1]


def push_sequence(eng, codes, formats):
    """two streams, pushes of 3 + 5 + 1 frames, the last with finish where the stream has a sink -> per stream the list of pushes"""
    sids = [eng.codec_stream_begin(9, sample_rate=r, dtype=d) for r, d in formats]
    sunk = [not (r == 24000 and d == "float32") for r, d in formats]
    parts, at = [[] for _ in formats], 0
    for k, n in enumerate(PUSHES):
        last = k + 1 == len(PUSHES)
        out = eng.codec_stream_push_batch(sids, [c[at:at + n] for c in codes], finish=[last and s for s in sunk] if any(sunk) else None)
        for i, o in enumerate(out):
            parts[i].append(o)
        at += n
    for s in sids:
        eng.codec_stream_end(s)
    return parts


def test_streams_with_sinks(eng):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(9)
    codes = [rng.integers(0, CB, (9, G)).astype(np.int64) for _ in range(2)]
    plain = push_sequence(eng, codes, [(24000, "float32"), (24000, "float32")])
    sunk = push_sequence(eng, codes, [(8000, "int16"), (48000, "float32")])
    n24 = [sum(p.size for p in plain[i]) for i in range(2)]
    assert n24[0] == eng.codec_decode_len(9)
    for i, (rate, dtype) in enumerate([(8000, "int16"), (48000, "float32")]):
        # lengths by the host rule
        got24 = 0
        for k, part in enumerate(sunk[i]):
            before = q3tts.sink_emitted(rate, got24)
            got24 += plain[i][k].size
            assert part.size == q3tts.sink_emitted(rate, got24, k + 1 == len(PUSHES)) - before, (i, k)
        # the standalone sink over the sink-less streams' pushes
        sid = eng.pcm_sink_begin(rate, dtype)
        ref = [eng.pcm_sink_push_batch([sid], [plain[i][k]], [k + 1 == len(PUSHES)])[0] for k in range(len(PUSHES))]
        eng.pcm_sink_end(sid)
        got, want = np.concatenate(sunk[i]), np.concatenate(ref)
        assert got.dtype == want.dtype and got.shape == want.shape
        x = np.concatenate(plain[i])
        # Measured on an MI355X: the two are bit-identical (the same calls give the same vocoder bits, and a sink's sample depends on its
        # absolute index alone), so equality is asserted, not the tolerance; the tolerance holds the result to the fp64 fold.
        assert np.array_equal(got, want), (i, rate, dtype)
        tol = tolerance(rate, x)
        exact = fold64(x, rate, got.size)
        if dtype == "int16":
            err = float(np.abs(got.astype(np.float64) - np.clip(exact, -1.0, 1.0) * 32767.0).max())
            print("stream %d at %d int16: max |int16 - fp64 fold| = %.3g LSB (allowed 1 + %.3g)" % (i, rate, err, tol * 32767))
            assert err <= 1 + tol * 32767
        else:
            err = float(np.abs(got.astype(np.float64) - exact).max())
            print("stream %d at %d float: max |float - fp64 fold| = %.3g (allowed %.3g)" % (i, rate, err, tol))
            assert err <= tol


def test_refusals_and_untouched_neighbours(eng):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(10)
    codes = [rng.integers(0, CB, (9, G)).astype(np.int64) for _ in range(2)]
    plain = push_sequence(eng, codes, [(24000, "float32"), (24000, "float32")])
    mixed = push_sequence(eng, codes, [(24000, "float32"), (16000, "int16")])
    for k in range(len(PUSHES)):   # the sink-less stream beside a sink: the same bits as without any sink in the call
        assert mixed[0][k].dtype == np.float32 and np.array_equal(mixed[0][k], plain[0][k]), k
    a = eng.codec_stream_begin(9, sample_rate=8000, dtype="int16")
    b = eng.codec_stream_begin(9)
    with pytest.raises(RuntimeError, match="has a sink"):   # the float entry refuses a stream with a sink, by name
        eng._push_batch(np.array([a, b], np.int32), [codes[0][:3], codes[1][:3]], np.array([0, 3, 6], np.int32))
    with pytest.raises(RuntimeError, match="has a sink"):
        eng.codec_stream_push(a, codes[0][:3])
    with pytest.raises(RuntimeError, match="no sink"):      # finish belongs to sinks
        eng.codec_stream_push_batch([b], [codes[1][:3]], finish=[True])
    out = eng.codec_stream_push_batch([a, b], [codes[0][:3], codes[1][:3]])   # nothing above moved either stream
    assert out[0].dtype == np.int16 and out[0].size == q3tts.sink_emitted(8000, plain[0][0].size)
    assert np.array_equal(out[1], plain[1][0])
    for sid in (a, b):
        with pytest.raises(RuntimeError, match="already delivered"):
            eng.codec_stream_set_sink(sid, 16000, "float32")
    with pytest.raises(RuntimeError, match="3999"):
        eng.codec_stream_begin(9, sample_rate=3999)
    tail = eng.codec_stream_push_batch([a], [codes[0][:0]], finish=[True])[0]   # a push of 0 frames with finish flushes the tail
    assert tail.size == q3tts.sink_emitted(8000, plain[0][0].size, True) - out[0].size and tail.size > 0
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([a], [codes[0][3:5]])
    eng.codec_stream_end(a)
    eng.codec_stream_end(b)


def test_scheduler_through_a_sink(eng):
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=14)   # greedy
    toks = [frame_tokens([11, 22, 33]), frame_tokens([5, 6, 7, 8]), frame_tokens([40, 41])]
    caps = [14, 6, 9]
    kw = dict(seed=5, ignore_eos=True, max_new_per_utt=caps)

    def run(**extra):
        log = [[] for _ in toks]

        def on_audio(utt, fb, fe, pcm, fin):
            log[utt].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_stream(toks, sp, 4, on_audio, **kw, **extra)
        return log, pcm, codes, nf
    log0, pcm0, codes0, nf0 = run()
    log1, pcm1, codes1, nf1 = run(sample_rate=16000, dtype="int16")
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        assert [(c[0], c[1]) for c in calls] == [(c[0], c[1]) for c in log0[u]], u
        got = np.concatenate([c[2] for c in calls])
        assert got.dtype == np.int16 and np.array_equal(got, pcm1[u])
        n24 = pcm0[u].size
        assert got.size == -(-n24 * 2 // 3)
        tol = tolerance(16000, pcm0[u])
        exact = np.clip(fold64(pcm0[u], 16000, got.size), -1.0, 1.0) * 32767.0
        err = float(np.abs(got.astype(np.float64) - exact).max())
        print("utterance %d: max |int16 - fp64 fold| = %.3g LSB (allowed 1 + %.3g)" % (u, err, tol * 32767))
        assert err <= 1 + tol * 32767
    # a non-NULL pcm_out with a sink is refused
    eng.set_sink(16000, "int16", lambda *a: 0)
    try:
        with pytest.raises(RuntimeError, match="pcm_out"):
            eng.synthesize_stream(toks, sp, 4, lambda *a: 0, **kw)
    finally:
        eng.set_sink(None)
    # with the sink taken away the run is the parent-style run again
    log2, pcm2, codes2, nf2 = run()
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u])
        for c0, c2 in zip(log0[u], log2[u]):
            assert c0[0] == c2[0] and c0[1] == c2[1] and c0[3] == c2[3] and c2[2].dtype == np.float32 and np.array_equal(c0[2], c2[2])
        assert np.array_equal(pcm0[u], pcm2[u])
