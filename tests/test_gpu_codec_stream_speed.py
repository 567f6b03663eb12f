"""Vocoder streams and the streaming scheduler delivering through a stretcher (q3tts_codec_stream_set_speed,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_speed).  Reference: the standalone stage (tests/test_gpu_speed.py, itself held
bit for bit against numpy) fed the 24 kHz PCM that the same sequence of calls returns from streams without a speed.  The same calls
give the same vocoder bits and the stage's output is a function of its input alone, so every comparison is np.array_equal.  Tiny
synthetic config; pushes of 1 / 3 / 25 frames: a push that completes no frame, one shorter than the carry, one of many frames."""
import numpy as np
import pytest

import q3tts
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

PUSHES = [1, 3, 25]
NF = sum(PUSHES)


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=256)
    orc.close()
    yield e
    e.close()


def push_sequence(eng, codes, kinds):
    """one stream per entry of kinds = (sample_rate, dtype, speed), pushes of 1 + 3 + 25 frames, the last with finish where the stream
    has a stage -> per stream the list of pushes"""
    sids = [eng.codec_stream_begin(NF, sample_rate=r, dtype=d, speed=s) for r, d, s in kinds]
    staged = [not (r == 24000 and d == "float32" and s in (None, 1000)) for r, d, s in kinds]
    parts, at = [[] for _ in kinds], 0
    for k, n in enumerate(PUSHES):
        last = k + 1 == len(PUSHES)
        out = eng.codec_stream_push_batch(sids, [c[at:at + n] for c in codes], finish=[last and s for s in staged] if any(staged) else None)
        for i, o in enumerate(out):
            parts[i].append(o)
        at += n
    for s in sids:
        eng.codec_stream_end(s)
    return parts


def standalone_speed(eng, S, pushes):
    sid = eng.speed_begin(S)
    out = [eng.speed_push_batch([sid], [p], [k + 1 == len(pushes)])[0] for k, p in enumerate(pushes)]
    eng.speed_end(sid)
    return out


def standalone_sink(eng, rate, dtype, pushes):
    sid = eng.pcm_sink_begin(rate, dtype)
    out = [eng.pcm_sink_push_batch([sid], [p], [k + 1 == len(pushes)])[0] for k, p in enumerate(pushes)]
    eng.pcm_sink_end(sid)
    return out


@pytest.fixture(scope="module")
def codes(eng):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(9)
    return [rng.integers(0, CB, (NF, G)).astype(np.int64) for _ in range(2)]


@pytest.fixture(scope="module")
def plain(eng, codes):
    """the two streams without any stage, under the same cuts: computed once, shared, never modified"""
    p = push_sequence(eng, codes, [(24000, "float32", None), (24000, "float32", None)])
    assert sum(a.size for a in p[0]) == eng.codec_decode_len(NF)
    return p


def test_streams_with_a_speed(eng, codes, plain):
    sped = push_sequence(eng, codes, [(24000, "float32", 750), (24000, "float32", 1500)])
    for i, S in enumerate((750, 1500)):
        ref = standalone_speed(eng, S, plain[i])
        got24 = 0
        for k in range(len(PUSHES)):
            before = q3tts.speed_emitted(S, got24)
            got24 += plain[i][k].size
            assert sped[i][k].size == q3tts.speed_emitted(S, got24, k + 1 == len(PUSHES)) - before, (i, k)   # lengths by the host rule
            assert sped[i][k].dtype == np.float32 and np.array_equal(sped[i][k].view(np.uint32), ref[k].view(np.uint32)), (i, k)
        assert sum(p.size for p in sped[i]) == -(-1000 * got24 // S)
    # speed 1000 is no stage: the parent's bytes, and a stream without a speed beside a sped one is untouched
    mixed = push_sequence(eng, codes, [(24000, "float32", 1000), (24000, "float32", 1250)])
    for k in range(len(PUSHES)):
        assert np.array_equal(mixed[0][k].view(np.uint32), plain[0][k].view(np.uint32)), k


def test_streams_with_a_speed_and_a_sink(eng, codes, plain):
    both = push_sequence(eng, codes, [(8000, "int16", 1250), (48000, "float32", 750)])
    for i, (rate, dtype, S) in enumerate([(8000, "int16", 1250), (48000, "float32", 750)]):
        mid = standalone_speed(eng, S, plain[i])              # the standalone stage, then the standalone sink
        ref = standalone_sink(eng, rate, dtype, mid)
        total_mid = 0
        for k in range(len(PUSHES)):
            before = q3tts.sink_emitted(rate, total_mid)
            total_mid += mid[k].size                          # the sink's n_in is the stretcher's push length
            assert both[i][k].size == q3tts.sink_emitted(rate, total_mid, k + 1 == len(PUSHES)) - before, (i, k)
            assert both[i][k].dtype == ref[k].dtype and np.array_equal(both[i][k], ref[k]), (i, k)
        assert np.abs(np.concatenate(both[i]).astype(np.float64)).max() > 0


def test_refusals(eng, codes, plain):
    a = eng.codec_stream_begin(NF, speed=750)
    b = eng.codec_stream_begin(NF)
    with pytest.raises(RuntimeError, match="has a speed"):   # the float entries refuse a stream with a speed, by name
        eng._push_batch(np.array([a, b], np.int32), [codes[0][:1], codes[1][:1]], np.array([0, 1, 2], np.int32))
    with pytest.raises(RuntimeError, match="has a speed"):
        eng.codec_stream_push(a, codes[0][:1])
    for S in (499, 2001):
        with pytest.raises(RuntimeError, match=str(S)):
            eng.codec_stream_set_speed(b, S)
    out = eng.codec_stream_push_batch([a, b], [codes[0][:1], codes[1][:1]])   # nothing above moved either stream
    assert out[0].size == q3tts.speed_emitted(750, plain[0][0].size) and np.array_equal(out[1], plain[1][0])
    for sid in (a, b):                                       # set_speed after the first sample (a: after the first push) is refused
        with pytest.raises(RuntimeError, match="already delivered"):
            eng.codec_stream_set_speed(sid, 1250)
    tail = eng.codec_stream_push_batch([a], [codes[0][:0]], finish=[True])[0]   # a push of 0 frames with finish flushes the tail
    assert out[0].size + tail.size == -(-1000 * plain[0][0].size // 750) and tail.size > 0
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([a], [codes[0][1:3]])
    eng.codec_stream_end(a)
    eng.codec_stream_end(b)


def test_scheduler_with_a_speed(eng):
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=14)   # greedy
    toks = [frame_tokens([11, 22, 33]), frame_tokens([5, 6, 7, 8]), frame_tokens([40, 41]), frame_tokens([9, 10, 12])]
    caps = [14, 6, 9, 3]
    kw = dict(seed=5, ignore_eos=True, max_new_per_utt=caps)
    S = 1250

    def run(**extra):
        log = [[] for _ in toks]

        def on_audio(utt, fb, fe, pcm, fin):
            log[utt].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_stream(toks, sp, 4, on_audio, **kw, **extra)
        return log, pcm, codes, nf
    log0, pcm0, codes0, nf0 = run()
    log1, pcm1, codes1, nf1 = run(speed=S)
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        got = np.concatenate([c[2] for c in calls])
        assert got.dtype == np.float32 and np.array_equal(got, pcm1[u])
        n24 = pcm0[u].size
        assert got.size == -(-1000 * n24 // S), u
        ref = standalone_speed(eng, S, [pcm0[u]])[0]                       # the stage is cut-invariant: one push + finish
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), u
    # with the speed taken away the run is the parent-style run again
    log2, pcm2, codes2, nf2 = run()
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u]) and np.array_equal(pcm0[u], pcm2[u])
    # through a sink as well: the sink's format, the stretched length resampled
    log3, pcm3, codes3, nf3 = run(speed=S, sample_rate=8000, dtype="int16")
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes3[u])
        mid = standalone_speed(eng, S, [pcm0[u]])
        assert pcm3[u].dtype == np.int16 and np.array_equal(pcm3[u], standalone_sink(eng, 8000, "int16", mid)[0]), u
