"""Vocoder streams and the streaming scheduler delivering through a pitch stage (q3tts_codec_stream_set_pitch,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_pitch).  Reference: the standalone stages (tests/test_gpu_pitch.py,
tests/test_gpu_speed.py, tests/test_gpu_level.py, tests/test_gpu_pcm_sink.py, each held against numpy) fed the 24 kHz PCM that the
same sequence of calls returns from streams without a stage.  The same calls give the same vocoder bits and every stage's output is a
function of its input alone, so every comparison is byte for byte.  The synthetic vocoder's output may never be voiced: this file
checks the chain, tests/test_gpu_pitch.py the arithmetic.  Tiny synthetic config; pushes of 1 / 3 / 25 and of 25 / 3 / 1 frames."""
import numpy as np
import pytest

import q3tts
import pitch_ref as R
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

NF = 29
CUTS = [(1, 3, 25), (25, 3, 1)]


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=256)
    orc.close()
    yield e
    e.close()


def push_sequence(eng, codes, kinds, pushes):
    """one stream per entry of kinds = dict of codec_stream_begin's keywords; the last push with finish where the stream has a stage
    -> per stream the list of pushes"""
    sids = [eng.codec_stream_begin(NF, **kw) for kw in kinds]
    staged = [bool(kw) and kw != dict(pitch=1000) for kw in kinds]
    parts, at = [[] for _ in kinds], 0
    for k, n in enumerate(pushes):
        last = k + 1 == len(pushes)
        out = eng.codec_stream_push_batch(sids, [c[at:at + n] for c in codes], finish=[last and s for s in staged] if any(staged) else None)
        for i, o in enumerate(out):
            parts[i].append(o)
        at += n
    for s in sids:
        eng.codec_stream_end(s)
    return parts


def chain(eng, pushes, pitch=None, speed=None, level=None, sink=None):
    """the standalone stages in the stream's order, push by push, the last with finish"""
    for begin, push, end, args in ((eng.pitch_begin, eng.pitch_push_batch, eng.pitch_end, pitch),
                                   (eng.speed_begin, eng.speed_push_batch, eng.speed_end, speed),
                                   (eng.level_begin, eng.level_push_batch, eng.level_end, level),
                                   (eng.pcm_sink_begin, eng.pcm_sink_push_batch, eng.pcm_sink_end, sink)):
        if args is None:
            continue
        sid = begin(*args)
        pushes = [push([sid], [p], [k + 1 == len(pushes)])[0] for k, p in enumerate(pushes)]
        end(sid)
    return pushes


@pytest.fixture(scope="module")
def codes(eng):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(9)
    return [rng.integers(0, CB, (NF, G)).astype(np.int64) for _ in range(2)]


@pytest.fixture(scope="module")
def plain(eng, codes):
    """the two streams without any stage, per cut pattern: computed once, shared, never modified"""
    out = {}
    for pushes in CUTS:
        p = push_sequence(eng, codes, [{}, {}], pushes)
        assert sum(a.size for a in p[0]) == eng.codec_decode_len(NF)
        out[pushes] = p
    assert np.array_equal(np.concatenate(out[CUTS[0]][0]), np.concatenate(out[CUTS[1]][0]))          # the vocoder's own cut-invariance
    return out


def test_streams_with_a_pitch(eng, codes, plain):
    whole = {}
    for pushes in CUTS:
        got = push_sequence(eng, codes, [dict(pitch=794), dict(pitch=1498)], pushes)
        for i, r in enumerate((794, 1498)):
            ref = chain(eng, plain[pushes][i], pitch=(r,))
            n24 = 0
            for k in range(len(pushes)):
                before = q3tts.pitch_emitted(n24)
                n24 += plain[pushes][i][k].size
                assert got[i][k].size == q3tts.pitch_emitted(n24, k + 1 == len(pushes)) - before, (i, k)
                assert got[i][k].dtype == np.float32 and got[i][k].tobytes() == ref[k].tobytes(), (pushes, i, k)
            y = np.concatenate(got[i])
            assert y.size == n24 and np.abs(y).max() > 0                                              # the same length as without the stage
            assert y.tobytes() == R.psola32(np.concatenate(plain[pushes][i]), r).tobytes(), (pushes, i)   # and the restatement itself
            whole.setdefault(i, []).append(y)
    for i in whole:                                                                                   # however the frames were cut
        assert whole[i][0].tobytes() == whole[i][1].tobytes(), i


def test_streams_with_pitch_speed_level_and_sink(eng, codes, plain):
    whole = []
    for pushes in CUTS:
        kinds = [dict(pitch=1260, speed=1250, gain_db=6.0, ceiling=0.5, sample_rate=8000, dtype="int16"),
                 dict(pitch=891, speed=750, gain_db=-3.0, sample_rate=48000, dtype="float32")]
        both = push_sequence(eng, codes, kinds, pushes)
        for i, (P, S, lv, sink) in enumerate([(1260, 1250, (60, 500), (8000, "int16")), (891, 750, (-30, 0), (48000, "float32"))]):
            ref = chain(eng, plain[pushes][i], pitch=(P,), speed=(S,), level=lv, sink=sink)
            for k in range(len(pushes)):
                assert both[i][k].dtype == ref[k].dtype and both[i][k].tobytes() == ref[k].tobytes(), (pushes, i, k)
            assert np.abs(np.concatenate(both[i]).astype(np.float64)).max() > 0
        whole.append(np.concatenate(both[0]))
    assert whole[0].tobytes() == whole[1].tobytes()
    # pitch and level, pitch and sink: every hand-over from the first stage
    pushes = CUTS[0]
    two = push_sequence(eng, codes, [dict(pitch=1122, gain_db=6.0, ceiling=0.5), dict(pitch=1122, sample_rate=16000, dtype="int16")], pushes)
    for i, kw in enumerate((dict(level=(60, 500)), dict(sink=(16000, "int16")))):
        ref = chain(eng, plain[pushes][i], pitch=(1122,), **kw)
        for k in range(len(pushes)):
            assert two[i][k].dtype == ref[k].dtype and two[i][k].tobytes() == ref[k].tobytes(), (i, k)


def test_pitch_1000_is_no_stage(eng, codes, plain):
    pushes = CUTS[0]
    mixed = push_sequence(eng, codes, [dict(pitch=1000), dict(pitch=1260)], pushes)
    for k in range(len(pushes)):
        assert mixed[0][k].tobytes() == plain[pushes][0][k].tobytes(), k
    a, b = eng.codec_stream_begin(NF, pitch=1000), eng.codec_stream_begin(NF, pitch=1260)
    assert a not in eng.__dict__.get("_codec_stream_pitch", {}) and b in eng._codec_stream_pitch
    out = eng.codec_stream_push(a, codes[0][:1])                                   # the float entry serves it: it has no stage
    assert np.asarray(out).tobytes() == plain[pushes][0][0].tobytes()
    with pytest.raises(RuntimeError, match="has a pitch"):                         # and refuses the stream that has one, by name
        eng.codec_stream_push(b, codes[1][:1])
    with pytest.raises(RuntimeError, match="already delivered"):
        eng.codec_stream_set_pitch(a, 1260)
    for bad in (499, 2001):
        with pytest.raises(RuntimeError, match=str(bad)):
            eng.codec_stream_set_pitch(b, bad)
    eng.codec_stream_set_pitch(b, 1000)                                            # 1000 takes the stage away again
    assert np.asarray(eng.codec_stream_push(b, codes[1][:1])).tobytes() == plain[pushes][1][0].tobytes()
    # finish is allowed on a stream with a pitch stage and no sink: a push of 0 frames flushes the tail
    c = eng.codec_stream_begin(NF, pitch=794)
    head = eng.codec_stream_push_batch([c], [codes[0][:1]])[0]
    tail = eng.codec_stream_push_batch([c], [codes[0][:0]], finish=[True])[0]
    n1 = plain[pushes][0][0].size
    assert head.size == q3tts.pitch_emitted(n1) and head.size + tail.size == n1
    assert np.concatenate([head, tail]).tobytes() == R.psola32(plain[pushes][0][0], 794).tobytes()
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([c], [codes[0][1:3]])
    for s in (a, b, c):
        eng.codec_stream_end(s)


@pytest.mark.parametrize("top_k", [1, 8])
def test_scheduler_with_a_pitch(eng, top_k):
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=top_k, max_new_tokens=14)   # greedy, and sampled: the RNG's use is untouched
    toks = [frame_tokens([11, 22, 33]), frame_tokens([5, 6, 7, 8]), frame_tokens([40, 41]), frame_tokens([9, 10, 12])]
    caps = [14, 6, 9, 3]
    kw = dict(seed=5, ignore_eos=True, max_new_per_utt=caps)

    def run(**extra):
        log = [[] for _ in toks]

        def on_audio(utt, fb, fe, pcm, fin):
            log[utt].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_stream(toks, sp, 4, on_audio, **kw, **extra)
        return log, pcm, codes, nf
    log0, pcm0, codes0, nf0 = run()
    log1, pcm1, codes1, nf1 = run(pitch=1260)
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        got = np.concatenate([c[2] for c in calls])
        assert got.dtype == np.float32 and np.array_equal(got, pcm1[u])
        assert got.size == pcm0[u].size, u                                 # the calls add up to the length without the stage
        ref = chain(eng, [pcm0[u]], pitch=(1260,))[0]                      # the same samples as the standalone stage
        assert got.tobytes() == ref.tobytes(), u
    # with the pitch taken away the run is the parent-style run again (pitch=1000 is no stage)
    log2, pcm2, codes2, nf2 = run(pitch=1000)
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u]) and pcm0[u].tobytes() == pcm2[u].tobytes()
    if top_k == 1:   # with a stretcher, a level and a sink as well: pitch -> stretcher -> level -> sink
        log3, pcm3, codes3, nf3 = run(pitch=794, speed=1250, gain_db=6.0, ceiling=0.5, sample_rate=8000, dtype="int16")
        for u in range(len(toks)):
            assert np.array_equal(codes0[u], codes3[u])
            ref = chain(eng, [pcm0[u]], pitch=(794,), speed=(1250,), level=(60, 500), sink=(8000, "int16"))[0]
            assert pcm3[u].dtype == np.int16 and np.array_equal(pcm3[u], ref), u
