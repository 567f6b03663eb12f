"""Vocoder streams and the streaming scheduler delivering through a tone stage (q3tts_codec_stream_set_tone,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_tone).  References: the plain-Python restatement (tests/tone_ref.py) fed
the library's coefficients and the 24 kHz PCM that the same sequence of calls returns from streams without a stage; and, for all six
stages together, the standalone stages (each held against its own restatement in its own test) chained by hand.  The same calls give
the same vocoder bits and every stage's output is a function of its input alone, so every comparison is byte for byte.  Tiny synthetic
config; pushes of 1 / 2 / 5 and of 5 / 2 / 1 frames."""
import numpy as np
import pytest

import q3tts
import tone_ref as R
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

NF = 8
CUTS = [(1, 2, 5), (5, 2, 1)]
TEL, WIDE = R.SECTIONS[5], R.SECTIONS[8]


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
    staged = [any(v is not None for v in kw.values()) for kw in kinds]
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


def chain(eng, pushes, pitch=None, speed=None, tone=None, loud=None, level=None, sink=None):
    """the standalone stages in the stream's order, push by push, the last with finish"""
    for begin, push, end, args in ((eng.pitch_begin, eng.pitch_push_batch, eng.pitch_end, pitch),
                                   (eng.speed_begin, eng.speed_push_batch, eng.speed_end, speed),
                                   (eng.tone_begin, eng.tone_push_batch, eng.tone_end, tone),
                                   (eng.loudness_begin, eng.loudness_push_batch, eng.loudness_end, loud),
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


def test_streams_with_only_a_tone(eng, codes, plain):
    whole = {}
    for pushes in CUTS:
        got = push_sequence(eng, codes, [dict(tone="telephone"), dict(tone=WIDE)], pushes)
        for i, sec in enumerate((TEL, WIDE)):
            for k in range(len(pushes)):
                assert got[i][k].dtype == np.float32 and got[i][k].size == plain[pushes][i][k].size, (pushes, i, k)   # it emits what it receives
            y = np.concatenate(got[i])
            want = R.cascade(np.concatenate(plain[pushes][i]), q3tts.tone_coeffs(sec))
            assert np.abs(y).max() > 0 and y.tobytes() == want.tobytes(), (pushes, i)
            whole.setdefault(i, []).append(y)
    for i in whole:                                                                                   # however the frames were cut
        assert whole[i][0].tobytes() == whole[i][1].tobytes(), i


def test_streams_without_a_tone_beside_streams_with_one(eng, codes, plain):
    for pushes in CUTS:
        mixed = push_sequence(eng, codes, [dict(tone="warm"), {}], pushes)
        other = push_sequence(eng, codes, [dict(tone=None), dict(tone="rumble")], pushes)     # no sections: no stage
        for k in range(len(pushes)):
            assert mixed[1][k].tobytes() == plain[pushes][1][k].tobytes(), (pushes, k)         # the bytes of a batch where nobody has one
            assert other[0][k].tobytes() == plain[pushes][0][k].tobytes(), (pushes, k)
        assert np.concatenate(mixed[0]).tobytes() == R.cascade(np.concatenate(plain[pushes][0]), q3tts.tone_coeffs("warm")).tobytes()


def test_streams_with_all_six_stages(eng, codes, plain):
    whole = []
    for pushes in CUTS:
        kinds = [dict(pitch=1260, speed=1250, tone="telephone", loudness=-16.0, gain_db=6.0, ceiling=0.5, sample_rate=8000, dtype="mulaw"),
                 dict(pitch=891, speed=750, tone=WIDE, loudness=-30.0, loudness_range=12.0, loudness_start=3.0, gain_db=-3.0, sample_rate=48000, dtype="float32")]
        both = push_sequence(eng, codes, kinds, pushes)
        for i, (P, S, T, L, lv, sink) in enumerate([(1260, 1250, TEL, (-160, 200, 0), (60, 500), (8000, "mulaw")),
                                                    (891, 750, WIDE, (-300, 120, 30), (-30, 0), (48000, "float32"))]):
            ref = chain(eng, plain[pushes][i], pitch=(P,), speed=(S,), tone=(T,), loud=L, level=lv, sink=sink)
            for k in range(len(pushes)):
                assert both[i][k].dtype == ref[k].dtype and both[i][k].tobytes() == ref[k].tobytes(), (pushes, i, k)
            assert len(set(np.concatenate(both[i]).tolist())) > 8
        whole.append(np.concatenate(both[0]))
    assert whole[0].tobytes() == whole[1].tobytes()
    # the tone stage with each neighbour alone: every hand-over into and out of the stage
    pushes = CUTS[0]
    for kw, ch in ((dict(speed=1250, tone="telephone"), dict(speed=(1250,), tone=(TEL,))),
                   (dict(tone="telephone", loudness=-16.0), dict(tone=(TEL,), loud=(-160, 200, 0))),
                   (dict(tone="telephone", gain_db=6.0, ceiling=0.5), dict(tone=(TEL,), level=(60, 500))),
                   (dict(tone="telephone", sample_rate=8000, dtype="int16"), dict(tone=(TEL,), sink=(8000, "int16"))),
                   (dict(pitch=1122, tone="telephone"), dict(pitch=(1122,), tone=(TEL,)))):
        two = push_sequence(eng, codes, [kw, kw], pushes)
        for i in range(2):
            ref = chain(eng, plain[pushes][i], **ch)
            for k in range(len(pushes)):
                assert two[i][k].dtype == ref[k].dtype and two[i][k].tobytes() == ref[k].tobytes(), (sorted(kw), i, k)


def test_refusals(eng, codes, plain):
    p0 = plain[CUTS[0]]
    a = eng.codec_stream_begin(NF, tone="telephone")
    b = eng.codec_stream_begin(NF)
    with pytest.raises(RuntimeError, match="has a tone"):   # the float entries refuse a stream with a tone stage, by name
        eng._push_batch(np.array([a, b], np.int32), [codes[0][:1], codes[1][:1]], np.array([0, 1, 2], np.int32))
    with pytest.raises(RuntimeError, match="has a tone"):
        eng.codec_stream_push(a, codes[0][:1])
    for bad, name in (([(1, 19, 0, 707)], "codec_stream_set_tone: tone: section 0 freq_hz 19"), ([(5, 300, 0, 707)] * 9, "9 sections"),
                      ([(1, 300, 0, 707), (2, 300, 1, 707)], "section 1 gain_cb 1 centibels must be 0")):
        with pytest.raises(RuntimeError, match=name):
            eng.codec_stream_set_tone(b, bad)
    out = eng.codec_stream_push_batch([a, b], [codes[0][:1], codes[1][:1]])   # nothing above moved either stream
    assert out[0].size == p0[0][0].size and np.array_equal(out[1], p0[1][0])
    assert out[0].tobytes() == R.cascade(p0[0][0], q3tts.tone_coeffs("telephone")).tobytes()
    for sid in (a, b):                                       # set_tone after the first sample is refused, by name
        with pytest.raises(RuntimeError, match="codec_stream_set_tone: stream %d has already delivered samples" % sid):
            eng.codec_stream_set_tone(sid, "rumble")
    assert eng.codec_stream_push_batch([a], [codes[0][:0]], finish=[True])[0].size == 0   # a push of 0 frames with finish: nothing is flushed
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([a], [codes[0][1:3]])
    eng.codec_stream_end(a)
    eng.codec_stream_end(b)


def test_scheduler_with_a_tone(eng):
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=14)   # greedy
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
    log1, pcm1, codes1, nf1 = run(tone="telephone")
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    c = q3tts.tone_coeffs("telephone")
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [x[3] for x in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        got = np.concatenate([x[2] for x in calls])
        assert got.dtype == np.float32 and np.array_equal(got, pcm1[u]) and got.size == pcm0[u].size, u   # the calls add up to the plain length
        assert got.tobytes() == R.cascade(pcm0[u], c).tobytes(), u         # each utterance: the restatement of the same job without tone
        assert got.tobytes() != pcm0[u].tobytes()
    # with the tone taken away the run is the parent-style run again
    log2, pcm2, codes2, nf2 = run()
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u]) and np.array_equal(pcm0[u], pcm2[u])
    with pytest.raises(RuntimeError, match="engine_set_tone: tone: section 0 q_permille 99"):
        eng.set_tone([(1, 300, 0, 99)])
    # with a sink as well: tone -> sink, the telephone leg
    log3, pcm3, codes3, nf3 = run(tone="telephone", sample_rate=8000, dtype="mulaw")
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes3[u])
        ref = chain(eng, [pcm0[u]], tone=("telephone",), sink=(8000, "mulaw"))[0]
        assert pcm3[u].dtype == np.uint8 and pcm3[u].tobytes() == ref.tobytes(), u
