"""Vocoder streams and the streaming scheduler delivering through a loudness stage (q3tts_codec_stream_set_loudness,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_loudness).  Reference: the standalone stages (tests/test_gpu_pitch.py,
tests/test_gpu_speed.py, tests/test_gpu_loudness.py, tests/test_gpu_level.py, tests/test_gpu_pcm_sink.py, each held against numpy)
chained by hand and fed the 24 kHz PCM that the same sequence of calls returns from streams without a stage.  The same calls give the
same vocoder bits and every stage's output is a function of its input alone, so every comparison is byte for byte.  Tiny synthetic
config; pushes of 1 / 3 / 25 and of 25 / 3 / 1 frames, and a subset of the streams pushing in other cuts than the rest."""
import numpy as np
import pytest

import q3tts
import loudness_ref as R
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
    staged = [bool(kw) for kw in kinds]
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


def chain(eng, pushes, pitch=None, speed=None, loud=None, level=None, sink=None):
    """the standalone stages in the stream's order, push by push, the last with finish"""
    for begin, push, end, args in ((eng.pitch_begin, eng.pitch_push_batch, eng.pitch_end, pitch),
                                   (eng.speed_begin, eng.speed_push_batch, eng.speed_end, speed),
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


def test_streams_with_a_loudness(eng, codes, plain):
    whole = {}
    for pushes in CUTS:
        got = push_sequence(eng, codes, [dict(loudness=-16.0), dict(loudness=-23.0, loudness_range=6.0, loudness_start=-10.0)], pushes)
        for i, p in enumerate(((-160, 200, 0), (-230, 60, -100))):
            ref = chain(eng, plain[pushes][i], loud=p)
            n24 = 0
            for k in range(len(pushes)):
                before = q3tts.loudness_emitted(p[0], n24)
                n24 += plain[pushes][i][k].size
                assert got[i][k].size == q3tts.loudness_emitted(p[0], n24, k + 1 == len(pushes)) - before, (i, k)
                assert got[i][k].dtype == np.float32 and got[i][k].tobytes() == ref[k].tobytes(), (pushes, i, k)
            y = np.concatenate(got[i])
            assert y.size == n24 and np.abs(y).max() > 0                                              # the same length as without the stage
            assert y.tobytes() == R.stage(np.concatenate(plain[pushes][i]), *p)[0].tobytes(), (pushes, i)   # and the restatement itself
            whole.setdefault(i, []).append(y)
    for i in whole:                                                                                   # however the frames were cut
        assert whole[i][0].tobytes() == whole[i][1].tobytes(), i


def test_streams_with_all_five_stages(eng, codes, plain):
    whole = []
    for pushes in CUTS:
        kinds = [dict(pitch=1260, speed=1250, loudness=-16.0, gain_db=6.0, ceiling=0.5, sample_rate=8000, dtype="int16"),
                 dict(pitch=891, speed=750, loudness=-30.0, loudness_range=12.0, loudness_start=3.0, gain_db=-3.0, sample_rate=48000, dtype="float32")]
        both = push_sequence(eng, codes, kinds, pushes)
        for i, (P, S, L, lv, sink) in enumerate([(1260, 1250, (-160, 200, 0), (60, 500), (8000, "int16")), (891, 750, (-300, 120, 30), (-30, 0), (48000, "float32"))]):
            ref = chain(eng, plain[pushes][i], pitch=(P,), speed=(S,), loud=L, level=lv, sink=sink)
            for k in range(len(pushes)):
                assert both[i][k].dtype == ref[k].dtype and both[i][k].tobytes() == ref[k].tobytes(), (pushes, i, k)
            assert np.abs(np.concatenate(both[i]).astype(np.float64)).max() > 0
        whole.append(np.concatenate(both[0]))
    assert whole[0].tobytes() == whole[1].tobytes()
    # loudness with each neighbour alone: every hand-over into and out of the stage
    pushes = CUTS[0]
    for kw, ch in ((dict(speed=1250, loudness=-16.0), dict(speed=(1250,), loud=(-160, 200, 0))),
                   (dict(loudness=-16.0, gain_db=6.0, ceiling=0.5), dict(loud=(-160, 200, 0), level=(60, 500))),
                   (dict(loudness=0, sample_rate=16000, dtype="int16"), dict(loud=(0, 200, 0), sink=(16000, "int16"))),
                   (dict(pitch=1122, loudness=-16.0), dict(pitch=(1122,), loud=(-160, 200, 0)))):
        two = push_sequence(eng, codes, [kw, kw], pushes)
        for i in range(2):
            ref = chain(eng, plain[pushes][i], **ch)
            for k in range(len(pushes)):
                assert two[i][k].dtype == ref[k].dtype and two[i][k].tobytes() == ref[k].tobytes(), (kw, i, k)


def test_subsets_of_streams_push_in_different_cuts(eng, codes, plain):
    """stream 0 pushes 1 / 3 / 25 frames, stream 1 sits the second call out and takes 28 frames in the third: the calls' stages share
    launches, each stream's samples are its own chain's"""
    kw = dict(speed=1250, loudness=-16.0, gain_db=6.0, ceiling=0.5)
    a, b = eng.codec_stream_begin(NF, **kw), eng.codec_stream_begin(NF, **kw)
    o1 = eng.codec_stream_push_batch([a, b], [codes[0][:1], codes[1][:1]], finish=[False, False])
    o2 = eng.codec_stream_push_batch([a], [codes[0][1:4]], finish=[False])
    o3 = eng.codec_stream_push_batch([a, b], [codes[0][4:], codes[1][1:]], finish=[True, True])
    eng.codec_stream_end(a), eng.codec_stream_end(b)
    ch = dict(speed=(1250,), loud=(-160, 200, 0), level=(60, 500))
    ref_a = chain(eng, plain[CUTS[0]][0], **ch)
    whole_b = np.concatenate(plain[CUTS[0]][1])
    n1 = plain[CUTS[0]][1][0].size
    ref_b = chain(eng, [whole_b[:n1], whole_b[n1:]], **ch)
    for got, want in ((o1[0], ref_a[0]), (o2[0], ref_a[1]), (o3[0], ref_a[2]), (o1[1], ref_b[0]), (o3[1], ref_b[1])):
        assert got.tobytes() == want.tobytes()


def test_the_stage_on_a_stream(eng, codes, plain):
    pushes = CUTS[0]
    a, b = eng.codec_stream_begin(NF), eng.codec_stream_begin(NF, loudness=-16.0)
    assert a not in eng.__dict__.get("_codec_stream_loud", {}) and eng._codec_stream_loud[b] == (-160, 200, 0)
    out = eng.codec_stream_push(a, codes[0][:1])                                   # the float entry serves the stream without a stage
    assert np.asarray(out).tobytes() == plain[pushes][0][0].tobytes()
    with pytest.raises(RuntimeError, match="has a loudness"):                      # and refuses the stream that has one, by name
        eng.codec_stream_push(b, codes[1][:1])
    with pytest.raises(RuntimeError, match="already delivered"):
        eng.codec_stream_set_loudness(a, -160, 200, 0)
    for bad, word in (((-401, 200, 0), "-401"), ((-160, 401, 0), "401"), ((-160, 200, -401), "-401")):
        with pytest.raises(RuntimeError, match=word):
            eng.codec_stream_set_loudness(b, *bad)
    # finish is allowed on a stream with a loudness stage and no sink: a push of 0 frames flushes the tail
    c = eng.codec_stream_begin(NF, loudness=-16.0)
    head = eng.codec_stream_push_batch([c], [codes[0][:4]])[0]
    tail = eng.codec_stream_push_batch([c], [codes[0][:0]], finish=[True])[0]
    x = np.concatenate(plain[pushes][0][:2])                                       # frames 0 .. 3, whatever the cuts
    n1 = x.size
    assert head.size == q3tts.loudness_emitted(-160, n1) and head.size + tail.size == n1
    assert np.concatenate([head, tail]).tobytes() == R.stage(x, -160, 200, 0)[0].tobytes()
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([c], [codes[0][4:6]])
    for s in (a, b, c):
        eng.codec_stream_end(s)


@pytest.mark.parametrize("top_k", [1, 8])
def test_scheduler_with_a_loudness(eng, top_k):
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
    log1, pcm1, codes1, nf1 = run(loudness=-16.0)
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        got = np.concatenate([c[2] for c in calls])
        assert got.dtype == np.float32 and np.array_equal(got, pcm1[u])
        assert got.size == pcm0[u].size, u                                 # the calls add up to the length without the stage
        ref = chain(eng, [pcm0[u]], loud=(-160, 200, 0))[0]                # the same samples as the standalone stage
        assert got.tobytes() == ref.tobytes(), u
        assert got.tobytes() == R.stage(pcm0[u], -160, 200, 0)[0].tobytes(), u
    # with the stage taken away the run is the parent-style run again
    log2, pcm2, codes2, nf2 = run()
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u]) and pcm0[u].tobytes() == pcm2[u].tobytes()
    if top_k == 1:   # with the other four as well: pitch -> stretcher -> loudness -> level -> sink
        log3, pcm3, codes3, nf3 = run(pitch=794, speed=1250, loudness=(-20.0, 12.0, 3.0), gain_db=6.0, ceiling=0.5, sample_rate=8000, dtype="int16")
        for u in range(len(toks)):
            assert np.array_equal(codes0[u], codes3[u])
            ref = chain(eng, [pcm0[u]], pitch=(794,), speed=(1250,), loud=(-200, 120, 30), level=(60, 500), sink=(8000, "int16"))[0]
            assert pcm3[u].dtype == np.int16 and np.array_equal(pcm3[u], ref), u
