"""Vocoder streams and the streaming scheduler delivering through a level stage (q3tts_codec_stream_set_level,
q3tts_codec_stream_push_batch_any_host, q3tts_engine_set_level).  Reference: the standalone stages (tests/test_gpu_level.py,
tests/test_gpu_speed.py, tests/test_gpu_pcm_sink.py, each held against numpy) fed the 24 kHz PCM that the same sequence of calls
returns from streams without a stage.  The same calls give the same vocoder bits and every stage's output is a function of its input
alone, so every comparison is np.array_equal.  Tiny synthetic config; pushes of 1 / 3 / 25 and of 25 / 3 / 1 frames.  The gain is
chosen from the plain streams' peak so that the limiter has overs to work on (asserted on the numpy restatement)."""
import numpy as np
import pytest

import q3tts
from level_ref import level32
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

NF = 29
CEIL = 500


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=256)
    orc.close()
    yield e
    e.close()


def gain_for(peak):
    """centibels that bring `peak` to about three times the ceiling, inside the stage's range"""
    cb = int(np.clip(round(200.0 * np.log10(3.0 * CEIL / 1000.0 / max(float(peak), 1e-9))), -600, 400))
    return cb if cb != 0 else 10          # never the "no stage" pair


def push_sequence(eng, codes, kinds, pushes):
    """one stream per entry of kinds = dict of codec_stream_begin's keywords; the last push with finish where the stream has a stage
    -> per stream the list of pushes"""
    sids = [eng.codec_stream_begin(NF, **kw) for kw in kinds]
    staged = [kw.get("sample_rate", 24000) != 24000 or kw.get("dtype", "float32") != "float32" or kw.get("speed") not in (None, 1000)
              or q3tts.level_params(kw.get("gain_db"), kw.get("ceiling")) != (0, 0) for kw in kinds]
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


def chain(eng, pushes, speed=None, level=None, sink=None):
    """the standalone stages in the stream's order, push by push, the last with finish"""
    for begin, push, end, args in ((eng.speed_begin, eng.speed_push_batch, eng.speed_end, speed),
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
    for pushes in ((1, 3, 25), (25, 3, 1)):
        p = push_sequence(eng, codes, [{}, {}], pushes)
        assert sum(a.size for a in p[0]) == eng.codec_decode_len(NF)
        out[pushes] = p
    a, b = (np.concatenate(out[(1, 3, 25)][i]) for i in range(2))
    assert np.array_equal(a, np.concatenate(out[(25, 3, 1)][0]))          # the vocoder's own cut-invariance
    return out


@pytest.mark.parametrize("pushes", [(1, 3, 25), (25, 3, 1)])
def test_streams_with_a_level(eng, codes, plain, pushes):
    cbs = [gain_for(np.abs(np.concatenate(plain[pushes][i])).max()) for i in range(2)]
    kinds = [dict(gain_db=cbs[0] / 10.0, ceiling=CEIL / 1000.0), dict(gain_db=cbs[1] / 10.0)]      # a limiter and a gain-only stage
    got = push_sequence(eng, codes, kinds, pushes)
    whole = None
    for i, lv in enumerate([(cbs[0], CEIL), (cbs[1], 0)]):
        ref = chain(eng, plain[pushes][i], level=lv)
        n24 = 0
        for k in range(len(pushes)):
            before = q3tts.level_emitted(lv[0], lv[1], n24)
            n24 += plain[pushes][i][k].size
            assert got[i][k].size == q3tts.level_emitted(lv[0], lv[1], n24, k + 1 == len(pushes)) - before, (i, k)
            assert got[i][k].dtype == np.float32 and np.array_equal(got[i][k].view(np.uint32), ref[k].view(np.uint32)), (i, k)
        x = np.concatenate(plain[pushes][i])
        y, s = level32(x, lv[0], lv[1], want_s=True)
        assert np.array_equal(np.concatenate(got[i]).view(np.uint32), y.view(np.uint32)), i             # and the restatement itself
        if i == 0:
            whole = s
    assert np.count_nonzero(whole < 1.0) > 0                                                            # the limiter had work
    # (0, 0) is no stage: the bytes of a plain stream, beside a stream with a stage
    mixed = push_sequence(eng, codes, [dict(gain_db=0.0, ceiling=0.0), dict(gain_db=-3.0, ceiling=0.25)], pushes)
    for k in range(len(pushes)):
        assert np.array_equal(mixed[0][k].view(np.uint32), plain[pushes][0][k].view(np.uint32)), k


def test_streams_with_speed_level_and_sink(eng, codes, plain):
    pushes = (1, 3, 25)
    cbs = [gain_for(np.abs(np.concatenate(plain[pushes][i])).max()) for i in range(2)]
    kinds = [dict(sample_rate=8000, dtype="int16", speed=1250, gain_db=cbs[0] / 10.0, ceiling=CEIL / 1000.0),
             dict(sample_rate=48000, dtype="float32", speed=750, gain_db=cbs[1] / 10.0, ceiling=0.9)]
    both = push_sequence(eng, codes, kinds, pushes)
    for i, (sink, S, lv) in enumerate([((8000, "int16"), 1250, (cbs[0], CEIL)), ((48000, "float32"), 750, (cbs[1], 900))]):
        ref = chain(eng, plain[pushes][i], speed=(S,), level=lv, sink=sink)
        for k in range(len(pushes)):
            assert both[i][k].dtype == ref[k].dtype and np.array_equal(both[i][k], ref[k]), (i, k)
        assert np.abs(np.concatenate(both[i]).astype(np.float64)).max() > 0
    # level and sink without a stretcher
    one = push_sequence(eng, codes, [dict(sample_rate=16000, dtype="int16", gain_db=cbs[0] / 10.0, ceiling=CEIL / 1000.0), {}], pushes)
    ref = chain(eng, plain[pushes][0], level=(cbs[0], CEIL), sink=(16000, "int16"))
    for k in range(len(pushes)):
        assert np.array_equal(one[0][k], ref[k]), k
        assert np.array_equal(one[1][k], plain[pushes][1][k]), k


def test_every_subset_of_stages_in_one_push_sequence(eng, codes, plain):
    """Eight streams with the eight subsets of {stretcher, level stage, sink} share every call, so each launch set hands over along
    every pair of stages at once.  Ragged pushes (1 .. 8 frames, then 5 each: the second call's streams differ in left context);
    in the last call two streams finish without frames beside streams that bring frames.  The stream without a stage never
    finishes.  Reference: the same calls on eight plain streams, fed through the standalone stages."""
    subsets = [(s, l, k) for s in (False, True) for l in (False, True) for k in (False, True)]      # index 0: no stage
    cb = gain_for(max(np.abs(np.concatenate(plain[(1, 3, 25)][i])).max() for i in range(2)))
    args = [((1250,) if s else None, (cb, CEIL) if l else None, (8000, "int16") if k else None) for s, l, k in subsets]
    kinds = [dict(**(dict(speed=1250) if s else {}), **(dict(gain_db=cb / 10.0, ceiling=CEIL / 1000.0) if l else {}),
                  **(dict(sample_rate=8000, dtype="int16") if k else {})) for s, l, k in subsets]
    idle = (5, 7)                                            # stretcher + sink and all three: the tails alone, each pair handed over
    frames = [[i + 1 for i in range(8)], [5] * 8, [0 if i in idle else 3 for i in range(8)]]

    def run(kinds, staged):
        sids = [eng.codec_stream_begin(NF, **kw) for kw in kinds]
        parts, at = [[] for _ in kinds], [0] * len(kinds)
        for c, ns in enumerate(frames):
            fin = [c + 1 == len(frames) and s for s in staged]
            out = eng.codec_stream_push_batch(sids, [codes[i % 2][at[i]:at[i] + n] for i, n in enumerate(ns)], finish=fin if any(staged) else None)
            for i, o in enumerate(out):
                parts[i].append(o)
                at[i] += ns[i]
        for s in sids:
            eng.codec_stream_end(s)
        return parts
    base = run([{}] * 8, [False] * 8)
    got = run(kinds, [any(sub) for sub in subsets])
    for i, (speed, level, sink) in enumerate(args):
        assert sum(p.size for p in base[i]) == eng.codec_decode_len(sum(f[i] for f in frames)), i
        ref = chain(eng, base[i], speed=speed, level=level, sink=sink)
        for c in range(len(frames)):
            assert got[i][c].dtype == ref[c].dtype and got[i][c].size == ref[c].size, (i, c)
            assert got[i][c].tobytes() == ref[c].tobytes(), (i, c)
        assert np.abs(np.concatenate(got[i]).astype(np.float64)).max() > 0, i
        if any(subsets[i]) and i in idle:
            assert base[i][-1].size == 0 and got[i][-1].size > 0, i                      # the last call delivered the stages' tails alone


def test_refusals(eng, codes, plain):
    p0 = plain[(1, 3, 25)]
    a = eng.codec_stream_begin(NF, gain_db=6.0, ceiling=0.9)
    b = eng.codec_stream_begin(NF)
    with pytest.raises(RuntimeError, match="has a level"):   # the float entries refuse a stream with a level stage, by name
        eng._push_batch(np.array([a, b], np.int32), [codes[0][:1], codes[1][:1]], np.array([0, 1, 2], np.int32))
    with pytest.raises(RuntimeError, match="has a level"):
        eng.codec_stream_push(a, codes[0][:1])
    for cb, c, name in ((-601, 0, "-601"), (401, 0, "401"), (0, 1001, "1001")):
        with pytest.raises(RuntimeError, match=name):
            eng.codec_stream_set_level(b, cb, c)
    out = eng.codec_stream_push_batch([a, b], [codes[0][:1], codes[1][:1]])   # nothing above moved either stream
    assert out[0].size == q3tts.level_emitted(60, 900, p0[0][0].size) and np.array_equal(out[1], p0[1][0])
    for sid in (a, b):                                       # set_level after the first sample is refused
        with pytest.raises(RuntimeError, match="already delivered"):
            eng.codec_stream_set_level(sid, 30, 0)
    tail = eng.codec_stream_push_batch([a], [codes[0][:0]], finish=[True])[0]   # a push of 0 frames with finish flushes the tail
    assert out[0].size + tail.size == p0[0][0].size and tail.size == min(127, p0[0][0].size)
    assert np.array_equal(np.concatenate([out[0], tail]).view(np.uint32), level32(p0[0][0], 60, 900).view(np.uint32))
    with pytest.raises(RuntimeError, match="finished"):
        eng.codec_stream_push_batch([a], [codes[0][1:3]])
    eng.codec_stream_end(a)
    eng.codec_stream_end(b)


def test_scheduler_with_a_level(eng):
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
    cb = gain_for(max(np.abs(p).max() for p in pcm0))
    log1, pcm1, codes1, nf1 = run(gain_db=cb / 10.0, ceiling=CEIL / 1000.0)
    assert np.array_equal(nf0, nf1) and list(nf1) == caps
    work = 0
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                     # codes and frame counts untouched
        calls = log1[u]
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u   # finished = 1 last, exactly once
        got = np.concatenate([c[2] for c in calls])
        assert got.dtype == np.float32 and np.array_equal(got, pcm1[u])
        assert got.size == pcm0[u].size, u                                 # the calls add up to the plain length
        ref = chain(eng, [pcm0[u]], level=(cb, CEIL))[0]                   # the same samples as the stream entry / the standalone stage
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), u
        y, s = level32(pcm0[u], cb, CEIL, want_s=True)
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), u
        work += int(np.count_nonzero(s < 1.0))
    assert work > 0
    # with the level taken away the run is the parent-style run again
    log2, pcm2, codes2, nf2 = run()
    for u in range(len(toks)):
        assert len(log2[u]) == len(log0[u]) and np.array_equal(pcm0[u], pcm2[u])
    # with a stretcher and a sink as well: stretcher -> level -> sink
    log3, pcm3, codes3, nf3 = run(speed=1250, gain_db=cb / 10.0, ceiling=CEIL / 1000.0, sample_rate=8000, dtype="int16")
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes3[u])
        ref = chain(eng, [pcm0[u]], speed=(1250,), level=(cb, CEIL), sink=(8000, "int16"))[0]
        assert pcm3[u].dtype == np.int16 and np.array_equal(pcm3[u], ref), u
