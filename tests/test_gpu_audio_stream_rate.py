"""Encoder streams at the source's own rate and sample format (q3tts_audio_stream_begin_rate): the codes and latents of a
stream begun at rate R (float or int16), however its samples are cut into pushes and whatever streams of whatever rates share its
calls, are bit-identical (np.array_equal, no tolerance anywhere) to Engine.audio_encode_batch([x], sample_rates=R) of the whole audio.

The tiny golden config of tests/test_gpu_audio_stream.py: 1920 samples per frame at 24 kHz, window 6; every clip gives 5 to 10 frames,
so the K/V ring wraps."""
import ctypes as C

import numpy as np
import pytest

import mimi_ref
import q3tts
from test_gpu_audio_stream import RAGGED, cuts_of, gold, make_tiny, tiny  # noqa: F401  (gold and tiny are fixtures)

pytestmark = pytest.mark.gpu

CLIPS = {8000: 6000, 16000: 6000, 44100: 20011, 48000: 20011, 96000: 40000}
E = q3tts.resample_stream_emitted


@pytest.fixture(scope="module")
def oneshot(tiny):
    """(codes, latents) of the one-shot encode at rate R per (n, seed, rate), computed once; int16 clips as v / 32768.0f"""
    memo = {}

    def get(n, seed, rate):
        if (n, seed, rate) not in memo:
            c, l = tiny.audio_encode_batch([mimi_ref.clip(n, seed)], sample_rates=rate, want_latents=True)
            memo[(n, seed, rate)] = (c[0], l[0])
        return memo[(n, seed, rate)]
    return get


def to_s16(x):
    return np.round(np.clip(x, -1, 1) * 32767.0).astype(np.int16)


def from_s16(v):
    return (v.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def run_stream(eng, x, rate, cuts, dtype="float32", max_samples=0, poison=False):
    """push x[a:b] for every cut, then finish; checks the frame count, push_len's prediction and audio_stream_info after every push"""
    sid = eng.audio_stream_begin_rate(rate, dtype, max_samples)
    assert eng.audio_stream_format(sid) == (rate, dtype)
    codes, lats, total = [], [], 0
    try:
        for a, b in list(cuts) + [(None, None)]:
            part = x[a:b] if a is not None else x[:0]
            fin = a is None
            want = eng.audio_stream_push_len(sid, part.size, fin)
            if poison:
                eng.poison_workspace()
            c, l = eng.audio_stream_push(sid, part, fin, want_latents=True)
            assert c.shape[0] == l.shape[0] == want, (a, b, c.shape, want)
            total += part.size
            codes.append(c)
            lats.append(l)
            ns, nf, finished, _ = eng.audio_stream_info(sid)
            assert ns == total and finished == fin and nf == sum(k.shape[0] for k in codes)
            if not fin:
                assert nf == E(rate, 24000, total, False) // 1920, (total, nf)
    finally:
        eng.audio_stream_end(sid)
    return np.concatenate(codes), np.concatenate(lats)


PATTERNS = {
    "one_push": lambda n: [(0, n)],
    "ragged": lambda n: cuts_of(n, RAGGED),
    "hundreds": lambda n: cuts_of(n, [100] * (n // 100 + 1)),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("rate", list(CLIPS))
def test_cut_patterns(tiny, oneshot, rate, pattern):
    n = CLIPS[rate]
    x = mimi_ref.clip(n, 5)
    rc, rl = oneshot(n, 5, rate)
    assert 5 <= rc.shape[0] <= 10
    c, l = run_stream(tiny, x, rate, PATTERNS[pattern](n))
    assert c.shape == rc.shape and l.shape == rl.shape
    assert np.array_equal(c, rc) and np.array_equal(l, rl)


def test_one_sample_pushes_at_8k(tiny, oneshot):
    n = 400                                              # 1200 samples at 24 kHz: the finish completes the one frame
    rc, rl = oneshot(n, 6, 8000)
    c, l = run_stream(tiny, mimi_ref.clip(n, 6), 8000, [(i, i + 1) for i in range(n)])
    assert rc.shape[0] == 1 and np.array_equal(c, rc) and np.array_equal(l, rl)


def test_pushes_shorter_than_the_carry_at_384k(tiny, oneshot):
    n = 3000                                             # 187 samples at 24 kHz; 5 < the 17-sample carry, and most pushes emit nothing
    rc, rl = oneshot(n, 7, 384000)
    emits = [E(384000, 24000, b, False) - E(384000, 24000, a, False) for a, b in cuts_of(n, [5] * 600)]
    assert emits.count(0) > len(emits) // 2
    c, l = run_stream(tiny, mimi_ref.clip(n, 7), 384000, cuts_of(n, [5] * 600))
    assert np.array_equal(c, rc) and np.array_equal(l, rl)


def test_stream_without_any_output(tiny):
    x = np.array([0.5, -0.25, 0.125], np.float32)        # 96 kHz: floor(3 * 0.25) = 0 samples at 24 kHz
    c, l = run_stream(tiny, x, 96000, [(0, 2), (2, 3)])
    assert c.shape[0] == 0 and l.shape[0] == 0
    with pytest.raises(RuntimeError, match="no sample left at 24 kHz"):          # the one-shot agrees: it has nothing to encode
        tiny.audio_encode_batch([x], sample_rates=96000)


@pytest.mark.parametrize("rate", [16000, 44100])
def test_int16_equals_float(tiny, rate):
    n = CLIPS[rate]
    v = to_s16(mimi_ref.clip(n, 8))
    xf = from_s16(v)
    rc, rl = tiny.audio_encode_batch([xf], sample_rates=rate, want_latents=True)
    cuts = cuts_of(n, RAGGED)
    cs, ls = run_stream(tiny, v, rate, cuts, dtype="int16")
    cf, lf = run_stream(tiny, xf, rate, cuts)
    assert np.array_equal(cs, cf) and np.array_equal(ls, lf)
    assert np.array_equal(cs, rc[0]) and np.array_equal(ls, rl[0])
    # int16 arrays for int16 streams, and only for them
    sid = tiny.audio_stream_begin_rate(rate)
    try:
        with pytest.raises(ValueError, match="expected float samples"):
            tiny.audio_stream_push(sid, v[:100])
    finally:
        tiny.audio_stream_end(sid)


def test_mixed_rates_and_formats_share_calls(tiny, oneshot):
    rates = [24000, 16000, 44100, 48000]
    dts = ["float32", "int16", "float32", "int16"]
    N = [5 * 1920 + 333, 6000, 20011, 20011]
    raw = [mimi_ref.clip(n, 40 + i) for i, n in enumerate(N)]
    xs = [to_s16(a) if d == "int16" else a for a, d in zip(raw, dts)]
    fl = [from_s16(a) if d == "int16" else a for a, d in zip(xs, dts)]
    # three rounds: stream 1 finishes in round 1 (early), stream 2 gets zero samples in round 1
    r0 = [(0, 3000), (0, 2501), (0, 7777), (0, 5)]
    r1 = [(3000, 7001), (2501, N[1]), (7777, 7777), (5, 12000)]
    r2 = [(7001, N[0]), None, (7777, N[2]), (12000, N[3])]
    fin = [[False] * 4, [False, True, False, False], [True, False, True, True]]
    sids = [tiny.audio_stream_begin_rate(r, d) for r, d in zip(rates, dts)]
    got_c, got_l = [[] for _ in N], [[] for _ in N]
    try:
        for rnd, cuts in enumerate((r0, r1, r2)):
            idx = [i for i in range(4) if cuts[i] is not None]
            before = tiny.audio_stream_info(sids[2])
            c, l = tiny.audio_stream_push_batch([sids[i] for i in idx], [xs[i][cuts[i][0]:cuts[i][1]] for i in idx], [fin[rnd][i] for i in idx],
                                                want_latents=True)
            for k, i in enumerate(idx):
                got_c[i].append(c[k])
                got_l[i].append(l[k])
            if rnd == 1:
                assert tiny.audio_stream_info(sids[2]) == before and got_c[2][-1].shape[0] == 0          # zero samples: unchanged
    finally:
        for s in sids:
            tiny.audio_stream_end(s)
    for i in range(4):
        c, l = np.concatenate(got_c[i]), np.concatenate(got_l[i])
        rc, rl = tiny.audio_encode_batch([fl[i]], sample_rates=rates[i], want_latents=True)
        assert np.array_equal(c, rc[0]) and np.array_equal(l, rl[0]), i
        cuts = [r[i] for r in (r0, r1, r2) if r[i] is not None]
        sc, sl = run_stream(tiny, xs[i], rates[i], cuts, dtype=dts[i])                              # the same cuts, alone
        assert np.array_equal(c, sc) and np.array_equal(l, sl), i
    # the 24 kHz member through the float-only entry of the parent commit
    sid = tiny.audio_stream_begin()
    try:
        parts = [_raw_push_float(tiny, sid, xs[0][a:b], False) for a, b in (r0[0], r1[0], r2[0])] + [_raw_push_float(tiny, sid, xs[0][:0], True)]
    finally:
        tiny.audio_stream_end(sid)
    assert np.array_equal(np.concatenate(parts), np.concatenate(got_c[0]))


def _raw_push_float(eng, sid, pcm, finish, cap=16):
    """q3tts_audio_stream_push_host, the float-only entry, without the binding"""
    a = np.ascontiguousarray(pcm, np.float32)
    out = np.zeros((cap, eng.cfg.n_groups), np.int64)
    nf = C.c_int32(0)
    eng._ck(eng.L.q3tts_audio_stream_push_host(eng.h, int(sid), a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, 1 if finish else 0,
                                               out.ctypes.data_as(C.c_void_p), cap, C.byref(nf)))
    return out[: nf.value]


def test_carry_lives_outside_the_workspace(tiny, oneshot):
    n = CLIPS[44100]
    rc, rl = oneshot(n, 5, 44100)
    c, l = run_stream(tiny, mimi_ref.clip(n, 5), 44100, cuts_of(n, RAGGED), poison=True)       # NaN bytes over the workspace before every push
    assert np.array_equal(c, rc) and np.array_equal(l, rl)


def test_validation_leaves_streams_unmoved(tiny, oneshot):
    n = CLIPS[16000]
    x = mimi_ref.clip(n, 5)
    rc, rl = oneshot(n, 5, 16000)
    v = to_s16(mimi_ref.clip(CLIPS[44100], 8))
    vc, vl = tiny.audio_encode_batch([from_s16(v)], sample_rates=44100, want_latents=True)
    for bad in (0, 384001, -5):
        with pytest.raises(RuntimeError, match="sample_rate must be 1..384000, got %d" % bad):
            tiny.audio_stream_begin_rate(bad)
    with pytest.raises(ValueError, match="dtype must be float32 or int16"):
        tiny.audio_stream_begin_rate(16000, "int32")
    sid = C.c_int(-1)
    assert tiny.L.q3tts_audio_stream_begin_rate(tiny.h, 16000, 7, 0, C.byref(sid)) == -1 and sid.value == -1
    assert "format must be Q3TTS_PCM_F32 (0) or Q3TTS_PCM_S16 (1), got 7" in q3tts.lib().q3tts_last_error(tiny.h).decode()
    with pytest.raises(RuntimeError, match="max_samples must be 0"):                 # one hour of the stream's own samples
        tiny.audio_stream_begin_rate(16000, max_samples=3600 * 16000 + 1)
    a = tiny.audio_stream_begin_rate(16000)
    b = tiny.audio_stream_begin_rate(48000, max_samples=5000)                 # 5000 of ITS samples, about 2500 at 24 kHz
    s = tiny.audio_stream_begin_rate(44100, "int16")
    try:
        c0, l0 = tiny.audio_stream_push(a, x[:2000], want_latents=True)
        s0, sl0 = tiny.audio_stream_push(s, v[:9000], want_latents=True)
        state = [tiny.audio_stream_info(k) for k in (a, b, s)]
        with pytest.raises(RuntimeError, match="takes int16 samples"):               # float samples to an int16 stream through the float entry
            _raw_push_float(tiny, s, np.zeros(100, np.float32), False)
        with pytest.raises(RuntimeError, match="over its max_samples: 0 \\+ 5001 samples"):
            tiny.audio_stream_push_batch([a, b], [x[2000:3000], np.zeros(5001, np.float32)])
        with pytest.raises(RuntimeError, match="push too long: 960001 samples, the cap per push is 960000"):
            tiny.audio_stream_push_batch([a, b], [np.zeros(960001, np.float32), np.zeros(10, np.float32)])
        with pytest.raises(RuntimeError, match="no open audio stream with id 977"):   # a bad second member of a mixed call
            tiny.audio_stream_push_batch([s, 977], [v[9000:9100], x[:10]])
        with pytest.raises(ValueError, match="expected int16 samples"):
            tiny.audio_stream_push_batch([a, s], [x[2000:3000], np.zeros(10, np.float32)])
        assert tiny.audio_stream_push_len(b, 5000, False) >= 0
        with pytest.raises(RuntimeError, match="outside the stream's limits"):
            tiny.audio_stream_push_len(b, 5001, False)
        assert [tiny.audio_stream_info(k) for k in (a, b, s)] == state
        c1, l1 = tiny.audio_stream_push(a, x[2000:], finish=True, want_latents=True)
        s1, sl1 = tiny.audio_stream_push(s, v[9000:], finish=True, want_latents=True)
    finally:
        for k in (a, b, s):
            tiny.audio_stream_end(k)
    assert np.array_equal(np.concatenate([c0, c1]), rc) and np.array_equal(np.concatenate([l0, l1]), rl)
    assert np.array_equal(np.concatenate([s0, s1]), vc[0]) and np.array_equal(np.concatenate([sl0, sl1]), vl[0])


def test_reuse_at_another_rate_carries_nothing_over(tiny, oneshot):
    y = mimi_ref.clip(CLIPS[48000], 5)
    sid = tiny.audio_stream_begin_rate(48000, "int16")
    tiny.audio_stream_push(sid, to_s16(y[:15000]))         # left unfinished: rings and carry full
    tiny.audio_stream_end(sid)
    n = CLIPS[16000]
    rc, rl = oneshot(n, 5, 16000)
    again = tiny.audio_stream_begin_rate(16000)
    assert again == sid and tiny.audio_stream_format(again) == (16000, "float32") and tiny.audio_stream_info(again)[:3] == (0, 0, False)
    tiny.audio_stream_end(again)
    c, l = run_stream(tiny, mimi_ref.clip(n, 5), 16000, cuts_of(n, [2500] * 3))
    assert np.array_equal(c, rc) and np.array_equal(l, rl)
    with q3tts.AudioEncodeStream(tiny, n, sample_rate=16000) as st:
        assert st.sid == sid
        st.push(mimi_ref.clip(n, 5)[:777])
        st.push(mimi_ref.clip(n, 5)[777:])
        st.finish()
        assert np.array_equal(st.codes, rc)
    assert np.array_equal(tiny.audio_encode_long_rate(mimi_ref.clip(n, 5), 16000, chunk_samples=1000), rc)
