"""G.711 into the encoder streams (include/q3tts.h "G.711"): a stream begun with dtype "mulaw" / "alaw" takes bytes and
gives, bit for bit (np.array_equal on codes and latents, no tolerance), what an int16 stream at the same rate gives for the numpy
restatement's decode (tests/g711_ref.py) of those bytes under the same cuts — and the same under every cut pattern.  The tiny golden
config of tests/test_gpu_audio_stream.py: 1920 samples per frame at 24 kHz; both clips give 5 frames."""
import ctypes as C

import numpy as np
import pytest

import g711_ref
import mimi_ref
import q3tts
from test_gpu_audio_stream import RAGGED, cuts_of, gold, tiny  # noqa: F401  (gold and tiny are fixtures)
from test_gpu_audio_stream_rate import _raw_push_float, from_s16, run_stream, to_s16

pytestmark = pytest.mark.gpu

LAWS = ["mulaw", "alaw"]
CLIPS = {8000: 3000, 24000: 9000}          # 24 kHz G.711 goes through the resampling kernel like 24 kHz int16
PATTERNS = {
    "one_push": lambda n: [(0, n)],
    "single_samples_first": lambda n: [(i, i + 1) for i in range(40)] + [(40, n)],
    "ragged": lambda n: cuts_of(n, RAGGED),
}


def byte_clip(n, seed):
    """every byte value, then seeded random bytes"""
    b = np.concatenate([np.tile(np.arange(256, dtype=np.uint8), 2), np.random.default_rng(seed).integers(0, 256, n - 512).astype(np.uint8)])
    assert b.size == n and np.unique(b).size == 256
    return b


@pytest.fixture(scope="module")
def as_int16(tiny):
    """(codes, latents) of the int16 stream fed dec(bytes) in one push, per (rate, law): computed once, shared, never modified"""
    out = {}
    for rate, n in CLIPS.items():
        for law in LAWS:
            out[(rate, law)] = run_stream(tiny, g711_ref.DEC[law](byte_clip(n, rate)), rate, [(0, n)], dtype="int16")
    return out


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("rate", list(CLIPS))
def test_bytes_equal_the_int16_stream_of_their_decode(tiny, as_int16, rate, law, pattern):
    n = CLIPS[rate]
    b = byte_clip(n, rate)
    cuts = PATTERNS[pattern](n)
    rc, rl = as_int16[(rate, law)]
    assert rc.shape[0] == 5
    sc, sl = run_stream(tiny, g711_ref.DEC[law](b), rate, cuts, dtype="int16")     # the same cuts through the int16 stream
    gc, gl = run_stream(tiny, b, rate, cuts, dtype=law)
    assert gc.shape == rc.shape and gl.shape == rl.shape
    assert np.array_equal(gc, sc) and np.array_equal(gl, sl)
    assert np.array_equal(gc, rc) and np.array_equal(gl, rl)                      # and the one-push result, whatever the cuts


def test_four_formats_share_calls(tiny):
    rates = [16000, 44100, 8000, 24000]
    dts = ["float32", "int16", "mulaw", "alaw"]
    N = [6000, 20011, 3000, 9000]
    xs = [mimi_ref.clip(N[0], 40), to_s16(mimi_ref.clip(N[1], 41)), byte_clip(N[2], 42), byte_clip(N[3], 43)]
    # three rounds: the mu-law stream finishes in round 1 (early), the A-law stream gets zero samples in round 1
    r0 = [(0, 3000), (0, 7777), (0, 1501), (0, 5)]
    r1 = [(3000, 3001), (7777, 12000), (1501, N[2]), (5, 5)]
    r2 = [(3001, N[0]), (12000, N[1]), None, (5, N[3])]
    fin = [[False] * 4, [False, False, True, False], [True, True, False, True]]
    sids = [tiny.audio_stream_begin_rate(r, d) for r, d in zip(rates, dts)]
    got_c, got_l = [[] for _ in N], [[] for _ in N]
    try:
        for i, sid in enumerate(sids):
            assert tiny.audio_stream_format(sid) == (rates[i], dts[i])
        for rnd, cuts in enumerate((r0, r1, r2)):
            idx = [i for i in range(4) if cuts[i] is not None]
            c, l = tiny.audio_stream_push_batch([sids[i] for i in idx], [xs[i][cuts[i][0]:cuts[i][1]] for i in idx], [fin[rnd][i] for i in idx],
                                                want_latents=True)
            for k, i in enumerate(idx):
                got_c[i].append(c[k])
                got_l[i].append(l[k])
    finally:
        for s in sids:
            tiny.audio_stream_end(s)
    for i in range(4):
        cuts = [r[i] for r in (r0, r1, r2) if r[i] is not None]
        sc, sl = run_stream(tiny, xs[i], rates[i], cuts, dtype=dts[i])            # the same cuts, alone
        c, l = np.concatenate(got_c[i]), np.concatenate(got_l[i])
        assert c.shape[0] >= 4 and np.array_equal(c, sc) and np.array_equal(l, sl), i
    for i, law in ((2, "mulaw"), (3, "alaw")):                                    # and the one-shot encode of the decoded bytes
        rc, rl = tiny.audio_encode_batch([from_s16(g711_ref.DEC[law](xs[i]))], sample_rates=rates[i], want_latents=True)
        assert np.array_equal(np.concatenate(got_c[i]), rc[0]) and np.array_equal(np.concatenate(got_l[i]), rl[0]), i


def test_refusals_move_nothing(tiny, as_int16):
    b = byte_clip(CLIPS[8000], 8000)
    sid = C.c_int(-1)
    assert tiny.L.q3tts_audio_stream_begin_rate(tiny.h, 8000, 7, 0, C.byref(sid)) == -1 and sid.value == -1
    msg = q3tts.lib().q3tts_last_error(tiny.h).decode()
    assert "format must be Q3TTS_PCM_F32 (0) or Q3TTS_PCM_S16 (1), got 7" in msg and "Q3TTS_PCM_MULAW (2)" in msg
    mu, al = tiny.audio_stream_begin_rate(8000, "mulaw"), tiny.audio_stream_begin_rate(8000, "alaw")
    try:
        assert tiny.audio_stream_format(mu) == (8000, "mulaw") and tiny.audio_stream_format(al) == (8000, "alaw")
        c0, l0 = tiny.audio_stream_push(mu, b[:1000], want_latents=True)
        state = [tiny.audio_stream_info(k) for k in (mu, al)]
        with pytest.raises(RuntimeError, match="mu-law"):                          # the float entry refuses a G.711 stream by name
            _raw_push_float(tiny, mu, np.zeros(100, np.float32), False)
        with pytest.raises(RuntimeError, match="A-law"):
            _raw_push_float(tiny, al, np.zeros(100, np.float32), False)
        with pytest.raises(ValueError, match="expected uint8 samples"):           # bytes for G.711 streams, and only bytes
            tiny.audio_stream_push(mu, np.zeros(10, np.int16))
        with pytest.raises(ValueError, match="expected uint8 samples"):
            tiny.audio_stream_push(al, np.zeros(10, np.float32))
        assert [tiny.audio_stream_info(k) for k in (mu, al)] == state
        c1, l1 = tiny.audio_stream_push(mu, b[1000:], finish=True, want_latents=True)
    finally:
        tiny.audio_stream_end(mu)
        tiny.audio_stream_end(al)
    rc, rl = as_int16[(8000, "mulaw")]
    assert np.array_equal(np.concatenate([c0, c1]), rc) and np.array_equal(np.concatenate([l0, l1]), rl)
    with q3tts.AudioEncodeStream(tiny, b.size, sample_rate=8000, dtype="ulaw") as st:    # the context manager, and the other name
        st.push(b[:777])
        st.push(b[777:])
        st.finish()
        assert np.array_equal(st.codes, rc)
    f = tiny.audio_stream_begin_rate(8000)
    try:
        with pytest.raises(ValueError, match="expected float samples"):           # and no bytes for a float stream
            tiny.audio_stream_push(f, b[:100])
    finally:
        tiny.audio_stream_end(f)
