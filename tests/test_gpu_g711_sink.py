"""G.711 out of the sinks (include/q3tts.h "G.711"): a sink of format "mulaw" / "alaw" delivers, byte for byte, the numpy
restatement (tests/g711_ref.py) of the law applied to the int16 that an int16 sink at the same rate, fed the same pushes, delivers.
No tolerance anywhere: the int16 is the same kernel's, the law is integer arithmetic.  The standalone sink, mixed formats in one
launch, vocoder streams and the scheduler; the tiny synthetic config of tests/test_gpu_codec_stream_sink.py."""
import numpy as np
import pytest

import g711_ref
import q3tts
from test_gpu_codec_stream_sink import PUSHES, push_sequence
from test_gpu_pcm_sink import N, cut_patterns, run, x  # noqa: F401  (x is a fixture: the signal with two full-scale runs)
from util import frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

LAWS = ["mulaw", "alaw"]
RATES = [8000, 11025, 48000]


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=256)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """each rate as int16 and under each law in one push + finish: computed once, shared, never modified"""
    return {(r, d): run(eng, x, r, d, [N], True) for r in RATES for d in ["int16"] + LAWS}


@pytest.mark.parametrize("law", LAWS)
def test_every_int16_through_the_format_only_path(eng, law):
    s = np.arange(-32767, 32768, dtype=np.int64)
    xs = ((s + 0.5 * np.sign(s)) / 32767.0).astype(np.float32)
    assert np.array_equal(g711_ref.s16_rule(xs), s.astype(np.int16))          # the int16 rule maps these to every s exactly
    sid = eng.pcm_sink_begin(24000, law)
    out = eng.pcm_sink_push_batch([sid], [xs], [True])[0]
    eng.pcm_sink_end(sid)
    assert out.dtype == np.uint8 and out.size == s.size
    assert np.array_equal(out, g711_ref.ENC[law](s))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("rate", RATES)
def test_resampled_bytes_are_the_law_of_the_int16_sink(eng, x, one_shot, rate, law):
    got, s = one_shot[(rate, law)], one_shot[(rate, "int16")]
    assert got.dtype == np.uint8 and got.size == s.size == q3tts.sink_emitted(rate, N, True)
    assert s.max() == 32767 and s.min() == -32767                             # the two full-scale runs reach the clip
    assert np.array_equal(got, g711_ref.ENC[law](s))
    for name, (ends, fin_last) in cut_patterns(rate).items():                 # run() holds every push's length to sink_emitted
        cut = run(eng, x, rate, law, ends, fin_last)
        assert cut.dtype == np.uint8 and np.array_equal(cut, got), (rate, law, name)


def test_four_formats_at_different_rates_in_one_call(eng, x, one_shot):
    keys = [(16000, "float32"), (11025, "int16"), (8000, "mulaw"), (48000, "alaw"), (24000, "mulaw")]
    alone = {k: one_shot[k] if k in one_shot else run(eng, x, k[0], k[1], [N], True) for k in keys}
    sids = [eng.pcm_sink_begin(r, d) for r, d in keys]
    ends = [1, 700, 701, 3333, N]
    parts, at = [[] for _ in keys], 0
    for k, b in enumerate(ends):
        outs = eng.pcm_sink_push_batch(sids, [x[at:b]] * len(keys), [k + 1 == len(ends)] * len(keys))
        for i, o in enumerate(outs):
            parts[i].append(o)
        at = b
    for i, key in enumerate(keys):
        got = np.concatenate(parts[i])
        assert got.dtype == alone[key].dtype and np.array_equal(got, alone[key]), key
        eng.pcm_sink_end(sids[i])
    assert np.array_equal(alone[(24000, "mulaw")], g711_ref.mu_enc(g711_ref.s16_rule(x)))


def test_unknown_format_is_still_refused_by_name(eng):
    import ctypes as C
    sid = C.c_int(-1)
    eng.L.q3tts_pcm_sink_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_int)]
    assert eng.L.q3tts_pcm_sink_begin(eng.h, 8000, 7, C.byref(sid)) == -1 and sid.value == -1
    msg = q3tts.lib().q3tts_last_error(eng.h).decode()
    assert "format 7 is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16" in msg and "Q3TTS_PCM_MULAW" in msg


@pytest.mark.parametrize("law", LAWS)
def test_vocoder_streams(eng, law):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    rng = np.random.default_rng(9)
    codes = [rng.integers(0, CB, (9, G)).astype(np.int64) for _ in range(2)]
    s16 = push_sequence(eng, codes, [(8000, "int16"), (24000, "int16")])
    g = push_sequence(eng, codes, [(8000, law), (24000, law)])
    for i in range(2):
        assert sum(p.size for p in g[i]) > 0
        for k in range(len(PUSHES)):
            assert g[i][k].dtype == np.uint8 and np.array_equal(g[i][k], g711_ref.ENC[law](s16[i][k])), (i, k)


@pytest.mark.parametrize("law", LAWS)
def test_scheduler(eng, law):
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=7)   # greedy
    toks = [frame_tokens([11, 22, 33]), frame_tokens([5, 6, 7, 8])]
    caps = [7, 5]

    def go(dtype):
        log = [[] for _ in toks]

        def on_audio(utt, fb, fe, pcm, fin):
            log[utt].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_stream(toks, sp, 3, on_audio, seed=5, ignore_eos=True, max_new_per_utt=caps, sample_rate=8000, dtype=dtype)
        return log, pcm, codes, nf
    log0, pcm0, codes0, nf0 = go("int16")
    log1, pcm1, codes1, nf1 = go(law)
    assert list(nf1) == caps and np.array_equal(nf0, nf1)
    for u in range(len(toks)):
        assert np.array_equal(codes0[u], codes1[u]), u                        # the codes are untouched
        assert [(c[0], c[1], c[3]) for c in log1[u]] == [(c[0], c[1], c[3]) for c in log0[u]], u
        for c0, c1 in zip(log0[u], log1[u]):
            assert c1[2].dtype == np.uint8 and np.array_equal(c1[2], g711_ref.ENC[law](c0[2])), u
        assert pcm1[u].dtype == np.uint8 and pcm1[u].size > 0 and np.array_equal(pcm1[u], g711_ref.ENC[law](pcm0[u])), u
