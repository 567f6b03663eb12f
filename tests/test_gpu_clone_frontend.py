"""The voice-clone front end on the GPU for audio already in memory: q3tts_resample_gpu_host, q3tts_mel_gpu_host and
q3tts_speaker_embed_pcm_batch_host (Engine.resample_gpu / log_mel_gpu / speaker_embeddings).

What is compared with what, and why the bound is what it is:
  resample      bit-exact against q3tts.resample (itself pinned bit-exact to the compiled reference): the same IEEE operations.
  log-mel       the reference's own recorded answers with the tolerance of tests/test_audio_frontend.py, unchanged.
  encoder       the oracle fed the GPU's own mel, with test_gpu_clone.close() (1e-4 of the embedding's max magnitude), unchanged.
  batching      bit-exact: a clip alone == its row in any batch, in any order, under any split into workspace groups.
  end to end    against the host front end (the file-path entry point); bound in test_end_to_end_against_host_front_end."""
import ctypes as C

import numpy as np
import pytest

import q3_oracle as qo
from test_audio_frontend import signals
from test_gpu_clone import close, voice, write_wav16
from util import frame_tokens, tiny_pair, to_osampling

pytestmark = pytest.mark.gpu
RESAMPLE_PAIRS = [(16000, 24000), (44100, 24000), (48000, 24000), (8000, 24000), (22050, 24000), (24000, 24000), (24000, 16000), (11025, 48000)]
# the four clips of the isolated-encoder test: (seconds, rate, seed of test_gpu_clone.voice)
STAGE_CLIPS = [(1.3, 16000, 10), (3.0, 16000, 11), (1.3, 24000, 12), (3.0, 24000, 13)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frames_of(n, rate):
    n24 = n if rate == 24000 else int(float(n) * (24000.0 / rate))
    return 0 if n24 == 0 else (1 if n24 < 1024 else (n24 - 1024) // 256 + 1)


@pytest.fixture(scope="module")
def tiny():
    import q3tts
    eng, orc, _ = tiny_pair(seed=8, max_batch=2, max_ctx=96, flags=q3tts.FLAG_TEST_HOOKS)
    yield eng, orc
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def full():
    """0.6B speaker dims, the weight recipe of test_gpu_clone.test_full_size_speaker_encoder_vs_oracle"""
    import q3tts
    cfg = q3tts.default_config("0.6b")
    ocfg = qo.Config.from_dict(cfg.to_dict())
    eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=64)
    eng.fill_synthetic(seed=0)
    rng = np.random.default_rng(5)
    orc = qo.Oracle(ocfg, max_ctx=8)
    for name, shape, kind in qo.tensor_specs(ocfg):
        if not name.startswith("spk."):
            continue
        fan = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        a = qo.bf16_round(rng.standard_normal(shape).astype(np.float32) * (1.0 / np.sqrt(fan) if kind == "w" else 0.1))
        eng.set_tensor(name, a)
        orc.set_tensor(name, a)
    eng.finalize()
    yield eng, orc
    eng.close()
    orc.close()


@pytest.mark.parametrize("src,dst", RESAMPLE_PAIRS)
def test_resample_gpu_is_bit_exact(tiny, src, dst):
    import q3tts
    eng, _ = tiny
    rng = np.random.default_rng(src + dst)   # the inputs of test_audio_frontend.test_resample_matches_reference
    for n in (1, 2, 3, 1000, 12345):
        a = rng.standard_normal(n).astype(np.float32)
        want = q3tts.resample(a, src, dst)
        got = eng.resample_gpu(a, src, dst)
        assert got.size == want.size, (n, src, dst, got.size, want.size)
        assert np.array_equal(bits(got), bits(want)), (n, src, dst, int((bits(got) != bits(want)).sum()))


def test_log_mel_gpu_matches_reference_answers(tiny):
    """The nine signals and the tolerance of test_audio_frontend.test_log_mel_matches_reference:
    |E - E_ref| <= 1e-4 E_ref + 1e-6 sqrt(E_ref E_max) + 1e-10 on E = exp(logmel) - 1e-10, |d log| < 1e-3 where E_ref > 1e-6 E_max."""
    import build_ref
    import q3tts
    from ref_io import RefIO
    eng, _ = tiny
    ref = RefIO(build_ref.build())   # live where the reference can be compiled, else its recorded answers (never re-recorded from here)
    for name, a in signals():
        cap = 128 * (a.size // 256 + 2)
        out = np.zeros(cap, np.float32)
        k = ref.ref_mel(a.ctypes.data, a.size, out.ctypes.data, cap)
        frames = k // 128
        want = out[:k].reshape(128, frames)
        got = eng.log_mel_gpu(a)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        e_w = np.exp(want.astype(np.float64)) - 1e-10
        e_g = np.exp(got.astype(np.float64)) - 1e-10
        emax = e_w.max(axis=0, keepdims=True)
        tol = 1e-4 * np.abs(e_w) + 1e-6 * np.sqrt(np.abs(e_w) * emax) + 1e-10
        err = np.abs(e_g - e_w)
        strong = e_w > 1e-6 * emax
        dlog = float(np.abs(got - want)[strong].max()) if strong.any() else 0.0
        host = q3tts.log_mel(a)
        print("log_mel_gpu %-16s frames %3d  worst err/tol %.3g  max |dlog| on strong bands %.3g  bits differing from the host mel %d / %d"
              % (name, frames, float((err / tol).max()), dlog, int((bits(got) != bits(host)).sum()), got.size))
        assert not (err > tol).any(), (name, int((err > tol).sum()), float(err.max()))
        assert dlog < 1e-3, name
    # the fused entry point is the two stages
    a16 = voice(0.7, 16000, 4)
    assert np.array_equal(bits(eng.log_mel_gpu(a16, 16000)), bits(eng.log_mel_gpu(q3tts.resample(a16, 16000, 24000), 24000)))
    assert np.array_equal(bits(eng.log_mel_gpu(a16, 16000)), bits(eng.log_mel_gpu(eng.resample_gpu(a16, 16000, 24000))))
    # the empty clip, as q3tts_mel_host / q3tts.log_mel
    assert eng.log_mel_gpu(np.zeros(0, np.float32)).shape == (128, 0)
    fr = C.c_int32(7)
    assert eng.L.q3tts_mel_gpu_host(eng.h, None, 0, 24000, None, 0, C.byref(fr)) == -1 and fr.value == 0


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_encoder_stage_vs_oracle_on_the_gpu_mel(tiny, full, which):
    eng, orc = tiny if which == "tiny" else full
    for sec, rate, seed in STAGE_CLIPS:
        clip = voice(sec, rate, seed)
        mel = eng.log_mel_gpu(clip, rate)
        assert mel.shape == (128, frames_of(clip.size, rate))
        # the clip's noise floor keeps every band that has a triangle far above the 1e-10 floor (the lowest bands of this filterbank are
        # empty: their corners snap to one FFT bin, and they read log(1e-10) on every input)
        assert float(np.exp(mel[mel > -20.0]).min()) > 1e-8 and (mel <= -20.0).all(axis=1).sum() == (mel <= -20.0).any(axis=1).sum()
        got = eng.speaker_embeddings([clip], rate)[0]
        want = orc.speaker_encoder(mel)
        print("encoder stage %s %.1fs @%d: max dev %.3g of max |embed| %.3g" % (which, sec, rate, float(np.abs(got - want).max()), float(np.abs(want).max())))
        assert got.shape == want.shape and close(got, want), (which, sec, rate, float(np.abs(got - want).max()), float(np.abs(want).max()))


def ragged_clips():
    """9 clips from exactly 5 mel frames to about 5 s at mixed rates"""
    spec = [(2048, 24000), (1366, 16000), (int(0.4 * 44100), 44100), (int(1.1 * 22050), 22050), (int(2.0 * 16000), 16000),
            (int(2.7 * 24000), 24000), (int(3.3 * 44100), 44100), (int(4.1 * 22050), 22050), (int(5.0 * 16000), 16000)]
    clips, rates = [], []
    for i, (n, rate) in enumerate(spec):
        clips.append(voice(n / rate + 0.01, rate, 20 + i)[:n])
        assert clips[-1].size == n
        rates.append(rate)
    assert frames_of(*spec[0]) == 5 and frames_of(*spec[1]) == 5 and frames_of(1365, 16000) == 4
    assert len({frames_of(n, r) for n, r in spec[1:]}) == 8 and max(frames_of(n, r) for n, r in spec) > 460
    return clips, rates


def test_batch_invariance_bit_for_bit(tiny, monkeypatch):
    eng, _ = tiny
    clips, rates = ragged_clips()
    monkeypatch.delenv("Q3TTS_SPK_WS_MAX_BYTES", raising=False)
    batch = eng.speaker_embeddings(clips, rates)
    assert batch.shape == (9, eng.cfg.spk_enc_dim) and np.isfinite(batch).all()
    assert len({batch[i].tobytes() for i in range(9)}) == 9
    for i in range(9):
        alone = eng.speaker_embeddings([clips[i]], rates[i])[0]
        assert np.array_equal(bits(alone), bits(batch[i])), ("alone", i, float(np.abs(alone - batch[i]).max()))
    rev = eng.speaker_embeddings(clips[::-1], rates[::-1])[::-1]
    assert np.array_equal(bits(rev), bits(batch)), ("reversed", np.flatnonzero((bits(rev) != bits(batch)).any(axis=1)).tolist())
    sub = eng.speaker_embeddings([clips[7], clips[0], clips[4]], [rates[7], rates[0], rates[4]])
    assert np.array_equal(bits(sub), bits(batch[[7, 0, 4]]))
    # forced into workspace groups: every clip alone (1 byte), and bounds that cut the batch in other places
    for bound in (1, 1 << 19, 1 << 21, 1 << 22, 1 << 23):
        monkeypatch.setenv("Q3TTS_SPK_WS_MAX_BYTES", str(bound))
        grouped = eng.speaker_embeddings(clips, rates)
        assert np.array_equal(bits(grouped), bits(batch)), ("groups", bound, np.flatnonzero((bits(grouped) != bits(batch)).any(axis=1)).tolist())
    monkeypatch.delenv("Q3TTS_SPK_WS_MAX_BYTES")
    assert np.array_equal(bits(eng.speaker_embeddings(clips, rates)), bits(batch))


def test_batch_invariance_full_size(full):
    eng, _ = full
    clips = [voice(sec, rate, seed) for sec, rate, seed in STAGE_CLIPS] + [voice(0.2, 44100, 3)]
    rates = [r for _, r, _ in STAGE_CLIPS] + [44100]
    batch = eng.speaker_embeddings(clips, rates)
    for i in range(len(clips)):
        assert np.array_equal(bits(eng.speaker_embeddings([clips[i]], rates[i])[0]), bits(batch[i])), i
    assert np.array_equal(bits(eng.speaker_embeddings(clips[::-1], rates[::-1])[::-1]), bits(batch))


# relative deviation (of the embedding's max magnitude) between the GPU front end and the host front end, as measured on an MI355X for
# the five clips below at tiny and full-size dims (the values are in the docstring of the test); the assertion is 10x the largest
E2E_MEASURED_MAX = 6.23e-7
E2E_BOUND = 10 * E2E_MEASURED_MAX


def test_end_to_end_against_host_front_end(tiny, full, tmp_path):
    """speaker_embeddings on in-memory audio against the unchanged host front end (read_wav -> resample -> log_mel on the CPU ->
    speaker_encoder; for the file, extract_speaker_embedding itself).  The GPU FFT runs the host's butterflies in the host's order, so
    the two mels differ only by the rounding of logf (see the "bits differing" figures the log-mel test prints) and the encoder's
    batched kernels are bit-identical to the single-clip ones; what is left is pushed through the encoder.

    Measured on an MI355X, max |gpu - host| / max |host| per clip (stereo file, then STAGE_CLIPS in order):
        tiny dims       2.28e-07, 3.35e-07, 1.81e-07, 1.31e-07, 1.26e-07
        full-size dims  6.18e-07, 5.27e-07, 4.97e-07, 6.23e-07, 4.92e-07
    (see E2E_MEASURED_MAX; the assertion is 10x the largest, the margin covers other clips' spectra: both sides are deterministic).
    Then clone synthesis with the batch's embedding rows equals the oracle's given the same rows."""
    import q3tts
    wav = str(tmp_path / "ref.wav")
    write_wav16(wav, np.stack([voice(1.3, 16000, 0), voice(1.3, 16000, 1)], 1).reshape(-1), 16000, channels=2)
    audio, sr = q3tts.read_wav(wav)
    assert sr == 16000 and audio.size == int(1.3 * 16000)
    worst = 0.0
    for which, (eng, orc) in (("tiny", tiny), ("full", full)):
        devs = []
        host = eng.extract_speaker_embedding(wav)
        got = eng.speaker_embeddings([audio], 16000)[0]
        devs.append(float(np.abs(got - host).max()) / float(np.abs(host).max()))
        for sec, rate, seed in STAGE_CLIPS:
            clip = voice(sec, rate, seed)
            host = eng.speaker_encoder(q3tts.log_mel(q3tts.resample(clip, rate, 24000)))
            got = eng.speaker_embeddings([clip], rate)[0]
            devs.append(float(np.abs(got - host).max()) / float(np.abs(host).max()))
        print("end to end %s dims: max |gpu - host| / max |host| per clip: %s" % (which, ", ".join("%.3g" % d for d in devs)))
        worst = max(worst, max(devs))
    print("end to end: largest %.3g, bound %.3g" % (worst, E2E_BOUND))
    assert worst <= E2E_BOUND, (worst, E2E_BOUND)

    # clone synthesis with rows of a batched call: codes equal the oracle's on the same (bf16-rounded) rows
    eng, orc = tiny
    rows = eng.speaker_embeddings([audio, voice(1.3, 24000, 12)], [16000, 24000])
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=10)   # greedy
    toks = [frame_tokens([11, 22, 33, 44]), frame_tokens([5, 6, 7])]
    spk = [qo.bf16_round(rows[0]), qo.bf16_round(rows[1])]
    pcm, codes, nfr = eng.synthesize_batch(toks, sp, lang=2, seed=4, ignore_eos=True, speakers=spk)
    for u, t in enumerate(toks):
        ref = orc.generate(orc.build_prompt(t, 2, speaker=spk[u]), to_osampling(sp), seed=4, stream=u, cp_cached=True, ignore_eos=True)
        assert nfr[u] == 10 and np.array_equal(codes[u], ref), u


def test_errors_name_the_clip_and_leave_the_engine_usable(tiny):
    import q3tts
    eng, _ = tiny
    good = voice(0.5, 16000, 1)
    before = eng.speaker_embeddings([good, good[:4000]], 16000)
    cases = [
        ([], [], "n_clips must be at least 1"),
        ([good, None], 16000, "clip 1: NULL audio pointer"),
        ([good, good, np.zeros(0, np.float32)], 16000, "clip 2: n_samples must be at least 1"),
        ([good, good], [16000, 0], "clip 1: sample_rate must be at least 1"),
        ([good, good], [16000, -5], "clip 1: sample_rate must be at least 1"),
        ([good, good[:1365]], 16000, "clip 1: speaker encoder needs at least 5 mel frames"),
        ([good[:3], good], 48000, "clip 0: speaker encoder needs at least 5 mel frames"),   # resamples to one sample
        ([np.zeros(16385 * 256 + 1024, np.float32), good], 24000, "clip 0: reference clip too long for the speaker encoder \\(more than 16384 mel frames\\)"),
    ]
    for clips, rates, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            eng.speaker_embeddings(clips, rates)
        after = eng.speaker_embeddings([good, good[:4000]], 16000)
        assert np.array_equal(bits(after), bits(before)), msg
    # no partial output: a refused call leaves the caller's buffer as it was
    out = np.full((2, eng.cfg.spk_enc_dim), 7.0, np.float32)
    ptrs = (C.c_void_p * 2)(good.ctypes.data, good.ctypes.data)
    ns, rt = np.array([good.size, 100], np.int64), np.array([16000, 16000], np.int32)
    assert eng.L.q3tts_speaker_embed_pcm_batch_host(eng.h, 2, ptrs, ns.ctypes.data, rt.ctypes.data, out.ctypes.data) == -1
    assert (out == 7.0).all() and b"clip 1" in eng.L.q3tts_last_error(eng.h)

    cfg = q3tts.Config.from_dict(dict(eng.cfg.to_dict(), spk_enc_dim=0))
    bare = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=64)
    bare.fill_synthetic(seed=0)
    assert not bare.has_speaker_encoder
    with pytest.raises(RuntimeError, match="model has no speaker encoder"):
        bare.speaker_embeddings([good], 16000)
    assert bare.log_mel_gpu(good, 16000).shape == (128, frames_of(good.size, 16000))   # the stage entry points need no encoder
    bare.close()
    raw = q3tts.Engine(eng.cfg, device=0, max_batch=1, max_ctx=64)
    with pytest.raises(RuntimeError, match="weights not finalized"):
        raw.speaker_embeddings([good], 16000)
    raw.close()
