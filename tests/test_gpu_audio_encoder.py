"""Audio encoder on the GPU (12 Hz tokenizer, audio -> codes) against the fp64 restatement tests/mimi_ref.py, which
tests/test_cpu_audio_encoder.py ties to the transformers golden tests/golden/hf_mimi_encoder.npz.

Bounds (from the golden, not from the code under test): latents within 10 x the fp32-against-fp64 error transformers itself shows on
these clips (hf_fp32_err); a code mismatch passes only where the checker's relative top-2 gap is under 10 x the measured relative
distance perturbation (dist_rel_err), excuses the rest of that frame only, and excused frames stay <= 10 % of the clip's frames."""
import json
import os

import numpy as np
import pytest

import mimi_ref
import q3_oracle as qo
import q3tts
from util import calibrate_codec, frame_tokens

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hf_mimi_encoder.npz")
LENGTHS = [1, 1919, 1920, 1921, 5 * 1920 + 777, 39177]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    w = {k[6:]: z[k] for k in z.files if k.startswith("w:enc.")}
    return w, json.loads(str(z["cfg"])), 10.0 * float(z["hf_fp32_err"]), 10.0 * float(z["dist_rel_err"])


@pytest.fixture(scope="module")
def tiny(gold):
    w_enc, cfg, _, _ = gold
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)
    w.update({"enc." + k: v for k, v in w_enc.items()})
    eng = q3tts.Engine(q3tts.Config.from_dict(dict(ocfg.to_dict(), **cfg)), device=0, max_batch=2, max_ctx=192, flags=q3tts.FLAG_TEST_HOOKS)
    eng.load(w)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ref(gold):
    """the restatement's (latents, codes, gaps) per probe length, computed once"""
    w, cfg, _, _ = gold
    return {n: mimi_ref.encode(w, cfg, mimi_ref.clip(n, seed)) for seed, n in enumerate(LENGTHS)}


def test_symbols_and_len(tiny):
    assert tiny.has_audio_encoder
    for n, f in ((1, 1), (1919, 1), (1920, 1), (1921, 2), (39177, 21)):
        assert tiny.audio_encode_len(n) == f


@pytest.mark.parametrize("idx", range(len(LENGTHS)))
def test_latents_and_codes_against_ref(tiny, gold, ref, idx):
    _, _, bound, gate = gold
    n = LENGTHS[idx]
    codes, lat = tiny.audio_encode(mimi_ref.clip(n, idx), want_latents=True)
    rlat, rcodes, gaps = ref[n]
    assert lat.shape == rlat.shape and codes.shape == rcodes.shape
    err = float(np.abs(lat.astype(np.float64) - rlat).max())
    print("n=%d: latents max err %.3e (bound %.3e), |latents| max %.2f" % (n, err, bound, float(np.abs(rlat).max())))
    assert err <= bound
    excused = mimi_ref.check_codes(codes, rcodes, gaps, gate)
    print("n=%d: %d of %d frames excused" % (n, len(excused), rcodes.shape[0]))
    assert np.array_equal(tiny.audio_encode(mimi_ref.clip(n, idx)), codes)    # the codes-only entry, and run-to-run identity


def test_causality(tiny, gold):
    _, _, bound, _ = gold
    x = mimi_ref.clip(39177, 5)
    _, whole = tiny.audio_encode(x, want_latents=True)
    for N in (1, 7, 20):
        _, part = tiny.audio_encode(x[: N * 1920], want_latents=True)
        assert part.shape[0] == N
        err = float(np.abs(part - whole[:N]).max())
        print("first %d frames: max diff %.3e" % (N, err))
        assert err <= bound


def test_ragged_batch_bit_identical(tiny):
    # 1, 3, 21, 2 and 8 frames; the 2-frame clip at 16 kHz (2560 samples -> 3840 at 24 kHz through the GPU resampler)
    clips = [mimi_ref.clip(1000, 10), mimi_ref.clip(3 * 1920 - 5, 11), mimi_ref.clip(39177, 12), mimi_ref.clip(2560, 13), mimi_ref.clip(8 * 1920, 14)]
    rates = [24000, 24000, 24000, 16000, 24000]
    codes, lats = tiny.audio_encode_batch(clips, rates, want_latents=True)
    assert [c.shape[0] for c in codes] == [1, 3, 21, 2, 8]
    for i, (a, r) in enumerate(zip(clips, rates)):
        c1, l1 = tiny.audio_encode_batch([a], [r], want_latents=True)
        assert np.array_equal(c1[0], codes[i]), i
        assert np.array_equal(l1[0], lats[i]), i
    # the resampled clip is what encoding its GPU-resampled samples gives
    c16 = tiny.audio_encode(tiny.resample_gpu(clips[3], 16000, 24000))
    assert np.array_equal(c16, codes[3])
    assert all(np.array_equal(a, b) for a, b in zip(tiny.audio_encode_batch(clips, rates), codes))


def _set_scales(eng, cfg, rng):
    """LayerScale drawn in [0.25, 0.75] (the synthetic fill's 0.01 would hide the transformer behind the residual stream)"""
    for l in range(cfg.enc_layers):
        for nme in ("attn_scale", "mlp_scale"):
            eng.set_tensor("enc.layers.%d.%s" % (l, nme), (0.25 + 0.5 * rng.random(cfg.enc_hidden)).astype(np.float32))


@pytest.fixture(scope="module")
def full():
    """the enabled default config at full encoder dimensions, synthetic fill (the talker side shrunk: it plays no part here)"""
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64, flags=q3tts.FLAG_TEST_HOOKS)
    eng.fill_synthetic(7)
    synth_codes = eng.audio_encode(mimi_ref.clip(40 * 1920, 21))     # as q3tts_fill_synthetic leaves the encoder
    _set_scales(eng, cfg, np.random.default_rng(3))
    eng.finalize()
    w = {n[4:]: eng.get_tensor(n, s) for n, s, _ in q3tts.tensor_specs(cfg) if n.startswith("enc.")}
    yield eng, cfg, w, synth_codes
    eng.close()


def test_full_dimensions(full, gold):
    _, _, bound, gate = gold
    eng, cfg, w, _ = full
    x = mimi_ref.clip(2 * 1920 + 1, 20)
    codes, lat = eng.audio_encode(x, want_latents=True)
    rlat, rcodes, gaps = mimi_ref.encode(w, cfg, x)
    assert lat.shape == rlat.shape == (3, 512)
    err = float(np.abs(lat.astype(np.float64) - rlat).max())
    print("full dims: latents max err %.3e (bound %.3e), |latents| max %.2f, distinct code0 %d" % (err, bound, float(np.abs(rlat).max()), len(set(rcodes[:, 0]))))
    assert err <= bound
    mimi_ref.check_codes(codes, rcodes, gaps, gate)


def test_window_at_real_size(full, gold):
    _, _, bound, _ = gold
    eng, cfg, w, _ = full
    rows = np.random.default_rng(5).standard_normal((300, 512)).astype(np.float32)
    got = eng.audio_encoder_transformer(rows)
    want = mimi_ref.transformer({k: np.asarray(v, np.float64) for k, v in w.items()}, cfg, rows.astype(np.float64))
    for r in (0, 249, 250, 299):
        err = float(np.abs(got[r] - want[r]).max())
        print("row %d: max err %.3e (bound %.3e)" % (r, err, bound))
        assert err <= bound


def test_synthetic_codebooks_are_calibrated(full):
    _, cfg, _, codes = full
    distinct = [len(set(codes[:, g])) for g in range(cfg.n_groups)]
    print("synthetic fill, 40 frames: distinct ids per codebook", distinct)
    assert min(distinct) >= 8


def test_icl_recipe_bit_identical(tiny):
    ref_pcm = mimi_ref.clip(3 * 1920, 30)
    ref_ids, ids = [101, 102, 103, 104], frame_tokens([11, 22, 33])
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=20, max_new_tokens=6)
    pcm, codes, F0 = tiny.synthesize_icl(ref_pcm, ref_ids, ids, sp, seed=4, stream_id=2, ignore_eos=True)
    # the manual sequence of INTEGRATION.md section 5c
    ref_codes = tiny.audio_encode(ref_pcm)
    toks = np.concatenate([ids[:3], np.array(ref_ids, np.int64), ids[3:]])
    prompt, trailing = tiny.build_prompt(toks, 0, None)
    tiny.slot_begin(0, prompt, trailing, sp, 4, 2, True, prefix_codes=ref_codes)
    tiny.decode_steps(6)
    manual = tiny.slot_codes(0)
    manual_pcm = tiny.slot_codec_decode_range(0, 3, manual.shape[0], 3)
    tiny.slot_release(0)
    assert F0 == 3 and codes.shape == (9, 16)
    assert np.array_equal(codes[:3], ref_codes) and np.array_equal(codes, manual)
    assert np.array_equal(pcm, manual_pcm)
    assert len(pcm) == tiny.codec_decode_len(9) - tiny.codec_decode_len(3)      # the target's samples only


def test_refusals(tiny):
    eng = q3tts.Engine(q3tts.Config.from_dict(qo.config_tiny().to_dict()), device=0, max_batch=1, max_ctx=32)
    try:
        eng.fill_synthetic(0)
        assert not eng.has_audio_encoder
        with pytest.raises(RuntimeError, match="model has no audio encoder"):
            eng.audio_encode(mimi_ref.clip(1920, 0))
        assert eng.text_project([1, 2]).shape == (2, eng.cfg.hidden)            # still usable
    finally:
        eng.close()
    too_long = np.zeros(1440001, np.float32)
    with pytest.raises(RuntimeError, match="clip too long for the audio encoder"):
        tiny.audio_encode(too_long)
    with pytest.raises(RuntimeError, match="samples to resample, the cap is 23040000"):     # the raw upload is bounded too, before anything moves
        tiny.audio_encode_batch([mimi_ref.clip(1920, 1), np.zeros(23040001, np.float32)], [24000, 384000])
    with pytest.raises(RuntimeError, match="n_samples must be at least 1"):
        tiny.audio_encode(np.zeros(0, np.float32))
    assert tiny.audio_encode(mimi_ref.clip(1920, 0)).shape == (1, 16)          # and the engine goes on working
