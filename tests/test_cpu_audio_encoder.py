"""Audio encoder (12 Hz tokenizer, audio -> codes), the parts that need no GPU: the numpy restatement tests/mimi_ref.py against the
transformers golden tests/golden/hf_mimi_encoder.npz (made by tests/golden/make_hf_mimi_golden.py), the fixture's power to tell
implementations apart, the registry with the encoder off and on, the host-only length rule, the symbols, and the importer's rules."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import mimi_ref
import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hf_mimi_encoder.npz")
LENGTHS = [1, 1919, 1920, 1921, 5 * 1920 + 777, 39177]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    w = {k[6:]: z[k] for k in z.files if k.startswith("w:enc.")}
    return w, json.loads(str(z["cfg"])), z


def test_ref_reproduces_golden(gold):
    w, cfg, z = gold
    bound = 10.0 * float(z["hf_fp32_err"])
    for seed, n in enumerate(LENGTHS):
        lat, codes, gaps = mimi_ref.encode(w, cfg, mimi_ref.clip(n, seed))
        assert lat.shape == z["lat_%d" % n].shape == (mimi_ref.encode_len(cfg, n), cfg["enc_hidden"])
        err = float(np.abs(lat - z["lat_%d" % n]).max())
        print("n=%d latents err %.3e (bound %.3e)" % (n, err, bound))
        assert err <= bound
        assert np.array_equal(codes, z["codes_%d" % n])
        assert np.allclose(gaps, z["gaps_%d" % n], rtol=1e-3, atol=1e-7)   # the golden's latents carry transformers' float32 RoPE tables (~4e-8)


def test_transformers_own_codes_agree_with_the_checker(gold):
    """The stored decisions (codes_<n>) are the restatement's on transformers' fp64 latents, because transformers' cdist runs in float32
    whatever the model's dtype.  transformers' own codes, for its fp64 and its fp32 model, must agree with them under the margin-aware
    rule the GPU tests use; and the stored count of frames the fp32 model moved is what the stored codes say."""
    w, cfg, z = gold
    gate = 10.0 * float(z["dist_rel_err"])
    moved = frames = 0
    for n in LENGTHS:
        ref, gaps = z["codes_%d" % n], z["gaps_%d" % n]
        for key in ("hfcodes64_%d", "hfcodes32_%d"):
            excused = mimi_ref.check_codes(z[key % n], ref, gaps, gate)
            print("n=%d %s: %d of %d frames excused" % (n, key % n, len(excused), ref.shape[0]))
        moved += int((z["hfcodes32_%d" % n] != ref).any(1).sum())
        frames += ref.shape[0]
    assert [moved, frames] == list(z["hf_fp32_moved"]) and moved <= 0.10 * frames


def test_fixture_discriminates(gold):
    w, cfg, z = gold
    codes = z["codes_39177"]
    assert codes.shape == (21, 16)
    distinct = [len(set(codes[:, g])) for g in range(16)]
    print("distinct ids per codebook on the 21-frame clip:", distinct)
    assert min(distinct) >= 8
    gate = 10.0 * float(z["dist_rel_err"])
    frames = marginal = 0
    for n in LENGTHS:
        g = z["gaps_%d" % n]
        frames += g.shape[0]
        marginal += int((g < gate).any(1).sum())
    print("gate %.3e: %d of %d frames hold a decision under it" % (gate, marginal, frames))
    assert marginal <= 0.10 * frames


def _names(cfg):
    return [n for n, _, _ in q3tts.tensor_specs(cfg)]


def test_registry_off_and_on():
    for name in ("0.6b", "1.7b"):
        off = q3tts.default_config(name)
        assert off.enc_hidden == 0
        names_off = _names(off)
        assert not any(n.startswith("enc.") for n in names_off)
        on = q3tts.enable_audio_encoder(q3tts.default_config(name))
        names_on = _names(on)
        assert names_on[: len(names_off)] == names_off                      # appended behind spk.*
        extra = names_on[len(names_off):]
        assert extra and all(n.startswith("enc.") for n in extra)
        assert "enc.conv_in.w" in extra and "enc.vq.codebook.15" in extra and "enc.layers.7.fc2" in extra and "enc.downsample.w" in extra
        assert "enc.downsample.b" not in extra
        shapes = {n: s for n, s, _ in q3tts.tensor_specs(on)}
        assert shapes["enc.stages.3.down.w"] == (1024, 512, 16) and shapes["enc.conv_out.w"] == (512, 1024, 3)
        assert shapes["enc.vq.codebook.0"] == (2048, 256) and shapes["enc.vq.ac.in_proj"] == (256, 512)


def test_config_from_dict_defaults_encoder_off():
    d = q3tts.default_config("0.6b").to_dict()
    for k in [k for k in d if k.startswith("enc_")]:
        del d[k]
    c = q3tts.Config.from_dict(d)
    assert c.enc_hidden == 0 and list(c.enc_ratios) == [0, 0, 0, 0] and c.enc_rope_theta == 0.0
    assert _names(c) == _names(q3tts.default_config("0.6b"))


def test_encode_len_rule(gold):
    """the checker's rule; q3tts_audio_encode_len itself takes an engine handle, which needs a GPU: tests/test_gpu_audio_encoder.py
    asserts the same five values on it"""
    _, cfg, _ = gold
    for n, f in ((1, 1), (1919, 1), (1920, 1), (1921, 2), (39177, 21)):
        assert mimi_ref.encode_len(cfg, n) == f


def test_symbols_in_header_and_exports():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    new = ["q3tts_config_enable_audio_encoder", "q3tts_has_audio_encoder", "q3tts_audio_encode_len", "q3tts_audio_encode_host",
           "q3tts_audio_encode_batch_host", "q3tts_audio_encode_latents_host", "q3tts_audio_encode_batch_latents_host", "q3tts_last_audio_encode_ms",
           "q3tts_test_audio_encoder_transformer_host"]
    L = C.CDLL(q3tts.LIB_PATH)
    for s in new:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in q3tts.EXPORTS, s
        assert hasattr(L, s), s


def test_importer_maps_mimi_state_dict(gold):
    _, cfg, z = gold
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import import_safetensors as imp
    keys = json.loads(str(z["state_dict_keys"]))
    names = ["speech_tokenizer.encoder_model." + k for k in keys]
    mapping = imp.map_names(names, {"audio_encoder": "speech_tokenizer.encoder_model."})
    c = q3tts.Config.from_dict(dict(q3tts.default_config("0.6b").to_dict(), **cfg))
    want = {n for n in _names(c) if n.startswith("enc.")}
    got = {imp.fold_target(v) for v in mapping.values()}
    assert want <= got, sorted(want - got)[:8]
    # every codebook has both halves of the fold, and nothing of the decoder side is claimed
    for g in range(16):
        assert "enc.vq.codebook.%d" % g in mapping.values() and "enc.vq.codebook.%d#usage" % g in mapping.values()
    assert not any(k.startswith("speech_tokenizer.encoder_model.decoder") for k in mapping)
    # the fold itself: embed_sum / clamp(cluster_usage, 1e-5)
    es, cu = np.arange(12, dtype=np.float32).reshape(4, 3), np.array([2.0, 0.0, 1e-7, 4.0], np.float32)
    out = imp.fold_codebooks({"enc.vq.codebook.0": es, "enc.vq.codebook.0#usage": cu})
    assert np.allclose(out["enc.vq.codebook.0"], es / np.maximum(cu, 1e-5)[:, None]) and list(out) == ["enc.vq.codebook.0"]
