"""Engines that hold one set of weights (q3tts_create_sharing; SURVEY.md 8b: "weights immutable & shareable across handles").

A sharer launches the kernels a private engine launches, over the same bytes, so every comparison here is np.array_equal: codes,
logits, PCM, speaker embeddings, encoder codes and latents, carried-state vocoder pushes.  The accounting (q3tts_weights_info), the
refusals of a shared set, the holders' lifetimes in both orders, three holders stepping at once while a fourth comes and goes, and at
0.6B dims the layer-0 QKV table that the first holder it applies to builds once for the set."""
import json
import os
import threading

import numpy as np
import pytest

import q3_oracle as qo
from util import calibrate_codec, frame_tokens, tiny_pair, to_q3cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 24


def _sp(sampled, n=FRAMES):
    import q3tts
    return q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=n + 4) if sampled else \
        q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=n + 4)


def _prompt(eng):
    return eng.build_prompt(np.asarray(frame_tokens([11, 22, 33, 44, 55]), np.int64), 0)


def _run(eng, prompt, trailing, sampled, n=FRAMES, slot=0, stream_id=3):
    """(codes, logits after the begin, PCM) of n frames in one slot"""
    eng.slot_release(slot)
    eng.slot_begin(slot, prompt, trailing, _sp(sampled, n), seed=5, stream_id=stream_id, ignore_eos=True)
    logits = eng.slot_logits(slot)[0].copy()
    eng.decode_steps(n)
    codes = eng.slot_codes(slot).copy()
    assert codes.shape[0] == n
    pcm = eng.slot_codec_decode(slot).copy()
    eng.slot_release(slot)
    return codes, logits, pcm


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _private(w, ocfg=None, **kw):
    import q3tts
    eng = q3tts.Engine(to_q3cfg(ocfg or qo.config_tiny()), device=0, **kw)
    eng.load(w)
    return eng


# ---- 1. same output as a private engine -------------------------------------------------------------------------------------------
def test_sharer_equals_a_private_engine_and_leaves_the_donor_alone():
    donor, orc, w = tiny_pair(max_batch=4)
    orc.close()
    prompt, trailing = _prompt(donor)
    before = [_run(donor, prompt, trailing, s) for s in (False, True)]
    sharer = donor.share(max_batch=4)
    private = _private(w, max_batch=4, max_ctx=128)
    try:
        for i, sampled in enumerate((False, True)):
            got, want = _run(sharer, prompt, trailing, sampled), _run(private, prompt, trailing, sampled)
            assert np.array_equal(got[0], want[0]), "codes"
            assert np.array_equal(got[1], want[1]), "logits after the begin"
            assert np.array_equal(got[2], want[2]), "PCM"
            assert _same(_run(donor, prompt, trailing, sampled), before[i]), "the donor's results changed when a sharer appeared"
            assert _same(got, before[i])
        assert not np.array_equal(before[0][0], before[1][0])      # greedy and sampled are different runs
    finally:
        for e in (sharer, private, donor):
            e.close()


# ---- 2. accounting and lifetimes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("donor_first", [True, False])
def test_accounting_and_either_holder_may_go_first(donor_first):
    donor, orc, _ = tiny_pair(max_batch=4)
    orc.close()
    prompt, trailing = _prompt(donor)
    info0 = donor.weights_info()
    assert info0["holders"] == 1 and info0["shared_bytes"] > 0 and info0["private_weight_bytes"] == 0
    # the registry alone is a lower bound of what the set holds: 2 bytes per bf16 element, 4 per fp32 one
    assert info0["shared_bytes"] >= sum(2 * int(np.prod(s)) for _, s in donor.tensor_infos())
    sharer = donor.share(max_batch=4)
    try:
        for e in (donor, sharer):
            info = e.weights_info()
            assert info["holders"] == 2 and info["shared_bytes"] == info0["shared_bytes"], info
        assert sharer.weights_info()["private_weight_bytes"] == 0
        want = _run(sharer, prompt, trailing, True)
        first, rest = (donor, sharer) if donor_first else (sharer, donor)
        first.close()
        info = rest.weights_info()
        assert info["holders"] == 1 and info["shared_bytes"] == info0["shared_bytes"]
        assert _same(_run(rest, prompt, trailing, True), want)      # the set outlives the holder that left
    finally:
        sharer.close()
        donor.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_shared_set_refuses_mutation_and_an_unshared_one_takes_it_again(tmp_path):
    import q3tts
    donor, orc, w = tiny_pair(max_batch=2)
    orc.close()
    prompt, trailing = _prompt(donor)
    path = str(tmp_path / "tiny.q3w")
    donor.save_weights(path)
    sharer = donor.share(max_batch=2)
    try:
        name = "talker.codec_head"
        for e in (donor, sharer):
            with pytest.raises(RuntimeError, match="shared by 2 engines"):
                e.set_tensor(name, w[name])
            with pytest.raises(RuntimeError, match="shared"):
                e.fill_synthetic(1)
            with pytest.raises(RuntimeError, match="shared"):
                e.load_weights(path)
            e.finalize()                                            # returns without error and does nothing
            assert np.array_equal(e.get_tensor(name, w[name].shape), w[name])      # the read-only calls work on every holder
        sharer.save_weights(str(tmp_path / "again.q3w"))
        assert open(path, "rb").read() == open(str(tmp_path / "again.q3w"), "rb").read()
        base = _run(donor, prompt, trailing, False, n=4)
        assert _same(_run(sharer, prompt, trailing, False, n=4), base)             # nothing above moved a byte
        sharer.close()
        assert donor.weights_info()["holders"] == 1
        w2 = dict(w)
        w2[name] = qo.bf16_round(-w[name])
        donor.set_tensor(name, w2[name])                           # alone again: the donor's weights can change
        donor.finalize()
        flipped = _run(donor, prompt, trailing, False, n=4)
        assert not np.array_equal(flipped[1], base[1])             # the head's sign went into the logits
        private = _private(w2, max_batch=2, max_ctx=128)
        try:
            assert _same(flipped, _run(private, prompt, trailing, False, n=4))      # and everything derived was rebuilt from the new weights
        finally:
            private.close()
    finally:
        sharer.close()
        donor.close()
    raw = q3tts.Engine(to_q3cfg(qo.config_tiny()), device=0, max_batch=1, max_ctx=64)
    try:
        with pytest.raises(RuntimeError, match="not finalized"):
            raw.share()
        for k, v in w.items():
            raw.set_tensor(k, v)                                    # filled but not finalized: still refused
        with pytest.raises(RuntimeError, match="not finalized"):
            raw.share()
    finally:
        raw.close()


def test_flags_that_select_a_derived_layout_must_match_the_others_may_differ():
    import q3tts
    FP32_CODEC = 4
    donor, orc, w = tiny_pair(max_batch=2)
    orc.close()
    exact = _private(w, max_batch=1, max_ctx=128, flags=FP32_CODEC)
    prompt, trailing = _prompt(donor)
    try:
        with pytest.raises(RuntimeError, match="Q3TTS_FLAG_FP32_CODEC"):
            donor.share(flags=FP32_CODEC)
        with pytest.raises(RuntimeError, match="Q3TTS_FLAG_FP32_CODEC"):
            exact.share(flags=0)
        assert donor.weights_info()["holders"] == 1 and exact.weights_info()["holders"] == 1      # a refused share holds nothing
        with pytest.raises(RuntimeError, match="max_batch"):
            donor.share(max_batch=0)                                # what q3tts_create_pooled refuses
        assert donor.weights_info()["holders"] == 1
        sharer = donor.share(max_batch=2, flags=q3tts.FLAG_KV_BF16)
        private = _private(w, max_batch=2, max_ctx=128, flags=q3tts.FLAG_KV_BF16)
        try:
            assert _same(_run(sharer, prompt, trailing, True, n=8), _run(private, prompt, trailing, True, n=8))
        finally:
            sharer.close()
            private.close()
    finally:
        exact.close()
        donor.close()


# ---- 4. the other components on a sharer ---------------------------------------------------------------------------------------------
def _voice(seconds, rate, seed):      # tests/test_gpu_clone.py's clip
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    f0 = 120 + 40 * np.sin(2 * np.pi * 0.7 * t)
    x = sum(a * np.sin(2 * np.pi * k * np.cumsum(f0) / rate) for k, a in ((1, 0.3), (2, 0.2), (3, 0.12), (5, 0.05)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)


def test_speaker_embedding_on_a_sharer():
    donor, orc, _ = tiny_pair(seed=6, max_batch=1, max_ctx=64)
    orc.close()
    sharer = donor.share()
    try:
        clip = _voice(0.5, 16000, 0)
        want = donor.speaker_embeddings([clip], 16000)
        got = sharer.speaker_embeddings([clip], 16000)
        assert want.shape == (1, donor.cfg.spk_enc_dim) and np.abs(want).max() > 0
        assert np.array_equal(got, want)
        mel = (2.0 * np.random.default_rng(1).standard_normal((128, 17)) - 4.0).astype(np.float32)
        assert np.array_equal(sharer.speaker_encoder(mel), donor.speaker_encoder(mel))
    finally:
        sharer.close()
        donor.close()


def test_audio_encode_on_a_sharer():
    import mimi_ref
    import q3tts
    z = np.load(os.path.join(ROOT, "tests", "golden", "hf_mimi_encoder.npz"))
    w_enc = {k[6:]: z[k] for k in z.files if k.startswith("w:enc.")}
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)
    w.update({"enc." + k: v for k, v in w_enc.items()})
    cfg = q3tts.Config.from_dict(dict(ocfg.to_dict(), **json.loads(str(z["cfg"]))))
    donor = q3tts.Engine(cfg, device=0, max_batch=2, max_ctx=192)
    donor.load(w)
    sharer = donor.share()
    try:
        clip = mimi_ref.clip(1921, 3)                               # two frames, the second one ragged
        want_codes, want_lat = donor.audio_encode(clip, want_latents=True)
        got_codes, got_lat = sharer.audio_encode(clip, want_latents=True)
        assert want_codes.shape == (2, cfg.n_groups)
        assert np.array_equal(got_codes, want_codes) and np.array_equal(got_lat, want_lat)
        assert sharer.weights_info()["private_weight_bytes"] == 0
    finally:
        sharer.close()
        donor.close()


def test_carried_state_vocoder_pushes_on_a_sharer():
    donor, orc, _ = tiny_pair(seed=2, max_batch=3, max_ctx=512)
    orc.close()
    sharer = donor.share(max_batch=3)
    try:
        rng = np.random.default_rng(4)
        codes = [rng.integers(0, donor.cfg.cd_codebook, (6, donor.cfg.n_groups)).astype(np.int64) for _ in range(2)]
        outs = []
        for e in (donor, sharer):
            sids = [e.codec_stream_begin(6) for _ in range(2)]
            first = e.codec_stream_push_batch(sids, [c[:3] for c in codes])
            second = e.codec_stream_push_batch(sids, [c[3:] for c in codes])      # carried state: K / V and output rows of the first push
            for s in sids:
                e.codec_stream_end(s)
            outs.append(first + second)
        assert all(o.size > 0 for o in outs[0])
        assert _same(outs[1], outs[0])
    finally:
        sharer.close()
        donor.close()


# ---- 5. concurrent holders ------------------------------------------------------------------------------------------------------------
def test_three_holders_step_concurrently_while_a_fourth_comes_and_goes():
    B, steps = 4, 24
    donor, orc, _ = tiny_pair(max_batch=B)
    orc.close()
    holders = [donor, donor.share(max_batch=B), donor.share(max_batch=B)]
    sp = _sp(True, steps)
    prompt, trailing = _prompt(donor)

    def arm(e, g):
        for b in range(B):
            e.slot_release(b)
        for b in range(B):
            e.slot_begin(b, prompt, trailing, sp, seed=5, stream_id=g * B + b, ignore_eos=True)
    try:
        bytes0 = donor.weights_info()["shared_bytes"]
        solo = []
        for g, e in enumerate(holders):
            arm(e, g)
            e.decode_steps(steps)
            solo.append([e.slot_codes(b).copy() for b in range(B)])
        assert not np.array_equal(solo[0][0], solo[1][0])          # different RNG streams: the holders do different work
        for g, e in enumerate(holders):
            arm(e, g)
        bar, errs, seen = threading.Barrier(len(holders) + 1), [], []

        def run(e):
            try:
                bar.wait()
                e.decode_steps(steps)
            except Exception as ex:   # noqa: BLE001 - reported below
                errs.append(ex)

        def visit():
            try:
                bar.wait()
                extra = donor.share(max_batch=B)                    # while the donor generates on another thread
                seen.append(extra.weights_info()["holders"])
                extra.close()
            except Exception as ex:   # noqa: BLE001 - reported below
                errs.append(ex)
        th = [threading.Thread(target=run, args=(e,)) for e in holders] + [threading.Thread(target=visit)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        assert seen == [4]
        for g, e in enumerate(holders):
            for b in range(B):
                assert np.array_equal(e.slot_codes(b), solo[g][b]), ("holder %d slot %d differs from its solo run" % (g, b))
            info = e.weights_info()
            assert info["holders"] == 3 and info["shared_bytes"] == bytes0
    finally:
        for e in reversed(holders):
            e.close()


# ---- 6. 0.6B dims: packed copies and the layer-0 QKV table ----------------------------------------------------------------------------
def _full(max_batch):
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=max_batch, max_ctx=96)
    eng.fill_synthetic(seed=0)
    return eng


def _table_bytes(cfg):
    qkv = (cfg.cp_heads + 2 * cfg.cp_kv_heads) * cfg.cp_head_dim
    return (cfg.n_groups - 2) * cfg.sub_vocab * qkv * 4


@pytest.fixture(scope="module")
def full_b1():
    """a private one-slot engine at 0.6B dims and its 16 sampled frames: the reference of both table cases, computed once"""
    eng = _full(1)
    prompt, trailing = _prompt(eng)
    want = _run(eng, prompt, trailing, True, n=16)
    info = eng.weights_info()
    yield eng, prompt, trailing, want, info
    eng.close()


def test_full_dims_the_first_qualifying_sharer_builds_the_table(full_b1):
    import q3tts
    _, prompt, trailing, want, info_b1 = full_b1
    donor = _full(8)                                                # more than two slots: no table at finalize
    try:
        before = donor.weights_info()
        assert before["shared_bytes"] == info_b1["shared_bytes"] - _table_bytes(donor.cfg)      # a one-slot engine's set: the same + the table
        os.environ["Q3TTS_CP_QKV_TABLE"] = "0"                      # the knob that gates the table, honoured by a hook engine
        try:
            off = donor.share(max_batch=1, flags=q3tts.FLAG_TEST_HOOKS)
        finally:
            os.environ.pop("Q3TTS_CP_QKV_TABLE", None)
        try:
            assert off.weights_info()["shared_bytes"] == before["shared_bytes"]      # knob off: nothing is built
            assert off.weights_info()["private_weight_bytes"] == 0
            assert _same(_run(off, prompt, trailing, True, n=16), want)              # the GEMV path: the same bits
        finally:
            off.close()
        sharer = donor.share(max_batch=1)
        try:
            for e in (donor, sharer):
                info = e.weights_info()
                assert info["holders"] == 2 and info["shared_bytes"] == before["shared_bytes"] + _table_bytes(donor.cfg), info
            assert sharer.weights_info()["private_weight_bytes"] == 0
            assert _same(_run(sharer, prompt, trailing, True, n=16), want)           # rows built on the sharer's stream == rows built at finalize
            second = donor.share(max_batch=2)                       # the table applies again: reused
            try:
                assert second.weights_info()["shared_bytes"] == before["shared_bytes"] + _table_bytes(donor.cfg)
            finally:
                second.close()
        finally:
            sharer.close()
    finally:
        donor.close()


def test_full_dims_a_second_qualifying_holder_reuses_the_table(full_b1):
    donor, prompt, trailing, want, info_b1 = full_b1
    sharer = donor.share(max_batch=1)
    try:
        info = sharer.weights_info()
        assert info["holders"] == 2 and info["shared_bytes"] == info_b1["shared_bytes"] and info["private_weight_bytes"] == 0
        assert _same(_run(sharer, prompt, trailing, True, n=16), want)
        assert _same(_run(donor, prompt, trailing, True, n=16), want)
    finally:
        sharer.close()
    assert donor.weights_info()["holders"] == 1
