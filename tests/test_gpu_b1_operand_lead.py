"""The two b = 1 launches that issue their small operands ahead of their weight loads — k_gemv1 PSUM (gate/up behind a kv-head-split
o_proj: x, the 8 partial rows and one 16-byte unit of gamma per thread, gamma shared through LDS; GemvArgs::psum_lead) and k_cp_attn_kvh
(the predictor attention's operands ahead of the o_proj K-slice; CpAttnOprojArgs::lead), both the engine's default — against the same
build with both orders as they were (Q3TTS_GEMV_PSUM_LEAD=0 Q3TTS_CP_KVH_LEAD=0, the A/B knobs).  Only the order of the loads and the
way gamma reaches the registers differ: every lane holds the same values in the same registers and the summation order is kept, so
everything is compared with np.array_equal on the raw fp32.  Covered: PSUM at K = 1024 with one row (the talker's 28 layers), with two
rows (the predictor's first pass) and at K = 2048 (1.7B dims, the largest prologue); k_cp_attn_kvh with two new
rows and with one new row over 2..15 cached tokens (U = 1..4)."""
import os

import numpy as np
import pytest

from util import Hip, frame_tokens

pytestmark = pytest.mark.gpu

KNOBS = ("Q3TTS_GEMV_PSUM_LEAD", "Q3TTS_CP_KVH_LEAD")


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free()


def _engine(lead, model="0.6b", max_batch=1, max_ctx=128):
    """lead None: a default engine; "0": a hooks engine with both load orders as they were"""
    import q3tts
    cfg = q3tts.default_config(model)
    if lead is None:
        eng = q3tts.Engine(cfg, device=0, max_batch=max_batch, max_ctx=max_ctx)
    else:
        for k in KNOBS:
            os.environ[k] = lead
        try:
            eng = q3tts.Engine(cfg, device=0, max_batch=max_batch, max_ctx=max_ctx, flags=q3tts.FLAG_TEST_HOOKS)
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
    eng.fill_synthetic(seed=0)
    return eng


def _pair(**kw):
    new = _engine(None, **kw)
    try:
        return new, _engine("0", **kw)
    except Exception:
        new.close()
        raise


def _talker_steps(hip, eng, n_steps, seed):
    """8-row prefill, then n_steps teacher-forced q3tts_talker_decode_dev steps: [(logits, hidden)] and the last hidden row's buffer"""
    H, V = eng.cfg.hidden, eng.cfg.vocab
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((8, H)) * 0.05).astype(np.float32)
    x_d, e_d, lg_d, lh_d = hip.put(x), hip.alloc(H * 4), hip.alloc(V * 4), hip.alloc(H * 4)
    eng.talker_prefill_dev(x_d, 1, 8, None, lg_d, lh_d)
    out = []
    for _ in range(n_steps):
        hip.write(e_d, (rng.standard_normal(H) * 0.05).astype(np.float32))
        eng.talker_decode_dev(e_d, 1, None, lg_d, lh_d)
        out.append((hip.get(lg_d, (V,), np.float32), hip.get(lh_d, (H,), np.float32)))
    return out, lh_d


def test_talker_steps_and_predictor_frame_bit_equal_06b(hip):
    """0.6B dims, one slot: 6 teacher-forced talker steps (logits and hidden rows: PSUM at K = 1024, one row, 28 layers), one predictor
    frame on device pointers (sampled sub-codes: its first pass has two new rows, the passes at bases 2..15 cover U = 1..4), and 3 fused
    steps read back through step_logits (the logits row behind each of the 16 decisions of a frame, and the codes)."""
    import q3tts
    new, old = _pair()
    try:
        G = new.cfg.n_groups
        subs = []
        for eng in (new, old):
            steps, lh_d = _talker_steps(hip, eng, 6, 21)
            c0_d, sub_d = hip.put(np.array([1234], np.int64)), hip.alloc((G - 1) * 4)
            eng.code_predictor_dev(lh_d, c0_d, 1, q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=1), 99, 40, 5, sub_d)
            subs.append((steps, hip.get(sub_d, (G - 1,), np.int32)))
        (sa, ca), (sb, cb) = subs
        for i in range(6):
            assert np.isfinite(sa[i][0]).all()
            assert np.array_equal(sa[i][0], sb[i][0]) and np.array_equal(sa[i][1], sb[i][1]), i
        assert np.array_equal(ca, cb), (ca, cb)
        p, t = new.build_prompt(frame_tokens(np.random.default_rng(7).integers(0, 151643, 12)), 0)
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=4)
        rows = []
        for eng in (new, old):
            eng.slot_begin(0, p, t, sp, 11, 3, True)
            rows.append(([eng.step_logits(0) for _ in range(3)], eng.slot_codes(0)))
            eng.slot_release(0)
        (la, fa), (lb, fb) = rows
        assert fa.shape == (3, G) and np.array_equal(fa, fb)
        for i in range(3):
            assert np.asarray(la[i]).shape[0] == G and np.isfinite(la[i]).all()
            assert np.array_equal(la[i], lb[i]), i
    finally:
        new.close()
        old.close()


def test_two_slots_three_fused_steps_same_codes_and_logits():
    """Two slots with different prompts and seeds, 3 fused steps: codes and logits of both slots.  A step of two rows has two distinct
    rows in each of its GEMV launches; the launches that take partial rows are one-utterance launches (run_layers: nb == 1, or M == 1
    over split-T partials), so what this pins is that the knobs move nothing else in a wider engine.  Two distinct rows in a PSUM launch
    (row stride in LDS, row clamp) are the predictor's first pass in the test above."""
    import q3tts
    new, old = _pair(max_batch=2)
    try:
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=3)
        got = []
        for eng in (new, old):
            for slot in (0, 1):
                p, t = eng.build_prompt(frame_tokens(np.random.default_rng(40 + slot).integers(0, 151643, 9 + 4 * slot)), 0)
                eng.slot_begin(slot, p, t, sp, 5 + slot, slot, True)
            eng.decode_steps(3)
            got.append([eng.slot_codes(slot) for slot in (0, 1)] + [eng.slot_logits(slot)[0] for slot in (0, 1)])
        a, b = got
        assert a[0].shape == (3, new.cfg.n_groups) and not np.array_equal(a[0], a[1])
        assert np.isfinite(a[2]).all() and np.isfinite(a[3]).all()
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    finally:
        new.close()
        old.close()


def test_talker_steps_bit_equal_17b(hip):
    """1.7B dims: 2 talker steps — PSUM at K = 2048 (two 16-byte units of every row and of gamma per thread), the largest prologue"""
    new, old = _pair(model="1.7b", max_ctx=64)
    try:
        assert new.cfg.hidden == 2048
        a, _ = _talker_steps(hip, new, 2, 5)
        b, _ = _talker_steps(hip, old, 2, 5)
        for i in range(2):
            assert np.isfinite(a[i][0]).all()
            assert np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]), i
    finally:
        new.close()
        old.close()


def test_synthesize_batch_four_frames_bit_equal():
    """The whole job at b = 1 (prefill, captured decode step, vocoder): codes and PCM"""
    import q3tts
    new, old = _pair(max_ctx=256)
    try:
        ids = frame_tokens(np.random.default_rng(1).integers(0, 151643, 16))
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=4)
        pa, ca, na = new.synthesize_batch([ids], sp, seed=3, ignore_eos=True)
        pb, cb, nb = old.synthesize_batch([ids], sp, seed=3, ignore_eos=True)
        assert na[0] == 4 and nb[0] == 4 and np.isfinite(pa[0]).all()
        assert np.array_equal(ca[0], cb[0]) and np.array_equal(pa[0], pb[0])
    finally:
        new.close()
        old.close()
