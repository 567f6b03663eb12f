"""b = 1 decode with the layer-0 QKV rows of predictor passes 1..14 looked up in the engine's table (Engine::cp_qkv_tab, copied into
`qkv` by the sampler in front of the pass) against the GEMV launch of the same build (Q3TTS_CP_QKV_TABLE=0, the A/B knob).  A table
row is made by the very launch the step would issue, so everything is compared with np.array_equal: logits rows, sub-codes, frames,
the talker's logits after the last frame.  0.6B dims."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 11


def _engine(table, max_batch=1, max_ctx=256, env=None):
    import q3tts
    cfg = q3tts.default_config("0.6b")
    env = dict(env or {})
    env["Q3TTS_CP_QKV_TABLE"] = "1" if table else "0"
    os.environ.update(env)
    try:
        eng = q3tts.Engine(cfg, device=0, max_batch=max_batch, max_ctx=max_ctx, flags=q3tts.FLAG_TEST_HOOKS)
    finally:
        for k in env:
            os.environ.pop(k, None)
    eng.fill_synthetic(seed=0)
    return eng


def _prompt(eng, seed=7, n=12):
    from util import frame_tokens
    return eng.build_prompt(frame_tokens(np.random.default_rng(seed).integers(0, 151643, n)), 0)


def _forcing_stream(group, code, V):
    """A stream id whose uniform for (SEED, frame 0, group) falls in the middle fifth of `code`'s bin of a flat distribution over V
    ids: with a temperature of 1e6 and no top-k / top-p the sampler's distribution is flat to ~1e-6, so it draws exactly `code`."""
    import q3tts
    lo, hi = (code + 0.4) / V, (code + 0.6) / V
    for sid in range(1, 400000):
        if lo <= q3tts.rng_uniform(SEED, sid, 0, group) < hi:
            return sid
    raise AssertionError("no stream id found for (%d, %d)" % (group, code))


def _pairs(G, V):
    """every group whose sampler feeds a later pass (1 .. G - 2), codes 0, V - 1 and two seeded ones in between"""
    rng = np.random.default_rng(2024)
    return [(g, int(c)) for g in range(1, G - 1) for c in (0, V - 1, *rng.integers(1, V - 1, 2))]


def test_table_rows_equal_the_launch():
    """Teacher-forced: the sampler of group g is made to draw a chosen code (flat distribution, chosen uniform), so pass g + 1 runs on
    table row (g, code); the logits row behind every decision of the frame and the frame's codes equal the GEMV path's bit for bit."""
    import q3tts
    on, off = _engine(True), _engine(False)
    try:
        G, V = on.cfg.n_groups, on.cfg.sub_vocab
        p, t = _prompt(on)
        flat = q3tts.Sampling(temperature=1e6, top_p=1.0, top_k=0, max_new_tokens=4)
        for g, code in _pairs(G, V):
            sid = _forcing_stream(g, code, V)
            got = []
            for eng in (on, off):
                eng.slot_begin(0, p, t, flat, SEED, sid, True)
                lg = eng.step_logits(0)
                got.append((lg, eng.slot_codes(0)))
                eng.slot_release(0)
            (la, ca), (lb, cb) = got
            assert ca.shape == (1, G) and ca[0, g] == code, (g, code, ca)
            assert np.isfinite(la).all()
            assert np.array_equal(ca, cb), (g, code)
            assert np.array_equal(la, lb), (g, code, np.abs(la - lb).max(axis=1))
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("kw", [dict(temperature=0.8, top_k=50, top_p=0.95), dict(temperature=1.0, top_k=1, top_p=1.0)], ids=["sampled", "greedy"])
def test_free_running_frames_match(kw):
    """160 frames through the captured graph: the same codes and the same talker logits after the last frame, and twice the same on
    the table engine."""
    import q3tts
    on, off = _engine(True), _engine(False)
    try:
        p, t = _prompt(on)
        sp = q3tts.Sampling(max_new_tokens=160, **kw)
        ca = on.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
        la, ha = on.slot_logits(0)
        cb = off.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
        lb, hb = off.slot_logits(0)
        ca2 = on.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
        la2, ha2 = on.slot_logits(0)
    finally:
        on.close()
        off.close()
    assert ca.shape == (160, 16) and np.array_equal(ca, cb)
    assert np.array_equal(la, lb) and np.array_equal(ha, hb)
    assert np.array_equal(ca2, ca) and np.array_equal(la2, la) and np.array_equal(ha2, ha)


def test_wider_engines():
    """A four-slot engine builds no table and keeps the GEMV when it decodes one slot: the same codes as the one-slot engine's table
    path (its talker attention on the one-slot engine's 64-token splits, so that nothing else differs).  A two-slot engine running both
    slots takes the batched path with or without its table."""
    import q3tts
    from util import frame_tokens
    one, four = _engine(True), _engine(True, max_batch=4, env={"Q3TTS_ATTN_CHUNK": "64"})
    try:
        p, t = _prompt(one)
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=48)
        c1 = one.generate(p, t, sp, seed=9, stream_id=3, ignore_eos=True)
        c4 = four.generate(p, t, sp, seed=9, stream_id=3, ignore_eos=True)
    finally:
        one.close()
        four.close()
    assert c1.shape == (48, 16) and np.array_equal(c1, c4)
    two_on, two_off = _engine(True, max_batch=2), _engine(False, max_batch=2)
    try:
        rng = np.random.default_rng(13)
        toks = [frame_tokens(rng.integers(0, 151643, 10)), frame_tokens(rng.integers(0, 151643, 10))]
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=32)
        _, ca, na = two_on.synthesize_batch(toks, sp, seed=4, ignore_eos=True)
        _, cb, nb = two_off.synthesize_batch(toks, sp, seed=4, ignore_eos=True)
        # one of its slots alone: the table path of a two-slot engine
        p, t = _prompt(two_on)
        sa = two_on.generate(p, t, sp, seed=9, stream_id=3, ignore_eos=True)
        sb = two_off.generate(p, t, sp, seed=9, stream_id=3, ignore_eos=True)
    finally:
        two_on.close()
        two_off.close()
    assert list(na) == [32, 32] and list(nb) == [32, 32]
    for u in range(2):
        assert np.array_equal(ca[u], cb[u]), u
    assert np.array_equal(sa, sb)


def test_weight_change_rebuilds_the_table():
    """set_tensor of the predictor's layer-0 q projection + finalize: the frames change, and they change to what the GEMV path makes of
    the new weights — the table was rebuilt and no graph captured over the old one was replayed."""
    import q3tts
    on, off = _engine(True), _engine(False)
    try:
        p, t = _prompt(on)
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=32)
        before = on.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
        name, shape = next((n, s) for n, s in on.tensor_infos() if n == "cp.layers.0.q_proj")
        w = (np.random.default_rng(99).standard_normal(shape) * 0.02).astype(np.float32)
        for eng in (on, off):
            eng.set_tensor(name, w)
            eng.finalize()
        after_on = on.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
        after_off = off.generate(p, t, sp, seed=5, stream_id=0, ignore_eos=True)
    finally:
        on.close()
        off.close()
    assert not np.array_equal(before[:, 2:], after_on[:, 2:])
    assert np.array_equal(after_on, after_off)
