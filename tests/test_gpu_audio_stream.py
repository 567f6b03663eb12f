"""Streamed audio-to-codes (q3tts_audio_stream_*): the codes and latents of a stream, however its samples were cut into pushes and whatever
other streams shared its calls, are bit-identical (np.array_equal) to Engine.audio_encode of the concatenated audio.

The tiny golden config has window 6, so the K/V ring wraps after 5 760 samples; the full-dimension case crosses the real window of 250
rows on the real MFMA tile shapes.  The only tolerance is in the case beyond the old RoPE table, whose one-shot does not exist: the
golden's existing bound (10 x hf_fp32_err) against the fp64 restatement of the clip's tail."""
import json
import os

import numpy as np
import pytest

import mimi_ref
import q3_oracle as qo
import q3tts
from util import calibrate_codec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hf_mimi_encoder.npz")
RAGGED = [777, 1, 1919, 4000, 1143, 960, 961]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    w = {k[6:]: z[k] for k in z.files if k.startswith("w:enc.")}
    return w, json.loads(str(z["cfg"])), 10.0 * float(z["hf_fp32_err"])


def make_tiny(gold):
    w_enc, cfg, _ = gold
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)
    w.update({"enc." + k: v for k, v in w_enc.items()})
    eng = q3tts.Engine(q3tts.Config.from_dict(dict(ocfg.to_dict(), **cfg)), device=0, max_batch=2, max_ctx=192, flags=q3tts.FLAG_TEST_HOOKS)
    eng.load(w)
    return eng


@pytest.fixture(scope="module")
def tiny(gold):
    eng = make_tiny(gold)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oneshot(tiny):
    """(codes, latents) of the one-shot encode per (n, seed), computed once"""
    memo = {}

    def get(n, seed):
        if (n, seed) not in memo:
            memo[(n, seed)] = tiny.audio_encode(mimi_ref.clip(n, seed), want_latents=True)
        return memo[(n, seed)]
    return get


def cuts_of(n, sizes, rest=True):
    out, at = [], 0
    for s in sizes:
        out.append((at, min(at + s, n)))
        at = min(at + s, n)
    if rest and at < n:
        out.append((at, n))
    return out


def run_stream(eng, x, cuts, batch_api=False, max_samples=0):
    """push x[a:b] for every cut, then finish; checks the frame count and push_len's prediction after every push"""
    sid = eng.audio_stream_begin(max_samples)
    codes, lats, total = [], [], 0
    try:
        for a, b in list(cuts) + [(None, None)]:
            part = x[a:b] if a is not None else x[:0]
            fin = a is None
            want = eng.audio_stream_push_len(sid, part.size, fin)
            if batch_api:
                c, l = eng.audio_stream_push_batch([sid], [part], [fin], want_latents=True)
                c, l = c[0], l[0]
            else:
                c, l = eng.audio_stream_push(sid, part, fin, want_latents=True)
            assert c.shape[0] == l.shape[0] == want, (a, b, c.shape, want)
            total += part.size
            codes.append(c)
            lats.append(l)
            ns, nf, finished, _ = eng.audio_stream_info(sid)
            assert ns == total and finished == fin and nf == sum(k.shape[0] for k in codes)
            if not fin:
                assert nf == total // 1920, (total, nf)
    finally:
        eng.audio_stream_end(sid)
    return np.concatenate(codes), np.concatenate(lats), codes[-1].shape[0]


CUTS = {
    "one_push": (39177, lambda n: [(0, n)]),
    "frame_pushes": (39177, lambda n: cuts_of(n, [1920] * (n // 1920 + 1))),
    "ragged": (39177, lambda n: cuts_of(n, RAGGED)),
    "hundreds": (10560, lambda n: cuts_of(n, [100] * (n // 100 + 1))),
    "one_sample": (1, lambda n: [(0, 1)]),
    "three_frames_exactly": (5760, lambda n: cuts_of(n, [2000, 2000])),
}


@pytest.mark.parametrize("name", list(CUTS))
def test_cut_patterns(tiny, oneshot, name):
    n, mk = CUTS[name]
    x = mimi_ref.clip(n, 5)
    rc, rl = oneshot(n, 5)
    c, l, last = run_stream(tiny, x, mk(n))
    assert c.shape == rc.shape and l.shape == rl.shape
    assert np.array_equal(c, rc) and np.array_equal(l, rl)
    assert last == (0 if n % 1920 == 0 else 1)          # the finish emits the one frame the right edge completes, or none


def test_one_sample_pushes_through_push_batch(tiny, oneshot):
    n = 3841
    x = mimi_ref.clip(n, 5)
    rc, rl = oneshot(n, 5)
    c, l, last = run_stream(tiny, x, [(i, i + 1) for i in range(n)], batch_api=True)
    assert last == 1 and np.array_equal(c, rc) and np.array_equal(l, rl)


def test_batched_pushes_bit_identical_to_solo(tiny, oneshot):
    # per stream: (samples, seed, the cut of each round; None = not in that round's call)
    # 0 fresh in round 1; 1 past the window (4 frames > window 6 rows at 25 Hz) before round 1; 2 gets 0 samples in round 1;
    # 3 finishes in round 1 with a partial frame; 4 finishes in round 1 with 0 new samples
    N = [3 * 1920 + 500, 9 * 1920 + 77, 2 * 1920 + 901, 5 * 1920 + 333, 2 * 1920 + 1000]
    r0 = [None, (0, 4 * 1920 + 11), (0, 1000), (0, 1920 + 5), (0, N[4])]
    r1 = [(0, 2000), (r0[1][1], r0[1][1] + 3000), (1000, 1000), (r0[3][1], N[3]), (N[4], N[4])]
    fin1 = [False, False, False, True, True]
    xs = [mimi_ref.clip(n, 30 + i) for i, n in enumerate(N)]
    sids = [tiny.audio_stream_begin() for _ in N]
    got_c, got_l = [[] for _ in N], [[] for _ in N]

    def push(idx, cuts, fins):
        c, l = tiny.audio_stream_push_batch([sids[i] for i in idx], [xs[i][cuts[i][0]:cuts[i][1]] for i in idx], [fins[i] for i in idx], want_latents=True)
        for k, i in enumerate(idx):
            got_c[i].append(c[k])
            got_l[i].append(l[k])
    try:
        push([1, 2, 3, 4], r0, [False] * 5)
        before = tiny.audio_stream_info(sids[2])
        push([0, 1, 2, 3, 4], r1, fin1)
        assert tiny.audio_stream_info(sids[2]) == before and got_c[2][-1].shape[0] == 0          # 0 samples: unchanged
        assert got_c[3][-1].shape[0] == 5 and got_c[4][-1].shape[0] == 1             # 6 frames in all, 1 before; the partial third frame
        # the streams still open take the rest and finish, all in one call
        rest = [0, 1, 2]
        r2 = [(r1[0][1], N[0]), (r1[1][1], N[1]), (1000, N[2]), None, None]
        push(rest, r2, [True] * 5)
    finally:
        for s in sids:
            tiny.audio_stream_end(s)
    for i, n in enumerate(N):
        rc, rl = oneshot(n, 30 + i)
        c, l = np.concatenate(got_c[i]), np.concatenate(got_l[i])
        assert np.array_equal(c, rc) and np.array_equal(l, rl), i
        cuts = [r for r in (r0[i], r1[i], r2[i] if i < 3 else None) if r is not None]
        sc, sl, _ = run_stream(tiny, xs[i], cuts)                                               # the same cuts, alone
        assert np.array_equal(c, sc) and np.array_equal(l, sl), i


def test_state_lives_outside_the_workspace(gold, oneshot):
    n = 19 * 1920 + 77
    x = mimi_ref.clip(n, 6)
    rc, rl = oneshot(n, 6)
    half = n // 2
    eng = make_tiny(gold)          # an engine of its own: the half clip is all its workspace has seen, whatever ran before in this module
    try:
        sid = eng.audio_stream_begin()
        c0, l0 = eng.audio_stream_push(sid, x[:half], want_latents=True)
        big = eng.audio_encode(mimi_ref.clip(60000, 8))          # larger than anything this engine encoded so far: the workspace regrows
        assert big.shape[0] == 32
        c1, l1 = eng.audio_stream_push(sid, x[half:], finish=True, want_latents=True)
        eng.audio_stream_end(sid)
    finally:
        eng.close()
    assert np.array_equal(np.concatenate([c0, c1]), rc) and np.array_equal(np.concatenate([l0, l1]), rl)


def test_validation_leaves_streams_unmoved(tiny, oneshot):
    n = 4 * 1920 + 123
    x = mimi_ref.clip(n, 9)
    rc, rl = oneshot(n, 9)
    a = tiny.audio_stream_begin()
    b = tiny.audio_stream_begin(max_samples=5000)
    done = tiny.audio_stream_begin()
    two_min = tiny.audio_stream_begin(max_samples=2880000)      # the per-push cap, not max_samples, must refuse 1 440 001 samples
    try:
        tiny.audio_stream_push(done, x[:100], finish=True)
        c0, l0 = tiny.audio_stream_push(a, x[:3000], want_latents=True)
        state = tiny.audio_stream_info(a)
        with pytest.raises(RuntimeError, match="no open audio stream with id 977"):
            tiny.audio_stream_push(977, x[:10])
        with pytest.raises(RuntimeError, match="given twice in one push"):           # the binding refuses duplicates itself: go below it
            _raw_push(tiny, [a, a], [x[3000:3100], x[3100:3200]])
        with pytest.raises(RuntimeError, match="is finished"):
            tiny.audio_stream_push(done, x[:10])
        with pytest.raises(RuntimeError, match="over its max_samples"):
            tiny.audio_stream_push_batch([a, b], [x[3000:4000], np.zeros(5001, np.float32)])
        with pytest.raises(RuntimeError, match="push too long"):
            tiny.audio_stream_push_batch([a, two_min], [x[3000:4000], np.zeros(1440001, np.float32)])
        with pytest.raises(RuntimeError, match="output buffer too small"):
            _raw_push(tiny, [a, b], [x[3000:4000], x[:4000]], caps=[4, 1])
        assert tiny.audio_stream_info(a) == state                                   # the good first stream of the refused calls has not advanced
        c1, l1 = tiny.audio_stream_push(a, x[3000:], finish=True, want_latents=True)
    finally:
        for s in (a, b, done, two_min):
            tiny.audio_stream_end(s)
    assert np.array_equal(np.concatenate([c0, c1]), rc) and np.array_equal(np.concatenate([l0, l1]), rl)


def _raw_push(eng, sids, pcms, caps=None):
    """q3tts_audio_stream_push_batch_host without the binding's own checks"""
    import ctypes as C
    n = len(sids)
    keep = [np.ascontiguousarray(p, np.float32) for p in pcms]
    caps = caps or [8] * n
    outs = [np.zeros((c, eng.cfg.n_groups), np.int64) for c in caps]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in keep])
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ids, ns, cp, nf = np.array(sids, np.int32), np.array([a.size for a in keep], np.int64), np.array(caps, np.int32), np.zeros(n, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._ck(eng.L.q3tts_audio_stream_push_batch_host(eng.h, n, vp(ids), ptrs, vp(ns), None, optrs, None, vp(cp), vp(nf)))
    return nf


def test_reuse_after_end(tiny, oneshot):
    x = mimi_ref.clip(39177, 5)
    sid = tiny.audio_stream_begin()
    tiny.audio_stream_push(sid, x[:30000])              # left unfinished, rings full
    tiny.audio_stream_end(sid)
    with pytest.raises(RuntimeError, match="no open audio stream"):
        tiny.audio_stream_info(sid)
    n = 7 * 1920 + 955
    y = mimi_ref.clip(n, 12)
    rc, rl = oneshot(n, 12)
    with q3tts.AudioEncodeStream(tiny) as st:
        assert st.sid == sid                            # the ended stream's id and buffers serve the next begin
        for a, b in cuts_of(n, [2500] * 8):
            st.push(y[a:b])
        st.finish()
        assert np.array_equal(st.codes, rc)
    c, l, _ = run_stream(tiny, y, cuts_of(n, [2500] * 8))
    assert np.array_equal(c, rc) and np.array_equal(l, rl)
    assert np.array_equal(tiny.audio_encode_long(y, chunk_samples=4000), rc)


def test_beyond_the_old_rope_table(tiny, gold):
    w, cfg, bound = gold
    n = 1464333                                          # 763 frames, 1526 rows at 25 Hz: the 60 s table had 1501
    x = mimi_ref.clip(n, 7)
    c, l, last = run_stream(tiny, x, cuts_of(n, [96000] * 16), max_samples=n)
    assert c.shape[0] == l.shape[0] == 763 and last == 1
    rc, rl = tiny.audio_encode(x[:1440000], want_latents=True)
    assert np.array_equal(c[:750], rc) and np.array_equal(l[:750], rl)
    # the tail against the fp64 restatement of a cut at a frame boundary: exact from its 9th frame on (receptive field < 8 frames).
    # n = 762 * 1920 + 1293, so the cut that keeps 20 whole frames and the partial one is 20 * 1920 + 1293 samples from the end
    # (a cut 20 * 1920 + 333 from the end falls on sample 1 425 600 = 742.5 frames: an odd 25 Hz row, where the stride-2 conv of the
    # tail pairs other rows than the whole clip's does, and nothing is comparable: measured distance 2.1)
    assert (n - (20 * 1920 + 1293)) % 1920 == 0
    tail = mimi_ref.latents(w, cfg, x[-(20 * 1920 + 1293):])
    err = float(np.abs(l[-12:].astype(np.float64) - tail[-12:]).max())
    print("last 12 latent rows against the fp64 tail: max err %.3e (bound %.3e)" % (err, bound))
    assert err <= bound


def _set_scales(eng, cfg, rng):
    """LayerScale drawn in [0.25, 0.75] (the synthetic fill's 0.01 would hide the transformer behind the residual stream)"""
    for l in range(cfg.enc_layers):
        for nme in ("attn_scale", "mlp_scale"):
            eng.set_tensor("enc.layers.%d.%s" % (l, nme), (0.25 + 0.5 * rng.random(cfg.enc_hidden)).astype(np.float32))


def test_full_dimensions():
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64, flags=q3tts.FLAG_TEST_HOOKS)
    try:
        eng.fill_synthetic(7)
        _set_scales(eng, cfg, np.random.default_rng(3))
        eng.finalize()
        n = 264500                                       # 276 rows at 25 Hz: the window of 250 is crossed, the 249-row ring wraps
        x = mimi_ref.clip(n, 22)
        rc, rl = eng.audio_encode(x, want_latents=True)
        c, l, last = run_stream(eng, x, cuts_of(n, [38400] * 7))
        assert rc.shape[0] == 138 and last == 1
        assert np.array_equal(c, rc) and np.array_equal(l, rl)
        sid = eng.audio_stream_begin()
        state_bytes = eng.audio_stream_info(sid)[3]
        eng.audio_stream_end(sid)
        assert state_bytes > 8 * 249 * 2 * 512 * 4      # the K/V rings alone: 8.2 MB
    finally:
        eng.close()
