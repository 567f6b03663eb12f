"""The codec decoder on fp32-origin weights: every cd.* tensor of an imported checkpoint is stored as fp32 (tools/pack_weights.py), so
its fp16 split has a non-zero lo plane and every conv launch takes the three-product kernels (k_conv_split<..., WLO = true>, the lo half
of the chunk-major planes, the fused 96-channel unit's B fragments of the lo plane).  Every other test of the suite feeds
bf16-representable weights, whose lo plane is identically zero: the two-product kernels.

Reference everywhere: the fp32 oracle on the identical weights.  Bound everywhere (tests/test_gpu_full.py::test_codec_full_size,
north_star): RMS error < 1e-4 and < 2e-3 x signal RMS, signal RMS > 1e-3.  Each test prints the measured error and, beside it, the
error of the exact-fp32 matrix-core engine (Q3TTS_FLAG_FP32_CODEC) on the same weights.  tests/test_cpu_codec_split.py shows on the CPU
that these inputs discriminate: an engine that ignored a class's lo plane would be off by >= 10 x the bound; the full-size tests here
repeat that condition on the weights they use.

Only convs with C_in % 32 == 0 and C_out >= 32 run k_conv_split (codec_split_ref.on_split_route): 26 of the tiny config's 49 planes
tensors, all 91 (75 plane pairs) at 0.6B dims — which is why the per-class and the edge tests run at both sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import codec_split_ref as cs
import q3_oracle as qo
from util import Hip, calibrate_codec, frame_tokens, to_ocfg, to_q3cfg

pytestmark = pytest.mark.gpu

FP32_SEED = 1
EDGE_FRAMES = 40
RES1_TINY, DOWN_TINY = "cd.dec.blocks.0.res.1.conv1.w", "cd.layers.1.down_proj"       # 32 -> 32 x 7 taps: on the split route; 48 -> 32: not
RES1_FULL, DOWN_FULL = "cd.dec.blocks.3.res.1.conv1.w", "cd.layers.5.down_proj"       # the fused 96-channel unit; 3072 -> 1024 (split-K slabs)


def _codes(cfg, F, seed=None):
    return np.random.default_rng(F if seed is None else seed).integers(0, cfg.cd_codebook, (F, cfg.n_groups)).astype(np.int64)


def _measure(tag, eng, exact, orc, codes):
    """decode on the split engine and the exact-fp32 engine, print both errors, assert the project's bound on the split engine's"""
    pcm, ref = eng.codec_decode(codes), orc.vocoder(codes)
    assert pcm.shape == ref.shape == (eng.codec_decode_len(codes.shape[0]),)
    assert np.isfinite(pcm).all(), tag
    sig, err = cs.rms(ref), cs.rms(pcm - ref)
    err32 = cs.rms(exact.codec_decode(codes) - ref) if exact is not None else float("nan")
    print("%s, %d frames: rms error vs oracle split-fp16 %.3g, exact-fp32 %.3g, signal rms %.3g, max abs error %.3g; 2 / 3 products: %s"
          % (tag, codes.shape[0], err, err32, sig, float(np.abs(pcm - ref).max()), eng.codec_plane_stats()))
    cs.check_bound(err, sig)
    return err, sig, pcm, ref


class Trio:
    """split engine + exact-fp32 engine + oracle that always hold the same weights"""

    def __init__(self, eng, exact, orc):
        self.eng, self.exact, self.orc = eng, exact, orc

    def set(self, tensors):
        for n, a in tensors.items():
            self.eng.set_tensor(n, a)
            self.exact.set_tensor(n, a)
            self.orc.set_tensor(n, a)
        self.eng.finalize()
        self.exact.finalize()

    def close(self):
        self.eng.close()
        self.exact.close()
        self.orc.close()


# ---------------------------------------------------------------- tiny config

def _tiny_weights():
    ocfg = qo.config_tiny()
    w0 = calibrate_codec(qo.random_weights(ocfg, 0), ocfg)      # bf16-origin
    return ocfg, w0, cs.fp32_codec_weights(w0, FP32_SEED)


def _tiny_trio(ocfg, w, max_batch=2, max_ctx=192):
    import q3tts
    eng = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=max_batch, max_ctx=max_ctx)
    exact = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=1, max_ctx=max_ctx, flags=q3tts.FLAG_FP32_CODEC)
    eng.load(w)
    exact.load(w)
    return Trio(eng, exact, qo.Oracle(ocfg, max_ctx=max_ctx, weights=w))


@pytest.fixture(scope="module")
def tiny32():
    ocfg, w0, w = _tiny_weights()
    t = _tiny_trio(ocfg, w)
    yield t, w0, w
    t.close()


@pytest.mark.parametrize("F", [1, 2, 5, 17, 40, 130])
def test_tiny_all_classes_fp32(tiny32, F):
    """The frame counts of test_gpu_codec.py::test_codec_vs_oracle (64-row tiles, the 4-token attention window, transposed-conv phase
    boundaries).  Every planes tensor counts as three-product."""
    t, _, w = tiny32
    n = cs.n_planes(cs.planes_names(w.keys()))
    assert n == 45 and t.eng.codec_plane_stats() == (0, n)
    assert t.exact.codec_plane_stats() == (0, 0)                 # the exact-fp32 engine keeps no planes
    _measure("tiny, all classes fp32-origin", t.eng, t.exact, t.orc, _codes(t.eng.cfg, F))


def _one_class_at_a_time(t, w0, w, codes, label, expect_all):
    names = list(w0.keys())
    total = cs.n_planes(cs.planes_names(names))
    try:
        for cls in cs.PLANE_CLASSES:
            members = cs.class_names(names, cls)
            wc = cs.with_class(w0, w, cls)
            t.set({n: wc[n] for n in cs.planes_names(names)})
            k = cs.n_planes(members)
            assert k == expect_all[cls], (cls, k)
            assert t.eng.codec_plane_stats() == (total - k, k), (cls, t.eng.codec_plane_stats())
            err, sig, pcm, ref = _measure("%s, only %s fp32-origin" % (label, cls), t.eng, t.exact, t.orc, codes)
            # the inputs discriminate: the reference itself moves by >= 10 x the bound when this class (the part of it that runs
            # k_conv_split) loses its lo plane
            dropped = cs.map_planes(wc, cs.routed(wc, members), cs.drop_lo)
            for n in members:
                t.orc.set_tensor(n, dropped[n])
            d = cs.rms(t.orc.vocoder(codes) - ref)
            print("%s, %s: lo plane dropped -> oracle PCM moves by %.3g = %.1f x the bound" % (label, cls, d, d / cs.bound_for(sig)))
            assert d >= 10.0 * cs.bound_for(sig), (cls, d, sig)
    finally:
        t.set({n: w[n] for n in cs.planes_names(names)})


def test_tiny_one_class_fp32_at_a_time(tiny32):
    t, w0, w = tiny32
    _one_class_at_a_time(t, w0, w, _codes(t.eng.cfg, 40), "tiny",
                         dict(attention=4, mlp=6, up=6, conv_in=1, block_tconv=4, res_conv1=12, res_conv2=12))


def _edge_variants(a, rng):
    """(label, tensor) for the dynamic-range sweep: every element except sixteen (the largest among them, so amax stays) x 2^-r"""
    keep = np.zeros(a.size, bool)
    keep[rng.choice(a.size, 15, replace=False)] = True
    keep[int(np.abs(a).argmax())] = True
    assert 15 <= keep.sum() <= 16
    keep = keep.reshape(a.shape)
    return [(r, np.where(keep, a, a * np.float32(2.0 ** -r)).astype(np.float32)) for r in (4, 8, 12, 16, 20)]


def _prescale_edges(t, w, name, codes, label, zero_and_tiny=True):
    """6 (a) all zeros, (b) x 2^-120 (k = 12 - e > 127: an unbounded 2^k is inf), (c) a wide dynamic range inside the tensor"""
    names = cs.planes_names(w.keys())
    n3 = cs.n_planes(names)
    base, sig0, _, ref0 = _measure("%s, unmodified" % label, t.eng, t.exact, t.orc, codes)
    try:
        if zero_and_tiny:
            t.set({name: np.zeros_like(w[name])})
            assert t.eng.codec_plane_stats() == (1, n3 - 1)                    # k = 0, both planes zero
            _, _, _, ref_z = _measure("%s, %s all zeros" % (label, name), t.eng, t.exact, t.orc, codes)
            t.set({name: (w[name] * np.float32(2.0 ** -120)).astype(np.float32)})
            assert cs.split_model(w[name] * np.float32(2.0 ** -120))[0] > 127
            assert t.eng.codec_plane_stats() == (0, n3)
            _, _, pcm_t, ref_t = _measure("%s, %s x 2^-120" % (label, name), t.eng, t.exact, t.orc, codes)
            assert float(np.abs(ref_t - ref_z).max()) <= 1e-6 and cs.rms(ref0 - ref_z) > 1e-3 * sig0
        rows = []
        for r, a in _edge_variants(w[name], np.random.default_rng(7)):
            assert np.abs(a).max() == np.abs(w[name]).max()
            t.set({name: a})
            assert t.eng.codec_plane_stats() == (0, n3)
            pcm, ref = t.eng.codec_decode(codes), t.orc.vocoder(codes)
            err32 = cs.rms(t.exact.codec_decode(codes) - ref)
            # the model: the oracle on the weights the planes hold, (hi + lo) 2^-k, for every tensor that runs k_conv_split
            wr = dict(w)
            wr[name] = a
            routed = cs.routed(wr, names)
            rec = cs.map_planes(wr, routed, cs.reconstruct)
            for n in routed:
                t.orc.set_tensor(n, rec[n])
            model = cs.rms(t.orc.vocoder(codes) - ref)
            for n in routed:
                t.orc.set_tensor(n, wr[n])
            err, sig = cs.rms(pcm - ref), cs.rms(ref)
            rows.append((r, model, err, err32, sig))
            print("%s, %s: all but 16 elements x 2^-%d: model error %.3g, split-fp16 error %.3g, exact-fp32 error %.3g, signal rms %.3g"
                  % (label, name, r, model, err, err32, sig))
        for r, model, err, err32, sig in rows:
            assert np.isfinite(err) and sig > cs.MIN_SIGNAL
            assert err <= 4.0 * model + base, (name, r, err, model, base)
    finally:
        t.set({name: w[name]})


def test_tiny_prescale_edges_residual_conv1(tiny32):
    t, _, w = tiny32
    assert cs.on_split_route(RES1_TINY, w[RES1_TINY].shape)
    _prescale_edges(t, w, RES1_TINY, _codes(t.eng.cfg, EDGE_FRAMES), "tiny")


def test_tiny_dynamic_range_down_proj(tiny32):
    """The tiny MLP is 48 wide, so its down_proj (C_in = 48) runs the fp32 kernel and its planes are never read: the sweep passes
    there by construction.  test_full_size_prescale_edges covers a down_proj that takes the projection route."""
    t, _, w = tiny32
    assert not cs.on_split_route(DOWN_TINY, w[DOWN_TINY].shape)
    _prescale_edges(t, w, DOWN_TINY, _codes(t.eng.cfg, EDGE_FRAMES), "tiny", zero_and_tiny=False)


def test_tiny_weight_file_round_trip(tiny32, tmp_path):
    """save_weights / load_weights keep every cd.* tensor bit for bit, so the loaded engine takes the same three-product route."""
    import q3tts
    t, _, w = tiny32
    path = str(tmp_path / "fp32.q3w")
    t.eng.save_weights(path)
    e2 = q3tts.Engine(t.eng.cfg, device=0, max_batch=1, max_ctx=192)
    try:
        e2.load_weights(path)
        for n, a in w.items():
            if n.startswith("cd."):
                assert np.array_equal(e2.get_tensor(n, a.shape).view(np.uint32), np.ascontiguousarray(a, np.float32).view(np.uint32)), n
        assert e2.codec_plane_stats() == t.eng.codec_plane_stats() == (0, 45)
        codes = _codes(t.eng.cfg, 17)
        err, sig, pcm, _ = _measure("tiny, engine loaded from a weight file", e2, None, t.orc, codes)
        assert np.array_equal(pcm, t.eng.codec_decode(codes))
    finally:
        e2.close()


def _entry_points(eng, orc, F, batch_caps, gen_frames, label):
    """Every way into the vocoder against the one-shot decode, at the tolerance of its bf16-weight twin (tests/test_gpu_codec.py,
    tests/test_gpu_full.py, tests/test_gpu_codec_stress.py: 2e-5 worst sample; the device-pointer entry bit for bit), and the one-shot
    decode against the oracle."""
    import q3tts
    cfg = eng.cfg
    codes = _codes(cfg, F, seed=1000 + F)
    err, sig, whole, ref = _measure("%s, one-shot decode" % label, eng, None, orc, codes)
    out = {}
    for chunk in (16, 25):
        out["chunked by %d, full history" % chunk] = eng.codec_decode_chunked(codes, chunk, left_context=F)
    for push in (25, 1):
        n = F if push > 1 else min(F, 30)
        sid = eng.codec_stream_begin(n)
        got = np.concatenate([eng.codec_stream_push(sid, codes[a:a + push]) for a in range(0, n, push)])
        eng.codec_stream_end(sid)
        out["stream pushes of %d" % push] = got
    for tag, got in out.items():
        want = whole[: got.size]
        assert got.size in (whole.size, eng.codec_decode_len(30)), tag
        d = float(np.abs(got - want).max())
        print("%s, %s: max |it - one-shot| %.3g" % (label, tag, d))
        assert d < 2e-5, (tag, d)
        if got.size == whole.size:
            cs.check_bound(cs.rms(got - ref), sig)
    # a ragged job: batched blocks and singles
    rng = np.random.default_rng(77)
    job = [rng.integers(0, cfg.cd_codebook, (f, cfg.n_groups)).astype(np.int64) for f in batch_caps]
    pcm = eng.codec_decode_batch(job)
    worst = 0.0
    for u, c in enumerate(job):
        alone = eng.codec_decode(c)
        assert pcm[u].shape == alone.shape == (eng.codec_decode_len(c.shape[0]),), u
        worst = max(worst, float(np.abs(pcm[u] - alone).max()))
    longest = int(np.argmax(batch_caps))
    rj = orc.vocoder(job[longest])
    cs.check_bound(cs.rms(pcm[longest] - rj), cs.rms(rj))
    small = int(np.argmin([abs(f - 8) for f in batch_caps]))            # a member of the small batched block
    rs = orc.vocoder(job[small])
    cs.check_bound(cs.rms(pcm[small] - rs), cs.rms(rs))
    print("%s, codec_decode_batch of %s frames: max |job - alone| %.3g" % (label, list(batch_caps), worst))
    assert worst < 2e-5, worst
    # device-resident codes and PCM
    hip = Hip()
    try:
        n = whole.size
        codes_d, pcm_d = hip.put(codes.astype(np.int32)), hip.put(np.full(n + 16, 7.0, np.float32))
        assert eng.codec_decode_dev(codes_d, F, pcm_d, n) == n and eng.stream is not None
        got = hip.get(pcm_d, (n + 16,), np.float32)
        assert np.array_equal(got[:n], whole) and (got[n:] == 7.0).all()
    finally:
        hip.free()
    # a slot's own codes after a short greedy generation
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=gen_frames)
    prompt, trailing = eng.build_prompt(frame_tokens([9, 8, 7, 6, 5]), 0)
    eng.slot_release(0)
    eng.slot_begin(0, prompt, trailing, sp, seed=5, stream_id=0, ignore_eos=True)
    eng.decode_steps(gen_frames)
    assert eng.slot_status(0)[0] == gen_frames
    got, gc = eng.slot_codec_decode(0), eng.slot_codes(0)
    eng.slot_release(0)
    alone = eng.codec_decode(gc)
    d = float(np.abs(got - alone).max())
    rg = orc.vocoder(gc)
    print("%s, slot_codec_decode after %d greedy frames: max |it - one-shot| %.3g, rms vs oracle %.3g" % (label, gen_frames, d, cs.rms(got - rg)))
    assert got.shape == alone.shape and d < 2e-5, d
    cs.check_bound(cs.rms(got - rg), cs.rms(rg))


def test_tiny_every_entry_point(tiny32):
    t, _, _ = tiny32
    _entry_points(t.eng, t.orc, 50, (40, 9, 2, 8, 6, 38), 12, "tiny")


# ---------------------------------------------------------------- 0.6B dims

def _full_cd_tensors(eng):
    return {n: eng.get_tensor(n, s) for n, s in eng.tensor_infos() if n.startswith("cd.")}


def _full_trio(make_w0):
    """Split engine, exact-fp32 engine and oracle at 0.6B dims.  The engines' own synthetic fill supplies the talker / predictor / text
    stacks; the cd.* tensors are make_w0(engine) (bf16-origin) with their matrices given a full fp32 mantissa."""
    import q3tts
    cfg = q3tts.default_config("0.6b")
    eng = q3tts.Engine(cfg, device=0, max_batch=2, max_ctx=512)
    exact = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=512, flags=q3tts.FLAG_FP32_CODEC)
    eng.fill_synthetic(seed=0)
    exact.fill_synthetic(seed=0)
    assert eng.codec_plane_stats() == (75, 0)
    w0 = make_w0(eng)
    assert set(w0) == {n for n, _ in eng.tensor_infos() if n.startswith("cd.")}
    w = cs.fp32_codec_weights(w0, FP32_SEED)
    t = Trio(eng, exact, qo.Oracle(to_ocfg(cfg), max_ctx=16))
    t.set(w)
    assert all(cs.on_split_route(n, w[n].shape) for n in cs.planes_names(w.keys()))
    assert t.eng.codec_plane_stats() == (0, 75)
    return t, w0, w


@pytest.fixture(scope="module")
def full_syn():
    """The engine's synthetic fill read back (the pattern of tests/test_gpu_full.py: the oracle gets what the engine holds)."""
    t, w0, w = _full_trio(_full_cd_tensors)
    yield t, w0, w
    t.close()


@pytest.fixture(scope="module")
def full32():
    """Random codec weights of the oracle's recipe (codec_split_ref.full_size_codec_weights): a network whose PCM reacts to a dropped
    lo plane by 40 - 120 x the bound (tests/test_cpu_codec_split.py), where the synthetic fill reacts by 1.3 x."""
    t, w0, w = _full_trio(lambda eng: cs.full_size_codec_weights(0)[1])
    yield t, w0, w
    t.close()


def _drop_all(t, w, codes, ref):
    names = cs.planes_names(w.keys())
    dropped = cs.map_planes(w, names, cs.drop_lo)
    try:
        for n in names:
            t.orc.set_tensor(n, dropped[n])
        return cs.rms(t.orc.vocoder(codes) - ref)
    finally:
        for n in names:
            t.orc.set_tensor(n, w[n])


@pytest.mark.parametrize("F", [24, 300])
def test_full_size_all_classes_fp32(full32, F):
    """24 frames: the 256-row tiles and the split-K pre-transformer GEMMs; 300 frames: the sliding window active on most rows, the large-F
    tile shapes, more than 256 row tiles per conv.  All 75 plane pairs three-product.  The condition on the inputs: with every lo plane
    dropped the oracle's own PCM moves by >= 10 x the bound."""
    t, _, w = full32
    assert t.eng.codec_plane_stats() == (0, 75)
    codes = _codes(t.eng.cfg, F)
    err, sig, pcm, ref = _measure("0.6B dims, random weights, all classes fp32-origin", t.eng, t.exact, t.orc, codes)
    tail = slice(-1920 * 8, None)
    assert cs.rms(pcm[tail] - ref[tail]) < cs.RMS_BOUND
    d = _drop_all(t, w, codes, ref)
    print("0.6B dims, random weights, %d frames: every lo plane dropped -> oracle PCM moves by %.3g = %.1f x the bound" % (F, d, d / cs.bound_for(sig)))
    assert d >= 10.0 * cs.bound_for(sig), (d, sig)


@pytest.mark.parametrize("F", [24, 300])
def test_full_size_synthetic_fill_all_classes_fp32(full_syn, F):
    """The same on the engine's synthetic fill (seed 0) read back and given a full fp32 mantissa — the weights every other full-size test
    and the benchmark use.  Correctness at the project's bound and the three-product count are asserted; these inputs by themselves
    discriminate little (every lo plane dropped moves the oracle's PCM by 9.5e-5 at 24 frames and 8.9e-5 at 300, 1.3 x and 1.2 x the
    bound 2e-3 x 0.037; printed), which is why the cases above exist."""
    t, _, w = full_syn
    assert t.eng.codec_plane_stats() == (0, 75)
    codes = _codes(t.eng.cfg, F)
    err, sig, pcm, ref = _measure("0.6B dims, synthetic fill, all classes fp32-origin", t.eng, t.exact, t.orc, codes)
    tail = slice(-1920 * 8, None)
    assert cs.rms(pcm[tail] - ref[tail]) < cs.RMS_BOUND
    d = _drop_all(t, w, codes, ref)
    print("0.6B dims, synthetic fill, %d frames: every lo plane dropped -> oracle PCM moves by %.3g = %.1f x the bound" % (F, d, d / cs.bound_for(sig)))


def test_full_size_one_class_fp32_at_a_time(full32):
    """res_conv1 alone gives the fused 96-channel unit (conv1 three-product, conv2 exact in fp16), res_conv2 alone the opposite: both
    must take the three-product fused kernel (ConvKArgs::wlo mixes the two convs' flags) and be right."""
    t, w0, w = full32
    _one_class_at_a_time(t, w0, w, _codes(t.eng.cfg, 24), "0.6B dims",
                         dict(attention=16, mlp=24, up=6, conv_in=1, block_tconv=4, res_conv1=12, res_conv2=12))
    assert t.eng.codec_plane_stats() == (0, 75)


def test_full_size_every_entry_point(full_syn):
    """On the synthetic fill with fp32-origin cd.* tensors, the weights of the bf16 twins whose tolerances are used.  Against the
    one-shot decode these inputs do discriminate: a lo plane ignored by one entry point alone would move its PCM by ~9e-5 rms, the
    tolerance is 2e-5 on the worst sample.  (The random network of full32 amplifies fp32 summation order to 1.3e-4 between two
    tilings of the same decode — its one-shot decode is itself 2.4e-4 from the oracle on the worst sample — so the twins'
    tolerance says nothing there.)"""
    t, _, w = full_syn
    assert t.eng.codec_plane_stats() == (0, 75)
    _entry_points(t.eng, t.orc, 100, (40, 9, 2, 8, 6, 38), 12, "0.6B dims, synthetic fill")


@pytest.mark.parametrize("name", [RES1_FULL, DOWN_FULL])
def test_full_size_prescale_edges(full32, name):
    """The pre-scale edges where every tensor is on the split route: a first conv of the fused 96-channel unit, and a pre-transformer
    down_proj (3072 -> 1024: the split-K slabs at 24 frames)."""
    t, _, w = full32
    _prescale_edges(t, w, name, _codes(t.eng.cfg, 24, seed=61), "0.6B dims")


# ---------------------------------------------------------------- the A/B knob

_CHILD_3PRODUCT = r"""
import sys, hashlib
import numpy as np
sys.path.insert(0, sys.argv[1])
import q3tts
cfg = q3tts.default_config("0.6b")
eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=128, flags=q3tts.FLAG_TEST_HOOKS)   # A/B knobs are honoured only by hook-enabled engines
eng.fill_synthetic(seed=5)
assert eng.codec_plane_stats() == (75, 0)          # bf16-origin: every lo plane is zero
out = {}
for F in (9, 70):
    codes = np.random.default_rng(F).integers(0, cfg.cd_codebook, (F, cfg.n_groups)).astype(np.int64)
    out["f%d" % F] = eng.codec_decode(codes)
np.savez(sys.argv[2], **out)
"""


def test_three_product_knob_on_zero_lo_planes_is_bit_identical(tmp_path):
    """Q3TTS_CONV_3PRODUCT=1 sends bf16-origin weights through the three-product kernels.  The extra product multiplies an all-zero
    plane, so every fp32 accumulator receives + 0 and keeps its value: the PCM equals the default's bit for bit (0.6B dims, the frame
    counts of test_conv_ab_switches_reproduce_the_default_bit_for_bit).  Child processes: the knob is read once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "leaxer-qwen3-tts_amd")

    def run(tag, extra):
        env = dict(os.environ)
        env.update(extra)
        path = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", _CHILD_3PRODUCT, pkg, path], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.load(path)

    base, forced = run("base", {}), run("forced", {"Q3TTS_CONV_3PRODUCT": "1"})
    for k in ("f9", "f70"):
        assert np.isfinite(base[k]).all() and cs.rms(base[k]) > 1e-6
        d = float(np.abs(forced[k] - base[k]).max())
        print("Q3TTS_CONV_3PRODUCT=1 on bf16-origin weights, %s: max |forced - default| %.3g" % (k, d))
        assert np.array_equal(forced[k], base[k]), (k, d)
