"""The inputs of tests/test_gpu_codec_fp32_weights.py, judged without a GPU: fp32-origin codec weights do have a non-zero lo plane
(bf16-origin ones do not), and an engine that ignored that plane would be caught — the oracle's own PCM moves by at least 10 x the
bound the GPU tests assert when a class of tensors loses its lo plane.  Both are conditions on the inputs, computed from the
reference alone (oracle/q3_oracle.c, fp32)."""
import numpy as np
import pytest

import codec_split_ref as cs
import q3_oracle as qo
from util import calibrate_codec

FRAMES_TINY = 40
FRAMES_FULL = 24       # the short full-size case of the GPU tests
MARGIN = 10.0


@pytest.fixture(scope="module")
def tiny():
    cfg = qo.config_tiny()
    w0 = calibrate_codec(qo.random_weights(cfg, 0), cfg)          # bf16-origin
    w = cs.fp32_codec_weights(w0, 1)
    return cfg, w0, w


def _pcm(cfg, w, codes):
    o = qo.Oracle(cfg, max_ctx=16, weights=w)
    try:
        return o.vocoder(codes)
    finally:
        o.close()


def test_fp32_origin_weights_have_a_lo_plane_and_bf16_origin_ones_do_not(tiny):
    """hi + lo against a * 2^k.  Two 11-bit planes hold 22 bits: |a 2^k - hi| <= 2^-11 |a 2^k| (half an fp16 ulp), and the fp16
    rounding of that remainder loses at most 2^-11 of it, or half the subnormal step 2^-24 where the remainder is subnormal — so
    the error is at most max(2^-25, 2^-22 |a 2^k|).  For the elements below 2^-2 that is within the 2^-24 absolute resolution the
    kernel comment documents; the largest elements (2^11 .. 2^12) are resolved to 2^-12, i.e. to half an fp32 ulp."""
    cfg, w0, w = tiny
    names = cs.planes_names(w.keys())
    assert cs.n_planes(names) == 5 * cfg.cd_layers + 3 * cfg.cd_n_up + 1 + 7 * cfg.cd_n_blocks
    assert "cd.dec.conv_out.w" not in names
    for n in names:
        k, hi, lo = cs.split_model(w[n])
        x = np.ldexp(w[n].astype(np.float64), k)
        assert 2.0 ** 11 <= np.abs(x).max() < 2.0 ** 12, n
        assert np.any(lo != 0), n
        e = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x)
        assert (e <= np.maximum(2.0 ** -25, 2.0 ** -22 * np.abs(x))).all(), (n, float(e.max()))
        small = np.abs(x) <= 0.25
        assert (e[small] <= 2.0 ** -24).all(), n
        assert np.array_equal(cs.reconstruct(w[n]).astype(np.float64) * 2.0 ** k, hi.astype(np.float64) + lo.astype(np.float64)), n
        k0, hi0, lo0 = cs.split_model(w0[n])
        assert not np.any(lo0 != 0), n                                   # bf16-origin: exact in fp16 after the pre-scale
        assert np.array_equal(np.ldexp(hi0.astype(np.float64), -k0), w0[n].astype(np.float64)), n
        assert np.array_equal(cs.drop_lo(w0[n]), w0[n]), n
    # everything outside cd.* and every vector is untouched; the matrices keep their scale
    for n in w:
        if not n.startswith("cd.") or w[n].ndim < 2:
            assert w[n] is w0[n] or np.array_equal(w[n], w0[n]), n
        else:
            assert w[n].dtype == np.float32 and np.all(np.abs(w[n] - w0[n]) <= 2.0 ** -9 * np.abs(w0[n]) * (1 + 2.0 ** -20)), n


def _discrimination(cfg, w, codes, label):
    names = list(w.keys())
    full = _pcm(cfg, w, codes)
    sig = cs.rms(full)
    assert sig > cs.MIN_SIGNAL and np.abs(full).max() < 1.0, (sig, float(np.abs(full).max()))   # not silent, not clamped
    need = MARGIN * cs.bound_for(sig)
    rows = []
    for cls in list(cs.PLANE_CLASSES) + ["all"]:
        members = cs.routed(w, cs.planes_names(names) if cls == "all" else cs.class_names(names, cls))   # only what k_conv_split reads
        assert members, cls
        d = cs.rms(_pcm(cfg, cs.map_planes(w, members, cs.drop_lo), codes) - full)
        rows.append((cls, len(members), d))
        print("%s, %d frames, signal rms %.3g: lo plane of %-11s (%2d tensors) dropped -> oracle PCM moves by %.3g rms = %.1f x the bound %.3g"
              % (label, codes.shape[0], sig, cls, len(members), d, d / cs.bound_for(sig), cs.bound_for(sig)))
    for cls, _, d in rows:
        assert d >= need, (label, cls, d, need)


def test_dropping_a_class_lo_plane_moves_the_reference_by_10x_the_gpu_bound(tiny):
    """Tiny config, seed 0, 40 frames: per class of PLANE_CLASSES and for all of them together."""
    cfg, _, w = tiny
    codes = np.random.default_rng(40).integers(0, cfg.cd_codebook, (FRAMES_TINY, cfg.n_groups)).astype(np.int64)
    _discrimination(cfg, w, codes, "tiny")


def test_dropping_a_class_lo_plane_moves_the_reference_at_full_size():
    """The same at 0.6B dims (random codec weights of the oracle's recipe), at the 24 frames of the GPU file's short full-size case.
    The GPU file uses these same weights for its discriminating full-size cases and repeats the condition there, at 24 and 300 frames
    (the engine's own synthetic fill is a much tamer network: every lo plane dropped moves its PCM by only 1.3 x the bound)."""
    cfg, w0 = cs.full_size_codec_weights(0)
    w = cs.fp32_codec_weights(w0, 1)
    assert cs.n_planes(cs.planes_names(w.keys())) == 75
    codes = np.random.default_rng(24).integers(0, cfg.cd_codebook, (FRAMES_FULL, cfg.n_groups)).astype(np.int64)
    _discrimination(cfg, w, codes, "0.6B dims")


def test_a_tensor_below_2_pow_minus_115_asks_for_a_scale_fp32_cannot_hold(tiny):
    """One residual conv1 scaled by 2^-120: the split's k = 12 - e exceeds 127, so 2^k is not an fp32 number and an engine has to bound
    it.  What it must still compute is recorded here: the reference PCM is finite and equals, within 1e-6, the PCM with that tensor
    zeroed (the tensor contributes ~2^-120 of its usual share)."""
    cfg, _, w = tiny
    name = "cd.dec.blocks.1.res.1.conv1.w"
    tiny_w = dict(w)
    tiny_w[name] = (w[name] * np.float32(2.0 ** -120)).astype(np.float32)
    assert np.abs(tiny_w[name]).max() > 0
    k, hi, lo = cs.split_model(tiny_w[name])
    with np.errstate(over="ignore"):
        assert k > 127 and np.isinf(np.ldexp(np.float32(1.0), k))
    assert np.isfinite(hi.astype(np.float32)).all() and np.any(lo != 0)            # the model itself scales in double
    assert cs.split_model(np.zeros((4, 4, 7), np.float32))[0] == 0                  # an all-zero tensor: k = 0, planes of zeros
    zero_w = dict(w)
    zero_w[name] = np.zeros_like(w[name])
    codes = np.random.default_rng(6).integers(0, cfg.cd_codebook, (6, cfg.n_groups)).astype(np.int64)
    a, z, full = _pcm(cfg, tiny_w, codes), _pcm(cfg, zero_w, codes), _pcm(cfg, w, codes)
    assert np.isfinite(a).all() and np.isfinite(z).all()
    assert float(np.abs(a - z).max()) <= 1e-6
    assert cs.rms(full - z) > 1e-3                                             # the tensor matters at its ordinary scale
