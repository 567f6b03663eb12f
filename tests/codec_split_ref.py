"""Reference side of the codec decoder's split-precision weight planes (csrc/q3_codec.cpp, Engine::finalize_codec): plain numpy
restatements of the finalize split, weights that carry a full fp32 mantissa (what an imported checkpoint's cd.* tensors are), and
the groups of tensors that share a kernel route.  No GPU, no engine: tests/test_cpu_codec_split.py and
tests/test_gpu_codec_fp32_weights.py both build on it."""
import re

import numpy as np

# the bound every oracle comparison of the codec uses (tests/test_gpu_full.py::test_codec_full_size, north_star)
RMS_BOUND = 1e-4
REL_BOUND = 2e-3
MIN_SIGNAL = 1e-3


def fp32_codec_weights(w, seed):
    """Copy of `w` where every cd.* tensor with >= 2 dimensions is multiplied elementwise by 1 + U(-2^-9, 2^-9) in fp32: same scale,
    full fp32 mantissa.  Everything outside cd.* is the same array as in `w`."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, a in w.items():
        a = np.asarray(a)
        if name.startswith("cd.") and a.ndim >= 2:
            f = np.float32(1.0) + rng.uniform(-2.0 ** -9, 2.0 ** -9, a.shape).astype(np.float32)
            out[name] = (a.astype(np.float32) * f).astype(np.float32)
        else:
            out[name] = a
    return out


def split_model(a):
    """The finalize split of one tensor: amax, k = 12 - (frexp exponent of amax) so that amax * 2^k lies in [2^11, 2^12),
    hi = fp16(a * 2^k), lo = fp16(a * 2^k - hi).  numpy's float16 conversion is round-to-nearest-even with subnormals, like the
    device's.  k is what the arithmetic asks for, unbounded: a scale that fp32 cannot hold (k > 127) is the caller's finding.
    Returns (k, hi, lo), hi and lo as float16."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    amax = float(np.abs(a).max()) if a.size else 0.0
    k = 0
    if amax > 0.0 and np.isfinite(amax):
        k = 12 - int(np.frexp(np.float32(amax))[1])
    x = np.ldexp(a.astype(np.float64), k)                 # exact: a power of two, in double
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float64)).astype(np.float16)   # the difference is exact in fp32, hence in double
    return k, hi, lo


def reconstruct(a):
    """(hi + lo) * 2^-k in fp32: the weights the three-product kernels multiply by."""
    k, hi, lo = split_model(a)
    return np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), -k).astype(np.float32).reshape(np.shape(a))


def drop_lo(a):
    """hi * 2^-k in fp32: what a kernel that ignored the lo plane would multiply by."""
    k, hi, _ = split_model(a)
    return np.ldexp(hi.astype(np.float64), -k).astype(np.float32).reshape(np.shape(a))


# Groups of weight tensors that share a kernel route.  cd.dec.conv_out has no planes (scalar fp32 kernel) and is in no class.
PLANE_CLASSES = {
    "attention": r"cd\.layers\.\d+\.[qkvo]_proj$",                     # pre-transformer: fused q/k/v projection and o_proj
    "mlp": r"cd\.layers\.\d+\.(gate|up|down)_proj$",                   # pre-transformer MLP
    "up": r"cd\.up\.\d+\.(tconv|cnx\.pw1|cnx\.pw2)\.w$",                # upsampling stages: transposed conv + the two pointwise convs
    "conv_in": r"cd\.dec\.conv_in\.w$",
    "block_tconv": r"cd\.dec\.blocks\.\d+\.tconv\.w$",
    "res_conv1": r"cd\.dec\.blocks\.\d+\.res\.\d+\.conv1\.w$",         # 7 taps
    "res_conv2": r"cd\.dec\.blocks\.\d+\.res\.\d+\.conv2\.w$",         # 1x1; behind conv1 in the fused 96-channel unit
}


def class_names(names, cls):
    pat = re.compile(PLANE_CLASSES[cls])
    return [n for n in names if pat.match(n)]


def planes_names(names):
    """Every tensor name of `names` that the engine splits into planes."""
    return [n for n in names if any(re.match(p, n) for p in PLANE_CLASSES.values())]


def on_split_route(name, shape):
    """Does a conv / projection with this weight run k_conv_split (launch_conv in csrc/q3_codec_kernels.hip: C_in a multiple of 32, at
    least 32 output channels, a multiple of 4)?  Narrower ones run the fp32 matrix-core kernel on the fp32 weights and never read
    their planes — most of the tiny config's decoder (64 -> 4 channels) and its 48-wide MLP's down_proj; at 0.6B dims every
    tensor of PLANE_CLASSES is on the route.  Linear weights are [out][in], convs [out][in][k], transposed convs [in][out][k]."""
    if name.endswith("tconv.w"):
        cin, cout = shape[0], shape[1]
    else:
        cout, cin = shape[0], shape[1]
    return cin % 32 == 0 and cout >= 32 and cout % 4 == 0


def routed(w, names):
    return [n for n in names if on_split_route(n, w[n].shape)]


def n_planes(names):
    """How many plane pairs the engine keeps for the tensors `names` (Engine.codec_plane_stats counts these): one per tensor, except
    that a layer's q_proj, k_proj and v_proj are one fused tensor."""
    keys = set()
    for n in names:
        m = re.match(r"(cd\.layers\.\d+\.)[qkv]_proj$", n)
        keys.add(m.group(1) + "qkv" if m else n)
    return len(keys)


def with_class(base, fp32, cls):
    """`base` (bf16-origin) with the tensors of class `cls` taken from `fp32`."""
    w = dict(base)
    for n in class_names(base.keys(), cls):
        w[n] = fp32[n]
    return w


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def check_bound(err, sig):
    """The project's codec bound: RMS error < 1e-4 and < 2e-3 x signal RMS, the signal not silent."""
    assert sig > MIN_SIGNAL, ("silent reference", sig)
    assert err < RMS_BOUND and err < REL_BOUND * sig, (err, sig)


def bound_for(sig):
    return min(RMS_BOUND, REL_BOUND * sig)


def map_planes(w, names, fn):
    """Copy of `w` with fn (drop_lo or reconstruct) applied to the tensors `names`, each with the scale the engine would give it:
    a layer's q_proj, k_proj and v_proj share one (they are one tensor to the engine, rows q | k | v)."""
    out = dict(w)
    done = set()
    for n in names:
        m = re.match(r"(cd\.layers\.\d+\.)[qkv]_proj$", n)
        if not m:
            out[n] = fn(w[n])
            continue
        if m.group(1) in done:
            continue
        done.add(m.group(1))
        parts = [m.group(1) + p for p in ("q_proj", "k_proj", "v_proj")]
        fused = fn(np.concatenate([np.asarray(w[p], np.float32) for p in parts], axis=0))
        r = 0
        for p in parts:
            if p in names:
                out[p] = fused[r:r + w[p].shape[0]]
            r += w[p].shape[0]
    return out


def full_size_codec_weights(seed=0):
    """bf16-origin cd.* tensors at 0.6B dims by the recipe of q3_oracle.random_weights, the last conv calibrated to a PCM of 0.2 rms
    (the other stacks are not needed by the vocoder and stay zero in the oracle)."""
    import q3_oracle as qo
    from util import calibrate_codec
    cfg = qo.config_06b()
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape, kind in qo.tensor_specs(cfg):
        if not name.startswith("cd."):
            continue
        if kind == "w":
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            if name.endswith("tconv.w"):
                fan_in = shape[0] * max(1, shape[2] // 2) if shape[2] > 2 else shape[0]
            a = rng.standard_normal(shape, dtype=np.float32)
            if name != "cd.code_embed":
                a = a / np.float32(np.sqrt(fan_in))
        elif kind == "norm":
            a = 1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif kind == "b":
            a = 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif kind == "scale":
            a = 0.5 + 0.1 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.3 * rng.standard_normal(shape, dtype=np.float32)
        w[name] = qo.bf16_round(a)
    return cfg, calibrate_codec(w, cfg)
