"""numpy restatement of the 12 Hz speech tokenizer's encoder (transformers MimiModel.encode, the first n_groups quantizers) — the
checker between the HIP encoder and the transformers golden (tests/golden/hf_mimi_encoder.npz).  fp64 by default.

Weights: {registry name without "enc.": array} in torch layouts (Conv1d [out][in][k], Linear [out][in]); cfg: a dict (or q3tts.Config)
with the enc_* fields and n_groups.  Rows are time-major [T][C] throughout."""
import math

import numpy as np


def cfg_dict(cfg):
    if isinstance(cfg, dict):
        return cfg
    d = cfg.to_dict()
    return d


def clip(n, seed):
    """The tests' input clips: an FM tone plus noise, from a seeded formula (never stored).  float32, n samples at 24 kHz."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n, dtype=np.float64) / 24000.0
    f0 = 180.0 + 40.0 * seed
    x = 0.4 * np.sin(2 * np.pi * f0 * t + 3.0 * np.sin(2 * np.pi * 3.0 * t)) + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32)


def frame_samples(cfg):
    cfg = cfg_dict(cfg)
    return 2 * int(np.prod(cfg["enc_ratios"][: cfg["enc_n_ratios"]]))


def encode_len(cfg, n):
    cfg = cfg_dict(cfg)
    T = n
    for r in cfg["enc_ratios"][: cfg["enc_n_ratios"]]:
        T = -(-T // r)
    return -(-T // 2)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def conv1d(x, w, b=None, stride=1, dil=1, replicate=False):
    """MimiConv1d, causal: left pad (k - 1) dil + 1 - stride, right pad just enough to complete the last output."""
    T, k = x.shape[0], w.shape[2]
    keff = (k - 1) * dil + 1
    padl = keff - stride
    T_out = -(-T // stride)
    padr = max((T_out - 1) * stride + keff - padl - T, 0)
    xp = np.pad(x, ((padl, padr), (0, 0)), mode="edge" if replicate else "constant")
    idx = np.arange(T_out) * stride
    out = np.zeros((T_out, w.shape[0]), x.dtype)
    for tap in range(k):
        out += xp[idx + tap * dil] @ w[:, :, tap].T
    return out if b is None else out + b


def layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    return (0.5 * x * (1.0 + _erf(x.astype(np.float64) / math.sqrt(2.0)))).astype(x.dtype)


def transformer(w, cfg, x):
    cfg = cfg_dict(cfg)
    nh, d, win = cfg["enc_heads"], cfg["enc_head_dim"], cfg["enc_window"]
    T = x.shape[0]
    pos = np.arange(T, dtype=np.float64)
    inv = 1.0 / (float(cfg["enc_rope_theta"]) ** (np.arange(0, d, 2, dtype=np.float64) / d))
    ang = pos[:, None] * inv[None]
    cos, sin = np.cos(ang).astype(x.dtype), np.sin(ang).astype(x.dtype)

    def rope(v):   # [T][nh][d], rotate-half
        a, b = v[..., : d // 2], v[..., d // 2:]
        return np.concatenate([a * cos[:, None] - b * sin[:, None], b * cos[:, None] + a * sin[:, None]], -1)

    i, j = np.arange(T)[:, None], np.arange(T)[None]
    mask = (j <= i) & (i - j < win)
    eps = float(cfg["enc_norm_eps"])
    for l in range(cfg["enc_layers"]):
        p = "layers.%d." % l
        h = layernorm(x, w[p + "input_norm.w"], w[p + "input_norm.b"], eps)
        q = rope((h @ w[p + "q_proj"].T).reshape(T, nh, d))
        k = rope((h @ w[p + "k_proj"].T).reshape(T, nh, d))
        v = (h @ w[p + "v_proj"].T).reshape(T, nh, d)
        s = np.einsum("ihd,jhd->hij", q, k) / math.sqrt(d)
        s = np.where(mask[None], s, -np.inf)
        s = np.exp(s - s.max(-1, keepdims=True))
        s = s / s.sum(-1, keepdims=True)
        a = np.einsum("hij,jhd->ihd", s, v).reshape(T, nh * d)
        x = x + w[p + "attn_scale"] * (a @ w[p + "o_proj"].T)
        h = layernorm(x, w[p + "post_norm.w"], w[p + "post_norm.b"], eps)
        x = x + w[p + "mlp_scale"] * (gelu(h @ w[p + "fc1"].T) @ w[p + "fc2"].T)
    return x


def latents(w, cfg, pcm, dtype=np.float64):
    """pcm [n] at 24 kHz -> the rows the quantiser sees, [F][enc_hidden]"""
    cfg = cfg_dict(cfg)
    w = {k: np.asarray(v, dtype) for k, v in w.items()}
    x = np.asarray(pcm, dtype).reshape(-1, 1)
    x = conv1d(x, w["conv_in.w"], w["conv_in.b"])
    for s in range(cfg["enc_n_ratios"]):
        p = "stages.%d." % s
        h = conv1d(elu(x), w[p + "res.conv1.w"], w[p + "res.conv1.b"])
        x = x + conv1d(elu(h), w[p + "res.conv2.w"], w[p + "res.conv2.b"])
        x = conv1d(elu(x), w[p + "down.w"], w[p + "down.b"], stride=cfg["enc_ratios"][s])
    x = conv1d(elu(x), w["conv_out.w"], w["conv_out.b"])
    x = transformer(w, cfg, x)
    return conv1d(x, w["downsample.w"], None, stride=2, replicate=True)


def quantize(w, cfg, lat, dtype=np.float64):
    """-> (codes [F][G] int64, gaps [F][G]): per decision the relative top-2 distance gap (d2 - d1) / d1 of squared distances"""
    cfg = cfg_dict(cfg)
    G = cfg["n_groups"]
    lat = np.asarray(lat, dtype)
    F = lat.shape[0]
    codes, gaps = np.zeros((F, G), np.int64), np.zeros((F, G), np.float64)
    res = {"sem": lat @ np.asarray(w["vq.sem.in_proj"], dtype).T, "ac": lat @ np.asarray(w["vq.ac.in_proj"], dtype).T}
    for g in range(G):
        key = "sem" if g == 0 else "ac"
        E = np.asarray(w["vq.codebook.%d" % g], dtype)
        d = ((res[key][:, None, :] - E[None]) ** 2).sum(-1)
        idx = d.argmin(-1)
        codes[:, g] = idx
        if E.shape[0] > 1:
            two = np.partition(d, 1, axis=-1)[:, :2]
            gaps[:, g] = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 0], 1e-300)
        else:
            gaps[:, g] = np.inf
        res[key] = res[key] - E[idx]
    return codes, gaps


def encode(w, cfg, pcm, dtype=np.float64):
    lat = latents(w, cfg, pcm, dtype)
    codes, gaps = quantize(w, cfg, lat, dtype)
    return lat, codes, gaps


def check_codes(got, ref, gaps, gate, max_excused_frac=0.10):
    """Margin-aware comparison, like the greedy tests: per frame walk the codebooks in order; the first mismatch passes only if the
    checker's relative gap at that decision is under `gate`, and then excuses the rest of that frame.  Returns the excused frames;
    raises on a mismatch at a comfortable margin or when more than max_excused_frac of the frames are excused."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    excused = []
    for f in range(ref.shape[0]):
        for g in range(ref.shape[1]):
            if got[f, g] != ref[f, g]:
                assert gaps[f, g] < gate, "frame %d codebook %d: got %d, reference %d at relative gap %.3e (gate %.1e)" % (
                    f, g, got[f, g], ref[f, g], gaps[f, g], gate)
                excused.append(f)
                break
    limit = max_excused_frac * ref.shape[0]
    assert len(excused) <= limit, "%d of %d frames excused (limit %.1f)" % (len(excused), ref.shape[0], limit)
    return excused
