"""Peaked-softmax inputs for the attention kernels, and a float64 restatement of the decoder stack to judge them by (helper, not a test).

Every other numerical test of the talker and predictor stacks runs unit norm gains on `randn * 0.05` rows: q and k are normalised per
head, so every score is about N(0, 1), no probability passes 0.1 and every `exp(m_old - m_new)` of an online softmax sits within e^+-3
of 1.  The builders here raise the q_norm gains (`peaked`) or plant a layer whose scores are known in closed form (`plant_layer0` +
`planted_rows`); `stack_forward64` restates `dec_forward` of oracle/q3_oracle.c in numpy float64 and reports, per (layer, head, row),
how peaked the softmax actually was, so a test can assert the condition it claims to run under before it compares anything."""
import functools

import numpy as np

import q3_oracle as qo

PROFILES = ("recency", "peak_at_0", "peak_at_mid", "oldest_first")
SCENARIOS = ("peaked4", "peaked16") + PROFILES
PLANT_GAIN = 4.0       # layer-0 q_norm gain of the planted scenarios: score span about 80
UPPER_GAIN = 8.0       # their layers >= 1


def bf16_round64(a):
    """float64 -> float32 -> bf16 (round to nearest even), back as float64: the rounding the bf16 KV cache applies on append"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def stack_dims(dims, prefix):
    """(n_layers, n_q_heads, n_kv_heads, head_dim, rope_theta, rms_eps) of the `talker.` / `cp.` stack"""
    c = dims
    if prefix == "talker.":
        return c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, float(c.rope_theta), float(c.rms_eps)
    assert prefix == "cp."
    return c.cp_layers, c.cp_heads, c.cp_kv_heads, c.cp_head_dim, float(c.cp_rope_theta), float(c.cp_rms_eps)


def stack_forward64(dims, weights, prefix, x, kv_bf16=False, step=0):
    """dec_forward (oracle/q3_oracle.c) over all rows of x at positions 0.., causal, in float64, then the final norm and the head
    (`talker.codec_head`, or `cp.head.{step}`).  -> (logits [T][V], last normalised hidden row [H], stats): stats["pmax" | "argmax" |
    "span"] are [layer][head][row] — the largest probability, its key position, and min(score) - max(score) over the row's visible
    keys; stats["hn"] holds every row's normalised hidden state."""
    L, nq, nkv, d, theta, eps = stack_dims(dims, prefix)
    W = lambda n: np.asarray(weights[prefix + n], np.float64)
    norm = lambda v, g: g * (v / np.sqrt((v * v).mean(-1, keepdims=True) + eps))
    x = np.asarray(x, np.float64)
    if prefix + "proj.w" in weights:
        x = x @ W("proj.w").T + W("proj.b")
    T, half = x.shape[0], d // 2
    ang = np.arange(T)[:, None] * theta ** (-2.0 * np.arange(half) / d)[None, :]
    cs, sn = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    rope = lambda v: np.concatenate([v[..., :half] * cs - v[..., half:] * sn, v[..., half:] * cs + v[..., :half] * sn], -1)   # rotate-half
    seen = np.tril(np.ones((T, T), bool))
    st = {k: np.zeros((L, nq, T), np.int64 if k == "argmax" else np.float64) for k in ("pmax", "argmax", "span")}
    for l in range(L):
        p = "layers.%d." % l
        h = norm(x, W(p + "input_norm"))
        q = rope(norm((h @ W(p + "q_proj").T).reshape(T, nq, d), W(p + "q_norm")))
        k = rope(norm((h @ W(p + "k_proj").T).reshape(T, nkv, d), W(p + "k_norm")))
        v = (h @ W(p + "v_proj").T).reshape(T, nkv, d)
        if kv_bf16:
            k, v = bf16_round64(k), bf16_round64(v)
        k, v = np.repeat(k, nq // nkv, 1), np.repeat(v, nq // nkv, 1)
        s = np.einsum("thd,shd->hts", q, k) / np.sqrt(d)
        mx = np.where(seen, s, -np.inf).max(-1)
        pr = np.where(seen, np.exp(np.minimum(s - mx[..., None], 0.0)), 0.0)
        pr /= pr.sum(-1, keepdims=True)
        st["pmax"][l], st["argmax"][l] = pr.max(-1), np.where(seen, s, -np.inf).argmax(-1)
        st["span"][l] = np.where(seen, s, np.inf).min(-1) - mx
        x = x + np.einsum("hts,shd->thd", pr, v).reshape(T, nq * d) @ W(p + "o_proj").T
        h = norm(x, W(p + "post_norm"))
        g = h @ W(p + "gate_proj").T
        x = x + (g / (1.0 + np.exp(-g)) * (h @ W(p + "up_proj").T)) @ W(p + "down_proj").T
    hn = norm(x, W("norm"))
    st["hn"] = hn
    return hn @ W("codec_head" if prefix == "talker." else "head.%d" % step).T, hn[-1], st


def config_2l():
    """0.6B talker and predictor dims (hidden 1024, 16 query / 8 KV heads of 128, ffn 3072, vocab 3072, 2048 sub-codes) cut to two
    layers each, a 512-row text table and config_tiny's codec and speaker encoder: head_dim 128, two query heads per KV head,
    nkv == 8 && nq == 16 and K % 128 == 0 are the gates of k_attn_stream, the per-KV-head o_proj, the fused predictor kernels and the
    MFMA path."""
    d = qo.config_tiny().to_dict()
    big = qo.config_06b().to_dict()
    for k in ("hidden", "n_heads", "n_kv_heads", "head_dim", "ffn", "vocab", "cp_heads", "cp_kv_heads", "cp_head_dim", "cp_ffn", "sub_vocab",
              "codec_eos", "suppress_begin", "suppress_end"):
        d[k] = big[k]
    d.update(n_layers=2, cp_layers=2, text_vocab=512, text_hidden=32, cd_codebook=2048, spk_enc_dim=1024)
    return qo.Config.from_dict(d)


def stack_names(cfg):
    """the tensors stack_forward64 reads, by qo.tensor_specs: both stacks, their final norms and heads"""
    return [(n, s, k) for n, s, k in qo.tensor_specs(cfg)
            if n.startswith(("talker.layers.", "cp.layers.", "cp.head.", "cp.proj.")) or n in ("talker.norm", "talker.codec_head", "cp.norm")]


@functools.lru_cache(maxsize=None)
def _base(which, seed):
    cfg = config_2l() if which == "2l" else qo.config_tiny()
    rng = np.random.default_rng(seed)
    w = {}
    for n, shape, kind in stack_names(cfg):
        w[n] = np.ones(shape, np.float32) if kind == "norm" else qo.bf16_round(rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02 if which == "2l" else shape[-1] ** -0.5))
    return cfg, w


def base_weights(which="2l", seed=0):
    """(config, {name: array}) of both stacks in the style of Engine.fill_synthetic: matrices N(0, 0.02^2) rounded to bf16, every norm
    gain 1 ("tiny": config_tiny with 1 / sqrt(fan_in) matrices).  Shared and cached: derive scenarios with peaked() / plant_layer0(),
    which copy what they change, and never write into the arrays."""
    cfg, w = _base(which, seed)
    return cfg, dict(w)


def peaked(weights, prefix, g, layers=None):
    """a copy of the dict with q_norm of every layer (or of `layers`) times g — exact in bf16 for powers of two; k_norm stays"""
    out = dict(weights)
    for n in weights:
        if n.startswith(prefix + "layers.") and n.endswith(".q_norm") and (layers is None or int(n.split(".")[2]) in layers):
            out[n] = weights[n] * np.float32(g)
    return out


def plant_layer0(weights, prefix):
    """a copy whose layer-0 q_proj / k_proj are zero but for two rows per head: dims half-1 and d-1 — the lowest-frequency RoPE pair,
    under 3e-4 rad over 200 positions at theta 1e6 — read input channels 0, 1 (q) and 2, 3 (k) with weight 1.  With planted_rows() the
    per-head RMSNorm leaves sqrt(d) * (cos, sin) in that pair, so query t scores sqrt(d) * q_gain * cos(a_t - b_s) on key s in every head."""
    out = dict(weights)
    d = weights[prefix + "layers.0.q_norm"].shape[0]
    for name, ch0 in (("q_proj", 0), ("k_proj", 2)):
        n = prefix + "layers.0." + name
        out[n] = _plant_matrix(weights[n].shape, d, ch0)
    return out


@functools.lru_cache(maxsize=None)
def _plant_matrix(shape, d, ch0):
    m = np.zeros(shape, np.float32)
    for h in range(shape[0] // d):
        m[h * d + d // 2 - 1, ch0] = 1.0
        m[h * d + d - 1, ch0 + 1] = 1.0
    return m


def planted_rows(T, profile, rng, H):
    """-> (rows [T][H], where [T]): `randn * 0.05` rows whose channels 0..3 carry (cos a_t, sin a_t, cos b_t, sin b_t), and the key
    position the profile gives the largest layer-0 score of query t (argmax over s <= t of cos(a_t - b_s)).
      recency       a_t = b_t = 2.5 t / T: scores rise with the key position, the newest key (self) is the maximum — every running max moves
      peak_at_0     a = 0, b_0 = 0, other b_s = 2.0 + 0.3 u: one key (the sink) holds all the mass, later splits' merge weights underflow
      peak_at_mid   the same with the peak at p = 70, inside the second 64-token split (p = T // 2 below 128 rows)
      oldest_first  a = 0, b_s = 2.5 s / T: the maximum is token 0 and scores fall monotonically"""
    x = (rng.standard_normal((T, H)) * 0.05).astype(np.float32)
    t = np.arange(T, dtype=np.float64)
    if profile == "recency":
        a = b = 2.5 * t / T
    elif profile == "oldest_first":
        a, b = np.zeros(T), 2.5 * t / T
    else:
        p = 0 if profile == "peak_at_0" else (70 if T >= 128 else T // 2)
        a, b = np.zeros(T), 2.0 + 0.3 * rng.random(T)
        b[p] = 0.0
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    c = np.where(np.tril(np.ones((T, T), bool)), np.cos(a[:, None] - b[None, :]), -np.inf)
    return x, c.argmax(-1)


def scenario(which, prefix, name, T, seed, twin=False):
    """-> (config, weights, rows [T][H], where or None): scenario `name` of SCENARIOS on the `prefix` stack of base_weights(which), T
    input rows drawn from `seed`; twin=True: the same rows and matrices with every q_norm gain back at 1 (the scenario's flat-softmax
    twin, the unit of the error bound)."""
    cfg, w = base_weights(which)
    rng = np.random.default_rng(seed)
    if name.startswith("peaked"):
        g = 1.0 if twin else float(name[6:])
        return cfg, peaked(w, prefix, g), (rng.standard_normal((T, cfg.hidden)) * 0.05).astype(np.float32), None
    x, where = planted_rows(T, name, rng, cfg.hidden)
    w = plant_layer0(w, prefix)
    if not twin:
        w = peaked(peaked(w, prefix, PLANT_GAIN, layers=(0,)), prefix, UPPER_GAIN, layers=range(1, 64))
    return cfg, w, x, where


def new_oracle(cfg, weights, max_ctx, kv_bf16=False):
    """an oracle holding the stack tensors of `weights` (its other tensors stay zero: only prefill / decode / code_predictor are run)"""
    orc = qo.Oracle(cfg, max_ctx=max_ctx, kv_bf16=kv_bf16)
    for n, _, _ in stack_names(cfg):
        orc.set_tensor(n, weights[n])
    return orc


@functools.lru_cache(maxsize=None)
def talker_case(which, name, T, seed, kv_bf16=False):
    """One talker scenario, computed once and shared: dict with the rows `x`, the weights `w`, float64 `logits` [T][V] and normalised
    rows `hn` [T][H], `stats`, `where`, and the oracle's own error against float64 on the scenario (`eo_g`) and on its gain-1 twin
    (`eo_1`): max |difference| over all T rows' logits (one prefill pass; bit-equal to teacher-forced decode in the oracle, whose
    per-row arithmetic does not depend on the pass shape) and the last hidden row."""
    out = {}
    for twin in (True, False):
        cfg, w, x, where = scenario(which, "talker.", name, T, seed, twin)
        lg, lh, st = stack_forward64(cfg, w, "talker.", x, kv_bf16)
        orc = new_oracle(cfg, w, T, kv_bf16)
        olg, olh = orc.prefill(x)
        orc.close()
        eo = max(float(np.abs(olg - lg).max()), float(np.abs(olh - lh).max()))
        assert np.isfinite(eo)
        out["eo_1" if twin else "eo_g"] = eo
    out.update(cfg=cfg, w=w, x=x, where=where, logits=lg, hn=st["hn"], stats=st)
    return out


@functools.lru_cache(maxsize=None)
def cp_case(name, seed, n_max=16):
    """One predictor scenario on config_2l: sequences seq[:n], n = 2..n_max, through code_predictor(seq[:n], step = n - 2).  float64
    `logits[n]` of the last row under head n - 2 (one causal pass: row n - 1 of the n_max-row pass is the n-row sequence's last row),
    `hn`, `stats`, and the oracle's error over the 15 calls on the scenario and its twin."""
    out = {}
    for twin in (True, False):
        cfg, w, x, where = scenario("2l", "cp.", name, n_max, seed, twin)
        _, _, st = stack_forward64(cfg, w, "cp.", x)
        lg = {n: st["hn"][n - 1] @ np.asarray(w["cp.head.%d" % (n - 2)], np.float64).T for n in range(2, n_max + 1)}
        orc = new_oracle(cfg, w, 16)
        eo = max(float(np.abs(orc.code_predictor(x[:n], n - 2) - lg[n]).max()) for n in lg)
        orc.close()
        assert np.isfinite(eo)
        out["eo_1" if twin else "eo_g"] = eo
    out.update(cfg=cfg, w=w, x=x, where=where, logits=lg, hn=st["hn"], stats=st)
    return out


def clear():
    """drop the cached weights and cases (a test module calls this when it is done: the 2l weights alone are 0.4 GB)"""
    for f in (talker_case, cp_case, _base, _plant_matrix):
        f.cache_clear()


def bound(b1, case):
    """B1 * max(1, eo_g / eo_1) * 2: the path's bound at gain 1, scaled by how much the peaked softmax amplifies the oracle's own fp32
    rounding on this scenario, times 2 because two implementations' noise is not amplified identically.  CPU numbers only."""
    return b1 * max(1.0, case["eo_g"] / case["eo_1"]) * 2.0
