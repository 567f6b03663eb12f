"""Generate the golden that pins the audio encoder's [HINT] architecture: transformers MimiModel.encode at tiny seeded dims.

    python tests/golden/make_hf_mimi_golden.py      # rewrites tests/golden/hf_mimi_encoder.npz

Run in the build container only (needs torch + transformers); the .npz is committed and is what the tests read.  It holds
  w:enc.*            the weights under the registry's names (float32; codebooks already folded embed_sum / clamp(cluster_usage, 1e-5))
  cfg                the enc_* config fields + n_groups as JSON
  lat_<n>, codes_<n>, gaps_<n>   for each probe length n: fp64 latents [F][hidden], codes [F][16], relative top-2 gaps (d2 - d1) / d1
  hfcodes64_<n>, hfcodes32_<n>   the codes transformers itself returns for the fp64 and the fp32 model (its cdist runs in float32 either way);
                     tests/test_cpu_audio_encoder.py holds them against codes_<n> with the margin-aware rule
  hf_fp32_err        max |latents of the fp32 model - latents of the fp64 model| over the probes (the tests assert 10 x this)
  dist_rel_err       max relative perturbation of the two nearest squared distances, fp32 against fp64 (the code gate is 10 x this)
  hf_fp32_moved      frames whose codes differ between the fp32 and the fp64 model, and the frame total
  state_dict_keys    the model's state_dict key list as JSON (what tools/import_safetensors.py must map), with shapes
Input clips come from tests/mimi_ref.py clip(n, seed): a seeded formula, not stored."""
import json
import os
import sys

import numpy as np
import torch
from transformers import MimiConfig, MimiModel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mimi_ref  # noqa: E402

torch.manual_seed(0)
torch.set_grad_enabled(False)
G = 16
LENGTHS = [1, 1919, 1920, 1921, 5 * 1920 + 777, 39177]
CFG = dict(enc_hidden=32, enc_filters=4, enc_n_ratios=4, enc_ratios=[4, 5, 6, 8], enc_kernel=7, enc_res_kernel=3, enc_last_kernel=3,
           enc_layers=2, enc_heads=2, enc_head_dim=16, enc_ffn=64, enc_window=6, enc_vq_dim=16, enc_codebook=64,
           enc_rope_theta=10000.0, enc_norm_eps=1e-5, n_groups=G)


def build():
    hc = MimiConfig(hidden_size=32, num_filters=4, upsampling_ratios=[8, 6, 5, 4], num_hidden_layers=2, num_attention_heads=2,
                    num_key_value_heads=2, head_dim=16, intermediate_size=64, sliding_window=6, vector_quantization_hidden_dimension=16,
                    codebook_size=64, codebook_dim=16, num_quantizers=G, num_semantic_quantizers=1, upsample_groups=32)
    hc._attn_implementation = "eager"
    m = MimiModel(hc).eval()
    g = torch.Generator().manual_seed(1)
    for n, p in m.named_parameters():
        if not (n.startswith("encoder.") or n.startswith("encoder_transformer.") or n.startswith("downsample.") or n.startswith("quantizer.")):
            continue
        if n.endswith("layer_scale.scale"):
            p.copy_(0.25 + 0.5 * torch.rand(p.shape, generator=g))
        elif "layernorm.weight" in n:
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        elif n.endswith(".bias"):
            p.copy_(0.1 * torch.randn(p.shape, generator=g))
        else:
            fan = int(np.prod(p.shape[1:]))
            p.copy_(torch.randn(p.shape, generator=g) / np.sqrt(fan))
    return m


def latents_of(m, x):
    got = {}
    h = m.downsample.register_forward_hook(lambda mod, i, o: got.__setitem__("lat", o))
    codes = m.encode(x, num_quantizers=G).audio_codes
    h.remove()
    return got["lat"][0].transpose(0, 1).contiguous(), codes[0].transpose(0, 1).contiguous()


def registry_weights(m):
    sd = {k: v.detach().double().numpy() for k, v in m.state_dict().items()}
    w = {}
    w["conv_in.w"], w["conv_in.b"] = sd["encoder.layers.0.conv.weight"], sd["encoder.layers.0.conv.bias"]
    for s in range(4):
        r, d = 1 + 3 * s, 3 + 3 * s
        p = "stages.%d." % s
        w[p + "res.conv1.w"], w[p + "res.conv1.b"] = sd["encoder.layers.%d.block.1.conv.weight" % r], sd["encoder.layers.%d.block.1.conv.bias" % r]
        w[p + "res.conv2.w"], w[p + "res.conv2.b"] = sd["encoder.layers.%d.block.3.conv.weight" % r], sd["encoder.layers.%d.block.3.conv.bias" % r]
        w[p + "down.w"], w[p + "down.b"] = sd["encoder.layers.%d.conv.weight" % d], sd["encoder.layers.%d.conv.bias" % d]
    w["conv_out.w"], w["conv_out.b"] = sd["encoder.layers.14.conv.weight"], sd["encoder.layers.14.conv.bias"]
    for l in range(CFG["enc_layers"]):
        s, p = "encoder_transformer.layers.%d." % l, "layers.%d." % l
        w[p + "input_norm.w"], w[p + "input_norm.b"] = sd[s + "input_layernorm.weight"], sd[s + "input_layernorm.bias"]
        w[p + "post_norm.w"], w[p + "post_norm.b"] = sd[s + "post_attention_layernorm.weight"], sd[s + "post_attention_layernorm.bias"]
        for n in "qkvo":
            w[p + n + "_proj"] = sd[s + "self_attn.%s_proj.weight" % n]
        w[p + "fc1"], w[p + "fc2"] = sd[s + "mlp.fc1.weight"], sd[s + "mlp.fc2.weight"]
        w[p + "attn_scale"], w[p + "mlp_scale"] = sd[s + "self_attn_layer_scale.scale"], sd[s + "mlp_layer_scale.scale"]
    w["downsample.w"] = sd["downsample.conv.weight"]
    for key, q in (("sem", "semantic"), ("ac", "acoustic")):
        w["vq.%s.in_proj" % key] = sd["quantizer.%s_residual_vector_quantizer.input_proj.weight" % q][:, :, 0]
    for gidx in range(G):
        q, j = ("semantic", 0) if gidx == 0 else ("acoustic", gidx - 1)
        b = "quantizer.%s_residual_vector_quantizer.layers.%d.codebook." % (q, j)
        w["vq.codebook.%d" % gidx] = sd[b + "embed_sum"] / np.maximum(sd[b + "cluster_usage"], 1e-5)[:, None]
    return w


def calibrate_codebooks(m):
    """codebooks at the projected latents' spread, decaying 0.75 per level, level 0 of each quantizer centred on their mean; stored as
    embed_sum = rows x usage with a random cluster_usage so that the importer's fold is exercised"""
    g = torch.Generator().manual_seed(2)
    lats = [latents_of(m, torch.from_numpy(mimi_ref.clip(n, s))[None, None])[0] for s, n in enumerate((39177, 24000, 30000))]
    lat = torch.cat(lats, 0)
    for q in (m.quantizer.semantic_residual_vector_quantizer, m.quantizer.acoustic_residual_vector_quantizer):
        z = lat @ q.input_proj.weight[:, :, 0].T
        mean, sd = z.mean(0), float((z - z.mean(0)).std())
        for j, layer in enumerate(q.layers):
            cb = layer.codebook
            rows = sd * (0.75 ** j) * torch.randn(cb.embed_sum.shape, generator=g) + (mean if j == 0 else 0.0)
            usage = 0.5 + 1.5 * torch.rand(cb.cluster_usage.shape, generator=g)
            cb.cluster_usage.copy_(usage)
            cb.embed_sum.copy_(rows * usage[:, None])
            cb._embed = None


def main():
    m = build()
    calibrate_codebooks(m)
    m64 = MimiModel(m.config).eval().double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    for q in (m64.quantizer.semantic_residual_vector_quantizer, m64.quantizer.acoustic_residual_vector_quantizer):
        for layer in q.layers:
            layer.codebook._embed = None
    w = registry_weights(m)
    out = {"w:enc." + k: v.astype(np.float32) for k, v in w.items()}
    w32 = {k: v.astype(np.float32).astype(np.float64) for k, v in w.items()}   # what the tests load: the float32 values
    err, rel, moved, frames = 0.0, 0.0, 0, 0
    for seed, n in enumerate(LENGTHS):
        x = torch.from_numpy(mimi_ref.clip(n, seed))[None, None]
        lat32, codes32 = latents_of(m, x)
        lat64, codes64 = latents_of(m64, x.double())
        lat64, codes64 = lat64.numpy(), codes64.numpy()
        # cdist in transformers quantises in float32 whatever the model's dtype: the fp64 reference decisions are the restatement's
        # on the fp64 latents (direct squared distances in fp64), checked against the model's own where the margin is comfortable
        codes, gaps = mimi_ref.quantize(w32, CFG, lat64)
        first = [(f, int(np.argmax(codes[f] != codes64[f]))) for f in range(codes.shape[0]) if (codes[f] != codes64[f]).any()]
        for f, gi in first:
            assert gaps[f, gi] < 1e-4, ("transformers fp64 model disagrees with the restatement at a comfortable margin", n, f, gi, gaps[f, gi])
        out["lat_%d" % n], out["codes_%d" % n], out["gaps_%d" % n] = lat64, codes, gaps
        out["hfcodes64_%d" % n], out["hfcodes32_%d" % n] = codes64.astype(np.int64), codes32.numpy().astype(np.int64)   # transformers' own decisions
        err = max(err, float(np.abs(lat32.numpy().astype(np.float64) - lat64).max()))
        # distance perturbation fp32 against fp64: the two nearest rows of every decision the two paths share
        c32, _ = mimi_ref.quantize(w32, CFG, lat32.numpy(), dtype=np.float32)
        z64 = {"sem": lat64 @ w32["vq.sem.in_proj"].T, "ac": lat64 @ w32["vq.ac.in_proj"].T}
        z32 = {"sem": lat32.numpy() @ w32["vq.sem.in_proj"].astype(np.float32).T, "ac": lat32.numpy() @ w32["vq.ac.in_proj"].astype(np.float32).T}
        alive = np.ones(codes.shape[0], bool)
        for gi in range(G):
            key = "sem" if gi == 0 else "ac"
            E = w32["vq.codebook.%d" % gi]
            d64 = ((z64[key][:, None] - E[None]) ** 2).sum(-1)
            d32 = ((z32[key][:, None] - E[None].astype(np.float32)) ** 2).sum(-1, dtype=np.float32)
            near = np.argsort(d64, -1)[:, :2]
            r = np.abs(np.take_along_axis(d32.astype(np.float64), near, 1) - np.take_along_axis(d64, near, 1)) / np.take_along_axis(d64, near, 1)
            if alive.any():
                rel = max(rel, float(r[alive].max()))
            alive &= codes[:, gi] == c32[:, gi]
            z64[key] = z64[key] - E[codes[:, gi]]
            z32[key] = z32[key] - E[c32[:, gi]].astype(np.float32)
        moved += int((codes32.numpy() != codes).any(1).sum())
        frames += codes.shape[0]
    out["cfg"] = np.array(json.dumps(CFG))
    out["hf_fp32_err"] = np.float64(err)
    out["dist_rel_err"] = np.float64(rel)
    out["hf_fp32_moved"] = np.array([moved, frames], np.int64)
    out["state_dict_keys"] = np.array(json.dumps({k: list(v.shape) for k, v in m.state_dict().items()}))
    path = os.path.join(HERE, "hf_mimi_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes; hf fp32-vs-fp64 latents err %.3e, distance rel err %.3e, fp32 moved %d of %d frames" % (
        path, os.path.getsize(path), err, rel, moved, frames))
    for n in LENGTHS:
        c = out["codes_%d" % n]
        print("  n=%d frames=%d distinct ids per codebook: %s" % (n, c.shape[0], [len(set(c[:, gi])) for gi in range(G)]))


if __name__ == "__main__":
    main()
