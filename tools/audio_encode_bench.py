"""Audio encoder (12 Hz tokenizer, audio -> codes), measured at full dimensions with synthetic weights: device time of
q3tts_audio_encode_batch_host (HIP events around the uploads and launches, q3tts_last_audio_encode_ms) for one clip of 3 s, 10 s and
30 s and for a batch of 8 x 10 s, beside the floors this script computes itself from the config: the FLOPs of every conv / linear /
attention / distance product at the fp32 matrix rate, and the bytes of a pass in which the weights are read once and every layer's
output is written once and read once, at the HBM rate.

    python tools/audio_encode_bench.py [--reps 5] [--out profiles/audio_encode.txt]

The talker side of the engine is shrunk to one layer (it plays no part).  Prints what it writes."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

FP32_MATRIX_FLOPS = 157.3e12   # MI355X fp32 matrix peak
HBM_BYTES_PER_S = 8.0e12       # MI355X HBM3E peak


def floors(cfg, lens):
    """(flops, bytes) of encoding clips of `lens` samples at 24 kHz"""
    ratios = list(cfg.enc_ratios)[: cfg.enc_n_ratios]
    EH, AO, ffn, D, CB, G, W = cfg.enc_hidden, cfg.enc_heads * cfg.enc_head_dim, cfg.enc_ffn, cfg.enc_vq_dim, cfg.enc_codebook, cfg.n_groups, cfg.enc_window
    flops = act = 0.0
    for n in lens:
        T, dim = n, cfg.enc_filters
        flops += 2.0 * T * dim * cfg.enc_kernel
        act += T * dim
        for r in ratios:
            flops += 2.0 * T * (dim // 2) * dim * cfg.enc_res_kernel + 2.0 * T * dim * (dim // 2)
            act += T * (dim // 2) + T * dim
            T = -(-T // r)
            flops += 2.0 * T * (2 * dim) * dim * (2 * r)
            dim *= 2
            act += T * dim
        flops += 2.0 * T * EH * dim * cfg.enc_last_kernel
        act += T * EH
        per_row = 2.0 * (EH * 3 * AO + AO * EH + 2 * EH * ffn)
        attn = sum(4.0 * min(t + 1, W) * AO for t in range(T))
        flops += cfg.enc_layers * (T * per_row + attn)
        act += cfg.enc_layers * T * (2 * EH + 3 * AO + AO + ffn + 2 * EH)
        F = -(-T // 2)
        flops += 2.0 * F * EH * EH * 4 + F * (2 * 2.0 * D * EH + G * 3.0 * CB * D)
        act += F * EH
    weights = sum(int(np.prod(s)) for nme, s, _ in q3tts.tensor_specs(cfg) if nme.startswith("enc."))
    return flops, 4.0 * (weights + sum(lens) + 2.0 * act)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_encode.txt"))
    a = ap.parse_args()
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64)
    eng.fill_synthetic(0)
    rng = np.random.default_rng(0)
    lines = ["Audio encoder (audio -> codes): device time at full dimensions, synthetic weights, one MI355X",
             "python tools/audio_encode_bench.py --reps %d   (HIP events around uploads + launches; median of the reps after 1 warm-up)" % a.reps,
             "floors: FLOPs at %.1f TF/s (fp32 matrix peak); bytes = weights once + every layer's output written once and read once, at %.1f TB/s" % (
                 FP32_MATRIX_FLOPS / 1e12, HBM_BYTES_PER_S / 1e12), ""]
    for label, lens in (("1 x 3 s", [72000]), ("1 x 10 s", [240000]), ("1 x 30 s", [720000]), ("8 x 10 s", [240000] * 8)):
        clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
        ts = []
        for _ in range(a.reps + 1):
            codes = eng.audio_encode_batch(clips, 24000)
            ts.append(eng.last_audio_encode_ms())
        ts = ts[1:]
        fl, by = floors(cfg, lens)
        distinct = min(len(set(codes[0][:, g])) for g in range(cfg.n_groups))
        lines.append("%-9s %6d frames: median %8.2f ms (min %.2f, max %.2f)   %7.2f GFLOP -> floor %6.3f ms   %7.1f MB -> floor %6.3f ms   real-time factor %.0fx   "
                     "(>= %d distinct ids per codebook in clip 0)" % (
                         label, sum(c.shape[0] for c in codes), statistics.median(ts), min(ts), max(ts), fl / 1e9, fl / FP32_MATRIX_FLOPS * 1e3,
                         by / 1e6, by / HBM_BYTES_PER_S * 1e3, sum(lens) / 24000.0 / (statistics.median(ts) / 1e3), distinct))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
