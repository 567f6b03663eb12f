"""G.711 on both legs, measured against int16 (0.6B dims, synthetic fill): what the eight-bit formats cost, or save, on the
pushes they ride on.

Out: 64 streams x 25 frames and 1 stream x 1 frame per vocoder push, after a 100-frame history, through 8 kHz int16 sinks and 8 kHz
mu-law sinks; one set of streams per format, the formats alternate round by round in one process.  Per format and case: the median
over the rounds of q3tts_last_codec_ms (device events around the push, its sinks' launch included) and of the wall clock around the
synchronising call (device -> host copies included), each with its spread (min .. max), and the bytes copied back per push.

In: 64 encoder streams at 8 kHz given 2 s each in one q3tts_audio_stream_push_batch_any_host, int16 against mu-law (the bytes are the
mu-law code of the int16 samples); the formats alternate round by round; median and spread of q3tts_last_audio_encode_ms and of the
wall clock, and the bytes uploaded per push.

    python tools/g711_bench.py [--rounds 15] [--out profiles/g711.txt]

Prints what it writes."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))

HIST = 100
CASES = [(64, 25), (1, 1)]
FORMATS = [(8000, "int16"), (8000, "mulaw")]
ENC_STREAMS, ENC_RATE, ENC_SECONDS = 64, 8000, 2


def med(v):
    return "%8.3f ms (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def sinks(q3tts, rounds, lines):
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=64)
    eng.fill_synthetic(seed=0)
    rng = np.random.default_rng(0)

    def rand(n):
        return rng.integers(0, eng.cfg.cd_codebook, (n, eng.cfg.n_groups)).astype(np.int64)
    for S, n in CASES:
        total = HIST + n * (rounds + 3)
        sids = {f: [eng.codec_stream_begin(total, sample_rate=f[0], dtype=f[1]) for _ in range(S)] for f in FORMATS}
        for f in FORMATS:
            eng.codec_stream_push_batch(sids[f], [rand(HIST) for _ in range(S)])
        dev, wall, nbytes = {f: [] for f in FORMATS}, {f: [] for f in FORMATS}, {}
        for r in range(rounds + 2):
            for f in FORMATS:
                codes = [rand(n) for _ in range(S)]
                t0 = time.perf_counter()
                out = eng.codec_stream_push_batch(sids[f], codes)
                w = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    dev[f].append(eng.last_codec_ms())
                    wall[f].append(w)
                    nbytes[f] = sum(o.nbytes for o in out)
        for f in FORMATS:
            for s in sids[f]:
                eng.codec_stream_end(s)
        lines.append("vocoder push, %d stream%s x %d frame%s" % (S, "" if S == 1 else "s", n, "" if n == 1 else "s"))
        base_d, base_w = statistics.median(dev[FORMATS[0]]), statistics.median(wall[FORMATS[0]])
        for f in FORMATS:
            lines.append("  %6d Hz %-6s: device %s, %+.3f ms on int16 | wall %s, %+.3f ms | %9d bytes back" % (
                f[0], f[1], med(dev[f]), statistics.median(dev[f]) - base_d, med(wall[f]), statistics.median(wall[f]) - base_w, nbytes[f]))
        lines.append("")
    eng.close()


def encoder(q3tts, rounds, lines):
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64)
    eng.fill_synthetic(0)
    rng = np.random.default_rng(1)
    n = ENC_RATE * ENC_SECONDS
    total = n * (rounds + 3)
    formats = ["int16", "mulaw"]
    sids = {f: [eng.audio_stream_begin_rate(ENC_RATE, f, total) for _ in range(ENC_STREAMS)] for f in formats}
    dev, wall, nbytes = {f: [] for f in formats}, {f: [] for f in formats}, {}
    for r in range(rounds + 2):
        s16 = [(rng.uniform(-0.5, 0.5, n) * 32767.0).astype(np.int16) for _ in range(ENC_STREAMS)]
        pcm = {"int16": s16, "mulaw": [q3tts.g711_encode("mulaw", a) for a in s16]}
        for f in formats:
            t0 = time.perf_counter()
            eng.audio_stream_push_batch(sids[f], pcm[f])
            w = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                dev[f].append(eng.last_audio_encode_ms())
                wall[f].append(w)
                nbytes[f] = sum(a.nbytes for a in pcm[f])
    for f in formats:
        for s in sids[f]:
            eng.audio_stream_end(s)
    eng.close()
    lines.append("encoder push, %d streams x %d s at %d Hz (one batched call; the wall clock includes the Python binding's per-stream bookkeeping)" % (ENC_STREAMS, ENC_SECONDS, ENC_RATE))
    base_d, base_w = statistics.median(dev["int16"]), statistics.median(wall["int16"])
    for f in formats:
        lines.append("  %6d Hz %-6s: device %s, %+.3f ms on int16 | wall %s, %+.3f ms | %9d bytes up" % (
            ENC_RATE, f, med(dev[f]), statistics.median(dev[f]) - base_d, med(wall[f]), statistics.median(wall[f]) - base_w, nbytes[f]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g711.txt"))
    a = ap.parse_args()
    import q3tts
    lines = ["G.711 against int16 on both legs: 8 kHz sinks on the batched vocoder push, 8 kHz encoder streams; 0.6B dims, synthetic weights, one MI355X",
             "python tools/g711_bench.py --rounds %d" % a.rounds,
             "2 warm-up rounds; formats alternate round by round in one process; median (min .. max) over %d rounds" % a.rounds,
             "device: q3tts_last_codec_ms / q3tts_last_audio_encode_ms (events around the push) | wall: host clock around the synchronising call, copies included", ""]
    sinks(q3tts, a.rounds, lines)
    encoder(q3tts, a.rounds, lines)
    text = "\n".join(lines)
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
