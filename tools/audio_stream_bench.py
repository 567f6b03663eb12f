"""Streamed audio-to-codes (q3tts_audio_stream_push_batch_host) measured at full dimensions with synthetic weights: one push to each of
1, 8 and 64 streams, 1 920, 9 600 and 48 000 samples per stream and push.  Per case: device time (HIP events around the uploads and
launches, q3tts_last_audio_encode_ms) and wall clock around the synchronising call, median of --rounds rounds after a warm-up; beside
it the one-shot audio_encode_batch of the same total audio (as many clips of the push's length), the two alternating in one process.
Also ms per push as a share of real time: ms / (audio ms per stream and push).

    python tools/audio_stream_bench.py [--rounds 20] [--out profiles/audio_stream.txt]

Streams are warmed past the transformer's window (250 rows: 10 s) before the timed rounds, so every timed push reads full K/V rings.
The talker side of the engine is shrunk to one layer (it plays no part).  Prints what it writes."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream.txt"))
    a = ap.parse_args()
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64)
    eng.fill_synthetic(0)
    rng = np.random.default_rng(0)
    lines = ["Streamed audio -> codes: one push to each of S streams, full dimensions, synthetic weights, one MI355X",
             "python tools/audio_stream_bench.py --rounds %d   (median of the rounds after 1 warm-up round; streams warmed past the 250-row window first)" % a.rounds,
             "dev = HIP events around uploads + launches; wall = clock around the synchronising call; one-shot = audio_encode_batch of S clips of the push's length,",
             "alternating with the push in one process; share = device ms per push / audio ms per stream and push", ""]
    for S in (1, 8, 64):
        for n in (1920, 9600, 48000):
            total = 264000 + (a.rounds + 2) * n
            sids = [eng.audio_stream_begin(total) for _ in range(S)]
            warm = [(0.3 * rng.standard_normal(264000)).astype(np.float32) for _ in range(S)]
            eng.audio_stream_push_batch(sids, warm)
            dev, wall, dev1, wall1 = [], [], [], []
            for r in range(a.rounds + 1):
                clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for _ in range(S)]
                t0 = time.perf_counter()
                eng.audio_stream_push_batch(sids, clips)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(eng.last_audio_encode_ms())
                t0 = time.perf_counter()
                eng.audio_encode_batch(clips, 24000)
                wall1.append((time.perf_counter() - t0) * 1e3)
                dev1.append(eng.last_audio_encode_ms())
            for s in sids:
                eng.audio_stream_end(s)
            md = statistics.median(dev[1:])
            lines.append("%2d streams x %5d samples (%4.0f ms): push dev %7.3f ms (min %.3f, max %.3f) wall %7.3f ms | one-shot dev %7.3f ms wall %7.3f ms | share of real time %5.1f %%" % (
                S, n, n / 24.0, md, min(dev[1:]), max(dev[1:]), statistics.median(wall[1:]), statistics.median(dev1[1:]), statistics.median(wall1[1:]),
                100.0 * md / (n / 24.0)))
    lines.append("")
    sid = eng.audio_stream_begin()
    lines.append("state per stream: %d bytes" % eng.audio_stream_info(sid)[3])
    eng.audio_stream_end(sid)
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
