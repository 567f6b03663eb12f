"""Wall-clock comparison of the two voice-clone front ends on one engine (1.7B dims, synthetic weights), same process, same card,
alternating rounds:

  parent path        n x Engine.extract_speaker_embedding(path): host WAV reader, host resampler, host log-mel, one encoder pass and
                     one stream sync per clip
  new, from files    n x q3tts.read_wav + ONE Engine.speaker_embeddings call (GPU resample + log-mel + batched encoder, one sync)
  new, from memory   one Engine.speaker_embeddings call on arrays already loaded

for n = 8 and n = 1.  The clips are the eight 3 s sine sweeps at 16 kHz of bench.py's clone record.  Median, min and max of the timed
rounds in ms, per call and per clip.  `python tools/clone_frontend_bench.py [--rounds 20] [--warmup 3] [--out FILE]`"""
import argparse
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))


def write_sweep_wav(path, seconds, f0, f1, sr):
    """the clone reference of bench.py: a 16-bit mono sine sweep"""
    t = np.arange(int(seconds * sr)) / sr
    x = (0.5 * np.sin(2 * np.pi * (f0 * t + (f1 - f0) * t * t / (2 * seconds))) * 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import q3tts

    eng = q3tts.Engine(q3tts.default_config("1.7b"), device=args.device, max_batch=8, max_ctx=64)
    eng.fill_synthetic(seed=0)
    td = tempfile.mkdtemp(prefix="q3clone_front_")
    wavs = []
    for u in range(8):
        wavs.append(os.path.join(td, "ref%d.wav" % u))
        write_sweep_wav(wavs[-1], 3.0, 80.0 + 10 * u, 3000.0 + 200 * u, 16000)
    loaded = [q3tts.read_wav(w) for w in wavs]
    clips, rates = [a for a, _ in loaded], [sr for _, sr in loaded]

    def parent(n):
        return np.stack([eng.extract_speaker_embedding(w) for w in wavs[:n]])

    def new_files(n):
        got = [q3tts.read_wav(w) for w in wavs[:n]]
        return eng.speaker_embeddings([a for a, _ in got], [sr for _, sr in got])

    def new_memory(n):
        return eng.speaker_embeddings(clips[:n], rates[:n])

    paths = [("parent path (n x extract_speaker_embedding)", parent), ("new path from files (n x read_wav + 1 call)", new_files),
             ("new path from memory (1 call)", new_memory)]
    lines = ["clone front end, 1.7B dims (spk_enc_dim %d), 3 s clips at 16 kHz, %d warm-up + %d timed rounds, alternating, wall clock in ms"
             % (eng.cfg.spk_enc_dim, args.warmup, args.rounds)]
    for n in (8, 1):
        times = {name: [] for name, _ in paths}
        ref = parent(n)
        for name, fn in paths[1:]:
            dev = float(np.abs(fn(n) - ref).max()) / float(np.abs(ref).max())
            lines.append("n = %d  %-46s max |new - parent| / max |parent| = %.3g" % (n, name, dev))
        for r in range(args.warmup + args.rounds):
            for name, fn in paths:
                t0 = time.perf_counter()
                fn(n)
                dt = (time.perf_counter() - t0) * 1e3
                if r >= args.warmup:
                    times[name].append(dt)
        for name, _ in paths:
            t = times[name]
            lines.append("n = %d  %-46s median %8.3f  min %8.3f  max %8.3f  per clip (median) %7.3f"
                         % (n, name, statistics.median(t), min(t), max(t), statistics.median(t) / n))
    eng.close()
    for w in wavs:
        os.remove(w)
    os.rmdir(td)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
