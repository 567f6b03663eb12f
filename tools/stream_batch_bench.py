"""Batched vocoder streaming, measured (0.6B dims, synthetic fill; writes profiles/stream_batch_push.txt when given --out):

  push:   g in {8, 64} streams, pushes of 25 random frames after a 100-frame warm history — (A) g single q3tts_codec_stream_push_host
          calls against (B) one q3tts_codec_stream_push_batch_host, same process, five alternating rounds, medians of
          q3tts_last_codec_ms (device events; A is the sum over its g calls).
  stream: q3tts_synthesize_stream_host at b = 64 x 256 frames, chunk 25: wall time to the first callback of the last utterance of the
          first wave, and the job's RTF beside q3tts_synthesize_schedule_host on the same job (the throughput price of streaming).
  one:    a single batched push of g streams and nothing else timed — the program for `rocprofv3 --kernel-trace --stats -- python
          tools/stream_batch_bench.py one G` (a run of its own, under its own timeout); the launch count must not depend on G.

    python tools/stream_batch_bench.py [push|stream|all|one G] [--out FILE]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

HIST, N, ROUNDS = 100, 25, 5


def engine(max_batch, max_ctx):
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=max_batch, max_ctx=max_ctx)
    eng.fill_synthetic(seed=0)
    return eng


def rand(rng, eng, n):
    return rng.integers(0, eng.cfg.cd_codebook, (n, eng.cfg.n_groups)).astype(np.int64)


def warm_streams(eng, rng, g, frames):
    sids = [eng.codec_stream_begin(frames) for _ in range(g)]
    eng.codec_stream_push_batch(sids, [rand(rng, eng, HIST) for _ in range(g)])
    return sids


def bench_push(eng, g, say):
    rng = np.random.default_rng(g)
    sids = warm_streams(eng, rng, g, HIST + N * (2 * ROUNDS + 2))
    eng.codec_stream_push_batch(sids, [rand(rng, eng, N) for _ in range(g)])   # both paths' work buffers sized before the clock starts
    for s in sids:
        eng.codec_stream_push(s, rand(rng, eng, N))
    A, B = [], []
    for _ in range(ROUNDS):
        a = 0.0
        for s in sids:
            eng.codec_stream_push(s, rand(rng, eng, N))
            a += eng.last_codec_ms()
        A.append(a)
        eng.codec_stream_push_batch(sids, [rand(rng, eng, N) for _ in range(g)])
        B.append(eng.last_codec_ms())
    for s in sids:
        eng.codec_stream_end(s)
    a, b = statistics.median(A), statistics.median(B)
    say("push g=%d x %d frames: (A) %d single pushes %.2f ms  (B) one batched push %.2f ms  B/A %.3f  (%.1f / %.1f us per frame)"
        % (g, N, g, a, b, b / a, 1e3 * a / (g * N), 1e3 * b / (g * N)))


def bench_stream(say):
    b, F, chunk = 64, 256, 25
    eng = engine(b, 16 + F + 64)
    sp = q3tts.Sampling(max_new_tokens=F)
    rng = np.random.default_rng(1)
    toks = [np.concatenate([[151644, 77091, 151672], rng.integers(0, 151643, 16), [151673, 151645]]).astype(np.int64) for _ in range(b)]
    audio_s = b * eng.codec_decode_len(F) / 24000.0
    for rep in range(2):   # the first pass sizes every arena
        t0 = time.perf_counter()
        eng.synthesize_batch(toks, sp, seed=3, ignore_eos=True, want_codes=False)
        t_sched = time.perf_counter() - t0
        first = {}
        t0 = time.perf_counter()

        def on_audio(utt, fb, fe, pcm, fin):
            first.setdefault(utt, time.perf_counter() - t0)
            return 0
        eng.synthesize_stream(toks, sp, chunk, on_audio, seed=3, ignore_eos=True, want_codes=False)
        t_stream = time.perf_counter() - t0
    say("stream b=%d x %d frames, chunk %d: first audio of the last utterance of the first wave after %.1f ms; job %.3f s (RTF %.5f) "
        "against %.3f s (RTF %.5f) for the schedule entry: streaming costs %.1f %%"
        % (b, F, chunk, 1e3 * max(first.values()), t_stream, t_stream / audio_s, t_sched, t_sched / audio_s, 100.0 * (t_stream / t_sched - 1.0)))
    eng.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mode = args[0] if args else "all"
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if mode == "one":
        g = int(args[1])
        eng = engine(1, 512)
        rng = np.random.default_rng(g)
        sids = warm_streams(eng, rng, g, HIST + 2 * N)
        eng.codec_stream_push_batch(sids, [rand(rng, eng, N) for _ in range(g)])
        eng.close()
        return
    if mode in ("push", "all"):
        eng = engine(1, 512)
        for g in (8, 64):
            bench_push(eng, g, say)
        eng.close()
    if mode in ("stream", "all"):
        bench_stream(say)


if __name__ == "__main__":
    main()
