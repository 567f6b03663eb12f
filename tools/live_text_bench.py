"""Live text input, measured (0.6B dims, synthetic weights):
  1. one q3tts_slots_text_append_ids call of 1 id per slot for 1 / 8 / 64 slots (wall clock, median of --reps);
  2. time to the first audio chunk of a 40-id utterance whose ids arrive one every --token-ms: begun after 5 ids (live text) against
     begun after all 40 (what every other entry needs).  The arrival schedule is simulated on the host: the text source hands out the
     ids whose arrival time has passed and sleeps 1 ms when it has nothing.
Prints one line per figure; the output belongs in profiles/live_text.txt."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

ROLE = [151644, 77091, 151672]
TAIL = [151673, 151645]


def bench_append(reps):
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=64, max_ctx=128)
    eng.fill_synthetic(seed=0)
    sp = q3tts.Sampling(max_new_tokens=8)
    ids = np.array(ROLE + [1001, 1002], np.int64)
    prompt, trailing = eng.build_prompt_open(ids, 0)
    for b in range(64):
        eng.slot_begin(b, prompt, trailing, sp, seed=1, stream_id=b, ignore_eos=True)
        eng.slot_text_open(b)
    for n in (1, 8, 64):
        ts = []
        for r in range(reps + 2):
            t0 = time.perf_counter()
            eng.slots_text_append_ids(list(range(n)), [[2000 + r]] * n)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[2:]
        print("append_ids 1 id x %2d slots: median %.3f ms (min %.3f, max %.3f, %d calls)" % (n, statistics.median(ts), min(ts), max(ts), len(ts)))
    eng.close()


def bench_first_audio(token_ms, chunk, reps):
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=512)
    eng.fill_synthetic(seed=0)
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=60)
    ids = ROLE + [3000 + 7 * k for k in range(35)] + TAIL        # 40 ids
    for name, hold in (("begun after 5 usable ids (live)", False), ("begun after all 40 ids", True)):
        firsts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            given, first = [0], []

            def source(u):
                have = min(len(ids), int((time.perf_counter() - t0) * 1e3 / token_ms))
                if hold and have < len(ids):
                    have = 0
                if have == given[0]:
                    time.sleep(0.001)
                    return [], False
                a, given[0] = given[0], have
                return ids[a:have], have == len(ids)

            def on_audio(u, fb, fe, pcm, fin):
                if not first and pcm.size:
                    first.append((time.perf_counter() - t0) * 1e3)
                return 0
            eng.synthesize_live(1, source, sp, chunk, on_audio, seed=3, ignore_eos=True, want_codes=False)
            firsts.append(first[0])
        firsts = firsts[1:]
        print("first audio chunk (%d frames), ids every %g ms, %s: median %.1f ms after the first id (min %.1f, max %.1f)"
              % (chunk, token_ms, name, statistics.median(firsts), min(firsts), max(firsts)))
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--token-ms", type=float, default=20.0)
    ap.add_argument("--chunk", type=int, default=4)
    a = ap.parse_args()
    bench_append(a.reps)
    bench_first_audio(a.token_ms, a.chunk, 3)
