"""Cost of long begins: 64 one-at-a-time forced begins against one ragged begin of the same members.

0.6B dims, 64 slots; each member has a 10-row prompt plus forced frames whose counts are drawn once, with a fixed seed, from 20..110.
A round runs (a) 64 slot_begin(prefix_codes=...) calls — the one-at-a-time path — and (b) one slots_begin_ragged call, alternating,
with the wall clock around each (both end synchronised); after a warm-up round, >= 10 rounds, medians and spread.  Both columns and the
pass counts go to profiles/ragged_prefill.txt.  The yardstick is column (a) of the same run, never column (b) alone.

    python tools/ragged_prefill_bench.py [--rounds 10] [--out profiles/ragged_prefill.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))


def main():
    import q3tts
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_prefill.txt"))
    a = ap.parse_args()
    rounds = max(10, a.rounds)
    cfg = q3tts.default_config("0.6b")
    n, H, G = a.slots, cfg.hidden, cfg.n_groups
    eng = q3tts.Engine(cfg, device=0, max_batch=n, max_ctx=256)
    eng.fill_synthetic(seed=0)
    rng = np.random.default_rng(1234)
    frames = rng.integers(20, 111, n)
    prompts = [(rng.standard_normal((10, H)) * 0.1).astype(np.float32) for _ in range(n)]
    trail = [(rng.standard_normal((1, H)) * 0.1).astype(np.float32) for _ in range(n)]
    codes = []
    for f in frames:
        c = rng.integers(0, cfg.sub_vocab, (int(f), G)).astype(np.int64)
        c[:, 0] = rng.integers(0, min(cfg.vocab, cfg.suppress_begin), int(f))
        codes.append(c)
    sp = q3tts.Sampling(max_new_tokens=8)
    slots = list(range(n))
    rows = int(sum(10 + int(f) for f in frames))

    def release():
        for s in slots:
            eng.slot_release(s)

    def one_at_a_time():
        t0 = time.perf_counter()
        for s in slots:
            eng.slot_begin(s, prompts[s], trail[s], sp, seed=1, stream_id=s, ignore_eos=True, prefix_codes=codes[s])
        return (time.perf_counter() - t0) * 1e3

    def ragged():
        t0 = time.perf_counter()
        eng.slots_begin_ragged(slots, prompts, trail, sp, prefix_codes=codes, seed=1, ignore_eos=True)
        return (time.perf_counter() - t0) * 1e3

    ta, tb = [], []
    for r in range(rounds + 1):   # round 0 warms up (workspaces, staging buffers)
        x = one_at_a_time()
        release()
        y = ragged()
        release()
        if r:
            ta.append(x)
            tb.append(y)
    eng.close()
    passes_a = sum((10 + int(f) + 127) // 128 for f in frames)
    passes_b = (rows + 127) // 128
    lines = [
        "ragged prefill: %d members at 0.6B dims, 10-row prompt + forced frames in 20..110 (seed 1234), %d rows in all" % (n, rows),
        "%d rounds after one warm-up, (a) and (b) alternating, wall clock around each, both end synchronised" % rounds,
        "(a) %d x slot_begin(prefix_codes): %d talker passes; median %.3f ms, min %.3f, max %.3f" % (n, passes_a, statistics.median(ta), min(ta), max(ta)),
        "(b) 1 x slots_begin_ragged:        %d talker passes; median %.3f ms, min %.3f, max %.3f" % (passes_b, statistics.median(tb), min(tb), max(tb)),
        "every (b) below every (a) by more than their spread: %s" % (max(tb) + (max(tb) - min(tb)) + (max(ta) - min(ta)) < min(ta)),
        "(a) ms: " + " ".join("%.3f" % v for v in ta),
        "(b) ms: " + " ".join("%.3f" % v for v in tb),
    ]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
