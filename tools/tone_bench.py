"""The tone stage on the batched vocoder push, measured (0.6B dims, synthetic fill): what a cascade of 1, 5 and 8
biquads costs on top of the push it rides on, and whether the cost depends on the number of sections.

Cases: 64 streams x 25 frames and 1 stream x 1 frame per push, after a 100-frame history.  Stages: none (the parent commit's push),
1 section (rumble), 5 (telephone) and 8.  One set of streams per stage; the stages alternate round by round in one process.  Per stage
and case: the median over the rounds of the wall clock around the synchronising call (device -> host copies included) and of
q3tts_last_codec_ms (device events around the push, its stages' launch included), each with its spread (min .. max).  The recursion
runs over every sample whatever the signal, so the synthetic vocoder's output costs what speech costs.  No threshold is set in
advance; the comparison points are the same push without a stage and the loudness stage's overhead in profiles/loudness.txt.

    python tools/tone_bench.py [--rounds 15] [--out profiles/tone.txt]
    Q3TTS_LIB=<the parent commit's library> python tools/tone_bench.py --no-stage-only --out <file>

The second form measures the push without a stage on a library that does not know the stage (an absent stage must cost nothing);
--append FILE adds that file's lines to what the first form writes.  Prints what it writes."""
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
EIGHT = [(1, 80, 0, 707), (3, 200, 30, 707), (5, 1000, -60, 4000), (5, 2500, 45, 1000), (4, 6000, -40, 707), (2, 11000, 0, 500),
         (5, 500, 20, 1000), (1, 20, 0, 707)]
STAGES = {"no stage": None, "1 section": "rumble", "5 sections": "telephone", "8 sections": EIGHT}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone.txt"))
    ap.add_argument("--no-stage-only", action="store_true")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    import q3tts
    stages = {"no stage": None} if a.no_stage_only else STAGES
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=64)
    eng.fill_synthetic(seed=0)
    rng = np.random.default_rng(0)

    def rand(n):
        return rng.integers(0, eng.cfg.cd_codebook, (n, eng.cfg.n_groups)).astype(np.int64)
    lines = ["The tone stage on the batched vocoder push: one q3tts_codec_stream_push_batch(_any)_host per round and stage, 0.6B dims, synthetic weights, one MI355X",
             "python tools/tone_bench.py --rounds %d%s   (library: %s)" % (a.rounds, " --no-stage-only" if a.no_stage_only else "", "the one Q3TTS_LIB names" if os.environ.get("Q3TTS_LIB") else "this tree's"),
             "after a %d-frame history and 2 warm-up rounds; stages alternate round by round; median (min .. max) over %d rounds" % (HIST, a.rounds),
             "wall: host clock around the synchronising call, copies included | device: q3tts_last_codec_ms (events around the push and its stages' launch)", ""]
    for S, n in CASES:
        total = HIST + n * (a.rounds + 3)
        sids = {k: [eng.codec_stream_begin(total, **({} if t is None else dict(tone=t))) for _ in range(S)] for k, t in stages.items()}
        for k in stages:
            eng.codec_stream_push_batch(sids[k], [rand(HIST) for _ in range(S)])
        dev, wall = {k: [] for k in stages}, {k: [] for k in stages}
        for r in range(a.rounds + 2):
            for k in stages:
                codes = [rand(n) for _ in range(S)]
                t0 = time.perf_counter()
                eng.codec_stream_push_batch(sids[k], codes)
                w = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    dev[k].append(eng.last_codec_ms())
                    wall[k].append(w)
        for k in stages:
            for s in sids[k]:
                eng.codec_stream_end(s)
        lines.append("%d stream%s x %d frame%s per push" % (S, "" if S == 1 else "s", n, "" if n == 1 else "s"))
        base_d, base_w = statistics.median(dev["no stage"]), statistics.median(wall["no stage"])
        for k in stages:
            d, w = statistics.median(dev[k]), statistics.median(wall[k])
            lines.append("  %-11s: wall %8.3f ms (%.3f .. %.3f), %+.3f ms on no stage | device %8.3f ms (%.3f .. %.3f), %+.3f ms%s" % (
                k, w, min(wall[k]), max(wall[k]), w - base_w, d, min(dev[k]), max(dev[k]), d - base_d, "  (no new launch)" if k == "no stage" else ""))
        lines.append("")
    eng.close()
    if a.append and os.path.exists(a.append):
        lines += ["The push without a stage on the parent commit's library, measured the same way in a process of its own:", ""] + open(a.append).read().split("\n")
    text = "\n".join(lines)
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
