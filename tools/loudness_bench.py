"""The loudness stage on the batched vocoder push, measured (0.6B dims, synthetic fill): what the BS.1770 meter and
normaliser cost on top of the push they ride on.

Cases: 64 streams x 25 frames and 1 stream x 1 frame per push, after a 100-frame history.  Stages: none (the parent commit's push, to
be read against profiles/pitch.txt and profiles/level.txt), meter only, and a target of -16 LUFS.  One set of streams per stage; the
stages alternate round by round in one process.  Per stage and case: the median over the rounds of q3tts_last_codec_ms (device events
around the push, its loudness stages' launch included) and of the wall clock around the synchronising call (device -> host copies
included), each with its spread (min .. max), and the bytes copied back per push.  The recursion runs over every sample whatever the
signal, so the synthetic vocoder's output costs what speech costs.  No threshold is set in advance; the comparison points are the
same push without a stage and the pitch stage's overhead in profiles/pitch.txt.

    python tools/loudness_bench.py [--rounds 15] [--out profiles/loudness.txt]

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
STAGES = [None, 0.0, -16.0]
NAMES = {None: "no stage", 0.0: "meter only", -16.0: "-16 LUFS"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness.txt"))
    a = ap.parse_args()
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=64)
    eng.fill_synthetic(seed=0)
    rng = np.random.default_rng(0)

    def rand(n):
        return rng.integers(0, eng.cfg.cd_codebook, (n, eng.cfg.n_groups)).astype(np.int64)
    lines = ["The loudness stage on the batched vocoder push: one q3tts_codec_stream_push_batch(_any)_host per round and stage, 0.6B dims, synthetic weights, one MI355X",
             "python tools/loudness_bench.py --rounds %d" % a.rounds,
             "after a %d-frame history and 2 warm-up rounds; stages alternate round by round; median (min .. max) over %d rounds" % (HIST, a.rounds),
             "device: q3tts_last_codec_ms (events around the push and its loudness stages' launch) | wall: host clock around the synchronising call, copies included", ""]
    for S, n in CASES:
        total = HIST + n * (a.rounds + 3)
        sids = {f: [eng.codec_stream_begin(total, **({} if f is None else dict(loudness=f))) for _ in range(S)] for f in STAGES}
        for f in STAGES:
            eng.codec_stream_push_batch(sids[f], [rand(HIST) for _ in range(S)])
        dev, wall, nbytes = {f: [] for f in STAGES}, {f: [] for f in STAGES}, {}
        for r in range(a.rounds + 2):
            for f in STAGES:
                codes = [rand(n) for _ in range(S)]
                t0 = time.perf_counter()
                out = eng.codec_stream_push_batch(sids[f], codes)
                w = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    dev[f].append(eng.last_codec_ms())
                    wall[f].append(w)
                    nbytes[f] = sum(o.nbytes for o in out)
        for f in STAGES:
            for s in sids[f]:
                eng.codec_stream_end(s)
        lines.append("%d stream%s x %d frame%s per push" % (S, "" if S == 1 else "s", n, "" if n == 1 else "s"))
        base_d, base_w = statistics.median(dev[None]), statistics.median(wall[None])
        for f in STAGES:
            d, w = statistics.median(dev[f]), statistics.median(wall[f])
            lines.append("  %-13s: device %8.3f ms (%.3f .. %.3f), %+.3f ms on no stage | wall %8.3f ms (%.3f .. %.3f), %+.3f ms | %9d bytes back%s" % (
                NAMES[f], d, min(dev[f]), max(dev[f]), d - base_d, w, min(wall[f]), max(wall[f]), w - base_w, nbytes[f],
                "  (no new launch)" if f is None else ""))
        lines.append("")
    eng.close()
    text = "\n".join(lines)
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
