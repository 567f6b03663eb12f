"""Encoder streams at the source's own rate measured at full dimensions with synthetic weights: 64 streams and one
stream, 80 ms and 2 s of audio per stream and push, median wall clock around the synchronising call.

  (a) 16 kHz int16 streams through the resampling path (q3tts_audio_stream_push_batch_any_host);
  (b) the same audio resampled on the host with q3tts_resample_host and pushed to 24 kHz float streams: what a caller had to do before,
      the conversion from int16 and the resampling counted.  (a) and (b) alternate round by round in one process.
  (c) 24 kHz float streams, this tree against a build of the parent commit (--parent DIR: a checkout of it with its library built):
      fresh processes of the two alternate, --processes of each; per tree the median of its processes' medians and their spread.

    python tools/audio_stream_rate_bench.py [--rounds 30] [--parent DIR] [--processes 3] [--out profiles/audio_stream_rate.txt]

Streams are warmed past the transformer's window (250 rows: 10 s) before the timed rounds.  Prints what it writes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(64, 80), (64, 2000), (1, 80), (1, 2000)]          # streams, ms of audio per stream and push
WARM_S = 11


def engine(q3tts):
    cfg = q3tts.enable_audio_encoder(q3tts.default_config("0.6b"))
    cfg.n_layers, cfg.cp_layers, cfg.cd_layers, cfg.text_vocab, cfg.spk_enc_dim = 1, 1, 1, 1024, 0
    eng = q3tts.Engine(cfg, device=0, max_batch=3, max_ctx=64)
    eng.fill_synthetic(0)
    return eng


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def child(pkg, rounds):
    """(c): 24 kHz float streams with the q3tts of `pkg`, through the calls both trees have; prints {case: [wall ms per round]}"""
    sys.path.insert(0, pkg)
    import q3tts
    eng = engine(q3tts)
    rng = np.random.default_rng(0)
    res = {}
    for S, ms in CASES:
        n = 24 * ms
        sids = [eng.audio_stream_begin(WARM_S * 24000 + (rounds + 2) * n) for _ in range(S)]
        eng.audio_stream_push_batch(sids, [(0.3 * rng.standard_normal(WARM_S * 24000)).astype(np.float32) for _ in range(S)])
        wall = []
        for _ in range(rounds + 1):
            clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for _ in range(S)]
            wall.append(timed(lambda: eng.audio_stream_push_batch(sids, clips)))
        for s in sids:
            eng.audio_stream_end(s)
        res["%d x %d" % (S, ms)] = wall[1:]
    eng.close()
    print("RESULT " + json.dumps(res))


def run_child(pkg, rounds):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, "--rounds", str(rounds)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("child for %s failed:\n%s" % (pkg, r.stdout + r.stderr))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with leaxer-qwen3-tts_amd/libq3tts_hip.so built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream_rate.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds)
    here = os.path.join(ROOT, "leaxer-qwen3-tts_amd")
    lines = ["Encoder streams at the source's rate: one push to each of S streams, full dimensions, synthetic weights, one MI355X",
             "python tools/audio_stream_rate_bench.py --rounds %d --processes %d%s" % (a.rounds, a.processes, " --parent DIR" if a.parent else ""),
             "wall clock in ms around the synchronising call, median of the rounds after 1 warm-up round (min .. max); streams warmed past the 250-row window", ""]
    # (c) first: fresh processes, alternating, before this process opens the GPU
    if a.parent:
        meds = {"this": {}, "parent": {}}
        for _ in range(a.processes):
            for who, pkg in (("parent", os.path.join(a.parent, "leaxer-qwen3-tts_amd")), ("this", here)):
                for case, wall in run_child(pkg, a.rounds).items():
                    meds[who].setdefault(case, []).append(statistics.median(wall))
        lines.append("(c) 24 kHz float streams, this tree against the parent commit: %d alternating processes each, median of their medians (spread of the medians)" % a.processes)
        for S, ms in CASES:
            k = "%d x %d" % (S, ms)
            t, p = meds["this"][k], meds["parent"][k]
            inside = min(p) <= statistics.median(t) <= max(p)
            lines.append("%2d streams x %4d ms: this %8.3f ms (%.3f .. %.3f) | parent %8.3f ms (%.3f .. %.3f) | this tree's median %s the spread of the parent's runs" % (
                S, ms, statistics.median(t), min(t), max(t), statistics.median(p), min(p), max(p), "inside" if inside else ("BELOW" if statistics.median(t) < min(p) else "ABOVE")))
        lines.append("")
    else:
        lines += ["(c) not measured: no --parent checkout given", ""]

    sys.path.insert(0, here)
    import q3tts
    eng = engine(q3tts)
    rng = np.random.default_rng(0)
    lines.append("(a) 16 kHz int16 streams, resampled on the GPU on the way in | (b) int16 -> float and q3tts_resample_host on the host, then 24 kHz float streams (before: the figure to beat)")
    for S, ms in CASES:
        n = 16 * ms
        total = WARM_S * 16000 + (a.rounds + 2) * n
        sa = [eng.audio_stream_begin_rate(16000, "int16", total) for _ in range(S)]
        sb = [eng.audio_stream_begin(q3tts.resample_stream_emitted(16000, 24000, total, True) + 8) for _ in range(S)]
        warm = [np.round(0.3 * 32767 * np.clip(rng.standard_normal(WARM_S * 16000), -3, 3) / 3).astype(np.int16) for _ in range(S)]
        eng.audio_stream_push_batch(sa, warm)
        eng.audio_stream_push_batch(sb, [q3tts.resample(w.astype(np.float32) / np.float32(32768), 16000, 24000) for w in warm])
        wa, wb, wb_host = [], [], []
        for _ in range(a.rounds + 1):
            clips = [np.round(0.3 * 32767 * np.clip(rng.standard_normal(n), -3, 3) / 3).astype(np.int16) for _ in range(S)]
            wa.append(timed(lambda: eng.audio_stream_push_batch(sa, clips)))
            t0 = time.perf_counter()
            rs = [q3tts.resample(c.astype(np.float32) / np.float32(32768), 16000, 24000) for c in clips]
            host = (time.perf_counter() - t0) * 1e3
            wb_host.append(host)
            wb.append(host + timed(lambda: eng.audio_stream_push_batch(sb, rs)))
        for s in sa + sb:
            eng.audio_stream_end(s)
        ma, mb = statistics.median(wa[1:]), statistics.median(wb[1:])
        lines.append("%2d streams x %4d ms: (a) %8.3f ms (%.3f .. %.3f) | (b) %8.3f ms (%.3f .. %.3f), of it %.3f ms on the host | (a) / (b) = %.2f" % (
            S, ms, ma, min(wa[1:]), max(wa[1:]), mb, min(wb[1:]), max(wb[1:]), statistics.median(wb_host[1:]), ma / mb))
    lines += ["", "(b) resamples each push on its own, so its codes are NOT the one-shot's at the chunk boundaries; (a)'s are, bit for bit."]
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
