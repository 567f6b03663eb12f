"""Streaming behind a prefix, measured at 0.6B dimensions with synthetic weights on one MI355X:

1. device time (q3tts_last_codec_ms, HIP events) of PRIMING g in {1, 16, 64} fresh streams with 125 frames each
   (q3tts_codec_stream_prime_batch_host: pre-transformer only) against the batched push of the same frames on g other fresh streams with
   the audio dropped (q3tts_codec_stream_push_batch_host) — the only way to reach that state before priming existed.  The two alternate;
   median of 5 rounds after one warm-up round, with the spread;
2. each stream's bytes afterwards (q3tts_codec_stream_info), for 125 and for 375 frames;
3. wall time from the call of q3tts_synthesize_continue_stream_host to the first audio callback for 16 clone-shaped utterances (a 125-frame
   prefix each, chunk_frames 5), median of 3 after one warm-up;
4. the b=1 decode step against the parent commit: `--parent DIR` names a checkout of the parent commit built from its own tree with the
   same flags; bench.py runs alternate parent / new, three each (as profiles/audio_encode.txt does).  Without --parent the section says
   "not measured".

    python tools/continue_stream_bench.py [--parent DIR] [--out profiles/continue_stream.txt]

Prints what it writes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q3tts  # noqa: E402

FRAMES, ROUNDS = 125, 5


def prime_vs_push(eng, g, rng, lines):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    codes = [rng.integers(0, CB, (FRAMES, G)).astype(np.int64) for _ in range(g)]
    A, B, info = [], [], None
    for r in range(ROUNDS + 1):
        sp = [eng.codec_stream_begin(FRAMES) for _ in range(g)]
        sq = [eng.codec_stream_begin(FRAMES) for _ in range(g)]
        eng.codec_stream_prime_batch(sp, codes)
        a = eng.last_codec_ms()
        eng.codec_stream_push_batch(sq, codes)
        b = eng.last_codec_ms()
        info = (eng.codec_stream_info(sp[0]), eng.codec_stream_info(sq[0]))
        for s in sp + sq:
            eng.codec_stream_end(s)
        if r > 0:
            A.append(a); B.append(b)
    a, b = statistics.median(A), statistics.median(B)
    lines.append("   g = %2d x %d frames: priming %8.3f ms (min %.3f, max %.3f)   discarded push %8.3f ms (min %.3f, max %.3f)   ratio %.3f   "
                 "per primed frame %.2f us, per pushed frame %.2f us" % (g, FRAMES, a, min(A), max(A), b, min(B), max(B), a / b,
                                                                        1e3 * a / (g * FRAMES), 1e3 * b / (g * FRAMES)))
    return info


def stream_bytes(eng, rng, lines):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    for n in (125, 375):
        c = rng.integers(0, CB, (n, G)).astype(np.int64)
        sp, sq = eng.codec_stream_begin(n), eng.codec_stream_begin(n)
        begun = eng.codec_stream_info(sp)
        eng.codec_stream_prime_batch([sp], [c])
        eng.codec_stream_push_batch([sq], [c])
        p, q = eng.codec_stream_info(sp), eng.codec_stream_info(sq)
        eng.codec_stream_end(sp); eng.codec_stream_end(sq)
        lines.append("   %3d frames: begun %d K / V rows, %.1f MB;  primed %d rows, %.1f MB;  pushed %d rows, %.1f MB" % (
            n, begun[1], begun[2] / 1e6, p[1], p[2] / 1e6, q[1], q[2] / 1e6))


def first_audio(lines):
    from util import frame_tokens
    cfg = q3tts.default_config("0.6b")
    eng = q3tts.Engine(cfg, device=0, max_batch=16, max_ctx=512)
    eng.fill_synthetic(0)
    rng = np.random.default_rng(1)
    n = 16
    toks = [frame_tokens(rng.integers(0, 151643, 40)) for _ in range(n)]
    _, plain, _ = eng.synthesize_batch(toks, q3tts.Sampling(max_new_tokens=FRAMES), seed=1, ignore_eos=True)
    sp = q3tts.Sampling(max_new_tokens=10)
    ts = []
    for r in range(4):
        t = {}

        def on_audio(utt, fb, fe, pcm, fin):
            t.setdefault("first", time.perf_counter())
            return 0
        t0 = time.perf_counter()
        eng.synthesize_continue(toks, plain, sp, seed=2, ignore_eos=True, chunk_frames=5, on_audio=on_audio)
        if r > 0:
            ts.append(1e3 * (t["first"] - t0))
    eng.close()
    lines.append("   16 utterances behind %d-frame prefixes, chunk_frames 5: call -> first callback %.1f ms median of 3 (min %.1f, max %.1f); includes the "
                 "wrapper's argument packing, 16 forced begins, one priming call, 5 decode steps and one batched push" % (FRAMES, statistics.median(ts), min(ts), max(ts)))


def step_vs_parent(parent, lines):
    if not parent:
        lines.append("   not measured (no --parent checkout given)")
        return

    def run(tree):
        out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-b64", "--no-long"], capture_output=True, text=True,
                             cwd=tree, timeout=900).stdout
        d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        return float(d.get("decode_ms_per_frame_step", float("nan"))), d.get("value")
    P, N = [], []
    lines.append("   parent = the commit before this change, built from its own tree with the same flags; runs alternate parent / new, three each:")
    for _ in range(3):
        p, pv = run(parent)
        P.append(p)
        lines.append("   parent decode_ms_per_frame_step %.4f  RTF value %s" % (p, pv))
        q, qv = run(ROOT)
        N.append(q)
        lines.append("   new    decode_ms_per_frame_step %.4f  RTF value %s" % (q, qv))
    lines.append("   median parent %.4f ms, median new %.4f ms: difference %+.4f ms; parent's own spread %.4f ms (%.4f .. %.4f), new %.4f ms (%.4f .. %.4f)" % (
        statistics.median(P), statistics.median(N), statistics.median(N) - statistics.median(P), max(P) - min(P), min(P), max(P), max(N) - min(N), min(N), max(N)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continue_stream.txt"))
    a = ap.parse_args()
    lines = ["Streaming behind a prefix: primed vocoder streams, 0.6B dimensions, synthetic weights, one MI355X",
             "python tools/continue_stream_bench.py", "",
             "1. priming against the discarded push (device time, median of %d alternating rounds after 1 warm-up round)" % ROUNDS]
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=512)
    eng.fill_synthetic(0)
    rng = np.random.default_rng(0)
    for g in (1, 16, 64):
        prime_vs_push(eng, g, rng, lines)
    lines += ["", "2. a stream's K / V rows and bytes (q3tts_codec_stream_info) on a fresh engine's streams"]
    eng.close()
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=512)
    eng.fill_synthetic(0)
    stream_bytes(eng, rng, lines)
    eng.close()
    lines += ["", "3. time to first audio"]
    first_audio(lines)
    lines += ["", "4. b=1 decode step against the parent commit (the feature touches no launch of it)"]
    step_vs_parent(a.parent, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
