"""Cost of arming a slot behind F0 teacher-forced frames (q3tts_slot_begin_codes; the rows are reference src/tts_onnx.cpp:824-842) at
0.6B dims, one slot, synthetic weights, beside what a caller could do before it for the same state of the KV cache:

  forced     q3tts_slot_begin_codes: rows made on the device, chunked prefill of S + F0 rows
  emulation  the host-built rows: 16 q3tts_codec_embed_host / q3tts_cp_embed_host round trips per frame summed in numpy, appended to the
             prompt, q3tts_slot_begin — only entry points the code before this feature had, so this column is that code's figure
             (q3tts_slot_begin without a prefix takes the launches it took before)
  decode     F0 decode steps of the fused loop at b = 1 (q3tts_decode_steps; device time per step from its HIP events)

    python tools/continue_bench.py [--F0 64,256,1024] [--reps 5] [--out profiles/continue_from_codes.txt]

forced and emulation are wall-clock times of host-synchronous calls (uploads, launches and the final synchronisation included), one
untimed warm-up call per shape and `reps` timed ones: median, min and max.  decode is the device time of F0 graph-replayed steps after
a warm-up, three runs.  Nothing here is asserted by a test."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--F0", default="64,256,1024")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()
sizes = [int(v) for v in a.F0.split(",")]

cfg = q3tts.default_config("0.6b")
max_ctx = max(sizes) + 128
eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=max_ctx)
eng.fill_synthetic(seed=0)
ids = np.array([151644, 77091, 151672] + list(np.random.default_rng(1).integers(0, 151643, 16)) + [151673, 151645], np.int64)
prompt, trailing = eng.build_prompt(ids, 0)
sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=8)
rng = np.random.default_rng(2)


def timed(fn, reps):
    fn()
    eng.slot_release(0)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
        eng.slot_release(0)
    return float(np.median(out)), float(min(out)), float(max(out))


def forced(codes):
    eng.slot_begin(0, prompt, trailing, sp, seed=3, stream_id=0, ignore_eos=True, prefix_codes=codes)


def emulation(codes):
    rows = eng.codec_embed(codes[:, 0])
    for i, fr in enumerate(codes):
        x = rows[i]
        for j in range(1, cfg.n_groups):
            x = x + eng.cp_embed(int(fr[j]), j - 1)
        rows[i] = x + (trailing[i] if i < len(trailing) else pad)
    eng.slot_begin(0, np.concatenate([prompt, rows]), trailing[len(codes):], sp, seed=3, stream_id=0, ignore_eos=True)


pad = eng.text_project([151671])[0]
lines = ["continue from codes: arming a slot behind F0 forced frames, 0.6B dims, b = 1, synthetic weights, prompt of %d rows" % prompt.shape[0],
         "forced / emulation: wall ms of the host-synchronous call, median [min .. max] of %d after one warm-up; decode: device ms of F0 steps, median [min .. max] of 3" % a.reps,
         "%6s  %28s  %28s  %28s" % ("F0", "forced begin", "host-built rows + slot_begin", "F0 decode steps")]
for F0 in sizes:
    codes = rng.integers(0, 2048, (F0, cfg.n_groups)).astype(np.int64)
    f = timed(lambda: forced(codes), a.reps)
    e = timed(lambda: emulation(codes), max(2, a.reps // 2))
    runs = []
    for _ in range(3):
        eng.slot_begin(0, prompt, trailing, q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=F0 + 8), seed=3, stream_id=0, ignore_eos=True)
        eng.decode_steps(4)
        eng.decode_steps(F0)
        runs.append(eng.last_decode_ms()[0])
        eng.slot_release(0)
    d = (float(np.median(runs)), float(min(runs)), float(max(runs)))
    lines.append("%6d  %28s  %28s  %28s" % (F0, "%.2f [%.2f .. %.2f]" % f, "%.1f [%.1f .. %.1f]" % e, "%.1f [%.1f .. %.1f]" % d))
eng.close()
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
