"""Decode step with a repetition penalty armed (bench.py cannot pass one): B slots of the 0.6B synthetic engine, sampled 0.8 / 50 / 0.95,
EOS suppressed, `--frames` frames; prints one JSON line with the step time of the timed replays.

    python tools/penalty_step_bench.py [--penalty 1.1] [--batch 1] [--frames 512] [--no-graph]
    rocprofv3 --kernel-trace --stats -- python tools/penalty_step_bench.py --no-graph --frames 256    (the code0 sampler is k_sample<false, 12, true>)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--penalty", type=float, default=1.1)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--frames", type=int, default=512)
ap.add_argument("--no-graph", action="store_true")
a = ap.parse_args()
eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=a.batch, max_ctx=a.frames + 64, flags=q3tts.FLAG_NO_GRAPH if a.no_graph else 0)
eng.fill_synthetic(seed=0)
ids = np.array([151644, 77091, 151672] + list(np.random.default_rng(1).integers(0, 151643, 16)) + [151673, 151645], np.int64)
prompt, trailing = eng.build_prompt(ids, 0)
sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, repetition_penalty=a.penalty, max_new_tokens=a.frames)
for b in range(a.batch):
    eng.slot_begin(b, prompt, trailing, sp, seed=0, stream_id=b, ignore_eos=True)
eng.decode_steps(16)                      # graph capture + warm-up, untimed
eng.counters(reset=True)
eng.decode_steps(a.frames - 16)
c = eng.counters()
distinct = len(set(eng.slot_codes(0)[:, 0].tolist()))
print(json.dumps(dict(penalty=a.penalty, batch=a.batch, frames=a.frames, graph=not a.no_graph, step_ms=round(c["decode_ms"] / c["decode_steps"], 4),
                      distinct_code0_slot0=distinct)))
eng.close()
