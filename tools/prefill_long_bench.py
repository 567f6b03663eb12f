"""Device time of the chunked long-prompt prefill (run_prefill, reference src/tts_onnx.cpp:615-665, past 16 rows) at 0.6B dims, one slot,
synthetic weights, against the only route the code before it offered to the same cache state: a 16-row prefill plus S - 16 decode steps
shaped like q3tts_talker_decode_host (one new row through every talker layer and the codec head).

    python tools/prefill_long_bench.py [--S 16,128,512] [--reps 8] [--out profiles/prefill_long.json]

Per S: q3tts_prefill_profile (one untimed warm-up pass, then `reps` passes between HIP events on the engine's stream), repeated three
times to show the spread.  The old route is priced as prefill(16) + (S - 16) x the eager talker stage of q3tts_stage_profile (out[2]:
layers + codec head of a one-row step, 64 eager steps after a 4-step warm-up) — measured at a context of ~30 tokens, so it is a LOWER
bound for that route (its steps at contexts of hundreds of tokens read more KV).  Also recorded: the talker weight bytes one pass
streams, and the share of the HBM peak (8 TB/s) that ceil(S / 128) such passes over the measured time come to — an end-to-end figure
for the whole prefill, not a kernel's share of peak.
Profiling target:  rocprofv3 --kernel-trace --stats -- python tools/prefill_long_bench.py --S 512 --reps 2   (per-launch kernel times)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s

ap = argparse.ArgumentParser()
ap.add_argument("--S", default="16,128,512")
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--out", default="")
a = ap.parse_args()
sizes = [int(v) for v in a.S.split(",")]

cfg = q3tts.default_config("0.6b")
max_ctx = max(sizes) + 64
eng = q3tts.Engine(cfg, device=0, max_batch=1, max_ctx=max_ctx, flags=q3tts.FLAG_NO_GRAPH)
eng.fill_synthetic(seed=0)

# talker weight bytes of one pass: every layer's matrices once + the codec head (bf16)
H, QKV, AO = cfg.hidden, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim, cfg.n_heads * cfg.head_dim
w_pass = 2.0 * (cfg.n_layers * (H * QKV + AO * H + 3 * H * cfg.ffn) + H * cfg.vocab)

# the old route's step: the eager talker stage of a one-slot decode step
ids = np.array([151644, 77091, 151672] + list(np.random.default_rng(1).integers(0, 151643, 16)) + [151673, 151645], np.int64)
prompt, trailing = eng.build_prompt(ids, 0)
sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=max_ctx - 16)
eng.slot_begin(0, prompt, trailing, sp, seed=3, stream_id=0, ignore_eos=True)
eng.decode_steps(4)
talker_ms = [eng.stage_profile(64)["talker_decode_ms"] for _ in range(3)]
eng.slot_release(0)
step_ms = float(np.median(talker_ms))

rec = {"dims": "0.6b", "slots": 1, "weights": "synthetic", "reps": a.reps, "talker_weight_bytes_per_pass": w_pass,
       "old_route_step_ms": {"median": round(step_ms, 5), "runs": [round(v, 5) for v in talker_ms],
                             "what": "eager talker stage (layers + codec head) of a one-row decode step at a ~30-token context"},
       "sizes": []}
p16 = None
for S in sizes:
    eng.prefill_profile(1, S, 1)                                  # this shape's first launches (and the long workspace)
    runs = [eng.prefill_profile(1, S, a.reps) for _ in range(3)]
    ms = float(np.median(runs))
    if S == 16:
        p16 = ms
    passes = (S + 127) // 128
    e = {"S": S, "prefill_ms": round(ms, 4), "runs_ms": [round(v, 4) for v in runs], "weight_passes": passes,
         "hbm_fraction_weights_only": round(passes * w_pass / (ms * 1e-3) / HBM_PEAK, 4)}
    rec["sizes"].append(e)
if p16 is None:
    p16 = float(np.median([eng.prefill_profile(1, 16, a.reps) for _ in range(3)]))
for e in rec["sizes"]:
    if e["S"] > 16:
        old = p16 + (e["S"] - 16) * step_ms
        e["old_route_ms"] = round(old, 3)
        e["speedup_vs_old_route"] = round(old / e["prefill_ms"], 2)
eng.close()
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
