"""Time of arming 64 slots behind one 64-row instruction at 0.6B dims (synthetic weights), two ways, between HIP events recorded on
the engine's stream (every begin entry returns after its work has completed, so the events bracket all of it, host staging included):

  parent's route — what q3tts_synthesize_instruct_host does at admission: every utterance's prompt is instruction rows + its own rows
                   (64 + 8), each one prefilled on its own through the long-prompt path (q3tts_slots_begin_prefixed with every
                   prefix_id == -1 is exactly Engine::slots_begin);
  shared route   — q3tts_prefix_create once (64 rows) + one q3tts_slots_begin_prefixed of the 64 own prompts behind it.

    python tools/prefix_bench.py [--slots 64] [--rows 64] [--reps 3] [--out profiles/prefix_share.txt]

Prints both times (median of --reps, after one untimed pass of each route) and their ratio."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))
import q3tts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=64)
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="")
a = ap.parse_args()

cfg = q3tts.default_config("0.6b")
B, P, S, H = a.slots, a.rows, 8, cfg.hidden
eng = q3tts.Engine(cfg, device=0, max_batch=B, max_ctx=256)
eng.fill_synthetic(seed=0)
rt = C.CDLL("libamdhip64.so.7")
rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
rt.hipEventSynchronize.argtypes = [C.c_void_p]
rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
ev0, ev1 = C.c_void_p(), C.c_void_p()
assert rt.hipEventCreate(C.byref(ev0)) == 0 and rt.hipEventCreate(C.byref(ev1)) == 0
stream = eng.stream   # a property

rng = np.random.default_rng(0)
ins = (rng.standard_normal((P, H)) * 0.1).astype(np.float32)
own = [(rng.standard_normal((S, H)) * 0.1).astype(np.float32) for _ in range(B)]
full = [np.concatenate([ins, o]) for o in own]
tr = [np.zeros((1, H), np.float32)] * B
sp = q3tts.Sampling(max_new_tokens=8)
slots = list(range(B))


def timed(fn):
    assert rt.hipEventRecord(ev0, stream) == 0
    fn()
    assert rt.hipEventRecord(ev1, stream) == 0 and rt.hipEventSynchronize(ev1) == 0
    ms = C.c_float(0)
    assert rt.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
    for s in slots:
        eng.slot_release(s)
    return float(ms.value)


def parent():
    eng.slots_begin_prefixed(slots, None, full, tr, sp, ignore_eos=True)


def shared():
    pid = eng.prefix_create(ins)
    eng.slots_begin_prefixed(slots, [pid] * B, own, tr, sp, ignore_eos=True)
    made.append(pid)


made = []
timed(parent)
timed(shared)
t_parent = [timed(parent) for _ in range(a.reps)]
t_shared = [timed(shared) for _ in range(a.reps)]
for pid in made:
    eng.prefix_release(pid)
eng.close()
mp, ms_ = float(np.median(t_parent)), float(np.median(t_shared))
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
lines = [
    "prefix_bench: %d slots behind a %d-row instruction, own prompts of %d rows, 0.6B dims, synthetic weights; parent commit %s + this change" % (B, P, S, commit),
    "parent's route (instruction repeated per utterance, %d long prefills of %d rows): %.3f ms  (runs: %s)" % (B, P + S, mp, ", ".join("%.3f" % v for v in t_parent)),
    "shared route (1 prefix_create of %d rows + 1 grouped begin of %d x %d rows):       %.3f ms  (runs: %s)" % (P, B, S, ms_, ", ".join("%.3f" % v for v in t_shared)),
    "ratio parent / shared: %.2f" % (mp / ms_),
]
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
