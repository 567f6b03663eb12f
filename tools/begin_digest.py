"""Bits of every way of beginning utterances in slots, as text: a refactor of the begin family (csrc/q3_begin.cpp, q3_begin_plan.h) must
leave this output byte-identical, which the oracle tests' 2e-4 would not notice if it changed which prompts share a pass.  Nothing timed.

    Q3TTS_LIB=<the other build's libq3tts_hip.so> python tools/begin_digest.py > a.txt;  python tools/begin_digest.py > b.txt;  cmp a.txt b.txt

One engine of the `medium` test config (synthetic weights, max_batch 8, max_ctx 256, greedy sampling) runs a fixed list of begins; per
begin and slot it prints a SHA-256 of the slot's armed logits and last hidden row, the slot's codes after 4 decode steps, and the pool's
free pages right after the begin.  The slots are released between cases.  profiles/begin_digest.txt is the recorded output."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("leaxer-qwen3-tts_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import q3_oracle as qo  # noqa: E402
import q3tts  # noqa: E402
from util import Hip, to_q3cfg  # noqa: E402

LENS, SLOTS = [17, 40, 3, 70, 25], [5, 0, 3, 6, 2]      # tests/test_gpu_ragged_prefill.py's ragged case
PREFIX, FORCED = [40, 65, 0, 40, 130], [0, 31, 7, 1, 60]

cfg = to_q3cfg(qo.config_medium())
eng = q3tts.Engine(cfg, device=0, max_batch=8, max_ctx=256)
eng.fill_synthetic(seed=0)
H, V = cfg.hidden, cfg.vocab
sp = q3tts.Sampling(top_k=1, max_new_tokens=8)


def rows(seed, n):
    return (np.random.default_rng(seed).standard_normal((n, H)) * 0.1).astype(np.float32)


def codes(seed, n):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, cfg.sub_vocab, (n, cfg.n_groups)).astype(np.int64)
    c[:, 0] = rng.integers(0, min(cfg.vocab, cfg.suppress_begin), n)
    return c


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def report(name, slots):
    free = eng.kv_pool_info()[2]
    armed = [sha(*eng.slot_logits(s)) for s in slots]
    eng.decode_steps(4)
    for s, d in zip(slots, armed):
        print("%s slot %d free %d logits %s codes %s" % (name, s, free, d, " ".join(str(v) for v in eng.slot_codes(s).reshape(-1))))
    for s in slots:
        eng.slot_release(s)


def plain(name, slots, lens):
    own = [rows(100 + i, n) for i, n in enumerate(lens)]
    if len(slots) == 1:
        eng.slot_begin(slots[0], own[0], rows(2, 1), sp, seed=1, ignore_eos=True)
    else:   # every prefix id -1: exactly Engine::slots_begin
        eng.slots_begin_prefixed(slots, None, own, [rows(2, 1)] * len(slots), sp, seed=1, ignore_eos=True)
    report(name, slots)


pid = {P: eng.prefix_create(rows(6000 + P, P)) for P in (40, 65, 130)}

plain("plain 5 consecutive S=8", [0, 1, 2, 3, 4], [8] * 5)
plain("plain scattered S=8", [5, 0, 3], [8] * 3)
plain("plain 2 slots S=3", [0, 1], [3] * 2)
plain("plain lengths 8,8,17,8", [0, 1, 2, 3], [8, 8, 17, 8])
for F0 in (5, 31):   # 13 rows: the short path; 39: the chunk path
    eng.slot_begin(2, rows(200, 8), rows(3, 4), sp, seed=1, ignore_eos=True, prefix_codes=codes(300 + F0, F0))
    report("forced S=8 F0=%d" % F0, [2])
own4 = [rows(400 + i, 8) for i in range(4)]
ids4 = [pid[40], pid[65], None, pid[40]]
eng.slots_begin_prefixed([1, 4, 2, 7], ids4, own4, [rows(2, 1)] * 4, sp, seed=1, ignore_eos=True)
report("prefixed a,b,none,a S=8", [1, 4, 2, 7])
# The same four with the third carrying 7 forced frames.  No C entry passes forced frames to a many-member slots_begin_prefixed call
# (the job layer begins such a member on its own or through the ragged entry), so the member that would split the run is begun the way
# the run would begin it, on its own through the forced begin at its base, between the two pairs the run leaves
eng.slots_begin_prefixed([1, 4], ids4[:2], own4[:2], [rows(2, 1)] * 2, sp, seed=1, ignore_eos=True)
eng.slot_begin(2, own4[2], rows(3, 4), sp, seed=1, stream_id=2, ignore_eos=True, prefix_codes=codes(77, 7), prefix_id=pid[65])
eng.slots_begin_prefixed([7], [pid[40]], own4[3:], [rows(2, 1)], sp, seed=1, stream_ids=[3], ignore_eos=True)
report("prefixed a,b,forced behind b,a S=8", [1, 4, 2, 7])
eng.slots_begin_ragged([1, 4], own4[:2], [rows(2, 1)] * 2, sp, prefix_ids=ids4[:2], seed=1, ignore_eos=True)   # 16 rows: past mfma_min_rows, one chunk
report("ragged 2 x S=8 behind a,b", [1, 4])
eng.slots_begin_ragged([1, 4], [own4[0][:3], own4[1][:3]], [rows(2, 1)] * 2, sp, prefix_ids=ids4[:2], seed=1, ignore_eos=True)   # 6 rows: one at a time
report("ragged 2 x S=3 behind a,b (one at a time)", [1, 4])
eng.slot_begin(3, rows(501, 20), rows(2, 1), sp, seed=1, ignore_eos=True, prefix_id=pid[40])
report("prefixed one member S=20 behind a", [3])
eng.slots_begin_ragged([6], [rows(500, 20)], [rows(2, 1)], sp, prefix_ids=[pid[65]], seed=1, ignore_eos=True)   # n == 1: slots_begin_prefixed
report("ragged one member S=20 behind b", [6])
ownr = [rows(7000 + i, n) for i, n in enumerate(LENS)]
eng.slots_begin_ragged(SLOTS, ownr, [rows(2, 4)] * 5, sp, prefix_ids=[pid.get(P) for P in PREFIX],
                       prefix_codes=[codes(900 + i, f) if f else None for i, f in enumerate(FORCED)], seed=1, ignore_eos=True)
report("ragged lens/slots/prefix/forced", SLOTS)

hip = Hip()
lens = np.array([8, 8, 8, 3, 17], np.int32)
x = (np.random.default_rng(21).standard_normal((5, 17, H)) * 0.05).astype(np.float32)
x_d, lg_d, lh_d = hip.put(x), hip.alloc(5 * V * 4), hip.alloc(5 * H * 4)
eng.talker_prefill_dev(x_d, 5, 17, lens, lg_d, lh_d)
free = eng.kv_pool_info()[2]
lg, lh = hip.get(lg_d, (5, V), np.float32), hip.get(lh_d, (5, H), np.float32)
for b in range(5):
    print("talker_prefill_dev row %d len %d free %d logits %s state %s" % (b, lens[b], free, sha(lg[b], lh[b]), sha(*eng.slot_logits(b))))
    eng.slot_release(b)
hip.free()
eng.close()
