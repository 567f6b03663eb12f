"""Bits of every decode path of the vocoder, as text: a refactor of csrc/q3_codec.cpp (the one-shot decode, the whole-job front, the single
and the batched push, priming) must leave this output byte-identical, which the tests' 2e-5 would not notice if a launch moved.  Nothing
is timed.

    Q3TTS_LIB=<the other build's libq3tts_hip.so> python tools/codec_digest.py > a.txt;  python tools/codec_digest.py > b.txt;  cmp a.txt b.txt

Two engines with synthetic weights.  A: the `tiny` test config (head size 16: the batched push takes the per-stream attention launch;
window 4, K / V buffers of 64 rows).  B: 0.6B vocoder dims, as tests/test_gpu_stream_batch.py's `full` fixture (the windowed stream
attention).  Per case it prints a SHA-256 of every PCM array returned, and after every streaming call the streams' codec_stream_info.
profiles/codec_digest.txt is the recorded output."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("leaxer-qwen3-tts_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import q3_oracle as qo  # noqa: E402
import q3tts  # noqa: E402
from util import to_q3cfg  # noqa: E402


def sha(a):
    a = np.ascontiguousarray(a)
    return "%s[%d] %s" % (a.dtype, a.size, hashlib.sha256(a.tobytes()).hexdigest())


def run(name, eng, full):
    G, CB = eng.cfg.n_groups, eng.cfg.cd_codebook
    ctxB = 12   # Engine::codec_stage_b_context() of both configs (tests/test_cpu_codec_plan.py)

    def codes(seed, n):
        return np.random.default_rng(seed).integers(0, CB, (n, G)).astype(np.int64)

    def say(case, arrays, sids=()):
        for i, a in enumerate(arrays):
            print("%s %s pcm %d %s" % (name, case, i, sha(a)))
        for s in sids:
            print("%s %s stream %d info %s" % (name, case, s, " ".join(str(v) for v in eng.codec_stream_info(s))))

    def batched(case, lens_per_call, seed, prime=None):
        """streams primed with prime[i] frames (None: not primed), then one batched push per entry of lens_per_call"""
        k = len(lens_per_call[0])
        total = [(prime[i] if prime else 0) + sum(call[i] for call in lens_per_call) for i in range(k)]
        cs = [codes(seed + i, t) for i, t in enumerate(total)]
        sids = [eng.codec_stream_begin(max(t, 1)) for t in total]
        at = [0] * k
        if prime:
            eng.codec_stream_prime_batch(sids, [c[:p] for c, p in zip(cs, prime)])
            at = list(prime)
            say(case + " primed %s" % (prime,), [], sids)
        for call in lens_per_call:
            out = eng.codec_stream_push_batch(sids, [c[a:a + n] for c, a, n in zip(cs, at, call)])
            at = [a + n for a, n in zip(at, call)]
            say(case + " push %s" % (call,), out, sids)
        for s in sids:
            eng.codec_stream_end(s)

    if full:
        say("one-shot F=3", [eng.codec_decode(codes(1, 3))])
        batched("two streams", [(3, 1), (1, 2)], 10)
        batched("two streams", [(1, 1)], 20, prime=(2, 80))
        return
    for F in (1, 9):
        say("one-shot F=%d" % F, [eng.codec_decode(codes(F, F))])
    say("decode_batch (1, 9, 4)", eng.codec_decode_batch([codes(30 + i, n) for i, n in enumerate((1, 9, 4))]))
    say("chunked 9 by 4, left_context 9 (pushes)", [eng.codec_decode_chunked(codes(40, 9), 4, 9)])
    say("chunked 9 by 4, left_context 2 (windowed range decode)", [eng.codec_decode_chunked(codes(40, 9), 4, 2)])
    c68 = codes(50, 68)
    sid, at = eng.codec_stream_begin(68), 0
    for n in (1, 7, 30, 30):   # the last one makes the 64-row K / V buffer slide
        say("single push %d" % n, [eng.codec_stream_push(sid, c68[at:at + n])], [sid])
        at += n
    eng.codec_stream_end(sid)
    # stream 1 is younger than the look-back of the stages behind the transformer when the second call comes: two left-context groups
    batched("three streams", [(5, 0, 2), (2, 3, 0)], 60)
    c3 = codes(70, 3)
    sid = eng.codec_stream_begin(8, sample_rate=8000, dtype="int16")
    say("sink 8 kHz int16 push 3", eng.codec_stream_push_batch([sid], [c3]), [sid])
    say("sink 8 kHz int16 finish", eng.codec_stream_push_batch([sid], [c3[:0]], finish=[True]), [sid])
    eng.codec_stream_end(sid)
    batched("three streams", [(2, 2, 2)], 80, prime=(0, 2, ctxB + 5))
    H = eng.cfg.hidden
    rows = (np.random.default_rng(90).standard_normal((9, H)) * 0.1).astype(np.float32)
    eng.slot_begin(0, rows[:8], rows[8:], q3tts.Sampling(top_k=1, max_new_tokens=8), seed=1, ignore_eos=True)
    eng.decode_steps(4)
    eng.slots_codec_prime([0], [2])
    for fb, fe, pcm in eng.slots_codec_decode_new([0]):
        print("%s slot 0 primed 2, decode_new frames [%d, %d) %s" % (name, fb, fe, sha(pcm)))
    eng.slot_release(0)


eng = q3tts.Engine(to_q3cfg(qo.config_tiny()), device=0, max_batch=2, max_ctx=128)
eng.fill_synthetic(seed=0)
run("A", eng, False)
eng.close()
eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=512)
eng.fill_synthetic(seed=0)
run("B", eng, True)
eng.close()
