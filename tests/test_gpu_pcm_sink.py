"""The sink stage alone (q3tts_pcm_sink_begin / _push_batch_host / _end): 24 kHz float in, the sink's rate and format out, whatever the
cuts.  Float output is held against a numpy fp64 fold of the library's own table over the same input, within the standard bound for an
fp32 sum of T products in any order, gamma_T * sum|h| * max|x| with gamma_T = T u / (1 - T u), u = 2^-24, computed here from the table;
int16 output within 1 LSB of the CLI's rule applied to that fold, and bit for bit equal to the rule applied to the sink's own float
output.  Every cut pattern must give the same bits (np.array_equal)."""
import numpy as np
import pytest

import q3tts
from util import tiny_pair

pytestmark = pytest.mark.gpu

N = 6000
RATES = [8000, 11025, 16000, 44100, 48000]


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def x():
    rng = np.random.default_rng(7)
    a = rng.uniform(-1.0, 1.0, N).astype(np.float32)
    a[1000:1040] = 1.0     # two runs at full scale: the sinc's overshoot reaches the clip
    a[3000:3040] = -1.0
    return a


def s16_rule(v):
    """save_wav16: clip to [-1, 1], then (int16_t)(v * 32767.0f), truncating; in float32 like the C code"""
    v = np.clip(np.asarray(v, np.float32), np.float32(-1.0), np.float32(1.0))
    return np.trunc(v * np.float32(32767.0)).astype(np.int16)


def fold64(x, rate, n_out):
    """y[j] = sum_t tab[p][t] x[kc - half + 1 + t] in float64 over the library's float table, zeros outside the clip"""
    L, M, half, taps, tab = q3tts.sink_plan(rate)
    j = np.arange(n_out, dtype=np.int64)
    kc, p = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(half, np.float64), x.astype(np.float64), np.zeros(half + 1, np.float64)])
    idx = (kc + 1)[:, None] + np.arange(taps)[None, :]          # kc - half + 1 + t, shifted by the half zeros in front
    return (tab.astype(np.float64)[p] * xp[idx]).sum(axis=1), tab


def cut_patterns(rate):
    L, M, half, taps, _ = q3tts.sink_plan(rate, want_table=False)
    carry = 2 * half + -(-M // L)
    rng = np.random.default_rng(rate)
    rand, at = [], 0
    while at < N:
        at = min(N, at + int(rng.choice([1, 2, 5, 37, 250, 1111])))
        rand.append(at)
    short = list(range(carry - 1, N, carry - 1)) + [N]             # every push shorter than the carry
    mid = [2000, 2000, 4500, N]                                    # an empty push in the middle
    return {
        "one": ([N], True),
        "ones": (list(range(1, 301)) + [N], True),
        "random": (rand, True),
        "short": (short, True),
        "empty_mid": (mid, True),
        "late_finish": ([1500, N], False),                         # the finish carries no samples
    }


def run(eng, x, rate, dtype, ends, finish_with_last):
    sid = eng.pcm_sink_begin(rate, dtype)
    parts, at, total = [], 0, 0
    for k, b in enumerate(ends):
        last = k + 1 == len(ends)
        fin = last and finish_with_last
        out = eng.pcm_sink_push_batch([sid], [x[at:b]], [fin])[0]
        total_after = q3tts.sink_emitted(rate, b, fin)
        assert out.size == total_after - total, (rate, k)          # a push's length is E(after) - E(before)
        if b == at and not fin:
            assert out.size == 0
        total, at = total_after, b
        parts.append(out)
    if not finish_with_last:
        out = eng.pcm_sink_push_batch([sid], [x[:0]], [True])[0]
        assert out.size == q3tts.sink_emitted(rate, at, True) - total
        parts.append(out)
    eng.pcm_sink_end(sid)
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """each rate and format in one push + finish: computed once, shared, never modified"""
    return {(r, d): run(eng, x, r, d, [N], True) for r in RATES for d in ("float32", "int16")}


@pytest.mark.parametrize("rate", RATES)
def test_float_against_the_fp64_fold(eng, x, one_shot, rate):
    L, M, half, taps, _ = q3tts.sink_plan(rate, want_table=False)
    y = one_shot[(rate, "float32")]
    assert y.dtype == np.float32 and y.size == -(-N * L // M)
    ref, tab = fold64(x, rate, y.size)
    u = 2.0 ** -24
    bound = taps * u / (1 - taps * u) * float(np.abs(tab.astype(np.float64)).sum(axis=1).max()) * float(np.abs(x).max())
    err = float(np.max(np.abs(y.astype(np.float64) - ref)))
    print("rate %d: max |float - fp64 fold| = %.3g, bound %.3g" % (rate, err, bound))
    assert err <= bound
    assert np.max(np.abs(ref)) > 1.0        # the overshoot does reach the clip


@pytest.mark.parametrize("rate", RATES)
def test_int16_rule(eng, x, one_shot, rate):
    y, s = one_shot[(rate, "float32")], one_shot[(rate, "int16")]
    assert s.dtype == np.int16 and s.size == y.size
    assert np.array_equal(s, s16_rule(y))                          # the kernel's conversion is the CLI's rule on the same float
    ref, _ = fold64(x, rate, y.size)
    exact = np.trunc(np.clip(ref, -1.0, 1.0) * 32767.0)
    assert np.max(np.abs(s.astype(np.int64) - exact.astype(np.int64))) <= 1
    assert s.max() == 32767 and s.min() == -32767                  # clipped, not wrapped


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_every_cut_gives_the_same_bits(eng, x, one_shot, rate, dtype):
    for name, (ends, fin_last) in cut_patterns(rate).items():
        got = run(eng, x, rate, dtype, ends, fin_last)
        assert got.dtype == one_shot[(rate, dtype)].dtype and np.array_equal(got, one_shot[(rate, dtype)]), (rate, dtype, name)


def test_mixed_sinks_in_one_call_equal_themselves_alone(eng, x, one_shot):
    keys = [(r, d) for r in RATES for d in ("float32", "int16")]
    sids = [eng.pcm_sink_begin(r, d) for r, d in keys]
    ends = [1, 700, 701, 3333, N]
    parts, at = [[] for _ in keys], 0
    for k, b in enumerate(ends):
        outs = eng.pcm_sink_push_batch(sids, [x[at:b]] * len(keys), [k + 1 == len(ends)] * len(keys))
        for i, o in enumerate(outs):
            parts[i].append(o)
        at = b
    for i, key in enumerate(keys):
        assert np.array_equal(np.concatenate(parts[i]), one_shot[key]), key
        eng.pcm_sink_end(sids[i])


def test_pass_through_and_24k_int16(eng, x):
    sid, s16 = eng.pcm_sink_begin(24000, "float32"), eng.pcm_sink_begin(24000, "int16")
    at = 0
    for b in [1, 2, 500, 500, 4097, N]:
        f, s = eng.pcm_sink_push_batch([sid, s16], [x[at:b], x[at:b]], [b == N, b == N])
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), x[at:b].view(np.uint32))   # the input's bits, no latency
        assert np.array_equal(s, s16_rule(x[at:b]))                                                     # only the conversion runs
        at = b
    eng.pcm_sink_end(sid)
    eng.pcm_sink_end(s16)


def test_refusals_leave_every_sink_where_it_was(eng, x):
    with pytest.raises(RuntimeError, match="3999"):
        eng.pcm_sink_begin(3999, "float32")
    with pytest.raises(RuntimeError, match="191999"):
        eng.pcm_sink_begin(191999, "int16")
    a, b = eng.pcm_sink_begin(8000, "float32"), eng.pcm_sink_begin(16000, "int16")
    first = eng.pcm_sink_push_batch([a, b], [x[:1000], x[:1000]])
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.pcm_sink_push_batch([a, a], [x[:10], x[:10]])
    with pytest.raises(RuntimeError, match="no such sink"):
        eng.pcm_sink_push_batch([a, 4000], [x[:10], x[:10]])
    rest = eng.pcm_sink_push_batch([a, b], [x[1000:], x[1000:]], [True, True])
    one_a, one_b = run(eng, x, 8000, "float32", [N], True), run(eng, x, 16000, "int16", [N], True)
    assert np.array_equal(np.concatenate([first[0], rest[0]]), one_a) and np.array_equal(np.concatenate([first[1], rest[1]]), one_b)
    with pytest.raises(RuntimeError, match="finished"):
        eng.pcm_sink_push_batch([a], [x[:10]])
    eng.pcm_sink_end(a)
    eng.pcm_sink_end(b)
