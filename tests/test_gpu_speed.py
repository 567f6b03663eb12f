"""The speaking-rate stage alone (q3tts_speed_begin / _push_batch_host / _end): 24 kHz float in, the same audio S / 1000 times as fast
out, whatever the cuts.  The kernel's arithmetic is fixed by the header, so the samples and every frame's offset are held bit for bit
against a float32 numpy restatement in the same order (tests/speed_ref.py: np.array_equal, no tolerance).  Independently, every frame's
search is repeated in float64 (plain dot products, plain arg-max) over the template the device used: the offsets must agree wherever
the float64 top-2 gap exceeds the bound of the fp32 sums' error, 2 gamma_N max_lag sum|t x| (gamma_N = N u / (1 - N u), u = 2^-24: each
c is within gamma_N sum|t x| of its exact value whatever the order of the N adds, so a larger gap cannot be reordered), at most 10 % of
a run's frames may fall under that bound, and the samples of agreeing frames are within 4 u max|x| of the float64 overlap-add (two
products and one add, w[i] + w[i + Hs] = 1).  Every cut pattern must give the same bits."""
import numpy as np
import pytest

import q3tts
from speed_ref import D, HS, LAGS, N, PAD, SPEEDS, clip, padded, pos, wsola32
from util import tiny_pair

pytestmark = pytest.mark.gpu

NS = 9000


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def x():
    return clip(NS)


def run(eng, x, S, ends, finish_with_last):
    """one stretcher, pushes ending at `ends` -> (samples, offsets); every push's length is checked against the host rule"""
    sid = eng.speed_begin(S)
    parts, offs, at, total = [], [], 0, 0
    n = len(x)
    for k, b in enumerate(ends):
        fin = k + 1 == len(ends) and finish_with_last
        out, of = eng.speed_push_batch([sid], [x[at:b]], [fin], want_offsets=True)
        total_after = q3tts.speed_emitted(S, b, fin)
        assert out[0].size == total_after - total, (S, k)          # a push's length is E(after) - E(before)
        assert of[0].size == -(-total_after // HS) - -(-total // HS), (S, k)
        total, at = total_after, b
        parts.append(out[0])
        offs.append(of[0])
    if not finish_with_last:
        out, of = eng.speed_push_batch([sid], [x[:0]], [True], want_offsets=True)
        assert out[0].size == q3tts.speed_emitted(S, n, True) - total
        parts.append(out[0])
        offs.append(of[0])
    eng.speed_end(sid)
    return np.concatenate(parts), np.concatenate(offs)


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """each speed in one push + finish: computed once, shared, never modified"""
    return {S: run(eng, x, S, [NS], True) for S in SPEEDS}


@pytest.fixture(scope="module")
def ref32(x):
    w = q3tts.speed_window()
    return {S: wsola32(x, S, w) for S in SPEEDS}


@pytest.mark.parametrize("S", SPEEDS)
def test_bit_exact_against_fp32_numpy(one_shot, ref32, S):
    y, offs = one_shot[S]
    ry, roffs = ref32[S]
    assert y.dtype == np.float32 and y.size == -(-1000 * NS // S)     # the duration, exactly
    assert np.array_equal(offs, roffs), (S, np.flatnonzero(offs != roffs)[:8])
    assert np.array_equal(y.view(np.uint32), ry.view(np.uint32)), S


@pytest.mark.parametrize("S", SPEEDS)
def test_independent_fp64_search(x, one_shot, S):
    y, offs = one_shot[S]
    w = q3tts.speed_window().astype(np.float64)
    xp = padded(x, np.float64)
    u = 2.0 ** -24
    gamma = N * u / (1 - N * u)
    F = offs.size
    exempt, p_prev, worst = [], -HS, 0.0
    for m in range(F):
        a = pos(S, m)
        t = xp[PAD + p_prev + HS: PAD + p_prev + HS + N]
        win = np.lib.stride_tricks.sliding_window_view(xp[PAD + a - D: PAD + a + D + N], N)   # [lag][i]
        assert win.shape == (LAGS, N)
        c = win @ t
        order = np.argsort(-c, kind="stable")
        gap = c[order[0]] - c[order[1]]
        bound = 2 * gamma * float((np.abs(win) * np.abs(t)).sum(axis=1).max())
        if gap > bound:
            assert offs[m] == order[0] - D, (S, m, int(offs[m]), int(order[0]) - D, gap, bound)
            blk = y[m * HS: (m + 1) * HS].astype(np.float64)
            lag = offs[m] + D
            ref = w[HS:HS + blk.size] * t[:blk.size] + w[:blk.size] * win[lag][:blk.size]
            worst = max(worst, float(np.abs(blk - ref).max()))
        else:
            exempt.append((m, int(offs[m]), int(order[0]) - D, float(gap), bound))
        p_prev = a + int(offs[m])        # the device's trajectory: each frame's search is checked on the template the device used
    print("speed %d: %d of %d frames exempt (gap under the fp32 bound): %s" % (S, len(exempt), F, exempt))
    print("speed %d: max |sample - fp64 overlap-add| on agreeing frames = %.3g (allowed %.3g)" % (S, worst, 4 * u * float(np.abs(x).max())))
    assert len(exempt) <= 0.10 * F
    assert worst <= 4 * u * float(np.abs(x).max())


def cut_patterns(S):
    rng = np.random.default_rng(S)
    rand, at = [], 0
    while at < NS:
        at = min(NS, at + int(rng.choice([1, 2, 5, 37, 250, 1111])))
        rand.append(at)
    return {
        "ones": (list(range(1, 301)) + [NS], True),                    # 300 pushes of 1 sample, then the rest
        "random": (rand, True),
        "short": (list(range(500, NS, 500)) + [NS], True),             # every push shorter than the carry (>= 2 D + N once frames run)
        "empty_mid": ([2000, 2000, 4500, NS], True),                   # an empty push in the middle
        "late_finish": ([1500, NS], False),                            # the finish carries no samples
    }


@pytest.mark.parametrize("S", SPEEDS)
def test_every_cut_gives_the_same_bits(eng, x, one_shot, S):
    for name, (ends, fin_last) in cut_patterns(S).items():
        y, offs = run(eng, x, S, ends, fin_last)
        assert np.array_equal(offs, one_shot[S][1]), (S, name)
        assert np.array_equal(y.view(np.uint32), one_shot[S][0].view(np.uint32)), (S, name)


def test_six_stretchers_in_one_call_equal_themselves_alone(eng, x, one_shot):
    sids = [eng.speed_begin(S) for S in SPEEDS]
    ends = [1, 700, 701, 3333, NS]
    parts, at = [[] for _ in SPEEDS], 0
    for k, b in enumerate(ends):
        outs = eng.speed_push_batch(sids, [x[at:b]] * len(SPEEDS), [k + 1 == len(ends)] * len(SPEEDS))
        for i, o in enumerate(outs):
            parts[i].append(o)
        at = b
    for i, S in enumerate(SPEEDS):
        assert np.array_equal(np.concatenate(parts[i]).view(np.uint32), one_shot[S][0].view(np.uint32)), S
        eng.speed_end(sids[i])


def test_silence_and_the_tie_rule(eng):
    z = np.zeros(3000, np.float32)
    for S in (500, 2000):
        y, offs = run(eng, z, S, [1000, 3000], True)
        assert y.size == -(-1000 * 3000 // S) and not y.view(np.uint32).any()      # zeros in, +0.0 out
        assert np.all(offs == -D)                                                  # every lag ties at 0: the smallest delta
    # an all-zero template in front of sound: frame 0's template is x[0 .. N) = 0, so delta_0 = -D whatever follows
    s = np.concatenate([np.zeros(N, np.float32), clip(3000)])
    y, offs = run(eng, s, 1250, [s.size], True)
    assert offs[0] == -D and np.abs(y).max() > 0.1


def test_refusals_leave_every_stretcher_where_it_was(eng, x, one_shot):
    for S in (499, 2001, 0):
        with pytest.raises(RuntimeError, match=str(S)):
            eng.speed_begin(S)
    with pytest.raises(RuntimeError, match="1000"):
        eng.speed_begin(1000)
    a, b = eng.speed_begin(750), eng.speed_begin(1500)
    first = eng.speed_push_batch([a, b], [x[:4000], x[:4000]])
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.speed_push_batch([a, a], [x[:10], x[:10]])
    with pytest.raises(RuntimeError, match="no such stretcher"):
        eng.speed_push_batch([a, 4000], [x[:10], x[:10]])
    rest = eng.speed_push_batch([a, b], [x[4000:], x[4000:]], [True, True])
    assert np.array_equal(np.concatenate([first[0], rest[0]]), one_shot[750][0])
    assert np.array_equal(np.concatenate([first[1], rest[1]]), one_shot[1500][0])
    with pytest.raises(RuntimeError, match="finished"):
        eng.speed_push_batch([a], [x[:10]])
    eng.speed_end(a)
    eng.speed_end(b)
