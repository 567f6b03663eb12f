"""The host rule of the streaming resampler (q3tts_resample_stream_emitted): how many output samples a stream at rate R has emitted once
it holds N samples.  A numpy restatement that emits E(after) - E(before) outputs per push, reading only samples it has received, must
equal q3tts_resample_host of the whole clip bit for bit, whatever the cuts.  No engine, no GPU; every comparison is np.array_equal."""
import math

import numpy as np
import pytest

import q3tts

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 384000, 23999, 24001]
LENGTHS = [1, 2, 3, 5, 17, 1000, 4097]
E = q3tts.resample_stream_emitted


def ratio_of(rate):
    return np.float64(24000) / np.float64(rate)


def tap(i, rate):
    """the lower input sample of output i, the one-shot's own expression: (size_t)((double)i / ratio)"""
    return int(np.float64(i) / ratio_of(rate))


def random_cuts(rng, n):
    cuts, at = [], 0
    while at < n:
        step = int(rng.choice([1, 1, 2, 3, 7, 40, 333, 2000]))
        cuts.append((at, min(at + step, n)))
        at = min(at + step, n)
    return cuts


def stream_resample(x, rate, cuts):
    """the stream on the host: the pushes x[a:b] of cuts, then the finish; per push the outputs the rule releases, formed from absolute
    indices and reading received samples only.  Returns (samples, per push: the samples before the push minus the smallest index it
    read, None for a push that emitted nothing)."""
    ratio = ratio_of(rate)
    out, reach, got = [], [], 0
    for total, fin in [(b, False) for _, b in cuts] + [(cuts[-1][1] if cuts else 0, True)]:
        before_n, before = got, E(rate, 24000, got, False)
        got = total
        after = E(rate, 24000, got, fin)
        assert after >= before
        if after == before:
            reach.append(None)
            continue
        pos = np.arange(before, after).astype(np.float64) / ratio
        k = pos.astype(np.int64)
        w = pos - k.astype(np.float64)
        k1 = np.minimum(k + 1, got - 1)
        assert k.min() >= 0 and k.max() < got                     # only what has arrived
        assert fin or k.max() + 1 <= got - 1                      # unclamped before the finish
        out.append((x[k].astype(np.float64) * (1.0 - w) + x[k1].astype(np.float64) * w).astype(np.float32))
        reach.append(before_n - int(k.min()))
    return (np.concatenate(out) if out else np.zeros(0, np.float32)), reach


@pytest.mark.parametrize("rate", RATES)
def test_stream_equals_one_shot_whatever_the_cuts(rate):
    rng = np.random.default_rng(rate)
    carry = math.ceil(rate / 24000) + 1
    for n in LENGTHS:
        x = rng.standard_normal(n).astype(np.float32)
        ref = q3tts.resample(x, rate, 24000)
        for trial in range(6):
            cuts = [(0, n)] if trial == 0 else random_cuts(rng, n)
            got, reach = stream_resample(x, rate, cuts)
            assert got.shape == ref.shape, (rate, n, cuts)
            assert np.array_equal(got, ref), (rate, n, cuts)
            # back-reach: a push never reads further behind the previous total than the carry holds
            assert all(r is None or r <= carry for r in reach), (rate, n, cuts, reach, carry)


@pytest.mark.parametrize("rate", RATES)
def test_monotone_and_never_above_a_longer_clip(rate):
    prev = 0
    for n in range(0, 400):
        e = E(rate, 24000, n, False)
        assert e >= prev and e <= E(rate, 24000, n, True)
        prev = e
        for m in (n, n + 1, n + 2, n + 17, n + 1000):
            assert e <= E(rate, 24000, m, True), (n, m)
        # taps: every emitted output has both taps received unclamped; the next one does not, or lies beyond the clip's length
        if e > 0:
            assert tap(e - 1, rate) + 1 <= n - 1
        if n >= 2 and e < E(rate, 24000, n, True):
            assert tap(e, rate) + 1 > n - 1
    assert E(rate, 24000, 0, False) == 0 and E(rate, 24000, 0, True) == 0 and E(rate, 24000, 1, False) == (1 if rate == 24000 else 0)


def test_finish_is_the_one_shot_length_and_equal_rates_pass_through():
    for rate in RATES + [1, 7, 383999]:
        for n in (LENGTHS + [0, 24000, 99999] if rate >= 8000 else [0, 1, 2, 17]):          # 17 samples at 1 Hz are 408 000 outputs
            x = np.zeros(n, np.float32)
            assert E(rate, 24000, n, True) == q3tts.resample(x, rate, 24000).size, (rate, n)
    for n in (0, 1, 5, 2 ** 31 + 5):
        assert E(24000, 24000, n, False) == n and E(24000, 24000, n, True) == n
        assert E(16000, 16000, n, False) == n
    with pytest.raises(ValueError):
        E(0, 24000, 5)
    with pytest.raises(ValueError):
        E(8000, 24000, -1)


def test_truncation_case_96k_two_then_one():
    # both taps of output 0 are there after 2 samples, but the one-shot of the 3 samples has floor(0.75) = 0 outputs
    assert tap(0, 96000) + 1 <= 2 - 1
    assert E(96000, 24000, 2, False) == 0 and E(96000, 24000, 3, False) == 0 and E(96000, 24000, 3, True) == 0
    x = np.array([0.5, -0.25, 0.125], np.float32)
    got, _ = stream_resample(x, 96000, [(0, 2), (2, 3)])
    assert got.size == 0 and q3tts.resample(x, 96000, 24000).size == 0


@pytest.mark.parametrize("rate,n", [(8000, 2 ** 31 + 5), (44100, 2 ** 31 + 5), (96000, 2 ** 31 + 5), (384000, 2 ** 31 + 5),
                                    (384000, 3600 * 384000), (48000, 3600 * 48000), (23999, 3600 * 23999)])
def test_large_indices(rate, n):
    carry = math.ceil(rate / 24000) + 1
    prev = E(rate, 24000, n - 3, False)
    for m in range(n - 2, n + 4):
        e = E(rate, 24000, m, False)
        full = E(rate, 24000, m, True)
        assert full == int(np.float64(m) * ratio_of(rate))
        assert prev <= e <= full
        assert e > 0 and tap(e - 1, rate) + 1 <= m - 1
        if e < full:
            assert tap(e, rate) + 1 > m - 1
        for longer in (m + 1, m + 5, m + 100000):
            assert e <= E(rate, 24000, longer, True)
        # back-reach of the push that brought the stream from m - 1 to m samples
        if e > prev:
            assert (m - 1) - tap(prev, rate) <= carry, (m, prev, carry)
        prev = e
