"""numpy restatements of the speaking-rate stage (include/q3tts.h "speaking rate"), shared by the speed tests: the host rule counted
from its definition, the WSOLA arithmetic in float32 in the header's order, and the clip the GPU tests use."""
import numpy as np

N, HS, D = 720, 360, 240
LAGS = 2 * D + 1
SPEEDS = [500, 750, 1250, 1333, 1500, 2000]
PAD = D          # the earliest sample any frame reads is a_0 - D = -D
TAIL = 4 * N     # behind the clip: a_m <= n + 1 for every frame of a finished stretcher, plus D + N


def pos(S, m):
    return m * HS * S // 1000


def need(S, m):
    a = pos(S, m) + D + N
    return max(a, pos(S, m - 1) + D + HS + N) if m >= 1 else a


def frames_brute(S, R):
    """#{m : need(m) <= R}, counted over every m that could qualify (need(m) >= a_m, so m Hs S / 1000 - 1 <= R bounds them)"""
    m = np.arange(0, (R + 2) * 1000 // (HS * S) + 3, dtype=np.int64)
    a = m * HS * S // 1000
    nd = a + D + N
    nd[1:] = np.maximum(nd[1:], a[:-1] + D + HS + N)
    return int(np.count_nonzero(nd <= R))


def emitted(S, R, finished=False):
    return -(-1000 * R // S) if finished else HS * frames_brute(S, R)


def clip(n=9000):
    """the issue's clip: a vibrato harmonic tone with tremolo and a little noise, peak 0.5, float32"""
    tt = np.arange(n) / 24000.0
    rng = np.random.default_rng(3)
    f0 = 110 + 60 * np.sin(2 * np.pi * 1.3 * tt)
    ph = 2 * np.pi * np.cumsum(f0) / 24000.0
    x = sum((0.5 / k) * np.sin(k * ph + k) for k in range(1, 9))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * tt)) + 0.05 * rng.standard_normal(n)
    return (x * (0.5 / np.abs(x).max())).astype(np.float32)


def padded(x, dtype):
    return np.concatenate([np.zeros(PAD, dtype), np.asarray(x, dtype), np.zeros(TAIL, dtype)])


def wsola32(x, S, w):
    """the whole finished clip in float32, the header's order: vectorised over the lags, a loop over i, four accumulators
    -> (samples, offsets)"""
    x = np.asarray(x, np.float32)
    n = x.size
    T = -(-1000 * n // S)
    F = -(-T // HS)
    xp = padded(x, np.float32)
    w = np.asarray(w, np.float32)
    y = np.zeros(F * HS, np.float32)
    offs = np.zeros(F, np.int32)
    p_prev = -HS
    for m in range(F):
        a = pos(S, m)
        t = xp[PAD + p_prev + HS: PAD + p_prev + HS + N]
        region = xp[PAD + a - D: PAD + a + D + N]
        acc = np.zeros((4, LAGS), np.float32)
        for i in range(N):
            acc[i & 3] = acc[i & 3] + t[i] * region[i: i + LAGS]
        c = (acc[0] + acc[1]) + (acc[2] + acc[3])
        lag = int(np.argmax(c))     # the first of equal maxima: the smallest delta
        y[m * HS: (m + 1) * HS] = (w[HS:] * t[:HS]) + (w[:HS] * region[lag: lag + HS])
        offs[m] = lag - D
        p_prev = a + lag - D
    return y[:T], offs
