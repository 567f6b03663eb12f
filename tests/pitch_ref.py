"""numpy restatements of the pitch stage (include/q3tts.h "pitch"), shared by the pitch tests: the host rule, the period search in
float32 in the header's order, the grains in float32 (or, over the same marks, in float64), the synthetic voiced signals and the two
measurements the property tests make (fundamental, strongest line near the second formant)."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

PMIN, PMAX, PU, W = 48, 400, 120, 240
LAGS = PMAX - PMIN + 3            # lags Pmin - 1 .. Pmax + 1
REACH = W + PMAX + 1
GATE = PMAX // 2 + REACH
LA = PMAX + GATE - 1
FRAC = 20
VOICED2, OCTAVE2, FLOOR = np.float32(0.25), np.float32(0.81), np.float32(0.0625)
RATIOS = [794, 1260, 1498]
F0S = [90, 140, 180]


def emitted(R, finished=False):
    return R if finished else max(0, R - LA)


def ratio(cents):
    return int(math.floor(1000.0 * 2.0 ** (cents / 1200.0) + 0.5))


_win = {}


def window(P):
    """h[m] = (float)(0.5 - 0.5 cos(pi m / P)), m < 2 P, formed in double by the C library's cos as the host table is"""
    if P not in _win:
        _win[P] = np.array([0.5 - 0.5 * math.cos(math.pi * m / P) for m in range(2 * P)], np.float64)
    return _win[P]


def _sum4(prod):
    """rows of products -> (s0 + s1) + (s2 + s3), s_q the ascending float32 sum over i = q mod 4 (cumsum adds one after the other)"""
    s = [np.cumsum(prod[:, q::4], axis=1, dtype=np.float32)[:, -1] for q in range(4)]
    return (s[0] + s[1]) + (s[2] + s[3])


class Analysis:
    """the analysis marks of a finished signal: period and voicing of the mark at a, searched once and kept"""

    def __init__(self, x):
        self.x = np.asarray(x, np.float32)
        self.n = self.x.size
        self.known = {}

    def mark(self, a):
        if a not in self.known:
            self.known[a] = self._search(a)
        return self.known[a]

    def _search(self, a):
        if a < W or a + REACH > self.n:
            return PU, False
        region = self.x[a - W: a + REACH]
        t = region[: 2 * W]
        X = sliding_window_view(region[PMIN - 1:], 2 * W)          # [LAGS][2 W]
        with np.errstate(all="ignore"):
            num = _sum4(t[None, :] * X)
            el = _sum4(X * X)
            et = _sum4((t * t)[None, :])[0]
            den = np.float32(et) * el
            sc = np.where(den > 0, (num * np.abs(num)) / np.where(den > 0, den, np.float32(1)), np.float32(0)).astype(np.float32)
            cand = np.zeros(LAGS, bool)
            cand[1:-1] = (sc[1:-1] >= sc[:-2]) & (sc[1:-1] >= sc[2:])
            if not cand.any():
                return PU, False
            best = sc[cand].max()
            if not best >= VOICED2:
                return PU, False
            ok = cand & (sc >= OCTAVE2 * best)
        return PMIN - 1 + int(np.flatnonzero(ok)[0]), True


def marks(an, r):
    """the synthesis marks of the finished signal -> [(t, a, P, voiced)] in order"""
    n = an.n
    out = []
    a_cur, (P_cur, v_cur) = 0, an.mark(0)
    s = 0
    while True:
        t = s >> FRAC
        if not t < n + PMAX:
            break
        while a_cur + P_cur <= t:
            a_cur += P_cur
            P_cur, v_cur = an.mark(a_cur)
        a, P, v = a_cur, P_cur, v_cur
        if a_cur + P_cur - t <= t - a_cur:
            a = a_cur + P_cur
            P, v = an.mark(a)
        out.append((t, a, P, v))
        s += ((P * 1000) << FRAC) // r if v else P << FRAC
    return out


def synth(an, mk, dtype=np.float32):
    """the grains of the marks, added in mark order, and the division.  float32: the stage's arithmetic bit for bit.  float64: the same
    marks with exact windows, the yardstick of the float32 rounding"""
    n = an.n
    pad = 2 * PMAX
    xp = np.concatenate([np.zeros(pad, dtype), an.x.astype(dtype), np.zeros(3 * PMAX, dtype)])
    acc = np.zeros(n + 3 * PMAX + pad, dtype)
    ws = np.zeros_like(acc)
    for t, a, P, _ in mk:
        h = window(P).astype(dtype)
        k0 = t - P
        m0 = max(0, -k0)                                  # outputs below 0 do not exist
        g = h[m0:] * xp[pad + a - P + m0: pad + a + P]
        acc[k0 + m0: t + P] = acc[k0 + m0: t + P] + g
        ws[k0 + m0: t + P] = ws[k0 + m0: t + P] + h[m0:]
    floor = dtype(FLOOR)
    with np.errstate(all="ignore"):
        return (acc[:n] / np.where(ws[:n] > floor, ws[:n], floor)).astype(dtype)


def psola32(x, r, an=None):
    an = Analysis(x) if an is None else an
    return synth(an, marks(an, r), np.float32)


def voiced(f0, n=24000):
    """the issue's signal: a pulse train at f0 through two resonators at 700 Hz and 1 800 Hz, peak 0.5, float32"""
    sr = 24000.0
    e = np.zeros(n)
    pos = np.arange(0, n, sr / f0)
    e[np.floor(pos).astype(int)] = 1.0
    y = np.zeros(n)
    for fc, bw in ((700.0, 90.0), (1800.0, 140.0)):
        rr = math.exp(-math.pi * bw / sr)
        c1, c2 = 2 * rr * math.cos(2 * math.pi * fc / sr), -rr * rr
        z = np.zeros(n)
        z1 = z2 = 0.0
        for i in range(n):
            v = e[i] + c1 * z1 + c2 * z2
            z[i] = v
            z2, z1 = z1, v
        y += z
    return (y * (0.5 / np.abs(y).max())).astype(np.float32)


def noise(n=24000, seed=5):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def fundamental(y):
    """Hz: the first autocorrelation peak within 0.9 of the maximum (lags Pmin .. Pmax), over the middle half of the signal"""
    y = np.asarray(y, np.float64)
    n = y.size
    z = y[n // 4: 3 * n // 4]
    z = z - z.mean()
    f = np.fft.rfft(z, 2 * z.size)
    ac = np.fft.irfft(f * np.conj(f))[: PMAX + 2]
    lags = np.arange(PMIN, PMAX + 1)
    peak = (ac[lags] >= ac[lags - 1]) & (ac[lags] >= ac[lags + 1])
    top = ac[lags][peak].max()
    L = int(lags[peak & (ac[lags] >= 0.9 * top)][0])
    return 24000.0 / L


def formant_line(y, lo=1400.0, hi=2300.0):
    """Hz: the strongest spectral line in lo .. hi over the middle half of the signal (Hann window)"""
    y = np.asarray(y, np.float64)
    n = y.size
    z = y[n // 4: 3 * n // 4]
    sp = np.abs(np.fft.rfft(z * np.hanning(z.size)))
    fr = np.fft.rfftfreq(z.size, 1.0 / 24000.0)
    sel = (fr >= lo) & (fr <= hi)
    return float(fr[sel][np.argmax(sp[sel])])
