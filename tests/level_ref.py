"""A numpy restatement of the output-level stage's arithmetic (include/q3tts.h "output level"): float32 operations in the header's
order, integers for the window sum.  g comes from q3tts.level_gain, so the restatement multiplies by the very float the device uses.
`Stage` is the carried-state form (pushes of any length, E(R) = max(0, R - 127) until finished); `level32` is a whole clip at once."""
import numpy as np

import q3tts

W = 128                     # look-ahead window
CARRY = 2 * W - 2           # values of v a limiter carries
TILE = 1024                 # outputs of one workgroup of k_level (kLevelTile, csrc/q3_common.h)


def ceiling_f32(ceiling_permille):
    return np.float32(ceiling_permille / 1000.0)


def emitted(ceiling_permille, n_received, finished=False):
    return n_received if ceiling_permille == 0 or finished else max(0, n_received - (W - 1))


def _limit(v, T, k0, k1, n_total):
    """y[k0 .. k1) and s[k0 .. k1) from v[0 .. n_total) (r = 1 outside)"""
    lo, hi = k0 - (W - 1), k1 + (W - 1)                    # v[lo .. hi) is all these outputs read
    vv = np.zeros(hi - lo, np.float32)
    a, b = max(lo, 0), min(hi, n_total)
    if b > a:
        vv[a - lo: b - lo] = v[a:b]
    av = np.abs(vv)
    r = np.ones(vv.size, np.float32)
    over = av > T
    r[over] = T / av[over]                                 # float32 / float32: correctly rounded
    m = np.lib.stride_tricks.sliding_window_view(r, W).min(axis=1)        # m[j], j from lo
    q = np.floor(m * np.float32(65536.0)).astype(np.int64)
    S = np.lib.stride_tricks.sliding_window_view(q, W).sum(axis=1)        # S[k], k from k0
    assert S.size == k1 - k0 and S.max(initial=0) <= 2 ** 23
    s = S.astype(np.float32) * np.float32(2.0 ** -23)
    y = np.minimum(np.maximum(vv[W - 1: W - 1 + (k1 - k0)] * s, -T), T).astype(np.float32)
    return y, s


def level32(x, gain_cb, ceiling_permille, want_s=False):
    """the whole clip through a finished stage -> y (and s, all ones for gain only)"""
    x = np.ascontiguousarray(x, np.float32)
    v = (q3tts.level_gain(gain_cb) * x).astype(np.float32)
    if ceiling_permille == 0:
        return (v, np.ones(v.size, np.float32)) if want_s else v
    y, s = _limit(v, ceiling_f32(ceiling_permille), 0, x.size, x.size) if x.size else (v, np.ones(0, np.float32))
    return (y, s) if want_s else y


class Stage:
    """the carried-state form: keeps all of v (a restatement, not an implementation) and emits by the host rule"""

    def __init__(self, gain_cb, ceiling_permille):
        self.g, self.c = q3tts.level_gain(gain_cb), ceiling_permille
        self.v = np.zeros(0, np.float32)
        self.n_out = 0

    def push(self, x, finish=False):
        x = np.ascontiguousarray(x, np.float32)
        self.v = np.concatenate([self.v, (self.g * x).astype(np.float32)])
        e = emitted(self.c, self.v.size, finish)
        k0, self.n_out = self.n_out, e
        if self.c == 0:
            return self.v[k0:e].copy()
        if e == k0:
            return np.zeros(0, np.float32)
        # unfinished, output k < R - 127 reads v up to k + 127 < R: what lies beyond n_total is never looked at
        return _limit(self.v, ceiling_f32(self.c), k0, e, self.v.size)[0]


def clip(n=6000, seed=7):
    """seeded noise at amplitude 0.4 with bursts of up to 3.0"""
    rng = np.random.default_rng(seed)
    x = (0.4 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    for at in rng.integers(0, n, 14):
        ln = int(rng.integers(1, 40))
        x[at: at + ln] = (rng.uniform(1.0, 3.0) * rng.uniform(-1.0, 1.0, x[at: at + ln].size)).astype(np.float32)
    return x
