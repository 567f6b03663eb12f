"""Plain-Python and numpy restatement of the loudness stage (include/q3tts.h "loudness", items 1 - 7), shared by the loudness tests:
the coefficients, the two recursions in IEEE double (Python floats) in the header's order, the integer energies, gate, gain and slew,
the float32 output ramp and the host rule; the clips the tests use; an independent statement of the two-gate integrated loudness."""
import math

import numpy as np

BLOCK = 2400
GATE = 4834272
NORM = 41231686041600.0            # 9600 * 2^32
UP = np.float32(10.0 ** (1.0 / 20.0))
DN = np.float32(10.0 ** (-1.0 / 20.0))
PARAMS = [(-160, 200, 0), (-230, 60, -100), (-100, 400, 400), (0, 0, 0)]      # the last: meter only


def coeffs(rate):
    """{ b0, b1, b2, a1, a2 } of the shelf, then of the high-pass"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    KQ, K2 = K / Q, K * K
    a0 = 1.0 + KQ + K2
    out = [(Vh + Vb * KQ + K2) / a0, 2.0 * (K2 - Vh) / a0, (Vh - Vb * KQ + K2) / a0, 2.0 * (K2 - 1.0) / a0, (1.0 - KQ + K2) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    KQ, K2 = K / Q, K * K
    a0 = 1.0 + KQ + K2
    return out + [1.0, -2.0, 1.0, 2.0 * (K2 - 1.0) / a0, (1.0 - KQ + K2) / a0]


C24 = coeffs(24000)


def emitted(target, R, finished=False):
    return R if target == 0 or finished else BLOCK * (R // BLOCK)


def _biquad(x, b0, b1, b2, a1, a2):
    """x: float64 array -> u, by ff = (b0 x[k] + b1 x[k-1]) + b2 x[k-2] (numpy: one rounded operation each) and the recursion
    u[k] = (ff - a2 u[k-2]) - a1 u[k-1] in Python floats"""
    xp = np.concatenate([np.zeros(2), x])
    with np.errstate(all="ignore"):
        ff = ((b0 * xp[2:] + b1 * xp[1:-1]) + b2 * xp[:-2]).tolist()
    u1 = u2 = 0.0
    out = ff
    for k, f in enumerate(ff):
        u = (f - a2 * u2) - a1 * u1
        out[k] = u
        u2, u1 = u1, u
    return np.array(out, np.float64)


def weighted(x):
    """v: the K-weighted signal of float32 x, in double"""
    u = _biquad(np.asarray(x, np.float32).astype(np.float64), *C24[:5])
    return _biquad(u, *C24[5:])


def energies(x):
    """E_b of every complete sub-block: int64"""
    v = weighted(x)
    with np.errstate(all="ignore"):
        z = v * v
        q = np.floor(np.where(z < 4.0, z, 4.0) * 4294967296.0).astype(np.int64)
    nb = q.size // BLOCK
    return q[: nb * BLOCK].reshape(nb, BLOCK).sum(axis=1, dtype=np.int64)


def gains(E, target, range_cb, start_cb):
    """G_b after every sub-block, float32; G_-1 = (float)10^(start_cb / 200)"""
    G = np.float32(math.pow(10.0, start_cb / 200.0))
    if len(E) == 0:
        return np.zeros(0, np.float32), G
    R = math.pow(10.0, range_cb / 200.0)
    lo = 1.0 / R
    PT = math.pow(10.0, (target / 10.0 + 0.691) / 10.0) if target != 0 else 0.0
    A = N = 0
    out = np.zeros(len(E), np.float32)
    Ei = [int(e) for e in E]
    for b in range(len(Ei)):
        if b >= 3:
            W = Ei[b - 3] + Ei[b - 2] + Ei[b - 1] + Ei[b]
            if W >= GATE:
                A += W
                N += 1
        T = G
        if N > 0 and target != 0:
            P = float(A) / (float(N) * NORM)
            d = math.sqrt(PT / P)
            d = lo if d < lo else (R if d > R else d)
            T = np.float32(d)
        g = max(T, G * DN)                   # float32 products (numpy scalars)
        G = np.float32(min(g, G * UP))
        out[b] = G
    return out, np.float32(math.pow(10.0, start_cb / 200.0))


def apply(x, Gs, G0, target):
    """y: float32; the ramp of item 6, the partial tail at the last gain"""
    x = np.asarray(x, np.float32)
    if target == 0:
        return x.copy()
    nb = x.size // BLOCK
    ramp = np.arange(BLOCK, dtype=np.float32) / np.float32(2400.0)
    prev = np.concatenate([[G0], Gs[:-1]]).astype(np.float32) if nb else np.zeros(0, np.float32)
    with np.errstate(all="ignore"):
        g = prev[:, None] + (Gs[:nb] - prev)[:, None] * ramp[None, :]
        y = np.empty_like(x)
        y[: nb * BLOCK] = (x[: nb * BLOCK].reshape(nb, BLOCK) * g).reshape(-1)
        y[nb * BLOCK:] = x[nb * BLOCK:] * (Gs[nb - 1] if nb else G0)
    assert y.dtype == np.float32 and g.dtype == np.float32
    return y


def stage(x, target, range_cb, start_cb):
    """the finished stage over the whole clip -> (y float32, E int64, G float32)"""
    E = energies(x)
    Gs, G0 = gains(E, target, range_cb, start_cb)
    return apply(x, Gs, G0, target), E, Gs


def lufs_integrated(E):
    """BS.1770's integrated loudness of the sub-block energies, stated on loudness values: block loudness l = -0.691 + 10 log10(z);
    absolute gate (the stage's integer threshold, -70 LUFS); relative gate 10 LU below the loudness of the mean of what passed"""
    E = np.asarray(E, np.int64)
    if E.size < 4:
        return -math.inf
    W = E[3:] + E[2:-1] + E[1:-2] + E[:-3]
    W = W[W >= GATE]
    if W.size == 0:
        return -math.inf
    z = W.astype(np.float64) / NORM
    gamma = -0.691 + 10.0 * math.log10(z.mean()) - 10.0
    keep = z[(-0.691 + 10.0 * np.log10(z)) > gamma]
    return -0.691 + 10.0 * math.log10(keep.mean()) if keep.size else -math.inf


def sine(seconds=5.0, amp=1.0, f=997.0):
    n = int(round(24000 * seconds))
    return (amp * np.sin(2.0 * math.pi * f * np.arange(n) / 24000.0)).astype(np.float32)


def speech_like(seconds=8.0, lufs=-17.0, seed=3):
    """amplitude-modulated harmonics with pauses, scaled so that its integrated loudness is `lufs`.  Every part repeats after 2 s, so
    the clip's last 4 s are as loud as the whole and a reading over them shows the stage's gain, not the clip's own drift"""
    n = int(24000 * seconds)
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    f0 = 120.0 + 20.0 * np.sin(2 * math.pi * 0.5 * t)
    ph = 2 * math.pi * np.cumsum(f0) / 24000.0
    y = sum(np.sin(h * ph + rng.uniform(0, 6.28)) / h for h in range(1, 16))
    env = 0.55 + 0.45 * np.sin(2 * math.pi * 3.0 * t)                       # syllables
    talk = ((t % 2.0) < 1.6).astype(np.float64)                              # a 0.4 s pause every 2 s
    y = (y * env * talk).astype(np.float32)
    have = lufs_integrated(energies(y))
    return (y * np.float32(10.0 ** ((lufs - have) / 20.0))).astype(np.float32)


def gpu_clip():
    """14 sub-blocks + 1000 samples: sub-blocks 5 - 9 near silence (the gate opens, closes and reopens), one 0.9 peak one sample
    either side of a sub-block edge"""
    n = 14 * BLOCK + 1000
    rng = np.random.default_rng(17)
    t = np.arange(n) / 24000.0
    x = 0.2 * np.sin(2 * math.pi * 220.0 * t) + 0.12 * np.sin(2 * math.pi * 1510.0 * t) + 0.05 * rng.standard_normal(n)
    x[5 * BLOCK: 10 * BLOCK] *= 1e-5
    x[3 * BLOCK - 1] = 0.9
    x[3 * BLOCK + 1] = -0.9
    return x.astype(np.float32)
