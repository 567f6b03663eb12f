"""G.711 in numpy: the rules of include/q3tts.h "G.711" restated, vectorised, with floor(log2) taken in floating point (exact for the
integers below 2^15 it sees) where the library counts leading zeros.  Both laws are sign-magnitude codes on int16."""
import numpy as np


def _mag(s):
    s = np.asarray(s).astype(np.int32)
    return s, np.abs(s)


def _ilog2(v):
    return np.floor(np.log2(np.maximum(v, 1).astype(np.float64))).astype(np.int32)


def mu_enc(s):
    s, mag = _mag(s)
    m = np.minimum(mag, 32635) + 132
    e = _ilog2(m) - 7
    mant = (m >> (e + 3)) & 15
    return ((~(np.where(s < 0, 0x80, 0) | (e << 4) | mant)) & 0xFF).astype(np.uint8)


def a_enc(s):
    s, mag = _mag(s)
    a = np.minimum(mag, 32767) >> 3
    low = a < 32
    e = np.where(low, 0, _ilog2(a) - 4)
    mant = np.where(low, a >> 1, (a >> e) & 15)
    return ((np.where(s >= 0, 0x80, 0) | (e << 4) | mant) ^ 0x55).astype(np.uint8)


def mu_dec(b):
    u = ~np.asarray(b).astype(np.int32) & 0xFF
    e, mant = (u >> 4) & 7, u & 15
    m = (((mant << 3) + 132) << e) - 132
    return np.where(u & 0x80, -m, m).astype(np.int16)


def a_dec(b):
    x = np.asarray(b).astype(np.int32) ^ 0x55
    e, mant = (x >> 4) & 7, x & 15
    m = np.where(e == 0, (mant << 4) + 8, ((mant << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(x & 0x80, m, -m).astype(np.int16)


ENC = {"mulaw": mu_enc, "alaw": a_enc}
DEC = {"mulaw": mu_dec, "alaw": a_dec}


def s16_rule(v):
    """the engine's int16 rule: clip to [-1, 1], then (int16_t)(v * 32767.0f), truncating; in float32 like the C code"""
    v = np.clip(np.asarray(v, np.float32), np.float32(-1.0), np.float32(1.0))
    return np.trunc(v * np.float32(32767.0)).astype(np.int16)
