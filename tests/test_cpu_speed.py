"""The host side of the speaking-rate stage (include/q3tts.h "speaking rate"), checkable without a GPU: the window against its formula,
the host rule q3tts_speed_emitted against a count made from the rule's definition (tests/speed_ref.py), the refusals, and the surface
(header, exports, ctypes signatures, Python wrappers, TTSEngine, the CLI's help).  What the kernel computes is checked on the GPU:
tests/test_gpu_speed.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import q3tts
from speed_ref import D, HS, N, emitted, need

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_SPEEDS = [500, 501, 999, 1001, 1333, 2000]
NEW = ("q3tts_speed_emitted", "q3tts_speed_window", "q3tts_speed_begin", "q3tts_speed_push_batch_host", "q3tts_speed_end",
       "q3tts_codec_stream_set_speed", "q3tts_engine_set_speed")


def test_window():
    w = q3tts.speed_window()
    assert w.dtype == np.float32 and w.shape == (N,)
    i = np.arange(N, dtype=np.float64)
    assert np.abs(w.astype(np.float64) - (0.5 - 0.5 * np.cos(2 * np.pi * i / N))).max() <= 1e-7
    assert np.abs(w[:HS].astype(np.float64) + w[HS:].astype(np.float64) - 1.0).max() <= 2.0 ** -22
    assert w[0] == 0.0 and w[HS] == 1.0


@pytest.mark.parametrize("S", RULE_SPEEDS)
def test_emitted_rule(S):
    E = [q3tts.speed_emitted(S, R) for R in range(0, 5001)]
    F = [q3tts.speed_emitted(S, R, True) for R in range(0, 5001)]
    for R in range(0, 5001):
        assert E[R] == emitted(S, R), (S, R)
        assert F[R] == -(-1000 * R // S), (S, R)             # finished: ceil(1000 n / S)
        assert E[R] <= F[R], (S, R)                          # never above the finished count of this clip
        if R:
            assert E[R] >= E[R - 1] and F[R] >= F[R - 1]     # monotone
        m = E[R] // HS                                       # frames ready: exactly those with need(m) <= R
        assert E[R] % HS == 0 and need(S, m) > R and (m == 0 or need(S, m - 1) <= R)
    assert E[N + D - 1] == 0 and E[N + D] == HS              # frame 0 needs a_0 + D + N samples
    # latency: need(F) > R gives E S / 1000 > R - (N + D + Hs), so what is held back is under 1000 (N + D + Hs) / S + 1 outputs
    assert all(F[R] - E[R] <= -(-1000 * (N + D + HS) // S) for R in range(0, 5001))


@pytest.mark.parametrize("S", RULE_SPEEDS)
def test_emitted_large_counts(S):
    for R in (2 ** 31 + 5, 86400000):
        e, f = q3tts.speed_emitted(S, R), q3tts.speed_emitted(S, R, True)
        assert e == emitted(S, R) and f == -(-1000 * R // S) and e <= f, (S, R)


def test_need_is_monotone():
    for S in RULE_SPEEDS + [1000]:
        nd = [need(S, m) for m in range(0, 400)]
        assert all(b >= a for a, b in zip(nd, nd[1:])), S


@pytest.mark.parametrize("S", [499, 2001, 0])
def test_speeds_refused_by_name(S):
    with pytest.raises(ValueError, match=str(S)):
        q3tts.speed_emitted(S, 100)
    with pytest.raises(ValueError, match=str(S)):
        q3tts.speed_emitted(S, 100, True)


def test_negative_counts_refused_by_name():
    for n in (-1, -(2 ** 40)):
        with pytest.raises(ValueError, match="negative"):
            q3tts.speed_emitted(750, n)
    assert q3tts.speed_emitted(750, 0) == 0 and q3tts.speed_emitted(750, 0, True) == 0


def test_surface():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW + ("q3tts_speed_last_error",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int64_t q3tts_speed_emitted\(int32_t speed_permille, int64_t n_received, int finished\);", hdr)
    assert re.search(r"int q3tts_speed_window\(float\* table, int64_t cap\);", hdr)
    assert re.search(r"int q3tts_speed_begin\(q3tts_engine\* e, int32_t speed_permille, int\* id\);", hdr)
    assert re.search(r"int q3tts_codec_stream_set_speed\(q3tts_engine\* e, int stream_id, int32_t speed_permille\);", hdr)
    assert re.search(r"int q3tts_engine_set_speed\(q3tts_engine\* e, int32_t speed_permille\);", hdr)
    assert "offsets_out" in hdr and "n_offsets" in hdr
    for formula in ("a_m = floor(m Hs S / 1000)", "c(delta) = (s0 + s1) + (s2 + s3)", "need(m) = max(a_m + D + N, a_{m-1} + D + Hs + N)",
                    "T = ceil(1000 n / S)", "starts from"):
        assert formula in hdr, formula               # the header holds the formulas in full, and the known limit of primed streams
    # no engine: refused like every other entry point
    i64 = ctypes.c_int64
    assert L.q3tts_speed_begin(None, 750, None) == -1
    assert L.q3tts_speed_push_batch_host(None, 1, None, None, None, None, None, i64(0), None, None, None) == -1
    assert L.q3tts_speed_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_speed(None, 0, 750) == -1
    assert L.q3tts_engine_set_speed(None, 750) == -1
    assert L.q3tts_speed_window(None, i64(720)) == -1
    small = np.zeros(719, np.float32)
    assert L.q3tts_speed_window(small.ctypes.data_as(ctypes.c_void_p), i64(719)) == -1
    # ctypes signatures of the host-only calls
    q3tts.speed_emitted(750, 10)
    q3tts.speed_window()
    Lb = q3tts.lib()
    assert Lb.q3tts_speed_emitted.argtypes == [ctypes.c_int32, ctypes.c_int64, ctypes.c_int] and Lb.q3tts_speed_emitted.restype == ctypes.c_int64
    assert Lb.q3tts_speed_window.argtypes == [ctypes.c_void_p, ctypes.c_int64]
    # Python wrappers
    for name in ("speed_begin", "speed_push_batch", "speed_end", "codec_stream_set_speed", "set_speed"):
        assert callable(getattr(q3tts.Engine, name)), name
    assert "speed" in inspect.signature(q3tts.Engine.codec_stream_begin).parameters
    for fn in (q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        assert "speed" in inspect.signature(fn).parameters
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_speed\(float speed\);", th)


def test_cli_help_names_speed():
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--speed" in r.stdout
