"""The host side of PCM sinks (include/q3tts.h "audio out at the sink's rate"), checkable without a GPU: the plan q3tts_sink_plan returns
against a numpy restatement of its formula, the refusals, the host rule q3tts_sink_emitted, and the surface (header, exports, ctypes
signatures, Python wrappers, TTSEngine, the CLI's help).  What the kernel computes is checked on the GPU: tests/test_gpu_pcm_sink.py."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import q3tts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [4000, 8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 192000, 44101]
NEW = ("q3tts_sink_plan", "q3tts_sink_emitted", "q3tts_pcm_sink_begin", "q3tts_pcm_sink_push_batch_host", "q3tts_pcm_sink_end",
       "q3tts_codec_stream_set_sink", "q3tts_codec_stream_push_batch_any_host", "q3tts_engine_set_sink")


def plan_ref(rate):
    """the issue's formula in numpy: (L, M, half, taps, table in float64 before the float rounding)"""
    g = math.gcd(rate, 24000)
    L, M = rate // g, 24000 // g
    s = min(1.0, rate / 24000.0)
    H = 16.0 / s
    Hn = int(math.ceil(H))
    T = 2 * Hn
    f = 0.92 * s
    d = (np.arange(T, dtype=np.float64)[None, :] - Hn + 1) - np.arange(L, dtype=np.float64)[:, None] / L
    inside = np.abs(d) < H
    w = np.i0(10.0 * np.sqrt(np.where(inside, 1.0 - (d / H) ** 2, 0.0))) / np.i0(10.0)
    h = np.where(inside, f * np.sinc(f * d) * w, 0.0)
    h = h / h.sum(axis=1, keepdims=True)
    return L, M, Hn, T, h


@pytest.mark.parametrize("rate", RATES)
def test_plan_matches_the_formula(rate):
    L, M, half, taps, tab = q3tts.sink_plan(rate)
    rL, rM, rH, rT, ref = plan_ref(rate)
    assert (L, M, half, taps) == (rL, rM, rH, rT)
    assert tab.shape == (L, taps) and tab.dtype == np.float32
    assert np.max(np.abs(tab.astype(np.float64) - ref)) <= 1e-6
    assert np.max(np.abs(tab.astype(np.float64).sum(axis=1) - 1.0)) <= 2.0 ** -22
    assert np.abs(tab.astype(np.float64)).sum(axis=1).max() <= 2.004


def test_plan_sizes_of_the_table():
    sizes = {8000: (1, 96, 48), 16000: (2, 48, 24), 44100: (147, 32, 16), 48000: (2, 32, 16), 11025: (147, 70, 35), 4000: (1, 192, 96), 44101: (44101, 32, 16)}
    for rate, (L, T, Hn) in sizes.items():
        got = q3tts.sink_plan(rate, want_table=False)
        assert (got[0], got[3], got[2]) == (L, T, Hn), rate
    assert q3tts.sink_plan(24000)[:4] == (1, 1, 0, 0)   # pass-through: no filter


@pytest.mark.parametrize("rate", [3999, 192001, 191999, 0])
def test_rates_refused_by_name(rate):
    with pytest.raises(ValueError, match=str(rate)):
        q3tts.sink_plan(rate)
    with pytest.raises(ValueError, match=str(rate)):
        q3tts.sink_emitted(rate, 100)
    if rate == 191999:
        with pytest.raises(ValueError, match="table"):
            q3tts.sink_plan(rate)


def closed_form(rate, n, finished):
    L, M, Hn, _, _ = q3tts.sink_plan(rate, want_table=False)
    if rate == 24000:
        return n
    if finished:
        return -((-n * L) // M)
    return max(0, -((-(n - Hn) * L) // M))


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 44100, 48000, 4000, 192000])
def test_emitted_rule(rate):
    L, M, Hn, _, _ = q3tts.sink_plan(rate, want_table=False)
    E = [q3tts.sink_emitted(rate, n) for n in range(0, 3001)]
    F = [q3tts.sink_emitted(rate, n, True) for n in range(0, 3001)]
    for n in range(0, 3001):
        assert E[n] == closed_form(rate, n, False) and F[n] == closed_form(rate, n, True)
        if n:
            assert E[n] >= E[n - 1] and F[n] >= F[n - 1]
        assert E[n] <= F[n]                       # never above the finished count of this clip, nor (F monotone) of any longer one
        if E[n] > 0:                              # every emitted j has its last tap received ...
            j = E[n] - 1
            assert (j * M) // L + Hn <= n - 1
        assert (E[n] * M) // L + Hn > n - 1       # ... and the next one has not
        if F[n] > 0:                              # every finished output sits inside the clip, the next one does not
            assert ((F[n] - 1) * M) // L <= n - 1 and F[n] * M >= n * L


def test_emitted_large_counts_and_pass_through():
    hour = 86400000
    for rate in (8000, 44100, 48000, 192000, 44101):
        for n in (2 ** 31 + 5, hour):
            assert q3tts.sink_emitted(rate, n) == closed_form(rate, n, False)
            assert q3tts.sink_emitted(rate, n, True) == closed_form(rate, n, True)
    for n in (0, 1, 7, 2 ** 31 + 5):
        assert q3tts.sink_emitted(24000, n) == n and q3tts.sink_emitted(24000, n, True) == n
    with pytest.raises(ValueError):
        q3tts.sink_emitted(8000, -1)


def test_surface():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    L = ctypes.CDLL(q3tts.LIB_PATH)
    for name in NEW + ("q3tts_sink_last_error",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in q3tts.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"int q3tts_sink_plan\(int32_t rate, int32_t\* L, int32_t\* M, int32_t\* half, int32_t\* taps, float\* table, int64_t cap\);", hdr)
    assert re.search(r"int64_t q3tts_sink_emitted\(int32_t rate, int64_t n_received, int finished\);", hdr)
    assert re.search(r"typedef int \(\*q3tts_audio_any_cb\)\(void\* user, int utt, int frame_begin, int frame_end, const void\* pcm, int64_t n_samples, int finished\);", hdr)
    assert re.search(r"typedef struct \{ int32_t sample_rate; int32_t format; q3tts_audio_any_cb cb; void\* user; \} q3tts_sink;", hdr)
    assert re.search(r"int q3tts_engine_set_sink\(q3tts_engine\* e, const q3tts_sink\* sink\);", hdr)
    assert "starts from silence" in hdr   # the known limit of primed streams is written down
    # no engine: refused like every other entry point
    i64 = ctypes.c_int64
    assert L.q3tts_pcm_sink_begin(None, 8000, 1, None) == -1
    assert L.q3tts_pcm_sink_push_batch_host(None, 1, None, None, None, None, None, i64(0), None) == -1
    assert L.q3tts_pcm_sink_end(None, 0) == -1
    assert L.q3tts_codec_stream_set_sink(None, 0, 8000, 1) == -1
    assert L.q3tts_codec_stream_push_batch_any_host(None, 1, None, None, None, None, i64(0), None, None) == -1
    assert L.q3tts_engine_set_sink(None, None) == -1
    # ctypes signatures of the host-only calls
    q3tts.sink_plan(8000)
    q3tts.sink_emitted(8000, 10)
    Lb = q3tts.lib()
    assert Lb.q3tts_sink_emitted.argtypes == [ctypes.c_int32, ctypes.c_int64, ctypes.c_int] and Lb.q3tts_sink_emitted.restype == ctypes.c_int64
    assert len(Lb.q3tts_sink_plan.argtypes) == 7
    # Python wrappers
    for name in ("pcm_sink_begin", "pcm_sink_push_batch", "pcm_sink_end", "codec_stream_set_sink", "set_sink"):
        assert callable(getattr(q3tts.Engine, name)), name
    assert {"sample_rate", "dtype"} <= set(inspect.signature(q3tts.Engine.codec_stream_begin).parameters)
    assert "finish" in inspect.signature(q3tts.Engine.codec_stream_push_batch).parameters
    for fn in (q3tts.Engine.synthesize_stream, q3tts.Engine.synthesize_live):
        assert {"sample_rate", "dtype"} <= set(inspect.signature(fn).parameters)
    th = open(os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc", "tts_engine.h")).read()
    assert re.search(r"bool set_output_format\(int sample_rate, bool pcm16", th)


def test_cli_help_names_out_rate():
    cli = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--out-rate" in r.stdout
