"""The tone stage alone (q3tts_tone_begin / _push_batch_host / _end): 24 kHz float in, as many samples out through a cascade of
biquads, whatever the cuts.  The kernel's arithmetic is fixed by the header — every fp64 operation a single rounded one in a fixed
order, nothing rounded between sections, subnormals kept — so the samples (uint32 views) are held bit for bit against the plain-Python
restatement (tests/tone_ref.py: np.array_equal, no tolerance) fed the library's own coefficients: in one push, in pushes of 1, 2 and 3
samples throughout, in pushes cut around the kernel's segment length, with a finish of its own, for clips shorter than the pipeline is
deep, for 1, 2, 5 and 8 sections, and for stages of different depth and length that share a launch."""
import os
import re

import numpy as np
import pytest

import q3tts
import tone_ref as R
from util import tiny_pair

pytestmark = pytest.mark.gpu

SEG = int(re.search(r"kToneSegment = (\d+);", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leaxer-qwen3-tts_amd", "csrc",
                                                                 "q3_audio.h")).read()).group(1))   # the samples k_tone stages at a time
CASES = dict(R.SECTIONS, underflow=R.UNDERFLOW)


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def clip():
    x = R.gpu_clip()
    assert x.size == 20000 and x.max() == 1.0 and x.min() == -1.0
    return x


@pytest.fixture(scope="module")
def ref(clip):
    """the restatement over the whole clip, per section set: computed once, shared, never modified"""
    return {k: R.cascade(clip, q3tts.tone_coeffs(s)) for k, s in CASES.items()}


def run(eng, x, sections, ends, finish_with_last=True):
    """one stage, pushes ending at `ends` -> samples; every push's length is checked against the host rule n_out == n_in"""
    sid = eng.tone_begin(sections)
    ys, at = [], 0
    for k, b in enumerate(ends):
        y = eng.tone_push_batch([sid], [x[at:b]], [k + 1 == len(ends) and finish_with_last])[0]
        assert y.dtype == np.float32 and y.size == b - at, (k, y.size, b - at)
        ys.append(y)
        at = b
    if not finish_with_last:
        y = eng.tone_push_batch([sid], [x[:0]], [True])[0]        # a finish of its own with n_in = 0: nothing is flushed
        assert y.size == 0
        with pytest.raises(RuntimeError, match="finished"):
            eng.tone_push_batch([sid], [x[:1]])
    eng.tone_end(sid)
    return np.concatenate(ys) if ys else np.zeros(0, np.float32)


def same(y, want):
    return y.size == want.size and np.array_equal(y.view(np.uint32), want.view(np.uint32))


def where(y, want):
    return (y.size, want.size) if y.size != want.size else np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))[:8]


def test_the_zero_run_passes_through_the_subnormals(clip, ref):
    """on the CPU: the restatement's state goes through the double subnormals to exact zero inside the zero run, and its output through
    the float subnormals, so a kernel that flushes either is caught by test_one_push_bit_exact[underflow]"""
    y, tiny = R.cascade(clip[:R.ZERO1], q3tts.tone_coeffs(R.UNDERFLOW), want_state=True)
    z = y[R.ZERO0:R.ZERO1]
    n_sub = int(np.count_nonzero((z != 0) & (np.abs(z) < np.finfo(np.float32).tiny)))
    print("smallest non-zero state", tiny, "float-subnormal outputs", n_sub, "last non-zero output at", int(np.flatnonzero(z)[-1]))
    assert 0.0 < tiny < np.finfo(np.float64).tiny and n_sub > 16 and not z[-1000:].any()
    assert same(y, ref["underflow"][:R.ZERO1])


@pytest.mark.parametrize("case", list(CASES))
def test_one_push_bit_exact(eng, clip, ref, case):
    y = run(eng, clip, CASES[case], [clip.size])
    assert np.isfinite(y).all() and np.abs(y).max() > 0.001           # not silence (the underflow pair attenuates by 40 dB)
    assert same(y, ref[case]), where(y, ref[case])


@pytest.mark.parametrize("step", [1, 2, 3])
def test_pushes_shorter_than_the_history(eng, clip, ref, step):
    """pushes of 1, 2 and 3 samples throughout the clip with 8 sections (noise, sine, impulses, steps, the zero run and every multiple of
    the segment length included): every push is shorter than the pipeline is deep, and the first two than the biquad's history; and
    the same around the start of the zero run with the pair that underflows"""
    for case, a, b in ((8, 0, clip.size), ("underflow", R.ZERO0 - 200, R.ZERO0 + 1300)):
        sid = eng.tone_begin(CASES[case])
        eng.tone_push_batch([sid], [clip[:a]])
        got = [eng.tone_push_batch([sid], [clip[k:min(k + step, b)]])[0] for k in range(a, b, step)]
        eng.tone_end(sid)
        assert all(g.size == min(step, b - k) for g, k in zip(got, range(a, b, step)))
        y = np.concatenate(got)
        assert same(y, ref[case][a:b]), (case, where(y, ref[case][a:b]))


@pytest.mark.parametrize("cut", [SEG - 1, SEG, SEG + 1])
def test_pushes_cut_around_the_segment_length(eng, clip, ref, cut):
    ends = list(range(cut, clip.size, cut)) + [clip.size]
    for case in (1, 8):
        y = run(eng, clip, CASES[case], ends)
        assert same(y, ref[case]), (case, where(y, ref[case]))


def test_a_finish_of_its_own(eng, clip, ref):
    y = run(eng, clip, CASES[5], [7, 5000, clip.size], finish_with_last=False)
    assert same(y, ref[5]), where(y, ref[5])
    sid = eng.tone_begin(CASES[2])                                   # and a stage that finishes having received nothing
    assert eng.tone_push_batch([sid], [clip[:0]], [True])[0].size == 0
    eng.tone_end(sid)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
def test_clips_shorter_than_the_pipeline(eng, clip, n):
    x = clip[6598:6598 + n]                                          # the two impulses
    want = R.cascade(x, q3tts.tone_coeffs(CASES[8]))
    assert np.count_nonzero(want) > 0 or n < 3
    y = run(eng, x, CASES[8], [n])
    assert same(y, want), where(y, want)
    y = run(eng, x, CASES[8], list(range(1, n + 1)))                 # and sample by sample
    assert same(y, want), where(y, want)


def test_stages_of_different_depth_share_a_launch(eng, clip, ref):
    """four stages with 1, 2, 5 and 8 sections, pushes of different lengths in every call, one of them empty in each call but the
    first; the state left by the call before is read from the other half"""
    keys = [1, 2, 5, 8]
    sids = [eng.tone_begin(CASES[k]) for k in keys]
    ends = [[3, 3, 4000, 20000], [SEG + 5, 9000, 9000, 20000], [1, SEG, 2 * SEG + 1, 20000], [6000, 6001, 20000, 20000]]
    at, got = [0] * 4, [[] for _ in keys]
    for c in range(4):
        xs = [clip[at[i]:ends[i][c]] for i in range(4)]
        assert c == 0 or any(x.size == 0 for x in xs)
        out = eng.tone_push_batch(sids, xs, [c == 3] * 4)
        for i in range(4):
            assert out[i].size == xs[i].size, (c, i)
            got[i].append(out[i])
            at[i] = ends[i][c]
    for s in sids:
        eng.tone_end(s)
    for i, k in enumerate(keys):
        y = np.concatenate(got[i])
        assert same(y, ref[k]), (k, where(y, ref[k]))


def test_refusals(eng, clip):
    for bad, name in (([(0, 300, 0, 707)], "section 0 kind 0"), ([(1, 300, 0, 707), (2, 19, 0, 707)], "section 1 freq_hz 19"),
                      ([(5, 300, 241, 707)], "section 0 gain_cb 241"), ([(1, 300, 10, 707)], "section 0 gain_cb 10 centibels must be 0"),
                      ([(3, 300, 0, 99)], "section 0 q_permille 99"), ([(1, 300, 0, 707)] * 9, "9 sections")):
        with pytest.raises(RuntimeError, match=name):
            eng.tone_begin(bad)
    with pytest.raises(RuntimeError, match="0 sections"):
        eng.tone_begin([])
    with pytest.raises(RuntimeError, match="no such tone stage"):
        eng.tone_push_batch([4000], [clip[:4]])
    sid = eng.tone_begin("rumble")
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.tone_push_batch([sid, sid], [clip[:4], clip[:4]])
    eng.tone_end(sid)
