"""The host side of the output-level stage (include/q3tts.h "output level"), checkable without a GPU: q3tts_level_gain against its
formula, the host rule q3tts_level_emitted, the refusals, and the properties of the arithmetic on its numpy restatement
(tests/level_ref.py): cut-invariance, |y| <= T, and y = v bit for bit where nothing exceeds T.  What the kernel computes is checked
on the GPU: tests/test_gpu_level.py."""
import numpy as np
import pytest

import q3tts
from level_ref import CARRY, W, Stage, ceiling_f32, clip, emitted, level32


def test_gain_within_one_ulp_over_the_whole_range():
    for cb in range(-600, 401):
        g = q3tts.level_gain(cb)
        want = np.float32(10.0 ** (cb / 200.0))
        assert isinstance(g, np.float32)
        assert abs(float(g) - float(want)) <= float(np.spacing(want)), cb
    assert q3tts.level_gain(0) == np.float32(1.0)
    assert q3tts.level_gain(200) == np.float32(10.0) and q3tts.level_gain(-400) == np.float32(0.01)


@pytest.mark.parametrize("cb", [-601, 401, 10 ** 6])
def test_gain_refused_by_name(cb):
    with pytest.raises(ValueError, match=str(cb)):
        q3tts.level_gain(cb)
    with pytest.raises(ValueError, match=str(cb)):
        q3tts.level_emitted(cb, 900, 10)


@pytest.mark.parametrize("c", [-1, 1001])
def test_ceiling_refused_by_name(c):
    with pytest.raises(ValueError, match=str(c)):
        q3tts.level_emitted(0, c, 10)


def test_negative_counts_refused_by_name():
    with pytest.raises(ValueError, match="negative"):
        q3tts.level_emitted(60, 900, -1)


def test_emitted_rule():
    assert W == 128 and CARRY == 254
    for R in list(range(0, 300)) + [2 ** 31 + 5, 86400000]:
        for cb, c in ((60, 900), (0, 1), (-600, 1000)):
            assert q3tts.level_emitted(cb, c, R) == max(0, R - 127) == emitted(c, R), (R, c)
            assert q3tts.level_emitted(cb, c, R, True) == R
        assert q3tts.level_emitted(60, 0, R) == R and q3tts.level_emitted(60, 0, R, True) == R     # gain only: no latency
        assert q3tts.level_emitted(0, 0, R) == R                                                    # (0, 0): the same rule
    assert q3tts.level_emitted(0, 500, 127) == 0 and q3tts.level_emitted(0, 500, 128) == 1


def test_level_params_rounding():
    assert q3tts.level_params(None, None) == (0, 0)
    assert q3tts.level_params(6, 0.9) == (60, 900)
    assert q3tts.level_params(-3.04, 0.8996) == (-30, 900)      # nearest centibel, nearest permille
    assert q3tts.level_params(0.06, None) == (1, 0)
    with pytest.raises(ValueError, match="permille"):
        q3tts.level_params(0, 0.0004)


@pytest.fixture(scope="module")
def x():
    return clip()


PARAMS = [(60, 900), (0, 500), (-100, 1000), (400, 250)]


def test_the_test_clip_keeps_the_limiter_busy_but_not_always_on(x):
    """the clip tests/test_gpu_level.py holds the kernel against: s < 1 on 5 % .. 60 % of the restatement's samples"""
    assert x.size == 6000 and 0.39 < np.abs(x[np.abs(x) <= 0.4]).max() <= 0.4 and 1.0 < np.abs(x).max() <= 3.0
    for cb, c in PARAMS[:2]:
        s = level32(x, cb, c, want_s=True)[1]
        assert 0.05 <= np.count_nonzero(s < 1.0) / s.size <= 0.60, (cb, c)


@pytest.mark.parametrize("cb,c", PARAMS + [(60, 0)])
def test_restatement_is_cut_invariant(x, cb, c):
    whole = level32(x, cb, c)
    for step in (1, 127, 128, 129, 255, 1000):
        st, parts = Stage(cb, c), []
        if step == 1:
            ends = list(range(1, 400)) + [x.size]
        else:
            ends = list(range(step, x.size, step)) + [x.size]
        at = 0
        for b in ends:
            parts.append(st.push(x[at:b], finish=(b == x.size and step != 129)))
            at = b
        if step == 129:
            parts.append(st.push(x[:0], finish=True))          # the finish carries no samples
        y = np.concatenate(parts)
        assert np.array_equal(y.view(np.uint32), whole.view(np.uint32)), (cb, c, step)


@pytest.mark.parametrize("cb,c", PARAMS)
def test_restatement_never_exceeds_the_ceiling(x, cb, c):
    y, s = level32(x, cb, c, want_s=True)
    T = ceiling_f32(c)
    assert np.abs(y).max() <= T
    v = (q3tts.level_gain(cb) * x).astype(np.float32)
    # s[k] <= r[k]: the product alone already stays within one rounding of T, the clamp takes that away
    a = np.abs(v)
    r = np.where(a > T, T / np.maximum(a, np.float32(1e-30)), np.float32(1.0)).astype(np.float32)
    assert np.all(s <= r)


def test_restatement_is_transparent_below_the_ceiling(x):
    quiet = (x / np.abs(x).max() * np.float32(0.5)).astype(np.float32)          # |v| <= 0.5 g
    for cb, c in ((0, 500), (0, 1000), (60, 1000), (-100, 400)):
        v = (q3tts.level_gain(cb) * quiet).astype(np.float32)
        assert np.abs(v).max() <= ceiling_f32(c)
        y, s = level32(quiet, cb, c, want_s=True)
        assert np.all(s == np.float32(1.0))
        assert np.array_equal(y.view(np.uint32), v.view(np.uint32)), (cb, c)
    # and locally: a single over at k0 leaves every sample further than 127 away untouched
    z = quiet.copy()
    z[3000] = 2.5
    y = level32(z, 0, 500)
    far = np.abs(np.arange(z.size) - 3000) > 127
    assert np.array_equal(y[far].view(np.uint32), z[far].view(np.uint32))
    assert np.count_nonzero(y[~far] != z[~far]) > 200          # the gain dips over the whole look-ahead and release
    assert abs(float(y[3000])) <= 0.5
