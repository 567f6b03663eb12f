"""The pitch stage without a GPU (include/q3tts.h "pitch"): the host rule and the ratio helper through the C-ABI, and
the properties of the numpy restatement of the stage's float32 arithmetic (tests/pitch_ref.py) on synthetic voiced signals, noise and
silence.  tests/test_gpu_pitch.py holds the kernel to this restatement bit for bit."""
import numpy as np
import pytest

import pitch_ref as R
import q3tts

# the float32 restatement against a float64 evaluation of the same marks on the noise clip: the largest difference the rounding of
# sum(h x) / sum(h) makes (measured: DESIGN.md 4o).  The unvoiced test allows four times as much.
NOISE_ROUNDING = 3.0e-8


def test_host_rule():
    assert R.LA == 1240 and R.GATE == 841
    prev = 0
    for n in list(range(0, 3000)) + [2 ** 31 + 5, 86400000]:
        e, f = q3tts.pitch_emitted(n), q3tts.pitch_emitted(n, True)
        assert e == R.emitted(n) == max(0, n - R.LA) and f == n and e <= f
        if n < 3000:
            assert e >= prev
            prev = e
    assert q3tts.pitch_emitted(2 ** 31 + 5) == 2 ** 31 + 5 - R.LA
    assert q3tts.pitch_emitted(86400000) == 86400000 - R.LA
    with pytest.raises(ValueError, match="negative"):
        q3tts.pitch_emitted(-1)


def test_ratio_helper():
    for cents, want in ((0, 1000), (1200, 2000), (-1200, 500), (400, 1260), (-400, 794), (700, 1498)):
        assert q3tts.pitch_ratio(cents) == want == R.ratio(cents)
    for bad in (1200.5, -1201, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cents"):
            q3tts.pitch_ratio(bad)


@pytest.fixture(scope="module")
def analyses():
    return {f0: R.Analysis(R.voiced(f0)) for f0 in R.F0S}


@pytest.mark.parametrize("f0", R.F0S)
def test_search_finds_the_period(analyses, f0):
    an = analyses[f0]
    R.marks(an, 1000)
    inner = [(a, P, v) for a, (P, v) in an.known.items() if 2400 <= a <= an.n - 2400]
    assert inner and all(v for _, _, v in inner)
    assert all(abs(P - 24000.0 / f0) <= 1.0 for _, P, _ in inner), sorted(set(P for _, P, _ in inner))


@pytest.mark.parametrize("r", R.RATIOS)
@pytest.mark.parametrize("f0", R.F0S)
def test_voiced_properties(analyses, f0, r):
    an = analyses[f0]
    y = R.psola32(an.x, r, an)
    assert y.dtype == np.float32 and y.size == an.n and np.isfinite(y).all()          # 3. length
    want = f0 * r / 1000.0
    got = R.fundamental(y)
    print("f0 %d r %d: fundamental %.2f Hz (want %.2f, %.2f %%)" % (f0, r, got, want, 100 * abs(got - want) / want))
    assert abs(got - want) <= 0.015 * want                                            # 1. f0 scaling
    line = R.formant_line(y)
    print("f0 %d r %d: strongest line %.1f Hz, harmonic spacing %.1f Hz, a resampling shift would give %.1f Hz" % (f0, r, line, want, 1.8 * r))
    assert abs(line - 1800.0) <= want                                                 # 2. formant preservation
    assert abs(1.8 * r - 1800.0) > want                                               # ... which a resampling shift would miss


def test_unvoiced_noise_comes_out_as_it_went_in():
    x = R.noise()
    an = R.Analysis(x)
    mk = R.marks(an, 1260)
    assert not any(v for _, _, _, v in mk)
    y32, y64 = R.synth(an, mk, np.float32), R.synth(an, mk, np.float64)
    assert np.abs(y64 - x.astype(np.float64)).max() < 1e-15
    shown = float(np.abs(y32.astype(np.float64) - y64).max())
    print("noise: float32 against float64 over the same marks: %.3g" % shown)
    assert shown <= NOISE_ROUNDING
    assert float(np.abs(y32.astype(np.float64) - x.astype(np.float64)).max()) <= 4 * NOISE_ROUNDING
    # every ratio gives the same samples: unvoiced marks move by their own period
    assert np.array_equal(y32, R.psola32(x, 794, an))


def test_silence():
    x = np.zeros(12000, np.float32)
    for r in (794, 1498):
        y = R.psola32(x, r)
        assert y.size == x.size and not np.isnan(y).any() and not y.any()
