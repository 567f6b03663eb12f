"""The tone stage without a GPU (include/q3tts.h "tone"): the coefficients through the C-ABI against the numpy
restatement (tests/tone_ref.py) and against the cookbook's closed forms, their stability over the whole parameter grid, every
refusal with its text, the spec strings and presets, and a proof that the GPU test's clip tells three plausible wrong
implementations from the right one.  tests/test_gpu_tone.py holds the kernel to the restatement bit for bit."""
import numpy as np
import pytest

import q3tts
import tone_ref as R

FREQS, QS, GAINS = (20, 300, 2500, 11000), (100, 707, 10000), (-240, -30, 30, 240)
GRID = [(kind, f, g, q) for kind in (R.HP, R.LP, R.LS, R.HS, R.PEAK) for f in FREQS for q in QS
        for g in ((0,) if kind in (R.HP, R.LP) else GAINS)]            # a high- or low-pass takes no gain


def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_coefficients_against_the_restatement():
    worst, at = 0, None
    for s in GRID:
        got, want = q3tts.tone_coeffs([s])[0], R.coeffs([s])[0]
        for i in range(5):
            if ulps(got[i], want[i]) > worst:
                worst, at = ulps(got[i], want[i]), (s, i)
    print("largest distance between the library's and numpy's coefficients: %d ulp" % worst, at)
    # Measured: 0 ulp at every one of the 168 grid points x 5 coefficients (glibc's and numpy's sin / cos / pow / sqrt agree on all of
    # them here), so 8 x the measured distance is 0: the two must agree exactly.  Two libms that differ would show here, and only here:
    # the filter's bit-exactness rests on q3tts_tone_coeffs alone.
    assert worst <= 8 * 0
    assert q3tts.tone_coeffs(R.SECTIONS[8]).shape == (8, 5)
    assert np.array_equal(q3tts.tone_coeffs(R.SECTIONS[5]), q3tts.tone_coeffs("telephone"))


def closed_form_deviations(coeffs_of):
    """the largest relative deviation from each of the cookbook's closed forms over the grid (absolute where the form is 0)"""
    d = {}
    for kind, f, g, q in GRID:
        c, lin = coeffs_of((kind, f, g, q)), 10.0 ** (g / 200.0)
        def put(k, v):
            d[k] = max(d.get(k, 0.0), float(v))
        if kind == R.PEAK:
            put("peak at f0", abs(R.response(c, f) / lin - 1.0))
        elif kind == R.LS:
            put("low shelf at DC", abs(R.response(c, 0.0) / lin - 1.0))
        elif kind == R.HS:
            put("high shelf at 12 kHz", abs(R.response(c, 12000.0) / lin - 1.0))
        else:
            put("|H(f0)| = Q", abs(R.response(c, f) / (q / 1000.0) - 1.0))
            put("high-pass at DC" if kind == R.HP else "low-pass at 12 kHz", R.response(c, 0.0 if kind == R.HP else 12000.0))
            put("high-pass at 12 kHz" if kind == R.HP else "low-pass at DC", abs(R.response(c, 12000.0 if kind == R.HP else 0.0) - 1.0))
    return d


def test_closed_forms_on_the_librarys_coefficients():
    own = closed_form_deviations(lambda s: R.coeffs([s])[0])           # what numpy shows on its own coefficients: the forms' conditioning
    got = closed_form_deviations(lambda s: q3tts.tone_coeffs([s])[0])
    for k in sorted(own):
        print("%-22s numpy's own %.3g, the library's %.3g" % (k, own[k], got[k]))
        assert got[k] <= 100.0 * own[k], k
    # the deviations measured here: |H(f0)| = Q 3.8e-12, low shelf at DC 3.0e-11 (20 Hz, Q 10: 1 - cos(w0) cancels), peak 2.6e-13,
    # low-pass at DC 3.2e-12, high shelf at 12 kHz 1.2e-14, high-pass at 12 kHz 5.6e-16, and exactly 0 where the form is 0
    assert own["low shelf at DC"] < 1e-9 and own["|H(f0)| = Q"] < 1e-9 and own["high-pass at DC"] == 0.0 and own["low-pass at 12 kHz"] == 0.0


def test_every_section_is_stable():
    edges = [(kind, f, g, q) for kind in (R.HP, R.LP, R.LS, R.HS, R.PEAK) for f in (20, 11000) for q in (100, 10000)
             for g in ((0,) if kind in (R.HP, R.LP) else (-240, 240))]
    for s in GRID + edges:
        b0, b1, b2, a1, a2 = q3tts.tone_coeffs([s])[0]
        assert abs(a2) < 1.0 and abs(a1) < 1.0 + a2, s                 # the stability triangle


def test_refusals():
    ok = (R.PEAK, 1000, 0, 707)
    for j in (0, 3):                                                   # the section's index is named
        for field, col, values, unit in (("kind", 0, (0, 6, -1), ""), ("freq_hz", 1, (19, 11001, 0, -300), " Hz"),
                                         ("gain_cb", 2, (-241, 241), " centibels"), ("q_permille", 3, (99, 10001, 0), "")):
            for v in values:
                bad = list(ok)
                bad[col] = v
                with pytest.raises(ValueError, match=r"^tone: section %d %s %d%s is " % (j, field, v, unit)):
                    q3tts.tone_coeffs([ok] * j + [tuple(bad)])
    for kind in (R.HP, R.LP):
        with pytest.raises(ValueError, match=r"^tone: section 1 gain_cb 5 centibels must be 0 for a high-pass or a low-pass$"):
            q3tts.tone_coeffs([ok, (kind, 300, 5, 707)])
    for n in (0, 9):
        with pytest.raises(ValueError, match=r"^tone: %d sections is outside 1 \.\. 8$" % n):
            q3tts.tone_coeffs([ok] * n)
    for edge in ((R.HP, 20, 0, 100), (R.LP, 11000, 0, 10000), (R.LS, 20, -240, 100), (R.HS, 11000, 240, 10000)):
        assert np.isfinite(q3tts.tone_coeffs([edge])).all()
    with pytest.raises(ValueError, match="integers"):
        q3tts.tone_coeffs([(1, 300.5, 0, 707)])


def test_spec_strings_and_presets():
    assert q3tts.tone_sections("hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707").tolist() == [[1, 300, 0, 707], [5, 2500, 30, 1000], [2, 3400, 0, 707]]
    assert q3tts.tone_sections("ls:200:-4.5:0.5,hs:6000:2:10").tolist() == [[3, 200, -45, 500], [4, 6000, 20, 10000]]
    assert q3tts.tone_sections("telephone").tolist() == [list(s) for s in R.SECTIONS[5]]
    for name in ("rumble", "presence", "warm"):
        s = q3tts.tone_sections(name)
        assert 1 <= s.shape[0] <= 8 and s.dtype == np.int32 and np.isfinite(q3tts.tone_coeffs(name)).all()
    for bad, text in (("hp:5:0.707", "section 0 freq_hz 5 Hz is outside 20 .. 11000"), ("hp:300:0.7,peak:1000:30:1", "section 1 gain_cb 300 centibels"),
                      ("lp:300:20", "section 0 q_permille 20000"), ("foo:300:1", "section 0 kind 'foo'"), ("peak:1000:1.0", "is not kind:Hz:dB:Q"),
                      ("hp:300:+3:0.7", "is not kind:Hz:Q"), ("hp:300:x", "section 0 q_permille 'x' is no number"), ("hp:300:0.7,", "section 1 kind ''"),
                      ("", "empty spec"), (",".join(["hp:300:0.7"] * 9), "9 sections"), (",".join(["hp:300:0.7"] * 20), "20 sections is outside 1 .. 8")):
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace("..", r"\.\.")):
            q3tts.tone_sections(bad)


def test_the_clip_tells_wrong_restatements_apart():
    """each deliberately wrong variant changes at least one output bit of the GPU test's clip, so a kernel built that way fails it"""
    x = R.gpu_clip()
    c = q3tts.tone_coeffs(R.SECTIONS[8])
    right = R.cascade(x, c).view(np.uint32)
    for wrong in ("float", "swap", "reverse"):
        n = int(np.count_nonzero(R.cascade(x, c, wrong).view(np.uint32) != right))
        print("%-8s changes %d of %d samples" % (wrong, n, x.size))
        assert n > 0, wrong
