"""Restatement of the tone stage (include/q3tts.h "tone"): the cookbook coefficients in numpy float64 and the cascade as a plain-Python
float loop in the header's order.  Python's float is the IEEE double and every expression below is one rounded operation after the
other, so with the library's own coefficients (q3tts.tone_coeffs) the result is what the header fixes, bit for bit, subnormals
included.  The three wrong variants exist to show that the test clip tells them apart (tests/test_cpu_tone.py)."""
import numpy as np

HP, LP, LS, HS, PEAK = 1, 2, 3, 4, 5
FS = 24000.0


def coeffs(sections):
    """float64 [n][5], { b0, b1, b2, a1, a2 } of every (kind, freq_hz, gain_cb, q_permille), by the header's formulas"""
    out = np.zeros((len(sections), 5), np.float64)
    for j, (kind, f, g, q) in enumerate(sections):
        w0 = np.float64(2.0) * np.pi * np.float64(f) / FS
        c, alpha = np.cos(w0), np.sin(w0) / (2.0 * (np.float64(q) / 1000.0))
        A = np.power(np.float64(10.0), np.float64(g) / 400.0)
        if kind == HP:
            b, a = ((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)
        elif kind == LP:
            b, a = ((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)
        elif kind == PEAK:
            b, a = (1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A)
        else:
            s, p, m = 2.0 * np.sqrt(A) * alpha, A + 1.0, A - 1.0
            if kind == LS:
                b = (A * ((p - m * c) + s), 2.0 * A * (m - p * c), A * ((p - m * c) - s))
                a = ((p + m * c) + s, -2.0 * (m + p * c), (p + m * c) - s)
            else:
                b = (A * ((p + m * c) + s), -2.0 * A * (m + p * c), A * ((p + m * c) - s))
                a = ((p - m * c) + s, 2.0 * (m - p * c), (p - m * c) - s)
        out[j] = (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])
    return out


def cascade(x, c, wrong=None, want_state=False):
    """y[k] = (float)s_n[k] for float32 x and coefficients c [n][5].  wrong: None, or one of the deliberately wrong variants "float"
    (rounded to float between sections), "swap" (the two subtractions swapped), "reverse" (sections in reverse order).
    want_state: also the smallest non-zero |s_j[k]| any section's output took."""
    c = [tuple(float(v) for v in row) for row in np.asarray(c, np.float64)]
    if wrong == "reverse":
        c = c[::-1]
    s = [float(v) for v in np.asarray(x, np.float32)]
    tiny = float("inf")
    for j, (b0, b1, b2, a1, a2) in enumerate(c):
        i1 = i2 = o1 = o2 = 0.0
        out = [0.0] * len(s)
        for k, u in enumerate(s):
            ff = (b0 * u + b1 * i1) + b2 * i2
            y = (ff - a1 * o1) - a2 * o2 if wrong == "swap" else (ff - a2 * o2) - a1 * o1
            i2, i1, o2, o1 = i1, u, o1, y
            out[k] = y
            if want_state and y != 0.0 and abs(y) < tiny:
                tiny = abs(y)
        if wrong == "float" and j + 1 < len(c):
            out = [float(v) for v in np.asarray(out, np.float64).astype(np.float32)]
        s = out
    with np.errstate(under="ignore"):
        y = np.asarray(s, np.float64).astype(np.float32)
    return (y, tiny) if want_state else y


def response(c, f):
    """|H(e^{j 2 pi f / fs})| of one section's coefficients, in float64"""
    z = np.exp(-2j * np.pi * np.float64(f) / FS)
    b0, b1, b2, a1, a2 = (np.float64(v) for v in c)
    return abs((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z))


# ---- the GPU test's clip and sections (tests/test_gpu_tone.py, tests/test_cpu_tone.py) ----
ZERO0, ZERO1 = 9000, 15600       # the run of exact zeros

SECTIONS = {
    1: [(LS, 20, 60, 100)],
    2: [(HP, 300, 0, 707), (LP, 3400, 0, 707)],
    5: [(HP, 300, 0, 707), (HP, 300, 0, 707), (PEAK, 2500, 30, 1000), (LP, 3400, 0, 707), (LP, 3400, 0, 707)],      # "telephone"
    8: [(HP, 80, 0, 707), (LS, 200, 30, 707), (PEAK, 1000, -60, 4000), (PEAK, 2500, 45, 1000), (HS, 6000, -40, 707), (LP, 11000, 0, 500),
        (PEAK, 20, 240, 10000), (HP, 20, 0, 100)],
}
# Chosen for the zero run: at 6000 Hz cos(w0) = 0, so a1 = 0 and with Q 0.1 a2 = -2/3: s[k] = (2/3) s[k-2] once the input is zero.  The
# state falls by 0.088 decades a sample: through the float subnormals (1e-38 .. 1e-45, which the output shows) and then through the
# double subnormals (below 2.2e-308) to exact zero about 3700 samples into the run.
UNDERFLOW = [(HP, 6000, 0, 100), (LP, 6000, 0, 100)]


def gpu_clip():
    """20 000 samples: noise, a sine, single impulses, full-scale +-1 steps, a run of exact zeros, noise again"""
    rng = np.random.default_rng(42)
    x = np.zeros(20000, np.float32)
    x[:4000] = np.clip(0.5 * rng.standard_normal(4000), -0.95, 0.95).astype(np.float32)
    x[4000:6500] = (0.8 * np.sin(2.0 * np.pi * 440.0 * np.arange(2500) / FS)).astype(np.float32)
    x[6600] = 1.0
    x[6601] = -1.0
    x[6900] = np.float32(-0.25)
    x[7000:7400] = 1.0                 # full-scale steps
    x[7400:7800] = -1.0
    x[7800:8200] = 1.0
    x[8200:ZERO0] = np.clip(0.3 * rng.standard_normal(ZERO0 - 8200), -0.95, 0.95).astype(np.float32)
    x[ZERO1:] = np.clip(0.5 * rng.standard_normal(20000 - ZERO1), -0.95, 0.95).astype(np.float32)
    assert not x[ZERO0:ZERO1].any()
    return x
