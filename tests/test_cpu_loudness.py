"""The loudness stage without a GPU (include/q3tts.h "loudness"): the coefficients, the meter and the host rule through
the C-ABI, and the properties of the plain-Python restatement of the stage's arithmetic (tests/loudness_ref.py): the meter on the
BS.1770 sine, its filters against scipy, the normaliser on a speech-like clip, on inputs far below its range and on silence.
tests/test_gpu_loudness.py holds the kernel to this restatement bit for bit."""
import math

import numpy as np
import pytest

import loudness_ref as R
import q3tts

# ITU-R BS.1770-4, table 1 and table 2: the two filters at 48 kHz { b0, b1, b2, a1, a2 }
BS1770_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_coefficients():
    c48 = q3tts.loudness_coeffs(48000)
    worst = max(abs(a - b) for a, b in zip(c48, BS1770_48K))
    print("48 kHz against the BS.1770-4 table: %.3g" % worst)
    assert worst <= 1e-12
    c24 = q3tts.loudness_coeffs(24000)
    far = max(ulps(a, b) for a, b in zip(c24, R.C24))
    print("24 kHz against the restatement: %d ulp" % far)
    assert far <= 4                                     # libm's tan and pow are the only freedom
    assert c24[5:8].tolist() == [1.0, -2.0, 1.0]
    for bad in (7999, 384001, 0, -1):
        with pytest.raises(ValueError, match=str(bad)):
            q3tts.loudness_coeffs(bad)


@pytest.fixture(scope="module")
def sine_E():
    return R.energies(R.sine(5.0, 1.0)), R.energies(R.sine(5.0, 0.1))


def test_meter_on_the_sine(sine_E):
    full, tenth = sine_E
    assert full.size == 50 and full.dtype == np.int64 and int(full.max()) < 2 ** 46
    a, b = q3tts.loudness_lufs(full), q3tts.loudness_lufs(tenth)
    print("997 Hz full scale: %.4f LUFS; at 0.1: %.4f (%.4f lower)" % (a, b, a - b))
    assert abs(a - (-3.01)) <= 0.1
    assert abs((a - b) - 20.0) <= 0.01
    # a steady tone: momentary and short-term read what integrated reads
    assert abs(q3tts.loudness_lufs(full, "momentary") - a) <= 0.01 and abs(q3tts.loudness_lufs(full, "short-term") - a) <= 0.01


def test_lufs_is_the_two_gate_rule(sine_E):
    rng = np.random.default_rng(1)
    clips = [sine_E[0], sine_E[1], R.energies(R.speech_like(4.0)), R.energies(R.gpu_clip()),
             (rng.integers(0, 2 ** 40, 64) * (rng.random(64) < 0.6)).astype(np.int64)]
    for E in clips:
        got, want = q3tts.loudness_lufs(E), R.lufs_integrated(E)
        assert got == want or abs(got - want) <= 1e-9, (got, want)
    ninf = -math.inf
    assert q3tts.loudness_lufs(np.zeros(40, np.int64)) == ninf                      # nothing passes the absolute gate
    assert q3tts.loudness_lufs(np.zeros(0, np.int64)) == ninf and q3tts.loudness_lufs(sine_E[0][:3]) == ninf
    assert q3tts.loudness_lufs(sine_E[0][:3], "momentary") == ninf and q3tts.loudness_lufs(sine_E[0][:29], "short-term") == ninf
    assert q3tts.loudness_lufs(sine_E[0][:4], "momentary") > -4.0
    # the relative gate: a loud second behind nine quiet ones (30 LU down).  The 87 quiet windows fall 10 LU below the mean of all
    # and are dropped; left are the three windows with 1, 2, 3 loud sub-blocks and the seven loud ones: 10 log10(8.5 / 10) below the
    # loud second alone (the quiet sub-blocks inside the three add 0.1 % to them)
    loud, quiet = int(sine_E[0][10]), int(sine_E[0][10]) // 1000
    E = np.array([quiet] * 90 + [loud] * 10, np.int64)
    drop = q3tts.loudness_lufs(np.array([loud] * 10, np.int64)) - q3tts.loudness_lufs(E)
    assert abs(drop - (-10.0 * math.log10(0.85))) <= 0.002, drop
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="mode"):
            q3tts.loudness_lufs(E, bad)
    with pytest.raises(ValueError, match="energy"):
        q3tts.loudness_lufs(np.array([-5], np.int64))


def test_filters_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    x = R.speech_like(2.0)
    c = R.C24
    u = signal.lfilter(c[0:3], [1.0, c[3], c[4]], x.astype(np.float64))
    v = signal.lfilter(c[5:8], [1.0, c[8], c[9]], u)
    # the same energy measure over scipy's v: the floor takes up to 1 off every sample, 6e-9 of a sub-block at this level, so the
    # filters are compared behind it; the pauses' sub-blocks (E below 1e10, where one quantum is 1e-10) are left out
    z = np.floor(np.minimum(v * v, 4.0) * 4294967296.0)
    want = z[: 20 * R.BLOCK].reshape(20, R.BLOCK).sum(axis=1)
    got = R.energies(x).astype(np.float64)
    live = want > 1e10
    worst = float(np.abs(got[live] / want[live] - 1.0).max())
    print("E_b against scipy.signal.lfilter: %.3g relative over %d sub-blocks" % (worst, int(live.sum())))
    assert live.sum() >= 12 and worst <= 1e-9


def test_host_rule():
    for n, want in ((0, 0), (2399, 0), (2400, 2400), (2401, 2400), (4799, 2400), (4800, 4800), (86400000, 86400000), (2 ** 31 + 5, 2400 * ((2 ** 31 + 5) // 2400))):
        assert q3tts.loudness_emitted(-160, n) == want == R.emitted(-160, n), n
        assert q3tts.loudness_emitted(-160, n, True) == n == R.emitted(-160, n, True)
        assert q3tts.loudness_emitted(0, n) == n == R.emitted(0, n)                  # meter only: no latency
    with pytest.raises(ValueError, match="negative"):
        q3tts.loudness_emitted(-160, -1)


@pytest.fixture(scope="module")
def speech():
    x = R.speech_like(8.0, -17.0)
    return x, R.stage(x, -160, 200, 0)


def test_normaliser_lands_on_the_target(speech):
    x, (y, E, G) = speech
    assert abs(R.lufs_integrated(E) - (-17.0)) <= 0.01 and y.dtype == np.float32 and y.size == x.size
    got = R.lufs_integrated(R.energies(y[-4 * 24000:]))
    print("speech-like clip at -17 LUFS, target -16: the last 4 s read %.2f LUFS; last gain %.3f dB" % (got, 20 * math.log10(G[-1])))
    assert abs(got - (-16.0)) <= 0.5


def test_slew_and_range(speech):
    x, (y, E, G) = speech
    for start, gains in ((0, G), (400, R.stage(x, -100, 400, 400)[2]), (-100, R.stage(x, -230, 60, -100)[2])):
        prev = np.concatenate([[np.float32(10.0 ** (start / 200.0))], gains[:-1]]).astype(np.float32)
        assert (gains <= prev * R.UP).all() and (gains >= prev * R.DN).all()          # no G_b moves more than UP or DN from its predecessor
    # 20 dB and more below the range: the gain ends at exactly R
    for drop, rng_cb in ((10.0 ** (-40 / 20.0), 200), (10.0 ** (-46 / 20.0), 60)):
        quiet = (x * np.float32(drop)).astype(np.float32)
        g = R.stage(quiet, -160, rng_cb, 0)[2]
        assert g[-1] == np.float32(10.0 ** (rng_cb / 200.0)), (g[-1], rng_cb)
    # and 20 dB above it: exactly 1 / R
    hot = R.stage(R.sine(6.0, 1.0), -400, 100, 0)[2]
    assert hot[-1] == np.float32(1.0 / 10.0 ** (100 / 200.0))


def test_silence_keeps_the_start_gain():
    x = np.zeros(5 * R.BLOCK + 77, np.float32)
    for start in (0, -100, 400):
        y, E, G = R.stage(x, -160, 200, start)
        assert not E.any() and G.size == 5 and (G == np.float32(10.0 ** (start / 200.0))).all() and not y.any()


def test_meter_only_is_the_identity(speech):
    x = speech[0][:30000]
    y, E, G = R.stage(x, 0, 0, 0)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32)) and (G == np.float32(1)).all()
    assert np.array_equal(E, speech[1][1][: E.size])


def test_loudness_params():
    assert q3tts.loudness_params(-16) == (-160, 200, 0) and q3tts.loudness_params(-23.0, 6, -10) == (-230, 60, -100)
    assert q3tts.loudness_params((-16, 12)) == (-160, 120, 0) and q3tts.loudness_params(0) == (0, 200, 0)
