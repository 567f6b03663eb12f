"""The pitch stage alone (q3tts_pitch_begin / _push_batch_host / _end): 24 kHz float in, the same audio at the same length with the
fundamental moved out, whatever the cuts.  The kernel's arithmetic is fixed by the header — every fp32 operation a single rounded one
in a fixed order — so the samples are held bit for bit against the numpy restatement (tests/pitch_ref.py: np.array_equal on the bit
patterns, no tolerance): on the synthetic voiced signals (host-staged, so that the voiced path really runs) and on noise, at three
ratios, in one push, in fixed and random cuts with 1-sample and empty pushes, for stages that share a launch, and around a NaN."""
import ctypes as C

import numpy as np
import pytest

import q3tts
import pitch_ref as R
from util import tiny_pair

pytestmark = pytest.mark.gpu

NS = 12000          # 0.5 s
SIGNALS = ["v90", "v140", "v180", "noise"]


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def analyses():
    """the analysis marks of the shared signals: searched once, shared, the signals never modified"""
    sig = {"v%d" % f0: R.voiced(f0, NS) for f0 in R.F0S}
    sig["noise"] = R.noise(NS)
    return {k: R.Analysis(v) for k, v in sig.items()}


@pytest.fixture(scope="module")
def ref(analyses):
    return {(k, r): R.psola32(an.x, r, an) for k, an in analyses.items() for r in R.RATIOS}


def run(eng, x, r, ends, finish_with_last=True):
    """one stage, pushes ending at `ends` -> samples; every push's length is checked against the host rule"""
    sid = eng.pitch_begin(r)
    parts, at, total = [], 0, 0
    for k, b in enumerate(ends):
        fin = k + 1 == len(ends) and finish_with_last
        out = eng.pitch_push_batch([sid], [x[at:b]], [fin])[0]
        after = q3tts.pitch_emitted(b, fin)
        assert out.dtype == np.float32 and out.size == after - total, (r, k)      # a push's length is E(after) - E(before)
        total, at = after, b
        parts.append(out)
    if not finish_with_last:
        out = eng.pitch_push_batch([sid], [x[:0]], [True])[0]                     # finish with n_in = 0
        assert out.size == len(x) - total
        parts.append(out)
    eng.pitch_end(sid)
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def same_bits(a, b):
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_diff(a, b):
    return np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))[:8] if a.size == b.size else (a.size, b.size)


def test_the_voiced_path_really_runs(analyses):
    for k, an in analyses.items():
        mk = R.marks(an, 1260)
        share = sum(1 for m in mk if m[3]) / len(mk)
        print("%s: %d synthesis marks, %.0f %% voiced" % (k, len(mk), 100 * share))
        assert (share == 0.0) if k == "noise" else (share >= 0.6), (k, share)


@pytest.mark.parametrize("r", R.RATIOS)
@pytest.mark.parametrize("sig", SIGNALS)
def test_one_push_bit_exact(eng, analyses, ref, sig, r):
    y = run(eng, analyses[sig].x, r, [NS])
    assert same_bits(y, ref[(sig, r)]), (sig, r, first_diff(y, ref[(sig, r)]))


@pytest.mark.parametrize("sig,r", [("v140", 794), ("v90", 1498), ("noise", 1260)])
def test_every_cut_gives_the_same_bits(eng, analyses, ref, sig, r):
    x, want = analyses[sig].x, ref[(sig, r)]
    fixed = [1, 2, R.LA, R.LA + 1, R.LA + 2, 2 * R.LA + 1, R.GATE + 2000, 5000, 5001, 5001 + R.PMAX, 9000, NS - 1, NS]
    assert same_bits(run(eng, x, r, fixed), want), first_diff(run(eng, x, r, fixed), want)
    assert same_bits(run(eng, x, r, fixed, finish_with_last=False), want)
    rng = np.random.default_rng(11)
    cuts = sorted(int(c) for c in rng.integers(0, NS, 34))
    cuts = sorted(cuts + [cuts[3], cuts[3], cuts[10] + 1, cuts[20] + 1, cuts[20] + 2]) + [NS]      # 40 pushes, empty and 1-sample ones among them
    cuts = [min(c, NS) for c in cuts]
    assert len(cuts) == 40 and any(b == a for a, b in zip(cuts, cuts[1:])) and any(b == a + 1 for a, b in zip(cuts, cuts[1:]))
    y = run(eng, x, r, cuts)
    assert same_bits(y, want), first_diff(y, want)
    assert same_bits(run(eng, x, r, cuts[:-1] + [NS - 1, NS], finish_with_last=False), want)


@pytest.mark.parametrize("n", [1, R.PU, R.W + R.REACH - 1, R.W + R.REACH, R.LA, R.LA + 1, 2049, 3001])
def test_short_clips(eng, analyses, n):
    x = analyses["v180"].x[2000: 2000 + n]
    want = R.psola32(x, 1260)
    y = run(eng, x, 1260, [n])
    assert same_bits(y, want), (n, first_diff(y, want))
    if n > 1:
        assert same_bits(run(eng, x, 1260, [n // 2, n], finish_with_last=False), want), n


def test_eight_stages_in_one_call_equal_themselves_alone(eng, analyses):
    sigs = ["v90", "v140", "v180", "noise", "v140", "v90", "noise", "v180"]
    rats = [794, 1260, 1498, 500, 2000, 1122, 891, 667]
    lens = [NS, 7000, 3001, 5000, 9000, 1300, 700, NS - 1]
    xs = [analyses[s].x[:n] for s, n in zip(sigs, lens)]
    alone = [run(eng, x, r, [x.size]) for x, r in zip(xs, rats)]
    sids = [eng.pitch_begin(r) for r in rats]
    parts = [[] for _ in sids]
    cuts = [0.0, 0.13, 0.5, 0.5, 1.0]
    for k in range(1, len(cuts)):
        seg = [x[int(cuts[k - 1] * x.size): int(cuts[k] * x.size)] for x in xs]
        outs = eng.pitch_push_batch(sids, seg, [k + 1 == len(cuts)] * len(sids))
        for i, o in enumerate(outs):
            parts[i].append(o)
    for i, sid in enumerate(sids):
        y = np.concatenate(parts[i])
        assert same_bits(y, alone[i]), (i, first_diff(y, alone[i]))
        assert same_bits(y, R.psola32(xs[i], rats[i])), i
        eng.pitch_end(sid)


def test_refusals_leave_every_stage_where_it_was(eng, analyses, ref):
    x = analyses["v140"].x
    for bad in (499, 2001):
        with pytest.raises(RuntimeError, match=str(bad)):
            eng.pitch_begin(bad)
    with pytest.raises(RuntimeError, match="no stage"):
        eng.pitch_begin(1000)
    a, b = eng.pitch_begin(794), eng.pitch_begin(1260)
    first = eng.pitch_push_batch([a, b], [x[:4000], x[:4000]])
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.pitch_push_batch([a, a], [x[:10], x[:10]])
    with pytest.raises(RuntimeError, match="no such pitch stage"):
        eng.pitch_push_batch([a, 4000], [x[:10], x[:10]])
    # a negative count, which the wrapper cannot express: straight through the C-ABI
    ids = np.array([a, b], np.int32)
    lens = np.array([10, -1], np.int64)
    ptrs = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    outs = [np.empty(2000, np.float32) for _ in range(2)]
    optr = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    out_len = np.zeros(2, np.int64)
    eng.L.q3tts_pitch_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert eng.L.q3tts_pitch_push_batch_host(eng.h, 2, ids.ctypes.data, C.cast(ptrs, C.c_void_p), lens.ctypes.data, None, C.cast(optr, C.c_void_p), 2000,
                                             out_len.ctypes.data) != 0
    assert "negative sample count" in eng.L.q3tts_last_error(eng.h).decode()
    ended = eng.pitch_begin(667)
    eng.pitch_end(ended)
    with pytest.raises(RuntimeError, match="no such pitch stage"):
        eng.pitch_push_batch([a, ended], [x[:10], x[:10]])
    rest = eng.pitch_push_batch([a, b], [x[4000:], x[4000:]], [True, True])
    assert same_bits(np.concatenate([first[0], rest[0]]), ref[("v140", 794)])
    assert same_bits(np.concatenate([first[1], rest[1]]), ref[("v140", 1260)])
    with pytest.raises(RuntimeError, match="finished"):
        eng.pitch_push_batch([a], [x[:10]])
    eng.pitch_end(a)
    eng.pitch_end(b)
    with pytest.raises(RuntimeError, match="no such pitch stage"):
        eng.pitch_end(a)


def test_a_nan_stays_local(eng, analyses, ref):
    """On noise every mark is unvoiced with or without the NaN, so the marks are the same and both sides of it keep their bits.  On a
    voiced signal the marks behind a NaN lie at another phase of the period (a_{j+1} = a_j + P_j), so only the samples in front of it
    are held: they are final before the NaN can be read."""
    far = R.LA + 2 * R.PMAX
    at = 6000
    for sig, two_sided in (("noise", True), ("v140", False)):
        z = analyses[sig].x.copy()
        z[at] = np.nan
        y, want = run(eng, z, 1260, [3000, 7000, NS]), ref[(sig, 1260)]
        assert y.size == NS
        assert same_bits(y[: at - far], want[: at - far]), (sig, first_diff(y[: at - far], want[: at - far]))
        assert np.isnan(y).any()
        if two_sided:
            assert same_bits(y[at + far + 1:], want[at + far + 1:]), sig
            full = R.psola32(z, 1260)                                              # a NaN's own bits are not fixed: where, and the rest
            assert np.array_equal(np.isnan(y), np.isnan(full)) and same_bits(np.nan_to_num(y), np.nan_to_num(full)), sig
