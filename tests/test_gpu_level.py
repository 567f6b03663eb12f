"""The output-level stage alone (q3tts_level_begin / _push_batch_host / _end): 24 kHz float in, the same audio g times as loud and never
above the ceiling out, whatever the cuts.  The kernel's arithmetic is fixed by the header — every fp32 operation a single rounded one,
the minimum and the integer window sum order-free — so the samples are held bit for bit against the numpy restatement
(tests/level_ref.py: np.array_equal on the bit patterns, no tolerance): in one push, in pushes of 1, 127, 128, 129 and 255 samples,
at clip lengths around the kernel's tile, with single-sample peaks at both ends and 127 / 128 samples either side of a push boundary
and of a tile seam, for gain-only stages, and for stages that share a launch."""
import numpy as np
import pytest

import q3tts
from level_ref import TILE, W, ceiling_f32, clip, level32
from util import tiny_pair

pytestmark = pytest.mark.gpu

NS = 6000
PARAMS = [(60, 900), (0, 500), (-100, 1000), (400, 250)]        # (centibels, permille)


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def x():
    return clip(NS)


@pytest.fixture(scope="module")
def ref(x):
    """the restatement of the shared clip per parameter pair: computed once, shared, never modified"""
    return {p: level32(x, *p, want_s=True) for p in PARAMS + [(60, 0), (-600, 0)]}


def run(eng, x, cb, c, ends, finish_with_last=True):
    """one stage, pushes ending at `ends` -> samples; every push's length is checked against the host rule"""
    sid = eng.level_begin(cb, c)
    parts, at, total = [], 0, 0
    for k, b in enumerate(ends):
        fin = k + 1 == len(ends) and finish_with_last
        out = eng.level_push_batch([sid], [x[at:b]], [fin])[0]
        after = q3tts.level_emitted(cb, c, b, fin)
        assert out.dtype == np.float32 and out.size == after - total, (cb, c, k)      # a push's length is E(after) - E(before)
        total, at = after, b
        parts.append(out)
    if not finish_with_last:
        out = eng.level_push_batch([sid], [x[:0]], [True])[0]                        # finish with n_in = 0
        assert out.size == len(x) - total
        parts.append(out)
    eng.level_end(sid)
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def same_bits(a, b):
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_limiter_is_neither_idle_nor_always_on(ref):
    for p in PARAMS[:2]:
        s = ref[p][1]
        share = float(np.count_nonzero(s < 1.0)) / s.size
        print("gain %d cB, ceiling %d permille: s < 1 on %.1f %% of the samples" % (p[0], p[1], 100 * share))
        assert 0.05 <= share <= 0.60, (p, share)


@pytest.mark.parametrize("cb,c", PARAMS)
def test_one_push_bit_exact(eng, x, ref, cb, c):
    y = run(eng, x, cb, c, [NS])
    assert same_bits(y, ref[(cb, c)][0]), (cb, c, np.flatnonzero(y.view(np.uint32) != ref[(cb, c)][0].view(np.uint32))[:8])
    assert np.abs(y).max() <= ceiling_f32(c)


@pytest.mark.parametrize("step", [1, 127, 128, 129, 255])
def test_every_cut_gives_the_same_bits(eng, x, ref, step):
    cb, c = PARAMS[0]
    n = 700 if step == 1 else NS               # pushes of one sample: a shorter clip, still past the first tile-free 254 samples
    want = level32(x[:n], cb, c) if n != NS else ref[(cb, c)][0]
    ends = list(range(step, n, step)) + [n]
    assert same_bits(run(eng, x[:n], cb, c, ends), want), step
    assert same_bits(run(eng, x[:n], cb, c, ends, finish_with_last=False), want), step


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, TILE + W - 1, TILE + W])
def test_clip_lengths_around_the_tile(eng, x, n):
    cb, c = PARAMS[0]
    assert same_bits(run(eng, x[:n], cb, c, [n]), level32(x[:n], cb, c)), n
    # unfinished first push: n - 127 outputs, so the tile count changes at n - 127 = TILE as well
    assert same_bits(run(eng, x[:n + W], cb, c, [n + W - 1, n + W]), level32(x[:n + W], cb, c)), n


def peaks(n, at):
    rng = np.random.default_rng(n)
    z = (0.3 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    for k in at:
        z[k] = np.float32(2.75 if k % 2 else -2.75)
    return z


@pytest.mark.parametrize("seam,ends", [
    (1500, [1500, 3300]),                       # a push boundary
    (TILE, [3300]),                             # a tile seam inside one push
    (TILE + 700, [700, 3300]),                  # a tile seam of the second push (its first output is 700 - 127)
])
def test_single_peaks_around_seams(eng, seam, ends):
    n = 3300
    for at in ([0], [n - 1], [0, n - 1], [seam - 128], [seam - 127], [seam + 127], [seam + 128], [seam - 1], [seam]):
        z = peaks(n, at)
        want, s = level32(z, 0, 500, want_s=True)
        assert np.count_nonzero(s < 1.0) >= W                      # each peak pulls the gain down around itself
        assert same_bits(run(eng, z, 0, 500, ends), want), (seam, at)


def test_five_samples_and_empty_finish(eng, x):
    for cb, c in ((60, 900), (60, 0)):
        z = np.array([0.1, -3.0, 0.5, 2.0, -0.05], np.float32)
        assert same_bits(run(eng, z, cb, c, [5]), level32(z, cb, c))
        assert same_bits(run(eng, z, cb, c, [5], finish_with_last=False), level32(z, cb, c))
        assert run(eng, z[:0], cb, c, [0]).size == 0                                   # a stage finished without a sample
    sid = eng.level_begin(60, 900)
    assert eng.level_push_batch([sid], [x[:0]])[0].size == 0                           # an empty push leaves the stage as it was
    assert eng.level_push_batch([sid], [x[:100]])[0].size == 0                         # below the look-ahead: held back
    assert same_bits(eng.level_push_batch([sid], [x[:0]], [True])[0], level32(x[:100], 60, 900))
    eng.level_end(sid)


@pytest.mark.parametrize("cb", [60, -600])
def test_gain_only(eng, x, ref, cb):
    g = q3tts.level_gain(cb)
    want = (g * x).astype(np.float32)
    assert same_bits(ref[(cb, 0)][0], want)
    assert same_bits(run(eng, x, cb, 0, [NS]), want)
    assert same_bits(run(eng, x, cb, 0, [1, 2, 1025, 1026, NS], finish_with_last=False), want)      # no latency: every push returns its length


def test_transparent_below_the_ceiling(eng, x):
    quiet = (x / np.abs(x).max() * np.float32(0.45)).astype(np.float32)
    y = run(eng, quiet, 0, 500, [777, NS])
    assert same_bits(y, quiet)


def test_three_stages_in_one_call_equal_themselves_alone(eng, x):
    specs = [((60, 900), NS), ((0, 500), 2500), ((-100, 0), 1300)]
    sids = [eng.level_begin(*p) for p, _ in specs]
    alone = [run(eng, x[:n], p[0], p[1], [n]) for p, n in specs]
    parts = [[] for _ in specs]
    cuts = [0.0, 0.1, 0.55, 1.0]
    for k in range(1, len(cuts)):
        xs = [x[int(cuts[k - 1] * n): int(cuts[k] * n)] for _, n in specs]
        outs = eng.level_push_batch(sids, xs, [k + 1 == len(cuts)] * len(specs))
        for i, o in enumerate(outs):
            parts[i].append(o)
    for i, (p, n) in enumerate(specs):
        y = np.concatenate(parts[i])
        assert same_bits(y, alone[i]), p
        assert same_bits(y, level32(x[:n], *p)), p
        eng.level_end(sids[i])


def test_refusals_leave_every_stage_where_it_was(eng, x, ref):
    for cb, c in ((-601, 900), (401, 0), (0, 1001), (0, -1)):
        with pytest.raises(RuntimeError, match=str(cb if abs(cb) > 400 else c)):
            eng.level_begin(cb, c)
    with pytest.raises(RuntimeError, match="no stage"):
        eng.level_begin(0, 0)
    a, b = eng.level_begin(60, 900), eng.level_begin(0, 500)
    first = eng.level_push_batch([a, b], [x[:4000], x[:4000]])
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.level_push_batch([a, a], [x[:10], x[:10]])
    with pytest.raises(RuntimeError, match="no such level stage"):
        eng.level_push_batch([a, 4000], [x[:10], x[:10]])
    rest = eng.level_push_batch([a, b], [x[4000:], x[4000:]], [True, True])
    assert same_bits(np.concatenate([first[0], rest[0]]), ref[(60, 900)][0])
    assert same_bits(np.concatenate([first[1], rest[1]]), ref[(0, 500)][0])
    with pytest.raises(RuntimeError, match="finished"):
        eng.level_push_batch([a], [x[:10]])
    eng.level_end(a)
    eng.level_end(b)
    with pytest.raises(RuntimeError, match="no such level stage"):
        eng.level_end(a)
