"""The loudness stage alone (q3tts_loudness_begin / _push_batch_host / _end): 24 kHz float in, the same audio out behind a gain that
follows a BS.1770 measurement, whatever the cuts.  The kernel's arithmetic is fixed by the header — every fp64 and fp32 operation a
single rounded one in a fixed order, the energies exact integers — so samples (uint32 views), energies and gains are held bit for bit
against the plain-Python restatement (tests/loudness_ref.py: np.array_equal, no tolerance): in one push, in pushes of 1, 2399, 2400,
2401 and 4799 samples, at clip lengths around the sub-block edges, below one sub-block, with a finish of its own, and for stages
that share a launch.  The clip's gate opens, closes and reopens, and one peak sits either side of a sub-block edge."""
import ctypes as C

import numpy as np
import pytest

import q3tts
import loudness_ref as R
from util import tiny_pair

pytestmark = pytest.mark.gpu

B = R.BLOCK


@pytest.fixture(scope="module")
def eng():
    e, orc, _ = tiny_pair(seed=0, max_batch=1, max_ctx=64)
    orc.close()
    yield e
    e.close()


@pytest.fixture(scope="module")
def clip():
    x = R.gpu_clip()
    assert x.size == 34600 and abs(x[3 * B - 1]) == np.float32(0.9) and abs(x[3 * B + 1]) == np.float32(0.9)
    return x


@pytest.fixture(scope="module")
def ref(clip):
    """the restatement over the whole clip, per parameter set: computed once, shared, never modified"""
    return {p: R.stage(clip, *p) for p in R.PARAMS}


def run(eng, x, p, ends, finish_with_last=True):
    """one stage, pushes ending at `ends` -> (samples, energies, gains); every push's length is checked against the host rule"""
    sid = eng.loudness_begin(*p)
    ys, es, gs, at, total = [], [], [], 0, 0
    for k, b in enumerate(ends):
        fin = k + 1 == len(ends) and finish_with_last
        y, e, g = eng.loudness_push_batch([sid], [x[at:b]], [fin], report=True)[0]
        after = q3tts.loudness_emitted(p[0], b, fin)
        assert after == R.emitted(p[0], b, fin)
        assert y.dtype == np.float32 and y.size == after - total, (p, k, y.size, after - total)     # a push's length is E(after) - E(before)
        assert e.size == g.size == b // B - at // B, (p, k)                                         # the sub-blocks the push completed
        total, at = after, b
        ys.append(y), es.append(e), gs.append(g)
    if not finish_with_last:
        y, e, g = eng.loudness_push_batch([sid], [x[:0]], [True], report=True)[0]                   # finish with n_in = 0
        assert y.size == len(x) - total and e.size == 0
        ys.append(y)
    eng.loudness_end(sid)
    return np.concatenate(ys), np.concatenate(es), np.concatenate(gs)


def same(got, want):
    y, e, g = got
    wy, we, wg = want
    return (y.size == wy.size and np.array_equal(y.view(np.uint32), wy.view(np.uint32)) and e.dtype == np.int64 and np.array_equal(e, we)
            and g.size == wg.size and np.array_equal(g.view(np.uint32), wg.view(np.uint32)))


def where(got, want):
    y, e, g = got
    wy, we, wg = want
    if y.size != wy.size or e.size != we.size:
        return (y.size, wy.size, e.size, we.size)
    return (np.flatnonzero(y.view(np.uint32) != wy.view(np.uint32))[:6], np.flatnonzero(e != we)[:6], np.flatnonzero(g.view(np.uint32) != wg.view(np.uint32))[:6])


def test_the_clip_exercises_the_gate(ref):
    y, E, G = ref[R.PARAMS[0]]
    W = E[3:] + E[2:-1] + E[1:-2] + E[:-3]
    passed = W >= R.GATE
    print("windows that count:", passed.astype(int), "gains:", G)
    # W_3 counts; W_9 = E_6 .. E_9 does not (W_8 still holds the high-pass's ringing in E_5); the last counts again
    assert passed[0] and not passed[6] and passed[-1]
    assert len(set(G.tolist())) > 4                                              # the gain moves
    assert any(abs(float(b) / float(a) - 1.0) < 0.1 and a != b for a, b in zip(G[:-1], G[1:]))   # and not only by whole slew steps


@pytest.mark.parametrize("p", R.PARAMS)
def test_one_push_bit_exact(eng, clip, ref, p):
    got = run(eng, clip, p, [clip.size])
    assert same(got, ref[p]), (p, where(got, ref[p]))
    if p[0] == 0:                                                                # meter only: the input's bits
        assert np.array_equal(got[0].view(np.uint32), clip.view(np.uint32))


@pytest.mark.parametrize("step", [2399, 2400, 2401, 4799])
@pytest.mark.parametrize("p", R.PARAMS)
def test_every_cut_gives_the_same_bits(eng, clip, ref, p, step):
    ends = list(range(step, clip.size, step)) + [clip.size]
    got = run(eng, clip, p, ends)
    assert same(got, ref[p]), (p, step, where(got, ref[p]))
    assert same(run(eng, clip, p, ends, finish_with_last=False), ref[p]), (p, step)


@pytest.mark.parametrize("p", [R.PARAMS[0], R.PARAMS[3]])
def test_pushes_of_one_sample(eng, clip, ref, p):
    """one sample at a time across two sub-block edges and the peak, the rest in two pushes"""
    ends = [3 * B - 3] + list(range(3 * B - 2, 3 * B + 4)) + [4 * B - 1, 4 * B, 4 * B + 1, clip.size]
    got = run(eng, clip, p, ends)
    assert same(got, ref[p]), (p, where(got, ref[p]))
    x = clip[:B + 40]
    want = R.stage(x, *p)
    got = run(eng, x, p, list(range(1, x.size + 1, 1))[B - 20:], finish_with_last=False)
    assert same(got, want), (p, where(got, want))


@pytest.mark.parametrize("n", [B - 1, B, B + 1, 4 * B - 1, 4 * B, 4 * B + 1, 1, 700])
def test_clip_lengths_around_the_edges(eng, clip, n):
    x = clip[2 * B: 2 * B + n]
    for p in (R.PARAMS[0], R.PARAMS[2], R.PARAMS[3]):
        want = R.stage(x, *p)
        got = run(eng, x, p, [n])
        assert same(got, want), (n, p, where(got, want))
        if n > 1:
            assert same(run(eng, x, p, [n // 2, n], finish_with_last=False), want), (n, p)
        if n < B and p[0] != 0:                                                  # below one sub-block only the finish emits
            sid = eng.loudness_begin(*p)
            assert eng.loudness_push_batch([sid], [x])[0].size == 0
            tail = eng.loudness_push_batch([sid], [x[:0]], [True])[0]
            assert np.array_equal(tail.view(np.uint32), want[0].view(np.uint32))
            eng.loudness_end(sid)


def test_a_finish_at_nothing(eng):
    for p in (R.PARAMS[0], R.PARAMS[3]):
        sid = eng.loudness_begin(*p)
        y, e, g = eng.loudness_push_batch([sid], [np.zeros(0, np.float32)], [True], report=True)[0]
        assert y.size == 0 and e.size == 0 and g.size == 0
        with pytest.raises(RuntimeError, match="finished"):
            eng.loudness_push_batch([sid], [np.zeros(10, np.float32)])
        eng.loudness_end(sid)


def test_four_stages_in_one_launch_equal_themselves_alone(eng, clip, ref):
    lens = [clip.size, 4 * B + 1, clip.size - 1, 9000]
    xs = [clip[:n] for n in lens]
    alone = [run(eng, x, p, [x.size]) for x, p in zip(xs, R.PARAMS)]
    sids = [eng.loudness_begin(*p) for p in R.PARAMS]
    parts = [[[], [], []] for _ in sids]
    cuts = [0.0, 0.13, 0.5, 0.5, 1.0]
    for k in range(1, len(cuts)):
        seg = [x[int(cuts[k - 1] * x.size): int(cuts[k] * x.size)] for x in xs]
        outs = eng.loudness_push_batch(sids, seg, [k + 1 == len(cuts)] * len(sids), report=True)
        for i, o in enumerate(outs):
            for j in range(3):
                parts[i][j].append(o[j])
    for i, sid in enumerate(sids):
        got = tuple(np.concatenate(a) for a in parts[i])
        assert same(got, alone[i]), (i, where(got, alone[i]))
        assert same(got, R.stage(xs[i], *R.PARAMS[i])), i
        eng.loudness_end(sid)
    assert same(alone[0], ref[R.PARAMS[0]])


def test_refusals_leave_every_stage_where_it_was(eng, clip, ref):
    for bad, word in (((-401, 200, 0), "-401"), ((-49, 200, 0), "-49"), ((7, 0, 0), "target 7 "), ((-160, 401, 0), "401"), ((-160, -1, 0), "range -1"),
                      ((-160, 200, 401), "401"), ((-160, 200, -401), "-401")):
        with pytest.raises(RuntimeError, match=word):
            eng.loudness_begin(*bad)
    pa, pb = R.PARAMS[0], R.PARAMS[1]
    a, b = eng.loudness_begin(*pa), eng.loudness_begin(*pb)
    first = eng.loudness_push_batch([a, b], [clip[:5000], clip[:5000]], report=True)
    with pytest.raises(RuntimeError, match="listed twice"):
        eng.loudness_push_batch([a, a], [clip[:10], clip[:10]])
    with pytest.raises(RuntimeError, match="no such loudness stage"):
        eng.loudness_push_batch([a, 4000], [clip[:10], clip[:10]])
    # a negative count, which the wrapper cannot express: straight through the C-ABI
    ids = np.array([a, b], np.int32)
    lens = np.array([10, -1], np.int64)
    ptrs = (C.c_void_p * 2)(clip.ctypes.data, clip.ctypes.data)
    outs = [np.empty(4000, np.float32) for _ in range(2)]
    optr = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    out_len = np.zeros(2, np.int64)
    eng.L.q3tts_loudness_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]
    assert eng.L.q3tts_loudness_push_batch_host(eng.h, 2, ids.ctypes.data, C.cast(ptrs, C.c_void_p), lens.ctypes.data, None, C.cast(optr, C.c_void_p), 4000,
                                                out_len.ctypes.data, None, None, None) != 0
    assert "negative sample count" in eng.L.q3tts_last_error(eng.h).decode()
    # more than a push holds: refused before anything moves (the samples are never read)
    lens = np.array([10, 1440001], np.int64)
    assert eng.L.q3tts_loudness_push_batch_host(eng.h, 2, ids.ctypes.data, C.cast(ptrs, C.c_void_p), lens.ctypes.data, None, C.cast(optr, C.c_void_p), 4000,
                                                out_len.ctypes.data, None, None, None) != 0
    assert "at most 1440000" in eng.L.q3tts_last_error(eng.h).decode()
    ended = eng.loudness_begin(-160, 200, 0)
    eng.loudness_end(ended)
    with pytest.raises(RuntimeError, match="no such loudness stage"):
        eng.loudness_push_batch([a, ended], [clip[:10], clip[:10]])
    rest = eng.loudness_push_batch([a, b], [clip[5000:], clip[5000:]], [True, True], report=True)
    for i, p in enumerate((pa, pb)):
        got = tuple(np.concatenate([first[i][j], rest[i][j]]) for j in range(3))
        assert same(got, ref[p]), (p, where(got, ref[p]))
    with pytest.raises(RuntimeError, match="finished"):
        eng.loudness_push_batch([a], [clip[:10]])
    eng.loudness_end(a)
    eng.loudness_end(b)
    with pytest.raises(RuntimeError, match="no such loudness stage"):
        eng.loudness_end(a)


def test_over_one_hour_is_refused(eng, clip):
    """a stage accepts 86 400 000 samples: sixty pushes of the most a push holds (silence into a meter, so nothing but the filters runs),
    then one sample more is refused and the stage still finishes where it was.  The size cannot be smaller: the rule counts samples."""
    sid = eng.loudness_begin(0, 0, 0)
    n = 1440000
    x = np.zeros(n, np.float32)
    out = np.empty(n, np.float32)
    ids, lens, out_len, nb = np.array([sid], np.int32), np.array([n], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
    xp, op = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    f = eng.L.q3tts_loudness_push_batch_host
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for k in range(60):
        assert f(eng.h, 1, ids.ctypes.data, C.cast(xp, C.c_void_p), lens.ctypes.data, None, C.cast(op, C.c_void_p), n, out_len.ctypes.data, None, None,
                 nb.ctypes.data) == 0, eng.L.q3tts_last_error(eng.h).decode()
        assert out_len[0] == n and nb[0] == 600
    assert not out.any()
    with pytest.raises(RuntimeError, match="one hour"):
        eng.loudness_push_batch([sid], [clip[:1]])
    y, e, g = eng.loudness_push_batch([sid], [clip[:0]], [True], report=True)[0]
    assert y.size == 0 and e.size == 0
    eng.loudness_end(sid)
