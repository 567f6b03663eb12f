"""Ragged prefill (q3tts_slots_begin_ragged, Q3TTS_FLAG_RAGGED_PREFILL; run_prefill, reference src/tts_onnx.cpp:615-665, and the frame
loop's rows, :824-842): the rows of many slots — any lengths, bases and forced frames — share 128-row chunks through the segment form
of k_prefill_append / k_attn_prefill.  The checker is the CPU oracle's prefill of a member's concatenated rows (plus one decode per
forced row), as in tests/test_gpu_prefix.py and tests/test_gpu_continue.py.

NOISE = 2e-4 is the project's asserted bound on |HIP logit - oracle logit| (tests/test_gpu_full.py), 4e-3 the bf16 cache's
(include/q3tts.h): no new tolerance."""
import os

import numpy as np
import pytest

import q3_oracle as qo
from continue_ref import fold_rows, oracle_after_forced
from test_gpu_full import NOISE, check_free_running
from util import frame_tokens, tiny_pair, to_ocfg, to_q3cfg

pytestmark = pytest.mark.gpu

LENS, SLOTS = [17, 40, 3, 70, 25], [5, 0, 3, 6, 2]      # 155 rows: the 70-row member has 68 rows in the first chunk and 2 in the second
PREFIX = [40, 65, 0, 40, 130]                           # bases on both sides of a 64-token page edge and past 128
FORCED = [0, 31, 7, 1, 60]


def _rows(seed, n, H):
    return (np.random.default_rng(seed).standard_normal((n, H)) * 0.1).astype(np.float32)


def _sp(n=8, **kw):
    import q3tts
    return q3tts.Sampling(max_new_tokens=n, **kw)


def _codes(cfg, seed, n):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, cfg.sub_vocab, (n, cfg.n_groups)).astype(np.int64)
    c[:, 0] = rng.integers(0, min(cfg.vocab, cfg.suppress_begin), n)
    return c


def _close(got, ref, what, bound=NOISE):
    d_lg, d_lh = float(np.abs(got[0] - ref[0]).max()), float(np.abs(got[1] - ref[1]).max())
    print("%s: max |logit - oracle| %.3g, last_hidden %.3g" % (what, d_lg, d_lh))
    assert d_lg < bound and d_lh < bound, (what, d_lg, d_lh)


def _with(ocfg, **kw):
    d = ocfg.to_dict()
    d.update(kw)
    return qo.Config.from_dict(d)


def _own(H):
    """each member's rows: LENS[i] prompt rows + 3 rows for the teacher-forced decodes behind the begin"""
    return [_rows(7000 + i, n + 3, H) for i, n in enumerate(LENS)]


def _walk(orc, x, n):
    """(logits, last_hidden) behind row n - 1 of x and behind each row after it"""
    lo, ho = orc.prefill(x[:n])
    return [(lo[-1].copy(), ho.copy())] + [tuple(np.array(v) for v in orc.decode(r)) for r in x[n:]]


def _make(name):
    import q3tts
    if name == "big06":   # 0.6B dims cut to two layers (head_dim 128); the oracle gets the talker's tensors
        d = q3tts.default_config("0.6b").to_dict()
        d.update(n_layers=2)
        cfg = q3tts.Config.from_dict(d)
        eng = q3tts.Engine(cfg, device=0, max_batch=8, max_ctx=256)
        eng.fill_synthetic(seed=0)
        orc = qo.Oracle(to_ocfg(cfg), max_ctx=256)
        for tn, shape in eng.tensor_infos():
            if tn.startswith("talker."):
                orc.set_tensor(tn, eng.get_tensor(tn, shape))
        return eng, orc, None
    ocfg = {"medium": qo.config_medium(), "gqa1": _with(qo.config_medium(), n_heads=2, n_kv_heads=2),
            "gqa4": _with(qo.config_medium(), n_heads=4, n_kv_heads=1)}[name]
    return tiny_pair(seed=5, max_batch=8, max_ctx=256, ocfg=ocfg)


@pytest.fixture(scope="module")
def pairs():
    """engines and oracles by name, made on first use; refs: each engine's check-1 oracle rows, computed once"""
    made, refs = {}, {}

    def get(name):
        if name not in made:
            made[name] = _make(name)
            orc = made[name][1]
            refs[name] = [_walk(orc, x, n) for x, n in zip(_own(orc.cfg.hidden), LENS)]
        return made[name] + (refs[name],)
    yield get
    for eng, orc, _ in made.values():
        eng.close()
        orc.close()


def _begin(eng, own, prefix_ids=None, codes=None, trailings=None, sp=None):
    H = eng.cfg.hidden
    tr = trailings or [_rows(2, 1, H)] * len(SLOTS)
    eng.slots_begin_ragged(SLOTS, [x[:n] for x, n in zip(own, LENS)], tr, sp or _sp(8), prefix_ids=prefix_ids, prefix_codes=codes, seed=1, ignore_eos=True)


def _release(eng):
    for s in SLOTS:
        eng.slot_release(s)


# ---- 1. ragged lengths, scattered slots ----
@pytest.mark.parametrize("which", ["medium", "gqa1", "gqa4", "big06"])
def test_ragged_lengths_scattered_slots(pairs, which):
    eng, orc, _, ref = pairs(which)
    own = _own(eng.cfg.hidden)
    _begin(eng, own)
    try:
        first = [eng.slot_logits(s) for s in SLOTS]
        for k, s in enumerate(SLOTS):
            assert eng.slot_status(s) == (0, False)
            _close(first[k], ref[k][0], "%s member %d (slot %d, %d rows) begin" % (which, k, s, LENS[k]))
            for i in range(3):
                _close(eng.decode(own[k][LENS[k] + i], slot=s), ref[k][1 + i], "%s member %d decode %d" % (which, k, i))
        _release(eng)
        _begin(eng, own)   # the same call twice: the same bits
        for k, s in enumerate(SLOTS):
            again = eng.slot_logits(s)
            assert np.array_equal(first[k][0], again[0]) and np.array_equal(first[k][1], again[1]), k
    finally:
        _release(eng)


# ---- 2. bases and pages ----
def test_bases_and_pages(pairs):
    eng, orc, _, _ = pairs("medium")
    H = eng.cfg.hidden
    own = _own(H)
    pre = {P: _rows(8000 + P, P, H) for P in sorted(set(PREFIX)) if P}
    pids = {P: eng.prefix_create(r) for P, r in pre.items()}
    try:
        _begin(eng, own, prefix_ids=[pids.get(P) for P in PREFIX])
        for k, s in enumerate(SLOTS):
            x = np.concatenate([pre[PREFIX[k]], own[k]]) if PREFIX[k] else own[k]
            ref = _walk(orc, x, PREFIX[k] + LENS[k])
            _close(eng.slot_logits(s), ref[0], "member %d (slot %d, P=%d, S=%d) begin" % (k, s, PREFIX[k], LENS[k]))
            for i in range(3):
                _close(eng.decode(own[k][LENS[k] + i], slot=s), ref[1 + i], "member %d decode %d" % (k, i))
    finally:
        _release(eng)
        for pid in pids.values():
            eng.prefix_release(pid)


# ---- 3. forced frames ----
def test_forced_frames(pairs):
    eng, orc, _, _ = pairs("medium")
    H = eng.cfg.hidden
    own = _own(H)
    codes = [_codes(eng.cfg, 30 + i, f) if f else None for i, f in enumerate(FORCED)]
    trail = [_rows(40 + i, 5, H) for i in range(5)]
    orc.build_prompt(frame_tokens([11, 22, 33]), 0)
    pad = orc.trailing()[1]
    _begin(eng, own, codes=codes, trailings=trail)
    try:
        for k, s in enumerate(SLOTS):
            assert eng.slot_status(s) == (FORCED[k], False)
            if FORCED[k]:
                assert np.array_equal(eng.slot_codes(s), codes[k])
                rows = fold_rows(orc.codec_embed, orc.cp_embed, codes[k], 0, trail[k], pad)
                ref = oracle_after_forced(orc, own[k][:LENS[k]], rows)
            else:
                ref = _walk(orc, own[k], LENS[k])[0]
            _close(eng.slot_logits(s), ref, "member %d (slot %d, S=%d, %d forced frames)" % (k, s, LENS[k], FORCED[k]))
    finally:
        _release(eng)


class _RaggedContinuation:
    """check_free_running's engine: the utterance is begun in a ragged call beside two other members, behind the oracle's own first
    F0 frames as forced frames, and decoded to the end; generate returns forced + continued frames"""
    F0 = 7

    def __init__(self, eng, orc):
        self.eng, self.orc, self.cfg = eng, orc, eng.cfg

    def build_prompt(self, ids, lang):
        self.ids = ids
        return self.eng.build_prompt(ids, lang)

    def generate(self, p, t, sp, seed=0, stream_id=0, ignore_eos=False):
        import q3tts
        from util import to_osampling
        eng, H = self.eng, self.eng.cfg.hidden
        ref = self.orc.generate(self.orc.build_prompt(self.ids, 0), to_osampling(sp), seed=seed, stream=stream_id, cp_cached=True, ignore_eos=True)
        left = sp.max_new_tokens - self.F0
        sp2 = q3tts.Sampling(temperature=sp.temperature, top_p=sp.top_p, top_k=sp.top_k, max_new_tokens=left)
        eng.slots_begin_ragged([6, 3, 1], [_rows(1, 30, H), p, _rows(2, 45, H)], [_rows(3, 1, H), t, _rows(4, 1, H)], sp2,
                               prefix_codes=[None, ref[:self.F0], _codes(eng.cfg, 5, 20)], seed=seed, stream_ids=[9, stream_id, 11], ignore_eos=True)
        while left > 0 and eng.decode_steps(min(16, left)) > 0:
            left -= 16
        assert eng.slot_status(3) == (sp.max_new_tokens, True)
        out = eng.slot_codes(3)
        for s in (6, 3, 1):
            eng.slot_release(s)
        return out


def test_forced_member_continues_greedy(pairs):
    """Prompt seed 1, picked on the CPU (oracle alone, generate_margins over prompt seeds 0..7 at these weights, seed 5, stream 2): the
    smallest top-2 gap of the 24 greedy frames is 3.2e-3 >= 10 x NOISE, so check_free_running's margin rule never shortens the
    comparison."""
    eng, orc, _, _ = pairs("medium")
    ids = frame_tokens(np.random.default_rng(GREEDY_PROMPT_SEED).integers(0, 151643, 16))
    sp = _sp(24, temperature=1.0, top_p=1.0, top_k=1)
    n = check_free_running(_RaggedContinuation(eng, orc), orc, sp, ids, 5, "ragged forced begin, greedy continuation")
    assert n == 24, n


GREEDY_PROMPT_SEED = 1


# ---- 4. one member == q3tts_slot_begin_prefixed ----
@pytest.mark.parametrize("S", [17, 130])
def test_one_member_equals_prefixed_begin(pairs, S):
    eng, _, _, _ = pairs("medium")
    H = eng.cfg.hidden
    pid = eng.prefix_create(_rows(50, 40, H))
    try:
        own, tr = _rows(51 + S, S, H), _rows(1, 1, H)
        eng.slot_begin(4, own, tr, _sp(8), prefix_id=pid, ignore_eos=True)
        a = eng.slot_logits(4)
        eng.slot_release(4)
        eng.slots_begin_ragged([4], [own], [tr], _sp(8), prefix_ids=[pid], ignore_eos=True)
        b = eng.slot_logits(4)
        eng.slot_release(4)
        assert np.isfinite(a[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        eng.prefix_release(pid)


# ---- 5. the segment kernels pinned to the existing ones ----
@pytest.mark.parametrize("which", ["medium", "big06"])
def test_one_segment_equals_the_one_slot_kernels(pairs, which):
    import q3tts
    eng, _, w, _ = pairs(which)
    os.environ["Q3TTS_PREFILL_SEG"] = "1"
    try:
        seg = q3tts.Engine(eng.cfg, device=0, max_batch=2, max_ctx=256, flags=q3tts.FLAG_TEST_HOOKS)   # the knob is read at creation
    finally:
        del os.environ["Q3TTS_PREFILL_SEG"]
    try:
        if w is None:
            seg.fill_synthetic(seed=0)
        else:
            seg.load(w)
        x = _rows(60, 130, eng.cfg.hidden)
        a, b = eng.prefill(x, slot=1), seg.prefill(x, slot=1)
        eng.slot_release(1)
        assert np.isfinite(a[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        seg.close()


# ---- 6. bf16 cache: 16-bit storage == fp32 storage of the rounded rows, both within 4e-3 of the bf16 oracle ----
@pytest.mark.parametrize("which", ["medium", "gqa1", "gqa4", "big06"])
def test_bf16_cache(pairs, which):
    import q3tts
    base, orc0, w, _ = pairs(which)
    own = _own(base.cfg.hidden)
    outs = []
    for flag in (q3tts.FLAG_KV_BF16, q3tts.FLAG_KV_ROUND_BF16):
        eng = q3tts.Engine(base.cfg, device=0, max_batch=8, max_ctx=256, flags=flag)
        try:
            if w is None:
                eng.fill_synthetic(seed=0)
            else:
                eng.load(w)
            _begin(eng, own)
            outs.append([eng.slot_logits(s) for s in SLOTS])
        finally:
            eng.close()
    for p, q in zip(*outs):
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    orc = qo.Oracle(orc0.cfg, max_ctx=256, kv_bf16=True)
    try:
        for tn, shape in base.tensor_infos():
            if tn.startswith("talker."):
                orc.set_tensor(tn, base.get_tensor(tn, shape))
        for k in range(len(SLOTS)):
            _close(outs[0][k], _walk(orc, own[k][:LENS[k]], LENS[k])[0], "%s bf16 member %d" % (which, k), bound=4e-3)
    finally:
        orc.close()


# ---- 7. fallback: dims off the MFMA path begin their members one at a time, bit for bit ----
def test_fallback_equals_individual_begins():
    eng, orc, _ = tiny_pair(seed=3, max_batch=8, max_ctx=256)
    try:
        H = eng.cfg.hidden
        own = _own(H)
        _begin(eng, own)
        a = [eng.slot_logits(s) for s in SLOTS]
        _release(eng)
        for k, s in enumerate(SLOTS):
            eng.slot_begin(s, own[k][:LENS[k]], _rows(2, 1, H), _sp(8), seed=1, stream_id=k, ignore_eos=True)
            b = eng.slot_logits(s)
            eng.slot_release(s)
            assert np.array_equal(a[k][0], b[0]) and np.array_equal(a[k][1], b[1]), k
    finally:
        eng.close()
        orc.close()


# ---- 8. all or nothing ----
def test_all_or_nothing(pairs):
    import q3tts
    base, _, w, _ = pairs("medium")
    H = base.cfg.hidden
    own = _own(H)
    eng = q3tts.Engine(base.cfg, device=0, max_batch=8, max_ctx=256, kv_pool_tokens=4 * 64)   # the set needs 6 pages
    try:
        eng.load(w)

        def refused(text, **kw):
            before = [eng.slot_status(s) for s in range(8)], eng.kv_pool_info()
            with pytest.raises(RuntimeError, match=text):
                eng.slots_begin_ragged(kw.pop("slots", SLOTS), [x[:n] for x, n in zip(own, LENS)], [_rows(2, 1, H)] * 5, _sp(8), ignore_eos=True, **kw)
            assert ([eng.slot_status(s) for s in range(8)], eng.kv_pool_info()) == before
        refused("KV page pool exhausted: 5 slots need 6 more pages")
        refused("slot listed twice", slots=[5, 0, 3, 5, 2])
        bad = [None, None, None, _codes(eng.cfg, 1, 5), None]
        bad[3][3, 2] = eng.cfg.sub_vocab
        refused("frame codes: frame 3 group 2 holds", prefix_codes=bad)
    finally:
        eng.close()


# ---- 9. scheduler under Q3TTS_FLAG_RAGGED_PREFILL ----
def test_scheduler_with_the_flag(pairs):
    import q3tts
    base, _, w, _ = pairs("medium")
    eng = q3tts.Engine(base.cfg, device=0, max_batch=4, max_ctx=256, flags=q3tts.FLAG_RAGGED_PREFILL)
    try:
        eng.load(w)
        rng = np.random.default_rng(21)
        toks = [frame_tokens(rng.integers(0, 151643, n)) for n in (6, 9, 6, 12, 6, 7)]
        lens = {0: 20, 2: 70, 3: 33, 4: 0}
        instructs = [None] * 6
        for u, n in lens.items():
            instructs[u] = q3tts.frame_instruct_ids(rng.integers(0, 151643, n - 5)) if n else np.zeros(0, np.int64)
        sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=12)
        solo = []
        for u in range(6):
            p, t = eng.build_prompt(toks[u], 0, instruct_ids=instructs[u])
            solo.append(eng.generate(p, t, sp, seed=3, stream_id=u, ignore_eos=True))
            eng.slot_release(0)
        pcm, codes, nfr = eng.synthesize_batch(toks, sp, seed=3, ignore_eos=True, instructs=instructs)
        adm, pre, peak = eng.sched_stats()
        assert list(nfr) == [12] * 6 and adm == 6 + pre and peak <= 4
        for u in range(6):
            assert np.array_equal(codes[u], solo[u]), u
        got = [[] for _ in range(6)]

        def on_audio(utt, fb, fe, a, finished):
            got[utt].append(a)
            return False
        pcm2, codes2, nfr2 = eng.synthesize_stream(toks, sp, 5, on_audio, seed=3, ignore_eos=True, instructs=instructs)
        for u in range(6):
            assert np.array_equal(codes2[u], solo[u]), u
            assert len(np.concatenate(got[u])) == len(pcm2[u]) == len(pcm[u])
        # continued utterances: the forced begins of the look in one ragged call
        pcs = [solo[0][:5], None, solo[2][:9], solo[3][:2], None, solo[5][:7]]
        sp8 = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=8)
        ref = []
        for u in range(6):
            p, t = eng.build_prompt(toks[u], 0)
            eng.slot_begin(0, p, t, sp8, seed=3, stream_id=u, ignore_eos=True, prefix_codes=pcs[u])
            while eng.decode_steps(8) > 0:
                pass
            ref.append(eng.slot_codes(0))
            eng.slot_release(0)
        pcm3, codes3, nfr3 = eng.synthesize_continue(toks, pcs, sp8, seed=3, ignore_eos=True)
        adm, pre, peak = eng.sched_stats()
        assert adm == 6 + pre and peak <= 4
        for u in range(6):
            assert nfr3[u] == ref[u].shape[0] and np.array_equal(codes3[u][:nfr3[u]], ref[u]), u
    finally:
        eng.close()
