"""Live text input: an open slot takes its text rows while it generates and stalls, changing nothing, when the row of its next frame has
not arrived (q3tts_slot_text_open / _append_host / q3tts_slots_text_append_ids / _status, q3tts_build_prompt_open_host,
q3tts_synthesize_live_host).  Frame f reads text row f only (reference tts_onnx.cpp:833-842), so however the rows arrive the slot must
produce what it produces with the whole text in hand: "whole" below is the same slot number, batch, seed and stream id begun with
q3tts_build_prompt_host on the full ids, and every comparison is bit for bit unless it says otherwise."""
import os
import subprocess

import numpy as np
import pytest

from util import ASSISTANT, IM_START, TTS_BOS, frame_tokens, tiny_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "leaxer-qwen3-tts_amd", "leaxer-tts")
NOISE = 2e-4    # bound asserted on |HIP logit - oracle logit| by the teacher-forced tests (tests/test_gpu_full.py)
ABS = 2e-5      # vocoder pushes of differing sizes (tests/test_gpu_codec.py)
FRAMES = 24
GREEDY = dict(temperature=1.0, top_p=1.0, top_k=1)
SAMPLED = dict(temperature=0.8, top_p=0.95, top_k=50)
MODES = [pytest.param(GREEDY, id="greedy"), pytest.param(SAMPLED, id="sampled")]
# the first text id sits in the prompt; 14 more are trailing rows (2 at the begin + 12 appended), tts_eos is the 15th
TEXT = [31, 41, 59, 26, 53, 58, 97, 93, 23, 84, 62, 64, 33, 83, 27]
TEXTS = [TEXT, [7 * k + 3 for k in range(15)], [11 * k + 5 for k in range(15)]]


def sampling(mode, max_new=FRAMES):
    import q3tts
    return q3tts.Sampling(max_new_tokens=max_new, **mode)


def open_ids(text, n0):
    """role, first text id and n0 trailing ids: what an open begin holds"""
    return np.array([IM_START, ASSISTANT, TTS_BOS] + list(text[: 1 + n0]), np.int64)


def begin_whole(eng, slot, text, sp, seed, **kw):
    prompt, trailing = eng.build_prompt(frame_tokens(text), 0)
    eng.slot_begin(slot, prompt, trailing, sp, seed=seed, stream_id=slot, ignore_eos=True, **kw)
    return prompt, trailing


def begin_open(eng, slot, text, n0, sp, seed, **kw):
    prompt, trailing = eng.build_prompt_open(open_ids(text, n0), 0)
    assert trailing.shape[0] == n0
    eng.slot_begin(slot, prompt, trailing, sp, seed=seed, stream_id=slot, ignore_eos=True, **kw)
    eng.slot_text_open(slot)
    return prompt, trailing


def rows_of(eng, text, a, b):
    """projected rows of trailing ids [a, b) of `text` (trailing id k is text[1 + k])"""
    return eng.text_project(np.array(text[1 + a: 1 + b], np.int64))


def release_all(eng, n=4):
    for b in range(n):
        eng.slot_release(b)


def run_whole(eng, texts, sps, seed, n_steps=FRAMES, begin_kw=None):
    """slots 0.. begun whole, stepped one frame at a time: codes per slot and the logits rows after every step"""
    release_all(eng, eng_batch(eng))
    for b, (text, sp) in enumerate(zip(texts, sps)):
        begin_whole(eng, b, text, sp, seed, **((begin_kw or {}).get(b, {})))
    logits = [[] for _ in texts]
    for _ in range(n_steps):
        eng.decode_steps(1)
        for b in range(len(texts)):
            logits[b].append(eng.slot_logits(b)[0])
    codes = [eng.slot_codes(b) for b in range(len(texts))]
    return codes, logits


def eng_batch(eng):
    return getattr(eng, "_live_test_batch", 4)


@pytest.fixture(scope="module")
def pair():
    eng, orc, w = tiny_pair(max_batch=4, max_ctx=128)
    orc.close()
    yield eng
    eng.close()


_whole_b1 = {}


def whole_b1(eng, mode, key="tiny"):
    """the b = 1 whole run of TEXT, computed once per sampling mode and left unchanged"""
    k = (key, tuple(sorted(mode.items())))
    if k not in _whole_b1:
        _whole_b1[k] = run_whole(eng, [TEXT], [sampling(mode)], seed=7)
    return _whole_b1[k]


def test_open_prompt_and_rows_equal_the_whole_build(pair):
    eng = pair
    prompt, trailing = eng.build_prompt(frame_tokens(TEXT), 0)
    assert trailing.shape[0] == 15
    for n0 in (0, 2, 14):
        p, t = eng.build_prompt_open(open_ids(TEXT, n0), 0)
        assert np.array_equal(p, prompt) and t.shape[0] == n0 and np.array_equal(t, trailing[:n0])
    assert np.array_equal(rows_of(eng, TEXT, 2, 14), trailing[2:14])
    assert np.array_equal(rows_of(eng, TEXT, 5, 6), trailing[5:6])
    with pytest.raises(RuntimeError, match="too short"):
        eng.build_prompt_open(open_ids(TEXT, 0)[:3], 0)


@pytest.mark.parametrize("mode", MODES)
def test_fed_ahead_equals_whole(pair, mode):
    """12 rows in pieces of 1, 3 and 8, each before it is needed, the last one closing the text"""
    eng = pair
    codes, logits = whole_b1(eng, mode)
    release_all(eng)
    begin_open(eng, 0, TEXT, 2, sampling(mode), seed=7)
    assert eng.slot_text_status(0) == (2, True, False)
    eng.slot_text_append(0, rows=rows_of(eng, TEXT, 2, 3))
    eng.decode_steps(2)
    eng.slot_text_append(0, rows=rows_of(eng, TEXT, 3, 6))
    assert eng.slot_text_status(0) == (6, True, False)
    eng.decode_steps(3)
    eng.slot_text_append(0, rows=rows_of(eng, TEXT, 6, 14), close=True)
    assert eng.slot_text_status(0) == (15, False, False)
    eng.decode_steps(FRAMES - 5)
    assert eng.slot_status(0) == (FRAMES, True)
    assert np.array_equal(eng.slot_codes(0), codes[0])
    assert np.array_equal(eng.slot_logits(0)[0], logits[0][-1])


def starved_run(eng, mode, seed, codes, logits, n_frames=FRAMES, stalls=(2, 9), begin_kw=None, f0=0):
    """case 2: slot 0 starves at the frames `stalls` (steps are issued past them), is fed and goes on; f0: frames it was begun behind"""
    release_all(eng, eng_batch(eng))
    begin_open(eng, 0, TEXT, stalls[0], sampling(mode, n_frames - f0), seed=seed, **(begin_kw or {}))
    have, issued = stalls[0], 0
    for k, at in enumerate(stalls):
        active = eng.decode_steps(at - (stalls[k - 1] if k else f0) + 2)   # two steps more than it has rows for
        issued += at - (stalls[k - 1] if k else f0) + 2
        assert active == 1                                                   # a stalled slot is active and unfinished
        assert eng.slot_status(0) == (at, False)
        assert eng.slot_text_status(0) == (at, True, True)
        assert np.array_equal(eng.slot_logits(0)[0], logits[0][at - 1 - f0])
        assert np.array_equal(eng.slot_codes(0), codes[0][:at])
        nxt = stalls[k + 1] if k + 1 < len(stalls) else 14
        eng.slot_text_append(0, rows=rows_of(eng, TEXT, have, nxt), close=nxt == 14)
        have = nxt
        assert eng.slot_text_status(0) == (nxt + (nxt == 14), nxt != 14, False)
    eng.decode_steps(n_frames - stalls[-1])
    issued += n_frames - stalls[-1]
    assert issued > n_frames - f0                                            # more steps were issued than frames exist
    assert eng.slot_status(0) == (n_frames, True)
    assert np.array_equal(eng.slot_codes(0), codes[0])
    assert np.array_equal(eng.slot_logits(0)[0], logits[0][-1])


@pytest.mark.parametrize("mode", MODES)
def test_starved_equals_whole(pair, mode):
    eng = pair
    codes, logits = whole_b1(eng, mode)
    starved_run(eng, mode, 7, codes, logits)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch(pair, mode):
    """slot 0 closed text (8 frames), slot 1 fed ahead, slot 2 starved at frame 3 (all running) and at frame 12 (slot 0 finished); slot 3 free"""
    eng = pair
    sps = [sampling(mode, 8), sampling(mode), sampling(mode)]
    codes, logits = run_whole(eng, TEXTS, sps, seed=3)
    assert [c.shape[0] for c in codes] == [8, FRAMES, FRAMES]
    release_all(eng)
    begin_whole(eng, 0, TEXTS[0], sps[0], 3)
    begin_open(eng, 1, TEXTS[1], 2, sps[1], 3)
    begin_open(eng, 2, TEXTS[2], 3, sps[2], 3)
    eng.slot_text_append(1, rows=rows_of(eng, TEXTS[1], 2, 8))
    assert eng.decode_steps(5) == 3
    assert [eng.slot_status(b)[0] for b in range(3)] == [5, 5, 3]
    assert eng.slot_text_status(2) == (3, True, True) and eng.slot_text_status(1) == (8, True, False) and eng.slot_text_status(0) == (15, False, False)
    assert np.array_equal(eng.slot_logits(2)[0], logits[2][2])
    for b in range(2):
        assert np.array_equal(eng.slot_logits(b)[0], logits[b][4])
    eng.slot_text_append(2, rows=rows_of(eng, TEXTS[2], 3, 12))
    eng.slot_text_append(1, rows=rows_of(eng, TEXTS[1], 8, 14), close=True)
    assert eng.decode_steps(12) == 2                     # slot 0 finished at 8 frames; slot 2 stalled from frame 12 on
    assert [eng.slot_status(b) for b in range(3)] == [(8, True), (17, False), (12, False)]
    assert eng.slot_text_status(2) == (12, True, True)
    assert np.array_equal(eng.slot_logits(2)[0], logits[2][11]) and np.array_equal(eng.slot_logits(1)[0], logits[1][16])
    eng.slot_text_append(2, rows=rows_of(eng, TEXTS[2], 12, 14), close=True)
    eng.decode_steps(12)
    for b in range(3):
        assert eng.slot_status(b) == (codes[b].shape[0], True)
        assert np.array_equal(eng.slot_codes(b), codes[b]), b
    # slot 2 reaches its last frame in the last step issued, as in the whole run: its logits compare.  Slots 0 and 1 finished earlier
    # and this run issued more steps behind them than the whole run did; a finished slot's logits row is not kept.
    assert np.array_equal(eng.slot_logits(2)[0], logits[2][-1])
    assert eng.slot_text_status(3)[1:] == (False, False)


def fed_run(eng, mode, slots, how):
    """slots begun open with 2 rows and fed the other 12 in pieces of 1, 3, 8 through `how(slot_pieces, close)`; 24 frames"""
    release_all(eng)
    for b in slots:
        begin_open(eng, b, TEXTS[b], 2, sampling(mode), seed=5)
    at = 2
    for n, steps in ((1, 2), (3, 3), (8, FRAMES - 5)):
        how({b: TEXTS[b][1 + at: 1 + at + n] for b in slots}, at + n == 14)
        at += n
        eng.decode_steps(steps)
    return [eng.slot_codes(b) for b in slots], [eng.slot_logits(b)[0] for b in slots]


@pytest.mark.parametrize("mode", MODES)
def test_ids_form(pair, mode):
    eng = pair

    def by_ids(pieces, close):
        eng.slots_text_append_ids(list(pieces), list(pieces.values()), [close] * len(pieces))

    def by_ids_one_by_one(pieces, close):
        for b, ids in pieces.items():
            eng.slot_text_append(b, ids=ids, close=close)

    def by_rows(pieces, close):
        for b, ids in pieces.items():
            eng.slot_text_append(b, rows=eng.text_project(np.array(ids, np.int64)))
            if close:
                eng.slot_text_append(b, close=True)
    c_ids, l_ids = fed_run(eng, mode, [0], by_ids)
    c_rows, l_rows = fed_run(eng, mode, [0], by_rows)
    assert c_ids[0].shape == (FRAMES, eng.cfg.n_groups)
    assert np.array_equal(c_ids[0], c_rows[0]) and np.array_equal(l_ids[0], l_rows[0])
    # against the whole text: another projection call, so within the suite's noise bound on the logits
    release_all(eng)
    begin_whole(eng, 0, TEXTS[0], sampling(mode), 5)
    eng.decode_steps(FRAMES)
    d = float(np.abs(eng.slot_logits(0)[0] - l_ids[0]).max())
    print("ids form vs whole: max |logit difference| = %g" % d)
    assert d < NOISE
    # two slots fed in one call and in two calls
    c_one, l_one = fed_run(eng, mode, [0, 1], by_ids)
    c_two, l_two = fed_run(eng, mode, [0, 1], by_ids_one_by_one)
    for i in range(2):
        assert np.array_equal(c_one[i], c_two[i]) and np.array_equal(l_one[i], l_two[i])


def test_starved_equals_whole_bf16_kv():
    import q3tts
    eng, orc, _ = tiny_pair(max_batch=4, max_ctx=128, flags=q3tts.FLAG_KV_BF16)
    orc.close()
    try:
        codes, logits = whole_b1(eng, SAMPLED, key="bf16")
        starved_run(eng, SAMPLED, 7, codes, logits)
    finally:
        eng.close()


def test_one_slot_step_at_full_dims():
    """0.6B dims, one slot: the graph replay of the one-slot step and the table variant of the predictor samplers; 8 frames, one stall"""
    import q3tts
    eng = q3tts.Engine(q3tts.default_config("0.6b"), device=0, max_batch=1, max_ctx=256)
    eng._live_test_batch = 1
    try:
        eng.fill_synthetic(seed=0)
        codes, logits = run_whole(eng, [TEXT], [sampling(SAMPLED, 8)], seed=7, n_steps=8)
        starved_run(eng, SAMPLED, 7, codes, logits, n_frames=8, stalls=(3,))
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_behind_the_other_begins(pair, mode):
    """slot 0 behind 3 teacher-forced frames, slot 1 behind a shared prompt prefix; each open, starved once, equal to its whole twin"""
    eng = pair
    forced = whole_b1(eng, mode)[0][0][:3]
    release_all(eng)
    pid = eng.prefix_create(eng.text_project(np.array([901, 902, 903, 904, 905], np.int64)))
    try:
        sps = [sampling(mode, FRAMES - 3), sampling(mode)]
        kw = {0: dict(prefix_codes=forced), 1: dict(prefix_id=pid)}
        codes, logits = run_whole(eng, TEXTS[:2], sps, seed=9, n_steps=FRAMES, begin_kw=kw)
        assert codes[0].shape[0] == FRAMES and np.array_equal(codes[0][:3], forced) and codes[1].shape[0] == FRAMES
        release_all(eng)
        begin_open(eng, 0, TEXTS[0], 5, sps[0], 9, **kw[0])       # the forced frames read rows 0..2; frames 3, 4 have their rows
        begin_open(eng, 1, TEXTS[1], 4, sps[1], 9, **kw[1])
        assert eng.slot_status(0)[0] == 3 and eng.slot_text_status(0) == (5, True, False)
        assert eng.decode_steps(6) == 2
        assert [eng.slot_status(b)[0] for b in range(2)] == [5, 4]
        assert eng.slot_text_status(0) == (5, True, True) and eng.slot_text_status(1) == (4, True, True)
        assert np.array_equal(eng.slot_logits(0)[0], logits[0][1]) and np.array_equal(eng.slot_logits(1)[0], logits[1][3])
        eng.slots_text_append_ids([1, 0], [TEXTS[1][5:15], TEXTS[0][6:15]], [True, True])
        eng.decode_steps(FRAMES)
        for b in range(2):
            assert eng.slot_status(b) == (FRAMES, True)
            assert np.array_equal(eng.slot_codes(b), codes[b]), b
    finally:
        release_all(eng)
        eng.prefix_release(pid)


def snapshot(eng, slots=range(4)):
    return [(eng.slot_text_status(b), eng.slot_status(b), eng.slot_codes(b).tobytes()) for b in slots]


def test_refusals(pair):
    """every refusal is a host-side check made before any launch: its message, and the state left as it was"""
    eng = pair
    H = eng.cfg.hidden
    sp = sampling(GREEDY)
    codes, _ = whole_b1(eng, GREEDY)
    release_all(eng)
    begin_open(eng, 0, TEXT, 2, sp, 7)
    begin_whole(eng, 1, TEXTS[1], sp, 7)          # closed text
    before = snapshot(eng)
    row = np.zeros((1, H), np.float32)
    with pytest.raises(RuntimeError, match="text already closed"):
        eng.slot_text_append(1, rows=row)
    with pytest.raises(RuntimeError, match="not armed"):
        eng.slot_text_append(2, rows=row)
    with pytest.raises(RuntimeError, match="not armed"):
        eng.slot_text_open(3)
    with pytest.raises(RuntimeError, match="duplicate slots"):
        eng.slots_text_append_ids([0, 0], [[1], [2]])
    with pytest.raises(RuntimeError, match=r"text id out of range \[0, text_vocab\)"):
        eng.slots_text_append_ids([0], [[1, eng.cfg.text_vocab]])
    with pytest.raises(RuntimeError, match="text id out of range"):
        eng.slot_text_append(0, ids=[-1])
    with pytest.raises(RuntimeError, match="text too long for the trailing buffer"):
        eng.slot_text_append(0, rows=np.zeros((1023, H), np.float32))
    with pytest.raises(RuntimeError, match="text too long for the trailing buffer"):
        eng.slot_text_append(0, rows=np.zeros((1022, H), np.float32), close=True)
    with pytest.raises(RuntimeError, match="text already closed"):      # one bad member refuses the whole call
        eng.slots_text_append_ids([0, 1], [[1], [2]])
    assert snapshot(eng) == before
    eng.decode_steps(1)
    with pytest.raises(RuntimeError, match="has stepped since its begin"):
        eng.slot_text_open(1)
    with pytest.raises(RuntimeError, match="has stepped since its begin"):
        eng.slot_text_open(0)
    assert eng.slot_text_status(1) == (15, False, False) and eng.slot_status(0)[0] == 1
    # behind 3 teacher-forced frames with 2 text rows: the third forced frame took the pad row at the begin, so the text cannot be opened
    release_all(eng)
    prompt, trailing = eng.build_prompt_open(open_ids(TEXT, 2), 0)
    eng.slot_begin(0, prompt, trailing, sp, seed=7, stream_id=0, ignore_eos=True, prefix_codes=codes[0][:3])
    before = snapshot(eng)
    with pytest.raises(RuntimeError, match="must hold the text rows of its forced frames"):
        eng.slot_text_open(0)
    assert snapshot(eng) == before and eng.slot_text_status(0) == (2, False, False)
    # an open slot with no row for its first frame: decode_steps names it and launches nothing
    release_all(eng)
    begin_whole(eng, 0, TEXTS[1], sp, 7)
    begin_open(eng, 1, TEXT, 0, sp, 7)
    before = snapshot(eng)
    lg = [eng.slot_logits(b)[0] for b in range(2)]
    with pytest.raises(RuntimeError, match="slot 1: open text holds no row for the slot's first frame"):
        eng.decode_steps(3)
    assert snapshot(eng) == before
    assert all(np.array_equal(eng.slot_logits(b)[0], lg[b]) for b in range(2))
    release_all(eng)
    begin_open(eng, 0, TEXT, 0, sp, 7)             # the same slot number as the whole run: fed now, it is that run
    eng.slot_text_append(0, rows=rows_of(eng, TEXT, 0, 14), close=True)
    eng.decode_steps(FRAMES)
    assert np.array_equal(eng.slot_codes(0), codes[0])
    release_all(eng)


# ---- the scheduler entry ----
def utterances(n):
    rng = np.random.default_rng(17)
    return [frame_tokens(rng.integers(0, 1000, 6 + 3 * u)) for u in range(n)]


def check_calls(eng, log, nf):
    for u, calls in enumerate(log):
        assert calls and [c[3] for c in calls] == [False] * (len(calls) - 1) + [True], u    # finished once, and last
        at = 0
        for fb, fe, p, fin in calls:
            assert fb == at and (fe > fb or fin), (u, fb, fe)
            assert p.size == (eng.codec_decode_len(fe) if fe else 0) - (eng.codec_decode_len(fb) if fb else 0)
            at = fe
        assert at == nf[u], u


def test_synthesize_live_all_at_once_equals_stream():
    eng, orc, _ = tiny_pair(seed=2, max_batch=2, max_ctx=128)
    orc.close()
    try:
        sp = sampling(SAMPLED, 20)
        toks = utterances(5)
        caps = [20, 7, 13, 1, 16]
        kw = dict(seed=11, ignore_eos=True, max_new_per_utt=caps)
        ref_pcm, ref_codes, ref_nf = eng.synthesize_stream(toks, sp, 4, lambda *a: 0, **kw)
        polls, log = [0] * 5, [[] for _ in toks]

        def source(u):
            polls[u] += 1
            return toks[u], True

        def on_audio(u, fb, fe, pcm, fin):
            log[u].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_live(5, source, sp, 4, on_audio, **kw)
        assert polls == [1] * 5                                       # a closed text is not asked again
        assert list(nf) == caps and np.array_equal(nf, ref_nf)
        for u in range(5):
            assert np.array_equal(codes[u], ref_codes[u]), u
            assert pcm[u].shape == ref_pcm[u].shape and np.array_equal(pcm[u], ref_pcm[u]), u
            assert np.array_equal(np.concatenate([c[2] for c in log[u]]), pcm[u]), u
        check_calls(eng, log, nf)
    finally:
        eng.close()


def test_synthesize_live_trickle_and_cancel():
    eng, orc, _ = tiny_pair(seed=2, max_batch=1, max_ctx=128)
    orc.close()
    try:
        sp = sampling(SAMPLED, 20)
        toks = utterances(3)
        caps = [20, 9, 14]
        kw = dict(seed=11, ignore_eos=True, max_new_per_utt=caps)
        ref_pcm, ref_codes, ref_nf = eng.synthesize_stream(toks, sp, 4, lambda *a: 0, **kw)
        given, polls, log = [0] * 3, [0] * 3, [[] for _ in toks]

        def source(u):
            polls[u] += 1
            if polls[u] % 3 == 0:
                return [], False                                      # nothing yet
            a = given[u]
            given[u] = min(a + 2, len(toks[u]))
            return toks[u][a: given[u]], given[u] == len(toks[u])

        def on_audio(u, fb, fe, pcm, fin):
            log[u].append((fb, fe, pcm, fin))
            return 0
        pcm, codes, nf = eng.synthesize_live(3, source, sp, 4, on_audio, **kw)
        assert list(nf) == caps and given == [len(t) for t in toks]
        for u in range(3):
            assert np.array_equal(codes[u], ref_codes[u]), u
            d = float(np.abs(pcm[u] - ref_pcm[u]).max())
            print("utterance %d: max |pcm difference| = %g" % (u, d))
            assert pcm[u].shape == ref_pcm[u].shape and d < ABS, u
        check_calls(eng, log, nf)
        # (c) either callback can end the job; the slots are free afterwards
        for src, aud in ((lambda u: None, lambda *a: 0), (lambda u: (toks[u], True), lambda *a: 1)):
            with pytest.raises(RuntimeError, match="cancelled by callback"):
                eng.synthesize_live(3, src, sp, 4, aud, **kw)
            with pytest.raises(RuntimeError, match="not armed"):
                eng.slot_text_append(0, close=True)
            assert eng.slot_text_status(0)[1:] == (False, False)
    finally:
        eng.close()


def read_wav_bytes(path):
    return open(path, "rb").read()


def test_cli_feed_equals_unfed(tmp_path):
    """leaxer-tts --feed K: the tokens reach the engine K at a time through the live entry; codes file and WAV equal the unfed run's"""
    common = ["-m", "synthetic:0", "--tokens", "1001,2002,3003,4004,5005,6006,7007,8008,9009", "--stream-chunk", "5", "--max-tokens", "12", "--seed", "4"]
    out = {}
    for name, extra in (("fed", ["--feed", "2"]), ("unfed", [])):
        wav, codes = tmp_path / (name + ".wav"), tmp_path / (name + ".txt")
        r = subprocess.run([CLI, "-o", str(wav), "--save-codes", str(codes)] + common + extra, capture_output=True, text=True, timeout=600)   # a fresh child process per run
        assert r.returncode == 0 and "Streamed" in r.stdout and "Codes saved to" in r.stdout, r.stdout + r.stderr
        assert ("Text fed in" in r.stdout) == (name == "fed")
        out[name] = (open(codes).read(), read_wav_bytes(wav))
    assert out["fed"][0] == out["unfed"][0] and len(out["fed"][0].splitlines()) > 0
    assert out["fed"][1] == out["unfed"][1] and len(out["fed"][1]) > 44
