"""q3tts_synthesize_schedule_host's second page policy — EOS-terminated jobs: a slot owns what its context has reached, grows before
every look, the youngest utterance is preempted when the pool runs dry and is generated again from its prompt — behind every kind of
begin: shared prompt prefixes, teacher-forced frames, the ragged flag, unshared instructions, the bf16 cache, and more than 16 live
utterances (the look = 8 and `quantum` branches).  The reference grows one KVCache per utterance (src/tts_onnx.h:108-115) and has
none of this; the checker is the CPU oracle walked along the engine's own codes (tests/sched_pool_ref.py), every decision judged.

Every case runs its job on an ample pool (no preemption, asserted) and on a pool small enough to preempt (asserted, with
admitted == utterances + preempted).  On config_tiny nothing is grouped into MFMA passes, so at 4 slots the two runs must agree bit for
bit, as tests/test_gpu_kvpool.py::test_on_demand_growth_and_preemption already demands of plain utterances; the tight run's codes are
then held against the oracle (excused decisions: oracle margin below NOISE = 2e-4, at most one in eight of those checked), every
page is back in the pool, and the PCM is the vocoder's decode of the codes within the suite's 2e-5.

tests/test_sched_pool_surface.py shows on the CPU that each input set ends by EOS at three or more lengths, reaches a cap, and has
under 6 % sub-noise decisions on the oracle's own trajectory.

Pool sizes and what they gave on the MI355X are in each test's docstring; each test prints them again."""
import os

import numpy as np
import pytest

import q3_oracle as qo
import sched_pool_ref as R
from util import calibrate_codec, to_q3cfg

pytestmark = pytest.mark.gpu
PCM_BOUND = 2e-5      # max |pcm - codec_decode(codes)|: tests/test_gpu_continue.py


@pytest.fixture(scope="module")
def setup():
    ocfg = qo.config_tiny()
    w = calibrate_codec(qo.random_weights(ocfg, R.WEIGHT_SEED), ocfg)
    orc = qo.Oracle(ocfg, max_ctx=R.MAX_CTX, weights=w)
    yield ocfg, w, orc, R.jobs()
    orc.close()


def _engine(setup, pool_pages, max_batch=4, flags=0):
    import q3tts
    ocfg, w = setup[0], setup[1]
    eng = q3tts.Engine(to_q3cfg(ocfg), device=0, max_batch=max_batch, max_ctx=R.MAX_CTX, flags=flags, kv_pool_tokens=pool_pages * 64)
    eng.load(w)
    return eng


def _sp(job, cap=None, penalty=None):
    import q3tts
    return q3tts.Sampling(repetition_penalty=job.penalty if penalty is None else penalty, max_new_tokens=int(cap or job.cap), **R.SAMPLING)


def _forced_frames(eng, job):
    """the first joins[u] frames of utterance u's own EOS-suppressed generation on `eng` (None where the utterance is not continued)"""
    if not any(job.joins):
        return None
    _, codes, nfr = eng.synthesize_batch(job.toks, _sp(job, max(job.joins)), lang=job.lang, seed=job.seed, ignore_eos=True,
                                         max_new_per_utt=[max(1, f) for f in job.joins])
    for u, f in enumerate(job.joins):
        assert nfr[u] == max(1, f)
    return [codes[u][:f].copy() if f else None for u, f in enumerate(job.joins)]


def _run(eng, job, how, forced=None, penalty=None):
    """the job through one entry: (pcm, codes, n_frames, (admitted, preempted, peak live))"""
    sp = _sp(job, penalty=penalty)
    kw = dict(lang=job.lang, seed=job.seed, max_new_per_utt=job.caps)
    if how == "prefixed":       # q3tts_synthesize_prefixed_host: one shared prefix per distinct instruction
        made = {}
        try:
            for t in job.instructs:
                if t is not None and t.tobytes() not in made:
                    made[t.tobytes()] = eng.prefix_create_instruct(t)
            out = eng.synthesize_prefixed(job.toks, [None if t is None else made[t.tobytes()] for t in job.instructs], sp, **kw)
        finally:
            for pid in made.values():
                eng.prefix_release(pid)
    elif how == "continue":     # q3tts_synthesize_continue_host
        out = eng.synthesize_continue(job.toks, forced, sp, **kw)
    elif how == "instruct":     # q3tts_synthesize_instruct_host: every instruction prefilled with its prompt
        out = eng.synthesize_batch(job.toks, sp, instructs=job.instructs, **kw)
    else:                       # "shared": synthesize_batch(share_instructs=True) makes and releases the prefixes itself
        assert how == "shared"
        out = eng.synthesize_batch(job.toks, sp, instructs=job.instructs, share_instructs=True, **kw)
    return out + (eng.sched_stats(),)


def _joins(job, forced):
    return [0 if forced is None or forced[u] is None else len(forced[u]) for u in range(job.n)]


def _check_frames(job, codes, nfr, forced):
    F0 = _joins(job, forced)
    for u in range(job.n):
        assert codes[u].shape[0] == nfr[u] and F0[u] < nfr[u] <= F0[u] + job.caps[u], (u, nfr[u])
        if F0[u]:
            assert np.array_equal(codes[u][:F0[u]], forced[u]), u


def _check_pcm_and_pool(eng, job, pcm, codes, forced, pool_pages):
    assert eng.kv_pool_info() == (64, pool_pages, pool_pages)          # every page came back
    F0 = _joins(job, forced)
    worst = 0.0
    for u in range(job.n):
        whole = eng.codec_decode(codes[u])
        own = whole[eng.codec_decode_len(F0[u]):] if F0[u] else whole
        assert pcm[u].shape == own.shape and own.size > 0, (u, pcm[u].shape, own.shape)
        worst = max(worst, float(np.abs(pcm[u] - own).max()))
    assert worst <= PCM_BOUND, worst
    return worst


def _replay(setup, job, codes, forced, which=None, penalty=None):
    """replay_verdict of the utterances `which` (all): (checked, excused) summed, and the walks for later comparisons"""
    orc = setup[2]
    F0 = _joins(job, forced)
    pen = job.penalty if penalty is None else penalty
    checked = excused = 0
    for u in (range(job.n) if which is None else which):
        p, tr, pad = job.oracle_prompt(orc, u)
        n, x = R.replay_verdict(orc, p, tr, pad, codes[u], R.osampling(job.caps[u], pen), job.seed, u, forced=F0[u], penalty=pen,
                                label="%s utterance %d" % (job.name, u))
        checked, excused = checked + n, excused + x
    return checked, excused


def _walk(setup, job, codes, forced, u):
    p, tr, pad = job.oracle_prompt(setup[2], u)
    return R.replay(setup[2], p, tr, pad, codes[u], R.osampling(job.caps[u], job.penalty), job.seed, u, forced=_joins(job, forced)[u], penalty=job.penalty)


def _pair(setup, job, how, tight_pages, flags=0, oracle=True, label=None):
    """the job on an ample and on a tight pool of `tight_pages`: everything the module docstring lists.  Returns what later checks of
    the same job need: (ample run, tight run, forced frames)."""
    label = label or "%s / %s" % (job.name, how)
    ample = _engine(setup, 0, flags=flags)
    try:
        forced = _forced_frames(ample, job)
        a = _run(ample, job, how, forced)
        assert a[3][1] == 0 and a[3][0] == job.n, a[3]
        _check_frames(job, a[1], a[2], forced)
    finally:
        ample.close()
    tight = _engine(setup, tight_pages, flags=flags)
    try:
        t = _run(tight, job, how, forced)
        admitted, preempted, peak = t[3]
        print("%s: %d-page pool, 4 slots: admitted %d, preempted %d, peak live %d; frames %s" % (label, tight_pages, admitted, preempted, peak, [int(n) for n in t[2]]))
        assert preempted > 0 and admitted == job.n + preempted, t[3]
        assert list(t[2]) == list(a[2]), (list(t[2]), list(a[2]))
        for u in range(job.n):
            assert np.array_equal(t[1][u], a[1][u]), (label, u)           # bit for bit, whichever utterance was preempted
        worst = _check_pcm_and_pool(tight, job, t[0], t[1], forced, tight_pages)
    finally:
        tight.close()
    if oracle:
        checked, excused = _replay(setup, job, t[1], forced)
        print("%s: %d decisions checked against the oracle, %d excused (margin < %.0e); max |pcm - decode(codes)| %.3g" % (label, checked, excused, R.NOISE, worst))
        assert excused <= checked * R.EXCUSED_SHARE, (label, checked, excused)
    return a, t, forced


# pool sizes (pages of 64 tokens) at which the jobs below preempt, found on the MI355X and asserted by every test; one utterance alone
# can need 4 (prefix / instruction + prompt + 150 frames, or prompt + 100 forced + 120 new frames), which is the least a pool may hold
POOL = {"prefixed": 5, "continued": 4, "ragged_instruct": 5, "ragged_continued": 6, "wide32": 35}


def test_shared_prefix(setup):
    """Case 1.  4 utterances behind a 70-row instruction prefix, 2 behind a 40-row one (q3tts_synthesize_prefixed_host): the 70-row
    prefix and the prompt cross the first page edge at the begin, so k_kv_prefix_copy and the own rows' prefill write two scattered
    pages, and pl(u) stands in every page count of the scheduler.  Replay prompt: text_project(instruction) rows, then build_prompt.
    Measured on the MI355X, 5-page pool: admitted 8, preempted 2, peak live 2 (pools of 4 to 7 pages preempt, 8 do not); frames 85,
    112, 60, 7, 150, 125; 8 628 decisions checked, 0 excused; max |pcm - decode(codes)| 0."""
    _pair(setup, setup[3]["prefixed"], "prefixed", POOL["prefixed"])


def test_forced_frames(setup):
    """Case 2.  q3tts_synthesize_continue_host behind 1, 7, 31, 60 and 100 of each utterance's own EOS-suppressed frames (prompt + 60
    crosses 64 tokens at the begin, prompt + 100 starts on the second page), repetition_penalty 1.3: a re-admitted utterance's code0
    history must be exactly its prefix again — the oracle walk penalises over codes[:f, 0], forced frames included — and the forced
    begin is the re-admission.  The penalty acts: the penalty-off run differs.
    Measured on the MI355X, 4-page pool (what one utterance alone can need; 5 pages do not preempt this set): admitted 7, preempted 2,
    peak live 2; frames with their prefixes 121, 30, 143, 99, 120; 5 028 decisions checked, 0 excused; max |pcm - decode(codes)| 0."""
    job = setup[3]["continued"]
    a, t, forced = _pair(setup, job, "continue", POOL["continued"])
    eng = _engine(setup, 0)
    try:
        off = _run(eng, job, "continue", forced, penalty=1.0)
    finally:
        eng.close()
    assert any(off[2][u] != a[2][u] or not np.array_equal(off[1][u], a[1][u]) for u in range(job.n))


def test_ragged_flag(setup):
    """Case 3.  Q3TTS_FLAG_RAGGED_PREFILL: what would be begun on its own joins one q3tts_slots_begin_ragged call per look, fresh
    admissions and re-admissions alike.  One entry point takes instructions or forced frames, not both, so the mix is two jobs on the
    same pair of engines' settings: short prompts beside 20 / 33 / 70-row instruction prompts (S > 16), and short prompts beside
    continued utterances.  (On these dims the ragged call begins its members one at a time — tests/test_gpu_ragged_prefill.py,
    fallback — which is what keeps the ample and the tight run bit-equal; its reservation for the whole set is what is new here.)
    Measured on the MI355X: instructions, 5-page pool: admitted 9, preempted 3, peak live 3; frames 150, 150, 130, 19, 150, 20; 9 907
    decisions checked, 0 excused.  Continued, 6-page pool: admitted 7, preempted 1, peak live 3; frames with their prefixes 87, 89, 126,
    76, 42, 151; 7 413 decisions checked, 0 excused.  max |pcm - decode(codes)| 0 in both."""
    import q3tts
    _pair(setup, setup[3]["ragged_instruct"], "instruct", POOL["ragged_instruct"], flags=q3tts.FLAG_RAGGED_PREFILL)
    _pair(setup, setup[3]["ragged_continued"], "continue", POOL["ragged_continued"], flags=q3tts.FLAG_RAGGED_PREFILL)


def test_instructions_unshared_and_shared(setup):
    """Case 4.  Case 1's utterances with their instructions prefilled per utterance (q3tts_synthesize_instruct_host: prompts of 78 and
    48 rows through the long prefill), and through synthesize_batch(share_instructs=True).  Each is bit-equal to its own ample-pool
    run and passes the oracle walk.  Against each other the two routes differ in launches (instruction + prompt in one prefill, or
    prefix rows copied and the prompt prefilled at a base), so they agree up to the first decision whose oracle margin is below NOISE
    (tests/test_gpu_prefix.py::test_scheduler_prefixed documents the same of its solo and grouped passes).
    Measured on the MI355X, 5-page pool, either route: admitted 8, preempted 2, peak live 2; unshared: 8 628 decisions checked, 0
    excused; all 6 utterances equal between the two routes to their last frame."""
    job = setup[3]["prefixed"]
    _, solo, _ = _pair(setup, job, "instruct", POOL["prefixed"])
    _, shared, _ = _pair(setup, job, "shared", POOL["prefixed"], oracle=False)
    equal = 0
    for u in range(job.n):
        ids, mgs = _walk(setup, job, solo[1], None, u)
        equal += int(R.same_up_to_noise(solo[1][u], shared[1][u], ids, mgs, "utterance %d, unshared vs shared" % u) == len(solo[1][u]) == len(shared[1][u]))
    print("unshared vs shared instructions: %d of %d utterances equal to the end, the rest part at a sub-noise decision" % (equal, job.n))


def test_bf16_cache(setup):
    """Case 5.  Case 1's job with Q3TTS_FLAG_KV_BF16 on both engines: growth and preemption over 16-bit pages.  Bit equality with the
    ample-pool bf16 engine only — the bf16 cache's logit bound (2e-2) would excuse every decision of an oracle walk.
    Measured on the MI355X, 5-page pool: admitted 8, preempted 2, peak live 2; frames 85, 112, 60, 7, 150, 125."""
    import q3tts
    _pair(setup, setup[3]["prefixed"], "prefixed", POOL["prefixed"], flags=q3tts.FLAG_KV_BF16, oracle=False, label="prefixed / bf16 cache")


def _wide(setup, pool_pages, flags=0):
    job = setup[3]["wide32"]
    eng = _engine(setup, pool_pages, max_batch=24, flags=flags)
    try:
        out = _run(eng, job, "instruct")
        _check_frames(job, out[1], out[2], None)
        worst = _check_pcm_and_pool(eng, job, out[0], out[1], None, pool_pages or 24 * 5)
    finally:
        eng.close()
    return out, worst


def test_more_than_16_live(setup):
    """Case 6.  24 slots, 32 utterances with caps of 22..40 frames, a pool on which more than 16 run at once and growth preempts: the
    look = 8 branch, and the `quantum` branch while utterances queue — the batched step's table-mapped attention under a page table
    that changes between looks.  Plain utterances cannot do this: prompt + 40 frames is 49 tokens, one page for life, and admission
    keeps a page of head-room per live utterance, so nothing ever grows into a dry pool.  So 26 of the 32 carry one unshared 47-row
    instruction: prompt + first look fits one page, every one of them needs a second page 9 frames in, and the 18 that a 35-page pool
    admits at once ask for 36.  The ample and the tight run have different live sets, hence different row-count regimes, and with
    Q3TTS_SCHED_QUANTUM=12 the looks fall elsewhere again: the runs agree up to the first decision whose oracle margin is below
    NOISE, and six utterances of the tight run (first, last, four between) pass the oracle walk.
    Measured on the MI355X, 35-page pool, at either quantum: admitted 33, preempted 1, peak live 18 (33 pages: peak 17, preempted 1;
    31 pages: peak 16; 37 pages preempt only at quantum 12); all 32 utterances equal to the ample run and between the quanta to
    their last frame; 2 786 decisions of the six utterances checked, 0 excused; max |pcm - decode(codes)| 0."""
    job = setup[3]["wide32"]
    ample, _ = _wide(setup, 0)
    assert ample[3][1] == 0 and ample[3][0] == job.n, ample[3]
    tight, worst = _wide(setup, POOL["wide32"])
    assert os.environ.get("Q3TTS_SCHED_QUANTUM") is None
    os.environ["Q3TTS_SCHED_QUANTUM"] = "12"                          # read by every job as it starts
    try:
        q12, _ = _wide(setup, POOL["wide32"])
        q12_roomy, _ = _wide(setup, POOL["wide32"] + 2)
    finally:
        del os.environ["Q3TTS_SCHED_QUANTUM"]
    roomy, _ = _wide(setup, POOL["wide32"] + 2)
    # that the knob took and the quantum branch ran: on two pages more a first look of 12 steps already asks for second pages and
    # preempts, the default look of 8 never does
    assert roomy[3][1] == 0 and q12_roomy[3][1] > 0 and roomy[3][2] > 16, (roomy[3], q12_roomy[3])
    for name, run in (("default quantum", tight), ("quantum 12", q12)):
        admitted, preempted, peak = run[3]
        print("wide32, %s: %d-page pool, 24 slots: admitted %d, preempted %d, peak live %d; frames %s" % (name, POOL["wide32"], admitted, preempted, peak, [int(n) for n in run[2]]))
        assert preempted > 0 and admitted == job.n + preempted and peak > 16, run[3]
    walks = {}
    parted = {"ample": 0, "quantum 12": 0}
    for u in range(job.n):
        for name, other in (("ample", ample), ("quantum 12", q12)):
            if len(other[1][u]) != len(tight[1][u]) or not np.array_equal(other[1][u], tight[1][u]):
                if u not in walks:
                    walks[u] = _walk(setup, job, tight[1], None, u)
                R.same_up_to_noise(tight[1][u], other[1][u], walks[u][0], walks[u][1], "utterance %d, tight pool vs %s" % (u, name))
                parted[name] += 1
    checked, excused = _replay(setup, job, tight[1], None, which=(0, 6, 12, 19, 25, 31))
    print("wide32: %d decisions of 6 utterances checked against the oracle, %d excused; utterances that part from the tight run at a sub-noise "
          "decision: %s of %d; max |pcm - decode(codes)| %.3g" % (checked, excused, parted, job.n, worst))
    assert excused <= checked * R.EXCUSED_SHARE, (checked, excused)
