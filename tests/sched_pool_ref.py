"""Checker of the scheduler's page growth and preemption (helper, not a test): a teacher-forced walk of the CPU oracle along the codes
an engine produced, every sampling decision judged on its own, and the inputs tests/test_gpu_sched_pool.py and
tests/test_sched_pool_surface.py share.

q3tts_synthesize_schedule_host has two page policies.  With EOS suppressed it reserves prompt + cap at admission; otherwise a slot owns
what its context has reached, grows before every look, and the youngest utterance is preempted (and generated again from its prompt)
when the pool runs dry.  The second policy decides where K / V rows land while an utterance runs, so a mistake in it changes ids some
frames later; the walk below follows the engine's own codes, so that one excused decision does not end the comparison and every later
decision is still held against the oracle.

NOISE = 2e-4 is the bound the suite asserts on |HIP logit - oracle logit| (tests/test_gpu_full.py): a decision whose oracle margin
(q3o_sample_margin: top-k gap, top-p cut, distance of the draw from the drawn interval's edges) is below it may legitimately fall the
other way on the GPU; any other must be the oracle's."""
import numpy as np

import q3_oracle as qo
from continue_ref import fold_rows
from penalty_ref import penalise, suppress
from util import frame_tokens

NOISE = 2e-4
WEIGHT_SEED = 31                                            # qo.random_weights(qo.config_tiny(), 31), as tests/test_gpu_kvpool.py
MAX_CTX = 320                                               # 5 pages of 64 tokens per slot
SAMPLING = dict(temperature=0.9, top_p=0.95, top_k=30)
SURFACE_SHARE = 0.06                                        # oracle alone: sub-noise decisions on its own trajectory, per input set
EXCUSED_SHARE = 1.0 / 8                                     # walk along the GPU's trajectory: 2.4 x the measured oracle-alone 5.1 %


def osampling(cap, penalty=1.0):
    return qo.Sampling(SAMPLING["temperature"], SAMPLING["top_p"], SAMPLING["top_k"], penalty, int(cap))


def _frame(orc, sp, seed, stream, f, last, lh, history, penalty, ignore_eos, follow):
    """the oracle's G decisions of frame f in front of which the talker gave (last, lh): (ids, margins).  code0 on the penalised, then
    suppressed row; the sub-codes through the predictor on lh and the codes of `follow` (the frame as the engine has it) or, with
    follow None, the oracle's own.  An EOS decision ends the frame: ids = [eos], margins = [m0]."""
    cfg = orc.cfg
    row = suppress(cfg, penalise(last, history, penalty), ignore_eos)
    c0, m0 = orc.sample_margin(row, sp, qo.rng_uniform(seed, stream, f, 0))
    ids, mgs = [c0], [m0]
    lead = c0 if follow is None else int(follow[0])
    if lead == cfg.codec_eos:
        return ids, mgs
    seq = [lh, orc.codec_embed([lead])[0]]
    for j in range(cfg.n_groups - 1):
        sc, mj = orc.sample_margin(orc.code_predictor(np.stack(seq), j), sp, qo.rng_uniform(seed, stream, f, j + 1))
        ids.append(sc)
        mgs.append(mj)
        seq.append(orc.cp_embed(sc if follow is None else int(follow[j + 1]), j))
    return ids, mgs


def replay(orc, prompt_rows, trailing, pad, codes, sp, seed, stream, forced=0, penalty=1.0, ignore_eos=False):
    """Teacher-forced walk along `codes` [F][G] (the first `forced` frames given, not decided): prefill(prompt_rows), then per frame the
    decode of its input row (continue_ref.fold_rows: the frame's 16 embeddings plus its text row).  Returns (ids, margins), both
    [F + 1][G]: the oracle's decision and its margin at every point of that trajectory, -1 / inf where nothing is decided (forced
    frames; row F, the decision behind the last frame, holds code0 only, and only when the utterance stopped short of its cap
    sp.max_new_tokens with EOS allowed)."""
    cfg = orc.cfg
    G = cfg.n_groups
    codes = np.asarray(codes, np.int64).reshape(-1, G)
    F = codes.shape[0]
    ids = np.full((F + 1, G), -1, np.int64)
    mgs = np.full((F + 1, G), np.inf, np.float64)
    lg, lh = orc.prefill(prompt_rows)
    last, lh = lg[-1].copy(), lh.copy()
    ended = not ignore_eos and F - forced < sp.max_new_tokens
    for f in range(F + 1):
        if f >= forced and (f < F or ended):
            i_f, m_f = _frame(orc, sp, seed, stream, f, last, lh, codes[:f, 0], penalty, ignore_eos, codes[f] if f < F else [cfg.codec_eos])
            ids[f, :len(i_f)], mgs[f, :len(m_f)] = i_f, m_f
        if f < F:
            last, lh = orc.decode(fold_rows(orc.codec_embed, orc.cp_embed, codes[f:f + 1], f, trailing, pad)[0])
    return ids, mgs


def replay_verdict(orc, prompt_rows, trailing, pad, codes, sp, seed, stream, forced=0, penalty=1.0, ignore_eos=False, label=""):
    """replay() judged: every decision behind the forced frames equals the oracle's, or the oracle's margin there is below NOISE
    (excused); with EOS allowed, an utterance shorter than its cap has EOS as the oracle's decision behind its last frame, or that
    decision is excused by the same rule.  Anything else fails, naming frame and group.  Returns (decisions checked, excused)."""
    codes = np.asarray(codes, np.int64).reshape(-1, orc.cfg.n_groups)
    F = codes.shape[0]
    ids, mgs = replay(orc, prompt_rows, trailing, pad, codes, sp, seed, stream, forced, penalty, ignore_eos)
    assert forced <= F <= forced + sp.max_new_tokens, (label, forced, F, sp.max_new_tokens)
    got = np.concatenate([codes, np.full((1, codes.shape[1]), -1, np.int64)])
    got[F, 0] = orc.cfg.codec_eos
    checked = ids >= 0
    wrong = checked & (ids != got)
    for f, g in np.argwhere(wrong):
        what = "the end (the oracle decides %d, not EOS)" % ids[f, g] if f == F else "the engine has %d, the oracle %d" % (got[f, g], ids[f, g])
        assert mgs[f, g] < NOISE, "%s: frame %d group %d: %s, although the oracle's margin there is %.3g" % (label, f, g, what, mgs[f, g])
    return int(checked.sum()), int(wrong.sum())


def same_up_to_noise(codes_a, codes_b, ids_a, mgs_a, label=""):
    """margin-aware equality of two engine runs of one utterance whose launches differ (another live set, another prefill route): equal,
    or the first decision at which they part — a frame one of them does not have counts as its EOS — has an oracle margin below NOISE
    on run a's trajectory (replay() of codes_a; the two trajectories are one up to there).  Returns the number of equal frames."""
    G = ids_a.shape[1]
    a, b = np.asarray(codes_a, np.int64).reshape(-1, G), np.asarray(codes_b, np.int64).reshape(-1, G)
    n = min(len(a), len(b))
    bad = np.argwhere(a[:n] != b[:n])
    if bad.size == 0 and len(a) == len(b):
        return n
    f, g = (int(bad[0][0]), int(bad[0][1])) if bad.size else (n, 0)   # (n, 0): one run ended there, the other went on
    assert mgs_a[f, g] < NOISE, "%s: the runs part at frame %d group %d although the oracle's margin there is %.3g" % (label, f, g, mgs_a[f, g])
    return f


def free_run(orc, prompt_rows, trailing, pad, sp, seed, stream, prefix=None, penalty=1.0, ignore_eos=False):
    """the oracle's own generation behind the forced frames `prefix`, by the same frame function: (codes [F][G] with the prefix in
    front, margins of every decision taken, flat — the EOS decision included)"""
    G = orc.cfg.n_groups
    codes = [] if prefix is None else [list(map(int, fr)) for fr in np.asarray(prefix, np.int64).reshape(-1, G)]
    forced = len(codes)
    lg, lh = orc.prefill(prompt_rows)
    last, lh = lg[-1].copy(), lh.copy()
    for f in range(forced):
        last, lh = orc.decode(fold_rows(orc.codec_embed, orc.cp_embed, [codes[f]], f, trailing, pad)[0])
    mgs = []
    for f in range(forced, forced + sp.max_new_tokens):
        ids, m = _frame(orc, sp, seed, stream, f, last, lh, [c[0] for c in codes], penalty, ignore_eos, None)
        mgs += m
        if ids[0] == orc.cfg.codec_eos:
            break
        codes.append(ids)
        last, lh = orc.decode(fold_rows(orc.codec_embed, orc.cp_embed, [ids], f, trailing, pad)[0])
    return np.array(codes, np.int64).reshape(-1, G), np.array(mgs, np.float64)


# ---- the inputs the GPU tests share; tests/test_sched_pool_surface.py pins what they must offer, on the oracle alone ----
class Job:
    """one scheduler job: token lists, framed instruction ids per utterance (None: none), forced-frame counts, caps on the new frames,
    sampling seed, repetition penalty.  A continued utterance's forced frames are the first F0 of its own EOS-suppressed generation
    with the job's penalty (the GPU tests take them from the ample-pool engine, the surface test from the oracle)."""

    def __init__(self, name, seed, lens, caps, instruct_rows=None, joins=None, penalty=1.0, prompt_seed=0, lang=0):
        import q3tts
        rng = np.random.default_rng(prompt_seed)
        n = len(lens)
        self.name, self.seed, self.penalty, self.lang, self.n = name, seed, penalty, lang, n
        self.toks = [frame_tokens(rng.integers(0, 1000, k)) for k in lens]
        self.caps = np.array(caps, np.int32)
        self.cap = int(self.caps.max())
        self.joins = list(joins) if joins is not None else [0] * n
        made = {}
        for r in sorted(set(instruct_rows or []) - {0}):   # one id array per distinct length: equal lengths share an instruction
            made[r] = q3tts.frame_instruct_ids(rng.integers(0, 1000, r - 5))
            assert len(made[r]) == r
        self.instructs = [made.get(r) for r in (instruct_rows or [0] * n)]

    def oracle_prompt(self, orc, u):
        """(prompt rows with the instruction's rows in front, trailing rows, pad row) of utterance u"""
        p = orc.build_prompt(self.toks[u], self.lang)
        tr, pad = orc.trailing()
        if self.instructs[u] is not None:
            p = np.concatenate([orc.text_project(self.instructs[u]), p])
        return p, tr.copy(), pad.copy()


def jobs():
    """the five input sets, by name"""
    return {j.name: j for j in (
        Job("prefixed", JOB_SEEDS["prefixed"], (5, 2, 12, 7, 3, 9), (150, 150, 60, 150, 150, 150), instruct_rows=(70, 70, 40, 70, 40, 70), prompt_seed=PROMPT_SEEDS["prefixed"]),
        Job("continued", JOB_SEEDS["continued"], (5, 2, 12, 7, 3), (120, 120, 120, 40, 120), joins=(1, 7, 31, 60, 100), penalty=1.3, prompt_seed=PROMPT_SEEDS["continued"]),
        Job("ragged_instruct", JOB_SEEDS["ragged_instruct"], (5, 2, 12, 7, 3, 9), (150, 150, 150, 60, 150, 150), instruct_rows=(20, 0, 33, 70, 0, 33), prompt_seed=PROMPT_SEEDS["ragged_instruct"]),
        Job("ragged_continued", JOB_SEEDS["ragged_continued"], (5, 2, 12, 7, 3, 9), (120, 120, 120, 120, 40, 120), joins=(12, 0, 60, 0, 5, 31), prompt_seed=PROMPT_SEEDS["ragged_continued"]),
        # 32 utterances for 24 slots.  The first 20 (and every second one behind them) carry one 47-row instruction, unshared: their
        # prompts end at token 55, so prompt + first look fits one page and every one of them crosses into a second page 9 frames in.
        Job("wide32", JOB_SEEDS["wide32"], tuple(1 + (7 * i) % 13 for i in range(32)), tuple(40 - (i % 4) * 6 for i in range(32)),
            instruct_rows=tuple(47 if i < 20 or i % 2 else 0 for i in range(32)), prompt_seed=PROMPT_SEEDS["wide32"]),
    )}


# sampling and prompt seeds, picked on the CPU (tests/test_sched_pool_surface.py states what each set must offer and prints what it has)
JOB_SEEDS = {"prefixed": 13, "continued": 9, "ragged_instruct": 15, "ragged_continued": 2, "wide32": 13}
PROMPT_SEEDS = {"prefixed": 4, "continued": 4, "ragged_instruct": 4, "ragged_continued": 4, "wide32": 4}


def oracle_run(orc, job, u):
    """utterance u of `job` on the oracle alone: (codes, margins, forced), a continued one behind its own EOS-suppressed frames"""
    p, tr, pad = job.oracle_prompt(orc, u)
    F0 = job.joins[u]
    prefix = None
    if F0:
        prefix, _ = free_run(orc, p, tr, pad, osampling(F0, job.penalty), job.seed, u, penalty=job.penalty, ignore_eos=True)
    codes, mg = free_run(orc, p, tr, pad, osampling(job.caps[u], job.penalty), job.seed, u, prefix=prefix, penalty=job.penalty)
    return codes, mg, F0
