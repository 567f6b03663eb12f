"""The batched decode step at every row-count regime of its kernel dispatch, at the widths that ship, every row against the CPU oracle.

The fused step picks its kernels by row count M (Engine::run_layers, head_proj, launch_gemm2 / 3 / 3_seam, gemm_seam_ok): the nb-row
talker pass and predictor passes 1..14 run M = nb rows, predictor pass 0 runs M = 2 nb.  The sweep walks nb across every switch — GEMV
family / k_gemv16 R8 / 16-row layout / MFMA slab GEMMs, MTILES 1 / 2 / 4, the seam's 32- and 64-row blocks, the nb * nkv >= 256
attention switch, the 128-row block — with the partial tiles and nearly empty row blocks in between (tests/row_sweep_ref.py holds the
config, the utterances and the oracle reference; DESIGN.md, testing section, names the regimes).

Two kinds of step run at each nb.  q3tts_decode_steps replays a captured graph whose width is nb up to 16 rows and nb rounded up to a
multiple of 8 beyond (capped at max_batch = 129): there the rows behind nb are unarmed slots carried through the launches.  The traced
eager step (q3tts_step_logits_host) records exactly nb rows: M = 17, 33, 65, 97, 129 and their doubles reach the kernels there.

Reference semantics per utterance: generate_codes / predict_subcodes of the reference, one utterance at a time; batching is this
build's, so every row of every batch must equal its own single-utterance oracle run."""
import os
import time

import numpy as np
import pytest

import q3_oracle as qo
import row_sweep_ref as rs
from util import tiny_pair, to_q3cfg

pytestmark = pytest.mark.gpu

ROWS_06B = [3, 5, 6, 8, 9, 11, 12, 13, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129]
ROWS_FINISH = [13, 17, 33, 65, 97]
ROWS_17B = [3, 9, 12, 17, 33]
PROMPT_SEED_06B = 135     # seeds 129..134 put more low-margin utterances among the first nb than some nb's cap grants (sweep06's docstring)
PROMPT_SEED_17B = 33
BOUND = rs.NOISE     # fp32 KV cache: the project's logit bound (tests/test_gpu_b64.py logit_bound), a ceiling and not a measurement


class Round:
    """one engine with the prompts of its utterances, and the reference they are held against"""

    def __init__(self, label, eng, ref, max_batch):
        self.label, self.eng, self.ref, self.max_batch = label, eng, ref, max_batch
        self.prompts = [eng.build_prompt(t, 0) for t in ref.toks]


def _build(base, n_utt, prompt_seed, rows, max_batch):
    import q3tts
    ocfg = rs.sweep_config(base)
    t0 = time.time()
    eng, orc, w = tiny_pair(seed=0, max_batch=max_batch, max_ctx=256, ocfg=ocfg)
    ref = rs.Reference(orc, rs.utterances(n_utt, prompt_seed))
    print("row sweep reference: %d utterances x %d greedy frames + teacher-forced pass at hidden %d, %d oracle threads: %.1f s; sub-noise margins "
          "in frames 0..1: %d utterances, in frames 0..%d: %d %s" % (n_utt, rs.FRAMES, ocfg.hidden, orc.threads, time.time() - t0, len(ref.close_01),
                                                                     rs.FRAMES - 1, len(ref.close), sorted(ref.close)))
    ref.assert_caps(rows)      # on the reference alone, before anything is compared with the GPU
    assert isinstance(eng, q3tts.Engine)
    return ocfg, w, eng, orc, ref


@pytest.fixture(scope="module")
def sweep06():
    """0.6B widths, 2 + 2 layers, 129 slots, 256-token contexts (two attention splits: the nb * nkv >= 256 switch is real; at these
    9..13-token contexts the second split is empty), default flags, fp32 KV.  129 utterances, each with 4 free-running greedy oracle
    frames and a teacher-forced pass.  Cost, paid once per module: 21 s on the GPU machine (16 oracle threads), 25 s on 8 threads.
    Utterances with a decision margin below 2e-4 (the only ones a row may be excused on): 2 of 129 in frames 0..1; 4 of 129 in frames 0..3, utterances
    27, 34, 74 and 97 — 1 among the first 32, 2 among the first 64, inside max(1, nb // 16) at every row count (asserted on the
    reference alone, Reference.assert_caps).  The prompt seeds 129..134 were tried first and each breaks the cap at some row count
    (129: utterances 8 and 11 among the first 12)."""
    ocfg, w, eng, orc, ref = _build(qo.config_06b(), 129, PROMPT_SEED_06B, ROWS_06B, 129)
    r = Round("0.6B", eng, ref, 129)
    r.ocfg, r.weights = ocfg, w
    yield r
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def finish06(sweep06):
    """The same weights and reference on an engine created under Q3TTS_SEAM=0 (FLAG_TEST_HOOKS honours the knob): the k_finish*
    launches the split-K seam replaces, at row counts with a partial last tile."""
    import q3tts
    env = {"Q3TTS_SEAM": "0"}
    os.environ.update(env)             # read at engine creation
    try:
        eng = q3tts.Engine(to_q3cfg(sweep06.ocfg), device=0, max_batch=129, max_ctx=256, flags=q3tts.FLAG_TEST_HOOKS)
    finally:
        for k in env:
            del os.environ[k]
    eng.load(sweep06.weights)
    yield Round("0.6B finish launches", eng, sweep06.ref, 129)
    eng.close()


@pytest.fixture(scope="module")
def sweep17():
    """1.7B widths shrunk the same way: talker 2048 wide, predictor 1024 wide behind cp.proj (no sampler planes, cp_project in row
    chunks).  33 utterances with a reference of their own on a 33-slot engine: the graph of the last row count is captured at exactly
    33 rows (widths are rounded up to a multiple of 8 only below max_batch).  Cost: 7.5 s on the GPU machine.  One utterance (27)
    holds a margin below 2e-4 in frames 0..3, none in frames 0..1."""
    ocfg, w, eng, orc, ref = _build(qo.config_17b(), 33, PROMPT_SEED_17B, ROWS_17B, 33)
    yield Round("1.7B", eng, ref, 33)
    eng.close()
    orc.close()


class _Worst:
    def __init__(self):
        self.err, self.where = 0.0, None

    def take(self, err, where):
        if not np.isfinite(err):
            err = float("inf")
        if self.where is None or err > self.err:
            self.err, self.where = float(err), where

    def __str__(self):
        return "%.3g at %s" % (self.err, self.where)


def _sweep(r, nb):
    """One row count on one engine: begin nb slots, 2 graph steps, 2 traced eager steps; every failed comparison is collected, the
    worst figures are printed, then everything is asserted at once (so that a failing row count still shows all its figures)."""
    import q3tts
    eng, ref = r.eng, r.ref
    V, SV, G = eng.cfg.vocab, eng.cfg.sub_vocab, eng.cfg.n_groups
    sp = q3tts.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=rs.FRAMES)
    excused = {}            # row -> (frame, group, oracle margin) of its first, sub-noise divergence
    failures = []

    def row_ref(u, codes_u, upto):
        """(logits, hidden) in front of frames 0..upto of row u: the shared reference, or — past an excused divergence — the
        teacher-forced pass over the engine's own codes"""
        if u in excused:
            return ref.forced(u, codes_u[:upto])
        return ref.logits[u], ref.hidden[u]

    def check_codes(codes, f0, f1):
        for u in range(nb):
            if u in excused:
                continue
            bad = np.argwhere(codes[u][f0:f1] != ref.codes[u][f0:f1])
            if bad.size == 0:
                continue
            f, g = f0 + int(bad[0][0]), int(bad[0][1])
            m = float(ref.margins[u][f, 2 + g])
            print("%s nb=%d: row %d parts from the oracle at frame %d group %d, oracle decision margin %.3g" % (r.label, nb, u, f, g, m))
            if m < rs.NOISE and u in ref.close:
                excused[u] = (f, g, m)
            else:
                failures.append(("codes", u, f, g, m))

    def check_talker(worst, codes, f, tag):
        """slot_logits of every row against what the oracle holds in front of frame f"""
        for u in range(nb):
            lg, lh = eng.slot_logits(u)
            lo, ho = row_ref(u, codes[u] if codes is not None else None, f)
            worst.take(max(float(np.abs(lg - lo[f]).max()), float(np.abs(lh - ho[f]).max())), "row %d" % u)
        if not worst.err < BOUND:
            failures.append((tag, str(worst)))

    # step 1: utterance u into slot u, the prefill's logits and hidden row
    for b in range(r.max_batch):
        eng.slot_release(b)
    for u in range(nb):
        p, t = r.prompts[u]
        eng.slot_begin(u, p, t, sp, seed=rs.SEED, stream_id=u, ignore_eos=True)
    w_prefill, w_graph, w_eager, w_cp = _Worst(), _Worst(), _Worst(), _Worst()
    check_talker(w_prefill, None, 0, "prefill logits")

    # step 2: two frames through the captured graph
    eng.decode_steps(2)
    codes = [eng.slot_codes(u) for u in range(nb)]
    assert all(c.shape == (2, G) for c in codes)
    check_codes(codes, 0, 2)
    check_talker(w_graph, codes, 2, "talker logits behind 2 graph steps")

    # step 3: two traced eager steps at exactly nb rows: the last row, then the first row of the last 16-row tile
    for f, s in ((2, nb - 1), (3, 16 * ((nb - 1) // 16))):
        before, _ = eng.slot_logits(s)
        tr = eng.step_logits(s)
        codes = [eng.slot_codes(u) for u in range(nb)]
        assert all(c.shape == (f + 1, G) for c in codes)
        if not np.array_equal(tr[0, :V], before):
            failures.append(("trace row 0 is not the slot's logits row", s, f))
        _, ho = row_ref(s, codes[s], f)
        po = ref.predictor_logits(ho[f], codes[s][f])
        err = np.abs(tr[1:, :SV] - po).max(axis=1)
        j = int(np.argmax(np.where(np.isfinite(err), err, np.inf)))
        w_cp.take(float(err[j]), "row %d frame %d group %d" % (s, f, j + 1))
        check_codes(codes, f, f + 1)
        check_talker(w_eager, codes, f + 1, "talker logits behind the eager step of frame %d" % f)
    if not w_cp.err < BOUND:
        failures.append(("predictor logits", str(w_cp)))

    line = ("row sweep %s nb=%d: prefill %s | talker behind 2 graph steps %s | talker behind eager steps %s | predictor logits %s | "
            "excused rows %d of cap %d %s" % (r.label, nb, w_prefill, w_graph, w_eager, w_cp, len(excused), rs.cap(nb), sorted(excused.items())))
    print(line)
    assert not failures, (failures, line)
    assert len(excused) <= rs.cap(nb), (sorted(excused.items()), rs.cap(nb))


@pytest.mark.parametrize("nb", ROWS_06B)
def test_every_row_at_every_row_count(sweep06, nb):
    """nb utterances begun into slots 0..nb-1 of the 129-slot engine; 2 graph steps, then 2 traced eager steps.  Every row: prefill
    logits / hidden, codes of frames 0..3 (a divergence excused only on an oracle margin below 2e-4, at most max(1, nb // 16) rows),
    talker logits / hidden in front of frames 2, 3 and 4 within 2e-4.  Two rows: the traced talker row bit-identical to the slot's, the
    15 predictor logits rows within 2e-4 of the uncached reference pattern over the engine's own codes.
    Measured figures: profiles/row_sweep.txt."""
    _sweep(sweep06, nb)


@pytest.mark.parametrize("nb", ROWS_FINISH)
def test_finish_launches_at_partial_tiles(finish06, nb):
    """Q3TTS_SEAM=0: the finish launches behind the slab GEMMs instead of the seam, at 13 rows (one partial tile) and one row past
    each MTILES / row-block switch."""
    _sweep(finish06, nb)


@pytest.mark.parametrize("nb", ROWS_17B)
def test_projected_predictor_at_17b_widths(sweep17, nb):
    """1.7B widths: K = 2048 talker projections, cp.proj in front of every predictor pass (2 nb rows in pass 0), no sampler planes."""
    _sweep(sweep17, nb)
