"""The talker's and the predictor's attention kernels under PEAKED softmax, against float64 (tests/attn_peak_ref.py).

Every other parity test of these stacks runs unit norm gains on `randn * 0.05` rows: no probability passes 0.21 and every rescale
`exp(m_old - m_new)` of the online softmaxes stays within e^+-7 of 1, so a dropped rescale or a merge weight taken against the wrong
maximum moves the logits by little.  Here the scores span 30 to 150 (tests/test_cpu_attn_peak_ref.py asserts it), the same bug is an
O(1) error, and every path that merges softmax state is run: engine logits and normalised hidden rows of EVERY row of a run against
`stack_forward64` on the same tensors.

Bound, one rule for every case: B1 * max(1, eo_g / eo_1) * 2.  B1 is the suite's bound for the path at gain 1 (2e-4 for one-row and
short-context paths and the long prefill, 3e-4 for the batched step over split contexts, 2e-2 with the bf16 KV cache); eo_g / eo_1 is
the CPU oracle's own error against float64 on the scenario over its error on the scenario's gain-1 twin — how much the peaked softmax
amplifies fp32 rounding — and 2 allows that two implementations' noise is not amplified identically.  Both come from the CPU; the
bound never sees the engine's output.  (The oracle's error covers every row's logits and the last hidden row, one prefill pass.)

Paths (config_2l of attn_peak_ref: 0.6B widths, two layers; knobs in os.environ for the engine's life, FLAG_TEST_HOOKS):
  b1-kvh          max_batch 1, max_ctx 256: k_attn<128, 4> over 64-token splits + k_oproj_kvh (per-KV-head merge); 8-row prefill (new rows
                  consumed from LDS), teacher-forced decode to context 200 — contexts 64/65, 128/129, 192/193 cross a split boundary
  b1-prologue     the same with Q3TTS_KVH_OPROJ=0: the merge in the o_proj GEMV's prologue
  b1-bf16kv       FLAG_KV_BF16, reference with K / V rounded to bf16; peaked4 only
  b1-ctx64-p8/16  max_ctx 64: one split, rows written directly; prefill of 8 and of 16 rows, decode to context 60.  Its gate: run_layers
                  sends a one-row pass at base <= 16 of ANY fp32 stack with one 64-token page through the fused
                  predictor kernel, so these engines' decode steps at positions 8..16 run k_cp_attn_kvh on the talker's weights (the
                  only way to reach that kernel at depth with free input rows) and k_attn from position 17 on
  b1-ctx64-oproj  the same with Q3TTS_KVH_OPROJ=0: k_cp_attn_oproj at positions 8..16
  b1-ctx64-kattn  the same with FLAG_NO_FUSED_CP: k_attn at every position
  b1-tiny         config_tiny (head_dim 16), max_ctx 256, to context 140: the D = 16 instantiation and, K = 64 being no GEMV fast path,
                  k_attn_combine in front of the plain GEMV; peaked scenarios only (the planted layer needs the 2l widths)
  b16-splits      max_batch 16, max_ctx 256, Q3TTS_ATTN_STREAM=0 / ATTN_CHUNK=64 / ATTN_KEEP_SPLITS: MFMA step, k_attn partials +
                  k_attn_combine; talker_prefill_dev 8 rows, talker_decode_dev to context 200, rows 0 and 9 on inputs of their own
  b16-splits6     the same at max_ctx 384, to context 330: six splits — k_attn_combine merges splits in batches of four, and only a second
                  batch makes its cross-batch rescale live (no other test of the suite gives that launch more than four); three scenarios
  b32-stream-one  max_batch 32, max_ctx 256: >= 256 (row, KV head) pairs, so ONE split walks the whole context in several batches with an
                  online softmax across them and writes the planes itself — k_attn_stream's one-split form; b32-kattn-one
                  (Q3TTS_ATTN_STREAM_ONE=0): k_attn's.  Where the 64-utterance bench spends most of its steps
  b16-stream      Q3TTS_ATTN_STREAM_CHUNK=64 / ATTN_KEEP_SPLITS: k_attn_stream over one-page splits + k_attn_combine; -bf16kv: its 16-bit cache
  b16-ctx64-stream   max_batch 16, max_ctx 64: one split, planes written directly.  Gate: with attn_stream_one (default) that launch is
                  k_attn_stream's one-split form, not k_attn ...
  b16-ctx64-kattn ... which Q3TTS_ATTN_STREAM=0 brings back
  prefill-long    one 196-row prompt through k_prefill_append + k_attn_prefill (every row's logits, last hidden row), then 4 decode
                  steps that read every cached row; -chunk16: Q3TTS_PREFILL_CHUNK=16 (12 chunks and a 4-row GEMV-family tail)
  cp-*            eng.code_predictor(seq[:n], n - 2), n = 2..16, all 15 heads, free rows.  Gate: n = 2 is the fused kernel
                  (k_cp_attn_kvh; cp-oproj: k_cp_attn_oproj), n >= 3 exceeds its two new rows and runs k_attn<128, 2> with n new rows from
                  LDS; cp-general (FLAG_NO_FUSED_CP) k_attn for n = 2 as well.  k_attn_tiny / k_attn_tiny2 need >= 2 batch rows, which
                  this entry point never has: cp-general-notiny (Q3TTS_NO_ATTN_TINY) pins that: it must equal cp-general bit for bit
  step-*          the fused step's KV-cached predictor passes (two new rows at base 0, then one at bases 2..15) read back through
                  step_logits and teacher-forced on the codes the engine drew: step-b1 k_cp_attn_kvh (+ the layer-0 QKV table),
                  step-b1-oproj k_cp_attn_oproj, step-b2 k_attn_tiny2 (two armed slots), step-b2-tiny k_attn_tiny (Q3TTS_ATTN_TINY2=0),
                  step-b2-kattn k_attn (Q3TTS_NO_ATTN_TINY).  Inputs are embedding rows, so peaked scenarios only.

Measured on the MI355X, engine error / bound (the worse of a batch's two checked rows); all 130 cases pass:
  path                  peaked4           peaked16          recency           peak_at_0         peak_at_mid       oldest_first
  b1-kvh                5.2e-05 / 1.7e-03 2.1e-04 / 7.1e-03 1.8e-05 / 1.4e-03 1.4e-05 / 4.0e-04 7.6e-05 / 4.9e-04 1.9e-05 / 7.4e-04
  b1-prologue           5.3e-05 / 1.7e-03 2.1e-04 / 7.1e-03 2.0e-05 / 1.4e-03 1.4e-05 / 4.0e-04 7.6e-05 / 4.9e-04 1.9e-05 / 7.4e-04
  b1-bf16kv             9.8e-03 / 1.6e-01 -                 -                 -                 -                 -
  b1-ctx64-p8           3.6e-05 / 8.7e-04 1.9e-04 / 2.6e-03 3.1e-05 / 1.3e-03 1.5e-05 / 4.0e-04 6.1e-05 / 7.1e-04 1.4e-05 / 8.3e-04
  b1-ctx64-p16          5.3e-05 / 8.7e-04 1.6e-04 / 2.6e-03 2.9e-05 / 1.3e-03 1.4e-05 / 4.0e-04 7.0e-05 / 7.1e-04 1.7e-05 / 8.3e-04
  b1-ctx64-oproj        3.6e-05 / 8.7e-04 1.9e-04 / 2.6e-03 3.2e-05 / 1.3e-03 1.5e-05 / 4.0e-04 6.1e-05 / 7.1e-04 1.4e-05 / 8.3e-04
  b1-ctx64-kattn        3.6e-05 / 8.7e-04 1.9e-04 / 2.6e-03 3.1e-05 / 1.3e-03 1.5e-05 / 4.0e-04 6.1e-05 / 7.1e-04 1.4e-05 / 8.3e-04
  b1-tiny               1.4e-05 / 8.0e-04 5.5e-05 / 4.0e-03 -                 -                 -                 -
  b16-splits            1.3e-04 / 3.2e-03 6.3e-04 / 8.6e-03 5.6e-05 / 2.1e-03 2.1e-05 / 6.0e-04 1.7e-04 / 7.4e-04 2.8e-05 / 1.2e-03
  b16-splits6           -                 5.9e-04 / 1.1e-02 5.0e-05 / 2.4e-03 2.0e-05 / 6.0e-04 -                 -
  b16-stream            1.1e-04 / 2.6e-03 6.5e-04 / 8.6e-03 5.7e-05 / 2.1e-03 2.1e-05 / 6.0e-04 1.7e-04 / 7.4e-04 3.0e-05 / 1.2e-03
  b16-stream-bf16kv     8.3e-03 / 1.5e-01 3.8e-02 / 5.4e-01 2.7e-03 / 2.3e-01 7.1e-04 / 3.0e-01 1.5e-03 / 2.0e-01 1.8e-03 / 7.7e-02
  b16-ctx64-stream      1.0e-04 / 8.7e-04 6.6e-04 / 2.2e-03 7.8e-05 / 1.3e-03 2.0e-05 / 4.0e-04 1.3e-04 / 6.5e-04 2.4e-05 / 8.3e-04
  b16-ctx64-kattn       9.6e-05 / 8.7e-04 6.3e-04 / 2.2e-03 7.5e-05 / 1.3e-03 1.9e-05 / 4.0e-04 1.3e-04 / 6.5e-04 2.3e-05 / 8.3e-04
  b32-stream-one        1.1e-04 / 2.6e-03 6.6e-04 / 8.6e-03 7.1e-05 / 2.5e-03 2.0e-05 / 6.0e-04 1.7e-04 / 7.4e-04 3.0e-05 / 1.2e-03
  b32-kattn-one         1.1e-04 / 2.6e-03 6.3e-04 / 8.6e-03 7.2e-05 / 2.5e-03 2.0e-05 / 6.0e-04 1.7e-04 / 7.4e-04 2.8e-05 / 1.2e-03
  prefill-long          8.8e-05 / 1.7e-03 4.2e-04 / 7.1e-03 4.3e-05 / 1.4e-03 1.6e-05 / 4.0e-04 1.3e-04 / 4.9e-04 1.6e-05 / 7.4e-04
  prefill-long-chunk16  8.0e-05 / 1.7e-03 4.2e-04 / 7.1e-03 4.3e-05 / 1.4e-03 1.4e-05 / 4.0e-04 1.3e-04 / 4.9e-04 1.6e-05 / 7.4e-04
  cp-kvh                3.7e-05 / 6.0e-04 1.3e-04 / 1.2e-03 2.8e-05 / 1.4e-03 1.3e-05 / 4.5e-04 1.0e-04 / 8.1e-04 1.4e-05 / 5.5e-04
  cp-oproj              3.7e-05 / 6.0e-04 1.3e-04 / 1.2e-03 2.8e-05 / 1.4e-03 1.3e-05 / 4.5e-04 1.0e-04 / 8.1e-04 1.4e-05 / 5.5e-04
  cp-general            3.7e-05 / 6.0e-04 1.3e-04 / 1.2e-03 2.8e-05 / 1.4e-03 1.3e-05 / 4.5e-04 1.0e-04 / 8.1e-04 1.4e-05 / 5.5e-04
  cp-general-notiny     3.7e-05 / 6.0e-04 1.3e-04 / 1.2e-03 2.8e-05 / 1.4e-03 1.3e-05 / 4.5e-04 1.0e-04 / 8.1e-04 1.4e-05 / 5.5e-04
  step-b1               2.8e-06 / 6.0e-04 6.6e-06 / 1.3e-03 -                 -                 -                 -
  step-b1-oproj         2.4e-06 / 6.0e-04 7.4e-06 / 1.3e-03 -                 -                 -                 -
  step-b2               1.7e-05 / 6.3e-04 5.0e-05 / 1.4e-03 -                 -                 -                 -
  step-b2-tiny          2.2e-05 / 6.3e-04 4.6e-05 / 1.4e-03 -                 -                 -                 -
  step-b2-kattn         1.7e-05 / 6.3e-04 4.6e-05 / 1.4e-03 -                 -                 -                 -
The fp32 engine errors sit 3 to 10 times above the oracle's (bf16-split activations and `__expf` against fp32 and libm) and 3 to 30
times under the bound; with the bf16 cache the rule's ratio (the twin's error is one flipped rounding) leaves the bound 15 to 400
times above the engine.  With `L *= corr; O *= corr;` dropped from k_attn_combine the three b16-splits6 cases fail (errors 3.2, 1.4
and 0.04) and nothing else in the suite does; with `* corr` dropped from the running sum where k_attn consumes a new token, 74 cases
here fail, and so does the flat-softmax attn-splits round of tests/test_gpu_b64.py (0.2 against 2e-4).
"""
import contextlib
import os

import numpy as np
import pytest

import attn_peak_ref as ap
from util import Hip, to_q3cfg

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 7, 11      # input rows of the checked utterances (row 0 / row 9 of a batch)
SPLITS = {"Q3TTS_ATTN_KEEP_SPLITS": "1", "Q3TTS_ATTN_CHUNK": "64", "Q3TTS_ATTN_STREAM": "0"}
STREAM = {"Q3TTS_ATTN_KEEP_SPLITS": "1", "Q3TTS_ATTN_STREAM_CHUNK": "64"}
KV16, NOFUSE = 8, 2         # q3tts.FLAG_KV_BF16, q3tts.FLAG_NO_FUSED_CP

@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    ap.clear()


TALKER_PATHS = {
    "b1-kvh": dict(kind="b1", batch=1, ctx=256, T=200, n0=8),
    "b1-prologue": dict(kind="b1", batch=1, ctx=256, T=200, n0=8, env={"Q3TTS_KVH_OPROJ": "0"}),
    "b1-bf16kv": dict(kind="b1", batch=1, ctx=256, T=200, n0=8, flags=KV16, only=("peaked4",)),
    "b1-ctx64-p8": dict(kind="b1", batch=1, ctx=64, T=60, n0=8),
    "b1-ctx64-p16": dict(kind="b1", batch=1, ctx=64, T=60, n0=16),
    "b1-ctx64-oproj": dict(kind="b1", batch=1, ctx=64, T=60, n0=8, env={"Q3TTS_KVH_OPROJ": "0"}),
    "b1-ctx64-kattn": dict(kind="b1", batch=1, ctx=64, T=60, n0=8, flags=NOFUSE),
    "b1-tiny": dict(kind="b1", which="tiny", batch=1, ctx=256, T=140, n0=8, only=("peaked4", "peaked16")),
    "b16-splits": dict(kind="dev", batch=16, ctx=256, T=200, n0=8, env=SPLITS, b1=3e-4),
    "b16-splits6": dict(kind="dev", batch=16, ctx=384, T=330, n0=8, env=SPLITS, b1=3e-4, only=("peaked16", "recency", "peak_at_0")),
    "b16-stream": dict(kind="dev", batch=16, ctx=256, T=200, n0=8, env=STREAM, b1=3e-4),
    "b16-stream-bf16kv": dict(kind="dev", batch=16, ctx=256, T=200, n0=8, env=STREAM, flags=KV16),
    "b16-ctx64-stream": dict(kind="dev", batch=16, ctx=64, T=60, n0=8),
    "b16-ctx64-kattn": dict(kind="dev", batch=16, ctx=64, T=60, n0=8, env={"Q3TTS_ATTN_STREAM": "0"}),
    "b32-stream-one": dict(kind="dev", batch=32, ctx=256, T=200, n0=8, b1=3e-4),
    "b32-kattn-one": dict(kind="dev", batch=32, ctx=256, T=200, n0=8, env={"Q3TTS_ATTN_STREAM_ONE": "0"}, b1=3e-4),
    "prefill-long": dict(kind="long", batch=1, ctx=256, T=200, n0=196),
    "prefill-long-chunk16": dict(kind="long", batch=1, ctx=256, T=200, n0=196, env={"Q3TTS_PREFILL_CHUNK": "16"}),
}
CP_PATHS = {
    "cp-kvh": dict(),
    "cp-oproj": dict(env={"Q3TTS_KVH_OPROJ": "0"}),
    "cp-general": dict(flags=NOFUSE),
    "cp-general-notiny": dict(flags=NOFUSE, env={"Q3TTS_NO_ATTN_TINY": "1"}),
}
STEP_PATHS = {
    "step-b1": dict(batch=1),
    "step-b1-oproj": dict(batch=1, env={"Q3TTS_KVH_OPROJ": "0"}),
    "step-b2": dict(batch=2),
    "step-b2-tiny": dict(batch=2, env={"Q3TTS_ATTN_TINY2": "0"}),
    "step-b2-kattn": dict(batch=2, env={"Q3TTS_NO_ATTN_TINY": "1"}),
}


@contextlib.contextmanager
def _engine(p):
    """the path's engine on synthetic weights; its knobs stay in the environment while it lives (some are read at every launch)"""
    import q3tts
    env = p.get("env", {})
    os.environ.update(env)
    eng = None
    try:
        cfg, _ = ap.base_weights(p.get("which", "2l"))
        eng = q3tts.Engine(to_q3cfg(cfg), device=0, max_batch=p.get("batch", 1), max_ctx=p.get("ctx", 64), flags=p.get("flags", 0) | q3tts.FLAG_TEST_HOOKS)
        eng.fill_synthetic(seed=0)      # embeddings, text projection, codec: whatever the stacks do not own
        eng.loaded = {}
        yield eng
    finally:
        if eng is not None:
            eng.close()
        for k in env:
            del os.environ[k]


def _load(eng, w):
    """the scenario's stack tensors into the engine (those that differ from what it holds), then finalize"""
    for n, a in w.items():
        if eng.loaded.get(n) is not a:
            eng.set_tensor(n, a)
    eng.loaded = dict(w)
    eng.finalize()


class _Engines:
    """one engine alive at a time: the cases are ordered by path, a new path closes the previous engine"""

    def __init__(self):
        self.name, self.stack, self.eng = None, None, None

    def get(self, name, p):
        if self.name != name:
            self.close()
            self.stack = contextlib.ExitStack()
            self.eng = self.stack.enter_context(_engine(p))
            self.name = name
        return self.eng

    def close(self):
        if self.stack is not None:
            self.stack.close()
        self.name, self.stack, self.eng = None, None, None


@pytest.fixture(scope="module")
def engines():
    h = _Engines()
    yield h
    h.close()


def _cases(paths, scenarios):
    return [pytest.param(pn, sn, id=pn + "-" + sn) for pn, p in paths.items() for sn in p.get("only", scenarios)]


def _err(lg, hn, case, t):
    e = float(np.abs(lg - case["logits"][t]).max())
    return e if hn is None else max(e, float(np.abs(hn - case["hn"][t]).max()))


def _run_host(eng, case, n0, T):
    """prefill of n0 rows (every row's logits, the last row's hidden state), teacher-forced decode of rows n0..T-1 -> worst error"""
    x = case["x"]
    lg, lh = eng.prefill(x[:n0])
    worst = max(max(_err(lg[t], None, case, t) for t in range(n0)), _err(lg[n0 - 1], lh, case, n0 - 1))
    for t in range(n0, T):
        l, h = eng.decode(x[t])
        worst = max(worst, _err(l, h, case, t))
    return worst


def _run_dev(eng, hip, cases, n0, T):
    """16 slots through talker_prefill_dev / talker_decode_dev; slot b of `cases` runs that case's rows, the others filler -> worst error per case"""
    B, H, V = eng.max_batch, eng.cfg.hidden, eng.cfg.vocab
    rng = np.random.default_rng(99)
    x0 = (rng.standard_normal((B, n0, H)) * 0.05).astype(np.float32)
    e = (rng.standard_normal((B, H)) * 0.05).astype(np.float32)
    for b, c in cases.items():
        x0[b] = c["x"][:n0]
    x_d, e_d, lg_d, lh_d = hip.put(x0), hip.alloc(B * H * 4), hip.alloc(B * V * 4), hip.alloc(B * H * 4)
    worst = dict.fromkeys(cases, 0.0)

    def look(t):
        lg, lh = hip.get(lg_d, (B, V), np.float32), hip.get(lh_d, (B, H), np.float32)
        for b, c in cases.items():
            worst[b] = max(worst[b], _err(lg[b], lh[b], c, t))
    eng.talker_prefill_dev(x_d, B, n0, None, lg_d, lh_d)
    look(n0 - 1)
    for t in range(n0, T):
        for b, c in cases.items():
            e[b] = c["x"][t]
        hip.write(e_d, e)
        eng.talker_decode_dev(e_d, B, None, lg_d, lh_d)
        look(t)
    hip.free()
    return worst


@pytest.mark.parametrize("path,name", _cases(TALKER_PATHS, ap.SCENARIOS))
def test_talker_paths(engines, path, name):
    p = dict(TALKER_PATHS[path], name=path)
    eng = engines.get(path, p)
    bf = bool(p.get("flags", 0) & KV16)
    b1 = 2e-2 if bf else p.get("b1", 2e-4)
    which, T, n0 = p.get("which", "2l"), p["T"], p["n0"]
    cases = {0: ap.talker_case(which, name, T, SEED_A, bf)}
    _load(eng, cases[0]["w"])
    if p["kind"] == "dev":
        cases[9] = ap.talker_case(which, name, T, SEED_B, bf)
        worst = _run_dev(eng, Hip(), cases, n0, T)
    else:
        worst = {0: _run_host(eng, cases[0], n0, T)}
    bad = []
    for b, c in cases.items():
        bound = ap.bound(b1, c)
        print("%s %s row %d: engine error %.3g, oracle error %.3g (gain-1 twin %.3g), bound %.3g" % (p["name"], name, b, worst[b], c["eo_g"], c["eo_1"], bound))
        if not worst[b] < bound:
            bad.append((b, worst[b], bound))
    assert not bad, bad


_cp_logits = {}


@pytest.mark.parametrize("path,name", _cases(CP_PATHS, ap.SCENARIOS))
def test_predictor_paths(engines, path, name):
    p = dict(CP_PATHS[path], name=path)
    eng = engines.get(path, p)
    c = ap.cp_case(name, SEED_A)
    _load(eng, c["w"])
    got = {n: eng.code_predictor(c["x"][:n], n - 2) for n in c["logits"]}
    worst = max(float(np.abs(got[n] - c["logits"][n]).max()) for n in got)
    bound = ap.bound(2e-4, c)
    print("%s %s: engine error %.3g, oracle error %.3g (gain-1 twin %.3g), bound %.3g" % (p["name"], name, worst, c["eo_g"], c["eo_1"], bound))
    assert worst < bound, (worst, bound)
    _cp_logits[(p["name"], name)] = got
    if p["name"] == "cp-general-notiny":      # one batch row: the tiny kernels are out of reach either way, the knob must change nothing
        for n, a in _cp_logits.get(("cp-general", name), {}).items():
            assert np.array_equal(a, got[n]), n


@pytest.mark.parametrize("path,name", _cases(STEP_PATHS, ("peaked4", "peaked16")))
def test_fused_step_predictor_passes(engines, path, name):
    """One fused step per armed slot, 3 frames: rows 1..15 of step_logits are the predictor's logits behind the frame's sub-code
    decisions; the float64 predictor runs on what the engine fed its own: the slot's hidden row, codec_embed(code0) and
    cp_embed(code j) of the codes it drew."""
    import q3tts
    p = dict(STEP_PATHS[path], name=path, ctx=64)
    eng = engines.get(path, p)
    cfg, w, _, _ = ap.scenario("2l", "cp.", name, 16, SEED_A)
    _, w1, _, _ = ap.scenario("2l", "cp.", name, 16, SEED_A, twin=True)
    _load(eng, w)
    G, H, SV = cfg.n_groups, cfg.hidden, cfg.sub_vocab
    rng = np.random.default_rng(SEED_B)
    sp = q3tts.Sampling(temperature=0.8, top_p=0.95, top_k=50, max_new_tokens=4)
    nb = p["batch"]
    for s in range(nb):
        eng.slot_begin(s, (rng.standard_normal((8, H)) * 0.05).astype(np.float32), (rng.standard_normal((2, H)) * 0.05).astype(np.float32), sp, 5, s, True)
    worst = eo_g = eo_1 = 0.0
    orc, orc1 = ap.new_oracle(cfg, w, 16), ap.new_oracle(cfg, w1, 16)
    try:
        for f in range(3):
            for s in range(nb if f == 0 else 1):      # frame 0: each slot's rows (its step also advances the others); then slot 0 alone
                hid = eng.slot_logits(s)[1]
                lg = eng.step_logits(s)
                codes = eng.slot_codes(s)[-1]
                seq = np.stack([hid, eng.codec_embed([int(codes[0])])[0]] + [eng.cp_embed(int(codes[j + 1]), j) for j in range(G - 2)])
                _, _, st = ap.stack_forward64(cfg, w, "cp.", seq)
                _, _, st1 = ap.stack_forward64(cfg, w1, "cp.", seq)
                for n in range(2, G + 1):
                    head = np.asarray(w["cp.head.%d" % (n - 2)], np.float64).T
                    worst = max(worst, float(np.abs(lg[n - 1, :SV] - st["hn"][n - 1] @ head).max()))
                    eo_g = max(eo_g, float(np.abs(orc.code_predictor(seq[:n], n - 2) - st["hn"][n - 1] @ head).max()))
                    eo_1 = max(eo_1, float(np.abs(orc1.code_predictor(seq[:n], n - 2) - st1["hn"][n - 1] @ head).max()))
    finally:
        orc.close()
        orc1.close()
        for s in range(nb):
            eng.slot_release(s)
    bound = ap.bound(2e-4, dict(eo_g=eo_g, eo_1=eo_1))
    print("%s %s: engine error %.3g, oracle error %.3g (gain-1 twin %.3g), bound %.3g" % (p["name"], name, worst, eo_g, eo_1, bound))
    assert worst < bound, (worst, bound)
