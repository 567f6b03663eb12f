"""Pins tests/attn_peak_ref.py before any GPU result leans on it: the float64 restatement against the CPU oracle at the gains the rest
of the suite runs, and the softmax conditions every peaked scenario claims — asserted from the reference's own statistics, so a seed
that misses one is changed, never the condition.  No GPU.

Measured (config_2l, 200 rows, seed 7; oracle against float64, max over all rows' logits and the last hidden row):
  scenario       largest probability (median)   widest span   oracle error   its gain-1 twin
  gain 1         at most 0.21                   6.8           6.0e-06
  peaked4        0.50                           28            2.6e-05        6.0e-06
  peaked16       0.96                           110           1.1e-04        6.0e-06
  recency        layer 0: 0.06, above: 0.46     81            7.8e-06        2.2e-06
  peak_at_0      layer 0: 1.00, above: 0.34     75            2.4e-06        3.2e-06
  peak_at_mid    layer 0: 1.00, above: 0.43     75            4.0e-06        3.2e-06
  oldest_first   layer 0: 0.06, above: 0.43     81            3.9e-06        2.1e-06"""
import numpy as np
import pytest

import attn_peak_ref as ap

T = 200
SEED = 7
CHECK = tuple(c - 1 for c in (63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 200))     # rows of the checked contexts (row = context - 1)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    ap.clear()


@pytest.mark.parametrize("kv_bf16", [False, True], ids=["fp32kv", "bf16kv"])
def test_reference_matches_the_oracle_at_default_gains(kv_bf16):
    """stack_forward64 against Oracle.prefill + Oracle.decode (talker; 8-row prefill, teacher-forced decode to 72 rows) and
    Oracle.code_predictor (all 15 steps), unit gains: every row's logits and hidden row within the suite's fp32 logit bound, 2e-4
    (measured 4.9e-6, predictor 2.6e-6); with K / V rounded to bf16 in both, that cache mode's bound, 2e-2 (a rounding that flips between float64 and
    fp32 moves a cache entry by one bf16 step)."""
    cfg, w = ap.base_weights("2l")
    n = 72
    x = (np.random.default_rng(SEED).standard_normal((n, cfg.hidden)) * 0.05).astype(np.float32)
    lg, _, st = ap.stack_forward64(cfg, w, "talker.", x, kv_bf16)
    orc = ap.new_oracle(cfg, w, n, kv_bf16)
    olg, olh = orc.prefill(x[:8])
    worst = max(float(np.abs(olg - lg[:8]).max()), float(np.abs(olh - st["hn"][7]).max()))
    for t in range(8, n):
        ol, oh = orc.decode(x[t])
        worst = max(worst, float(np.abs(ol - lg[t]).max()), float(np.abs(oh - st["hn"][t]).max()))
    print("talker, %s: oracle vs float64 over %d rows, max |logit / hidden error| %.3g" % ("bf16 KV" if kv_bf16 else "fp32 KV", n, worst))
    assert worst < (2e-2 if kv_bf16 else 2e-4), worst
    if not kv_bf16:   # the predictor's cache is fp32 in every mode
        _, _, st = ap.stack_forward64(cfg, w, "cp.", x[:16])
        worst = 0.0
        for m in range(1, 17):
            for step in ((m - 2) % 15, 14):
                ref = st["hn"][m - 1] @ np.asarray(w["cp.head.%d" % step], np.float64).T
                worst = max(worst, float(np.abs(orc.code_predictor(x[:m], step) - ref).max()))
        print("predictor: oracle vs float64 over sequences of 1..16 rows, max |logit error| %.3g" % worst)
        assert worst < 2e-4, worst
    orc.close()


def test_bf16_rounding_of_the_reference_is_the_oracles():
    import q3_oracle as qo
    a = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * np.float32(3.0)
    assert np.array_equal(ap.bf16_round64(a.astype(np.float64)).astype(np.float32), qo.bf16_round(a))


def _splits(stats, rows):
    """where the argmax of every (layer, head, checked row) falls: (in the first 64-token split, in a later one but not among the row's
    last 16 keys, among its last 16 keys)"""
    am = stats["argmax"][:, :, rows]
    age = np.asarray(rows)[None, None, :] - am
    return int((am < 64).sum()), int(((am >= 64) & (age >= 16)).sum()), int((age < 16).sum())


@pytest.mark.parametrize("name", ["peaked4", "peaked16"])
def test_random_peaked_scenarios_are_peaked(name):
    c = ap.talker_case("2l", name, T, SEED)
    st = c["stats"]
    pm, span = st["pmax"][:, :, CHECK], st["span"][:, :, CHECK]
    first, later, recent = _splits(st, CHECK)
    print("%s: largest probability median %.2f, > 0.5 in %.0f%% of (layer, head, checked row); widest span %.0f; argmax in first split / later split / last 16 keys: %d / %d / %d; oracle error %.3g (gain-1 twin %.3g)"
          % (name, float(np.median(pm)), 100.0 * float((pm > 0.5).mean()), float(-span.min()), first, later, recent, c["eo_g"], c["eo_1"]))
    assert first >= 1 and later >= 1 and recent >= 1
    if name == "peaked16":
        assert float(-span.min()) > 88.0      # past the point where fp32 exp underflows
        assert float((pm > 0.5).mean()) >= 0.5
    assert np.isfinite(c["eo_g"]) and np.isfinite(c["eo_1"])


def test_gain_8_puts_most_of_the_mass_on_one_key():
    """peaked(8) — what the planted scenarios' upper layers run: the largest probability passes 0.5 for at least half of all
    (layer, head, checked row) (82 % measured, median 0.80)"""
    cfg, w = ap.base_weights("2l")
    x = (np.random.default_rng(SEED).standard_normal((T, cfg.hidden)) * 0.05).astype(np.float32)
    _, _, st = ap.stack_forward64(cfg, ap.peaked(w, "talker.", 8.0), "talker.", x)
    pm = st["pmax"][:, :, CHECK]
    print("peaked8: largest probability median %.2f, > 0.5 in %.0f%%" % (float(np.median(pm)), 100.0 * float((pm > 0.5).mean())))
    assert float((pm > 0.5).mean()) >= 0.5
    _, _, st1 = ap.stack_forward64(cfg, w, "talker.", x)
    print("gain 1 (what the rest of the suite runs): largest probability at most %.3f, widest span %.1f" % (float(st1["pmax"][:, :, CHECK].max()), float(-st1["span"][:, :, CHECK].min())))
    assert float(st1["pmax"][:, :, CHECK].max()) < 0.25      # the gap this file's scenarios close


@pytest.mark.parametrize("name", ap.PROFILES)
def test_planted_profiles_peak_where_planted(name):
    """layer 0 of every planted profile: the argmax of every head and EVERY row (not only the checked ones) sits where the profile puts
    it, the span is the closed form's sqrt(d) * gain * (cos range), and the run stays finite in the oracle and in float64"""
    c = ap.talker_case("2l", name, T, SEED)
    st = c["stats"]
    assert np.array_equal(st["argmax"][0], np.broadcast_to(c["where"], st["argmax"][0].shape))
    if name == "recency":
        assert np.array_equal(c["where"], np.arange(T))
    elif name == "peak_at_mid":
        assert (c["where"][70:] == 70).all() and (c["where"][:70] < 70).all()
    else:
        assert (c["where"] == 0).all()
    span0 = float(-st["span"][0][:, CHECK[-1]].min())
    print("%s: layer-0 span at row %d %.0f, layer-0 largest probability median %.2f, upper layers' %.2f; oracle error %.3g (gain-1 twin %.3g)"
          % (name, CHECK[-1], span0, float(np.median(st["pmax"][0][:, CHECK])), float(np.median(st["pmax"][1:][:, :, CHECK])), c["eo_g"], c["eo_1"]))
    assert span0 > 60.0
    if name.startswith("peak_at"):
        assert float(st["pmax"][0][:, 130:].min()) > 0.999      # one key holds the mass
    assert np.isfinite(c["logits"]).all() and np.isfinite(c["eo_g"]) and np.isfinite(c["eo_1"])


@pytest.mark.parametrize("name", ap.SCENARIOS)
def test_predictor_scenarios(name):
    """the same scenarios through the predictor's 16 free rows: planted argmax in place, oracle error finite and printed"""
    c = ap.cp_case(name, SEED)
    st = c["stats"]
    if c["where"] is not None:
        assert np.array_equal(st["argmax"][0], np.broadcast_to(c["where"], st["argmax"][0].shape))
    print("predictor %s: largest probability median %.2f, widest span %.0f; oracle error %.3g (gain-1 twin %.3g)"
          % (name, float(np.median(st["pmax"][:, :, 2:])), float(-st["span"].min()), c["eo_g"], c["eo_1"]))
    assert np.isfinite(c["eo_g"]) and np.isfinite(c["eo_1"])
