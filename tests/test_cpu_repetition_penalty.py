"""repetition_penalty on the CPU: the checker the GPU tests compare against (tests/penalty_ref.py) is itself checked against the oracle
with the penalty off, the penalty rule against hand-written expectations, and the inputs of the GPU generation tests are shown to be
non-vacuous (the penalty changes the codes within the compared frames, for every prompt)."""
import numpy as np
import pytest

import q3_oracle as qo
from penalty_ref import FRAMES, PENALTY, PROMPT_SEEDS, SEED, STREAM, WEIGHT_SEED, generate_with_penalty, penalise, prompt_ids, suppress


@pytest.fixture(scope="module")
def orc():
    cfg = qo.config_tiny()
    o = qo.Oracle(cfg, max_ctx=128, weights=qo.random_weights(cfg, WEIGHT_SEED))
    yield o
    o.close()


@pytest.mark.parametrize("params", [dict(temperature=1.0, top_p=1.0, top_k=1), dict(temperature=0.8, top_p=0.95, top_k=50)])
@pytest.mark.parametrize("ignore_eos", [True, False])
def test_checker_equals_oracle_with_penalty_off(orc, params, ignore_eos):
    """p = 1: the Python frame loop equals q3o_generate id for id, 3 prompts x 48 frames, greedy and sampled, EOS suppressed and not.
    The oracle side runs with cp_cached=False: the loop calls code_predictor the reference's way (whole sequence per sub-code), and
    that is the call pattern q3o_generate uses with cp_cached=False, so the comparison is exact by construction.  (The cached
    predictor computes the same rows in another order; it is also compared below and reported, not asserted bit for bit.)"""
    sp = qo.Sampling(max_new_tokens=FRAMES, repetition_penalty=1.0, **params)
    for ps in PROMPT_SEEDS[:3]:
        prompt = orc.build_prompt(prompt_ids(ps), 0)
        ref = orc.generate(prompt, sp, seed=SEED, stream=STREAM, cp_cached=False, ignore_eos=ignore_eos)
        prompt = orc.build_prompt(prompt_ids(ps), 0)
        got = generate_with_penalty(orc, prompt, sp, seed=SEED, stream=STREAM, ignore_eos=ignore_eos)
        assert got.shape == ref.shape and np.array_equal(got, ref), (ps, params, ignore_eos)
        if ignore_eos:
            assert got.shape[0] == FRAMES
        prompt = orc.build_prompt(prompt_ids(ps), 0)
        cached = orc.generate(prompt, sp, seed=SEED, stream=STREAM, cp_cached=True, ignore_eos=ignore_eos)
        same = cached.shape == ref.shape and np.array_equal(cached, ref)
        print("prompt seed %d %s ignore_eos=%d: %d frames, cached predictor %s" % (ps, params, ignore_eos, ref.shape[0], "equal" if same else "differs"))


def test_penalise_by_hand():
    x = np.array([2.0, -2.0, 0.0, 3.0, -np.inf, 1.0, -0.5, 7.0], np.float32)
    y = penalise(x, [0, 1, 2, 4, 0, 0, 1], 2.0)
    assert y.dtype == np.float32
    assert np.array_equal(y, np.array([1.0, -4.0, 0.0, 3.0, -np.inf, 1.0, -0.5, 7.0], np.float32))   # divided, multiplied, zero kept, duplicates once, -inf kept
    assert np.array_equal(x, np.array([2.0, -2.0, 0.0, 3.0, -np.inf, 1.0, -0.5, 7.0], np.float32))   # the input row is not touched
    assert np.array_equal(penalise(x, [0, 1, 3], 1.0), x) and np.array_equal(penalise(x, [0, 1, 3], 0.0), x)
    assert np.array_equal(penalise(x, [], 2.0), x)
    assert np.array_equal(penalise(x, [-1, 8, 100], 2.0), x)                                         # ids outside the row
    z = penalise(x, [3, 6], 0.8)                                                                     # p < 1 rewards
    assert z[3] == np.float32(3.0) / np.float32(0.8) and z[6] == np.float32(-0.5) * np.float32(0.8)
    # one correctly rounded fp32 operation, not a double-precision one rounded afterwards
    a = np.array([0.1, -0.1], np.float32)
    r = penalise(a, [0, 1], 1.05)
    assert r[0] == np.float32(0.1) / np.float32(1.05) and r[1] == np.float32(-0.1) * np.float32(1.05)
    cfg = qo.config_tiny()
    row = np.arange(cfg.vocab, dtype=np.float32)
    s = suppress(cfg, row, ignore_eos=False)
    assert np.isinf(s[cfg.suppress_begin:cfg.suppress_end]).sum() == cfg.suppress_end - cfg.suppress_begin - 1 and s[cfg.codec_eos] == row[cfg.codec_eos]
    assert np.isinf(suppress(cfg, row, ignore_eos=True)[cfg.suppress_begin:cfg.suppress_end]).all()


def test_gpu_generation_inputs_are_not_vacuous(orc):
    """The prompts, penalty and frame count of the GPU generation tests: for EVERY prompt the penalised checker's code0 column differs
    from the unpenalised oracle's within the compared frames (and no code0 id repeats more often with the penalty than without), so a
    kernel that ignores the penalty cannot pass them."""
    sp1 = qo.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=1.0, max_new_tokens=FRAMES)
    spp = qo.Sampling(temperature=1.0, top_p=1.0, top_k=1, repetition_penalty=PENALTY, max_new_tokens=FRAMES)
    for ps in PROMPT_SEEDS:
        plain = orc.generate(orc.build_prompt(prompt_ids(ps), 0), sp1, seed=SEED, stream=STREAM, cp_cached=False, ignore_eos=True)
        pen = generate_with_penalty(orc, orc.build_prompt(prompt_ids(ps), 0), spp, seed=SEED, stream=STREAM, ignore_eos=True)
        assert plain.shape == pen.shape == (FRAMES, orc.cfg.n_groups)
        diff = np.nonzero(plain[:, 0] != pen[:, 0])[0]
        print("prompt seed %d: first code0 change at frame %s, %d of %d code0 differ; distinct code0 %d -> %d"
              % (ps, diff[:1], diff.size, FRAMES, np.unique(plain[:, 0]).size, np.unique(pen[:, 0]).size))
        assert diff.size >= 1, ps
        assert np.unique(pen[:, 0]).size >= np.unique(plain[:, 0]).size, ps
