"""Checker of "continue from codes" (helper, not a test): the talker input row of a given frame as a numpy fp32 left-fold, the oracle
walked through a prompt and forced rows, the margin-aware verdict on free-running ids, and the inputs the tests share.  The weight
seed, prompts and penalty are those of tests/penalty_ref.py: unpenalised greedy decoding of the synthetic weights can hold one id
forever, so the free-running checks run with the penalty (and their prefixes hold distinct code0 ids: tests/test_continue_surface.py
confirms that on the CPU, with the oracle alone)."""
import numpy as np

from penalty_ref import PENALTY, PROMPT_SEEDS, SEED, STREAM, WEIGHT_SEED, generate_with_penalty, prompt_ids  # noqa: F401

NOISE = 2e-4            # bound asserted on |HIP logit - oracle logit| everywhere else (tests/test_gpu_full.py)
N_FRAMES = 48           # frames the checker generates
JOINS = (1, 7, 31)      # prefix lengths F0 of the self-continuation
PROMPT_SEED = PROMPT_SEEDS[0]
GREEDY = dict(temperature=1.0, top_p=1.0, top_k=1)
SAMPLED = dict(temperature=0.8, top_p=0.95, top_k=50)


def fold_rows(codec_embed, cp_embed, codes, frame0, trailing, pad):
    """rows of the frames `codes` [n][G]: fp32 left-fold in the order code0, sub0 .. sub(G-2), then the text row trailing[frame0 + i]
    (tts_pad once the index passes the rows) — reference tts_onnx.cpp:824-842.  codec_embed(ids) -> [n][H], cp_embed(id, step) -> [H]."""
    codes = np.asarray(codes, np.int64)
    out = []
    for i, fr in enumerate(codes):
        x = np.array(codec_embed([int(fr[0])])[0], np.float32, copy=True)
        for j in range(1, codes.shape[1]):
            x = (x + np.asarray(cp_embed(int(fr[j]), j - 1), np.float32)).astype(np.float32)
        f = frame0 + i
        x = (x + (np.asarray(trailing[f], np.float32) if f < len(trailing) else np.asarray(pad, np.float32))).astype(np.float32)
        out.append(x)
    return np.stack(out) if out else np.zeros((0, 0), np.float32)


def oracle_after_forced(orc, prompt, rows):
    """orc.prefill(prompt), then one orc.decode per forced row: (logits, last_hidden) behind the last row"""
    lg, lh = orc.prefill(prompt)
    lg = lg[-1]
    for r in rows:
        lg, lh = orc.decode(r)
    return np.array(lg, np.float32), np.array(lh, np.float32)


def verdict(codes, ref, mg, label, noise=NOISE):
    """the margin-aware acceptance of tests/test_gpu_repetition_penalty.py (_verdict): bit-exact up to the first differing decision,
    which must have a checker margin (on the PENALISED row for code0) under the logit noise; returns the number of bit-exact frames"""
    assert codes.shape == ref.shape, (label, codes.shape, ref.shape)
    bad = np.argwhere(codes != ref)
    if bad.size == 0:
        print("continue %s: %d frames bit-exact; smallest decision margin %.3g" % (label, ref.shape[0], float(mg.min()) if mg.size else float("nan")))
        return ref.shape[0]
    f, g = int(bad[0][0]), int(bad[0][1])
    print("continue %s: first divergence at frame %d group %d, checker margin %.3g (noise bound %.0e)" % (label, f, g, float(mg[f, g]), noise))
    assert float(mg[f, g]) < noise, "%s: ids differ at frame %d group %d although the checker's margin there is %g" % (label, f, g, float(mg[f, g]))
    assert np.array_equal(codes[:f], ref[:f]) and np.array_equal(codes[f, :g], ref[f, :g])
    return f


def checker(orc, ids, so, seed=SEED, stream=STREAM):
    """(codes, margins) of the penalised generation, EOS suppressed: tests/penalty_ref.py's frame loop over the oracle"""
    return generate_with_penalty(orc, orc.build_prompt(ids, 0), so, seed=seed, stream=stream, ignore_eos=True, margins=True)
