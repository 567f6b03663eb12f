"""Checker of the repetition penalty (helper, not a test): the penalty itself in numpy and the reference's frame loop restated in Python
over the oracle's step functions.  The oracle (oracle/) knows nothing of the penalty; numpy's float32 divide and multiply are the same
correctly rounded IEEE operations the kernel performs."""
import numpy as np

import q3_oracle as qo


def penalise(logits, history, p):
    """transformers' RepetitionPenaltyLogitsProcessor on one fp32 row: x > 0 ? x / p : x * p for every id in `history` (an id listed
    several times is penalised once; ids outside the row are ignored).  p == 1 and p == 0 mean off."""
    x = np.array(logits, dtype=np.float32, copy=True)
    p = np.float32(p)
    if p == np.float32(1.0) or p == np.float32(0.0):
        return x
    ids = np.unique(np.asarray(history, dtype=np.int64).reshape(-1))
    ids = ids[(ids >= 0) & (ids < x.size)]
    if ids.size == 0:
        return x
    v = x[ids]
    with np.errstate(invalid="ignore"):
        x[ids] = np.where(v > 0, v / p, v * p).astype(np.float32)
    return x


def suppress(cfg, logits, ignore_eos):
    """the special-token suppression of the code0 row (reference tts_onnx.cpp:803-807; ignore_eos suppresses EOS too)"""
    x = np.array(logits, dtype=np.float32, copy=True)
    keep = None if ignore_eos else x[cfg.codec_eos]
    x[cfg.suppress_begin:cfg.suppress_end] = -np.inf
    if keep is not None and cfg.suppress_begin <= cfg.codec_eos < cfg.suppress_end:
        x[cfg.codec_eos] = keep
    return x


def generate_with_penalty(orc, prompt, sp, seed=0, stream=0, ignore_eos=False, margins=False):
    """generate_codes + predict_subcodes (reference tts_onnx.cpp:782-872) over the oracle's prefill / decode / code_predictor /
    embedding calls, with the draws q3o_generate uses (rng_uniform(seed, stream, frame, group)) and the penalty of
    sp.repetition_penalty applied to the raw code0 row before the suppression.  The predictor is called the reference's way (the whole
    sequence again for every sub-code, uncached).  The trailing text rows are those of the oracle's last build_prompt call.
    Returns codes [F][n_groups]; with margins=True also the sampler decision margin (orc.sample_margin) of every decision, [F][n_groups],
    the code0 one taken on the penalised row."""
    cfg = orc.cfg
    G = cfg.n_groups
    rows, pad = orc.trailing()
    logits, lh = orc.prefill(prompt)
    last = logits[-1].copy()
    codes, mgs, history = [], [], []
    for step in range(sp.max_new_tokens):
        row = suppress(cfg, penalise(last, history, sp.repetition_penalty), ignore_eos)
        code0, m0 = orc.sample_margin(row, sp, qo.rng_uniform(seed, stream, step, 0))
        if code0 == cfg.codec_eos:
            break
        frame, mg = [code0], [m0]
        e0 = orc.codec_embed([code0])[0]
        seq = [lh, e0]
        for j in range(G - 1):
            sub = orc.code_predictor(np.stack(seq), j)
            sc, mj = orc.sample_margin(sub, sp, qo.rng_uniform(seed, stream, step, j + 1))
            frame.append(sc)
            mg.append(mj)
            seq.append(orc.cp_embed(sc, j))
        codes.append(frame)
        mgs.append(mg)
        history.append(code0)
        x = e0.copy()                                  # fp32, order code0, sub0 .. sub14, then the text row (:824-842)
        for j in range(G - 1):
            x += seq[j + 2]
        x += rows[step] if step < rows.shape[0] else pad
        last, lh = orc.decode(x)
    codes = np.array(codes, np.int64).reshape(-1, G)
    if margins:
        return codes, np.array(mgs, np.float32).reshape(-1, G)
    return codes


# ---- the inputs the free-running tests share (CPU: the penalty must move a code0 within FRAMES for every prompt; GPU: fused loop vs
# the checker on the same prompts) ----
WEIGHT_SEED = 0             # tiny_pair(seed=0) / random_weights(config_tiny(), 0)
PROMPT_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)   # the first three at b = 1, all eight as one batch
PENALTY = 1.5               # tiny random weights: top-2 gaps of a few 1e-3..1e-2 on logits of ~0.1, so 1.5 dwarfs them
FRAMES = 48
STREAM = 2
SEED = 5


def prompt_ids(prompt_seed):
    from util import frame_tokens
    return frame_tokens(np.random.default_rng(prompt_seed).integers(0, 1000, 16))
