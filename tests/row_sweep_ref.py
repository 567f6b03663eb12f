"""CPU side of tests/test_gpu_row_sweep.py: the shrunk full-width configs, the utterances, and the per-utterance oracle reference.

A batch must not change an utterance's result, so the reference of utterance u does not depend on how many rows run beside it: it is
computed once (free-running greedy codes with their decision margins, then a teacher-forced pass for the talker's logits and hidden
row in front of every frame) and reused at every row count.  Nothing here touches the GPU."""
import numpy as np

import q3_oracle as qo
from util import frame_tokens

FRAMES = 4          # frames 0..3 are generated; the teacher-forced pass also holds what stands in front of frame 4
SEED = 77
NOISE = 2e-4        # the project's fp32-cache logit bound (tests/test_gpu_b64.py, logit_bound / margin_noise)


def sweep_config(base):
    """`base` (config_06b / config_17b) with two talker and two predictor layers, a 64-wide text table, the tiny codec decoder and no
    speaker encoder: every talker / predictor width, vocab, sub_vocab and text_vocab as shipped.  Two layers are the fewest that run
    every launch variant of a layer pass (layer 0 with a down-projection seam, a last layer that takes ssq_in and keeps the finish)."""
    d = base.to_dict()
    tiny = qo.config_tiny().to_dict()
    d.update({k: v for k, v in tiny.items() if k.startswith("cd_")})
    d.update(n_layers=2, cp_layers=2, text_hidden=64, spk_enc_dim=0)
    return qo.Config.from_dict(d)


def utterances(n, prompt_seed):
    rng = np.random.default_rng(prompt_seed)
    return [frame_tokens(rng.integers(0, 151643, int(k))) for k in rng.integers(3, 20, n)]


def cap(nb):
    """rows of an nb-row batch whose first divergence from the oracle may be excused by a sub-noise decision margin"""
    return max(1, nb // 16)


def greedy():
    return qo.Sampling(temperature=1.0, top_p=1.0, top_k=1, max_new_tokens=FRAMES)


def teacher_forced(orc, prompt, trailing, pad, codes):
    """prefill + decode of each frame's embedding sum (reference generate_codes: the frame's 16 code embeddings plus the trailing text
    row of that frame, the pad row once the text is used up): logits [F + 1][vocab] and hidden [F + 1][hidden], row f what stands in
    front of frame f"""
    G = orc.cfg.n_groups
    lo, ho = orc.prefill(prompt)
    lg, lh = [lo[-1].copy()], [ho.copy()]
    for f in range(codes.shape[0]):
        x = orc.codec_embed([int(codes[f, 0])])[0].copy()
        for j in range(G - 1):
            x = x + orc.cp_embed(int(codes[f, j + 1]), j)
        x = x + (trailing[f] if f < len(trailing) else pad)
        lo, ho = orc.decode(x)
        lg.append(lo.copy())
        lh.append(ho.copy())
    return np.stack(lg), np.stack(lh)


class Reference:
    """codes[u] [FRAMES][G], margins[u] [FRAMES][2 + G], logits[u] [FRAMES + 1][vocab], hidden[u] [FRAMES + 1][hidden];
    close: the utterances with a decision margin below NOISE somewhere in frames 0..FRAMES-1 (the only ones a row may be excused on)"""

    def __init__(self, orc, toks):
        self.orc, self.toks = orc, toks
        self.prompt, self.trailing, self.pad = [], [], None
        self.codes, self.margins, self.logits, self.hidden = [], [], [], []
        for u, t in enumerate(toks):
            po = orc.build_prompt(t, 0)
            tro, pad = orc.trailing()
            codes, mg = orc.generate_margins(po, greedy(), seed=SEED, stream=u, cp_cached=True, ignore_eos=True)
            assert codes.shape == (FRAMES, orc.cfg.n_groups)
            lg, lh = teacher_forced(orc, po, tro, pad, codes)
            self.prompt.append(po); self.trailing.append(tro.copy()); self.pad = pad.copy()
            self.codes.append(codes); self.margins.append(mg); self.logits.append(lg); self.hidden.append(lh)
        self.close = {u for u, mg in enumerate(self.margins) if float(mg[:, 2:].min()) < NOISE}
        self.close_01 = {u for u, mg in enumerate(self.margins) if float(mg[:2, 2:].min()) < NOISE}

    def assert_caps(self, row_counts):
        """on the reference alone: at no row count of the sweep can more rows ask for an excuse than its cap grants"""
        for nb in row_counts:
            n = sum(1 for u in self.close if u < nb)
            assert n <= cap(nb), "%d of the first %d utterances hold a sub-noise margin, the cap is %d: %s" % (n, nb, cap(nb), sorted(self.close))

    def forced(self, u, codes):
        """the teacher-forced pass of utterance u over the ENGINE's codes (a row past an excused divergence)"""
        return teacher_forced(self.orc, self.prompt[u], self.trailing[u], self.pad, codes)

    def predictor_logits(self, hidden_row, frame_codes):
        """predict_subcodes in the reference's uncached pattern (the growing sequence re-run per sub-code) over the given codes of one
        frame: [G - 1][sub_vocab], row j the logits behind sub-code j + 1"""
        orc = self.orc
        seq = [hidden_row, orc.codec_embed([int(frame_codes[0])])[0]]
        out = []
        for j in range(orc.cfg.n_groups - 1):
            out.append(orc.code_predictor(np.stack(seq), j))
            seq.append(orc.cp_embed(int(frame_codes[j + 1]), j))
        return np.stack(out)
