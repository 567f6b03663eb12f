"""What tests/test_gpu_sched_pool.py needs from its inputs, checked on the CPU with the oracle alone (no GPU): in every input set of
tests/sched_pool_ref.py the oracle's own free-running generation ends by EOS at three or more different lengths and at least one
utterance reaches its cap — so lengths are unknown to the scheduler, slots free up at different looks and the pool's pages scatter —
and at most 6 % of the decisions on the oracle's trajectory have a margin below NOISE, so the GPU tests' cap of one excused decision
in eight (the walk there follows the GPU's trajectory) leaves room for nothing but noise.

Measured (weights seed 31, prompt seed 4; the sampling seeds of sched_pool_ref.JOB_SEEDS were picked among 1..16 for sets that
offer the above and whose utterances are long enough to make a small pool preempt); every line is printed again by the test:
  prefixed          seed 13: new frames 85, 112, 60, 7, 150, 125                    399 of  8 628 decisions under NOISE = 4.6 %
  continued         seed  9: new frames 120, 23, 112, 39, 20 (behind 1 .. 100)      260 of  5 028 = 5.2 %
  ragged_instruct   seed 15: new frames 150, 150, 130, 19, 150, 20                  462 of  9 907 = 4.7 %
  ragged_continued  seed  2: new frames 75, 89, 66, 76, 37, 120                     368 of  7 413 = 5.0 %
  wide32            seed 13: 32 utterances, 2 .. 40 frames, 19 at their caps        588 of 12 685 = 4.6 %
The asserts below are the properties, not these figures."""
import numpy as np
import pytest

import q3_oracle as qo
import sched_pool_ref as R


@pytest.fixture(scope="module")
def orc():
    ocfg = qo.config_tiny()
    o = qo.Oracle(ocfg, max_ctx=R.MAX_CTX, weights=qo.random_weights(ocfg, R.WEIGHT_SEED))
    yield o
    o.close()


@pytest.mark.parametrize("name", ["prefixed", "continued", "ragged_instruct", "ragged_continued", "wide32"])
def test_input_set_ends_at_many_lengths_and_keeps_its_margins(orc, name):
    job = R.jobs()[name]
    new, low, total = [], 0, 0
    for u in range(job.n):
        codes, mg, F0 = R.oracle_run(orc, job, u)
        assert codes.shape[0] - F0 <= job.caps[u] and mg.size > 0
        if F0 > 1:   # a re-admitted utterance's code0 history must be its prefix: the check is vacuous on a prefix of one id
            assert len(set(codes[:F0, 0].tolist())) >= 2, (name, u)
        new.append(codes.shape[0] - F0)
        low += int((mg < R.NOISE).sum())
        total += int(mg.size)
    eos_lengths = sorted({n for n, c in zip(new, job.caps) if n < c})
    capped = [u for u, (n, c) in enumerate(zip(new, job.caps)) if n == c]
    share = low / total
    print("%s: new frames %s (caps %s): %d EOS lengths, %d at the cap; decisions under NOISE %d of %d = %.1f %%" % (
        name, new, [int(c) for c in job.caps], len(eos_lengths), len(capped), low, total, 100.0 * share))
    assert min(new) >= 1, (name, new)                       # every utterance has audio of its own
    assert len(eos_lengths) >= 3, (name, new)
    assert len(capped) >= 1, (name, new)
    assert share <= R.SURFACE_SHARE, (name, low, total)


def test_replay_follows_its_own_generation(orc):
    """the walk judges the oracle's own codes as all equal (nothing excused), names a planted wrong id, and holds the end decision"""
    job = R.jobs()["continued"]
    u = 1
    p, tr, pad = job.oracle_prompt(orc, u)
    codes, mg, F0 = R.oracle_run(orc, job, u)
    sp = R.osampling(job.caps[u], job.penalty)
    n, excused = R.replay_verdict(orc, p, tr, pad, codes, sp, job.seed, u, forced=F0, penalty=job.penalty)
    G = orc.cfg.n_groups
    ended = codes.shape[0] - F0 < job.caps[u]
    assert excused == 0 and n == (codes.shape[0] - F0) * G + int(ended) == mg.size
    ids, mgs = R.replay(orc, p, tr, pad, codes, sp, job.seed, u, forced=F0, penalty=job.penalty)
    assert np.array_equal(ids[F0:codes.shape[0]], codes[F0:]) and (ids[:F0] == -1).all()
    f, g = [(f, g) for f in range(F0, codes.shape[0]) for g in range(G) if mgs[f, g] > 10 * R.NOISE][3]
    bad = codes.copy()
    bad[f, g] = (bad[f, g] + 1) % 64
    with pytest.raises(AssertionError, match="frame %d group %d" % (f, g)):
        R.replay_verdict(orc, p, tr, pad, bad, sp, job.seed, u, forced=F0, penalty=job.penalty)
    if ended:   # cut short: the oracle does not decide EOS behind the frame in front of the last
        with pytest.raises(AssertionError, match="the end"):
            k = next(k for k in range(codes.shape[0] - 1, F0, -1) if mgs[k, 0] > R.NOISE)
            R.replay_verdict(orc, p, tr, pad, codes[:k], sp, job.seed, u, forced=F0, penalty=job.penalty)
    # the penalty matters on this trajectory: the walk without it disagrees somewhere above the noise
    with pytest.raises(AssertionError, match="frame"):
        R.replay_verdict(orc, p, tr, pad, codes, sp, job.seed, u, forced=F0, penalty=1.0)
    assert R.same_up_to_noise(codes, codes, ids, mgs) == codes.shape[0]
    with pytest.raises(AssertionError, match="part at frame %d group %d" % (f, g)):
        R.same_up_to_noise(codes, bad, ids, mgs)
