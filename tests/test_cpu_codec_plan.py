"""The vocoder's host arithmetic (leaxer-qwen3-tts_amd/csrc/q3_codec_plan.h: the decoder length formula, the look-back of the stages
behind the pre-transformer, the cut of a push's own samples out of its window's, the batched push's grouping, the arenas' byte counts
and the staging of host codes) without a GPU: a g++ harness (tests/cpp/codec_plan_harness.cpp), built with the address and
undefined-behaviour sanitizers, executes commands against the header the engine uses, and tests/codec_plan_ref.py restates the
arithmetic as the decode paths spelled it in place.  The reference decodes whole utterances (run_vocoder, src/tts_onnx.cpp:759-776)
and has no counterpart."""
import os
import random
import subprocess

import pytest

import codec_plan_ref as ref
import q3_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"tiny": qo.config_tiny, "medium": qo.config_medium, "0.6b": qo.config_06b, "1.7b": qo.config_17b}
# Engine::codec_stage_b_context() of the build before the arithmetic moved into the header, per config
STAGE_B_CONTEXT = {"tiny": 12, "medium": 12, "0.6b": 12, "1.7b": 12}
OUT_OF_RANGE = "err codec_decode: code out of range"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("codec_plan") / "codec_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "codec_plan_harness.cpp"), "-o", exe], check=True)

    def run(*script):
        r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report fails the run
        out = r.stdout.splitlines()
        assert len(out) == len(script)
        return out
    return run


def ask(harness, d, *script):
    out = harness(ref.cfg_command(d), *script)
    assert out[0] == "ok"
    return out[1:]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_stage_b_context_and_lengths(harness, name):
    d = ref.dims(CONFIGS[name]())
    frames = list(range(-1, 41)) + [2048]
    out = ask(harness, d, "ctx", "up", *["len %d" % F for F in frames])
    assert int(out[0]) == STAGE_B_CONTEXT[name] == ref.stage_b_context(d)
    assert out[1] == "%d %d" % (ref.up_front(d), ref.samples_per_frame(d))
    for F, got in zip(frames, out[2:]):
        assert got == "%d %d" % (ref.decode_len(d, F), ref.len_of(d, F)), F


@pytest.mark.parametrize("name", ["tiny", "0.6b"])
def test_window_cut_of_every_short_push(harness, name):
    d = ref.dims(CONFIGS[name]())
    ctxB = ref.stage_b_context(d)
    cases = [(a0, n) for a0 in range(3 * ctxB + 1) for n in range(1, 6)]
    script = []
    for a0, n in cases:                                              # the window [a0 - ctx, a0 + n) decodes to len(ctx + n) samples
        ctx = min(a0, ctxB)
        script.append("cut %d %d %d %d 1" % (a0, n, ctx, ref.decode_len(d, ctx + n)))
    for (a0, n), got in zip(cases, ask(harness, d, *script)):
        first, n_own, ok = (int(x) for x in got.split())
        ctx = min(a0, ctxB)
        assert (first, n_own) == ref.window_cut(d, a0, n, ctx), (a0, n)
        assert first >= 0 and first + n_own == ref.decode_len(d, ctx + n) and ok == 1, (a0, n, got)
    # consecutive pushes own, between them, exactly the samples of the frames pushed so far
    rng = random.Random(5)
    for _ in range(20):
        pushes = [rng.randint(1, 5) for _ in range(rng.randint(1, 12))]
        at, script = 0, []
        for n in pushes:
            ctx = min(at, ctxB)
            script.append("cut %d %d %d %d 1" % (at, n, ctx, ref.decode_len(d, ctx + n)))
            at += n
        assert sum(int(g.split()[1]) for g in ask(harness, d, *script)) == ref.decode_len(d, at), pushes
    # the consistency condition: a window of another length is refused; a padded group's shorter sequence only has to hold its samples
    n_win = ref.decode_len(d, ctxB + 2)
    out = ask(harness, d, "cut 40 2 %d %d 1" % (ctxB, n_win + 1), "cut 40 2 %d %d 0" % (ctxB, n_win + 1), "cut 40 2 %d %d 0" % (ctxB, n_win - 1),
              "cut 40 2 %d %d 1" % (ctxB + 1, n_win), "cut 3 2 0 %d 0" % (100 * n_win))
    assert [o.split()[2] for o in out] == ["0", "1", "0", "0", "0"]      # the last: history but no context, first < 0
    assert int(out[4].split()[0]) < 0


def test_groups_against_the_restatement(harness):
    d = ref.dims(qo.config_tiny())
    ctxB = ref.stage_b_context(d)
    rng = random.Random(11)
    lists = []
    for _ in range(200):
        g = rng.randint(1, 12)
        lists.append([(rng.choice((0, 0, 1, 5, ctxB - 1, ctxB, ctxB + 1, 40, 300)), rng.randint(1, 30)) for _ in range(g)])
    out = ask(harness, d, *[ref.groups_command(s, ctxB) for s in lists])
    for s, got in zip(lists, out):
        assert got == ref.groups_answer(s, ctxB), s
    assert sum(" g" in o and len(o.split(" g ")[1].split()) > 1 for o in out) >= 40          # several left contexts in one call are exercised
    # mature streams first, ties in call order; young streams of one age share a group
    got = ask(harness, d, ref.groups_command([(5, 2), (40, 3), (5, 4), (12, 1), (0, 2)], ctxB))[0]
    assert got == "o 1 3 0 2 4 g 0,2,%d 2,4,9 4,5,2" % (ctxB + 3)
    # 40 mature streams with windows of 101 rows: 36 x 101 x 4.7e6 < 2^34 < 37 x 101 x 4.7e6, so the 16 GiB rule cuts behind the 36th
    assert 36 * 101 * 4700000 < 2 ** 34 < 37 * 101 * 4700000
    got = ask(harness, d, ref.groups_command([(500, 101 - ctxB)] * 40, ctxB))[0]
    assert got.split(" g ")[1] == "0,36,101 36,40,101"
    assert got == ref.groups_answer([(500, 101 - ctxB)] * 40, ctxB)


@pytest.mark.parametrize("name", ["tiny", "0.6b"])
def test_arena_bytes(harness, name):
    d = ref.dims(CONFIGS[name]())
    rng = random.Random(3)
    script, want = [], []
    for _ in range(40):
        n, Fp, T, back = rng.randint(1, 9), rng.randint(1, 70), rng.randint(1, 200), rng.randint(1, 400)
        P = 1 << (Fp - 1).bit_length()
        up = rng.randint(0, 1)
        script += ["bytes batch %d %d %d %d" % (n, Fp, P, up), "bytes stream %d" % T, "bytes push %d %d" % (T, back), "bytes prime %d %d %d" % (n, Fp, P)]
        want += [ref.batch_arena_bytes(d, n, Fp, P, up), ref.pre_bytes(d, T), ref.sbatch_push_bytes(d, T, back), ref.sbatch_prime_bytes(d, n, Fp, P)]
    assert [int(o) for o in ask(harness, d, *script)] == want
    # the bump allocator: 256-byte steps, nothing handed out while planning
    assert ask(harness, d, "bump 1 64 65 0 1000")[0] == "0 256 512 1024 1024 5120"


def test_code_staging(harness):
    d = ref.dims(qo.config_tiny())
    K = d["cd_codebook"]
    out = ask(harness, d, "codes 3 0 %d 5" % (K - 1), "codes 3 0 -1 5", "codes 3 0 5 %d" % K, "codes 2 %d -1" % (2 ** 40), "codes 0",
              "codes 4 1 2 %d %d" % (-2 ** 33, K))
    assert out == ["ok 0 %d 5" % (K - 1), OUT_OF_RANGE, OUT_OF_RANGE, OUT_OF_RANGE, "ok", OUT_OF_RANGE]
