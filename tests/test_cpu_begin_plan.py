"""The host rules every way of beginning utterances in slots shares (leaxer-qwen3-tts_amd/csrc/q3_begin_plan.h: slots_begin,
slots_begin_prefixed, slots_begin_ragged and talker_prefill_dev's groups) without a GPU: a g++ harness (tests/cpp/begin_plan_harness.cpp),
built with the address and undefined-behaviour sanitizers, executes commands against the header the engine uses, and
tests/begin_plan_ref.py restates the rules entry by entry.  The reference begins one utterance at a time (run_prefill,
src/tts_onnx.cpp:615-665) and has no counterpart; what is checked is every refusal's text, which of two faults a call reports, the
arithmetic of a member's pages, frames and position, and which members share a pass."""
import os
import random
import subprocess

import pytest

import begin_plan_ref as ref
from begin_plan_ref import PLAIN, PREFIXED, RAGGED, member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (PLAIN, PREFIXED, RAGGED)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("begin_plan") / "begin_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "begin_plan_harness.cpp"), "-o", exe], check=True)

    def run(*script):
        r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report fails the run
        out = r.stdout.splitlines()
        assert len(out) == len(script)
        return out
    return run


def plans(harness, L, calls):
    """[(entry, members, max_new)] -> the harness's answers, each also compared with the restatement"""
    out = harness(ref.limits_command(L), *[ref.command(e, ms, mn) for e, ms, mn in calls])[1:]
    for (e, ms, mn), got in zip(calls, out):
        assert got == ref.plan(e, ms, mn, L), (e, mn, ms)
    return out


def groups_of(line):
    return [tuple(int(x) for x in g.split(",")) for g in line.split(" g ")[1].split()] if " g " in line else []


def test_every_refusal_text_of_every_entry(harness):
    L = ref.limits()                                                 # B 8, max_ctx 256, max_trailing 32, frame capacity 200
    ok = member(0, 8)
    shared = [   # (member, text), the same under every entry
        (member(8, 8), "slot out of range"),
        (member(-1, 8), "slot out of range"),
        (member(0, 8, n_trailing=33), "too many trailing text rows"),
        (member(0, 8, n_trailing=-1), "too many trailing text rows"),
        (member(0, 0), "prefill length must be 1..max_ctx rows"),
        (member(0, 257), "prefill length must be 1..max_ctx rows"),
        (member(0, 8, n_prefix=-1), "prefix codes: n_prefix must be >= 0 (and the codes given)"),
        (member(0, 8, n_prefix=3, codes=False), "prefix codes: n_prefix must be >= 0 (and the codes given)"),
    ]
    calls, want = [], []
    for e in ENTRIES:
        for q, text in shared:
            calls.append((e, [q] if e == PLAIN else [ok, dict(q, slot=q["slot"] if q["slot"] != 0 else 1)], 8))
            want.append("err " + text)
    # the context limit: plain's two texts, the other entries' one
    calls += [(PLAIN, [member(0, 200)], 57), (PLAIN, [member(0, 8)], 0), (PLAIN, [member(0, 100, n_prefix=100)], 57)]
    want += ["err prompt + max_new_tokens exceeds max_ctx"] * 2 + ["err prompt + prefix frames + max_new_tokens exceeds max_ctx"]
    for e in (PREFIXED, RAGGED):
        calls += [(e, [ok, member(1, 100, P=100)], 57), (e, [ok, member(1, 8)], 0), (e, [ok, member(1, 100, n_prefix=100)], 57)]
        want += ["err prefix + prompt + prefix frames + max_new_tokens exceeds max_ctx"] * 3
    # forced frames: the capacity, bad ids (the engine's own check, through the callable), and plain's "on its own"
    for e in ENTRIES:
        lead = [] if e == PLAIN else [ok]
        calls += [(e, lead + [member(1, 8, n_prefix=150)], 51), (e, lead + [member(1, 8, n_prefix=5, bad_codes=True)], 8)]
        want += ["err prefix frames + max_new_tokens exceeds the slot's frame capacity", "err " + ref.BAD_CODES]
    calls.append((PLAIN, [ok, member(1, 8, n_prefix=5)], 8))
    want.append("err slots_begin: a slot with prefix codes is begun on its own")
    # the pointers: plain does not look, the others under their own names; ragged alone for the trailing rows
    calls += [(PLAIN, [member(0, 8, prompt=False, n_trailing=2, trailing=False)], 8),
              (PREFIXED, [ok, member(1, 8, prompt=False)], 8), (RAGGED, [ok, member(1, 8, prompt=False)], 8),
              (PREFIXED, [ok, member(1, 8, n_trailing=2, trailing=False)], 8), (RAGGED, [ok, member(1, 8, n_trailing=2, trailing=False)], 8),
              (RAGGED, [ok, member(1, 8, n_trailing=0, trailing=False)], 8)]
    want += [None, "err slots_begin_prefixed: null prompt", "err slots_begin_ragged: null prompt", None,
             "err slots_begin_ragged: trailing rows announced but not given", None]
    # an unknown prefix id (the engine's own refusal, through the callable): plain never resolves one
    calls += [(PLAIN, [member(0, 8, bad_prefix=True)], 8), (PREFIXED, [ok, member(1, 8, bad_prefix=True)], 8), (RAGGED, [ok, member(1, 8, bad_prefix=True)], 8)]
    want += [None, "err " + ref.BAD_PREFIX, "err " + ref.BAD_PREFIX]
    # a slot listed twice, under each entry's name
    calls += [(PLAIN, [member(2, 8), member(2, 8)], 8), (PREFIXED, [member(2, 8), member(2, 20)], 8), (RAGGED, [member(2, 8), member(2, 20)], 8)]
    want += ["err slots_begin: slot listed twice", "err slots_begin_prefixed: slot listed twice", "err slots_begin_ragged: slot listed twice"]
    out = plans(harness, L, calls)
    for got, w, call in zip(out, want, calls):
        assert got == w if w is not None else got.startswith("ok m "), (call, got)


def test_of_two_faults_the_one_reached_first_is_reported(harness):
    L = ref.limits()
    ok = member(0, 8)
    calls = [
        # a bad S in member 1 against a doubled slot in member 2: members are checked in call order
        (PREFIXED, [ok, member(1, 0), member(0, 8)], 8), (RAGGED, [ok, member(1, 0), member(0, 8)], 8), (PLAIN, [ok, member(1, 0), member(0, 8)], 8),
        # bad codes in member 0 against a doubled slot in member 1
        (PREFIXED, [member(0, 8, n_prefix=4, bad_codes=True), ok], 8), (RAGGED, [member(0, 8, n_prefix=4, bad_codes=True), ok], 8),
        # ... and inside one member the codes are looked at before the slots
        (PREFIXED, [ok, member(0, 8, n_prefix=4, bad_codes=True)], 8), (RAGGED, [ok, member(0, 8, n_prefix=4, bad_codes=True)], 8),
        # plain looks for a doubled slot only inside a group, after every member check: a later member's fault wins
        (PLAIN, [member(2, 8), member(2, 8), member(9, 8)], 8),
        # plain: doubled inside one group is refused, in two groups (the length changes in between) accepted
        (PLAIN, [member(2, 8), member(3, 8), member(2, 8)], 8), (PLAIN, [member(2, 8), member(3, 9), member(2, 8)], 8),
        # the other entries look over the whole call
        (PREFIXED, [member(2, 8), member(3, 9), member(2, 8)], 8), (RAGGED, [member(2, 8), member(3, 9), member(2, 8)], 8),
        # plain: the context limit before the forced-frames arguments; the others the other way round
        (PLAIN, [member(0, 250, n_prefix=-1)], 8), (PREFIXED, [ok, member(1, 250, n_prefix=-1)], 8),
        # null prompt before an unknown prefix id, the id before the forced-frames arguments
        (PREFIXED, [ok, member(1, 8, prompt=False, bad_prefix=True)], 8), (RAGGED, [ok, member(1, 8, bad_prefix=True, n_prefix=-1)], 8),
        # plain: "on its own" before the codes are looked at, the capacity before "on its own"
        (PLAIN, [ok, member(1, 8, n_prefix=4, bad_codes=True)], 8), (PLAIN, [ok, member(1, 8, n_prefix=195)], 8),
    ]
    want = ["err prefill length must be 1..max_ctx rows"] * 3 + ["err " + ref.BAD_CODES] * 4 + ["err slot out of range",
            "err slots_begin: slot listed twice", "ok", "err slots_begin_prefixed: slot listed twice", "err slots_begin_ragged: slot listed twice",
            "err prompt + max_new_tokens exceeds max_ctx", "err prefix codes: n_prefix must be >= 0 (and the codes given)",
            "err slots_begin_prefixed: null prompt", "err " + ref.BAD_PREFIX,
            "err slots_begin: a slot with prefix codes is begun on its own", "err prefix frames + max_new_tokens exceeds the slot's frame capacity"]
    out = plans(harness, L, calls)
    assert len(want) == len(calls)
    for got, w, call in zip(out, want, calls):
        assert got == w if w != "ok" else got.startswith("ok m "), (call, got)
    assert groups_of(out[9]) == [(0, 1, 0, 1), (1, 1, 0, 1), (2, 1, 0, 1)]


def test_pages_frames_and_position_of_a_member(harness):
    L = ref.limits()
    mn = 50                                                           # max_new_tokens
    rows = []   # (entry, member, (tokens, cap, armed max_frames, position))
    for e, P, F0 in ((PLAIN, 0, 0), (PREFIXED, 40, 0), (PREFIXED, 40, 7), (RAGGED, 65, 3), (PLAIN, 0, 5)):
        own = P + 10 + F0
        for max_frames, cap in ((0, 50), (20, 20), (80, 50)):         # none, below max_new, above it
            for kv, tokens in ((0, own + cap), (own - 3, own), (own + 4, own + 4), (own + cap + 9, own + cap)):   # none, below own, between, above own + cap
                rows.append((e, member(1, 10, n_prefix=F0, max_frames=max_frames, kv_tokens=kv, P=P), (tokens, cap, F0 + cap, own)))
    ok = member(0, 8)
    calls = [(e, [q] if e == PLAIN else [ok, q], mn) for e, q, _ in rows]
    out = plans(harness, L, calls)
    for (e, q, want), got in zip(rows, out):
        assert got.startswith("ok m "), got
        nums = [tuple(int(x) for x in w.split(",")) for w in got.split()[2:(3 if e == PLAIN else 4)]]
        assert nums[-1] == want, (e, q, got)


def test_groups(harness):
    def run(L, e, ms):
        return groups_of(plans(harness, L, [(e, ms, 8)])[0])

    def eq(S, n, slot0=0):
        return [member((slot0 + i) % 200, S) for i in range(n)]
    big = dict(B=200)
    L128, L64, L16 = ref.limits(rows_max=128, **big), ref.limits(rows_max=64, **big), ref.limits(rows_max=16, **big)
    # plain: the cap follows rows_max; prefixed: always the 128-row long workspace
    assert run(L128, PLAIN, eq(8, 17)) == [(0, 16, 1, 1), (16, 1, 0, 1)]        # cap 16: the 17th opens a new group
    assert run(L64, PLAIN, eq(8, 17)) == [(0, 8, 1, 1), (8, 8, 1, 1), (16, 1, 0, 1)]
    assert run(L16, PLAIN, eq(8, 5)) == [(0, 2, 1, 1), (2, 2, 1, 1), (4, 1, 0, 1)]
    assert run(L16, PREFIXED, eq(8, 17)) == [(0, 16, 1, 1), (16, 1, 0, 1)]
    # S = 1: 128 members of one row; S = 3: two members are 6 rows, below mfma_min_rows = 12, one at a time; four are 12
    assert run(L128, PLAIN, eq(1, 130)) == [(0, 128, 1, 1), (128, 2, 0, 1)]
    assert run(L64, PLAIN, eq(1, 65)) == [(0, 64, 1, 1), (64, 1, 0, 1)]
    assert run(L128, PREFIXED, eq(1, 130)) == [(0, 128, 1, 1), (128, 2, 0, 1)]
    for e in (PLAIN, PREFIXED):
        assert run(L128, e, eq(3, 2)) == [(0, 2, 0, 1)]
        assert run(L128, e, eq(3, 3)) == [(0, 3, 0, 1)]
        assert run(L128, e, eq(3, 4)) == [(0, 4, 1, 1)]
        assert run(L128, e, eq(16, 9)) == [(0, 8, 1, 1), (8, 1, 0, 1)]            # S = 16: 8 members fill 128 rows
        assert run(L128, e, eq(17, 3)) == [(0, 1, 0, 1), (1, 1, 0, 1), (2, 1, 0, 1)]   # S = 17: the chunk path, each on its own
        # a length change in mid-run closes the group
        assert run(L128, e, eq(8, 3) + eq(9, 2, 3) + eq(8, 1, 5)) == [(0, 3, 1, 1), (3, 2, 1, 1), (5, 1, 0, 1)]
        # dims off the MFMA condition: all one at a time
        assert run(ref.limits(mfma_dims=False, **big), e, eq(8, 4)) == [(i, 1, 0, 1) for i in range(4)]
        # consecutive against scattered slot ids
        assert run(L128, e, [member(s, 8) for s in (5, 6, 7)]) == [(0, 3, 1, 1)]
        assert run(L128, e, [member(s, 8) for s in (5, 0, 3)]) == [(0, 3, 1, 0)]
        assert run(L128, e, [member(s, 8) for s in (5, 6, 8)]) == [(0, 3, 1, 0)]
    assert run(L16, PLAIN, eq(16, 2)) == [(0, 1, 0, 1), (1, 1, 0, 1)]
    # a forced member in a prefixed run is never batched and splits the run around it
    forced = [member(0, 8, P=40), member(1, 8, P=40), member(2, 8, n_prefix=7, P=40), member(3, 8), member(4, 8, P=65)]
    assert run(L128, PREFIXED, forced) == [(0, 2, 1, 1), (2, 1, 0, 1), (3, 2, 1, 1)]
    assert run(L128, PREFIXED, forced[2:]) == [(0, 1, 0, 1), (1, 2, 1, 1)]
    # plain hands a lone forced member to the forced begin
    assert plans(harness, L128, [(PLAIN, [member(0, 8, n_prefix=7)], 8)])[0].endswith(" forced")


def test_ragged_one_at_a_time_decision(harness):
    L = ref.limits()
    rows = [(12, 1, 0), (11, 1, 0), (500, 0, 0), (500, 1, 1), (500, 1, 0)]
    out = harness(ref.limits_command(L), *["ragged %d %d %d" % r for r in rows])[1:]
    assert out == ["one_at_a_time %d" % v for v in (0, 1, 1, 1, 0)]
    assert [ref.one_at_a_time(t, L, s, m) for t, s, m in rows] == [0, 1, 1, 1, 0]
    off = ref.limits(mfma_dims=False)
    assert harness(ref.limits_command(off), "ragged 500 1 0")[1] == "one_at_a_time 1" and ref.one_at_a_time(500, off, 1, 0) == 1
    # the rows it counts: prompts and forced frames, not the prefixes
    got = plans(harness, L, [(RAGGED, [member(0, 30, P=65), member(1, 8, n_prefix=7), member(2, 1)], 8)])[0]
    assert got.endswith(" rows 46")


@pytest.mark.parametrize("entry", ENTRIES)
def test_random_member_lists_against_the_restatement(harness, entry):
    rng = random.Random(1000 + entry)
    per_limits = {}
    for _ in range(200):
        L = ref.limits(B=rng.choice((4, 8, 40)), max_ctx=rng.choice((64, 256)), max_trailing=8, max_frames_cap=rng.choice((40, 200)),
                       rows_max=rng.choice((16, 64, 128)), mfma_dims=rng.random() < 0.85)
        n = rng.choice((1, 1, 2, 3, 4, 6, 20))
        base_S = rng.choice((1, 3, 8, 16, 17))
        ms = []
        for i in range(n):
            wild = rng.random() < 0.06                                # now and then a member that is refused
            ms.append(member(
                slot=rng.randrange(-1, L["B"] + 1) if wild else (i if rng.random() < 0.5 else rng.randrange(L["B"])),
                S=rng.choice((0, 300)) if wild and rng.random() < 0.5 else (base_S if rng.random() < 0.8 else rng.choice((1, 3, 8, 9, 16, 17, 30))),
                n_trailing=rng.choice((0, 1, 8, 9 if wild else 2)),
                n_prefix=rng.choice((0, 0, 0, 5, 31, -1 if wild else 0)),
                max_frames=rng.choice((0, 3, 100)), kv_tokens=rng.choice((0, 1, 40, 70, 1000)), P=rng.choice((0, 0, 40, 65)),
                prompt=rng.random() < 0.97, trailing=rng.random() < 0.9, codes=rng.random() < 0.95, bad_codes=rng.random() < 0.05,
                bad_prefix=rng.random() < 0.03))
        per_limits.setdefault(ref.limits_command(L), (L, []))[1].append((entry, ms, rng.choice((0, 8, 8, 8, 30, 60))))
    answers = []
    for L, calls in per_limits.values():
        answers += plans(harness, L, calls)
    assert len(answers) == 200
    assert sum(a.startswith("ok") for a in answers) >= 40 and sum(a.startswith("err") for a in answers) >= 40   # both sides are exercised
