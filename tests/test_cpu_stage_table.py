"""Host bookkeeping of the carried-state stages behind the vocoder (leaxer-qwen3-tts_amd/csrc/q3_stage.h: the stretcher, the level stage
and the PCM sink share it) without a GPU: a g++ harness (tests/cpp/stage_table_harness.cpp), built with the address and undefined-
behaviour sanitizers, executes commands against the header the engine uses.  The reference has no such stage; what is checked is the
id policy, every refusal's text, that a refusal changes nothing, and what a commit does to the counters and to `cur`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOUR = 86400000          # samples of one hour at 24 kHz


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_table") / "stage_table_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "leaxer-qwen3-tts_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "stage_table_harness.cpp"), "-o", exe], check=True)

    def run(*script):
        r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report fails the run
        out = r.stdout.strip().splitlines()
        assert len(out) == len(script)
        return out
    return run


def state(line):
    w = line.split()
    assert w[0] == "state"
    return {w[i]: int(w[i + 1]) for i in range(1, len(w), 2)}


def test_ids_are_reused_lowest_first_and_the_maximum_is_refused(harness):
    out = harness("init 3", "begin 0", "begin 0", "begin 0", "begin 0",      # 0 1 2, then full
                  "end 1", "end 0", "begin 5", "begin 6", "begin 7",          # 0 before 1, then full again
                  "end 2", "begin 8", "get 2", "state 2")
    assert out[1:4] == ["id 0", "id 1", "id 2"]
    assert out[4] == "err pcm sink: at most 3 sinks are open at a time"
    assert out[7:9] == ["id 0", "id 1"] and out[9] == out[4]
    assert out[11] == "id 2" and out[12] == "delay 8"
    assert state(out[13]) == {"used": 1, "finished": 0, "cur": 0, "n_in": 0, "n_out": 0}


def test_unknown_and_ended_ids_are_refused_by_the_stages_noun(harness):
    out = harness("init 4", "begin 3", "get 1", "get -1", "end 1", "len 1 10 0", "push 1 10 0",
                  "end 0", "get 0", "end 0", "len 0 10 0", "state 0")
    assert out[2:7] == ["err pcm sink: no such sink"] * 5
    assert out[7] == "ok" and out[8:11] == ["err pcm sink: no such sink"] * 3
    assert state(out[11])["used"] == 0


def test_refused_pushes_leave_the_counters_alone(harness):
    out = harness("init 4", "begin 100", "push 0 1000 0", "state 0",
                  "len 0 -1 0", "push 0 -1 0",                               # negative
                  "len 0 %d 0" % (HOUR - 1000 + 1), "push 0 %d 1" % (HOUR - 1000 + 1),   # one sample over the hour
                  "state 0", "len 0 %d 0" % (HOUR - 1000),                   # the hour itself is taken
                  "push 0 0 1", "state 0", "len 0 0 0", "push 0 5 0", "len 0 0 1", "state 0")   # finished
    assert out[2] == "out 900"
    before = state(out[3])
    assert before == {"used": 1, "finished": 0, "cur": 1, "n_in": 1000, "n_out": 900}
    assert out[4:6] == ["err pcm sink: negative sample count"] * 2
    assert out[6:8] == ["err pcm sink: sink 0 would exceed one hour of 24 kHz input"] * 2
    assert state(out[8]) == before
    assert out[9] == "len %d" % (HOUR - 1000)
    assert out[10] == "out 100"                                              # the finish flushes what the delay held back
    done = state(out[11])
    assert done == {"used": 1, "finished": 1, "cur": 1, "n_in": 1000, "n_out": 1000}
    assert out[12:15] == ["err pcm sink: sink 0 is finished"] * 3
    assert state(out[15]) == done


def test_commit_advances_the_counters_and_flips_cur_by_the_stages_rule(harness):
    # the harness's rule flips on a push that brings samples and does not finish
    out = harness("init 4", "begin 10", "begin 0",
                  "len 0 4 0", "state 0",                                    # push_len alone changes nothing
                  "push 0 4 0", "state 0", "push 0 0 0", "state 0", "push 0 20 0", "state 0", "push 0 3 1", "state 0",
                  "state 1", "end 0", "begin 2", "state 0")
    assert out[3] == "len 0" and state(out[4]) == {"used": 1, "finished": 0, "cur": 0, "n_in": 0, "n_out": 0}
    assert out[5] == "out 0" and state(out[6]) == {"used": 1, "finished": 0, "cur": 1, "n_in": 4, "n_out": 0}
    assert out[7] == "out 0" and state(out[8]) == state(out[6])             # an empty push: no flip, not finished
    assert out[9] == "out 14" and state(out[10]) == {"used": 1, "finished": 0, "cur": 0, "n_in": 24, "n_out": 14}
    assert out[11] == "out 13" and state(out[12]) == {"used": 1, "finished": 1, "cur": 0, "n_in": 27, "n_out": 27}   # finish: no flip
    assert state(out[13]) == {"used": 1, "finished": 0, "cur": 0, "n_in": 0, "n_out": 0}                             # the neighbour never moved
    assert out[15] == "id 0" and state(out[16]) == {"used": 1, "finished": 0, "cur": 0, "n_in": 0, "n_out": 0}       # a reused id starts afresh
