"""A second engine on a GPU: private weights against the first engine's weights, shared (q3tts_create_sharing; DESIGN.md 3, "The weight
set").  0.6B dims, synthetic fill.

The donor (max_batch 8: no layer-0 QKV table of its own) is created and filled once.  Then, --rounds times and alternating:
  private : q3tts_create + q3tts_fill_synthetic + q3tts_finalize of a second engine (max_batch 8)
  sharing : q3tts_create_sharing of a second engine (max_batch 8)
and, for the table, the same pair with one-slot second engines (a private one builds its table at finalize; the first sharer builds
the set's table, later sharers reuse it: both are reported, the first from one sample).
Per case: the wall clock from create to ready (the stream drained) and the drop in free device memory (hipMemGetInfo) around the
creation, medians over the rounds with their spread, beside q3tts_weights_info's figures for the new engine.

One process, two engines alive at most.  Every step (a creation, a close) runs under its own time limit (--step-timeout seconds, an
alarm that ends the run), and the whole run belongs under one too:

    timeout -k 10 900 python tools/weight_share_bench.py [--rounds 5] [--out profiles/weight_share.txt]

Prints what it writes."""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "leaxer-qwen3-tts_amd"))

MAX_CTX = 256


class StepTimeout(Exception):
    pass


class step:
    """a step's own time limit: the alarm raises in the main thread and the run ends there"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def on_alarm(signum, frame):
            raise StepTimeout("step '%s' ran longer than %d s" % (self.what, self.seconds))
        signal.signal(signal.SIGALRM, on_alarm)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            rt = C.CDLL(name)
            break
        except OSError:
            rt = None
    if rt is None:
        raise RuntimeError("the HIP runtime library was not found")
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rt.hipDeviceSynchronize.argtypes = []
    return rt


def free_bytes(rt):
    assert rt.hipDeviceSynchronize() == 0
    f, t = C.c_size_t(), C.c_size_t()
    assert rt.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


def med(v, unit, scale=1.0):
    v = [x * scale for x in v]
    return "%10.1f %s (%.1f .. %.1f)" % (statistics.median(v), unit, min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_share.txt"))
    a = ap.parse_args()
    import q3tts
    rt = hip_runtime()
    cfg = q3tts.default_config("0.6b")
    lim = a.step_timeout

    with step("donor", lim):
        donor = q3tts.Engine(cfg, device=0, max_batch=8, max_ctx=MAX_CTX)
        donor.fill_synthetic(seed=0)
    donor_info = donor.weights_info()

    def second(kind, max_batch):
        """(seconds from create to ready, bytes of free device memory it took, its weights_info) of one second engine, closed again"""
        f0 = free_bytes(rt)
        with step("%s b=%d: create" % (kind, max_batch), lim):
            t0 = time.perf_counter()
            if kind == "private":
                e = q3tts.Engine(cfg, device=0, max_batch=max_batch, max_ctx=MAX_CTX)
                e.fill_synthetic(seed=0)      # fill + finalize, as the donor
            else:
                e = donor.share(max_batch=max_batch, max_ctx=MAX_CTX)
            e.kv_pool_info()                  # ready: both constructors end with their stream drained
            dt = time.perf_counter() - t0
        took = f0 - free_bytes(rt)
        info = e.weights_info()
        with step("%s b=%d: close" % (kind, max_batch), lim):
            e.close()
        return dt, took, info

    lines = ["A second engine on one MI355X: private weights against the first engine's weights, shared; 0.6B dims, synthetic weights",
             "python tools/weight_share_bench.py --rounds %d" % a.rounds,
             "donor: max_batch 8, max_ctx %d; its set: %d bytes, %d holder; cases alternate round by round in one process, one warm-up round each;"
             % (MAX_CTX, donor_info["shared_bytes"], donor_info["holders"]),
             "median (min .. max) over %d rounds; wall: create to ready; memory: drop of hipMemGetInfo's free bytes around the creation" % a.rounds, ""]
    for max_batch in (8, 1):
        res = {"private": [], "sharing": []}
        first_share = None
        for r in range(a.rounds + 1):
            for kind in ("private", "sharing"):
                one = second(kind, max_batch)
                if kind == "sharing" and max_batch == 1 and first_share is None:
                    first_share = one         # builds the set's table: reported on its own
                    one = second(kind, max_batch)
                if r >= 1:
                    res[kind].append(one)
        lines.append("second engine with max_batch %d%s" % (max_batch, " (the layer-0 QKV table applies)" if max_batch <= 2 else ""))
        for kind in ("private", "sharing"):
            v = res[kind]
            info = v[-1][2]
            lines.append("    %-8s: wall %s | memory %s | weights_info: shared_bytes %d, holders %d, private_weight_bytes %d"
                         % (kind, med([x[0] for x in v], "ms", 1e3), med([x[1] for x in v], "MiB", 1.0 / (1 << 20)),
                            info["shared_bytes"], info["holders"], info["private_weight_bytes"]))
        if first_share is not None:
            lines.append("    the first one-slot sharer (builds the set's table, one sample): wall %.1f ms | memory %.1f MiB | shared_bytes %d"
                         % (first_share[0] * 1e3, first_share[1] / (1 << 20), first_share[2]["shared_bytes"]))
        mp, ms = statistics.median(x[1] for x in res["private"]), statistics.median(x[1] for x in res["sharing"])
        tp, ts = statistics.median(x[0] for x in res["private"]), statistics.median(x[0] for x in res["sharing"])
        lines.append("    sharing saves %.1f MiB of %.1f MiB and %.1f ms of %.1f ms" % ((mp - ms) / (1 << 20), mp / (1 << 20), (tp - ts) * 1e3, tp * 1e3))
        lines.append("")
    with step("donor: close", lim):
        donor.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
