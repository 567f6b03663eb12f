"""The begin rules of leaxer-qwen3-tts_amd/csrc/q3_begin_plan.h restated in plain Python, entry by entry as the three entries used to
spell them (one loop each), for tests/test_cpu_begin_plan.py to compare the header against.  A member is a dict with the keys of KEYS;
`P` is what its prefix id resolves to, and the flags say which pointers were given (`bad_codes` / `bad_prefix`: what the engine's own
checks, Engine::check_frame_codes and Engine::prefix_get, would refuse)."""
PLAIN, PREFIXED, RAGGED = 0, 1, 2
NAMES = {PLAIN: "slots_begin", PREFIXED: "slots_begin_prefixed", RAGGED: "slots_begin_ragged"}
KEYS = ("slot", "S", "n_trailing", "n_prefix", "max_frames", "kv_tokens", "P")
BAD_CODES, BAD_PREFIX = "frame codes: bad id", "unknown prefix id"


def member(slot, S, n_trailing=0, n_prefix=0, max_frames=0, kv_tokens=0, P=0, prompt=True, trailing=True, codes=True, bad_codes=False,
           bad_prefix=False):
    return dict(slot=slot, S=S, n_trailing=n_trailing, n_prefix=n_prefix, max_frames=max_frames, kv_tokens=kv_tokens, P=P, prompt=prompt,
                trailing=trailing, codes=codes, bad_codes=bad_codes, bad_prefix=bad_prefix)


def limits(B=8, max_ctx=256, max_trailing=32, max_frames_cap=200, rows_max=128, mfma_min_rows=12, mfma_dims=True):
    return dict(B=B, max_ctx=max_ctx, max_trailing=max_trailing, max_frames_cap=max_frames_cap, rows_max=rows_max,
                mfma_min_rows=mfma_min_rows, mfma_dims=mfma_dims)


def _front(q, L):
    if q["slot"] < 0 or q["slot"] >= L["B"]:
        return "slot out of range"
    if q["n_trailing"] < 0 or q["n_trailing"] > L["max_trailing"]:
        return "too many trailing text rows"
    if q["S"] < 1 or q["S"] > L["max_ctx"]:
        return "prefill length must be 1..max_ctx rows"
    return None


def check_plain(ms, max_new, L):
    """slots_begin: no look at the prompt pointer, at a prefix id or for a slot listed twice (that comes with the groups)."""
    for q in ms:
        err = _front(q, L)
        if err:
            return err
        if max_new < 1 or q["S"] + max_new > L["max_ctx"]:
            return "prompt + max_new_tokens exceeds max_ctx"
        if q["n_prefix"] < 0 or (q["n_prefix"] > 0 and not q["codes"]):
            return "prefix codes: n_prefix must be >= 0 (and the codes given)"
        if q["n_prefix"] > 0:
            if q["S"] + q["n_prefix"] + max_new > L["max_ctx"]:
                return "prompt + prefix frames + max_new_tokens exceeds max_ctx"
            if q["n_prefix"] + max_new > L["max_frames_cap"]:
                return "prefix frames + max_new_tokens exceeds the slot's frame capacity"
            if len(ms) != 1:
                return "slots_begin: a slot with prefix codes is begun on its own"
            if q["bad_codes"]:
                return BAD_CODES
    return None


def check_behind_prefixes(entry, ms, max_new, L):
    """slots_begin_prefixed and slots_begin_ragged: the same loop under two names, ragged with one check more."""
    for i, q in enumerate(ms):
        err = _front(q, L)
        if err:
            return err
        if not q["prompt"]:
            return NAMES[entry] + ": null prompt"
        if entry == RAGGED and q["n_trailing"] > 0 and not q["trailing"]:
            return "slots_begin_ragged: trailing rows announced but not given"
        if q["bad_prefix"]:
            return BAD_PREFIX
        if q["n_prefix"] < 0 or (q["n_prefix"] > 0 and not q["codes"]):
            return "prefix codes: n_prefix must be >= 0 (and the codes given)"
        if max_new < 1 or q["P"] + q["S"] + q["n_prefix"] + max_new > L["max_ctx"]:
            return "prefix + prompt + prefix frames + max_new_tokens exceeds max_ctx"
        if q["n_prefix"] > 0:
            if q["n_prefix"] + max_new > L["max_frames_cap"]:
                return "prefix frames + max_new_tokens exceeds the slot's frame capacity"
            if q["bad_codes"]:
                return BAD_CODES
        if any(o["slot"] == q["slot"] for o in ms[:i]):
            return NAMES[entry] + ": slot listed twice"
    return None


def derived(q, P, max_new):
    """(KV tokens reserved, frames the slot may generate, armed max_frames, position after the begin)"""
    cap = min(q["max_frames"], max_new) if q["max_frames"] > 0 else max_new
    own = P + q["S"] + q["n_prefix"]
    tokens = min(own + cap, max(q["kv_tokens"], own)) if q["kv_tokens"] > 0 else own + cap
    return tokens, cap, q["n_prefix"] + cap, own


def groups_plain(ms, L):
    """(i0, g, batched, consecutive) runs, then the error of plain's look for a slot listed twice inside a run (or None)"""
    out, i0 = [], 0
    while i0 < len(ms):
        S = ms[i0]["S"]
        cap = max(1, min(min(L["rows_max"], 128) // S, 128)) if L["mfma_dims"] and S <= 16 else 1
        g, consecutive = 1, True
        while i0 + g < len(ms) and g < cap and ms[i0 + g]["S"] == S:
            consecutive = consecutive and ms[i0 + g]["slot"] == ms[i0]["slot"] + g
            g += 1
        run = [q["slot"] for q in ms[i0:i0 + g]]
        if len(set(run)) != len(run):
            return out, "slots_begin: slot listed twice"
        out.append((i0, g, int(not (g == 1 or g * S < L["mfma_min_rows"])), int(consecutive)))
        i0 += g
    return out, None


def groups_prefixed(ms, L):
    def batchable(q):
        return L["mfma_dims"] and q["S"] <= 16 and q["n_prefix"] == 0
    out, i0 = [], 0
    while i0 < len(ms):
        S = ms[i0]["S"]
        cap = 128 // S if batchable(ms[i0]) else 1
        g, consecutive = 1, True
        while i0 + g < len(ms) and g < cap and batchable(ms[i0 + g]) and ms[i0 + g]["S"] == S:
            consecutive = consecutive and ms[i0 + g]["slot"] == ms[i0]["slot"] + g
            g += 1
        out.append((i0, g, int(not (g == 1 or g * S < L["mfma_min_rows"])), int(consecutive)))
        i0 += g
    return out


def plan(entry, ms, max_new, L):
    """The answer line of the harness's `plan` command."""
    err = check_plain(ms, max_new, L) if entry == PLAIN else check_behind_prefixes(entry, ms, max_new, L)
    if err:
        return "err " + err
    line = "ok m" + "".join(" %d,%d,%d,%d" % derived(q, 0 if entry == PLAIN else q["P"], max_new) for q in ms)
    if entry == RAGGED:
        return line + " rows %d" % sum(q["S"] + q["n_prefix"] for q in ms)
    if entry == PLAIN and len(ms) == 1 and ms[0]["n_prefix"] > 0:
        return line + " forced"
    if entry == PLAIN:
        gs, err = groups_plain(ms, L)
        if err:
            return "err " + err
    else:
        gs = groups_prefixed(ms, L)
    return line + " g" + "".join(" %d,%d,%d,%d" % g for g in gs)


def one_at_a_time(total, L, seg_kernels, seam_step):
    return int(not L["mfma_dims"] or not seg_kernels or total < L["mfma_min_rows"] or seam_step)


def command(entry, ms, max_new):
    flags = lambda q: 1 * q["prompt"] + 2 * q["trailing"] + 4 * q["codes"] + 8 * q["bad_codes"] + 16 * q["bad_prefix"]
    return "plan %d %d %d " % (entry, max_new, len(ms)) + " ".join(" ".join(str(q[k]) for k in KEYS) + " %d" % flags(q) for q in ms)


def limits_command(L):
    return "limits %d %d %d %d %d %d %d" % (L["B"], L["max_ctx"], L["max_trailing"], L["max_frames_cap"], L["rows_max"], L["mfma_min_rows"], L["mfma_dims"])
