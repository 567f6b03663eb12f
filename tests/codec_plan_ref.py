"""The vocoder's host arithmetic (leaxer-qwen3-tts_amd/csrc/q3_codec_plan.h) restated in plain Python, as the decode paths used to spell
it in place, for tests/test_cpu_codec_plan.py to compare the header against.  A config is a dict with the vocoder's dims (DIMS)."""
DIMS = ("cd_codebook", "cd_hidden", "cd_heads", "cd_head_dim", "cd_ffn", "cd_tconv_trim")
KSLAB_FLOATS = 32 * 128 * 4096


def dims(cfg):
    """the dict of a q3_oracle Config (or anything with the cd_* attributes)"""
    d = {k: int(getattr(cfg, k)) for k in DIMS}
    d["ratios"] = [int(cfg.cd_up_ratios[i]) for i in range(cfg.cd_n_up)]
    d["rates"] = [int(cfg.cd_up_rates[i]) for i in range(cfg.cd_n_blocks)]
    return d


def cfg_command(d):
    return "cfg %s %d %s %d %s" % (" ".join(str(d[k]) for k in DIMS), len(d["ratios"]), " ".join(map(str, d["ratios"])),
                                   len(d["rates"]), " ".join(map(str, d["rates"])))


def decode_len(d, F):
    """q3tts_codec_decode_len"""
    T = F
    for f in d["ratios"]:
        T *= f
    for r in d["rates"]:
        k = 2 * r
        pad = k - r
        left = pad if d["cd_tconv_trim"] == 0 else 0
        T = (T - 1) * r + k - left - pad
    return T


def len_of(d, n):
    return 0 if n <= 0 else decode_len(d, n)


def up_front(d):
    up = 1
    for f in d["ratios"]:
        up *= f
    return up


def samples_per_frame(d):
    up = up_front(d)
    for r in d["rates"]:
        up *= r
    return up


def stage_b_context(d):
    frames, rate = 0.0, 1.0
    for f in d["ratios"]:
        rate *= f
        frames += 6.0 / rate
    frames += 6.0 / rate
    for r in d["rates"]:
        frames += 1.0 / rate
        rate *= r
        frames += 6.0 * (1 + 3 + 9) / rate
    frames += 6.0 / rate
    return int(frames) + 3


def window_cut(d, a0, n, ctx):
    """(first, n_own) of frames [a0, a0 + n) inside the decode of the window [a0 - ctx, a0 + n)"""
    return len_of(d, a0) - samples_per_frame(d) * (a0 - ctx), len_of(d, a0 + n) - len_of(d, a0)


def push_groups(streams, ctxB):
    """streams: [(n_done, n)] -> (order, [(i0, i1, Tw)]): the batched push's stable order by left context, descending, and its groups"""
    order = sorted(range(len(streams)), key=lambda x: -min(streams[x][0], ctxB))      # sorted() is stable
    ctx = [min(streams[x][0], ctxB) for x in order]
    new = [streams[x][1] for x in order]
    groups, i0 = [], 0
    while i0 < len(order):
        i1, Tw = i0, 0
        while i1 < len(order) and ctx[i1] == ctx[i0]:
            Tw1 = max(Tw, ctx[i1] + new[i1])
            if i1 > i0 and (i1 - i0 + 1) * Tw1 * 4700000 > (16 << 30):
                break
            Tw, i1 = Tw1, i1 + 1
        groups.append((i0, i1, Tw))
        i0 = i1
    return order, groups


def groups_command(streams, ctxB):
    return "groups %d %d %s" % (ctxB, len(streams), " ".join("%d %d" % s for s in streams))


def groups_answer(streams, ctxB):
    order, groups = push_groups(streams, ctxB)
    return "o" + "".join(" %d" % x for x in order) + " g" + "".join(" %d,%d,%d" % g for g in groups)


def bytes_of(nfloat):
    return (nfloat * 4 + 255) & ~255


def pre_bytes(d, rows):
    CH, FF = d["cd_hidden"], d["cd_ffn"]
    return bytes_of(rows * CH) * 3 + bytes_of(rows * 3 * CH) + bytes_of(rows * FF) * 2 + bytes_of(KSLAB_FLOATS)


def upsample_bytes(d, rows):
    need = 0
    for f in d["ratios"]:
        rows *= f
        need += bytes_of(rows * d["cd_hidden"]) * 2 + bytes_of(rows * 4 * d["cd_hidden"])
    return need


def scratch_kv_bytes(d, n, P):
    return bytes_of(n * d["cd_heads"] * P * d["cd_head_dim"]) * 2


def batch_arena_bytes(d, n, Fp, P, with_upsampling):
    return pre_bytes(d, n * Fp) + scratch_kv_bytes(d, n, P) + (upsample_bytes(d, n * Fp) if with_upsampling else 0)


def sbatch_push_bytes(d, T, back_rows):
    return pre_bytes(d, T) + bytes_of(back_rows * d["cd_hidden"]) + upsample_bytes(d, back_rows)


def sbatch_prime_bytes(d, g, Fp, Ps):
    return pre_bytes(d, g * Fp) + scratch_kv_bytes(d, g, Ps)
