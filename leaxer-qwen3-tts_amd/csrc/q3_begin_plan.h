// q3_begin_plan.h — the host arithmetic every way of beginning utterances in slots shares (q3_begin.cpp: slots_begin, slots_begin_prefixed,
// slots_begin_ragged, slot_begin_forced beneath them; talker_prefill_dev takes its groups from here too): the member checks with their
// texts and order, the quantities derived from a member, the equal-length grouping rule and the ragged entry's one-at-a-time decision.
// No HIP in here: tests/test_cpu_begin_plan.py drives this header from a plain g++ harness.  The reference begins one utterance at a time
// (run_prefill, src/tts_onnx.cpp:615-665) and has none of this.
//
// What the three entries do NOT share is behaviour, and the reason they are not one function:
//   max_ctx       plain refuses S + max_new > max_ctx ("prompt + max_new_tokens exceeds max_ctx") and, with forced frames, then
//                 S + n_prefix + max_new ("prompt + prefix frames + ..."); prefixed and ragged have the one text "prefix + prompt + prefix
//                 frames + max_new_tokens exceeds max_ctx", behind the forced-frames argument check instead of in front of it.
//   forced frames plain takes a member with n_prefix > 0 only on its own (n == 1); the other two take it anywhere.
//   null prompt   plain does not look (talker_prefill refuses it later, under its own name); prefixed and ragged refuse it under their
//                 names; ragged alone refuses trailing rows that are announced but not given.
//   slot twice    prefixed and ragged look over the whole call, member by member, before anything is reserved.  Plain looks inside one
//                 group only, when it reaches the group (pages reserved, earlier groups prefilled), so it accepts one slot in two groups.
//   group cap     plain: max(1, min(min(rows_max, 128) / S, 128)) members (its pass runs in the rows_max-row workspace); prefixed:
//                 128 / S (its group lives in the 128-row long workspace).  Both: 1 for S > 16 or dims that fail
//                 Engine::mfma_dims_ok, and a member with forced frames never joins a group.  Ragged does not group at all.
//   forwarding    prefixed with no prefix anywhere IS plain (plain's texts); ragged with n == 1 IS prefixed; the ragged fallback reserves
//                 for the set and then begins each member through prefixed with n = 1.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace q3 {

enum BeginEntry { BEGIN_PLAIN = 0, BEGIN_PREFIXED = 1, BEGIN_RAGGED = 2 };

// What the rules read of an Engine::SlotInit.  P: rows of the shared prefix in front of the prompt (0: none), resolved by begin_check.
struct BeginMember {
    int slot = 0, S = 0, n_trailing = 0, n_prefix = 0, max_frames = 0, kv_tokens = 0, P = 0;
    bool has_prompt = false, has_trailing = false, has_codes = false;   // the pointers were given
};
struct BeginLimits {
    int B = 0, max_ctx = 0, max_trailing = 0, max_frames_cap = 0, rows_max = 0, mfma_min_rows = 0;
    bool mfma_dims = false;   // Engine::mfma_dims_ok(talker): batched passes take the MFMA path
};

// ---- derived quantities ----
inline int begin_cap(const BeginMember& q, int max_new) { return q.max_frames > 0 ? std::min(q.max_frames, max_new) : max_new; }   // frames the slot may generate
inline int begin_own(const BeginMember& q) { return q.P + q.S + q.n_prefix; }                        // rows in the cache after the begin: the slot's position
inline int begin_armed_max_frames(const BeginMember& q, int max_new) { return q.n_prefix + begin_cap(q, max_new); }
// KV tokens reserved at the begin: every frame the slot may generate, or what a caller that grows the share itself (the scheduler) asks for
inline int begin_tokens(const BeginMember& q, int max_new) {
    const int own = begin_own(q), all = own + begin_cap(q, max_new);
    return q.kv_tokens > 0 ? std::min(all, std::max(q.kv_tokens, own)) : all;
}

// ---- the member checks: every member in call order, the first fault found throws Err(text) ----
// resolve_P(i): the prefix length of member i (throws on an unknown id); not called by plain.  check_codes(i): the forced frames' ids
// (Engine::check_frame_codes, which needs the config); called where the entries always called it.
template <class Err, class ResolveP, class CheckCodes>
void begin_check(BeginEntry e, BeginMember* m, int n, int max_new, const BeginLimits& L, ResolveP resolve_P, CheckCodes check_codes) {
    static const char* const who[] = { "slots_begin", "slots_begin_prefixed", "slots_begin_ragged" };
    const bool plain = e == BEGIN_PLAIN;
    for (int i = 0; i < n; ++i) {
        BeginMember& q = m[i];
        if (q.slot < 0 || q.slot >= L.B) throw Err("slot out of range");
        if (q.n_trailing < 0 || q.n_trailing > L.max_trailing) throw Err("too many trailing text rows");
        if (q.S < 1 || q.S > L.max_ctx) throw Err("prefill length must be 1..max_ctx rows");
        if (plain && (max_new < 1 || q.S + max_new > L.max_ctx)) throw Err("prompt + max_new_tokens exceeds max_ctx");
        if (!plain) {
            if (!q.has_prompt) throw Err(std::string(who[e]) + ": null prompt");
            if (e == BEGIN_RAGGED && q.n_trailing > 0 && !q.has_trailing) throw Err("slots_begin_ragged: trailing rows announced but not given");
            q.P = resolve_P(i);
        }
        if (q.n_prefix < 0 || (q.n_prefix > 0 && !q.has_codes)) throw Err("prefix codes: n_prefix must be >= 0 (and the codes given)");
        if (!plain && (max_new < 1 || begin_own(q) + max_new > L.max_ctx)) throw Err("prefix + prompt + prefix frames + max_new_tokens exceeds max_ctx");
        if (q.n_prefix > 0) {
            if (plain && q.S + q.n_prefix + max_new > L.max_ctx) throw Err("prompt + prefix frames + max_new_tokens exceeds max_ctx");
            if (q.n_prefix + max_new > L.max_frames_cap) throw Err("prefix frames + max_new_tokens exceeds the slot's frame capacity");
            if (plain && n != 1) throw Err("slots_begin: a slot with prefix codes is begun on its own");
            check_codes(i);
        }
        if (!plain) for (int j = 0; j < i; ++j) if (m[j].slot == q.slot) throw Err(std::string(who[e]) + ": slot listed twice");
    }
}

// ---- the grouping rule: runs of members with the same S share one pass through the layers ----
// batched: the run takes one MFMA pass (g * S >= mfma_min_rows rows); otherwise its members are prefilled one at a time.
// consecutive: the run's slot ids ascend by one (plain writes its results in place then, and through a slot map otherwise).
struct BeginGroup { int i0 = 0, g = 1; bool batched = false, consecutive = true; };
inline int begin_group_cap(BeginEntry e, const BeginMember& q, const BeginLimits& L) {
    if (!L.mfma_dims || q.S > 16 || q.n_prefix > 0) return 1;   // a long prompt or forced frames: on its own, the chunk path
    return e == BEGIN_PLAIN ? std::max(1, std::min(std::min(L.rows_max, 128) / q.S, 128)) : 128 / q.S;
}
inline std::vector<BeginGroup> begin_groups(BeginEntry e, const BeginMember* m, int n, const BeginLimits& L) {
    std::vector<BeginGroup> out;
    for (int i0 = 0; i0 < n;) {
        BeginGroup gr;
        gr.i0 = i0;
        const int S = m[i0].S, cap = begin_group_cap(e, m[i0], L);
        while (i0 + gr.g < n && gr.g < cap && m[i0 + gr.g].S == S && m[i0 + gr.g].n_prefix == 0) {
            gr.consecutive = gr.consecutive && m[i0 + gr.g].slot == m[i0].slot + gr.g;
            ++gr.g;
        }
        gr.batched = gr.g > 1 && gr.g * S >= L.mfma_min_rows;
        out.push_back(gr);
        i0 += gr.g;
    }
    return out;
}

// plain's own look for a slot listed twice: inside the group it is about to prefill (one row group writes a slot's cache rows)
template <class Err>
void begin_check_group_slots(const BeginMember* m, const BeginGroup& gr) {
    for (int k = 1; k < gr.g; ++k)
        for (int j = 0; j < k; ++j) if (m[gr.i0 + k].slot == m[gr.i0 + j].slot) throw Err("slots_begin: slot listed twice");
}

// ---- the ragged entry ----
inline size_t begin_ragged_rows(const BeginMember* m, int n) {   // rows it stages: prompts and forced frames, not the prefixes
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)(m[i].S + m[i].n_prefix);
    return total;
}
// true: the members are begun one at a time (each exactly as slots_begin_prefixed with n = 1 begins it).  seg_kernels: the segment form of
// the chunk attention is instantiated for the talker's heads; seam_step: inside a decode step
inline bool begin_ragged_one_at_a_time(size_t total_rows, const BeginLimits& L, bool seg_kernels, bool seam_step) {
    return !L.mfma_dims || !seg_kernels || total_rows < (size_t)L.mfma_min_rows || seam_step;
}

} // namespace q3
