// q3_begin.cpp — beginning utterances in slots (q3_engine.h "fused generation"): slots_begin, slots_begin_prefixed and slots_begin_ragged
// with the forced begin beneath them, the shared prompt prefixes and the given frames' rows.  The three entries issue their rows in three
// ways (the equal-length pass in xp, the group form at per-member bases in the long workspace, the segment form over 128-row chunks) and
// which prompts share a pass decides the bits, so they stay three; everything around the launches is written once: the rules in
// q3_begin_plan.h, the helpers right below.
#include "q3_engine.h"

#include <algorithm>
#include <cstdio>

namespace q3 {

static BeginMember member_of(const Engine::SlotInit& q, int P = 0) {
    return BeginMember{q.slot, q.S, q.n_trailing, q.n_prefix, q.max_frames, q.kv_tokens, P, q.prompt != nullptr, q.trailing != nullptr, q.prefix != nullptr};
}

// the members as the plan reads them, checked (begin_check: the entry's refusals, before anything is reserved or armed)
std::vector<BeginMember> Engine::begin_members(BeginEntry e, const SlotInit* in, int n, int max_new) {
    std::vector<BeginMember> m((size_t)std::max(n, 0));
    for (size_t i = 0; i < m.size(); ++i) m[i] = member_of(in[i]);
    begin_check<Error>(e, m.data(), n, max_new, begin_limits(),
                       [&](int i) { return in[i].prefix_id != -1 ? prefix_get(in[i].prefix_id).P : 0; },
                       [&](int i) { check_frame_codes(in[i].prefix, in[i].n_prefix, true); });
    return m;
}

// KV pages for the members of a begin (begin_tokens: prefix, prompt, forced frames and every frame the slot may generate), all or nothing:
// nothing is reserved, and so nothing armed, if the pool cannot hold the set
void Engine::kv_reserve_set(const BeginMember* m, int n, int max_new) {
    auto want = [&](int i) { return kv_pages_for(begin_tokens(m[i], max_new)); };
    int need = 0;
    for (int i = 0; i < n; ++i) need += want(i) - kv_slot_pages(m[i].slot);
    if (need > kv_free_pages()) {
        char msg[160];
        snprintf(msg, sizeof msg, "KV page pool exhausted: %d slots need %d more pages, %d of %d free", n, need, kv_free_pages(), kv_total_pages());
        throw Error(msg);
    }
    for (int pass = 0; pass < 2; ++pass)   // slots that give pages back first
        for (int i = 0; i < n; ++i)
            if ((want(i) <= kv_slot_pages(m[i].slot)) == (pass == 0)) kv_reserve(m[i].slot, begin_tokens(m[i], max_new), true);
}

// each prefix's rows into the pages of its slots: one launch per prefix (per 128 slots)
void Engine::prefix_fan_out(const SlotInit* in, int n) {
    std::vector<int32_t> map_h;
    std::vector<char> done((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (done[(size_t)i] || in[i].prefix_id == -1) continue;
        map_h.clear();
        for (int j = i; j < n; ++j) if (in[j].prefix_id == in[i].prefix_id) { map_h.push_back(in[j].slot); done[(size_t)j] = 1; }
        const Prefix& pf = prefix_get(in[i].prefix_id);
        for (size_t o = 0; o < map_h.size(); o += 128) {
            const int m = (int)std::min<size_t>(128, map_h.size() - o);
            Q3_HIP_CHECK(hipMemcpyAsync(slot_map_d, map_h.data() + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, stream));
            kv_prefix_copy(pf, slot_map_d, m, 0, true);
            sync();   // map_h and slot_map_d are reused
        }
    }
}

// a member's head logits and normalised last row, from wherever its pass left them, into the fused path's state of its slot
void Engine::scatter_last_rows(const float* logits_row, const float* hidden_row, int slot) {
    const int H = c.hidden, V = c.vocab;
    launch_copy_rows(logits_row, V, logits_t + (size_t)slot * V, V, 1, V, stream);
    launch_copy_rows(hidden_row, H, x_cp + (size_t)slot * 2 * H, 2 * H, 1, H, stream);
}

// what a new utterance's first step reads besides the prefill's results: its trailing text rows and an empty code0 history.  The forced and ragged
// begins call this in front of frame_rows_launch, which reads the rows and sets the history's bits, and arm with stage_inputs == false.
void Engine::stage_slot_inputs(const SlotInit& q) {
    if (q.n_trailing > 0)
        Q3_HIP_CHECK(hipMemcpyAsync(trailing_d + (size_t)q.slot * max_trailing * c.hidden, q.trailing, (size_t)q.n_trailing * c.hidden * sizeof(float), hipMemcpyHostToDevice, stream));
    Q3_HIP_CHECK(hipMemsetAsync(seen_d + (size_t)q.slot * seen_ld, 0, (size_t)seen_ld * sizeof(uint32_t), stream));
}

// The one place that writes the armed SlotState: the slot as it is after its prefill behind P prefix rows, with its q.n_prefix forced
// frames counted as generated.  After the prefill, which writes prompt_len and n_frames; talker_pos_d is the prefill's to write.
void Engine::arm_slot(const SlotInit& q, int P, float rep_penalty, const q3tts_sampling& p, uint64_t seed, int ignore_eos, bool stage_inputs) {
    if (stage_inputs) stage_slot_inputs(q);
    slot_codec_stream_reset(q.slot);   // a new utterance: its streaming vocoder state starts over
    SlotState& s = st_h[q.slot];
    s.n_frames = q.n_prefix; s.finished = 0; s.active = 1; s.prompt_len = q.S; s.prefix_len = P; s.trailing_len = q.n_trailing; s.text_open = 0; stepped_h[q.slot] = 0;
    s.max_frames = begin_armed_max_frames(member_of(q), p.max_new_tokens);
    s.top_k = p.top_k; s.ignore_eos = ignore_eos; s.temperature = p.temperature; s.top_p = p.top_p; s.stream_id = q.stream_id; s.rep_penalty = rep_penalty; s.seed = seed;
    Q3_HIP_CHECK(hipMemcpyAsync(st_d + q.slot, &s, sizeof(SlotState), hipMemcpyHostToDevice, stream));
}

void Engine::slot_begin(int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                        const q3tts_sampling& p, uint64_t seed, uint32_t stream_id, int ignore_eos) {
    SlotInit in;
    in.slot = slot; in.prompt = prompt; in.S = S; in.trailing = trailing; in.n_trailing = n_trailing; in.stream_id = stream_id;
    slots_begin(&in, 1, p, seed, ignore_eos);
}

// Prefill of several slots at once: slots with equal prompt length share one pass through the talker stack (rows = slots x S,
// groups of at most 128 rows on the MFMA path), only the last row of each prompt goes through the codec head.  One
// synchronisation for the whole set instead of two per slot.
void Engine::slots_begin(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos) {
    if (!finalized) throw Error("weights not finalized");
    const int H = c.hidden, V = c.vocab;
    const float rep_penalty = checked_penalty(p);   // before anything is reserved or armed
    const std::vector<BeginMember> m = begin_members(BEGIN_PLAIN, in, n, p.max_new_tokens);
    if (n == 1 && in[0].n_prefix > 0) { slot_begin_forced(in[0], p, seed, ignore_eos, rep_penalty); return; }
    kv_reserve_set(m.data(), n, p.max_new_tokens);
    std::vector<int32_t> pos_h, map_h;
    // a group (begin_groups): consecutive slot ids write their results in place, scattered ones (the scheduler re-arming whatever
    // finished) go through a slot map and a scatter of the head's rows; a prompt of more than 16 rows is prefilled on its own, in
    // chunks (talker_prefill's long path)
    for (const BeginGroup& gr : begin_groups(BEGIN_PLAIN, m.data(), n, begin_limits())) {
        begin_check_group_slots<Error>(m.data(), gr);
        const int i0 = gr.i0, g = gr.g, S = in[i0].S, slot0 = in[i0].slot;
        if (!gr.batched) {
            for (int k = 0; k < g; ++k) talker_prefill(in[i0 + k].slot, in[i0 + k].prompt, S, nullptr, nullptr);
            continue;
        }
        for (int k = 0; k < g; ++k)
            Q3_HIP_CHECK(hipMemcpyAsync(xp + (size_t)k * S * H, in[i0 + k].prompt, (size_t)S * H * sizeof(float), hipMemcpyHostToDevice, stream));
        pos_h.assign((size_t)g, S);
        if (gr.consecutive) {
            const bool pr = run_layers(talker, xp, H, g, S, slot0, nullptr, 0, talker_norm, c.rms_eps, hn, H);
            if (!pr) throw Error("batched prefill expects the MFMA path");   // M = g*S >= mfma_min_rows by construction
            // codec head on the last row of every prompt straight into the fused path's logits; normalised last rows -> predictor input
            head_proj(codec_head, xp, H, talker_norm, c.rms_eps, nullptr, 0, logits_t + (size_t)slot0 * V, V, g, V, H, true, true, S - 1, S);
            launch_copy_rows(hn + (size_t)(S - 1) * H, S * H, x_cp + (size_t)slot0 * 2 * H, 2 * H, g, H, stream);
            Q3_HIP_CHECK(hipMemcpyAsync(talker_pos_d + slot0, pos_h.data(), (size_t)g * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        } else {
            map_h.resize((size_t)g);
            for (int k = 0; k < g; ++k) map_h[(size_t)k] = in[i0 + k].slot;
            Q3_HIP_CHECK(hipMemcpyAsync(slot_map_d, map_h.data(), (size_t)g * sizeof(int), hipMemcpyHostToDevice, stream));
            const bool pr = run_layers(talker, xp, H, g, S, 0, nullptr, 0, talker_norm, c.rms_eps, hn, H, slot_map_d);
            if (!pr) throw Error("batched prefill expects the MFMA path");
            head_proj(codec_head, xp, H, talker_norm, c.rms_eps, nullptr, 0, logits_g, V, g, V, H, true, true, S - 1, S);
            for (int k = 0; k < g; ++k) {
                scatter_last_rows(logits_g + (size_t)k * V, hn + (size_t)(k * S + S - 1) * H, in[i0 + k].slot);
                Q3_HIP_CHECK(hipMemcpyAsync(talker_pos_d + in[i0 + k].slot, pos_h.data(), sizeof(int32_t), hipMemcpyHostToDevice, stream));
            }
        }
        sync();   // pos_h / map_h are reused by the next group
    }
    for (int i = 0; i < n; ++i) arm_slot(in[i], 0, rep_penalty, p, seed, ignore_eos, true);
    sync();
}

void Engine::check_frame_codes(const int64_t* codes, int n, bool strict) const {
    const int G = c.n_groups;
    for (int f = 0; f < n; ++f)
        for (int g = 0; g < G; ++g) {
            const int64_t v = codes[(size_t)f * G + g];
            const bool ok = g == 0 ? v >= 0 && v < c.vocab && !(strict && ((v >= c.suppress_begin && v < c.suppress_end) || v == c.codec_eos)) : v >= 0 && v < c.sub_vocab;
            if (!ok) {
                char msg[200];
                snprintf(msg, sizeof msg, "frame codes: frame %d group %d holds %lld, outside %s", f, g, (long long)v,
                         g != 0 ? "[0, sub_vocab)" : (strict ? "[0, vocab) without the suppressed ids (EOS among them)" : "[0, vocab)"));
                throw Error(msg);
            }
        }
}

void Engine::frame_rows_launch(const int64_t* codes, int n, int frame0, const float* trailing_dev, int trailing_len, float* out_dev,
                               int32_t* codes_out, uint32_t* seen) {
    const int G = c.n_groups;
    if ((size_t)n * G > frame_codes_cap) regrow(frame_codes_d, frame_codes_cap, std::max((size_t)n, (size_t)256) * G);
    Q3_HIP_CHECK(hipMemcpyAsync(frame_codes_d, codes, (size_t)n * G * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    FrameRowsArgs a;
    a.codes = frame_codes_d; a.n = n; a.n_groups = G; a.H = c.hidden;
    a.embed0 = codec_embed_w; a.V0 = c.vocab; a.SV = c.sub_vocab;
    for (int g = 0; g < G - 1; ++g) a.embed_sub[g] = cp_embed_w[(size_t)g];
    a.trailing = trailing_dev; a.frame0 = frame0; a.trailing_len = trailing_len; a.tts_pad = tts_pad_d;
    a.out = out_dev; a.ldo = c.hidden; a.codes_out = codes_out; a.seen = seen;
    launch_frame_rows(a, stream);
}

// q3tts_frame_rows_host: the kernel on its own, for callers and tests
void Engine::frame_rows(const int64_t* codes, int n, int frame0, const float* trailing, int n_trailing, float* out) {
    if (!finalized) throw Error("weights not finalized");
    if (n < 0 || frame0 < 0 || n_trailing < 0) throw Error("frame_rows: negative argument");
    if (n == 0) return;
    if (!codes || !out || (n_trailing > 0 && !trailing)) throw Error("frame_rows: null argument");
    if (n > max_ctx) throw Error("frame_rows: more frames than max_ctx in one call");
    check_frame_codes(codes, n, false);
    const int H = c.hidden;
    const int n_text = std::max(0, std::min(n_trailing - frame0, n));   // frames frame0 .. frame0 + n_text - 1 have a text row, the rest tts_pad
    if ((size_t)n_text > frame_text_rows) regrow(frame_text_d, frame_text_rows, std::max((size_t)n_text, (size_t)64), H);
    float* x = long_rows(n);
    if (n_text > 0) Q3_HIP_CHECK(hipMemcpyAsync(frame_text_d, trailing + (size_t)frame0 * H, (size_t)n_text * H * sizeof(float), hipMemcpyHostToDevice, stream));
    frame_rows_launch(codes, n, frame0, frame_text_d, frame0 + n_text, x, nullptr, nullptr);
    Q3_HIP_CHECK(hipMemcpyAsync(out, x, (size_t)n * H * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
}

// Forced begin (include/q3tts.h: q3tts_slot_begin_codes): the slot as q3tts_slot_begin would have it after generating exactly q.prefix
// as its first frames.  The forced frames' rows are made on the device behind the prompt rows and the S + F0 rows take the prefill the
// same rows would take as a prompt (one pass up to 16 rows, causal chunks beyond); the launch that makes the rows also records the
// frames (codes, code0 bitmap).  Validated by the entry that calls it.
void Engine::slot_begin_forced(const SlotInit& q, const q3tts_sampling& p, uint64_t seed, int ignore_eos, float rep_penalty, int base) {
    const int H = c.hidden, G = c.n_groups, S = q.S, F0 = q.n_prefix, R = S + F0, slot = q.slot;
    const BeginMember m = member_of(q, base);
    kv_reserve_set(&m, 1, p.max_new_tokens);
    float* x = R <= 16 ? xp : long_rows(R);
    Q3_HIP_CHECK(hipMemcpyAsync(x, q.prompt, (size_t)S * H * sizeof(float), hipMemcpyHostToDevice, stream));
    stage_slot_inputs(q);   // in front of the launch that reads the trailing rows and sets the history's bits
    frame_rows_launch(q.prefix, F0, 0, trailing_d + (size_t)slot * max_trailing * H, q.n_trailing, x + (size_t)S * H, codes_d + (size_t)slot * max_frames_cap * G,
                      seen_d + (size_t)slot * seen_ld);
    if (R <= 16 && base == 0) prefill_rows_in_xp(slot, R);
    else prefill_rows_long(slot, x, R, nullptr, base);   // behind a shared prefix: the chunk path at base, whatever R
    arm_slot(q, base, rep_penalty, p, seed, ignore_eos, false);   // after the prefill, which writes prompt_len = R and n_frames = 0
    sync();
}

// ------------------------------------------------------------------------------------------------
// shared prompt prefix (q3_engine.h)
// ------------------------------------------------------------------------------------------------
const Engine::Prefix& Engine::prefix_get(int id) const {
    auto it = prefixes.find(id);
    if (it == prefixes.end()) throw Error("unknown prefix id " + std::to_string(id) + " (never created, or released)");
    return it->second;
}

void Engine::prefix_pin(int id, int delta) { const_cast<Prefix&>(prefix_get(id)).users += delta; }

void Engine::kv_prefix_copy(const Prefix& pf, const int* slots_dev, int n_dst, int slot0, bool scatter) {
    KvPrefixCopyArgs a;
    a.kcache = talker.kc; a.vcache = talker.vc; a.kstore = pf.k; a.vstore = pf.v;
    a.page_table = talker.page_table; a.pages_per_slot = talker.pages_per_slot;
    a.slots = slots_dev; a.n_dst = n_dst; a.slot0 = slot0; a.scatter = scatter ? 1 : 0;
    a.n_lk = talker.L * talker.nkv; a.P = pf.P; a.row16 = talker.d * (talker.kv_bf16 ? 2 : 4) / 16;
    if (talker.page_shift != 6 || (talker.d * (talker.kv_bf16 ? 2 : 4)) % 16 != 0) throw Error("kv prefix copy: 64-token pages and token rows of whole 16-byte units");
    launch_kv_prefix_copy(a, stream);
}

int Engine::prefix_create(const float* rows, int P) {
    if (!finalized) throw Error("weights not finalized");
    if (!rows) throw Error("prefix_create: null rows");
    if (P < 1 || P >= max_ctx) throw Error("prefix_create: 1 <= rows < max_ctx");
    if ((int)prefixes.size() >= kMaxPrefixes) throw Error("prefix_create: " + std::to_string(kMaxPrefixes) + " prefixes are live already (release one)");
    int slot = -1;   // borrowed: not armed and holding no pages (a session-shaped prefill's cache rows are left alone)
    for (int b = B - 1; b >= 0 && slot < 0; --b) if (!st_h[b].active && kv_slot_pages(b) == 0) slot = b;
    if (slot < 0) throw Error("prefix_create: no free slot to prefill the prefix in (every slot is armed or holds KV pages)");
    if (kv_pages_for(P) > kv_free_pages()) {
        char msg[160];
        snprintf(msg, sizeof msg, "KV page pool exhausted: a prefix of %d rows needs %d pages, %d of %d free", P, kv_pages_for(P), kv_free_pages(), kv_total_pages());
        throw Error(msg);
    }
    const int H = c.hidden;
    Prefix pf;
    pf.P = P;
    const size_t half = (size_t)P * talker.L * talker.nkv * talker.d * (talker.kv_bf16 ? 2 : 4);
    pf.bytes = (int64_t)(2 * half);
    float* x = P <= 16 ? xp : long_rows(P);   // before the store exists: long_rows may throw
    Q3_HIP_CHECK(hipMalloc(&pf.k, half));
    if (hipMalloc(&pf.v, half) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(pf.k); throw Error("prefix_create: out of device memory for the store"); }
    const SlotState keep = st_h[slot];
    try {
        kv_reserve(slot, P, true);
        Q3_HIP_CHECK(hipMemcpyAsync(x, rows, (size_t)P * H * sizeof(float), hipMemcpyHostToDevice, stream));
        if (P <= 16) { prefill_rows_in_xp(slot, P); sync(); }
        else prefill_rows_long(slot, x, P, nullptr);
        kv_prefix_copy(pf, nullptr, 1, slot, false);
        sync();
    } catch (...) {
        st_h[slot] = keep;
        try { kv_release(slot); sync(); } catch (...) { }
        (void)hipFree(pf.k); (void)hipFree(pf.v);
        throw;
    }
    st_h[slot] = keep;
    kv_release(slot);
    sync();   // the table row's upload reads the host mirror
    const int id = prefix_next_id++;
    prefixes[id] = pf;
    return id;
}

void Engine::prefix_release(int id) {
    const Prefix pf = prefix_get(id);
    if (pf.users > 0) throw Error("prefix_release: prefix " + std::to_string(id) + " is in use by a running job");
    sync();
    (void)hipFree(pf.k); (void)hipFree(pf.v);
    prefixes.erase(id);
}

// run_prefill (tts_onnx.cpp:615-665) for slots begun behind shared prefixes: see q3_engine.h.
void Engine::slots_begin_prefixed(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos) {
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || in[i].prefix_id != -1;
    if (!any) { slots_begin(in, n, p, seed, ignore_eos); return; }   // no prefix anywhere: the plain path, untouched
    if (!finalized) throw Error("weights not finalized");
    const int H = c.hidden, V = c.vocab;
    const float rep_penalty = checked_penalty(p);
    const std::vector<BeginMember> m = begin_members(BEGIN_PREFIXED, in, n, p.max_new_tokens);
    kv_reserve_set(m.data(), n, p.max_new_tokens);
    if (!grp_pos_d) { grp_pos_d = (int*)dmalloc(128 * sizeof(int)); grp_x_d = (float*)dmalloc((size_t)128 * H * sizeof(float)); }
    prefix_fan_out(in, n);
    std::vector<int32_t> pos_h, map_h;
    std::vector<char> armed((size_t)n, 0);   // the forced begin arms its slot itself
    for (const BeginGroup& gr : begin_groups(BEGIN_PREFIXED, m.data(), n, begin_limits())) {
        const int i0 = gr.i0, g = gr.g, S = in[i0].S;
        if (!gr.batched) {   // one at a time: the single-slot chunk path at base P (no prefix: what slots_begin does)
            for (int k = 0; k < g; ++k) {
                const SlotInit& q = in[i0 + k];
                const int P = m[(size_t)(i0 + k)].P;
                if (q.n_prefix > 0) { slot_begin_forced(q, p, seed, ignore_eos, rep_penalty, P); armed[(size_t)(i0 + k)] = 1; }
                else if (q.prefix_id == -1) talker_prefill(q.slot, q.prompt, S, nullptr, nullptr);
                else {
                    float* x = long_rows(S);
                    Q3_HIP_CHECK(hipMemcpyAsync(x, q.prompt, (size_t)S * H * sizeof(float), hipMemcpyHostToDevice, stream));
                    prefill_rows_long(q.slot, x, S, nullptr, P);
                }
            }
            continue;
        }
        // one pass for the group: chunk attention at per-member bases, the codec head on each member's last row
        long_ws_ensure();
        pos_h.resize((size_t)g); map_h.resize((size_t)g);
        int pmax = 0;
        for (int k = 0; k < g; ++k) {
            Q3_HIP_CHECK(hipMemcpyAsync(grp_x_d + (size_t)k * S * H, in[i0 + k].prompt, (size_t)S * H * sizeof(float), hipMemcpyHostToDevice, stream));
            pos_h[(size_t)k] = m[(size_t)(i0 + k)].P; map_h[(size_t)k] = in[i0 + k].slot;
            pmax = std::max(pmax, pos_h[(size_t)k]);
        }
        Q3_HIP_CHECK(hipMemcpyAsync(grp_pos_d, pos_h.data(), (size_t)g * sizeof(int), hipMemcpyHostToDevice, stream));
        Q3_HIP_CHECK(hipMemcpyAsync(slot_map_d, map_h.data(), (size_t)g * sizeof(int), hipMemcpyHostToDevice, stream));
        {
            LongWsScope scope(*this);
            float* const hnw = lws.hn;   // not swapped
            const bool pr = run_layers(talker, grp_x_d, H, g, S, 0, grp_pos_d, pmax, talker_norm, c.rms_eps, hnw, H, slot_map_d);
            if (!pr) throw Error("batched prefill expects the MFMA path");
            head_proj(codec_head, grp_x_d, H, talker_norm, c.rms_eps, nullptr, 0, logits_g, V, g, V, H, true, true, S - 1, S);
            for (int k = 0; k < g; ++k) scatter_last_rows(logits_g + (size_t)k * V, hnw + (size_t)(k * S + S - 1) * H, in[i0 + k].slot);
        }
        for (int k = 0; k < g; ++k) {
            pos_h[(size_t)k] = begin_own(m[(size_t)(i0 + k)]);
            Q3_HIP_CHECK(hipMemcpyAsync(talker_pos_d + in[i0 + k].slot, &pos_h[(size_t)k], sizeof(int32_t), hipMemcpyHostToDevice, stream));
        }
        sync();   // pos_h / map_h are reused by the next group
    }
    for (int i = 0; i < n; ++i)
        if (!armed[(size_t)i]) arm_slot(in[i], m[(size_t)i].P, rep_penalty, p, seed, ignore_eos, true);
    sync();
}

// ------------------------------------------------------------------------------------------------
// ragged prefill (q3_engine.h)
// ------------------------------------------------------------------------------------------------
float* Engine::rag_rows(size_t rows) {
    if (rows > rag_x_rows) regrow(rag_x_d, rag_x_rows, std::max(rows, (size_t)512), c.hidden);
    return rag_x_d;
}

void Engine::seg_tables_build(const std::vector<SegMember>& members, std::vector<SegChunk>& chunks) {
    const int TQ = attn_prefill_tile_rows(talker.nq, talker.nkv), CH = prefill_chunk;
    sync();   // seg_tab_h may still be read by the previous call's upload
    seg_tab_h.clear();
    chunks.clear();
    std::vector<int32_t> seg, row_seg, tiles, last;
    auto flush = [&](SegChunk& ch) {
        ch.n_seg = (int)seg.size() / 4; ch.n_tiles = (int)tiles.size() / 2; ch.n_last = (int)last.size();
        ch.seg = seg_tab_h.size(); seg_tab_h.insert(seg_tab_h.end(), seg.begin(), seg.end());
        ch.row_seg = seg_tab_h.size(); seg_tab_h.insert(seg_tab_h.end(), row_seg.begin(), row_seg.end());
        ch.tiles = seg_tab_h.size(); seg_tab_h.insert(seg_tab_h.end(), tiles.begin(), tiles.end());
        ch.last = seg_tab_h.size(); seg_tab_h.insert(seg_tab_h.end(), last.begin(), last.end());
        chunks.push_back(ch);
        seg.clear(); row_seg.clear(); tiles.clear(); last.clear();
    };
    SegChunk cur;
    int row = 0;   // rows staged so far
    for (size_t mi = 0; mi < members.size(); ++mi) {
        const SegMember& m = members[mi];
        if (m.rows < 1 || m.base < 0 || m.slot < 0 || m.slot >= B || m.base + m.rows > kv_slot_pages(m.slot) * 64)
            throw Error("ragged prefill: a member's rows do not fit its slot's pages");
        for (int done = 0; done < m.rows;) {
            if (cur.rows == CH) { flush(cur); cur = SegChunk(); cur.row0 = row; }
            const int n = std::min(m.rows - done, CH - cur.rows), si = (int)seg.size() / 4;
            seg.push_back(m.slot); seg.push_back(m.base + done); seg.push_back(cur.rows); seg.push_back(n);
            for (int r = 0; r < n; ++r) row_seg.push_back(si);
            for (int r = 0; r < n; r += TQ) { tiles.push_back(si); tiles.push_back(r); }
            cur.rows += n; done += n; row += n;
            if (done == m.rows) { last.push_back(cur.rows - 1); cur.last_member.push_back((int)mi); }
        }
    }
    if (cur.rows > 0) flush(cur);
    if (seg_tab_h.size() > seg_tab_cap) regrow(seg_tab_d, seg_tab_cap, std::max(seg_tab_h.size(), (size_t)4096), 1, true);   // drained above
    Q3_HIP_CHECK(hipMemcpyAsync(seg_tab_d, seg_tab_h.data(), seg_tab_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
}

// run_prefill (tts_onnx.cpp:615-665) and the frame loop's talker input rows (:824-842) for many slots at once: see q3_engine.h.
void Engine::slots_begin_ragged(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos) {
    if (n < 1) return;
    if (n == 1) { slots_begin_prefixed(in, 1, p, seed, ignore_eos); return; }   // one member: exactly its one-at-a-time begin
    if (!finalized) throw Error("weights not finalized");
    const int H = c.hidden, V = c.vocab, G = c.n_groups;
    const float rep_penalty = checked_penalty(p);
    const std::vector<BeginMember> m = begin_members(BEGIN_RAGGED, in, n, p.max_new_tokens);
    const size_t total = begin_ragged_rows(m.data(), n);
    kv_reserve_set(m.data(), n, p.max_new_tokens);
    if (begin_ragged_one_at_a_time(total, begin_limits(), attn_prefill_seg_ok(talker.d, talker.nq, talker.nkv), seam_step)) {
        // each member exactly as its own begin (its pages are reserved already: that call's reservation changes nothing)
        for (int i = 0; i < n; ++i) slots_begin_prefixed(in + i, 1, p, seed, ignore_eos);
        return;
    }
    prefix_fan_out(in, n);
    // ---- the members' rows, contiguous in call order: prompt rows from the host, forced frames' rows made on the device ----
    float* const x = rag_rows(total);
    long_ws_ensure();
    if (!rag_last_x_d) { rag_last_x_d = (float*)dmalloc((size_t)128 * H * sizeof(float)); rag_last_hn_d = (float*)dmalloc((size_t)128 * H * sizeof(float)); }
    std::vector<SegMember> members((size_t)n);
    size_t r = 0;
    for (int i = 0; i < n; ++i) {
        const SlotInit& q = in[i];
        Q3_HIP_CHECK(hipMemcpyAsync(x + r * H, q.prompt, (size_t)q.S * H * sizeof(float), hipMemcpyHostToDevice, stream));
        stage_slot_inputs(q);   // in front of the launch that reads the trailing rows and sets the history's bits
        if (q.n_prefix > 0)
            frame_rows_launch(q.prefix, q.n_prefix, 0, trailing_d + (size_t)q.slot * max_trailing * H, q.n_trailing, x + (r + (size_t)q.S) * H,
                              codes_d + (size_t)q.slot * max_frames_cap * G, seen_d + (size_t)q.slot * seen_ld);
        members[(size_t)i].slot = q.slot; members[(size_t)i].base = m[(size_t)i].P; members[(size_t)i].rows = q.S + q.n_prefix;
        r += (size_t)(q.S + q.n_prefix);
    }
    std::vector<SegChunk> chunks;
    seg_tables_build(members, chunks);
    {
        LongWsScope scope(*this);
        float* const hnw = lws.hn;   // not swapped
        SegAttn sa;
        for (const SegChunk& ch : chunks) {
            sa.seg = seg_tab_d + ch.seg; sa.row_seg = seg_tab_d + ch.row_seg; sa.tiles = seg_tab_d + ch.tiles; sa.n_seg = ch.n_seg; sa.n_tiles = ch.n_tiles;
            seg_attn = &sa;
            float* xc = x + (size_t)ch.row0 * H;
            run_layers(talker, xc, H, 1, ch.rows, 0, nullptr, 0, talker_norm, c.rms_eps, hnw, H);
            ++ragged_passes;
            if (ch.n_last == 0) continue;
            // final norm + codec head on the rows that end a member: gathered by row index, then scattered to their slots
            launch_gather_rows_f32(xc, H, seg_tab_d + ch.last, ch.n_last, rag_last_x_d, H, H, stream);
            head_proj(codec_head, rag_last_x_d, H, talker_norm, c.rms_eps, rag_last_hn_d, H, logits_g, V, ch.n_last, V, H, true);
            for (int k = 0; k < ch.n_last; ++k)
                scatter_last_rows(logits_g + (size_t)k * V, rag_last_hn_d + (size_t)k * H, in[ch.last_member[(size_t)k]].slot);
        }
    }
    std::vector<int32_t> pos_h((size_t)n);
    for (int i = 0; i < n; ++i) {   // per slot what its one-at-a-time begin leaves
        pos_h[(size_t)i] = begin_own(m[(size_t)i]);
        Q3_HIP_CHECK(hipMemcpyAsync(talker_pos_d + in[i].slot, &pos_h[(size_t)i], sizeof(int32_t), hipMemcpyHostToDevice, stream));
        arm_slot(in[i], m[(size_t)i].P, rep_penalty, p, seed, ignore_eos, false);
    }
    sync();   // pos_h, the tables' host copy and the callers' rows are read by the copies above
}

} // namespace q3

