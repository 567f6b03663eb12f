// q3_stage.cpp — what the carried-state stages behind the vocoder share on the device side: the grow-only workspaces
// of a call, the launch loop over a set of pushes and the standalone entry that stages its input from the host.  What a kind supplies
// (descriptor fill, launch, commit rule, begin) is in q3_pitch.cpp, q3_speed.cpp, q3_tone.cpp, q3_loudness.cpp, q3_level.cpp and q3_pcm_sink.cpp; the host-side table in q3_stage.h.
#include <algorithm>
#include <vector>

#include "q3_engine.h"

namespace q3 {

void Engine::ws_grow(DevBuf& b, size_t want, size_t el) {
    if (b.cap >= want && b.p) return;
    sync();
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t n = std::max((size_t)64, want);
    Q3_HIP_CHECK(hipMalloc((void**)&b.p, n * el));
    b.cap = n;
}

void Engine::Stage::ws_free() {
    for (DevBuf* b : { &desc, &out, &in, &offs }) { if (b->p) (void)hipFree(b->p); *b = DevBuf(); }
}

size_t Engine::Stage::plan(StagePush& q) const {
    q.n_out = push_len(q.id, q.n_new, q.finish);
    (void)idle(q);
    return padded((size_t)q.n_out * out_el(q.id));
}

void Engine::Stage::reserve(int n_total, size_t out_bytes_total, size_t offs_total) {
    e.ws_grow(desc, (size_t)n_total, desc_size());
    e.ws_grow(out, out_bytes_total, 1);
    if (has_offs) e.ws_grow(offs, offs_total, sizeof(int32_t));
    desc_reset((size_t)n_total);
    desc_n = (size_t)n_total; desc_used = out_used = offs_used = 0;
}

void Engine::Stage::launch(StagePush* ps, int n) {
    const size_t d0 = desc_used;
    int n_live = 0;
    for (int i = 0; i < n; ++i) {
        StagePush& q = ps[i];
        q.n_out = push_len(q.id, q.n_new, q.finish);
        q.desc = -1; q.out_dev = (const float*)out.p; q.offs_dev = nullptr;
        if (idle(q)) continue;
        if (d0 + n_live >= desc_n) throw Error(std::string(name) + ": more launches than the call reserved");
        const size_t bytes = padded((size_t)q.n_out * out_el(q.id));
        if (out_used + bytes > out.cap || offs_used + (size_t)q.n_frames > offs.cap) throw Error(std::string(name) + ": more output than the call reserved");
        if (!fill(q, d0 + n_live, out.p + out_used, (int32_t*)offs.p + offs_used)) continue;
        q.out_dev = (const float*)(out.p + out_used); q.offs_dev = (const int32_t*)offs.p + offs_used;
        q.desc = (int)(d0 + n_live);
        out_used += bytes; offs_used += (size_t)q.n_frames;
        ++n_live;
    }
    if (n_live == 0) return;
    Q3_HIP_CHECK(hipMemcpyAsync(desc.p + d0 * desc_size(), desc_at(d0), (size_t)n_live * desc_size(), hipMemcpyHostToDevice, e.stream));
    issue(d0, n_live);
    desc_used += (size_t)n_live;
    for (int i = 0; i < n; ++i) {
        const StagePush& q = ps[i];
        if (q.desc < 0) continue;
        const int64_t m = std::min(q.n_out, q.cap), k = std::min(q.n_frames, q.offs_cap);
        if (m > 0 && q.out_host) Q3_HIP_CHECK(hipMemcpyAsync(q.out_host, q.out_dev, (size_t)m * out_el(q.id), hipMemcpyDeviceToHost, e.stream));
        if (k > 0 && q.offs_host) Q3_HIP_CHECK(hipMemcpyAsync(q.offs_host, q.offs_dev, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
    }
}

// the standalone entry: its input is staged from the host
void Engine::Stage::push_batch_host(int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                                    void* const* out_host, int64_t cap, int64_t* out_len, int32_t* const* offsets_out, int64_t* n_offsets) {
    const std::string who = std::string(name) + " push: ";
    if (n < 0) throw Error(who + "negative " + count_noun + " count");
    if (n == 0) return;
    if (!ids || !n_in) throw Error(who + "NULL argument");
    if (cap < 0) throw Error(who + "negative cap_samples");
    if (n > 65535) throw Error(who + "at most 65535 " + noun + "s per call");
    // ---- everything is validated before any stage moves ----
    std::vector<StagePush> ps((size_t)n);
    size_t in_total = 0, out_total = 0, offs_total = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < i; ++k) if (ids[k] == ids[i]) throw Error(who + noun + " " + std::to_string(ids[i]) + " listed twice");
        if (n_in[i] < 0) throw Error(who + "negative sample count");
        if (n_in[i] > kStageMaxPush) throw Error(who + "a push holds at most " + std::to_string(kStageMaxPush) + " samples");
        if (n_in[i] > 0 && (!pcm24 || !pcm24[i])) throw Error(who + "NULL samples");
        StagePush& q = ps[(size_t)i];
        q.id = ids[i]; q.n_new = n_in[i]; q.finish = finish && finish[i]; q.out_host = out_host ? out_host[i] : nullptr; q.cap = cap;
        q.offs_host = offsets_out ? offsets_out[i] : nullptr; q.offs_cap = cap / kSpeedHs + 1;
        out_total += plan(q);   // throws for an unknown / finished / full stage
        if (out_len) out_len[i] = 0;
        if (n_offsets) n_offsets[i] = 0;
        if (q.n_out > 0 && q.out_host == nullptr && cap > 0) throw Error(who + "NULL output");
        in_total += ((size_t)q.n_new + 63) & ~(size_t)63;
        offs_total += (size_t)q.n_frames;
    }
    e.ws_grow(in, in_total, sizeof(float));
    reserve(n, out_total, offs_total);
    try {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            StagePush& q = ps[(size_t)i];
            q.x_dev = (const float*)in.p + off;
            if (q.n_new > 0) Q3_HIP_CHECK(hipMemcpyAsync((float*)in.p + off, pcm24[i], (size_t)q.n_new * sizeof(float), hipMemcpyHostToDevice, e.stream));
            off += ((size_t)q.n_new + 63) & ~(size_t)63;
        }
        launch(ps.data(), n);
        e.sync();
    } catch (...) { try { e.sync(); } catch (...) { } throw; }   // the callers' buffers must outlive the copies
    commit(ps.data(), n);
    for (int i = 0; i < n; ++i) {
        if (out_len) out_len[i] = ps[(size_t)i].n_out;
        if (n_offsets) n_offsets[i] = ps[(size_t)i].n_frames;
    }
}

} // namespace q3
