// q3_level.cpp — the output-level stage: a stage takes 24 kHz float PCM that already lies on the device (the vocoder's,
// a stretcher's, or samples staged by the standalone entry) and delivers it g times as loud, behind a look-ahead limiter when it has a
// ceiling (q3_audio.h: level_*; the arithmetic is fixed in include/q3tts.h).  A limiter's state is the last 254 values of v = g x and
// its counters.  All stages of a call share one launch (launch_level); how many samples a push delivers is the host rule
// level_emitted and nothing else.  [HINT] no counterpart in the reference, which has no volume control and clips.
#include <algorithm>
#include <cstring>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

static constexpr size_t kLevelerBytes = 2 * (size_t)kLevelCarry * sizeof(float);

int Engine::level_begin(int gain_cb, int ceiling) {
    try { level_check(gain_cb, ceiling); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    if (gain_cb == 0 && ceiling == 0) throw Error("level: gain 0 centibels without a ceiling is no stage: open no level stage");
    int id = -1;
    for (size_t i = 0; i < levelers.size(); ++i) if (!levelers[i].used) { id = (int)i; break; }
    if (id < 0) {
        if ((int)levelers.size() >= kMaxLevelers) throw Error("level: at most " + std::to_string(kMaxLevelers) + " level stages are open at a time");
        levelers.emplace_back();
        id = (int)levelers.size() - 1;
    }
    Leveler& S = levelers[(size_t)id];
    // a limiter's carry: an allocation of the stage's own, kept for the id's next stage
    if (ceiling > 0 && !S.mem) Q3_HIP_CHECK(hipMalloc((void**)&S.mem, kLevelerBytes));
    S.used = true; S.finished = false; S.gain_cb = gain_cb; S.ceiling = ceiling; S.cur = 0;
    S.n_in = S.n_out = 0;
    return id;
}

void Engine::level_end(int id) {
    if (id < 0 || id >= (int)levelers.size() || !levelers[(size_t)id].used) throw Error("level: no such level stage");
    levelers[(size_t)id].used = false;
}

void Engine::level_free() {
    for (Leveler& S : levelers) if (S.mem) (void)hipFree(S.mem);
    levelers.clear();
    if (level_desc_d) (void)hipFree(level_desc_d);
    if (level_out_d) (void)hipFree(level_out_d);
    if (level_in_d) (void)hipFree(level_in_d);
    level_desc_d = nullptr; level_out_d = nullptr; level_in_d = nullptr;
    level_desc_cap = level_out_cap = level_in_floats = 0;
}

const Engine::Leveler& Engine::level_get(int id) const {
    if (id < 0 || id >= (int)levelers.size() || !levelers[(size_t)id].used) throw Error("level: no such level stage");
    return levelers[(size_t)id];
}

int64_t Engine::level_push_len(int id, int64_t n_new, bool finish) const {
    const Leveler& S = level_get(id);
    if (S.finished) throw Error("level: level stage " + std::to_string(id) + " is finished");
    if (n_new < 0) throw Error("level: negative sample count");
    if (S.n_in + n_new > kPcmSinkMaxSamples) throw Error("level: level stage " + std::to_string(id) + " would exceed one hour of 24 kHz input");
    return level_emitted(S.ceiling, S.n_in + n_new, finish) - S.n_out;
}

// A call's launches: level_reserve once (the only place the workspaces may grow, before anything is enqueued), then one level_launch
// per set of stages whose input is ready, then (after the stream has been synchronised) level_commit for all.
void Engine::level_reserve(int n_total, size_t out_floats_total) {
    auto grow = [&](void** p, size_t* cap, size_t want, size_t el) {
        if (*cap >= want && *p) return;
        sync();
        if (*p) (void)hipFree(*p);
        *p = nullptr; *cap = 0;
        const size_t n = std::max((size_t)64, want);
        Q3_HIP_CHECK(hipMalloc(p, n * el));
        *cap = n;
    };
    grow((void**)&level_desc_d, &level_desc_cap, (size_t)n_total, sizeof(LevelDesc));
    grow((void**)&level_out_d, &level_out_cap, out_floats_total, sizeof(float));
    level_desc_h.assign((size_t)n_total, LevelDesc());   // never resized during the call: uploads read it until the sync
    level_desc_used = 0; level_out_used = 0;
}

void Engine::level_launch(LevelPush* ps, int n) {
    const size_t d0 = level_desc_used;
    int n_live = 0, max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        LevelPush& q = ps[i];
        const Leveler& S = level_get(q.id);
        q.n_out = level_push_len(q.id, q.n_new, q.finish);
        q.desc = -1; q.out_dev = level_out_d;
        if (q.n_new == 0 && q.n_out == 0) continue;   // an empty push: the carry stays, nothing is emitted
        if (d0 + n_live >= level_desc_h.size()) throw Error("level: more launches than the call reserved");
        if (q.n_new > 2147483647LL - 2 * kLevelTile || q.n_out > 2147483647LL - 2 * kLevelTile) throw Error("level: push too large");
        const size_t fl = level_out_floats(q.n_out);
        if (level_out_used + fl > level_out_cap) throw Error("level: more output than the call reserved");
        LevelDesc& d = level_desc_h[d0 + n_live];
        d.limit = S.ceiling > 0 ? 1 : 0;
        d.g = level_gain(S.gain_cb); d.T = d.limit ? level_ceiling(S.ceiling) : 1.0f;
        if (d.limit) {
            d.carry_in = S.mem + (size_t)S.cur * kLevelCarry; d.carry_out = S.mem + (size_t)(1 - S.cur) * kLevelCarry;
            d.keep = q.finish ? 0 : kLevelCarry;
        }
        d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
        if (!d.x_new) throw Error("level: a push without its samples");
        d.out = level_out_d + level_out_used;
        d.n_before = S.n_in; d.n_total = S.n_in + q.n_new; d.out0 = S.n_out;
        d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out;
        max_tiles = std::max(max_tiles, level_tiles(q.n_out));
        q.out_dev = d.out;
        q.desc = (int)(d0 + n_live);
        level_out_used += fl;
        ++n_live;
    }
    if (n_live == 0) return;
    Q3_HIP_CHECK(hipMemcpyAsync(level_desc_d + d0, level_desc_h.data() + d0, (size_t)n_live * sizeof(LevelDesc), hipMemcpyHostToDevice, stream));
    launch_level(level_desc_d + d0, n_live, max_tiles, stream);
    level_desc_used += (size_t)n_live;
    for (int i = 0; i < n; ++i) {
        const LevelPush& q = ps[i];
        if (q.desc < 0) continue;
        const int64_t m = std::min(q.n_out, q.cap);
        if (m > 0 && q.out_host) Q3_HIP_CHECK(hipMemcpyAsync(q.out_host, level_desc_h[(size_t)q.desc].out, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
}

void Engine::level_commit(const LevelPush* ps, int n) {
    for (int i = 0; i < n; ++i) {
        const LevelPush& q = ps[i];
        Leveler& S = levelers[(size_t)q.id];
        if (q.desc >= 0 && level_desc_h[(size_t)q.desc].keep > 0) S.cur = 1 - S.cur;
        S.n_in += q.n_new; S.n_out += q.n_out;
        if (q.finish) S.finished = true;
    }
}

// the standalone entry: its input is staged from the host
void Engine::level_push_batch_host(int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                                   float* const* out, int64_t cap, int64_t* out_len) {
    if (n < 0) throw Error("level push: negative stage count");
    if (n == 0) return;
    if (!ids || !n_in) throw Error("level push: NULL argument");
    if (cap < 0) throw Error("level push: negative cap_samples");
    if (n > 65535) throw Error("level push: at most 65535 level stages per call");
    // ---- everything is validated before any stage moves ----
    std::vector<LevelPush> ps((size_t)n);
    size_t in_total = 0, out_total = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < i; ++k) if (ids[k] == ids[i]) throw Error("level push: level stage " + std::to_string(ids[i]) + " listed twice");
        if (n_in[i] < 0) throw Error("level push: negative sample count");
        if (n_in[i] > kPcmSinkMaxPush) throw Error("level push: a push holds at most " + std::to_string(kPcmSinkMaxPush) + " samples");
        if (n_in[i] > 0 && (!pcm24 || !pcm24[i])) throw Error("level push: NULL samples");
        LevelPush& q = ps[(size_t)i];
        q.id = ids[i]; q.n_new = n_in[i]; q.finish = finish && finish[i]; q.out_host = out ? out[i] : nullptr; q.cap = cap;
        const int64_t len = level_push_len(q.id, q.n_new, q.finish);   // throws for an unknown / finished / full stage
        if (out_len) out_len[i] = 0;
        if (len > 0 && q.out_host == nullptr && cap > 0) throw Error("level push: NULL output");
        in_total += ((size_t)q.n_new + 63) & ~(size_t)63;
        out_total += level_out_floats(len);
    }
    if (level_in_floats < in_total) {
        sync();
        if (level_in_d) (void)hipFree(level_in_d);
        level_in_d = nullptr; level_in_floats = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&level_in_d, in_total * sizeof(float)));
        level_in_floats = in_total;
    }
    level_reserve(n, out_total);
    try {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            LevelPush& q = ps[(size_t)i];
            q.x_dev = level_in_d + off;
            if (q.n_new > 0) Q3_HIP_CHECK(hipMemcpyAsync(level_in_d + off, pcm24[i], (size_t)q.n_new * sizeof(float), hipMemcpyHostToDevice, stream));
            off += ((size_t)q.n_new + 63) & ~(size_t)63;
        }
        level_launch(ps.data(), n);
        sync();
    } catch (...) { try { sync(); } catch (...) { } throw; }   // the callers' buffers must outlive the copies
    level_commit(ps.data(), n);
    for (int i = 0; i < n; ++i) if (out_len) out_len[i] = ps[(size_t)i].n_out;
}

} // namespace q3
