// q3_speed.cpp — the speaking-rate stage: a stretcher takes 24 kHz float PCM that already lies on the device (the
// vocoder's, or samples staged by the standalone entry) and delivers it S / 1000 times as fast at the same pitch: WSOLA with a fixed
// synthesis hop (q3_audio.h: speed_*; the arithmetic is fixed in include/q3tts.h), whose state is the input from a_{F-1} - D on, the last
// chosen position and the frame counter.  All stretchers of a call share one launch (launch_wsola); how many samples a push delivers is
// the host rule speed_emitted and nothing else.  [HINT] no counterpart in the reference, which has no speed control.
#include <algorithm>
#include <cstring>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

static constexpr size_t kStretcherBytes = 2 * (size_t)kSpeedCarry * sizeof(float) + 2 * 2 * sizeof(int64_t);

int Engine::speed_begin(int speed) {
    try { speed_check(speed); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    if (speed == 1000) throw Error("speed: 1000 permille is no stage (the stretcher is not the identity there): open no stretcher");
    if (!speed_win_d) {
        const std::vector<float> w = speed_window();
        Q3_HIP_CHECK(hipMalloc((void**)&speed_win_d, w.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(speed_win_d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) { (void)hipFree(speed_win_d); speed_win_d = nullptr; Q3_HIP_CHECK(err); }
    }
    int id = -1;
    for (size_t i = 0; i < stretchers.size(); ++i) if (!stretchers[i].used) { id = (int)i; break; }
    if (id < 0) {
        if ((int)stretchers.size() >= kMaxStretchers) throw Error("speed: at most " + std::to_string(kMaxStretchers) + " stretchers are open at a time");
        stretchers.emplace_back();
        id = (int)stretchers.size() - 1;
    }
    Stretcher& S = stretchers[(size_t)id];
    // carry and state: an allocation of the stretcher's own, kept for the id's next stretcher
    if (!S.mem) Q3_HIP_CHECK(hipMalloc((void**)&S.mem, kStretcherBytes));
    S.used = true; S.finished = false; S.speed = speed; S.cur = 0;
    S.n_in = S.n_out = S.frames = S.carry_abs0 = 0;
    return id;
}

void Engine::speed_end(int id) {
    if (id < 0 || id >= (int)stretchers.size() || !stretchers[(size_t)id].used) throw Error("speed: no such stretcher");
    stretchers[(size_t)id].used = false;
}

void Engine::speed_free() {
    for (Stretcher& S : stretchers) if (S.mem) (void)hipFree(S.mem);
    stretchers.clear();
    if (speed_win_d) (void)hipFree(speed_win_d);
    if (speed_desc_d) (void)hipFree(speed_desc_d);
    if (speed_out_d) (void)hipFree(speed_out_d);
    if (speed_offs_d) (void)hipFree(speed_offs_d);
    if (speed_in_d) (void)hipFree(speed_in_d);
    speed_win_d = nullptr; speed_desc_d = nullptr; speed_out_d = nullptr; speed_offs_d = nullptr; speed_in_d = nullptr;
    speed_desc_cap = speed_out_cap = speed_offs_cap = speed_in_floats = 0;
}

const Engine::Stretcher& Engine::speed_get(int id) const {
    if (id < 0 || id >= (int)stretchers.size() || !stretchers[(size_t)id].used) throw Error("speed: no such stretcher");
    return stretchers[(size_t)id];
}

int64_t Engine::speed_push_len(int id, int64_t n_new, bool finish) const {
    const Stretcher& S = speed_get(id);
    if (S.finished) throw Error("speed: stretcher " + std::to_string(id) + " is finished");
    if (n_new < 0) throw Error("speed: negative sample count");
    if (S.n_in + n_new > kPcmSinkMaxSamples) throw Error("speed: stretcher " + std::to_string(id) + " would exceed one hour of 24 kHz input");
    return speed_emitted(S.speed, S.n_in + n_new, finish) - S.n_out;
}

int64_t Engine::speed_push_frames(int id, int64_t n_new, bool finish) const {
    const Stretcher& S = speed_get(id);
    (void)speed_push_len(id, n_new, finish);
    return speed_frames(S.speed, S.n_in + n_new, finish) - S.frames;
}

// A call's launches: speed_reserve once (the only place the workspaces may grow, before anything is enqueued), then one speed_launch per
// set of stretchers whose input is ready, then (after the stream has been synchronised) speed_commit for all.
void Engine::speed_reserve(int n_total, size_t out_floats_total, size_t frames_total) {
    auto grow = [&](void** p, size_t* cap, size_t want, size_t el) {
        if (*cap >= want && *p) return;
        sync();
        if (*p) (void)hipFree(*p);
        *p = nullptr; *cap = 0;
        const size_t n = std::max((size_t)64, want);
        Q3_HIP_CHECK(hipMalloc(p, n * el));
        *cap = n;
    };
    grow((void**)&speed_desc_d, &speed_desc_cap, (size_t)n_total, sizeof(SpeedDesc));
    grow((void**)&speed_out_d, &speed_out_cap, out_floats_total, sizeof(float));
    grow((void**)&speed_offs_d, &speed_offs_cap, frames_total, sizeof(int32_t));
    speed_desc_h.assign((size_t)n_total, SpeedDesc());   // never resized during the call: uploads read it until the sync
    speed_desc_used = 0; speed_out_used = 0; speed_offs_used = 0;
}

void Engine::speed_launch(SpeedPush* ps, int n) {
    const size_t d0 = speed_desc_used;
    int n_live = 0;
    for (int i = 0; i < n; ++i) {
        SpeedPush& q = ps[i];
        const Stretcher& S = speed_get(q.id);
        q.n_out = speed_push_len(q.id, q.n_new, q.finish);
        q.n_frames = speed_push_frames(q.id, q.n_new, q.finish);
        q.desc = -1; q.out_dev = speed_out_d;
        if (q.n_new == 0 && q.n_frames == 0) continue;   // an empty push: the carry stays, nothing is emitted
        if (d0 + n_live >= speed_desc_h.size()) throw Error("speed: more launches than the call reserved");
        if (q.n_new > 2147483647LL || q.n_out > 2147483647LL - 256 || q.n_frames > 2147483647LL) throw Error("speed: push too large");
        const size_t fl = speed_out_floats(q.n_out);
        if (speed_out_used + fl > speed_out_cap || speed_offs_used + (size_t)q.n_frames > speed_offs_cap) throw Error("speed: more output than the call reserved");
        SpeedDesc& d = speed_desc_h[d0 + n_live];
        float* carry = S.mem;
        int64_t* state = (int64_t*)(S.mem + 2 * (size_t)kSpeedCarry);
        d.carry_in = carry + (size_t)S.cur * kSpeedCarry; d.carry_out = carry + (size_t)(1 - S.cur) * kSpeedCarry;
        d.state_in = state + 2 * (size_t)S.cur; d.state_out = state + 2 * (size_t)(1 - S.cur);
        d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
        d.win = speed_win_d;
        d.out = speed_out_d + speed_out_used;
        d.offs = speed_offs_d + speed_offs_used;
        d.carry_abs0 = S.carry_abs0; d.n_before = S.n_in; d.n_total = S.n_in + q.n_new;
        d.frame0 = S.frames;
        d.n_new = (int32_t)q.n_new; d.n_frames = (int32_t)q.n_frames; d.n_out = (int32_t)q.n_out; d.speed = S.speed;
        // the next frame F reads nothing before a_{F-1} - D: the carry runs from there (a host rule, independent of every offset)
        const int64_t F = S.frames + q.n_frames;
        d.keep_abs0 = F >= 1 ? std::max<int64_t>(0, speed_pos(S.speed, F - 1) - kSpeedD) : 0;
        d.keep_abs0 = std::max(d.keep_abs0, S.carry_abs0);
        const int64_t keep = q.finish ? 0 : d.n_total - d.keep_abs0;
        if (keep < 0 || keep > kSpeedCarry) throw Error("speed: carry outside its buffer");
        d.keep = (int32_t)keep;
        q.out_dev = d.out;
        q.desc = (int)(d0 + n_live);
        speed_out_used += fl; speed_offs_used += (size_t)q.n_frames;
        ++n_live;
    }
    if (n_live == 0) return;
    Q3_HIP_CHECK(hipMemcpyAsync(speed_desc_d + d0, speed_desc_h.data() + d0, (size_t)n_live * sizeof(SpeedDesc), hipMemcpyHostToDevice, stream));
    launch_wsola(speed_desc_d + d0, n_live, stream);
    speed_desc_used += (size_t)n_live;
    for (int i = 0; i < n; ++i) {
        const SpeedPush& q = ps[i];
        if (q.desc < 0) continue;
        const SpeedDesc& d = speed_desc_h[(size_t)q.desc];
        const int64_t m = std::min(q.n_out, q.cap), k = std::min(q.n_frames, q.offs_cap);
        if (m > 0 && q.out_host) Q3_HIP_CHECK(hipMemcpyAsync(q.out_host, d.out, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (k > 0 && q.offs_host) Q3_HIP_CHECK(hipMemcpyAsync(q.offs_host, d.offs, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
}

void Engine::speed_commit(const SpeedPush* ps, int n) {
    for (int i = 0; i < n; ++i) {
        const SpeedPush& q = ps[i];
        Stretcher& S = stretchers[(size_t)q.id];
        if (q.desc >= 0) {
            S.cur = 1 - S.cur;
            S.carry_abs0 = speed_desc_h[(size_t)q.desc].keep_abs0;
        }
        S.n_in += q.n_new; S.n_out += q.n_out; S.frames += q.n_frames;
        if (q.finish) S.finished = true;
    }
}

// the standalone entry: its input is staged from the host
void Engine::speed_push_batch_host(int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                                   float* const* out, int64_t cap, int64_t* out_len, int32_t* const* offsets_out, int64_t* n_offsets) {
    if (n < 0) throw Error("speed push: negative stretcher count");
    if (n == 0) return;
    if (!ids || !n_in) throw Error("speed push: NULL argument");
    if (cap < 0) throw Error("speed push: negative cap_samples");
    if (n > 65535) throw Error("speed push: at most 65535 stretchers per call");
    // ---- everything is validated before any stretcher moves ----
    std::vector<SpeedPush> ps((size_t)n);
    size_t in_total = 0, out_total = 0, frames_total = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < i; ++k) if (ids[k] == ids[i]) throw Error("speed push: stretcher " + std::to_string(ids[i]) + " listed twice");
        if (n_in[i] < 0) throw Error("speed push: negative sample count");
        if (n_in[i] > kPcmSinkMaxPush) throw Error("speed push: a push holds at most " + std::to_string(kPcmSinkMaxPush) + " samples");
        if (n_in[i] > 0 && (!pcm24 || !pcm24[i])) throw Error("speed push: NULL samples");
        SpeedPush& q = ps[(size_t)i];
        q.id = ids[i]; q.n_new = n_in[i]; q.finish = finish && finish[i]; q.out_host = out ? out[i] : nullptr; q.cap = cap;
        q.offs_host = offsets_out ? offsets_out[i] : nullptr; q.offs_cap = cap / kSpeedHs + 1;
        const int64_t len = speed_push_len(q.id, q.n_new, q.finish);   // throws for an unknown / finished / full stretcher
        if (out_len) out_len[i] = 0;
        if (n_offsets) n_offsets[i] = 0;
        if (len > 0 && q.out_host == nullptr && cap > 0) throw Error("speed push: NULL output");
        in_total += ((size_t)q.n_new + 63) & ~(size_t)63;
        out_total += speed_out_floats(len);
        frames_total += (size_t)speed_push_frames(q.id, q.n_new, q.finish);
    }
    if (speed_in_floats < in_total) {
        sync();
        if (speed_in_d) (void)hipFree(speed_in_d);
        speed_in_d = nullptr; speed_in_floats = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&speed_in_d, in_total * sizeof(float)));
        speed_in_floats = in_total;
    }
    speed_reserve(n, out_total, frames_total);
    try {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            SpeedPush& q = ps[(size_t)i];
            q.x_dev = speed_in_d + off;
            if (q.n_new > 0) Q3_HIP_CHECK(hipMemcpyAsync(speed_in_d + off, pcm24[i], (size_t)q.n_new * sizeof(float), hipMemcpyHostToDevice, stream));
            off += ((size_t)q.n_new + 63) & ~(size_t)63;
        }
        speed_launch(ps.data(), n);
        sync();
    } catch (...) { try { sync(); } catch (...) { } throw; }   // the callers' buffers must outlive the copies
    speed_commit(ps.data(), n);
    for (int i = 0; i < n; ++i) {
        if (out_len) out_len[i] = ps[(size_t)i].n_out;
        if (n_offsets) n_offsets[i] = ps[(size_t)i].n_frames;
    }
}

} // namespace q3
