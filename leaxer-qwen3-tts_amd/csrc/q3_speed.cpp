// q3_speed.cpp — the speaking-rate stage: a stretcher takes 24 kHz float PCM that already lies on the device (the
// vocoder's, or samples staged by the standalone entry) and delivers it S / 1000 times as fast at the same pitch: WSOLA with a fixed
// synthesis hop (q3_audio.h: speed_*; the arithmetic is fixed in include/q3tts.h), whose state is the input from a_{F-1} - D on, the last
// chosen position and the frame counter.  All stretchers of a call share one launch (launch_wsola); how many samples a push delivers is
// the host rule speed_emitted and nothing else.  Reserve / launch / commit and the standalone entry are Stage's (q3_stage.cpp).
// [HINT] no counterpart in the reference, which has no speed control.
#include <algorithm>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

static constexpr size_t kStretcherBytes = 2 * (size_t)kSpeedCarry * sizeof(float) + 2 * 2 * sizeof(int64_t);

int Engine::SpeedStage::begin(int speed) {
    try { speed_check(speed); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    if (speed == 1000) throw Error("speed: 1000 permille is no stage (the stretcher is not the identity there): open no stretcher");
    if (!win_d) {
        const std::vector<float> w = speed_window();
        Q3_HIP_CHECK(hipMalloc((void**)&win_d, w.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(win_d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) { (void)hipFree(win_d); win_d = nullptr; Q3_HIP_CHECK(err); }
    }
    const int id = tab.free_id();
    float*& mem = tab.slots[(size_t)id].mem;
    // carry and state: an allocation of the stretcher's own, kept for the id's next stretcher
    if (!mem) Q3_HIP_CHECK(hipMalloc((void**)&mem, kStretcherBytes));
    Stretcher& S = tab.open(id);
    S.speed = speed; S.frames = S.carry_abs0 = 0;
    return id;
}

void Engine::SpeedStage::free_all() {
    for (Stretcher& S : tab.slots) if (S.mem) (void)hipFree(S.mem);
    tab.slots.clear();
    if (win_d) (void)hipFree(win_d);
    win_d = nullptr;
}

int64_t Engine::SpeedStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const Stretcher& S, int64_t n, bool f) { return speed_emitted(S.speed, n, f); });
}

bool Engine::SpeedStage::idle(StagePush& q) const {
    const Stretcher& S = tab.get(q.id);
    q.n_frames = speed_frames(S.speed, S.n_in + q.n_new, q.finish) - S.frames;
    return q.n_new == 0 && q.n_frames == 0;
}

bool Engine::SpeedStage::fill(StagePush& q, size_t di, char* out, int32_t* offs) {
    const Stretcher& S = tab.get(q.id);
    if (q.n_new > 2147483647LL || q.n_out > 2147483647LL - 256 || q.n_frames > 2147483647LL) throw Error("speed: push too large");
    SpeedDesc& d = desc_h[di];
    float* carry = S.mem;
    int64_t* state = (int64_t*)(S.mem + 2 * (size_t)kSpeedCarry);
    d.carry_in = carry + (size_t)S.cur * kSpeedCarry; d.carry_out = carry + (size_t)(1 - S.cur) * kSpeedCarry;
    d.state_in = state + 2 * (size_t)S.cur; d.state_out = state + 2 * (size_t)(1 - S.cur);
    d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
    d.win = win_d;
    d.out = (float*)out;
    d.offs = offs;
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
    return true;
}

void Engine::SpeedStage::issue(size_t d0, int n_live) { launch_wsola((const SpeedDesc*)desc.p + d0, n_live, e.stream); }

void Engine::SpeedStage::commit_one(const StagePush& q) {   // every live push flips: the state half moves with the carry
    Stretcher& S = tab.slots[(size_t)q.id];
    if (q.desc >= 0) S.carry_abs0 = desc_h[(size_t)q.desc].keep_abs0;
    S.frames += q.n_frames;
    tab.commit(q.id, q.n_new, q.n_out, q.finish, q.desc >= 0);
}

} // namespace q3
