// q3_pitch.cpp — the pitch stage: a stage takes 24 kHz float PCM that already lies on the device (the vocoder's, or
// samples staged by the standalone entry) and delivers the same audio at the same length with the fundamental multiplied by r / 1000:
// TD-PSOLA (q3_audio.h: pitch_*; the arithmetic is fixed in include/q3tts.h), whose state is the last kPitchCarry input samples, the two
// output accumulators beyond the last emitted sample and the mark state.  All stages of a call share one launch (launch_psola); how
// many samples a push delivers is the host rule pitch_emitted and nothing else.  Reserve / launch / commit and the standalone entry are
// Stage's (q3_stage.cpp).  [HINT] no counterpart in the reference, which has no pitch control.
#include <algorithm>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

static constexpr size_t kShifterBytes = 2 * (size_t)kPitchHalfFloats * sizeof(float);

int Engine::PitchStage::begin(int ratio) {
    try { pitch_check(ratio); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    if (ratio == 1000) throw Error("pitch: 1000 permille is no stage (the shifter is not the identity there): open no pitch stage");
    if (!win_d) {
        const std::vector<float> w = pitch_windows();
        Q3_HIP_CHECK(hipMalloc((void**)&win_d, w.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(win_d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) { (void)hipFree(win_d); win_d = nullptr; Q3_HIP_CHECK(err); }
    }
    const int id = tab.free_id();
    float*& mem = tab.slots[(size_t)id].mem;
    // carry, accumulators and state: an allocation of the stage's own, kept for the id's next stage
    if (!mem) Q3_HIP_CHECK(hipMalloc((void**)&mem, kShifterBytes));
    Shifter& S = tab.open(id);
    S.ratio = ratio; S.carry_abs0 = 0;
    return id;
}

void Engine::PitchStage::free_all() {
    for (Shifter& S : tab.slots) if (S.mem) (void)hipFree(S.mem);
    tab.slots.clear();
    if (win_d) (void)hipFree(win_d);
    win_d = nullptr;
}

int64_t Engine::PitchStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const Shifter&, int64_t n, bool f) { return pitch_emitted(n, f); });
}

bool Engine::PitchStage::fill(StagePush& q, size_t di, char* out, int32_t*) {
    const Shifter& S = tab.get(q.id);
    if (q.n_new > 2147483647LL || q.n_out > 2147483647LL) throw Error("pitch: push too large");
    PitchDesc& d = desc_h[di];
    d.half_in = S.mem + (size_t)S.cur * kPitchHalfFloats; d.half_out = S.mem + (size_t)(1 - S.cur) * kPitchHalfFloats;
    d.x_new = q.n_new > 0 ? q.x_dev : d.half_in;
    if (!d.x_new) throw Error("pitch: a push without its samples");
    d.win = win_d;
    d.out = (float*)out;
    d.carry_abs0 = S.carry_abs0; d.n_before = S.n_in; d.n_total = S.n_in + q.n_new; d.out0 = S.n_out;
    d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out; d.ratio = S.ratio; d.finish = q.finish ? 1 : 0; d.first = S.n_in == 0 ? 1 : 0;
    // nothing a later mark reads lies more than kPitchCarry samples back (a host rule, independent of every period)
    d.keep_abs0 = std::max(S.carry_abs0, d.n_total - kPitchCarry);
    const int64_t keep = q.finish ? 0 : d.n_total - d.keep_abs0;
    if (keep < 0 || keep > kPitchCarry || S.n_in - S.carry_abs0 < 0 || S.n_in - S.carry_abs0 > kPitchCarry) throw Error("pitch: carry outside its buffer");
    d.keep = (int32_t)keep;
    return true;
}

void Engine::PitchStage::issue(size_t d0, int n_live) { launch_psola((const PitchDesc*)desc.p + d0, n_live, e.stream); }

void Engine::PitchStage::commit_one(const StagePush& q) {   // every live push flips: accumulators and state move with the carry
    Shifter& S = tab.slots[(size_t)q.id];
    if (q.desc >= 0) S.carry_abs0 = desc_h[(size_t)q.desc].keep_abs0;
    tab.commit(q.id, q.n_new, q.n_out, q.finish, q.desc >= 0);
}

} // namespace q3
