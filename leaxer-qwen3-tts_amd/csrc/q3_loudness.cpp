// q3_loudness.cpp — the loudness stage: a stage takes 24 kHz float PCM that already lies on the device (the stretcher's,
// the vocoder's, or samples staged by the standalone entry), measures it as BS.1770 does — K-weighting in double, an exact integer
// energy per 100 ms sub-block, the absolute gate over windows of four — and delivers it with a gain that moves towards the target by at
// most 1 dB per sub-block (q3_audio.h: loudness_*; the arithmetic is fixed in include/q3tts.h).  Its state is the filters' history, the
// last three energies and the open sub-block's sum, the gated sum and count, the gain, and the open sub-block's input.  All stages of
// a call share one launch (launch_loudness); how many samples a push delivers is the host rule loudness_emitted and nothing else.  A
// push reports the sub-blocks it closed through the skeleton's per-frame words (four per sub-block: E, G, one unused).  Reserve / launch
// / commit and the standalone entry are Stage's (q3_stage.cpp).  [HINT] no counterpart in the reference, which has no loudness control.
#include <cmath>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

int Engine::LoudStage::begin(int target, int range, int start) {
    try { loudness_check(target, range, start); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    const int id = tab.free_id();
    char*& mem = tab.slots[(size_t)id].mem;
    // state and carry: an allocation of the stage's own, kept for the id's next stage
    if (!mem) Q3_HIP_CHECK(hipMalloc((void**)&mem, 2 * kLoudHalfBytes));
    Normaliser& S = tab.open(id);
    S.target = target;
    S.pt = target == 0 ? 0.0 : std::pow(10.0, ((double)target / 10.0 + 0.691) / 10.0);
    S.r_hi = std::pow(10.0, (double)range / 200.0);
    S.r_lo = 1.0 / S.r_hi;
    S.g_start = (float)std::pow(10.0, (double)start / 200.0);
    return id;
}

void Engine::LoudStage::free_all() {
    for (Normaliser& S : tab.slots) if (S.mem) (void)hipFree(S.mem);
    tab.slots.clear();
}

int64_t Engine::LoudStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const Normaliser& S, int64_t n, bool f) { return loudness_emitted(S.target, n, f); });
}

bool Engine::LoudStage::idle(StagePush& q) const {
    const Normaliser& S = tab.get(q.id);
    q.n_frames = 4 * ((S.n_in + q.n_new) / kLoudBlock - S.n_in / kLoudBlock);
    q.offs_cap = q.n_frames;   // whoever asks for the report holds room for every sub-block of the push (q3tts_loudness_push_batch_host)
    return q.n_new == 0 && q.n_out == 0;
}

bool Engine::LoudStage::fill(StagePush& q, size_t di, char* out, int32_t* offs) {
    const Normaliser& S = tab.get(q.id);
    if (q.n_new > 2147483647LL || q.n_out > 2147483647LL) throw Error("loudness: push too large");
    LoudDesc& d = desc_h[di];
    d.half_in = S.mem + (size_t)S.cur * kLoudHalfBytes; d.half_out = S.mem + (size_t)(1 - S.cur) * kLoudHalfBytes;
    d.x_new = q.n_new > 0 ? q.x_dev : (const float*)(d.half_in + (size_t)kLoudStateWords * 8);
    if (!d.x_new) throw Error("loudness: a push without its samples");
    d.out = (float*)out;
    const int64_t nb = q.n_frames / 4;
    d.energies = (int64_t*)offs; d.gains = (float*)(offs + 2 * nb);
    for (int i = 0; i < 10; ++i) d.c[i] = coeffs[i];
    d.pt = S.pt; d.r_lo = S.r_lo; d.r_hi = S.r_hi; d.g_start = S.g_start;
    d.n_before = S.n_in; d.n_total = S.n_in + q.n_new;
    d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out; d.n_blocks = (int32_t)nb;
    d.meter = S.target == 0 ? 1 : 0; d.finish = q.finish ? 1 : 0; d.first = S.n_in == 0 ? 1 : 0;
    return true;
}

void Engine::LoudStage::issue(size_t d0, int n_live) { launch_loudness((const LoudDesc*)desc.p + d0, n_live, e.stream); }

void Engine::LoudStage::commit_one(const StagePush& q) {   // every live push flips: the state moves with the carry
    tab.commit(q.id, q.n_new, q.n_out, q.finish, q.desc >= 0);
}

} // namespace q3
