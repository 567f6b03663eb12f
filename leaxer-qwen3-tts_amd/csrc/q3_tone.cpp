// q3_tone.cpp — the tone stage: a stage takes 24 kHz float PCM that already lies on the device (the stretcher's, the
// pitch stage's, the vocoder's, or samples staged by the standalone entry) and delivers it through a cascade of 1 .. 8 biquads in
// double (q3_audio.h: tone_*; the arithmetic is fixed in include/q3tts.h).  Its coefficients are formed once on the host at begin; its
// state is two doubles per signal.  It emits what it receives, so the host rule is the identity and a finishing push flushes nothing.
// All stages of a call share one launch (launch_tone).  Reserve / launch / commit and the standalone entry are Stage's (q3_stage.cpp).
// [HINT] no counterpart in the reference, which has no equaliser.
#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

int Engine::ToneStage::begin(int n, const ToneSection* sections) {
    try { tone_check(n, sections); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    const int id = tab.free_id();
    double*& mem = tab.slots[(size_t)id].mem;
    // the history: an allocation of the stage's own, two halves, kept for the id's next stage
    if (!mem) Q3_HIP_CHECK(hipMalloc((void**)&mem, 2 * (size_t)kToneStateDoubles * sizeof(double)));
    Equaliser& S = tab.open(id);
    S.n = n;
    tone_coeffs(n, sections, S.c);
    return id;
}

void Engine::ToneStage::free_all() {
    for (Equaliser& S : tab.slots) if (S.mem) (void)hipFree(S.mem);
    tab.slots.clear();
}

int64_t Engine::ToneStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const Equaliser&, int64_t n, bool) { return n; });
}

bool Engine::ToneStage::fill(StagePush& q, size_t di, char* out, int32_t*) {
    const Equaliser& S = tab.get(q.id);
    if (q.n_new > kStageMaxSamples || q.n_out != q.n_new) throw Error("tone: push too large");
    if (!q.x_dev) throw Error("tone: a push without its samples");
    ToneDesc& d = desc_h[di];
    d.state_in = S.mem + (size_t)S.cur * kToneStateDoubles; d.state_out = S.mem + (size_t)(1 - S.cur) * kToneStateDoubles;
    d.x_new = q.x_dev; d.out = (float*)out;
    for (int j = 0; j < S.n; ++j) for (int i = 0; i < 5; ++i) d.c[j][i] = S.c[j][i];
    d.n_new = (int32_t)q.n_new; d.n_sections = S.n; d.first = S.n_in == 0 ? 1 : 0;
    return true;
}

void Engine::ToneStage::issue(size_t d0, int n_live) { launch_tone((const ToneDesc*)desc.p + d0, n_live, e.stream); }

void Engine::ToneStage::commit_one(const StagePush& q) {   // every live push flips: the history moves on
    tab.commit(q.id, q.n_new, q.n_out, q.finish, q.desc >= 0);
}

} // namespace q3
