// q3_level.cpp — the output-level stage: a stage takes 24 kHz float PCM that already lies on the device (the vocoder's,
// a stretcher's, or samples staged by the standalone entry) and delivers it g times as loud, behind a look-ahead limiter when it has a
// ceiling (q3_audio.h: level_*; the arithmetic is fixed in include/q3tts.h).  A limiter's state is the last 254 values of v = g x and
// its counters.  All stages of a call share one launch (launch_level); how many samples a push delivers is the host rule
// level_emitted and nothing else.  Reserve / launch / commit and the standalone entry are Stage's (q3_stage.cpp).
// [HINT] no counterpart in the reference, which has no volume control and clips.
#include <algorithm>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

static constexpr size_t kLevelerBytes = 2 * (size_t)kLevelCarry * sizeof(float);

int Engine::LevelStage::begin(int gain_cb, int ceiling) {
    try { level_check(gain_cb, ceiling); } catch (const std::invalid_argument& ex) { throw Error(ex.what()); }
    if (gain_cb == 0 && ceiling == 0) throw Error("level: gain 0 centibels without a ceiling is no stage: open no level stage");
    const int id = tab.free_id();
    float*& mem = tab.slots[(size_t)id].mem;
    // a limiter's carry: an allocation of the stage's own, kept for the id's next stage
    if (ceiling > 0 && !mem) Q3_HIP_CHECK(hipMalloc((void**)&mem, kLevelerBytes));
    Leveler& S = tab.open(id);
    S.gain_cb = gain_cb; S.ceiling = ceiling;
    return id;
}

void Engine::LevelStage::free_all() {
    for (Leveler& S : tab.slots) if (S.mem) (void)hipFree(S.mem);
    tab.slots.clear();
}

int64_t Engine::LevelStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const Leveler& S, int64_t n, bool f) { return level_emitted(S.ceiling, n, f); });
}

bool Engine::LevelStage::fill(StagePush& q, size_t di, char* out, int32_t*) {
    const Leveler& S = tab.get(q.id);
    if (q.n_new > 2147483647LL - 2 * kLevelTile || q.n_out > 2147483647LL - 2 * kLevelTile) throw Error("level: push too large");
    LevelDesc& d = desc_h[di];
    d.limit = S.ceiling > 0 ? 1 : 0;
    d.g = level_gain(S.gain_cb); d.T = d.limit ? level_ceiling(S.ceiling) : 1.0f;
    if (d.limit) {
        d.carry_in = S.mem + (size_t)S.cur * kLevelCarry; d.carry_out = S.mem + (size_t)(1 - S.cur) * kLevelCarry;
        d.keep = q.finish ? 0 : kLevelCarry;
    }
    d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
    if (!d.x_new) throw Error("level: a push without its samples");
    d.out = (float*)out;
    d.n_before = S.n_in; d.n_total = S.n_in + q.n_new; d.out0 = S.n_out;
    d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out;
    return true;
}

void Engine::LevelStage::issue(size_t d0, int n_live) {
    int max_tiles = 1;
    for (int i = 0; i < n_live; ++i) max_tiles = std::max(max_tiles, level_tiles(desc_h[d0 + (size_t)i].n_out));
    launch_level((const LevelDesc*)desc.p + d0, n_live, max_tiles, e.stream);
}

void Engine::LevelStage::commit_one(const StagePush& q) {   // a limiter that goes on flips its carry; a gain-only stage has none
    tab.commit(q.id, q.n_new, q.n_out, q.finish, q.desc >= 0 && desc_h[(size_t)q.desc].keep > 0);
}

} // namespace q3
