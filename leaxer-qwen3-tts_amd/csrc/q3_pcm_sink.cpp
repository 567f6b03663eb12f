// q3_pcm_sink.cpp — PCM sinks: the output side's mirror of the encoder streams' resampler (4k).  A sink takes 24 kHz
// float PCM that already lies on the device (the vocoder's, or samples staged by the standalone entry) and delivers it at its own rate
// (4 000 .. 192 000 Hz) as float, int16 or G.711 bytes: a windowed-sinc polyphase resampler (q3_audio.h: sink_plan) whose state is the last
// 2 * half + ceil(M / L) input samples.  All sinks of a call share one launch (launch_pcm_sinks); how many samples a push delivers
// is the host rule sink_emitted and nothing else.  Reserve / launch / commit and the standalone entry are Stage's (q3_stage.cpp).
// [HINT] no counterpart in the reference, which writes 24 kHz only (main.cpp).
#include <algorithm>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

const Engine::SinkPlanDev& Engine::SinkStage::plan_for(int rate) {
    auto it = plans.find(rate);
    if (it != plans.end()) return it->second;
    SinkPlanDev pd;
    pd.plan = sink_plan(rate);   // throws, naming the rate, before anything is allocated
    if (!pd.plan.table.empty()) {
        Q3_HIP_CHECK(hipMalloc((void**)&pd.tab_d, pd.plan.table.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(pd.tab_d, pd.plan.table.data(), pd.plan.table.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) { (void)hipFree(pd.tab_d); Q3_HIP_CHECK(err); }
    }
    return plans.emplace(rate, std::move(pd)).first->second;
}

int Engine::SinkStage::begin(int rate, int format) {
    if (!pcm_format_known(format)) throw Error("pcm sink: format " + std::to_string(format) + " is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16, nor Q3TTS_PCM_MULAW (2) or Q3TTS_PCM_ALAW (3)");
    const SinkPlanDev& pd = plan_for(rate);
    const int id = tab.free_id();
    float*& carry = tab.slots[(size_t)id].carry;
    // the carry: two buffers of kPcmSinkCarry floats in an allocation of the sink's own, kept for the id's next sink
    if (!carry) Q3_HIP_CHECK(hipMalloc((void**)&carry, 2 * (size_t)kPcmSinkCarry * sizeof(float)));
    if (sink_carry(pd.plan) > kPcmSinkCarry) throw Error("pcm sink: carry larger than its buffer");
    PcmSink& S = tab.open(id);
    S.rate = rate; S.format = format; S.plan = &pd; S.carry_abs0 = 0;
    return id;
}

void Engine::SinkStage::free_all() {
    for (PcmSink& S : tab.slots) if (S.carry) (void)hipFree(S.carry);
    tab.slots.clear();
    for (auto& kv : plans) if (kv.second.tab_d) (void)hipFree(kv.second.tab_d);
    plans.clear();
}

int64_t Engine::SinkStage::push_len(int id, int64_t n_new, bool finish) const {
    return tab.push_len(id, n_new, finish, [](const PcmSink& S, int64_t n, bool f) { return sink_emitted(S.plan->plan, n, f); });
}

bool Engine::SinkStage::fill(StagePush& q, size_t di, char* out, int32_t*) {
    const PcmSink& S = tab.get(q.id);
    const SinkPlan& P = S.plan->plan;
    PcmSinkDesc& d = desc_h[di];
    d.carry_in = S.carry + (size_t)S.cur * kPcmSinkCarry; d.carry_out = S.carry + (size_t)(1 - S.cur) * kPcmSinkCarry;
    d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
    d.tab = S.plan->tab_d;
    d.out = out;
    d.carry_abs0 = S.carry_abs0; d.n_before = S.n_in; d.n_total = S.n_in + q.n_new; d.out0 = S.n_out;
    if (q.n_new > 2147483647LL || q.n_out > 2147483647LL - 256) throw Error("pcm sink: push too large");
    d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out;
    d.keep = q.n_new > 0 ? (int32_t)std::min<int64_t>(d.n_total, sink_carry(P)) : 0;
    d.L = P.L; d.M = P.M; d.half = P.half; d.taps = P.taps; d.format = S.format;
    d.tab_lds = pcm_sink_tab_in_lds(P.L, P.taps) ? 1 : 0;
    return d.n_out + d.keep != 0;   // 24 kHz float never comes here; a finish that adds nothing is dropped
}

void Engine::SinkStage::issue(size_t d0, int n_live) {
    int max_work = 0;
    bool any_lds = false;
    for (int i = 0; i < n_live; ++i) {
        const PcmSinkDesc& d = desc_h[d0 + (size_t)i];
        max_work = std::max(max_work, d.n_out + d.keep);
        any_lds = any_lds || d.tab_lds;
    }
    launch_pcm_sinks((const PcmSinkDesc*)desc.p + d0, n_live, max_work, any_lds, e.stream);
}

void Engine::SinkStage::commit_one(const StagePush& q) {
    const bool flip = q.desc >= 0 && desc_h[(size_t)q.desc].keep > 0;
    if (flip) tab.slots[(size_t)q.id].carry_abs0 = desc_h[(size_t)q.desc].n_total - desc_h[(size_t)q.desc].keep;
    tab.commit(q.id, q.n_new, q.n_out, q.finish, flip);
}

} // namespace q3
