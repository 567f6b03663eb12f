// q3_pcm_sink.cpp — PCM sinks: the output side's mirror of the encoder streams' resampler (4k).  A sink takes 24 kHz
// float PCM that already lies on the device (the vocoder's, or samples staged by the standalone entry) and delivers it at its own rate
// (4 000 .. 192 000 Hz) as float or int16: a windowed-sinc polyphase resampler (q3_audio.h: sink_plan) whose state is the last
// 2 * half + ceil(M / L) input samples.  All sinks of a call share one launch (launch_pcm_sinks); how many samples a push delivers
// is the host rule sink_emitted and nothing else.  [HINT] no counterpart in the reference, which writes 24 kHz only (main.cpp).
#include <algorithm>
#include <cstring>
#include <vector>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

const Engine::SinkPlanDev& Engine::pcm_sink_plan(int rate) {
    auto it = sink_plans.find(rate);
    if (it != sink_plans.end()) return it->second;
    SinkPlanDev pd;
    pd.plan = sink_plan(rate);   // throws, naming the rate, before anything is allocated
    if (!pd.plan.table.empty()) {
        Q3_HIP_CHECK(hipMalloc((void**)&pd.tab_d, pd.plan.table.size() * sizeof(float)));
        const hipError_t err = hipMemcpy(pd.tab_d, pd.plan.table.data(), pd.plan.table.size() * sizeof(float), hipMemcpyHostToDevice);
        if (err != hipSuccess) { (void)hipFree(pd.tab_d); Q3_HIP_CHECK(err); }
    }
    return sink_plans.emplace(rate, std::move(pd)).first->second;
}

int Engine::pcm_sink_begin(int rate, int format) {
    if (format != Q3TTS_PCM_F32 && format != Q3TTS_PCM_S16) throw Error("pcm sink: format " + std::to_string(format) + " is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16");
    const SinkPlanDev& pd = pcm_sink_plan(rate);
    int id = -1;
    for (size_t i = 0; i < sinks.size(); ++i) if (!sinks[i].used) { id = (int)i; break; }
    if (id < 0) {
        if ((int)sinks.size() >= kMaxPcmSinks) throw Error("pcm sink: at most " + std::to_string(kMaxPcmSinks) + " sinks are open at a time");
        sinks.emplace_back();
        id = (int)sinks.size() - 1;
    }
    PcmSink& S = sinks[(size_t)id];
    // the carry: two buffers of kPcmSinkCarry floats in an allocation of the sink's own, kept for the id's next sink
    if (!S.carry) Q3_HIP_CHECK(hipMalloc((void**)&S.carry, 2 * (size_t)kPcmSinkCarry * sizeof(float)));
    if (sink_carry(pd.plan) > kPcmSinkCarry) throw Error("pcm sink: carry larger than its buffer");
    S.used = true; S.rate = rate; S.format = format; S.plan = &pd;
    S.n_in = S.n_out = S.carry_abs0 = 0; S.finished = false; S.cur = 0;
    return id;
}

void Engine::pcm_sink_end(int id) {
    if (id < 0 || id >= (int)sinks.size() || !sinks[(size_t)id].used) throw Error("pcm sink: no such sink");
    sinks[(size_t)id].used = false;
}

void Engine::pcm_sink_free() {
    for (PcmSink& S : sinks) if (S.carry) (void)hipFree(S.carry);
    sinks.clear();
    for (auto& kv : sink_plans) if (kv.second.tab_d) (void)hipFree(kv.second.tab_d);
    sink_plans.clear();
    if (sink_desc_d) (void)hipFree(sink_desc_d);
    if (sink_out_d) (void)hipFree(sink_out_d);
    if (sink_in_d) (void)hipFree(sink_in_d);
    sink_desc_d = nullptr; sink_out_d = nullptr; sink_in_d = nullptr;
    sink_desc_cap = 0; sink_out_bytes = sink_in_floats = 0;
}

const Engine::PcmSink& Engine::pcm_sink_get(int id) const {
    if (id < 0 || id >= (int)sinks.size() || !sinks[(size_t)id].used) throw Error("pcm sink: no such sink");
    return sinks[(size_t)id];
}

int64_t Engine::pcm_sink_push_len(int id, int64_t n_new, bool finish) const {
    const PcmSink& S = pcm_sink_get(id);
    if (S.finished) throw Error("pcm sink: sink " + std::to_string(id) + " is finished");
    if (n_new < 0) throw Error("pcm sink: negative sample count");
    if (S.n_in + n_new > kPcmSinkMaxSamples) throw Error("pcm sink: sink " + std::to_string(id) + " would exceed one hour of 24 kHz input");
    return sink_emitted(S.plan->plan, S.n_in + n_new, finish) - S.n_out;
}

// A call's launches: pcm_sinks_reserve once (the only place the workspace may grow, before anything is enqueued), then one
// pcm_sinks_launch per set of sinks whose input is ready, then (after the stream has been synchronised) pcm_sinks_commit for all.
void Engine::pcm_sinks_reserve(int n_total, size_t out_bytes_total) {
    if (sink_desc_cap < (size_t)n_total) {
        sync();
        if (sink_desc_d) (void)hipFree(sink_desc_d);
        sink_desc_d = nullptr; sink_desc_cap = 0;
        const size_t cap = std::max((size_t)64, (size_t)n_total);
        Q3_HIP_CHECK(hipMalloc((void**)&sink_desc_d, cap * sizeof(PcmSinkDesc)));
        sink_desc_cap = cap;
    }
    if (sink_out_bytes < out_bytes_total) {
        sync();
        if (sink_out_d) (void)hipFree(sink_out_d);
        sink_out_d = nullptr; sink_out_bytes = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&sink_out_d, out_bytes_total));
        sink_out_bytes = out_bytes_total;
    }
    sink_desc_h.assign((size_t)n_total, PcmSinkDesc());   // never resized during the call: uploads read it until the sync
    sink_desc_used = 0; sink_out_used = 0;
}

void Engine::pcm_sinks_launch(SinkPush* ps, int n) {
    const size_t d0 = sink_desc_used;
    int n_live = 0, max_work = 0;
    bool any_lds = false;
    for (int i = 0; i < n; ++i) {
        SinkPush& q = ps[i];
        const PcmSink& S = pcm_sink_get(q.sink);
        const SinkPlan& P = S.plan->plan;
        q.n_out = pcm_sink_push_len(q.sink, q.n_new, q.finish);
        q.desc = -1;
        if (q.n_new == 0 && q.n_out == 0) continue;   // an empty push: the carry stays, nothing is emitted
        if (d0 + n_live >= sink_desc_h.size()) throw Error("pcm sink: more launches than the call reserved");
        PcmSinkDesc& d = sink_desc_h[d0 + n_live];
        const size_t bytes = ((size_t)q.n_out * (S.format == Q3TTS_PCM_S16 ? 2 : 4) + 255) & ~(size_t)255;
        if (sink_out_used + bytes > sink_out_bytes) throw Error("pcm sink: more output than the call reserved");
        d.carry_in = S.carry + (size_t)S.cur * kPcmSinkCarry; d.carry_out = S.carry + (size_t)(1 - S.cur) * kPcmSinkCarry;
        d.x_new = q.n_new > 0 ? q.x_dev : d.carry_in;
        d.tab = S.plan->tab_d;
        d.out = sink_out_d + sink_out_used;
        d.carry_abs0 = S.carry_abs0; d.n_before = S.n_in; d.n_total = S.n_in + q.n_new; d.out0 = S.n_out;
        if (q.n_new > 2147483647LL || q.n_out > 2147483647LL - 256) throw Error("pcm sink: push too large");
        d.n_new = (int32_t)q.n_new; d.n_out = (int32_t)q.n_out;
        d.keep = q.n_new > 0 ? (int32_t)std::min<int64_t>(d.n_total, sink_carry(P)) : 0;
        d.L = P.L; d.M = P.M; d.half = P.half; d.taps = P.taps; d.s16 = S.format == Q3TTS_PCM_S16;
        d.tab_lds = pcm_sink_tab_in_lds(P.L, P.taps) ? 1 : 0;
        any_lds = any_lds || d.tab_lds;
        if (d.n_out + d.keep == 0) continue;          // 24 kHz float never comes here; a finish that adds nothing
        max_work = std::max(max_work, d.n_out + d.keep);
        q.desc = (int)(d0 + n_live);
        sink_out_used += bytes;
        ++n_live;
    }
    if (n_live == 0) return;
    Q3_HIP_CHECK(hipMemcpyAsync(sink_desc_d + d0, sink_desc_h.data() + d0, (size_t)n_live * sizeof(PcmSinkDesc), hipMemcpyHostToDevice, stream));
    launch_pcm_sinks(sink_desc_d + d0, n_live, max_work, any_lds, stream);
    sink_desc_used += (size_t)n_live;
    for (int i = 0; i < n; ++i) {
        const SinkPush& q = ps[i];
        if (q.desc < 0) continue;
        const int64_t m = std::min(q.n_out, q.cap);
        const size_t el = sink_desc_h[(size_t)q.desc].s16 ? 2 : 4;
        if (m > 0 && q.out_host) Q3_HIP_CHECK(hipMemcpyAsync(q.out_host, sink_desc_h[(size_t)q.desc].out, (size_t)m * el, hipMemcpyDeviceToHost, stream));
    }
}

void Engine::pcm_sinks_commit(const SinkPush* ps, int n) {
    for (int i = 0; i < n; ++i) {
        const SinkPush& q = ps[i];
        PcmSink& S = sinks[(size_t)q.sink];
        if (q.desc >= 0 && sink_desc_h[(size_t)q.desc].keep > 0) {
            S.cur = 1 - S.cur;
            S.carry_abs0 = sink_desc_h[(size_t)q.desc].n_total - sink_desc_h[(size_t)q.desc].keep;
        }
        S.n_in += q.n_new; S.n_out += q.n_out;
        if (q.finish) S.finished = true;
    }
}

size_t Engine::pcm_sink_out_bytes(int id, int64_t n_new, bool finish) const {
    const PcmSink& S = pcm_sink_get(id);
    return ((size_t)pcm_sink_push_len(id, n_new, finish) * (S.format == Q3TTS_PCM_S16 ? 2 : 4) + 255) & ~(size_t)255;
}

// the standalone entry: its input is staged from the host
void Engine::pcm_sink_push_batch_host(int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                                      void* const* out, int64_t cap, int64_t* out_len) {
    if (n < 0) throw Error("pcm sink push: negative sink count");
    if (n == 0) return;
    if (!ids || !n_in) throw Error("pcm sink push: NULL argument");
    if (cap < 0) throw Error("pcm sink push: negative cap_samples");
    if (n > 65535) throw Error("pcm sink push: at most 65535 sinks per call");
    // ---- everything is validated before any sink moves ----
    std::vector<SinkPush> ps((size_t)n);
    size_t in_total = 0, out_total = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < i; ++k) if (ids[k] == ids[i]) throw Error("pcm sink push: sink " + std::to_string(ids[i]) + " listed twice");
        if (n_in[i] < 0) throw Error("pcm sink push: negative sample count");
        if (n_in[i] > kPcmSinkMaxPush) throw Error("pcm sink push: a push holds at most " + std::to_string(kPcmSinkMaxPush) + " samples");
        if (n_in[i] > 0 && (!pcm24 || !pcm24[i])) throw Error("pcm sink push: NULL samples");
        SinkPush& q = ps[(size_t)i];
        q.sink = ids[i]; q.n_new = n_in[i]; q.finish = finish && finish[i]; q.out_host = out ? out[i] : nullptr; q.cap = cap;
        const int64_t len = pcm_sink_push_len(q.sink, q.n_new, q.finish);   // throws for an unknown / finished / full sink
        if (out_len) out_len[i] = 0;
        if (len > 0 && q.out_host == nullptr && cap > 0) throw Error("pcm sink push: NULL output");
        in_total += ((size_t)q.n_new + 63) & ~(size_t)63;
        out_total += pcm_sink_out_bytes(q.sink, q.n_new, q.finish);
    }
    if (sink_in_floats < in_total) {
        sync();
        if (sink_in_d) (void)hipFree(sink_in_d);
        sink_in_d = nullptr; sink_in_floats = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&sink_in_d, in_total * sizeof(float)));
        sink_in_floats = in_total;
    }
    pcm_sinks_reserve(n, out_total);
    try {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            SinkPush& q = ps[(size_t)i];
            q.x_dev = sink_in_d + off;
            if (q.n_new > 0) Q3_HIP_CHECK(hipMemcpyAsync(sink_in_d + off, pcm24[i], (size_t)q.n_new * sizeof(float), hipMemcpyHostToDevice, stream));
            off += ((size_t)q.n_new + 63) & ~(size_t)63;
        }
        pcm_sinks_launch(ps.data(), n);
        sync();
    } catch (...) { try { sync(); } catch (...) { } throw; }   // the callers' buffers must outlive the copies
    pcm_sinks_commit(ps.data(), n);
    if (out_len) for (int i = 0; i < n; ++i) out_len[i] = ps[(size_t)i].n_out;
}

} // namespace q3
