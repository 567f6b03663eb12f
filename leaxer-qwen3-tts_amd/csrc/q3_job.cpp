// q3_job.cpp — the job layer (q3_job.h): the part every job shares (validation, the queue, admission, the begins, retiring), the offline
// loop and the streaming loop over it, and the vocoder phase.
#include "q3_job.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>

namespace q3 {

void vocoder_job(Engine& e, int n_utt, const std::vector<int32_t>& got_frames, int row_frames, float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len) {
    // Vocoder, once the decode queue is empty.  Utterances are taken longest first, in blocks of similar length (the shortest at least half
    // the longest, at most 2^16 padded frames): a block's pre-transformer and upsampling stages run as one batched pass, its conv decoder in
    // groups of up to 32 utterances per set of launches (about 4.7 MB of workspace per frame: groups sized to ~8 GB), each group padded to its
    // own longest member.  Padding is exact: every layer is causal.  Single utterances, the exact-fp32 codec and configs whose decoder the
    // batched kernels do not cover go one utterance at a time over the side lanes.
    // A failure in here (arena / pinned-buffer allocation, a launch error) must not leave lanes holding this job's pcm_out / pcm_len
    // pointers: the next job's drain would write through them.  codec_async_abort() waits for the lanes and forgets their items.
    try {
    std::vector<int> order((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) { order[(size_t)u] = u; if (pcm_len) pcm_len[u] = 0; }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return got_frames[(size_t)x] > got_frames[(size_t)y]; });
    const bool batchable = e.codec_batchable();
    std::vector<int> nf;
    std::vector<float*> up;
    std::vector<int64_t*> lp;
    for (int y0 = 0; y0 < n_utt;) {
        const int F0 = got_frames[(size_t)order[(size_t)y0]];
        if (F0 <= 0) break;                                            // sorted: the rest of the job produced no frame
        int y1 = y0 + 1;
        // a block is a batch dimension of the batched kernels (gridDim.y / .z <= 65535): at most 4096 sequences and 2^16 padded frames, and
        // no activation matrix of its batched front may reach 4 GB (k_conv_split addresses rows with 32-bit byte offsets): the widest is
        // the ConvNeXt hidden [frames x upsampling][4 x cd_hidden] — at 0.6B dims exactly 4 GB at 2^16 frames, hence the strict bound
        int64_t up_front = 1;
        for (int i = 0; i < e.c.cd_n_up; ++i) up_front *= e.c.cd_up_ratios[i];
        const int64_t widest = std::max<int64_t>((int64_t)4 * e.c.cd_hidden * up_front, std::max<int64_t>(e.c.cd_ffn, (int64_t)3 * e.c.cd_hidden));
        const int64_t frame_cap = std::min<int64_t>((int64_t)1 << 16, (((int64_t)1 << 32) - 1) / ((int64_t)sizeof(float) * widest));
        while (y1 < n_utt && y1 - y0 < 4096 && (int64_t)(y1 - y0 + 1) * F0 <= frame_cap && got_frames[(size_t)order[(size_t)y1]] * 2 >= F0) ++y1;
        const int nblk = y1 - y0;
        if (nblk >= 2 && batchable && F0 <= frame_cap / 2) {
            int rows = 0;
            e.codec_lanes_join();                                      // the previous block's groups still read the batched buffers
            const float* hb = e.codec_pre_batch(e.codec_job_codes(0, row_frames), row_frames, nblk, F0, true, &rows, order.data() + y0);
            const size_t ustride = (size_t)rows * e.c.cd_hidden;
            const int group = (int)std::max<int64_t>(1, std::min<int64_t>(32, ((int64_t)8 << 30) / ((int64_t)4700000 * F0)));
            for (int g0 = 0; g0 < nblk; g0 += group) {
                const int g = std::min(group, nblk - g0);
                nf.assign((size_t)g, 0); up.assign((size_t)g, nullptr); lp.assign((size_t)g, nullptr);
                for (int k = 0; k < g; ++k) {
                    const int u = order[(size_t)(y0 + g0 + k)];
                    nf[(size_t)k] = got_frames[(size_t)u];
                    if (pcm_len) lp[(size_t)k] = pcm_len + u;
                    if (pcm_out) up[(size_t)k] = pcm_out[u];
                }
                e.codec_async_submit_group(hb + (size_t)g0 * ustride, ustride, nf[0], g, nf.data(), up.data(), pcm_cap, lp.data());
            }
        } else {
            for (int y = y0; y < y1; ++y) {
                const int u = order[(size_t)y];
                e.codec_async_submit_dev(e.codec_job_codes(u, row_frames), got_frames[(size_t)u], pcm_out ? pcm_out[u] : nullptr, pcm_cap, pcm_len ? pcm_len + u : nullptr);
            }
        }
        y0 = y1;
    }
    e.codec_async_drain();
    } catch (...) {
        e.codec_async_abort();
        for (int u = 0; u < n_utt; ++u) if (pcm_len) pcm_len[u] = 0;
        throw;
    }
}

namespace {

// The stage settings as the slots' implicit streams take them (Engine::slot_stages: 0 is "none" throughout)
Engine::SlotStages slot_stages_of(const StageSettings& s) {
    const bool sunk = s.sink.sample_rate > 0, levelled = s.gain_cb != 0 || s.ceiling != 0;
    Engine::SlotStages o;
    o.sink_rate = sunk && !(s.sink.sample_rate == 24000 && s.sink.format == Q3TTS_PCM_F32) ? s.sink.sample_rate : 0;   // 24 kHz float is what the vocoder gives
    o.sink_format = s.sink.format;
    o.speed = s.speed != 1000 ? s.speed : 0; o.pitch = s.pitch != 1000 ? s.pitch : 0;
    o.gain_cb = levelled ? s.gain_cb : 0; o.ceiling = levelled ? s.ceiling : 0;
    o.tone_n = s.tone_n; for (int j = 0; j < s.tone_n; ++j) o.tone[j] = s.tone[j];
    o.loud = s.loud ? 1 : 0; o.loud_target = s.loud_target; o.loud_range = s.loud_range; o.loud_start = s.loud_start;
    return o;
}

// The streaming loop's chunk buffer: a chunk of at most `cap` vocoder samples leaves the stages as at most `deliver` samples of the
// delivered format, which take `floats` 4-byte words per slot.  One term per stage, in the order the samples pass them.
struct ChunkCapacity { int64_t floats, deliver; };
ChunkCapacity chunk_capacity(Engine& e, const StageSettings& s, int64_t cap) {
    // with a pitch (q3tts_engine_set_pitch) the stage in front hands on what it held back: at most kPitchLA samples more
    if (s.pitch != 1000) cap += kPitchLA;
    // with a speed (q3tts_engine_set_speed) the chunk first passes its stretcher: at most the chunk plus what the stretcher held back
    // (N + D + Hs input samples), 1000 / S times as long, plus the cut last block
    if (s.speed != 1000) cap = ((cap + kSpeedN + kSpeedD + kSpeedHs) * 1000 + s.speed - 1) / s.speed + kSpeedHs;
    // a tone stage (q3tts_engine_set_tone) emits what it receives: no term
    // a loudness stage (q3tts_engine_set_loudness) holds back less than one sub-block
    if (s.loud) cap += kLoudBlock - 1;
    // with a level (q3tts_engine_set_level) the limiter hands on what it held back as well: at most W - 1 samples more
    if (s.ceiling != 0) cap += kLevelW - 1;
    if (s.sink.sample_rate <= 0) return ChunkCapacity{ cap, cap };
    // with a sink a chunk's buffer holds the sink's samples: the chunk's share plus the flushed tail, by the host rule's closed form
    const SinkPlan& plan = e.sink.plan_for(s.sink.sample_rate).plan;
    const int64_t sink_cap = ((cap + plan.half) * plan.L + plan.M - 1) / plan.M + 2;
    return ChunkCapacity{ (sink_cap * (int64_t)pcm_format_bytes(s.sink.format) + 3) / 4, sink_cap };   // per slot, 4-byte aligned
}


// one utterance's prompt: rows, trailing rows, and where they start in the job's buffers
struct Prep { int S = 0, nt = 0; size_t poff = 0, toff = 0; };

// What the offline and the streaming loop share: the checks before any slot is touched, the prompts, the queue, and the three things
// that happen to an utterance — it is admitted to a slot, its slot is armed (begun), it is retired.
struct Job {
    Engine& e; const JobArgs& a; const q3tts_sampling& p;
    const int n_utt, H, G, B;
    int P = 0, live = 0;                     // the longest run of teacher-forced frames; utterances in a slot
    std::vector<Prep> prep; std::vector<float> prompts, trailing;
    std::deque<int> pending;                 // utterances waiting for a slot, in order
    std::vector<int> slot_utt, fresh;        // the utterance in each slot (-1: free); the slots the last admit() filled
    std::vector<int> pinned;                 // the shared prompt prefixes this job holds
    std::vector<Engine::SlotInit> init, rag;
    void offline(), stream();                // the two loops

    // rows of the shared prompt prefix in front of utterance u's prompt (0 without one): part of its context, not of prep[u].S
    int pl(int u) const { return a.prefix_ids && a.prefix_ids[u] != -1 ? e.prefix_get(a.prefix_ids[u]).P : 0; }
    // teacher-forced frames per utterance (q3tts_synthesize_continue_host / _continue_stream_host): pf(u) of them behind utterance u's prompt, P the longest
    int pf(int u) const { return a.prefix_codes ? (int)(a.prefix_offsets[u + 1] - a.prefix_offsets[u]) : 0; }
    const int64_t* pcodes(int u) const { return a.prefix_codes + (size_t)a.prefix_offsets[u] * (size_t)G; }
    int cap_of(int u) const { return a.max_new_per_utt ? std::min(std::max(1, (int)a.max_new_per_utt[u]), p.max_new_tokens) : p.max_new_tokens; }
    int ctx_of(int u) const { return pl(u) + prep[(size_t)u].S + pf(u); }   // positions utterance u holds before its first new frame

    Job(Engine& en, const JobArgs& ar) : e(en), a(ar), p(*ar.p), n_utt(ar.n_utt), H(en.c.hidden), G(en.c.n_groups), B(en.B), slot_utt((size_t)en.B, -1) {}
    ~Job() { for (int id : pinned) { try { e.prefix_pin(id, -1); } catch (...) { } } }

    // The checks every job makes before a slot is touched (the streaming loop makes its own first); then every slot is free
    void validate() {
        if (a.pcm_cap < 0) throw Error("synthesize: negative pcm_cap");
        (void)Engine::checked_penalty(p);   // refused before any slot is touched
        // the job's shared prompt prefixes (q3tts_synthesize_prefixed_host): validated up front, held against q3tts_prefix_release while the job runs
        for (int u = 0; a.prefix_ids && u < n_utt; ++u) if (a.prefix_ids[u] != -1) (void)e.prefix_get(a.prefix_ids[u]);   // throws on an unknown id, nothing held yet
        for (int u = 0; a.prefix_ids && u < n_utt; ++u) if (a.prefix_ids[u] != -1) { e.prefix_pin(a.prefix_ids[u], 1); pinned.push_back(a.prefix_ids[u]); }
        if (a.prefix_codes && !a.prefix_offsets) throw Error("synthesize: prefix_codes without prefix_offsets");
        if (a.prefix_codes && a.text_cb) throw Error("synthesize_live: live text behind prefix codes is not implemented");
        for (int u = 0; u < n_utt; ++u) {
            if (pf(u) < 0 || (a.prefix_codes && a.prefix_offsets[u] < 0)) throw Error("synthesize: prefix_offsets must start at >= 0 and not decrease");
            if (pf(u) > 0 && pf(u) + p.max_new_tokens > e.max_frames_cap) throw Error("synthesize: utterance " + std::to_string(u) + ": prefix frames + max_new_tokens exceeds the slot's frame capacity");
            try { if (pf(u) > 0) e.check_frame_codes(pcodes(u), pf(u), true); }
            catch (const Error& ex) { throw Error("synthesize: utterance " + std::to_string(u) + ": " + ex.msg); }
            P = std::max(P, pf(u));
        }
        for (int b = 0; b < B; ++b) e.slot_release(b);
    }

    // Prompt rows of every utterance of a job, assembled before the first step in one projection pass (Engine::build_prompts: one utterance
    // at a time it is a handful of small synchronous device round trips each).  Utterance u's prompt starts at row prep[u].poff of `prompts`;
    // with an instruction (include/q3tts.h: q3tts_synthesize_instruct_host) its text_project rows come first, all instructions of the job
    // through one further projection pass.
    void assemble() {
        prep.assign((size_t)n_utt, Prep());
        if (a.instruct_ids && !a.instruct_offsets) throw Error("synthesize: instruct_ids without instruct_offsets");
        auto n_ins = [&](int u) { return a.instruct_ids ? (int)(a.instruct_offsets[u + 1] - a.instruct_offsets[u]) : 0; };
        size_t prow = 0, trow = 0, n_ins_all = 0;
        for (int u = 0; u < n_utt; ++u) {
            if (n_ins(u) < 0) throw Error("synthesize: instruct_offsets must not decrease");
            prep[(size_t)u].poff = prow; prep[(size_t)u].toff = trow;
            prow += 16 + (size_t)n_ins(u); n_ins_all += (size_t)n_ins(u);
            trow += (size_t)std::max(1, a.offsets[u + 1] - a.offsets[u] - 3);   // trailing rows: text tokens minus the first, plus tts_eos
        }
        trailing.resize(trow * H);
        std::vector<size_t> toffs((size_t)n_utt);
        std::vector<int> Ss((size_t)n_utt), nts((size_t)n_utt);
        for (int u = 0; u < n_utt; ++u) toffs[(size_t)u] = prep[(size_t)u].toff;
        if (n_ins_all == 0) {
            prompts.resize(prow * H);
            e.build_prompts(a.ids, a.offsets, n_utt, a.lang, a.speakers, prompts.data(), Ss.data(), trailing.data(), toffs.data(), nts.data());
        } else {
            std::vector<float> base((size_t)n_utt * 16 * H), ins(n_ins_all * H);
            e.build_prompts(a.ids, a.offsets, n_utt, a.lang, a.speakers, base.data(), Ss.data(), trailing.data(), toffs.data(), nts.data());
            const int64_t i0 = a.instruct_offsets[0];
            if (n_ins_all > (size_t)e.max_ctx * (size_t)n_utt) throw Error("synthesize: instructions longer than max_ctx");
            e.text_project(a.instruct_ids + i0, (int)n_ins_all, ins.data());
            prompts.resize(prow * H);
            for (int u = 0; u < n_utt; ++u) {
                float* dst = prompts.data() + prep[(size_t)u].poff * H;
                const size_t ni = (size_t)n_ins(u);
                if (ni > 0) memcpy(dst, ins.data() + (size_t)(a.instruct_offsets[u] - i0) * H, ni * H * sizeof(float));
                memcpy(dst + ni * H, base.data() + (size_t)u * 16 * H, (size_t)Ss[(size_t)u] * H * sizeof(float));
                Ss[(size_t)u] += (int)ni;
            }
        }
        for (int u = 0; u < n_utt; ++u) { prep[(size_t)u].S = Ss[(size_t)u]; prep[(size_t)u].nt = nts[(size_t)u]; }
    }

    // Utterance u joins the queue, once the loop has made its own max_ctx refusals
    void enqueue(int u) {
        if (e.kv_pages_for(ctx_of(u) + cap_of(u)) > e.kv_total_pages())
            throw Error("synthesize: one utterance (prompt + max_new_tokens) needs more KV pages than the pool holds");
        pending.push_back(u);
    }

    // Admission in queue order (q3_kvpool.h: sched_admit_count) of the first n_cand queued utterances, pages_of(u) pages each, into `fresh`
    template <class PagesOf> void admit(size_t n_cand, bool lengths_known, PagesOf pages_of) {
        fresh.clear();
        std::vector<int> free_slots, need;
        for (int b = 0; b < B; ++b) if (slot_utt[(size_t)b] < 0) free_slots.push_back(b);
        for (size_t i = 0; i < n_cand && i < free_slots.size(); ++i) need.push_back(pages_of(pending[i]));
        const int n_adm = sched_admit_count(e.kv, need, (int)free_slots.size(), live, lengths_known);
        for (int i = 0; i < n_adm; ++i) { slot_utt[(size_t)free_slots[(size_t)i]] = pending.front(); pending.pop_front(); fresh.push_back(free_slots[(size_t)i]); }
    }

    // Begins the fresh slots; kv_tokens(u) is the SlotInit's (0: prompt + cap, reserved now).  The order of the begin calls is the job
    // layer's contract: it decides which prompts share a prefill pass, and so the bits.
    //   Q3TTS_FLAG_RAGGED_PREFILL: the long prompts (S > 16) and the forced begins of the look in one ragged begin — what would be begun
    //   on its own joins it — then the rest;  without it every forced begin on its own, in `fresh` order (a re-admission after a
    //   preemption too; the slot starts pf(u) frames in), then the rest.
    //   The rest: equal-length prompts share one prefill pass (behind their prefixes: at per-member bases).
    template <class KvTokens> void arm(KvTokens kv_tokens) {
        if (fresh.empty()) return;
        const bool ragged = (e.flags & Q3TTS_FLAG_RAGGED_PREFILL) != 0;
        init.clear(); rag.clear();
        for (int b : fresh) {
            const int u = slot_utt[(size_t)b];
            const Prep& pr = prep[(size_t)u];
            Engine::SlotInit q;
            q.slot = b; q.prompt = prompts.data() + pr.poff * H; q.S = pr.S; q.trailing = trailing.data() + pr.toff * H; q.n_trailing = pr.nt;
            q.stream_id = (uint32_t)u;
            q.max_frames = a.max_new_per_utt ? std::max(1, (int)a.max_new_per_utt[u]) : 0;
            q.kv_tokens = kv_tokens(u);
            if (a.prefix_ids) q.prefix_id = a.prefix_ids[u];
            if (pf(u) > 0) { q.prefix = pcodes(u); q.n_prefix = pf(u); }
            if (ragged && (q.n_prefix > 0 || q.S > 16)) rag.push_back(q);
            else if (q.n_prefix > 0) e.slots_begin(&q, 1, p, a.seed, a.ignore_eos);
            else init.push_back(q);
        }
        if (!rag.empty()) e.slots_begin_ragged(rag.data(), (int)rag.size(), p, a.seed, a.ignore_eos);
        if (!init.empty()) {
            if (a.prefix_ids) e.slots_begin_prefixed(init.data(), (int)init.size(), p, a.seed, a.ignore_eos);
            else e.slots_begin(init.data(), (int)init.size(), p, a.seed, a.ignore_eos);
        }
        live += (int)fresh.size();
        e.sched_admitted += (int64_t)fresh.size();
        e.sched_peak_live = std::max(e.sched_peak_live, live);
    }

    // Slot b's utterance is done: its codes go out, the slot is free
    void retire(int b) {
        const int u = slot_utt[(size_t)b];
        if (a.codes_out) e.slot_codes(b, a.codes_out + (size_t)u * (size_t)(P + p.max_new_tokens) * G, P + p.max_new_tokens);
        e.slot_release(b);
        slot_utt[(size_t)b] = -1; --live;
    }

    void release_all() { for (int b = 0; b < B; ++b) { try { e.slot_release(b); } catch (...) { } } }   // a job that failed leaves no slot armed
};

} // namespace

// Continuous batching: utterances queue for the engine's max_batch slots; a slot that finishes (EOS or max_new_tokens) stashes its codes
// and is re-armed with the next utterance at the following look, so ragged lengths do not idle the batch; the vocoder runs over the
// side lanes once the decode queue is empty.  Results do not depend on the schedule: the RNG stream of an utterance is its index,
// never its slot.
void Job::offline() {
    validate();
    const int row_frames = std::max(1, std::min(P + p.max_new_tokens, e.max_frames_cap));
    e.codec_async_prepare(row_frames, n_utt);
    std::vector<int32_t> got_frames((size_t)n_utt, 0);
    assemble();
    // KV pages.  With EOS suppressed every length is known: an utterance is admitted when the pool holds prompt + cap and never waits again.
    // Otherwise a slot owns what its context has reached plus the coming look (on-demand growth), so utterances that end early never hold
    // the pages of their cap; when the pool runs dry the YOUNGEST live utterance is preempted — its pages go back, it returns to the head
    // of the queue and is generated again from its prompt later (same RNG stream, same codes) — so the oldest always finishes.
    std::vector<int> done_frames((size_t)B, 0), retired;
    std::vector<SlotState> st;
    for (int u = 0; u < n_utt; ++u) {
        if ((pf(u) > 0 || pl(u) > 0) && ctx_of(u) + p.max_new_tokens > e.max_ctx)
            throw Error("synthesize: utterance " + std::to_string(u) + ": prefix + prompt + prefix frames + max_new_tokens exceeds max_ctx");
        enqueue(u);
    }
    const bool reserve_all = a.ignore_eos != 0;
    const int first_look = 8;
    // A preempted utterance is not re-admitted on the pages it just gave back: it waits until a live utterance has retired or the pool
    // holds what it owned when it was preempted plus one page of head-room — otherwise a pool just above one utterance's cap re-admits
    // and preempts the same utterance look after look, paying a prefill and discarding its frames each time.
    std::vector<int> hold_pages((size_t)n_utt, 0);
    std::vector<int64_t> hold_mark((size_t)n_utt, 0);
    int64_t n_retired = 0;
    e.sched_admitted = e.sched_preempted = 0; e.sched_peak_live = 0;
    const char* const quantum_env = getenv("Q3TTS_SCHED_QUANTUM");
    const int quantum = quantum_env ? std::max(1, atoi(quantum_env)) : 4;
    try {
        while (!pending.empty() || live > 0) {
            admit(pending.size(), reserve_all, [&](int u) {
                const int all = ctx_of(u) + cap_of(u);
                int pages = e.kv_pages_for(reserve_all ? all : std::min(all, ctx_of(u) + first_look));
                if (hold_pages[(size_t)u] > 0 && n_retired == hold_mark[(size_t)u] && live > 0) pages = std::max(pages, std::min(hold_pages[(size_t)u], e.kv_total_pages()));
                return pages;
            });
            arm([&](int u) { return reserve_all ? 0 : ctx_of(u) + first_look; });
            for (int b : fresh) done_frames[(size_t)b] = pf(slot_utt[(size_t)b]);   // a forced begin starts pf(u) frames in
            int rem = p.max_new_tokens;
            for (int b = 0; b < B; ++b) {
                const int u = slot_utt[(size_t)b];
                if (u >= 0) rem = std::min(rem, pf(u) + cap_of(u) - done_frames[(size_t)b]);
            }
            const int steps = sched_look_steps(rem, live, !pending.empty(), a.ignore_eos != 0, quantum);
            if (!reserve_all) {
                // every live slot gets pages for the positions these steps write; oldest first, so that when the pool runs dry it is the
                // youngest that goes back to the queue (q3_kvpool.h: sched_grow)
                std::vector<int> order, want, changed;
                for (int b = 0; b < B; ++b) if (slot_utt[(size_t)b] >= 0) order.push_back(b);
                std::sort(order.begin(), order.end(), [&](int x, int y) {
                    return done_frames[(size_t)x] != done_frames[(size_t)y] ? done_frames[(size_t)x] > done_frames[(size_t)y] : slot_utt[(size_t)x] < slot_utt[(size_t)y]; });
                for (int b : order) {
                    const int u = slot_utt[(size_t)b];
                    want.push_back(pl(u) + std::min(prep[(size_t)u].S + pf(u) + cap_of(u), prep[(size_t)u].S + done_frames[(size_t)b] + steps));
                }
                const std::vector<int> victims = sched_grow(e.kv, order, want, &changed);
                for (int vb : victims) {          // youngest first: pushed to the front one by one, the oldest of them ends up first in the queue
                    const int vu = slot_utt[(size_t)vb];
                    hold_pages[(size_t)vu] = e.kv_pages_for(pl(vu) + prep[(size_t)vu].S + done_frames[(size_t)vb]) + 1;
                    hold_mark[(size_t)vu] = n_retired;
                    e.slot_release(vb);           // deactivates the slot (its pages are already back in the pool)
                    pending.push_front(vu);
                    slot_utt[(size_t)vb] = -1; done_frames[(size_t)vb] = 0;
                    --live; ++e.sched_preempted;
                }
                for (int b : changed) e.kv_upload_row(b);
            }
            e.decode_steps(steps);
            e.slots_state(B, st);
            retired.clear();
            for (int b = 0; b < B; ++b) {
                const int u = slot_utt[(size_t)b];
                if (u < 0) continue;
                const SlotState& s = st[(size_t)b];
                done_frames[(size_t)b] = s.n_frames;
                if (!(s.finished || s.n_frames >= s.max_frames)) continue;
                got_frames[(size_t)u] = s.n_frames;
                if (a.n_frames) a.n_frames[u] = s.n_frames;
                e.codec_stash(b, s.n_frames, u, row_frames);
                retired.push_back(b);
            }
            for (int b : retired) { retire(b); done_frames[(size_t)b] = 0; ++n_retired; }
        }
    } catch (...) {
        try { e.codec_async_drain(); } catch (...) { }
        release_all();
        throw;
    }
    if (P == 0) { vocoder_job(e, n_utt, got_frames, row_frames, a.pcm_out, a.pcm_cap, a.pcm_len); return; }
    // With prefixes every utterance is decoded whole into a buffer of the job's own, and the caller receives the samples its new frames
    // own: [L(prefix), L(all)) of the whole decode (causal decoder: exact).  An utterance without a prefix receives all of its decode.
    std::vector<std::vector<float>> whole((size_t)n_utt);
    std::vector<float*> wp((size_t)n_utt, nullptr);
    std::vector<int64_t> wl((size_t)n_utt, 0);
    int64_t wcap = 1;
    for (int u = 0; u < n_utt; ++u) {
        const int64_t L = got_frames[(size_t)u] > 0 ? q3tts_codec_decode_len(&e.c, got_frames[(size_t)u]) : 0;
        if (a.pcm_out && a.pcm_out[u]) { whole[(size_t)u].resize((size_t)std::max<int64_t>(L, 1)); wp[(size_t)u] = whole[(size_t)u].data(); }
        wcap = std::max(wcap, L);
    }
    for (int u = 0; u < n_utt; ++u) if (wp[(size_t)u]) { whole[(size_t)u].resize((size_t)wcap); wp[(size_t)u] = whole[(size_t)u].data(); }   // one capacity for the job
    vocoder_job(e, n_utt, got_frames, row_frames, a.pcm_out ? wp.data() : nullptr, wcap, wl.data());
    for (int u = 0; u < n_utt; ++u) {
        const int64_t first = pf(u) > 0 ? q3tts_codec_decode_len(&e.c, pf(u)) : 0, own = std::max<int64_t>(0, wl[(size_t)u] - first);
        if (a.pcm_len) a.pcm_len[u] = own;
        if (wp[(size_t)u] && own > 0) memcpy(a.pcm_out[u], wp[(size_t)u] + first, (size_t)std::min(own, a.pcm_cap) * sizeof(float));
    }
}

// job_offline with the audio delivered chunk by chunk: decode chunk_frames steps, vocode every live slot's new frames in batched passes
// (Engine::slots_codec_decode_new), call back, retire / re-arm.  Admission reserves prompt + cap for every utterance (no growth, no
// preemption: delivered audio cannot be taken back), so the loop needs none of the offline loop's page policy.
// Behind teacher-forced frames (q3tts_synthesize_continue_stream_host; tts_onnx.cpp:824-842, :759-776): forced begins, primed vocoder
// streams.  With a text callback (q3tts_synthesize_live_host; tts_onnx.cpp:531-536, :833-842) the texts are pulled while the audio is
// generated, and prompts are built at admission.
void Job::stream() {
    const bool live_text = a.text_cb != nullptr;
    const q3tts_sink& sink = a.stages.sink;
    const bool sunk = sink.sample_rate > 0;   // deliver through the engine's sink (q3tts_engine_set_sink)
    if (!a.cb && !sunk) throw Error("synthesize_stream: null callback");
    if (sunk && a.pcm_out) throw Error("synthesize_stream: pcm_out must be NULL while a sink is set (q3tts_engine_set_sink): audio leaves through the sink's callback");
    if (a.chunk_frames < 1) throw Error("synthesize_stream: chunk_frames must be positive");
    validate();
    if (!live_text) assemble();
    else { prep.assign((size_t)n_utt, Prep()); for (int u = 0; u < n_utt; ++u) prep[(size_t)u].S = 16; }   // the most a prompt takes, for the page checks; set at admission
    // live text: what each utterance has received (got), whether its source is done, and how many ids are in its slot (prompt or appended).
    // The last two ids received are the chat template's tail once the text closes (every entry drops them): held back while it is open.
    std::vector<std::vector<int64_t>> got((size_t)(live_text ? n_utt : 0));
    std::vector<uint8_t> t_closed((size_t)n_utt, 0), t_sealed((size_t)n_utt, 0);
    std::vector<int> t_fed((size_t)n_utt, 0);
    std::vector<uint8_t> t_gave((size_t)n_utt, 0);   // the source returned ids (or closed) at this turn's poll
    std::vector<int32_t> flim((size_t)B, 0), held((size_t)B, 0), target((size_t)B, 0), deliv((size_t)B, 0);
    auto usable = [&](int u) { const int n = (int)got[(size_t)u].size(); return t_closed[(size_t)u] ? std::max(4, n - 2) : std::max(0, n - 2); };
    auto admissible = [&](int u) { return !live_text || usable(u) >= 5 || (t_closed[(size_t)u] && got[(size_t)u].size() >= 4); };
    std::vector<int64_t> poll_ids(256), app_ids;
    std::vector<int32_t> app_slots, app_off;
    std::vector<uint8_t> app_close;
    std::vector<int32_t> tl_host((size_t)B, 0), nf_host((size_t)B, 0);   // live text: each live slot's text rows and frames as of the last look
    for (int u = 0; u < n_utt; ++u) {
        if (pf(u) > 0 && ctx_of(u) + p.max_new_tokens > e.max_ctx)
            throw Error("synthesize: utterance " + std::to_string(u) + ": prefix + prompt + prefix frames + max_new_tokens exceeds max_ctx");
        if (pl(u) > 0 && pl(u) + prep[(size_t)u].S + p.max_new_tokens > e.max_ctx)
            throw Error("synthesize: utterance " + std::to_string(u) + ": prefix + prompt + max_new_tokens exceeds max_ctx");
        enqueue(u);
        if (a.pcm_len) a.pcm_len[u] = 0;
        if (a.n_frames) a.n_frames[u] = 0;
    }
    const int cf = std::min(a.chunk_frames, e.max_frames_cap);   // samples of cf frames at the start of an utterance / further in
    const int64_t chunk_cap = std::max(q3tts_codec_decode_len(&e.c, cf), q3tts_codec_decode_len(&e.c, cf + 1) - q3tts_codec_decode_len(&e.c, 1));
    const ChunkCapacity cap = chunk_capacity(e, a.stages, chunk_cap);
    std::vector<float> chunk_pcm((size_t)B * cap.floats);
    std::vector<float*> pcm_ptr((size_t)B);
    std::vector<int32_t> final_frames((size_t)B, -1);
    struct SlotStagesScope {   // the slots' implicit streams take the stages for the duration of this call only
        Engine& e;
        SlotStagesScope(Engine& en, const Engine::SlotStages& s) : e(en) { e.slot_stages = s; }
        ~SlotStagesScope() { e.slot_stages = Engine::SlotStages(); }
    } stages_scope(e, slot_stages_of(a.stages));
    std::vector<int32_t> slots, fb((size_t)B), fe((size_t)B);
    std::vector<int64_t> plen((size_t)B), written((size_t)n_utt, 0);
    std::vector<SlotState> st;
    e.sched_admitted = e.sched_preempted = 0; e.sched_peak_live = 0;
    // Live text: audio leaves in the pushes q3tts_synthesize_stream_host makes — frames up to the next multiple of chunk_frames, one
    // push per round — so a text that arrives in time gives the very samples of the whole text.  Frames past the last multiple
    // wait (held), except those of a finished slot (its tail) and of a starved slot whose source had nothing this turn (a
    // silent source must not hold audio back).  Without live text there is one round and every slot is at its frame count.
    auto plan_delivery = [&]() {   // live text: how far each live slot's audio may go this turn
        for (int b = 0; b < B; ++b) {
            const int u = slot_utt[(size_t)b];
            if (u < 0) continue;
            const SlotState& s = st[(size_t)b];
            const bool fin = s.finished || s.n_frames >= s.max_frames;
            const bool flush = fin || (s.text_open && s.n_frames >= s.trailing_len && !t_gave[(size_t)u]);
            target[(size_t)b] = flush ? s.n_frames : s.n_frames / cf * cf;
            nf_host[(size_t)b] = s.n_frames;
        }
    };
    // one push per live slot with frames to deliver (live text: up to its limit of this round) and the callbacks behind it; a finished
    // slot is retired with its last frames.  false: no slot had anything left.
    auto deliver_round = [&](bool first) -> bool {
        slots.clear();
        for (int b = 0; b < B; ++b) {
            if (slot_utt[(size_t)b] < 0) continue;
            const SlotState& s = st[(size_t)b];
            const bool fin = s.finished || s.n_frames >= s.max_frames;
            if (live_text) {
                if (!(deliv[(size_t)b] < target[(size_t)b] || (fin && first))) continue;   // nothing of this slot leaves in this round
                flim[slots.size()] = std::min(target[(size_t)b], (deliv[(size_t)b] / cf + 1) * cf);
            }
            pcm_ptr[slots.size()] = chunk_pcm.data() + slots.size() * (size_t)cap.floats;
            final_frames[slots.size()] = fin ? s.n_frames : -1;
            slots.push_back(b);
        }
        if (slots.empty()) return false;
        e.slots_codec_decode_new((int)slots.size(), slots.data(), pcm_ptr.data(), cap.deliver, plen.data(), fb.data(), fe.data(), live_text ? flim.data() : nullptr,
                                 final_frames.data());
        for (size_t i = 0; i < slots.size(); ++i) {
            const int b = slots[i], u = slot_utt[(size_t)b];
            const SlotState& s = st[(size_t)b];
            // live text: finished AND its last frames are in this round; without live text fe[i] is always the frame count
            const bool fin = (s.finished || s.n_frames >= s.max_frames) && (!live_text || fe[i] >= s.n_frames);
            deliv[(size_t)b] = fe[i];
            held[(size_t)b] = fin ? 0 : s.n_frames - fe[i];
            if (plen[i] > cap.deliver) throw Error("synthesize_stream: a chunk produced more samples than its buffer holds");
            if (a.pcm_out && a.pcm_out[u] && plen[i] > 0 && written[(size_t)u] < a.pcm_cap)
                memcpy(a.pcm_out[u] + written[(size_t)u], pcm_ptr[i], (size_t)std::min(plen[i], a.pcm_cap - written[(size_t)u]) * sizeof(float));
            written[(size_t)u] += plen[i];
            if (fin) {   // retired before the callback: whatever it does, the slot is free and the outputs are complete
                if (a.n_frames) a.n_frames[u] = s.n_frames;
                if (a.pcm_len) a.pcm_len[u] = written[(size_t)u];
                retire(b);
                deliv[(size_t)b] = 0;
            }
            if (plen[i] > 0 || fin)
                if ((sunk ? sink.cb(sink.user, u, fb[i], fe[i], pcm_ptr[i], plen[i], fin ? 1 : 0) : a.cb(a.user, u, fb[i], fe[i], pcm_ptr[i], plen[i], fin ? 1 : 0)) != 0)
                    throw Error("cancelled by callback");
        }
        return true;
    };
    try {
        while (!pending.empty() || live > 0) {
            bool skip_decode = false;
            if (live_text) {   // poll every utterance whose text is open, live or queued
                for (int u = 0; u < n_utt; ++u) {
                    if (t_closed[(size_t)u]) continue;
                    bool known = false;
                    for (int b = 0; b < B && !known; ++b) known = slot_utt[(size_t)b] == u;
                    for (size_t i = 0; i < pending.size() && !known; ++i) known = pending[i] == u;
                    if (!known) continue;
                    int32_t n_new = 0, cl = 0;
                    t_gave[(size_t)u] = 0;
                    if (a.text_cb(a.text_user, u, poll_ids.data(), (int)poll_ids.size(), &n_new, &cl) != 0) throw Error("cancelled by callback");
                    if (n_new < 0 || n_new > (int)poll_ids.size()) throw Error("synthesize_live: the text callback returned a bad id count");
                    got[(size_t)u].insert(got[(size_t)u].end(), poll_ids.begin(), poll_ids.begin() + n_new);
                    t_gave[(size_t)u] = n_new > 0 || cl;
                    if (cl) {
                        t_closed[(size_t)u] = 1;
                        if (got[(size_t)u].size() < 4) throw Error("token sequence too short: need at least 4 ids (the reference indexes input_ids[3])");
                    }
                }
            }
            size_t n_ready = 0;   // queued utterances, from the front, that hold enough text to begin
            while (n_ready < pending.size() && admissible(pending[n_ready])) ++n_ready;
            // admission in queue order, every utterance with the pages of its whole length
            admit(n_ready, true, [&](int u) { return e.kv_pages_for(ctx_of(u) + cap_of(u)); });
            if (live_text && !fresh.empty()) {   // the prompts of this look's admissions, from the ids they hold now (build_prompt_open)
                prompts.assign(fresh.size() * 16 * (size_t)H, 0.f);
                size_t trow = 0;
                for (size_t i = 0; i < fresh.size(); ++i) { prep[(size_t)slot_utt[(size_t)fresh[i]]].toff = trow; trow += (size_t)std::max(1, usable(slot_utt[(size_t)fresh[i]]) - 4); }
                trailing.assign(trow * (size_t)H, 0.f);
                for (size_t i = 0; i < fresh.size(); ++i) {
                    const int u = slot_utt[(size_t)fresh[i]], nu = usable(u);
                    Prep& pr = prep[(size_t)u];
                    pr.poff = i * 16;
                    e.build_prompt_open(got[(size_t)u].data(), nu, a.lang, a.speakers ? a.speakers[u] : nullptr, prompts.data() + pr.poff * H, &pr.S,
                                        trailing.data() + pr.toff * H, e.max_trailing, &pr.nt);
                    t_fed[(size_t)u] = nu;
                }
            }
            arm([](int) { return 0; });   // prompt + cap, reserved now
            if (P > 0 && !fresh.empty()) {   // the vocoder streams of the look's prefixed slots take their prefixes as history, in one call: audio starts at the first new frame
                std::vector<int32_t> ps_slots, ps_n;
                for (int b : fresh) if (pf(slot_utt[(size_t)b]) > 0) { ps_slots.push_back(b); ps_n.push_back(pf(slot_utt[(size_t)b])); }
                if (!ps_slots.empty()) e.slots_codec_prime((int)ps_slots.size(), ps_slots.data(), ps_n.data());
            }
            if (live_text) {
                for (int b : fresh) { e.slot_text_open(b); tl_host[(size_t)b] = prep[(size_t)slot_utt[(size_t)b]].nt; nf_host[(size_t)b] = 0; }
                // the new ids of every live slot, and the close of those whose source is done, in one call
                app_slots.clear(); app_ids.clear(); app_off.assign(1, 0); app_close.clear();
                for (int b = 0; b < B; ++b) {
                    const int u = slot_utt[(size_t)b];
                    if (u < 0 || t_sealed[(size_t)u]) continue;
                    const int nu = usable(u);
                    if (nu == t_fed[(size_t)u] && !t_closed[(size_t)u]) continue;
                    app_slots.push_back(b);
                    app_ids.insert(app_ids.end(), got[(size_t)u].begin() + t_fed[(size_t)u], got[(size_t)u].begin() + nu);
                    app_off.push_back((int32_t)app_ids.size());
                    app_close.push_back(t_closed[(size_t)u]);
                    tl_host[(size_t)b] += nu - t_fed[(size_t)u] + (t_closed[(size_t)u] ? 1 : 0);
                    t_fed[(size_t)u] = nu;
                    if (t_closed[(size_t)u]) t_sealed[(size_t)u] = 1;
                }
                if (!app_slots.empty()) e.slots_text_append((int)app_slots.size(), app_slots.data(), nullptr, app_ids.data(), app_off.data(), app_close.data());
                if (live == 0) {
                    if (n_ready > 0) throw Error("synthesize_stream: no utterance could be admitted");
                    continue;   // every queued utterance waits for text: poll again
                }
                bool all_starved = true;
                for (int b = 0; b < B && all_starved; ++b) {
                    const int u = slot_utt[(size_t)b];
                    if (u >= 0 && (t_sealed[(size_t)u] || nf_host[(size_t)b] < tl_host[(size_t)b])) all_starved = false;
                }
                bool any_held = false;   // frames generated but not delivered yet (held for the chunk cadence, below)
                for (int b = 0; b < B; ++b) if (slot_utt[(size_t)b] >= 0 && held[(size_t)b] > 0) any_held = true;
                if (all_starved && !any_held) continue;   // nothing would move: poll again at once
                skip_decode = all_starved;                // no step would move a slot, but a silent source releases the held frames
            }
            if (live == 0) throw Error("synthesize_stream: no utterance could be admitted");
            if (!skip_decode) e.decode_steps(a.chunk_frames);
            e.slots_state(B, st);
            if (live_text) plan_delivery();
            for (bool first = true; deliver_round(first) && live_text; first = false) { }
        }
    } catch (...) {
        release_all();
        throw;
    }
}

// A job without utterances is done; one that lacks its texts (ids and offsets, or the text callback of q3tts_synthesize_live_host) or its
// sampling is refused, by both loops alike
static bool job_present(const JobArgs& a) {
    if (a.n_utt > 0 && ((!a.text_cb && (!a.ids || !a.offsets)) || !a.p)) throw Error("synthesize: null argument");
    return a.n_utt > 0;
}
void job_offline(Engine& e, const JobArgs& a) { if (job_present(a)) Job(e, a).offline(); }
void job_stream(Engine& e, const JobArgs& a) { if (job_present(a)) Job(e, a).stream(); }

} // namespace q3
