// q3_speaker.cpp — ECAPA-TDNN speaker encoder on the GPU (voice-clone path).
// Replaces run_speaker_encoder (reference src/tts_onnx.cpp:367-403, an ORT session over speaker_encoder.onnx).
// Network [HINT: transformers qwen2_5_omni ECAPA_TimeDelayNet], pinned by tests/golden/hf_speaker.npz through the
// oracle: TDNN(k5) -> 3 x SE-Res2Net(k3, dilation 2/3/4) -> concat -> TDNN(k1) -> attentive statistics pooling -> 1x1.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

struct SpkConv {
    float* w = nullptr;       // [k][Cin][Cout]
    const float* b = nullptr;
    int cin = 0, cout = 0, k = 1;
};
// Weights only: the repacked convs live in the engine's WeightSet (their storage in its allocs), every holder's `spk` points at them.
struct SpeakerW {
    SpkConv tdnn0, tdnn1[3], res[3][16], tdnn2[3], se1[3], se2[3], mfa, asp_tdnn, asp_conv, fc;
};
void speaker_weights_free(SpeakerW* w) { delete w; }

// GPU front end of the clone path (in-memory audio -> resample -> log-mel -> batched encoder): the extractor's tables on the device,
// one pinned staging buffer and one device workspace, both grow-only, owned by the engine and freed with it.  The tables themselves
// are the set's (WeightSet::mel_tables_d): tb is this engine's view of them.
struct SpkFront {
    MelTablesDev tb;
    char* ws = nullptr; size_t ws_cap = 0;
    char* pin = nullptr; size_t pin_cap = 0;
};
// Device workspace of one group of clips (resampled audio, mel, encoder activations: ~46 KB per mel frame at 0.6B dims).  A batch that
// needs more is processed in consecutive groups, one after the other on the stream in the same memory; a clip's result does not depend
// on the grouping.  A single clip is never split (16384 frames stay below the bound).
static constexpr size_t kSpkWorkspaceMaxBytes = (size_t)1 << 30;
static constexpr int kSpkGroupMaxRows = 65535 * 16;   // the row-wise convolutions put 16 rows of a group on one blockIdx.y
static constexpr size_t kAlign = 256;
static size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

void Engine::speaker_free() {
    spk = nullptr;   // the set's
    if (spkf) {
        if (spkf->ws) (void)hipFree(spkf->ws);
        if (spkf->pin) (void)hipHostFree(spkf->pin);
        delete spkf;
        spkf = nullptr;
    }
}

// make_plan's tables (q3_audio.cpp: double -> float, single-precision corner arithmetic) uploaded once; k_logmel recomputes none of them
void Engine::front_finalize() {
    if (spkf) return;
    const MelPlan p = make_plan(MelSpec());
    if (p.n != 1024 || p.spec.win != 1024 || p.spec.hop != 256 || p.spec.n_mels != 128 || p.bins != 513) throw Error("log-mel kernel: built for n_fft = win = 1024, hop 256, 128 bands");
    for (int m = 0; m < 128; ++m)
        if (p.lo[(size_t)m] < 0 || p.lo[(size_t)m] > p.mid[(size_t)m] || p.mid[(size_t)m] > p.hi[(size_t)m] || p.hi[(size_t)m] > 512) throw Error("log-mel kernel: triangle corner outside the kept bins");
    for (int i = 0; i < 1024; ++i)
        if (p.rev[(size_t)i] >= 1024u) throw Error("log-mel kernel: bit-reversal index out of range");
    std::vector<uint32_t> h(1024 + 512 + 512 + 1024 + 3 * 128);
    memcpy(&h[0], p.window.data(), 1024 * 4);
    memcpy(&h[1024], p.tw_re.data(), 512 * 4);
    memcpy(&h[1536], p.tw_im.data(), 512 * 4);
    memcpy(&h[2048], p.rev.data(), 1024 * 4);
    memcpy(&h[3072], p.lo.data(), 128 * 4);
    memcpy(&h[3200], p.mid.data(), 128 * 4);
    memcpy(&h[3328], p.hi.data(), 128 * 4);
    ws.build_once([&] { return ws.mel_tables_d != nullptr; }, [&]() -> int64_t {   // once per set; the copy is synchronous
        void* t = nullptr;
        Q3_HIP_CHECK(hipMalloc(&t, h.size() * 4));
        if (hipMemcpy(t, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(t); throw Error("log-mel tables: upload failed"); }
        ws.mel_tables_d = t; ws.mel_bytes = (int64_t)(h.size() * 4);
        return ws.mel_bytes;
    });
    spkf = new SpkFront();
    const uint32_t* d = (const uint32_t*)ws.mel_tables_d;
    spkf->tb.window = (const float*)d; spkf->tb.tw_re = (const float*)(d + 1024); spkf->tb.tw_im = (const float*)(d + 1536);
    spkf->tb.rev = d + 2048;
    spkf->tb.lo = (const int32_t*)(d + 3072); spkf->tb.mid = (const int32_t*)(d + 3200); spkf->tb.hi = (const int32_t*)(d + 3328);
}

void Engine::speaker_finalize() {
    front_finalize();
    if (!has_speaker()) return;
    if (!ws.spk) ws.spk = new SpeakerW();
    spk = ws.spk;
    auto pack = [&](SpkConv& cv, const std::string& n) {
        const Tensor& w = T(n + ".w");
        cv.cout = (int)w.shape[0]; cv.cin = (int)w.shape[1]; cv.k = (int)w.shape[2];
        if (!cv.w) cv.w = (float*)ws.dmalloc((size_t)w.numel * sizeof(float));
        launch_spk_repack((const float*)w.dev, cv.w, cv.cout, cv.cin, cv.k, stream);
        cv.b = (const float*)T(n + ".b").dev;
    };
    pack(spk->tdnn0, "spk.tdnn0");
    for (int i = 0; i < 3; ++i) {
        const std::string p = "spk.blocks." + std::to_string(i) + ".";
        pack(spk->tdnn1[i], p + "tdnn1");
        for (int j = 0; j < c.spk_scale - 1; ++j) pack(spk->res[i][j], p + "res2net." + std::to_string(j));
        pack(spk->tdnn2[i], p + "tdnn2");
        pack(spk->se1[i], p + "se1");
        pack(spk->se2[i], p + "se2");
    }
    pack(spk->mfa, "spk.mfa");
    pack(spk->asp_tdnn, "spk.asp.tdnn");
    pack(spk->asp_conv, "spk.asp.conv");
    pack(spk->fc, "spk.fc");
}

void Engine::speaker_encode(const float* mel, int T_, float* out) {
    if (!has_speaker()) throw Error("model has no speaker encoder");
    if (!finalized || !spk) throw Error("weights not finalized");
    if (T_ < 5) throw Error("speaker encoder needs at least 5 mel frames (reflect padding), got " + std::to_string(T_));
    if (T_ > 16384) throw Error("reference clip too long for the speaker encoder (more than 16384 mel frames)");
    const int T = T_, SC = c.spk_channels, sub = SC / c.spk_scale, C3 = 3 * SC;
    // one arena per call: the encoder runs once per cloned voice
    const size_t n_floats = (size_t)c.spk_mel * T + (size_t)T * (4 * SC + 2 * C3 + 3 * C3 + c.spk_att + C3) + 2 * SC + c.spk_se + 2 * C3 + 2 * C3 + c.spk_enc_dim + 64;
    float* arena = nullptr;
    Q3_HIP_CHECK(hipMalloc((void**)&arena, n_floats * sizeof(float)));
    struct Free { float* p; ~Free() { (void)hipFree(p); } } guard{ arena };
    float* cur = arena;
    auto take = [&](size_t n) { float* p = cur; cur += n; return p; };
    float* mel_d = take((size_t)c.spk_mel * T);
    float* h = take((size_t)T * SC);
    float* a = take((size_t)T * SC);
    float* r2 = take((size_t)T * SC);
    float* y = take((size_t)T * SC);
    float* cat = take((size_t)T * C3);
    float* mf = take((size_t)T * C3);
    float* att_in = take((size_t)T * 3 * C3);
    float* at = take((size_t)T * c.spk_att);
    float* sc = take((size_t)T * C3);
    float* mean = take(SC);
    float* gate = take(SC);
    float* s1 = take(c.spk_se);
    float* mu3 = take(C3);
    float* sd3 = take(C3);
    float* pooled = take(2 * C3);
    float* out_d = take(c.spk_enc_dim);
    Q3_HIP_CHECK(hipMemcpyAsync(mel_d, mel, (size_t)c.spk_mel * T * sizeof(float), hipMemcpyHostToDevice, stream));

    auto conv = [&](const SpkConv& cv, const float* x, int ldx, const float* x2, int ldx2, int Tn, int dil, int act, float* yo, int ldy, int chan_major = 0) {
        SpkConvArgs g;
        g.x = x; g.ldx = ldx; g.x2 = x2; g.ldx2 = ldx2; g.x_channel_major = chan_major;
        g.T = Tn; g.Cin = cv.cin; g.Cout = cv.cout; g.k = cv.k; g.dil = dil; g.act = act; g.W = cv.w; g.bias = cv.b; g.y = yo; g.ldy = ldy;
        launch_spk_conv(g, stream);
    };
    conv(spk->tdnn0, mel_d, T, nullptr, 0, T, 1, 1, h, SC, 1);
    for (int i = 0; i < 3; ++i) {
        conv(spk->tdnn1[i], h, SC, nullptr, 0, T, 1, 1, a, SC);
        // Res2Net: chunk 0 passes through, chunk 1 = f(chunk 1), chunk j = f(chunk j + out j-1)
        Q3_HIP_CHECK(hipMemcpy2DAsync(r2, (size_t)SC * sizeof(float), a, (size_t)SC * sizeof(float), (size_t)sub * sizeof(float), (size_t)T, hipMemcpyDeviceToDevice, stream));
        for (int j = 1; j < c.spk_scale; ++j)
            conv(spk->res[i][j - 1], a + (size_t)j * sub, SC, j >= 2 ? r2 + (size_t)(j - 1) * sub : nullptr, SC, T, i + 2, 1, r2 + (size_t)j * sub, SC);
        conv(spk->tdnn2[i], r2, SC, nullptr, 0, T, 1, 1, y, SC);
        launch_spk_colstats(y, SC, T, SC, mean, nullptr, stream);
        conv(spk->se1[i], mean, SC, nullptr, 0, 1, 1, 1, s1, c.spk_se);
        conv(spk->se2[i], s1, c.spk_se, nullptr, 0, 1, 1, 0, gate, SC);
        launch_spk_se_gate(y, gate, h, cat + (size_t)i * SC, C3, T, SC, stream);
    }
    conv(spk->mfa, cat, C3, nullptr, 0, T, 1, 1, mf, C3);
    launch_spk_colstats(mf, C3, T, C3, mu3, sd3, stream);
    launch_spk_asp_input(mf, mu3, sd3, att_in, T, C3, stream);
    conv(spk->asp_tdnn, att_in, 3 * C3, nullptr, 0, T, 1, 2, at, c.spk_att);
    conv(spk->asp_conv, at, c.spk_att, nullptr, 0, T, 1, 0, sc, C3);
    launch_spk_asp_pool(sc, mf, T, C3, pooled, stream);
    conv(spk->fc, pooled, 2 * C3, nullptr, 0, 1, 1, 0, out_d, c.spk_enc_dim);
    Q3_HIP_CHECK(hipMemcpyAsync(out, out_d, (size_t)c.spk_enc_dim * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
}

// ---------------------------------------------------------------------------------------------
// In-memory audio -> embeddings.  Host side: lengths by q3_audio.cpp's own expressions, one table of SpkClip per call.
// ---------------------------------------------------------------------------------------------
namespace {

// resample_linear's output length and log_mel's frame count for a clip of n samples
int64_t resampled_len(int64_t n, int src_rate, int dst_rate) {
    if (src_rate == dst_rate || n == 0) return n;
    const double ratio = (double)dst_rate / src_rate;
    return (int64_t)(size_t)((double)(size_t)n * ratio);
}
int64_t mel_frames(int64_t n24) {
    const MelSpec spec;
    return n24 <= 0 ? 0 : (n24 < spec.win ? 1 : (n24 - spec.win) / spec.hop + 1);
}

struct Carve {   // sub-buffers of a workspace, each aligned
    char* base; size_t used = 0;
    explicit Carve(char* b) : base(b) {}
    float* take(size_t n_floats) { float* p = (float*)(base + used); used += aligned(n_floats * sizeof(float)); return p; }
};

} // namespace

// Staging layout, the same on the host (pinned) and at the start of the device workspace: [SpkClip table][raw audio of every clip].
// Grows the two buffers (no work of this engine's stream is in flight between calls: every call ends with a sync), fills the staging
// buffer, and enqueues the one upload.  `more_bytes`: workspace needed behind the staged part.
static void front_stage(Engine& e, std::vector<SpkClip>& clips, const float* const* pcm, size_t more_bytes, const SpkClip** clips_d, const float** raw_d, char** rest) {
    SpkFront& f = *e.spkf;
    const size_t table_b = aligned(clips.size() * sizeof(SpkClip));
    size_t total_in = 0;
    for (SpkClip& c : clips) {
        if (total_in + (size_t)c.n_in > (size_t)INT32_MAX) throw Error("reference audio: more than 2^31 samples in one call");
        c.in_off = (int32_t)total_in;
        total_in += (size_t)c.n_in;
    }
    const size_t staged = table_b + aligned(total_in * sizeof(float));
    if (f.pin_cap < staged) {
        if (f.pin) (void)hipHostFree(f.pin);
        f.pin = nullptr; f.pin_cap = 0;
        Q3_HIP_CHECK(hipHostMalloc((void**)&f.pin, staged));
        f.pin_cap = staged;
    }
    if (f.ws_cap < staged + more_bytes) {
        if (f.ws) (void)hipFree(f.ws);
        f.ws = nullptr; f.ws_cap = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&f.ws, staged + more_bytes));
        f.ws_cap = staged + more_bytes;
    }
    memcpy(f.pin, clips.data(), clips.size() * sizeof(SpkClip));
    for (size_t i = 0; i < clips.size(); ++i) memcpy(f.pin + table_b + (size_t)clips[i].in_off * sizeof(float), pcm[i], (size_t)clips[i].n_in * sizeof(float));
    Q3_HIP_CHECK(hipMemcpyAsync(f.ws, f.pin, table_b + total_in * sizeof(float), hipMemcpyHostToDevice, e.stream));
    *clips_d = (const SpkClip*)f.ws;
    *raw_d = (const float*)(f.ws + table_b);
    *rest = f.ws + staged;
}

int64_t Engine::resample_gpu(const float* in, int64_t n, int src_rate, int dst_rate, float* out, int64_t cap) {
    if (n < 0 || (n > 0 && !in) || src_rate < 1 || dst_rate < 1) throw Error("resample: needs n >= 0 samples and positive rates");
    if (n > INT32_MAX / 2) throw Error("resample: more than 2^30 samples");
    const int64_t n_out = resampled_len(n, src_rate, dst_rate);
    if (n_out > INT32_MAX / 2) throw Error("resample: more than 2^30 output samples");
    const int64_t n_copy = out ? std::min(n_out, std::max<int64_t>(cap, 0)) : 0;
    if (n_copy == 0) return n_out;
    if (src_rate == dst_rate) { memcpy(out, in, (size_t)n_copy * sizeof(float)); return n_out; }   // the input as it is, like the host
    if (!spkf) front_finalize();
    std::vector<SpkClip> clips(1);
    clips[0].n_in = (int32_t)n; clips[0].src_rate = src_rate; clips[0].dst_rate = dst_rate; clips[0].n_rs = (int32_t)n_out;
    const SpkClip* clips_d; const float* raw_d; char* rest;
    front_stage(*this, clips, &in, aligned((size_t)n_out * sizeof(float)), &clips_d, &raw_d, &rest);
    launch_resample_linear(raw_d, (float*)rest, clips_d, 1, (int)n_out, stream);
    Q3_HIP_CHECK(hipMemcpyAsync(out, rest, (size_t)n_copy * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    return n_out;
}

bool Engine::mel_gpu(const float* audio, int64_t n, int sample_rate, float* mel, int64_t cap, int* frames) {
    if (n < 0 || (n > 0 && !audio) || sample_rate < 1 || !frames) throw Error("log-mel: needs n >= 0 samples, a positive rate and a frame-count pointer");
    if (n > INT32_MAX / 2) throw Error("log-mel: more than 2^30 samples");
    if (!finalized || !spkf) throw Error("weights not finalized");
    const int64_t n24 = resampled_len(n, sample_rate, 24000);
    if (n24 > INT32_MAX / 2) throw Error("log-mel: more than 2^30 samples at 24 kHz");
    const int64_t T = mel_frames(n24);
    *frames = (int)T;
    if (T == 0) return false;
    if (!mel) return true;
    if (cap < 128 * T) throw Error("log-mel: output buffer too small for 128 x " + std::to_string(T) + " values");
    std::vector<SpkClip> clips(1);
    clips[0].n_in = (int32_t)n; clips[0].src_rate = sample_rate; clips[0].dst_rate = 24000; clips[0].n_rs = (int32_t)n24; clips[0].T = (int32_t)T;
    const bool rs = sample_rate != 24000;
    const SpkClip* clips_d; const float* raw_d; char* rest;
    front_stage(*this, clips, &audio, aligned(rs ? (size_t)n24 * sizeof(float) : 0) + aligned((size_t)128 * T * sizeof(float)), &clips_d, &raw_d, &rest);
    Carve cv(rest);
    float* rs_d = cv.take(rs ? (size_t)n24 : 0);
    float* mel_d = cv.take((size_t)128 * T);
    if (rs) launch_resample_linear(raw_d, rs_d, clips_d, 1, (int)n24, stream);
    launch_logmel(raw_d, rs_d, clips_d, 1, (int)T, spkf->tb, mel_d, stream);
    Q3_HIP_CHECK(hipMemcpyAsync(mel, mel_d, (size_t)128 * T * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    return true;
}

void Engine::speaker_embed_pcm(int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* rates, float* out) {
    if (!has_speaker()) throw Error("model has no speaker encoder");
    if (!finalized || !spk || !spkf) throw Error("weights not finalized");
    if (n_clips < 1) throw Error("speaker embeddings: n_clips must be at least 1, got " + std::to_string(n_clips));
    if (!pcm || !n_samples || !rates || !out) throw Error("speaker embeddings: NULL argument");
    if (c.spk_mel != 128) throw Error("speaker embeddings: the log-mel kernel produces 128 bands, the model wants " + std::to_string(c.spk_mel));
    const int SC = c.spk_channels, sub = SC / c.spk_scale, C3 = 3 * SC, ED = c.spk_enc_dim;
    // everything is validated before the first byte moves: a refused call leaves `out` and the engine untouched
    std::vector<SpkClip> clips((size_t)n_clips);
    for (int i = 0; i < n_clips; ++i) {
        const std::string who = "clip " + std::to_string(i) + ": ";
        if (!pcm[i]) throw Error(who + "NULL audio pointer");
        if (n_samples[i] < 1) throw Error(who + "n_samples must be at least 1, got " + std::to_string(n_samples[i]));
        if (rates[i] < 1) throw Error(who + "sample_rate must be at least 1, got " + std::to_string(rates[i]));
        if (n_samples[i] > INT32_MAX / 2) throw Error(who + "more than 2^30 samples");
        const int64_t n24 = resampled_len(n_samples[i], rates[i], 24000), T = mel_frames(n24);
        if (T < 5) throw Error(who + "speaker encoder needs at least 5 mel frames (reflect padding), got " + std::to_string(T));
        if (T > 16384) throw Error(who + "reference clip too long for the speaker encoder (more than 16384 mel frames)");
        SpkClip& cl = clips[(size_t)i];
        cl.n_in = (int32_t)n_samples[i]; cl.src_rate = rates[i]; cl.dst_rate = 24000; cl.n_rs = (int32_t)n24; cl.T = (int32_t)T;
    }
    // consecutive groups under the workspace bound (Q3TTS_SPK_WS_MAX_BYTES on a test-hook engine lowers it: tests/test_gpu_clone_frontend.py)
    size_t bound = kSpkWorkspaceMaxBytes;
    if (const char* kb = knob("Q3TTS_SPK_WS_MAX_BYTES")) bound = (size_t)std::max(1ll, atoll(kb));
    const size_t per_frame = (size_t)c.spk_mel + 4 * (size_t)SC + 2 * (size_t)C3 + 3 * (size_t)C3 + (size_t)c.spk_att + (size_t)C3;
    const size_t per_clip = 2 * (size_t)SC + (size_t)c.spk_se + 2 * (size_t)C3 + 2 * (size_t)C3;
    const size_t slack = 24 * kAlign;   // the alignment padding of a group's sub-buffers
    auto clip_bytes = [&](const SpkClip& cl) {
        return ((cl.src_rate != cl.dst_rate ? (size_t)cl.n_rs : 0) + (size_t)cl.T * per_frame + per_clip) * sizeof(float);
    };
    struct Group { int first, n, sumT, maxT, minT, max_rs; size_t sum_rs, bytes; };
    std::vector<Group> groups;
    for (int i = 0; i < n_clips; ++i) {
        SpkClip& cl = clips[(size_t)i];
        const size_t b = clip_bytes(cl);
        if (groups.empty() || groups.back().bytes + b > bound || groups.back().sumT + cl.T > kSpkGroupMaxRows) groups.push_back(Group{ i, 0, 0, 0, 1 << 30, 0, 0, slack });
        Group& g = groups.back();
        cl.row_off = g.sumT;
        const bool rs = cl.src_rate != cl.dst_rate;
        cl.rs_off = (int32_t)g.sum_rs;
        if (rs) { g.sum_rs += (size_t)cl.n_rs; g.max_rs = std::max(g.max_rs, (int)cl.n_rs); }
        if (g.sum_rs > (size_t)INT32_MAX || (size_t)g.sumT + (size_t)cl.T > (size_t)(INT32_MAX / 128)) throw Error("speaker embeddings: a workspace group exceeds 2^31 samples; lower the bound");
        g.n += 1; g.sumT += cl.T; g.maxT = std::max(g.maxT, (int)cl.T); g.minT = std::min(g.minT, (int)cl.T); g.bytes += b;
    }
    size_t group_bytes = 0;
    for (const Group& g : groups) group_bytes = std::max(group_bytes, g.bytes);
    const SpkClip* clips_d; const float* raw_d; char* rest;
    front_stage(*this, clips, pcm, aligned((size_t)n_clips * ED * sizeof(float)) + group_bytes, &clips_d, &raw_d, &rest);
    float* out_d = (float*)rest;
    char* group_base = rest + aligned((size_t)n_clips * ED * sizeof(float));

    for (const Group& g : groups) {
        const int n = g.n, R = g.sumT;
        const SpkClip* gc = clips_d + g.first;
        Carve cv(group_base);
        float* rs_d = cv.take(g.sum_rs);
        float* mel_d = cv.take((size_t)c.spk_mel * R);
        float* h = cv.take((size_t)R * SC);
        float* a = cv.take((size_t)R * SC);
        float* r2 = cv.take((size_t)R * SC);
        float* y = cv.take((size_t)R * SC);
        float* cat = cv.take((size_t)R * C3);
        float* mf = cv.take((size_t)R * C3);
        float* att_in = cv.take((size_t)R * 3 * C3);
        float* at = cv.take((size_t)R * c.spk_att);
        float* sc = cv.take((size_t)R * C3);
        float* mean = cv.take((size_t)n * SC);
        float* gate = cv.take((size_t)n * SC);
        float* s1 = cv.take((size_t)n * c.spk_se);
        float* mu3 = cv.take((size_t)n * C3);
        float* sd3 = cv.take((size_t)n * C3);
        float* pooled = cv.take((size_t)n * 2 * C3);
        if (cv.used > g.bytes) throw Error("speaker embeddings: workspace accounting");   // 17 sub-buffers, each padded by less than kAlign

        if (g.max_rs > 0) launch_resample_linear(raw_d, rs_d, gc, n, g.max_rs, stream);
        launch_logmel(raw_d, rs_d, gc, n, g.maxT, spkf->tb, mel_d, stream);
        // Convolutions across time (k > 1) take the clip from the grid; k = 1 convolutions and the per-clip vectors are plain row-wise
        // products, so they run over all rows of the group at once: a row's sum does not depend on its tile or on its neighbours.
        auto conv = [&](const SpkConv& cv_, const float* x, int ldx, const float* x2, int ldx2, int rows, int dil, int act, float* yo, int ldy, int chan_major = 0) {
            SpkConvArgs q;
            q.x = x; q.ldx = ldx; q.x2 = x2; q.ldx2 = ldx2; q.x_channel_major = chan_major;
            q.T = rows; q.Cin = cv_.cin; q.Cout = cv_.cout; q.k = cv_.k; q.dil = dil; q.act = act; q.W = cv_.w; q.bias = cv_.b; q.y = yo; q.ldy = ldy;
            if (cv_.k > 1 || chan_major) { q.clips = gc; q.n_clips = n; q.T = g.maxT; q.min_T = g.minT; }
            launch_spk_conv(q, stream);
        };
        conv(spk->tdnn0, mel_d, 0, nullptr, 0, R, 1, 1, h, SC, 1);
        for (int i = 0; i < 3; ++i) {
            conv(spk->tdnn1[i], h, SC, nullptr, 0, R, 1, 1, a, SC);
            Q3_HIP_CHECK(hipMemcpy2DAsync(r2, (size_t)SC * sizeof(float), a, (size_t)SC * sizeof(float), (size_t)sub * sizeof(float), (size_t)R, hipMemcpyDeviceToDevice, stream));
            for (int j = 1; j < c.spk_scale; ++j)
                conv(spk->res[i][j - 1], a + (size_t)j * sub, SC, j >= 2 ? r2 + (size_t)(j - 1) * sub : nullptr, SC, R, i + 2, 1, r2 + (size_t)j * sub, SC);
            conv(spk->tdnn2[i], r2, SC, nullptr, 0, R, 1, 1, y, SC);
            launch_spk_colstats(y, SC, g.maxT, SC, mean, nullptr, stream, gc, n);
            conv(spk->se1[i], mean, SC, nullptr, 0, n, 1, 1, s1, c.spk_se);
            conv(spk->se2[i], s1, c.spk_se, nullptr, 0, n, 1, 0, gate, SC);
            launch_spk_se_gate(y, gate, h, cat + (size_t)i * SC, C3, g.maxT, SC, stream, gc, n);
        }
        conv(spk->mfa, cat, C3, nullptr, 0, R, 1, 1, mf, C3);
        launch_spk_colstats(mf, C3, g.maxT, C3, mu3, sd3, stream, gc, n);
        launch_spk_asp_input(mf, mu3, sd3, att_in, g.maxT, C3, stream, gc, n);
        conv(spk->asp_tdnn, att_in, 3 * C3, nullptr, 0, R, 1, 2, at, c.spk_att);
        conv(spk->asp_conv, at, c.spk_att, nullptr, 0, R, 1, 0, sc, C3);
        launch_spk_asp_pool(sc, mf, g.maxT, C3, pooled, stream, gc, n);
        conv(spk->fc, pooled, 2 * C3, nullptr, 0, n, 1, 0, out_d + (size_t)g.first * ED, ED);
    }
    Q3_HIP_CHECK(hipMemcpyAsync(out, out_d, (size_t)n_clips * ED * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
}

} // namespace q3
