// q3_encoder.cpp — the 12 Hz speech tokenizer's encoder on the GPU: audio -> codes, the producer of what q3tts_slot_begin_codes
// consumes (the reference has no encoder; its clone path stops at the x-vector, tts_onnx.cpp:331-365).
// Network [HINT: transformers MimiModel.encode, the first n_groups quantizers], pinned by tests/golden/hf_mimi_encoder.npz through
// tests/mimi_ref.py: SEANet encoder (causal Conv1d: left pad (k - 1) dil + 1 - stride zeros, right pad just enough zeros to complete
// the last output, so n samples give ceil(n / 1920) frames) -> transformer at 25 Hz (LayerNorm, RoPE, causal window, LayerScale, GELU
// MLP) -> conv k4 stride 2 with replicate padding -> split residual VQ (1 semantic + n_groups - 1 acoustic levels).
// All fp32.  A batch is one set of launches per group of clips (EncSpan tables, one per rate level); a clip's result does not depend
// on the rest of the batch.  Workspace: grow-only, owned by the engine, freed with it; a clip is capped at kEncMaxClipSamples.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "q3_audio.h"
#include "q3_engine.h"

namespace q3 {

struct EncConvW {
    float* w = nullptr;        // [k][cout][cin] (packed copy, or the registry tensor itself when k == 1)
    const float* b = nullptr;
    int cin = 0, cout = 0, k = 1;
    bool owned = false;
};
struct EncLayerW {
    const float *ln1w = nullptr, *ln1b = nullptr, *qkv = nullptr, *o = nullptr, *s1 = nullptr;
    const float *ln2w = nullptr, *ln2b = nullptr, *fc1 = nullptr, *fc2 = nullptr, *s2 = nullptr;
};
// One audio stream's carried state.  rows[l]: rows emitted so far at rate level l (0 = samples received, l = 1 .. nr
// behind stage l - 1, nr + 1 = frames).  buf: the stream's carry rings, one per conv with k > 1 (k - 1 raw input rows, before ELU)
// and one per transformer layer ([window - 1][2 AO]: rotated K, then V); absolute row r of a ring's input sits in slot r mod cap.
// A stream at another rate or sample format than 24 kHz float resamples on the way in: rows[0] then counts the 24 kHz
// samples fed to the encoder, n_raw the stream's own samples received, and behind the rings buf holds two carry buffers of
// kEncCarryFloats floats: the last min(carry_len, n_raw) raw samples, as floats, are in buffer carry_cur; a push writes the other one.
struct EncStream {
    bool open = false, finished = false;
    int64_t max_samples = 0, rows[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float* buf = nullptr; size_t buf_floats = 0;
    int rate = 24000, format = Q3TTS_PCM_F32, carry_len = 0, carry_cur = 0;
    int64_t n_raw = 0;
    size_t carry_off = 0;   // the first carry buffer's first float in buf
    bool plain() const { return rate == 24000 && format == Q3TTS_PCM_F32; }
};
static constexpr size_t kEncCarryFloats = 64;   // a carry buffer: ceil(384000 / 24000) + 1 = 17 samples at most, one 256-byte line
// The weight half, in the engine's WeightSet: repacked convs, layer pointers, codebooks.
struct EncWeights {
    EncConvW conv_in, res1[4], res2[4], down[4], conv_out, ds;
    std::vector<EncLayerW> layers;
    const float *proj_sem = nullptr, *proj_ac = nullptr;
    float* books = nullptr;                    // [n_groups][codebook][vq_dim], the level tables back to back
    int64_t bytes = 0;                         // HBM of the owned copies (counted in the set's bytes)
};
void encoder_weights_free(EncWeights* w) {
    if (!w) return;
    if (w->books) (void)hipFree(w->books);
    auto drop = [](EncConvW& cv) { if (cv.owned && cv.w) (void)hipFree(cv.w); cv.w = nullptr; };
    drop(w->conv_in); drop(w->conv_out); drop(w->ds);
    for (int s = 0; s < 4; ++s) { drop(w->res1[s]); drop(w->res2[s]); drop(w->down[s]); }
    delete w;
}
// The run-time half, one per engine; it reads the weights through references of the same names.
struct EncoderW {
    explicit EncoderW(const EncWeights& w)
        : conv_in(w.conv_in), res1(w.res1), res2(w.res2), down(w.down), conv_out(w.conv_out), ds(w.ds), layers(w.layers), proj_sem(w.proj_sem),
          proj_ac(w.proj_ac), books(w.books) {}
    const EncConvW& conv_in; const EncConvW (&res1)[4]; const EncConvW (&res2)[4]; const EncConvW (&down)[4]; const EncConvW &conv_out, &ds;
    const std::vector<EncLayerW>& layers;
    const float* const& proj_sem; const float* const& proj_ac;
    float* const& books;
    float *rope_cs = nullptr, *rope_sn = nullptr; int rope_rows = 0;
    char* ws = nullptr; size_t ws_cap = 0;     // grow-only workspace
    std::vector<EncStream> streams;            // streamed pushes: state in allocations of its own, never in ws
};

static constexpr size_t kEncAlign = 256;
static size_t enc_aligned(size_t b) { return (b + kEncAlign - 1) / kEncAlign * kEncAlign; }
namespace {
struct EncCarve {
    char* base; size_t used = 0;
    explicit EncCarve(char* b) : base(b) {}
    void* take_bytes(size_t n) { void* p = base ? base + used : nullptr; used += enc_aligned(n); return p; }
    float* take(size_t n_floats) { return (float*)take_bytes(n_floats * sizeof(float)); }
};
int64_t enc_resampled_len(int64_t n, int src_rate, int dst_rate) {   // q3::resample_linear's output length
    if (src_rate == dst_rate || n == 0) return n;
    const double ratio = (double)dst_rate / src_rate;
    return (int64_t)(size_t)((double)(size_t)n * ratio);
}
int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
}

void Engine::encoder_free() {
    if (!enc) return;
    if (enc->ws) (void)hipFree(enc->ws);
    for (EncStream& st : enc->streams) if (st.buf) (void)hipFree(st.buf);
    if (enc->rope_cs) (void)hipFree(enc->rope_cs);
    if (enc->rope_sn) (void)hipFree(enc->rope_sn);
    delete enc;
    enc = nullptr;
}

void Engine::encoder_poison() {
    if (!(flags & Q3TTS_FLAG_TEST_HOOKS)) throw Error("encoder_poison needs Q3TTS_FLAG_TEST_HOOKS");
    if (!enc || !enc->ws) return;
    sync();
    Q3_HIP_CHECK(hipMemset(enc->ws, 0xFF, enc->ws_cap));
}

int64_t Engine::audio_encode_len(int64_t n24) const {
    if (!has_audio_encoder() || n24 < 1) return -1;
    int64_t T = n24;
    for (int s = 0; s < c.enc_n_ratios; ++s) T = ceil_div(T, c.enc_ratios[s]);
    return ceil_div(T, 2);
}

// RoPE tables for rows [0, rows), computed in double: a row's bits do not depend on how many rows the tables have
static void enc_rope_tables(Engine& e, int rows) {
    EncoderW* enc = e.enc;
    const q3tts_config& c = e.c;
    const int half = c.enc_head_dim / 2;
    if (enc->rope_rows != rows || !enc->rope_cs) {
        if (enc->rope_cs) (void)hipFree(enc->rope_cs);
        if (enc->rope_sn) (void)hipFree(enc->rope_sn);
        enc->rope_cs = enc->rope_sn = nullptr; enc->rope_rows = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&enc->rope_cs, (size_t)rows * half * sizeof(float)));
        Q3_HIP_CHECK(hipMalloc((void**)&enc->rope_sn, (size_t)rows * half * sizeof(float)));
        enc->rope_rows = rows;
    }
    std::vector<float> cs((size_t)rows * half), sn((size_t)rows * half);
    for (int j = 0; j < half; ++j) {
        const double inv = 1.0 / std::pow((double)c.enc_rope_theta, (double)(2 * j) / (double)c.enc_head_dim);
        for (int p = 0; p < rows; ++p) { cs[(size_t)p * half + j] = (float)std::cos(p * inv); sn[(size_t)p * half + j] = (float)std::sin(p * inv); }
    }
    Q3_HIP_CHECK(hipMemcpy(enc->rope_cs, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    Q3_HIP_CHECK(hipMemcpy(enc->rope_sn, sn.data(), sn.size() * sizeof(float), hipMemcpyHostToDevice));
}

void Engine::encoder_finalize() {
    if (!has_audio_encoder()) return;
    if (c.enc_hidden % 4) throw Error("audio encoder: enc_hidden must be a multiple of 4");
    if (!ws.enc) ws.enc = new EncWeights();
    EncWeights* enc = ws.enc;   // shadows the run-time part down to encoder_runtime_init
    auto pack = [&](EncConvW& cv, const std::string& n, bool bias = true) {
        const Tensor& w = T(n + ".w");
        cv.cout = (int)w.shape[0]; cv.cin = (int)w.shape[1]; cv.k = (int)w.shape[2];
        if (!cv.w) { cv.w = (float*)ws.take((size_t)w.numel * sizeof(float), enc->bytes); cv.owned = true; }
        launch_repack_conv((const float*)w.dev, cv.w, cv.cin, cv.cout, cv.k, 0, stream);
        cv.b = bias ? (const float*)T(n + ".b").dev : nullptr;
    };
    auto fp = [&](const std::string& n) { return (const float*)T(n).dev; };
    pack(enc->conv_in, "enc.conv_in");
    for (int s = 0; s < c.enc_n_ratios; ++s) {
        const std::string p = "enc.stages." + std::to_string(s) + ".";
        pack(enc->res1[s], p + "res.conv1"); pack(enc->res2[s], p + "res.conv2"); pack(enc->down[s], p + "down");
    }
    pack(enc->conv_out, "enc.conv_out");
    pack(enc->ds, "enc.downsample", false);
    enc->layers.resize((size_t)c.enc_layers);
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "enc.layers." + std::to_string(i) + ".";
        EncLayerW& w = enc->layers[(size_t)i];
        w.ln1w = fp(p + "input_norm.w"); w.ln1b = fp(p + "input_norm.b"); w.qkv = fp(p + "q_proj"); w.o = fp(p + "o_proj"); w.s1 = fp(p + "attn_scale");
        w.ln2w = fp(p + "post_norm.w"); w.ln2b = fp(p + "post_norm.b"); w.fc1 = fp(p + "fc1"); w.fc2 = fp(p + "fc2"); w.s2 = fp(p + "mlp_scale");
    }
    enc->proj_sem = fp("enc.vq.sem.in_proj"); enc->proj_ac = fp("enc.vq.ac.in_proj");
    const size_t book = (size_t)c.enc_codebook * c.enc_vq_dim;
    if (!enc->books) enc->books = (float*)ws.take(book * c.n_groups * sizeof(float), enc->bytes);
    for (int g = 0; g < c.n_groups; ++g)
        Q3_HIP_CHECK(hipMemcpyAsync(enc->books + (size_t)g * book, T("enc.vq.codebook." + std::to_string(g)).dev, book * sizeof(float), hipMemcpyDeviceToDevice, stream));
    encoder_runtime_init();
    sync();
}

void Engine::encoder_runtime_init() {
    if (!ws.enc) throw Error("weights not finalized");
    if (!enc) enc = new EncoderW(*ws.enc);
    // RoPE tables for every row a clip under the cap can have, computed in double
    int64_t prod = 1;
    for (int s = 0; s < c.enc_n_ratios; ++s) prod *= c.enc_ratios[s];
    const int rows = (int)ceil_div(kEncMaxClipSamples, prod) + 1;
    enc_rope_tables(*this, std::max(rows, enc->rope_rows));   // tables a stream has grown stay grown
}

namespace {
struct EncTfBufs { float *x = nullptr, *n = nullptr, *qkv = nullptr, *a = nullptr, *f = nullptr; };
// streamed pushes: per layer the streams' K/V rings (device tables, one entry per span) and the ring update behind the attention
struct EncTfCarry { std::vector<const EncHist*> hist; std::vector<const EncCarryCopy*> copy; int n_copy = 0; int64_t max_floats = 0; };
}

// the transformer over R rows laid out by `spans` (level of the 25 Hz rows), in place on b.x
static void enc_run_transformer(Engine& e, const EncTfBufs& b, const EncSpan* spans, int n_clips, int R, int maxT, const EncTfCarry* carry = nullptr) {
    const q3tts_config& c = e.c;
    const EncoderW& W = *e.enc;
    const int EH = c.enc_hidden, AO = c.enc_heads * c.enc_head_dim;
    auto lin = [&](const float* in, int K, const float* Wm, int N, float* out, int act, const float* scale, const float* res) {
        EncConvArgs q;
        q.in = in; q.out = out; q.W = Wm; q.Cin = K; q.Cout = N; q.act = act; q.scale = scale; q.res = res;
        q.sin = spans; q.sout = spans; q.n_clips = n_clips; q.max_T_out = maxT;
        launch_enc_conv(q, e.stream);
    };
    for (size_t li = 0; li < W.layers.size(); ++li) {
        const EncLayerW& w = W.layers[li];
        const EncHist* hist = carry ? carry->hist[li] : nullptr;
        launch_enc_layernorm(b.x, w.ln1w, w.ln1b, c.enc_norm_eps, R, EH, b.n, e.stream);
        lin(b.n, EH, w.qkv, 3 * AO, b.qkv, 0, nullptr, nullptr);
        launch_enc_rope(b.qkv, W.rope_cs, W.rope_sn, W.rope_rows, c.enc_heads, c.enc_head_dim, spans, n_clips, maxT, e.stream, hist);
        launch_enc_attn(b.qkv, b.a, c.enc_heads, c.enc_head_dim, c.enc_window, 1.0f / sqrtf((float)c.enc_head_dim), spans, n_clips, maxT, e.stream, hist);
        if (carry && carry->n_copy > 0) launch_enc_carry_copy(carry->copy[li], carry->n_copy, carry->max_floats, e.stream);
        lin(b.a, AO, w.o, EH, b.x, 0, w.s1, b.x);
        launch_enc_layernorm(b.x, w.ln2w, w.ln2b, c.enc_norm_eps, R, EH, b.n, e.stream);
        lin(b.n, EH, w.fc1, c.enc_ffn, b.f, 1, nullptr, nullptr);
        lin(b.f, c.enc_ffn, w.fc2, EH, b.x, 0, w.s2, b.x);
    }
}

static void enc_ws_reserve(EncoderW& W, size_t bytes) {
    if (W.ws_cap >= bytes) return;
    if (W.ws) (void)hipFree(W.ws);
    W.ws = nullptr; W.ws_cap = 0;
    Q3_HIP_CHECK(hipMalloc((void**)&W.ws, bytes));
    W.ws_cap = bytes;
}

void Engine::audio_encode(int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* rates, int64_t* const* codes_out,
                          float* const* latents_out, const int32_t* caps, int32_t* n_frames) {
    if (!has_audio_encoder()) throw Error("model has no audio encoder");
    if (!enc) throw Error("weights not finalized");
    if (n_clips < 1) throw Error("audio encoder: n_clips must be at least 1, got " + std::to_string(n_clips));
    if (!pcm || !n_samples || !rates || !n_frames) throw Error("audio encoder: NULL argument");
    const int nr = c.enc_n_ratios, NL = nr + 2, EH = c.enc_hidden, AO = c.enc_heads * c.enc_head_dim, G = c.n_groups;
    // everything is validated before the first byte moves: a refused call leaves the outputs and the engine untouched
    std::vector<int64_t> n24((size_t)n_clips);
    for (int i = 0; i < n_clips; ++i) {
        const std::string who = "clip " + std::to_string(i) + ": ";
        if (!pcm[i]) throw Error(who + "NULL audio pointer");
        if (n_samples[i] < 1) throw Error(who + "n_samples must be at least 1, got " + std::to_string(n_samples[i]));
        if (rates[i] < 1) throw Error(who + "sample_rate must be at least 1, got " + std::to_string(rates[i]));
        if (rates[i] != 24000 && n_samples[i] > kEncMaxRawSamples)
            throw Error(who + "clip too long for the audio encoder: " + std::to_string(n_samples[i]) + " samples to resample, the cap is " + std::to_string(kEncMaxRawSamples));
        if (n_samples[i] > INT32_MAX / 2) throw Error(who + "more than 2^30 samples");
        n24[(size_t)i] = enc_resampled_len(n_samples[i], rates[i], 24000);
        if (n24[(size_t)i] < 1) throw Error(who + "no sample left at 24 kHz");
        if (n24[(size_t)i] > kEncMaxClipSamples)
            throw Error(who + "clip too long for the audio encoder: " + std::to_string(n24[(size_t)i]) + " samples at 24 kHz, the cap is " + std::to_string(kEncMaxClipSamples) + " (60 s)");
        const int64_t F = audio_encode_len(n24[(size_t)i]);
        if ((codes_out && codes_out[i]) || (latents_out && latents_out[i])) {
            if (!caps || caps[i] < F) throw Error(who + "output buffer too small for " + std::to_string(F) + " frames");
        }
    }
    for (int i = 0; i < n_clips; ++i) n_frames[i] = (int32_t)audio_encode_len(n24[(size_t)i]);
    last_audio_encode_ms = 0.f;

    for (int g0 = 0; g0 < n_clips;) {
        int g1 = g0; int64_t sum = 0, raw_sum = 0;   // a group: at most kEncMaxGroupSamples at 24 kHz and kEncMaxRawSamples to resample (its first clip always fits)
        auto raw_of = [&](int i) { return rates[i] != 24000 ? n_samples[i] : (int64_t)0; };
        while (g1 < n_clips && g1 - g0 < 1024 && (g1 == g0 || (sum + n24[(size_t)g1] <= kEncMaxGroupSamples && raw_sum + raw_of(g1) <= kEncMaxRawSamples))) {
            sum += n24[(size_t)g1]; raw_sum += raw_of(g1); ++g1;
        }
        const int n = g1 - g0;
        // span tables: level 0 = samples, level s + 1 behind stage s, level nr + 1 = frames
        std::vector<EncSpan> spans((size_t)NL * n);
        std::vector<int64_t> tot((size_t)NL, 0); std::vector<int> maxT((size_t)NL, 0);
        std::vector<SpkClip> rs_clips; size_t raw_total = 0; int max_rs = 0;
        for (int i = 0; i < n; ++i) {
            int64_t T = n24[(size_t)(g0 + i)];
            for (int l = 0; l < NL; ++l) {
                if (l > 0) T = ceil_div(T, l <= nr ? c.enc_ratios[l - 1] : 2);
                spans[(size_t)l * n + i].off = (int32_t)tot[(size_t)l]; spans[(size_t)l * n + i].T = (int32_t)T;
                tot[(size_t)l] += T; maxT[(size_t)l] = std::max(maxT[(size_t)l], (int)T);
            }
            if (rates[g0 + i] != 24000) {
                SpkClip cl;
                cl.in_off = (int32_t)raw_total; cl.n_in = (int32_t)n_samples[g0 + i]; cl.src_rate = rates[g0 + i]; cl.dst_rate = 24000;
                cl.rs_off = spans[(size_t)i].off; cl.n_rs = (int32_t)n24[(size_t)(g0 + i)];
                raw_total += (size_t)n_samples[g0 + i]; max_rs = std::max(max_rs, (int)cl.n_rs);
                rs_clips.push_back(cl);
            }
        }
        size_t xmax = 0, mmax = 0;
        { int dim = c.enc_filters;
          for (int s = 0; s <= nr; ++s, dim *= 2) { xmax = std::max(xmax, (size_t)tot[(size_t)s] * dim); mmax = std::max(mmax, (size_t)tot[(size_t)s] * (dim / 2)); } }
        const size_t R = (size_t)tot[(size_t)nr], F = (size_t)tot[(size_t)nr + 1];
        struct Bufs { EncSpan* spans; SpkClip* rs; float *raw, *x24, *X, *Y, *M; EncTfBufs tf; float* lat; int32_t* codes; size_t used; };
        auto layout = [&](char* base) {
            EncCarve cv(base);
            Bufs b;
            b.spans = (EncSpan*)cv.take_bytes(spans.size() * sizeof(EncSpan));
            b.rs = (SpkClip*)cv.take_bytes(std::max<size_t>(1, rs_clips.size()) * sizeof(SpkClip));
            b.raw = cv.take(std::max<size_t>(1, raw_total));
            b.x24 = cv.take((size_t)tot[0]);
            b.X = cv.take(xmax); b.Y = cv.take(xmax); b.M = cv.take(mmax);
            b.tf.x = cv.take(R * EH); b.tf.n = cv.take(R * EH); b.tf.qkv = cv.take(R * 3 * AO); b.tf.a = cv.take(R * AO); b.tf.f = cv.take(R * (size_t)c.enc_ffn);
            b.lat = cv.take(F * EH);
            b.codes = (int32_t*)cv.take_bytes(F * G * sizeof(int32_t));
            b.used = cv.used;
            return b;
        };
        enc_ws_reserve(*enc, layout(nullptr).used);
        const Bufs b = layout(enc->ws);

        Q3_HIP_CHECK(hipEventRecord(ev0, stream));
        Q3_HIP_CHECK(hipMemcpyAsync(b.spans, spans.data(), spans.size() * sizeof(EncSpan), hipMemcpyHostToDevice, stream));
        for (int i = 0, k = 0; i < n; ++i) {
            if (rates[g0 + i] == 24000) Q3_HIP_CHECK(hipMemcpyAsync(b.x24 + spans[(size_t)i].off, pcm[g0 + i], (size_t)n_samples[g0 + i] * sizeof(float), hipMemcpyHostToDevice, stream));
            else { Q3_HIP_CHECK(hipMemcpyAsync(b.raw + rs_clips[(size_t)k].in_off, pcm[g0 + i], (size_t)n_samples[g0 + i] * sizeof(float), hipMemcpyHostToDevice, stream)); ++k; }
        }
        if (!rs_clips.empty()) {
            Q3_HIP_CHECK(hipMemcpyAsync(b.rs, rs_clips.data(), rs_clips.size() * sizeof(SpkClip), hipMemcpyHostToDevice, stream));
            launch_resample_linear(b.raw, b.x24, b.rs, (int)rs_clips.size(), max_rs, stream);
        }
        auto level = [&](int l) { return b.spans + (size_t)l * n; };
        auto conv = [&](const EncConvW& cv, const float* in, int lin_, float* out, int lout, int stride, int elu, const float* res, int replicate = 0) {
            EncConvArgs q;
            q.in = in; q.out = out; q.W = cv.w; q.bias = cv.b; q.res = res;
            q.Cin = cv.cin; q.Cout = cv.cout; q.taps = cv.k; q.stride = stride; q.pad_left = cv.k - stride; q.elu_in = elu; q.replicate = replicate;
            q.sin = level(lin_); q.sout = level(lout); q.n_clips = n; q.max_T_out = maxT[(size_t)lout];
            launch_enc_conv(q, stream);
        };
        float *X = b.X, *Y = b.Y;
        conv(enc->conv_in, b.x24, 0, X, 0, 1, 0, nullptr);
        for (int s = 0; s < nr; ++s) {
            conv(enc->res1[s], X, s, b.M, s, 1, 1, nullptr);
            conv(enc->res2[s], b.M, s, X, s, 1, 1, X);
            conv(enc->down[s], X, s, Y, s + 1, c.enc_ratios[s], 1, nullptr);
            std::swap(X, Y);
        }
        conv(enc->conv_out, X, nr, b.tf.x, nr, 1, 1, nullptr);
        enc_run_transformer(*this, b.tf, level(nr), n, (int)R, maxT[(size_t)nr]);
        conv(enc->ds, b.tf.x, nr, b.lat, nr + 1, 2, 0, nullptr, 1);
        launch_rvq_encode(b.lat, (int)F, EH, enc->proj_sem, enc->proj_ac, enc->books, G, c.enc_codebook, c.enc_vq_dim, b.codes, stream);

        Q3_HIP_CHECK(hipEventRecord(ev1, stream));
        std::vector<int32_t> codes_h(F * G);
        Q3_HIP_CHECK(hipMemcpyAsync(codes_h.data(), b.codes, codes_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        for (int i = 0; i < n; ++i) {
            const EncSpan sp = spans[(size_t)(nr + 1) * n + i];
            if (latents_out && latents_out[g0 + i])
                Q3_HIP_CHECK(hipMemcpyAsync(latents_out[g0 + i], b.lat + (size_t)sp.off * EH, (size_t)sp.T * EH * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        sync();
        { float ms = 0.f; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) last_audio_encode_ms += ms; }
        for (int i = 0; i < n; ++i) {
            const EncSpan sp = spans[(size_t)(nr + 1) * n + i];
            if (codes_out && codes_out[g0 + i])
                for (size_t k = 0; k < (size_t)sp.T * G; ++k) codes_out[g0 + i][k] = codes_h[(size_t)sp.off * G + k];
        }
        g0 = g1;
    }
}

// ------------------------------------------------------------------------------------------------
// Streamed pushes.  A level's buffer holds the NEW rows of the push's streams back to back; what a conv or the
// attention needs from before them it reads from the stream's carry rings (EncHist), and one k_enc_carry_copy launch behind each
// consumer writes the push's last rows into the rings.  Rings are written from workspace rows only, so a push shorter than a ring
// moves nothing inside it.  A normal push emits floor(n_in / stride) - n_out rows per level (complete outputs only), a finishing one
// ceil(...) with the one-shot's right edge; the K walk of every kernel is the one-shot's, hence the same bits.
// ------------------------------------------------------------------------------------------------
namespace {
// EncHist::n_in / shift and the kernels' ring-slot arithmetic (absolute row mod cap) are int32: a stream's sample count must fit
static_assert(Engine::kEncMaxStreamSamples <= INT32_MAX, "a stream's absolute rows are int32 in EncHist and the encoder kernels");
struct EncConvPlan { const EncConvW* w; int lin, lout, stride, elu, replicate, cap; size_t off; };   // off: the ring's first float in EncStream::buf
struct EncStreamPlan { std::vector<EncConvPlan> convs; std::vector<size_t> kv_off; int kv_cap = 0; size_t kv_width = 0, floats = 0; };
EncStreamPlan enc_stream_plan(const q3tts_config& c, const EncoderW& W) {
    EncStreamPlan p;
    const int nr = c.enc_n_ratios;
    auto add = [&](const EncConvW& w, int lin, int lout, int stride, int elu, int rep) {
        EncConvPlan q{ &w, lin, lout, stride, elu, rep, w.k - 1, p.floats };
        p.floats += enc_aligned((size_t)q.cap * w.cin * sizeof(float)) / sizeof(float);
        p.convs.push_back(q);
    };
    add(W.conv_in, 0, 0, 1, 0, 0);
    for (int s = 0; s < nr; ++s) { add(W.res1[s], s, s, 1, 1, 0); add(W.res2[s], s, s, 1, 1, 0); add(W.down[s], s, s + 1, c.enc_ratios[s], 1, 0); }
    add(W.conv_out, nr, nr, 1, 1, 0);
    add(W.ds, nr, nr + 1, 2, 0, 1);
    p.kv_cap = c.enc_window - 1; p.kv_width = (size_t)2 * c.enc_heads * c.enc_head_dim;
    for (int l = 0; l < c.enc_layers; ++l) { p.kv_off.push_back(p.floats); p.floats += enc_aligned((size_t)p.kv_cap * p.kv_width * sizeof(float)) / sizeof(float); }
    if (p.floats == 0) p.floats = 1;
    return p;
}
// rows every level has after `add` more samples: floor per level, ceil when the stream finishes (the one-shot's T = ceil(T / stride))
void enc_stream_advance(const q3tts_config& c, const int64_t* before, int64_t add, bool finish, int64_t* after) {
    const int nr = c.enc_n_ratios;
    after[0] = before[0] + add;
    for (int l = 1; l <= nr + 1; ++l) {
        const int64_t st = l <= nr ? c.enc_ratios[l - 1] : 2;
        after[l] = finish ? ceil_div(after[l - 1], st) : after[l - 1] / st;
    }
}
struct EncTab {   // the call's descriptor tables, built on the host and uploaded once
    std::vector<char> h;
    template <class T> size_t add(const std::vector<T>& v) {
        const size_t o = h.size();
        h.resize(o + enc_aligned(std::max<size_t>(1, v.size()) * sizeof(T)));
        if (!v.empty()) std::memcpy(&h[o], v.data(), v.size() * sizeof(T));
        return o;
    }
};
}

static EncStream& enc_stream_at(const Engine& e, int id, const char* who) {
    if (!e.has_audio_encoder()) throw Error("model has no audio encoder");
    if (!e.enc) throw Error("weights not finalized");
    if (id < 0 || id >= (int)e.enc->streams.size() || !e.enc->streams[(size_t)id].open)
        throw Error(std::string(who) + ": no open audio stream with id " + std::to_string(id));
    return e.enc->streams[(size_t)id];
}

int Engine::audio_stream_begin(int64_t max_samples, int sample_rate, int format) {
    if (!has_audio_encoder()) throw Error("model has no audio encoder");
    if (!enc) throw Error("weights not finalized");
    if (sample_rate < 1 || sample_rate > kEncMaxStreamRate)
        throw Error("audio stream: sample_rate must be 1.." + std::to_string(kEncMaxStreamRate) + ", got " + std::to_string(sample_rate));
    if (!pcm_format_known(format))
        throw Error("audio stream: format must be Q3TTS_PCM_F32 (0) or Q3TTS_PCM_S16 (1), got " + std::to_string(format) + "; or Q3TTS_PCM_MULAW (2) or Q3TTS_PCM_ALAW (3)");
    const int64_t hour = (int64_t)3600 * sample_rate;   // at 24 kHz: kEncMaxStreamSamples
    if (max_samples == 0) max_samples = (int64_t)60 * sample_rate;
    if (max_samples < 1 || max_samples > hour)
        throw Error("audio stream: max_samples must be 0 (60 s) or 1.." + std::to_string(hour) + " (one hour), got " + std::to_string(max_samples));
    const int64_t max24 = resample_stream_emitted(sample_rate, 24000, max_samples, true);   // what the encoder sees of it at most
    int id = -1, n_open = 0;
    for (size_t i = 0; i < enc->streams.size(); ++i) {
        if (enc->streams[i].open) ++n_open;
        else if (id < 0) id = (int)i;
    }
    if (n_open >= kEncMaxStreams) throw Error("audio stream: " + std::to_string(kEncMaxStreams) + " streams are open already");
    int64_t prod = 1;
    for (int s = 0; s < c.enc_n_ratios; ++s) prod *= c.enc_ratios[s];
    const int rows = (int)ceil_div(max24, prod) + 1;
    if (rows > enc->rope_rows) { sync(); enc_rope_tables(*this, rows); }   // the whole table again, by the same formula: existing rows keep their bits
    const EncStreamPlan plan = enc_stream_plan(c, *enc);
    if (id < 0) { enc->streams.emplace_back(); id = (int)enc->streams.size() - 1; }
    EncStream& st = enc->streams[(size_t)id];
    const size_t floats = plan.floats + 2 * kEncCarryFloats;   // every stream has room for a carry: an id may come back at another rate
    if (st.buf_floats < floats) {
        if (st.buf) (void)hipFree(st.buf);
        st.buf = nullptr; st.buf_floats = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&st.buf, floats * sizeof(float)));
        st.buf_floats = floats;
    }
    // no clearing: a ring slot, and a carry sample, is read only for an absolute row this stream has written
    st.open = true; st.finished = false; st.max_samples = max_samples;
    for (int64_t& r : st.rows) r = 0;
    st.rate = sample_rate; st.format = format; st.n_raw = 0; st.carry_cur = 0; st.carry_off = plan.floats;
    st.carry_len = resample_stream_carry(sample_rate, 24000);
    return id;
}

void Engine::audio_stream_end(int id) {
    EncStream& st = enc_stream_at(*this, id, "audio_stream_end");
    st.open = false; st.finished = false;
}

void Engine::audio_stream_info(int id, int64_t* n_samples, int32_t* n_frames, int* finished, int64_t* bytes) const {
    const EncStream& st = enc_stream_at(*this, id, "audio_stream_info");
    if (n_samples) *n_samples = st.n_raw;
    if (n_frames) *n_frames = (int32_t)st.rows[c.enc_n_ratios + 1];
    if (finished) *finished = st.finished ? 1 : 0;
    if (bytes) *bytes = (int64_t)(st.buf_floats * sizeof(float));
}

void Engine::audio_stream_format(int id, int32_t* sample_rate, int32_t* format) const {
    const EncStream& st = enc_stream_at(*this, id, "audio_stream_format");
    if (sample_rate) *sample_rate = st.rate;
    if (format) *format = st.format;
}

// the 24 kHz samples a push of n of the stream's own samples feeds the encoder: the host rule after the push minus before it
static int64_t enc_stream_new24(const EncStream& st, int64_t n, bool finish) {
    if (st.rate == 24000) return n;
    return resample_stream_emitted(st.rate, 24000, st.n_raw + n, finish) - st.rows[0];
}

int64_t Engine::audio_stream_push_len(int id, int64_t n_samples, bool finish) const {
    const EncStream& st = enc_stream_at(*this, id, "audio_stream_push_len");
    if (st.finished) throw Error("audio stream " + std::to_string(id) + " is finished");
    if (n_samples < 0 || n_samples > (int64_t)60 * st.rate || st.n_raw + n_samples > st.max_samples)
        throw Error("audio stream " + std::to_string(id) + ": a push of " + std::to_string(n_samples) + " samples is outside the stream's limits");
    int64_t after[8];
    enc_stream_advance(c, st.rows, enc_stream_new24(st, n_samples, finish), finish, after);
    return after[c.enc_n_ratios + 1] - st.rows[c.enc_n_ratios + 1];
}

void Engine::audio_stream_push_batch(int n_streams, const int32_t* ids, const void* const* pcm, const int64_t* n_samples, const int32_t* finish,
                                     int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames, bool float_only) {
    if (!has_audio_encoder()) throw Error("model has no audio encoder");
    if (!enc) throw Error("weights not finalized");
    if (n_streams < 1) throw Error("audio stream push: n_streams must be at least 1, got " + std::to_string(n_streams));
    if (!ids || !pcm || !n_samples || !n_frames) throw Error("audio stream push: NULL argument");
    const int nr = c.enc_n_ratios, NL = nr + 2, EH = c.enc_hidden, AO = c.enc_heads * c.enc_head_dim, G = c.n_groups;
    // everything is validated before any stream moves
    std::vector<int64_t> after((size_t)n_streams * 8, 0), n24((size_t)n_streams, 0);
    for (int i = 0; i < n_streams; ++i) {
        const std::string who = "audio stream " + std::to_string(ids[i]) + ": ";
        const EncStream& st = enc_stream_at(*this, ids[i], "audio stream push");
        for (int j = 0; j < i; ++j) if (ids[j] == ids[i]) throw Error(who + "given twice in one push");
        if (st.finished) throw Error(who + "is finished");
        if (float_only && st.format == Q3TTS_PCM_S16) throw Error(who + "takes int16 samples (Q3TTS_PCM_S16): push it through q3tts_audio_stream_push_any_host, not a float entry");
        if (float_only && pcm_format_g711(st.format)) throw Error(who + "takes " + pcm_format_name(st.format) + " bytes: push it through q3tts_audio_stream_push_any_host, not a float entry");
        if (n_samples[i] < 0) throw Error(who + "n_samples must not be negative, got " + std::to_string(n_samples[i]));
        if (n_samples[i] > 0 && !pcm[i]) throw Error(who + "NULL audio pointer");
        if (n_samples[i] > (int64_t)60 * st.rate)
            throw Error(who + "push too long: " + std::to_string(n_samples[i]) + " samples, the cap per push is " + std::to_string((int64_t)60 * st.rate) + " (60 s)");
        if (st.n_raw + n_samples[i] > st.max_samples)
            throw Error(who + "over its max_samples: " + std::to_string(st.n_raw) + " + " + std::to_string(n_samples[i]) + " samples, the stream was begun for " + std::to_string(st.max_samples));
        n24[(size_t)i] = enc_stream_new24(st, n_samples[i], finish && finish[i]);   // the host rule first: every cap below is about what it gives
        enc_stream_advance(c, st.rows, n24[(size_t)i], finish && finish[i], &after[(size_t)i * 8]);
        const int64_t F = after[(size_t)i * 8 + nr + 1] - st.rows[nr + 1];
        if (F > 0 && ((codes_out && codes_out[i]) || (latents_out && latents_out[i]))) {
            if (!caps || caps[i] < F) throw Error(who + "output buffer too small for " + std::to_string(F) + " frames");
        }
    }
    const EncStreamPlan plan = enc_stream_plan(c, *enc);
    last_audio_encode_ms = 0.f;

    for (int g0 = 0; g0 < n_streams;) {
        // a group: at most kEncMaxGroupSamples new samples at 24 kHz and kEncMaxRawSamples to resample (its first stream always fits); a stream's push is never split
        int g1 = g0; int64_t sum = 0, raw_sum = 0;
        auto raw_of = [&](int i) { return enc->streams[(size_t)ids[i]].plain() ? (int64_t)0 : n_samples[i]; };
        while (g1 < n_streams && g1 - g0 < 1024 && (g1 == g0 || (sum + n24[(size_t)g1] <= kEncMaxGroupSamples && raw_sum + raw_of(g1) <= kEncMaxRawSamples))) {
            sum += n24[(size_t)g1]; raw_sum += raw_of(g1); ++g1;
        }
        const int n = g1 - g0;
        auto stream_of = [&](int i) -> EncStream& { return enc->streams[(size_t)ids[g0 + i]]; };
        auto before = [&](int i, int l) { return stream_of(i).rows[l]; };
        auto newr = [&](int i, int l) { return (int)(after[(size_t)(g0 + i) * 8 + l] - stream_of(i).rows[l]); };
        // spans of the new rows: level 0 = samples, level s + 1 behind stage s, level nr + 1 = frames
        std::vector<EncSpan> spans((size_t)NL * n);
        std::vector<int64_t> tot((size_t)NL, 0);
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < NL; ++l) {
                spans[(size_t)l * n + i].off = (int32_t)tot[(size_t)l]; spans[(size_t)l * n + i].T = newr(i, l);
                tot[(size_t)l] += newr(i, l);
            }
        // the streams that resample on the way in: their new samples are staged as they came: float, int16 or G.711 bytes
        std::vector<EncRsStream> rs; size_t staged_bytes = 0; int rs_work = 0;
        for (int i = 0; i < n; ++i) {
            EncStream& st = stream_of(i);
            const int64_t add = n_samples[g0 + i];
            if (st.plain() || (add == 0 && newr(i, 0) == 0)) continue;
            EncRsStream d;
            const int64_t held = std::min<int64_t>(st.carry_len, st.n_raw);
            d.carry_in = st.buf + st.carry_off + (size_t)st.carry_cur * kEncCarryFloats;
            d.carry_out = st.buf + st.carry_off + (size_t)(1 - st.carry_cur) * kEncCarryFloats;
            d.carry_abs0 = st.n_raw - held; d.n_before = st.n_raw; d.n_total = st.n_raw + add; d.out0 = st.rows[0];
            d.in_off = (int64_t)staged_bytes; d.n_new = (int32_t)add; d.n_out = newr(i, 0);
            d.keep = add > 0 ? (int32_t)std::min<int64_t>(st.carry_len, d.n_total) : 0;
            d.x24_off = spans[(size_t)i].off; d.src_rate = st.rate; d.format = st.format;
            staged_bytes += ((size_t)add * pcm_format_bytes(st.format) + 3) / 4 * 4;
            rs_work = std::max(rs_work, d.n_out + d.keep);
            rs.push_back(d);
        }
        size_t xmax = 1, mmax = 1;
        { int dim = c.enc_filters;
          for (int s = 0; s <= nr; ++s, dim *= 2) { xmax = std::max(xmax, (size_t)tot[(size_t)s] * dim); mmax = std::max(mmax, (size_t)tot[(size_t)s] * (dim / 2)); } }
        const size_t R = (size_t)tot[(size_t)nr], F = (size_t)tot[(size_t)nr + 1], R1 = std::max<size_t>(1, R), F1 = std::max<size_t>(1, F);
        const size_t tab_cap = (size_t)n * (plan.convs.size() * (2 * enc_aligned(sizeof(EncSpan)) + enc_aligned(sizeof(EncHist)) + enc_aligned(sizeof(EncCarryCopy)))
                                            + (size_t)c.enc_layers * (enc_aligned(sizeof(EncHist)) + enc_aligned(sizeof(EncCarryCopy))) + enc_aligned(sizeof(EncSpan)))
                               + enc_aligned(std::max<size_t>(1, rs.size()) * sizeof(EncRsStream));
        struct Bufs { char* tab; char* staged; float *x24, *X, *Y, *M; EncTfBufs tf; float* lat; int32_t* codes; size_t used; };
        auto layout = [&](char* base) {
            EncCarve cv(base);
            Bufs b;
            b.tab = (char*)cv.take_bytes(tab_cap);
            b.staged = (char*)cv.take_bytes(staged_bytes + 4);   // + 4: a stream without new samples still has an address to clamp to
            b.x24 = cv.take(std::max<size_t>(1, (size_t)tot[0]));
            b.X = cv.take(xmax); b.Y = cv.take(xmax); b.M = cv.take(mmax);
            b.tf.x = cv.take(R1 * EH); b.tf.n = cv.take(R1 * EH); b.tf.qkv = cv.take(R1 * 3 * AO); b.tf.a = cv.take(R1 * AO); b.tf.f = cv.take(R1 * (size_t)c.enc_ffn);
            b.lat = cv.take(F1 * EH);
            b.codes = (int32_t*)cv.take_bytes(F1 * G * sizeof(int32_t));
            b.used = cv.used;
            return b;
        };
        enc_ws_reserve(*enc, layout(nullptr).used);
        const Bufs b = layout(enc->ws);

        // pass 1: every launch's tables (the streams that get a new row at the launch's output level; a stream that gets none is left out)
        EncTab tab;
        struct ConvStep { size_t sin, sout, hist, copy; int n = 0, maxT = 0, n_copy = 0; int64_t copy_floats = 0; const float* in; float* out; const float* res; };
        std::vector<ConvStep> steps(plan.convs.size());
        auto plan_conv = [&](size_t ci, const float* in, float* out, const float* res) {
            const EncConvPlan& p = plan.convs[ci];
            ConvStep& st = steps[ci];
            st.in = in; st.out = out; st.res = res;
            std::vector<EncSpan> si, so; std::vector<EncHist> hs; std::vector<EncCarryCopy> cp;
            for (int i = 0; i < n; ++i) {
                const int c_in = newr(i, p.lin);
                float* ring = stream_of(i).buf + p.off;
                if (newr(i, p.lout) >= 1) {
                    si.push_back(spans[(size_t)p.lin * n + i]); so.push_back(spans[(size_t)p.lout * n + i]);
                    EncHist h;
                    h.carry = ring; h.n_in = (int32_t)before(i, p.lin); h.shift = (int32_t)(before(i, p.lout) * p.stride - before(i, p.lin)); h.cap = p.cap;
                    hs.push_back(h);
                    st.maxT = std::max(st.maxT, newr(i, p.lout));
                }
                if (c_in >= 1 && p.cap >= 1) {
                    EncCarryCopy q;
                    q.rows = std::min(c_in, p.cap); q.width = p.w->cin; q.src_ld = p.w->cin; q.cap = p.cap;
                    q.src = in + ((size_t)spans[(size_t)p.lin * n + i].off + (size_t)(c_in - q.rows)) * p.w->cin;
                    q.dst = ring; q.slot0 = (int32_t)((before(i, p.lin) + c_in - q.rows) % p.cap);
                    cp.push_back(q);
                    st.copy_floats = std::max<int64_t>(st.copy_floats, (int64_t)q.rows * q.width);
                }
            }
            st.n = (int)hs.size(); st.n_copy = (int)cp.size();
            st.sin = tab.add(si); st.sout = tab.add(so); st.hist = tab.add(hs); st.copy = tab.add(cp);
        };
        {
            float *X = b.X, *Y = b.Y; size_t ci = 0;
            plan_conv(ci++, b.x24, X, nullptr);
            for (int s = 0; s < nr; ++s) {
                plan_conv(ci++, X, b.M, nullptr);
                plan_conv(ci++, b.M, X, X);
                plan_conv(ci++, X, Y, nullptr);
                std::swap(X, Y);
            }
            plan_conv(ci++, X, b.tf.x, nullptr);
            plan_conv(ci++, b.tf.x, b.lat, nullptr);
        }
        std::vector<EncSpan> tf_spans; int tf_maxT = 0;
        std::vector<size_t> tf_hist, tf_copy; int tf_n_copy = 0; int64_t tf_copy_floats = 0;
        for (int i = 0; i < n; ++i) if (newr(i, nr) >= 1) { tf_spans.push_back(spans[(size_t)nr * n + i]); tf_maxT = std::max(tf_maxT, newr(i, nr)); }
        const size_t tf_span_off = tab.add(tf_spans);
        for (int l = 0; l < c.enc_layers; ++l) {
            std::vector<EncHist> hs; std::vector<EncCarryCopy> cp;
            for (int i = 0; i < n; ++i) {
                const int rows = newr(i, nr);
                if (rows < 1) continue;
                float* ring = stream_of(i).buf + plan.kv_off[(size_t)l];
                EncHist h; h.carry = ring; h.n_in = (int32_t)before(i, nr); h.cap = plan.kv_cap;
                hs.push_back(h);
                if (plan.kv_cap >= 1) {
                    EncCarryCopy q;
                    q.rows = std::min(rows, plan.kv_cap); q.width = 2 * AO; q.src_ld = 3 * AO; q.cap = plan.kv_cap;
                    q.src = b.tf.qkv + ((size_t)spans[(size_t)nr * n + i].off + (size_t)(rows - q.rows)) * 3 * AO + AO;
                    q.dst = ring; q.slot0 = (int32_t)((before(i, nr) + rows - q.rows) % plan.kv_cap);
                    cp.push_back(q);
                    tf_copy_floats = std::max<int64_t>(tf_copy_floats, (int64_t)q.rows * q.width);
                }
            }
            tf_n_copy = (int)cp.size();
            tf_hist.push_back(tab.add(hs)); tf_copy.push_back(tab.add(cp));
        }
        const size_t rs_off = tab.add(rs);
        if (tab.h.size() > tab_cap) throw Error("audio stream push: descriptor tables larger than planned");

        // pass 2: one upload of the tables, the samples, then the launches
        Q3_HIP_CHECK(hipEventRecord(ev0, stream));
        if (!tab.h.empty()) Q3_HIP_CHECK(hipMemcpyAsync(b.tab, tab.h.data(), tab.h.size(), hipMemcpyHostToDevice, stream));
        for (int i = 0, k = 0; i < n; ++i) {
            const EncStream& st = stream_of(i);
            const size_t add = (size_t)n_samples[g0 + i];
            if (st.plain()) {
                if (add > 0) Q3_HIP_CHECK(hipMemcpyAsync(b.x24 + spans[(size_t)i].off, pcm[g0 + i], add * sizeof(float), hipMemcpyHostToDevice, stream));
            } else if (add > 0 || newr(i, 0) > 0) {
                if (add > 0) Q3_HIP_CHECK(hipMemcpyAsync(b.staged + rs[(size_t)k].in_off, pcm[g0 + i], add * pcm_format_bytes(st.format), hipMemcpyHostToDevice, stream));
                ++k;
            }
        }
        if (rs_work > 0) launch_resample_linear_streams(b.staged, b.x24, (const EncRsStream*)(b.tab + rs_off), (int)rs.size(), rs_work, stream);
        for (size_t ci = 0; ci < steps.size(); ++ci) {
            const EncConvPlan& p = plan.convs[ci];
            const ConvStep& st = steps[ci];
            if (ci + 1 == steps.size() && !tf_spans.empty()) {   // the transformer sits between conv_out and the downsample conv
                EncTfCarry tc;
                for (int l = 0; l < c.enc_layers; ++l) { tc.hist.push_back((const EncHist*)(b.tab + tf_hist[(size_t)l])); tc.copy.push_back((const EncCarryCopy*)(b.tab + tf_copy[(size_t)l])); }
                tc.n_copy = tf_n_copy; tc.max_floats = tf_copy_floats;
                enc_run_transformer(*this, b.tf, (const EncSpan*)(b.tab + tf_span_off), (int)tf_spans.size(), (int)R, tf_maxT, &tc);
            }
            if (st.n > 0) {
                EncConvArgs q;
                q.in = st.in; q.out = st.out; q.W = p.w->w; q.bias = p.w->b; q.res = st.res;
                q.Cin = p.w->cin; q.Cout = p.w->cout; q.taps = p.w->k; q.stride = p.stride; q.pad_left = p.w->k - p.stride; q.elu_in = p.elu; q.replicate = p.replicate;
                q.sin = (const EncSpan*)(b.tab + st.sin); q.sout = (const EncSpan*)(b.tab + st.sout); q.n_clips = st.n; q.max_T_out = st.maxT;
                launch_enc_conv_hist(q, (const EncHist*)(b.tab + st.hist), stream);
            }
            if (st.n_copy > 0) launch_enc_carry_copy((const EncCarryCopy*)(b.tab + st.copy), st.n_copy, st.copy_floats, stream);
        }
        if (F > 0) launch_rvq_encode(b.lat, (int)F, EH, enc->proj_sem, enc->proj_ac, enc->books, G, c.enc_codebook, c.enc_vq_dim, b.codes, stream);
        Q3_HIP_CHECK(hipEventRecord(ev1, stream));

        std::vector<int32_t> codes_h(F * G);
        if (F > 0) Q3_HIP_CHECK(hipMemcpyAsync(codes_h.data(), b.codes, codes_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        for (int i = 0; i < n; ++i) {
            const EncSpan sp = spans[(size_t)(nr + 1) * n + i];
            if (sp.T > 0 && latents_out && latents_out[g0 + i])
                Q3_HIP_CHECK(hipMemcpyAsync(latents_out[g0 + i], b.lat + (size_t)sp.off * EH, (size_t)sp.T * EH * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        sync();
        { float ms = 0.f; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) last_audio_encode_ms += ms; }
        for (int i = 0; i < n; ++i) {
            const EncSpan sp = spans[(size_t)(nr + 1) * n + i];
            n_frames[g0 + i] = sp.T;
            if (codes_out && codes_out[g0 + i])
                for (size_t k = 0; k < (size_t)sp.T * G; ++k) codes_out[g0 + i][k] = codes_h[(size_t)sp.off * G + k];
        }
        for (int i = 0; i < n; ++i) {   // the group's streams move
            EncStream& st = stream_of(i);
            for (int l = 0; l < NL; ++l) st.rows[l] = after[(size_t)(g0 + i) * 8 + l];
            if (n_samples[g0 + i] > 0) { st.n_raw += n_samples[g0 + i]; if (!st.plain()) st.carry_cur = 1 - st.carry_cur; }
            if (finish && finish[g0 + i]) st.finished = true;
        }
        g0 = g1;
    }
}

void Engine::enc_transformer_host(const float* rows, int n_rows, float* out) {
    if (!(flags & Q3TTS_FLAG_TEST_HOOKS)) throw Error("the encoder transformer hook needs an engine created with Q3TTS_FLAG_TEST_HOOKS");
    if (!has_audio_encoder()) throw Error("model has no audio encoder");
    if (!enc) throw Error("weights not finalized");
    if (!rows || !out || n_rows < 1 || n_rows > enc->rope_rows) throw Error("encoder transformer: needs 1.." + std::to_string(enc->rope_rows) + " rows");
    const size_t R = (size_t)n_rows, EH = (size_t)c.enc_hidden, AO = (size_t)c.enc_heads * c.enc_head_dim;
    auto layout = [&](char* base, EncSpan** sp, EncTfBufs* b) {
        EncCarve cv(base);
        *sp = (EncSpan*)cv.take_bytes(sizeof(EncSpan));
        b->x = cv.take(R * EH); b->n = cv.take(R * EH); b->qkv = cv.take(R * 3 * AO); b->a = cv.take(R * AO); b->f = cv.take(R * (size_t)c.enc_ffn);
        return cv.used;
    };
    EncSpan* sp_d; EncTfBufs b;
    enc_ws_reserve(*enc, layout(nullptr, &sp_d, &b));
    layout(enc->ws, &sp_d, &b);
    EncSpan sp; sp.off = 0; sp.T = n_rows;
    Q3_HIP_CHECK(hipMemcpyAsync(sp_d, &sp, sizeof sp, hipMemcpyHostToDevice, stream));
    Q3_HIP_CHECK(hipMemcpyAsync(b.x, rows, R * EH * sizeof(float), hipMemcpyHostToDevice, stream));
    enc_run_transformer(*this, b, sp_d, 1, n_rows, n_rows);
    Q3_HIP_CHECK(hipMemcpyAsync(out, b.x, R * EH * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
}

// Synthetic codebooks at the scale of the projected latents (q3tts_fill_synthetic).  With codebooks of arbitrary scale nearly every
// frame picks the same id and an encode exercises nothing.  The other enc.* tensors are filled already: encode 16 frames of seeded
// noise up to the latents, project them on the host, and draw level g of each quantizer from N(0, (0.75^g sigma)^2) per element,
// the first level of each quantizer centred on the projected latents' mean.
void Engine::enc_calibrate_synthetic(uint64_t seed) {
    encoder_finalize();
    int64_t frame = 2;
    for (int s = 0; s < c.enc_n_ratios; ++s) frame *= c.enc_ratios[s];
    const int Fc = 16, EH = c.enc_hidden, D = c.enc_vq_dim, CB = c.enc_codebook;
    uint64_t st = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    auto next = [&]() { st += 0x9E3779B97F4A7C15ull; uint64_t z = st; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    auto uni = [&]() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; };
    std::vector<float> noise((size_t)(Fc * frame));
    for (float& v : noise) v = (float)(uni() - 0.5);
    std::vector<float> lat((size_t)Fc * EH);
    const float* pp = noise.data(); const int64_t ns = (int64_t)noise.size(); const int32_t rate = 24000, cap = Fc; int32_t nf = 0;
    float* lp = lat.data();
    audio_encode(1, &pp, &ns, &rate, nullptr, &lp, &cap, &nf);
    std::vector<float> P((size_t)D * EH), book((size_t)CB * D);
    for (int q = 0; q < 2; ++q) {
        get_tensor(q == 0 ? "enc.vq.sem.in_proj" : "enc.vq.ac.in_proj", P.data(), (int64_t)P.size());
        std::vector<double> z((size_t)nf * D), mean((size_t)D, 0.0);
        for (int f = 0; f < nf; ++f)
            for (int d = 0; d < D; ++d) {
                double a = 0.0;
                for (int h = 0; h < EH; ++h) a += (double)P[(size_t)d * EH + h] * lat[(size_t)f * EH + h];
                z[(size_t)f * D + d] = a; mean[(size_t)d] += a / nf;
            }
        double var = 0.0;
        for (int f = 0; f < nf; ++f) for (int d = 0; d < D; ++d) { const double e = z[(size_t)f * D + d] - mean[(size_t)d]; var += e * e; }
        double sigma = std::sqrt(var / ((double)nf * D));
        if (!(sigma > 1e-12) || !std::isfinite(sigma)) sigma = 1.0;
        const int g_first = q == 0 ? 0 : 1, g_end = q == 0 ? 1 : c.n_groups;
        for (int g = g_first; g < g_end; ++g) {
            const double sd = sigma * std::pow(0.75, (double)(g - g_first));
            for (int r = 0; r < CB; ++r)
                for (int d = 0; d < D; d += 2) {   // Box-Muller, two values per draw (D is a multiple of 4)
                    const double u1 = uni(), u2 = uni(), m = std::sqrt(-2.0 * std::log(u1));
                    book[(size_t)r * D + d] = (float)(sd * m * std::cos(6.283185307179586 * u2) + (g == g_first ? mean[(size_t)d] : 0.0));
                    book[(size_t)r * D + d + 1] = (float)(sd * m * std::sin(6.283185307179586 * u2) + (g == g_first ? mean[(size_t)d + 1] : 0.0));
                }
            set_tensor("enc.vq.codebook." + std::to_string(g), book.data(), (int64_t)book.size());
        }
    }
}

} // namespace q3
