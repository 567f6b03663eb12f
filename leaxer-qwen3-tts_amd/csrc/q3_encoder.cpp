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
struct EncoderW {
    EncConvW conv_in, res1[4], res2[4], down[4], conv_out, ds;
    std::vector<EncLayerW> layers;
    const float *proj_sem = nullptr, *proj_ac = nullptr;
    float* books = nullptr;                    // [n_groups][codebook][vq_dim], the level tables back to back
    float *rope_cs = nullptr, *rope_sn = nullptr; int rope_rows = 0;
    char* ws = nullptr; size_t ws_cap = 0;     // grow-only workspace
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
    if (enc->books) (void)hipFree(enc->books);
    if (enc->rope_cs) (void)hipFree(enc->rope_cs);
    if (enc->rope_sn) (void)hipFree(enc->rope_sn);
    auto drop = [](EncConvW& cv) { if (cv.owned && cv.w) (void)hipFree(cv.w); cv.w = nullptr; };
    drop(enc->conv_in); drop(enc->conv_out); drop(enc->ds);
    for (int s = 0; s < 4; ++s) { drop(enc->res1[s]); drop(enc->res2[s]); drop(enc->down[s]); }
    delete enc;
    enc = nullptr;
}

int64_t Engine::audio_encode_len(int64_t n24) const {
    if (!has_audio_encoder() || n24 < 1) return -1;
    int64_t T = n24;
    for (int s = 0; s < c.enc_n_ratios; ++s) T = ceil_div(T, c.enc_ratios[s]);
    return ceil_div(T, 2);
}

void Engine::encoder_finalize() {
    if (!has_audio_encoder()) return;
    if (c.enc_hidden % 4) throw Error("audio encoder: enc_hidden must be a multiple of 4");
    if (!enc) enc = new EncoderW();
    auto pack = [&](EncConvW& cv, const std::string& n, bool bias = true) {
        const Tensor& w = T(n + ".w");
        cv.cout = (int)w.shape[0]; cv.cin = (int)w.shape[1]; cv.k = (int)w.shape[2];
        if (!cv.w) { Q3_HIP_CHECK(hipMalloc((void**)&cv.w, (size_t)w.numel * sizeof(float))); cv.owned = true; }
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
    if (!enc->books) Q3_HIP_CHECK(hipMalloc((void**)&enc->books, book * c.n_groups * sizeof(float)));
    for (int g = 0; g < c.n_groups; ++g)
        Q3_HIP_CHECK(hipMemcpyAsync(enc->books + (size_t)g * book, T("enc.vq.codebook." + std::to_string(g)).dev, book * sizeof(float), hipMemcpyDeviceToDevice, stream));
    // RoPE tables for every row a clip under the cap can have, computed in double
    int64_t prod = 1;
    for (int s = 0; s < c.enc_n_ratios; ++s) prod *= c.enc_ratios[s];
    const int rows = (int)ceil_div(kEncMaxClipSamples, prod) + 1, half = c.enc_head_dim / 2;
    if (enc->rope_rows != rows || !enc->rope_cs) {
        if (enc->rope_cs) (void)hipFree(enc->rope_cs);
        if (enc->rope_sn) (void)hipFree(enc->rope_sn);
        enc->rope_cs = enc->rope_sn = nullptr;
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
    sync();
}

namespace {
struct EncTfBufs { float *x = nullptr, *n = nullptr, *qkv = nullptr, *a = nullptr, *f = nullptr; };
}

// the transformer over R rows laid out by `spans` (level of the 25 Hz rows), in place on b.x
static void enc_run_transformer(Engine& e, const EncTfBufs& b, const EncSpan* spans, int n_clips, int R, int maxT) {
    const q3tts_config& c = e.c;
    const EncoderW& W = *e.enc;
    const int EH = c.enc_hidden, AO = c.enc_heads * c.enc_head_dim;
    auto lin = [&](const float* in, int K, const float* Wm, int N, float* out, int act, const float* scale, const float* res) {
        EncConvArgs q;
        q.in = in; q.out = out; q.W = Wm; q.Cin = K; q.Cout = N; q.act = act; q.scale = scale; q.res = res;
        q.sin = spans; q.sout = spans; q.n_clips = n_clips; q.max_T_out = maxT;
        launch_enc_conv(q, e.stream);
    };
    for (const EncLayerW& w : W.layers) {
        launch_enc_layernorm(b.x, w.ln1w, w.ln1b, c.enc_norm_eps, R, EH, b.n, e.stream);
        lin(b.n, EH, w.qkv, 3 * AO, b.qkv, 0, nullptr, nullptr);
        launch_enc_rope(b.qkv, W.rope_cs, W.rope_sn, W.rope_rows, c.enc_heads, c.enc_head_dim, spans, n_clips, maxT, e.stream);
        launch_enc_attn(b.qkv, b.a, c.enc_heads, c.enc_head_dim, c.enc_window, 1.0f / sqrtf((float)c.enc_head_dim), spans, n_clips, maxT, e.stream);
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
