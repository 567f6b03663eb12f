// q3_capi.cpp — extern "C" surface declared in include/q3tts.h.  No exception crosses the ABI.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "q3_audio.h"
#include "q3_bpe.h"
#include "q3_engine.h"
#include "q3_job.h"

using q3::Engine;

struct q3tts_engine {
    Engine* e = nullptr;
    std::string err;
    q3::StageSettings stages;   // what the q3tts_engine_set_* entries leave for the streaming jobs (q3_job.h)
};
static std::string g_create_err;

#define Q3_API_BEGIN(h)                                       \
    if (!(h) || !(h)->e) return -1;                           \
    try {                                                     \
        (void)hipSetDevice((h)->e->device);
#define Q3_API_END(h)                                         \
    }                                                         \
    catch (const q3::Error& ex) { (h)->err = ex.msg; return -1; } \
    catch (const std::exception& ex) { (h)->err = ex.what(); return -1; } \
    catch (...) { (h)->err = "unknown error"; return -1; }

extern "C" {

int q3tts_default_config(const char* name, q3tts_config* o) {
    if (!o || !name) return -1;
    const bool big = strcmp(name, "1.7b") == 0 || strcmp(name, "1.7B") == 0;
    if (!big && strcmp(name, "0.6b") != 0 && strcmp(name, "0.6B") != 0) return -1;
    memset(o, 0, sizeof *o);
    // talker dims: reference src/tts_onnx.h:31-37; the rest [HINT]
    o->hidden = 1024; o->n_layers = 28; o->n_heads = 16; o->n_kv_heads = 8; o->head_dim = 128; o->ffn = 3072; o->vocab = 3072;
    o->rope_theta = 1e6f; o->rms_eps = 1e-6f;
    o->cp_layers = 5; o->cp_heads = 16; o->cp_kv_heads = 8; o->cp_head_dim = 128; o->cp_ffn = 3072; o->n_groups = 16; o->sub_vocab = 2048;
    o->cp_rope_theta = 1e6f; o->cp_rms_eps = 1e-6f;
    o->text_vocab = 151936; o->text_hidden = 2048;
    o->cd_codebook = 2048; o->cd_hidden = 1024; o->cd_layers = 8; o->cd_heads = 16; o->cd_head_dim = 64; o->cd_ffn = 3072; o->cd_window = 72;
    o->cd_rope_theta = 10000.0f; o->cd_rms_eps = 1e-5f;
    o->cd_n_up = 2; o->cd_up_ratios[0] = 2; o->cd_up_ratios[1] = 2;
    o->cd_decoder_dim = 1536; o->cd_n_blocks = 4;
    o->cd_up_rates[0] = 8; o->cd_up_rates[1] = 5; o->cd_up_rates[2] = 4; o->cd_up_rates[3] = 3;
    o->cd_tconv_trim = 0;
    o->codec_eos = 2150; o->suppress_begin = 2048; o->suppress_end = 3072;
    // speaker encoder of the Base checkpoints [HINT: Qwen3-TTS speaker_encoder_config]: ECAPA-TDNN 512/1536 channels -> hidden
    o->spk_enc_dim = 1024; o->spk_mel = 128; o->spk_channels = 512; o->spk_scale = 8; o->spk_se = 128; o->spk_att = 128;
    if (big) { // [HINT: the public 1.7B checkpoints] talker twice as wide, predictor at the 0.6B width behind cp.proj, speaker row talker-wide.
               // Beyond the reference: README.md:125 lists 1.7B as planned and tts_onnx.h:31-37 hard-codes the 0.6B dims.
        o->hidden = 2048; o->ffn = 6144; o->cp_hidden = 1024; o->spk_enc_dim = 2048;
    }
    return 0;
}

int q3tts_config_enable_audio_encoder(q3tts_config* o) {
    if (!o) return -1;
    // [HINT: transformers MimiConfig defaults, as the Qwen3-TTS 12 Hz tokenizer uses them] upsampling_ratios (8, 6, 5, 4) reversed
    o->enc_hidden = 512; o->enc_filters = 64; o->enc_n_ratios = 4;
    o->enc_ratios[0] = 4; o->enc_ratios[1] = 5; o->enc_ratios[2] = 6; o->enc_ratios[3] = 8;
    o->enc_kernel = 7; o->enc_res_kernel = 3; o->enc_last_kernel = 3;
    o->enc_layers = 8; o->enc_heads = 8; o->enc_head_dim = 64; o->enc_ffn = 2048; o->enc_window = 250;
    o->enc_vq_dim = 256; o->enc_codebook = 2048;
    o->enc_rope_theta = 10000.0f; o->enc_norm_eps = 1e-5f;
    return 0;
}

int q3tts_config_num_tensors(const q3tts_config* cfg) {
    if (!cfg) return -1;
    try { return (int)q3::tensor_specs(*cfg).size(); } catch (...) { return -1; }
}
int q3tts_config_tensor_info(const q3tts_config* cfg, int index, char* name, int name_cap, int64_t* shape4, int* ndim, int* kind) {
    if (!cfg) return -1;
    try {
        const std::vector<q3::TensorSpec> specs = q3::tensor_specs(*cfg);
        if (index < 0 || index >= (int)specs.size()) return -1;
        const q3::TensorSpec& t = specs[index];
        if (name && name_cap > 0) { snprintf(name, (size_t)name_cap, "%s", t.name.c_str()); }
        if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
        if (ndim) *ndim = t.ndim;
        if (kind) *kind = t.kind;
        return 0;
    } catch (...) { return -1; }
}

q3tts_engine* q3tts_create(const q3tts_config* cfg, int device, int max_batch, int max_ctx, uint32_t flags) {
    return q3tts_create_pooled(cfg, device, max_batch, max_ctx, 0, flags);
}

q3tts_engine* q3tts_create_pooled(const q3tts_config* cfg, int device, int max_batch, int max_ctx, int64_t kv_pool_tokens, uint32_t flags) {
    if (!cfg) { g_create_err = "null config"; return nullptr; }
    try {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw q3::Error("no HIP device: libq3tts_hip needs an MI355X (gfx950); there is no CPU fallback");
        if (device < 0 || device >= n) throw q3::Error("device index out of range");
        if (const char* ng = getenv("Q3TTS_NO_GRAPH")) if (ng[0] == '1') flags |= Q3TTS_FLAG_NO_GRAPH; // profiling aid
        q3tts_engine* h = new q3tts_engine;
        h->e = new Engine(*cfg, device, max_batch, max_ctx, flags, kv_pool_tokens);
        return h;
    } catch (const q3::Error& ex) { g_create_err = ex.msg; }
    catch (const std::exception& ex) { g_create_err = ex.what(); }
    catch (...) { g_create_err = "unknown error"; }
    return nullptr;
}

q3tts_engine* q3tts_create_sharing(q3tts_engine* donor, int max_batch, int max_ctx, int64_t kv_pool_tokens, uint32_t flags) {
    if (!donor || !donor->e) { g_create_err = "weight sharing: null donor"; return nullptr; }
    try {
        // of the donor only what never changes after its creation is read: config, device, flags, the pointer to its set
        const Engine& d = *donor->e;
        if (!d.ws.is_published()) throw q3::Error("weight sharing: the donor's weights are not finalized");
        if ((flags ^ d.flags) & Q3TTS_FLAG_FP32_CODEC)
            throw q3::Error("weight sharing: Q3TTS_FLAG_FP32_CODEC must equal the donor's (the codec's derived weight layout depends on it)");
        if (const char* ng = getenv("Q3TTS_NO_GRAPH")) if (ng[0] == '1') flags |= Q3TTS_FLAG_NO_GRAPH; // profiling aid
        (void)hipSetDevice(d.device);
        q3tts_engine* h = new q3tts_engine;
        try { h->e = new Engine(d.c, d.device, max_batch, max_ctx, flags, kv_pool_tokens, d.hold.set); }
        catch (...) { delete h; throw; }
        return h;
    } catch (const q3::Error& ex) { g_create_err = ex.msg; }
    catch (const std::exception& ex) { g_create_err = ex.what(); }
    catch (...) { g_create_err = "unknown error"; }
    return nullptr;
}

int q3tts_weights_info(q3tts_engine* h, int64_t* shared_bytes, int* holders, int64_t* private_weight_bytes) {
    Q3_API_BEGIN(h)
    if (shared_bytes) *shared_bytes = h->e->ws.n_bytes();
    if (holders) *holders = h->e->ws.n_holders();
    if (private_weight_bytes) *private_weight_bytes = h->e->private_weight_bytes();
    return 0;
    Q3_API_END(h)
}

void q3tts_destroy(q3tts_engine* h) {
    if (!h) return;
    delete h->e;
    delete h;
}

const char* q3tts_last_error(q3tts_engine* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int q3tts_num_tensors(q3tts_engine* h) { return h && h->e ? (int)h->e->tensors.size() : -1; }

int q3tts_tensor_info(q3tts_engine* h, int i, char* name, int cap, int64_t* shape4, int* ndim) {
    Q3_API_BEGIN(h)
    if (i < 0 || i >= (int)h->e->tensors.size()) throw q3::Error("tensor index out of range");
    const q3::Tensor& t = h->e->tensors[i];
    if (name && cap > 0) { strncpy(name, t.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (shape4) for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
    if (ndim) *ndim = t.ndim;
    return 0;
    Q3_API_END(h)
}

int q3tts_set_tensor_host(q3tts_engine* h, const char* name, const float* data, int64_t n) {
    Q3_API_BEGIN(h) h->e->set_tensor(name, data, n); return 0; Q3_API_END(h)
}
int q3tts_get_tensor_host(q3tts_engine* h, const char* name, float* out, int64_t n) {
    Q3_API_BEGIN(h) h->e->get_tensor(name, out, n); return 0; Q3_API_END(h)
}
int q3tts_fill_synthetic(q3tts_engine* h, uint64_t seed) {
    Q3_API_BEGIN(h) h->e->fill_synthetic(seed); return 0; Q3_API_END(h)
}
int q3tts_finalize(q3tts_engine* h) {
    Q3_API_BEGIN(h) h->e->finalize(); return 0; Q3_API_END(h)
}

int q3tts_text_project_host(q3tts_engine* h, const int64_t* ids, int n, float* out) {
    Q3_API_BEGIN(h) h->e->text_project(ids, n, out); return 0; Q3_API_END(h)
}
int q3tts_frame_rows_host(q3tts_engine* h, const int64_t* codes, int n, int frame0, const float* trailing, int n_trailing, float* out) {
    Q3_API_BEGIN(h) h->e->frame_rows(codes, n, frame0, trailing, n_trailing, out); return 0; Q3_API_END(h)
}
int q3tts_codec_embed_host(q3tts_engine* h, const int64_t* ids, int n, float* out) {
    Q3_API_BEGIN(h) h->e->codec_embed(ids, n, out); return 0; Q3_API_END(h)
}
int q3tts_cp_embed_host(q3tts_engine* h, int64_t id, int step, float* out) {
    Q3_API_BEGIN(h) h->e->cp_embed(id, step, out); return 0; Q3_API_END(h)
}
int q3tts_talker_prefill_host(q3tts_engine* h, int slot, const float* embeds, int S, float* logits, float* last_hidden) {
    Q3_API_BEGIN(h) h->e->talker_prefill(slot, embeds, S, logits, last_hidden); return 0; Q3_API_END(h)
}
int q3tts_talker_decode_host(q3tts_engine* h, int slot, const float* embed, float* logits, float* last_hidden) {
    Q3_API_BEGIN(h) h->e->talker_decode(slot, embed, logits, last_hidden); return 0; Q3_API_END(h)
}
int q3tts_code_predictor_host(q3tts_engine* h, const float* seq, int n, int step, float* logits) {
    Q3_API_BEGIN(h) h->e->code_predictor(seq, n, step, logits); return 0; Q3_API_END(h)
}
int q3tts_codec_decode_host(q3tts_engine* h, const int64_t* codes, int F, float* pcm, int64_t cap, int64_t* out_len) {
    Q3_API_BEGIN(h)
    const int64_t n = h->e->codec_decode_host(codes, F, pcm, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}

int q3tts_codec_decode_batch_host(q3tts_engine* h, int n_utt, const int64_t* codes, const int32_t* frame_offsets, float* const* pcm_out, int64_t pcm_cap,
                                  int64_t* pcm_len) {
    Q3_API_BEGIN(h)
    Engine& e = *h->e;
    if (n_utt <= 0) return 0;
    if (!codes || !frame_offsets) throw q3::Error("codec_decode_batch: null argument");
    if (pcm_cap < 0) throw q3::Error("codec_decode_batch: negative pcm_cap");
    if (!e.finalized) throw q3::Error("weights not finalized");
    const int G = e.c.n_groups;
    int row_frames = 1;
    std::vector<int32_t> nf((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) {
        const int64_t f = (int64_t)frame_offsets[u + 1] - frame_offsets[u];
        if (f < 0) throw q3::Error("codec_decode_batch: frame_offsets must not decrease");
        if (f > e.max_frames_cap) throw q3::Error("codec_decode: F out of range");   // the single-utterance entry point's bound and message
        nf[(size_t)u] = (int32_t)f;
        row_frames = std::max(row_frames, (int)f);
    }
    e.codec_async_prepare(row_frames, n_utt);
    std::vector<int32_t> rows((size_t)n_utt * row_frames * G, 0);
    for (int u = 0; u < n_utt; ++u) {
        const int64_t* src = codes + (size_t)frame_offsets[u] * G;
        int32_t* dst = rows.data() + (size_t)u * row_frames * G;
        q3::stage_codes<q3::Error>(src, (size_t)nf[(size_t)u] * G, e.c.cd_codebook, dst);   // as q3tts_codec_decode_host
    }
    e.codec_job_upload(rows.data(), n_utt, row_frames);
    q3::vocoder_job(e, n_utt, nf, row_frames, pcm_out, pcm_cap, pcm_len);
    return 0;
    Q3_API_END(h)
}

int q3tts_codec_decode_dev(q3tts_engine* h, const int32_t* codes_dev, int F, float* pcm_dev, int64_t cap, int64_t* out_len) {
    Q3_API_BEGIN(h)
    const int64_t n = h->e->codec_decode_dev(codes_dev, F, pcm_dev, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}
void* q3tts_stream(q3tts_engine* h) { return h && h->e ? (void*)h->e->stream : nullptr; }

int q3tts_codec_decode_chunked_host(q3tts_engine* h, const int64_t* codes, int F, int chunk_frames, int left_context, float* pcm, int64_t cap,
                                    int64_t* out_len) {
    Q3_API_BEGIN(h)
    const int64_t n = h->e->codec_decode_chunked_host(codes, F, chunk_frames, left_context, pcm, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_begin(q3tts_engine* h, int max_frames, int* stream_id) {
    Q3_API_BEGIN(h)
    if (!stream_id) throw q3::Error("codec_stream_begin: null output");
    *stream_id = h->e->codec_stream_begin(max_frames);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_push_host(q3tts_engine* h, int stream_id, const int64_t* codes, int n_frames, float* pcm, int64_t cap, int64_t* out_len) {
    Q3_API_BEGIN(h)
    if (!codes) throw q3::Error("codec_stream_push: null codes");
    const int64_t n = h->e->codec_stream_push_host(stream_id, codes, n_frames, pcm, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_end(q3tts_engine* h, int stream_id) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_end(stream_id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_push_batch_host(q3tts_engine* h, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets,
                                       float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_push_batch_host(n_streams, stream_ids, codes, frame_offsets, pcm_out, pcm_cap, pcm_len);
    return 0;
    Q3_API_END(h)
}
int q3tts_slots_codec_decode_new_host(q3tts_engine* h, int n_slots, const int32_t* slots, float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len,
                                      int32_t* frame_begin, int32_t* frame_end) {
    Q3_API_BEGIN(h)
    h->e->slots_codec_decode_new(n_slots, slots, pcm_out, pcm_cap, pcm_len, frame_begin, frame_end);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_prime_batch_host(q3tts_engine* h, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_prime_batch_host(n_streams, stream_ids, codes, frame_offsets);
    return 0;
    Q3_API_END(h)
}
int q3tts_slots_codec_prime(q3tts_engine* h, int n_slots, const int32_t* slots, const int32_t* n_frames) {
    Q3_API_BEGIN(h)
    h->e->slots_codec_prime(n_slots, slots, n_frames);
    return 0;
    Q3_API_END(h)
}
// ---- PCM sinks (include/q3tts.h "audio out at the sink's rate") ----
static thread_local std::string g_sink_err;
const char* q3tts_sink_last_error(void) { return g_sink_err.c_str(); }
int q3tts_sink_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* half, int32_t* taps, float* table, int64_t cap) {
    g_sink_err.clear();
    try {
        q3::SinkPlan d;
        q3::sink_plan_dims(rate, &d);
        if (L) *L = d.L;
        if (M) *M = d.M;
        if (half) *half = d.half;
        if (taps) *taps = d.taps;
        if (table && d.taps > 0 && cap >= (int64_t)d.L * d.taps) {
            const q3::SinkPlan full = q3::sink_plan(rate);
            memcpy(table, full.table.data(), full.table.size() * sizeof(float));
        }
        return 0;
    } catch (const std::exception& ex) { g_sink_err = ex.what(); return -1; }
    catch (...) { g_sink_err = "unknown error"; return -1; }
}
int64_t q3tts_sink_emitted(int32_t rate, int64_t n_received, int finished) {
    g_sink_err.clear();
    try {
        if (n_received < 0) throw std::invalid_argument("pcm sink: negative sample count");
        q3::SinkPlan d;
        q3::sink_plan_dims(rate, &d);
        return q3::sink_emitted(d, n_received, finished != 0);
    } catch (const std::exception& ex) { g_sink_err = ex.what(); return -1; }
    catch (...) { g_sink_err = "unknown error"; return -1; }
}
// G.711 on the host (include/q3tts.h "G.711"): the inline functions of q3_common.h that pcm_sink_store and rs_stream_sample use
int q3tts_g711_encode_host(int format, const int16_t* in, int64_t n, uint8_t* out) {
    if (!q3::pcm_format_g711(format) || n < 0 || (n > 0 && (!in || !out))) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = q3::g711_enc(format, in[i]);
    return 0;
}
int q3tts_g711_decode_host(int format, const uint8_t* in, int64_t n, int16_t* out) {
    if (!q3::pcm_format_g711(format) || n < 0 || (n > 0 && (!in || !out))) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = q3::g711_dec(format, in[i]);
    return 0;
}
int q3tts_pcm_sink_begin(q3tts_engine* h, int32_t sample_rate, int format, int* sink_id) {
    Q3_API_BEGIN(h)
    if (!sink_id) throw q3::Error("pcm sink: NULL argument");
    *sink_id = h->e->sink.begin(sample_rate, format);
    return 0;
    Q3_API_END(h)
}
int q3tts_pcm_sink_push_batch_host(q3tts_engine* h, int n, const int32_t* sink_ids, const float* const* pcm24, const int64_t* n_in,
                                   const uint8_t* finish, void* const* out, int64_t cap_samples, int64_t* out_len) {
    Q3_API_BEGIN(h)
    h->e->sink.push_batch_host(n, sink_ids, pcm24, n_in, finish, out, cap_samples, out_len);
    return 0;
    Q3_API_END(h)
}
int q3tts_pcm_sink_end(q3tts_engine* h, int sink_id) {
    Q3_API_BEGIN(h)
    h->e->sink.end(sink_id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_sink(q3tts_engine* h, int stream_id, int32_t sample_rate, int format) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_set_sink(stream_id, sample_rate, format);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_push_batch_any_host(q3tts_engine* h, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets,
                                           void* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, const uint8_t* finish) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_push_batch_host(n_streams, stream_ids, codes, frame_offsets, (float* const*)pcm_out, pcm_cap, pcm_len, finish, false);
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_sink(q3tts_engine* h, const q3tts_sink* sink) {
    Q3_API_BEGIN(h)
    if (!sink) { h->stages.sink = q3tts_sink{ 0, 0, nullptr, nullptr }; return 0; }
    if (!q3::pcm_format_known(sink->format)) throw q3::Error("engine_set_sink: format " + std::to_string(sink->format) + " is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16, nor Q3TTS_PCM_MULAW (2) or Q3TTS_PCM_ALAW (3)");
    if (!sink->cb) throw q3::Error("engine_set_sink: null callback");
    (void)h->e->sink.plan_for(sink->sample_rate);   // refuses a bad rate by name, and has the table uploaded before the first utterance
    h->stages.sink = *sink;
    return 0;
    Q3_API_END(h)
}

// ---- speaking rate (include/q3tts.h "speaking rate") ----
static thread_local std::string g_speed_err;
const char* q3tts_speed_last_error(void) { return g_speed_err.c_str(); }
int64_t q3tts_speed_emitted(int32_t speed_permille, int64_t n_received, int finished) {
    g_speed_err.clear();
    try {
        q3::speed_check(speed_permille);
        if (n_received < 0) throw std::invalid_argument("speed: negative sample count " + std::to_string(n_received));
        return q3::speed_emitted(speed_permille, n_received, finished != 0);
    } catch (const std::exception& ex) { g_speed_err = ex.what(); return -1; }
    catch (...) { g_speed_err = "unknown error"; return -1; }
}
int q3tts_speed_window(float* table, int64_t cap) {
    g_speed_err.clear();
    if (!table || cap < q3::kSpeedN) { g_speed_err = "speed window: the table holds " + std::to_string(q3::kSpeedN) + " floats"; return -1; }
    const std::vector<float> w = q3::speed_window();
    memcpy(table, w.data(), w.size() * sizeof(float));
    return 0;
}
int q3tts_speed_begin(q3tts_engine* h, int32_t speed_permille, int* id) {
    Q3_API_BEGIN(h)
    if (!id) throw q3::Error("speed: NULL argument");
    *id = h->e->speed.begin(speed_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_speed_push_batch_host(q3tts_engine* h, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len,
                                int32_t* const* offsets_out, int64_t* n_offsets) {
    Q3_API_BEGIN(h)
    h->e->speed.push_batch_host(n, ids, pcm24, n_in, finish, (void* const*)out, cap_samples, out_len, offsets_out, n_offsets);
    return 0;
    Q3_API_END(h)
}
int q3tts_speed_end(q3tts_engine* h, int id) {
    Q3_API_BEGIN(h)
    h->e->speed.end(id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_speed(q3tts_engine* h, int stream_id, int32_t speed_permille) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_set_speed(stream_id, speed_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_speed(q3tts_engine* h, int32_t speed_permille) {
    Q3_API_BEGIN(h)
    try { q3::speed_check(speed_permille); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("engine_set_speed: ") + ex.what()); }
    h->stages.speed = speed_permille;
    return 0;
    Q3_API_END(h)
}

// ---- output level (include/q3tts.h "output level") ----
static thread_local std::string g_level_err;
const char* q3tts_level_last_error(void) { return g_level_err.c_str(); }
float q3tts_level_gain(int32_t gain_cb) {
    g_level_err.clear();
    try {
        q3::level_check(gain_cb, 0);
        return q3::level_gain(gain_cb);
    } catch (const std::exception& ex) { g_level_err = ex.what(); return -1.0f; }
    catch (...) { g_level_err = "unknown error"; return -1.0f; }
}
int64_t q3tts_level_emitted(int32_t gain_cb, int32_t ceiling_permille, int64_t n_received, int finished) {
    g_level_err.clear();
    try {
        q3::level_check(gain_cb, ceiling_permille);
        if (n_received < 0) throw std::invalid_argument("level: negative sample count " + std::to_string(n_received));
        return q3::level_emitted(ceiling_permille, n_received, finished != 0);
    } catch (const std::exception& ex) { g_level_err = ex.what(); return -1; }
    catch (...) { g_level_err = "unknown error"; return -1; }
}
int q3tts_level_begin(q3tts_engine* h, int32_t gain_cb, int32_t ceiling_permille, int* id) {
    Q3_API_BEGIN(h)
    if (!id) throw q3::Error("level: NULL argument");
    *id = h->e->level.begin(gain_cb, ceiling_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_level_push_batch_host(q3tts_engine* h, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len) {
    Q3_API_BEGIN(h)
    h->e->level.push_batch_host(n, ids, pcm24, n_in, finish, (void* const*)out, cap_samples, out_len);
    return 0;
    Q3_API_END(h)
}
int q3tts_level_end(q3tts_engine* h, int id) {
    Q3_API_BEGIN(h)
    h->e->level.end(id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_level(q3tts_engine* h, int stream_id, int32_t gain_cb, int32_t ceiling_permille) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_set_level(stream_id, gain_cb, ceiling_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_level(q3tts_engine* h, int32_t gain_cb, int32_t ceiling_permille) {
    Q3_API_BEGIN(h)
    try { q3::level_check(gain_cb, ceiling_permille); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("engine_set_level: ") + ex.what()); }
    h->stages.gain_cb = gain_cb; h->stages.ceiling = ceiling_permille;
    return 0;
    Q3_API_END(h)
}

// ---- pitch (include/q3tts.h "pitch") ----
static thread_local std::string g_pitch_err;
const char* q3tts_pitch_last_error(void) { return g_pitch_err.c_str(); }
int32_t q3tts_pitch_ratio(double cents) {
    g_pitch_err.clear();
    if (!(cents >= -1200.0 && cents <= 1200.0)) { g_pitch_err = "pitch: " + std::to_string(cents) + " cents is outside -1200 .. +1200"; return -1; }
    return q3::pitch_ratio(cents);
}
int64_t q3tts_pitch_emitted(int64_t n_received, int finished) {
    g_pitch_err.clear();
    if (n_received < 0) { g_pitch_err = "pitch: negative sample count " + std::to_string(n_received); return -1; }
    return q3::pitch_emitted(n_received, finished != 0);
}
int q3tts_pitch_begin(q3tts_engine* h, int32_t ratio_permille, int* id) {
    Q3_API_BEGIN(h)
    if (!id) throw q3::Error("pitch: NULL argument");
    *id = h->e->pitch.begin(ratio_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_pitch_push_batch_host(q3tts_engine* h, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len) {
    Q3_API_BEGIN(h)
    h->e->pitch.push_batch_host(n, ids, pcm24, n_in, finish, (void* const*)out, cap_samples, out_len);
    return 0;
    Q3_API_END(h)
}
int q3tts_pitch_end(q3tts_engine* h, int id) {
    Q3_API_BEGIN(h)
    h->e->pitch.end(id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_pitch(q3tts_engine* h, int stream_id, int32_t ratio_permille) {
    Q3_API_BEGIN(h)
    try { q3::pitch_check(ratio_permille); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("codec_stream_set_pitch: ") + ex.what()); }
    h->e->codec_stream_set_pitch(stream_id, ratio_permille);
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_pitch(q3tts_engine* h, int32_t ratio_permille) {
    Q3_API_BEGIN(h)
    try { q3::pitch_check(ratio_permille); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("engine_set_pitch: ") + ex.what()); }
    h->stages.pitch = ratio_permille;
    return 0;
    Q3_API_END(h)
}

// ---- loudness (include/q3tts.h "loudness") ----
static thread_local std::string g_loud_err;
const char* q3tts_loudness_last_error(void) { return g_loud_err.c_str(); }
int q3tts_loudness_coeffs(int32_t rate, double out[10]) {
    g_loud_err.clear();
    if (!out) { g_loud_err = "loudness: NULL argument"; return -1; }
    if (rate < 8000 || rate > 384000) { g_loud_err = "loudness: rate " + std::to_string(rate) + " is outside 8000 .. 384000"; return -1; }
    q3::loudness_coeffs(rate, out);
    return 0;
}
int64_t q3tts_loudness_emitted(int32_t target_dlufs, int64_t n_received, int finished) {
    g_loud_err.clear();
    if (n_received < 0) { g_loud_err = "loudness: negative sample count " + std::to_string(n_received); return -1; }
    try { q3::loudness_check(target_dlufs, 0, 0); } catch (const std::invalid_argument& ex) { g_loud_err = ex.what(); return -1; }
    return q3::loudness_emitted(target_dlufs, n_received, finished != 0);
}
double q3tts_loudness_lufs(const int64_t* E, int64_t n, int mode) {
    g_loud_err.clear();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (n < 0 || (n > 0 && !E)) { g_loud_err = "loudness: " + std::string(n < 0 ? "negative sub-block count" : "NULL argument"); return nan; }
    if (mode < Q3TTS_LOUDNESS_MOMENTARY || mode > Q3TTS_LOUDNESS_INTEGRATED) { g_loud_err = "loudness: mode " + std::to_string(mode) + " is none of momentary (0), short-term (1), integrated (2)"; return nan; }
    for (int64_t b = 0; b < n; ++b) if (E[b] < 0 || E[b] > ((int64_t)1 << 46)) { g_loud_err = "loudness: energy " + std::to_string(E[b]) + " is no sub-block's"; return nan; }
    return q3::loudness_lufs(E, n, mode);
}
int q3tts_loudness_begin(q3tts_engine* h, int32_t target_dlufs, int32_t range_cb, int32_t start_cb, int* id) {
    Q3_API_BEGIN(h)
    if (!id) throw q3::Error("loudness: NULL argument");
    *id = h->e->loud.begin(target_dlufs, range_cb, start_cb);
    return 0;
    Q3_API_END(h)
}
int q3tts_loudness_push_batch_host(q3tts_engine* h, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                                   float* const* out, int64_t cap_samples, int64_t* out_len, int64_t* const* energies_out, float* const* gains_out,
                                   int64_t* n_blocks) {
    Q3_API_BEGIN(h)
    // the stage reports four 4-byte words per sub-block a push closes (its energies, then its gains): staged here, handed on below
    const bool report = (energies_out || gains_out) && n > 0 && n <= 65535 && n_in;
    std::vector<std::vector<int32_t>> words(report ? (size_t)n : 0);
    std::vector<int32_t*> wptr(report ? (size_t)n : 0);
    for (size_t i = 0; i < words.size(); ++i) {
        words[i].assign(4 * (size_t)(std::max<int64_t>(0, std::min<int64_t>(n_in[i], q3::Engine::kStageMaxPush)) / q3::kLoudBlock + 1), 0);
        wptr[i] = words[i].data();
    }
    std::vector<int64_t> n_words(n > 0 && n <= 65535 ? (size_t)n : 0, 0);
    h->e->loud.push_batch_host(n, ids, pcm24, n_in, finish, (void* const*)out, cap_samples, out_len, report ? wptr.data() : nullptr, n_words.empty() ? nullptr : n_words.data());
    for (size_t i = 0; i < n_words.size(); ++i) {
        const int64_t nb = n_words[i] / 4;
        if (n_blocks) n_blocks[i] = nb;
        if (!report || nb == 0) continue;
        if (energies_out && energies_out[i]) memcpy(energies_out[i], words[i].data(), (size_t)nb * sizeof(int64_t));
        if (gains_out && gains_out[i]) memcpy(gains_out[i], words[i].data() + 2 * nb, (size_t)nb * sizeof(float));
    }
    return 0;
    Q3_API_END(h)
}
int q3tts_loudness_end(q3tts_engine* h, int id) {
    Q3_API_BEGIN(h)
    h->e->loud.end(id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_loudness(q3tts_engine* h, int stream_id, int32_t target_dlufs, int32_t range_cb, int32_t start_cb) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_set_loudness(stream_id, target_dlufs, range_cb, start_cb);
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_loudness(q3tts_engine* h, int enabled, int32_t target_dlufs, int32_t range_cb, int32_t start_cb) {
    Q3_API_BEGIN(h)
    if (enabled) {
        try { q3::loudness_check(target_dlufs, range_cb, start_cb); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("engine_set_loudness: ") + ex.what()); }
        h->stages.loud_target = target_dlufs; h->stages.loud_range = range_cb; h->stages.loud_start = start_cb;
    }
    h->stages.loud = enabled != 0;
    return 0;
    Q3_API_END(h)
}

// ---- tone (include/q3tts.h "tone") ----
static_assert(sizeof(q3tts_tone_section) == sizeof(q3::ToneSection) && offsetof(q3tts_tone_section, q_permille) == offsetof(q3::ToneSection, q_permille), "q3tts_tone_section is q3::ToneSection");
static const q3::ToneSection* tone_sections_of(const q3tts_tone_section* s) { return reinterpret_cast<const q3::ToneSection*>(s); }
static thread_local std::string g_tone_err;
const char* q3tts_tone_last_error(void) { return g_tone_err.c_str(); }
int q3tts_tone_coeffs(int32_t n, const q3tts_tone_section* sections, double (*out)[5]) {
    g_tone_err.clear();
    try {
        if (!out) throw std::invalid_argument("tone: NULL argument");
        q3::tone_check(n, tone_sections_of(sections));
        q3::tone_coeffs(n, tone_sections_of(sections), out);
        return 0;
    } catch (const std::exception& ex) { g_tone_err = ex.what(); return -1; }
    catch (...) { g_tone_err = "unknown error"; return -1; }
}
int q3tts_tone_parse(const char* spec, q3tts_tone_section* out, int32_t* n) {
    g_tone_err.clear();
    try {
        if (!spec || !out || !n) throw std::invalid_argument("tone: NULL argument");
        const std::vector<q3::ToneSection> v = q3::tone_parse(spec);
        for (size_t j = 0; j < v.size(); ++j) out[j] = q3tts_tone_section{ v[j].kind, v[j].freq_hz, v[j].gain_cb, v[j].q_permille };
        *n = (int32_t)v.size();
        return 0;
    } catch (const std::exception& ex) { g_tone_err = ex.what(); return -1; }
    catch (...) { g_tone_err = "unknown error"; return -1; }
}
int q3tts_tone_begin(q3tts_engine* h, int32_t n, const q3tts_tone_section* sections, int* id) {
    Q3_API_BEGIN(h)
    if (!id) throw q3::Error("tone: NULL argument");
    *id = h->e->tone.begin(n, tone_sections_of(sections));
    return 0;
    Q3_API_END(h)
}
int q3tts_tone_push_batch_host(q3tts_engine* h, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                               const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len) {
    Q3_API_BEGIN(h)
    h->e->tone.push_batch_host(n, ids, pcm24, n_in, finish, (void* const*)out, cap_samples, out_len);
    return 0;
    Q3_API_END(h)
}
int q3tts_tone_end(q3tts_engine* h, int id) {
    Q3_API_BEGIN(h)
    h->e->tone.end(id);
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_stream_set_tone(q3tts_engine* h, int stream_id, int32_t n, const q3tts_tone_section* sections) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_set_tone(stream_id, n, tone_sections_of(sections));
    return 0;
    Q3_API_END(h)
}
int q3tts_engine_set_tone(q3tts_engine* h, int32_t n, const q3tts_tone_section* sections) {
    Q3_API_BEGIN(h)
    if (n != 0) {
        try { q3::tone_check(n, tone_sections_of(sections)); } catch (const std::invalid_argument& ex) { throw q3::Error(std::string("engine_set_tone: ") + ex.what()); }
        for (int j = 0; j < n; ++j) h->stages.tone[j] = tone_sections_of(sections)[j];
    }
    h->stages.tone_n = n;
    return 0;
    Q3_API_END(h)
}

int q3tts_codec_stream_info(q3tts_engine* h, int stream_id, int* n_done, int* kv_capacity_rows, int64_t* bytes) {
    Q3_API_BEGIN(h)
    h->e->codec_stream_info(stream_id, n_done, kv_capacity_rows, bytes);
    return 0;
    Q3_API_END(h)
}
int q3tts_slot_codec_decode_range_host(q3tts_engine* h, int slot, int frame_begin, int frame_end, int left_context, float* pcm, int64_t cap,
                                       int64_t* out_len) {
    Q3_API_BEGIN(h)
    const int64_t n = h->e->slot_codec_decode_range(slot, frame_begin, frame_end, left_context, pcm, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}

int64_t q3tts_codec_decode_len(const q3tts_config* c, int F) {
    return q3::codec_decode_len(*c, F);
}

int q3tts_sample_host(q3tts_engine* h, const float* logits, int n, const q3tts_sampling* p, float u, int suppress, int64_t* token) {
    Q3_API_BEGIN(h) h->e->sample(logits, n, *p, u, suppress, token); return 0; Q3_API_END(h)
}

int q3tts_sample_hist_host(q3tts_engine* h, const float* logits, int n, const q3tts_sampling* p, float u, int suppress,
                           const int64_t* history, int n_history, int64_t* token) {
    Q3_API_BEGIN(h)
    if (!logits || !p || !token) throw q3::Error("sample_hist: null argument");
    h->e->sample_hist(logits, n, *p, u, suppress, history, n_history, token);
    return 0;
    Q3_API_END(h)
}

static uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float q3tts_rng_uniform(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t group) {
    uint64_t k = mix64(seed ^ mix64(((uint64_t)stream << 32) | frame));
    k = mix64(k + group);
    return (float)(k >> 40) * (1.0f / 16777216.0f);
}

// [HINT], unpinned (include/q3tts.h): the chat-turn frame of an instruction
static const int64_t INSTRUCT_HEAD[3] = { 151644, 872, 198 }, INSTRUCT_TAIL[2] = { 151645, 198 };
int64_t q3tts_frame_instruct_ids(const int32_t* text_ids, int64_t n, int64_t* out, int64_t cap) {
    if (n < 0 || (n > 0 && !text_ids) || cap < 0 || (cap > 0 && !out)) return -1;
    const int64_t total = n + 5;
    for (int64_t i = 0; i < total && i < cap; ++i)
        out[i] = i < 3 ? INSTRUCT_HEAD[i] : (i < 3 + n ? (int64_t)text_ids[i - 3] : INSTRUCT_TAIL[i - 3 - n]);
    return total;
}

int q3tts_build_prompt_instruct_host(q3tts_engine* h, const int64_t* ids, int n_ids, int lang, const float* speaker,
                                     const int64_t* instruct_ids, int n_instruct,
                                     float* prompt, int cap_prompt_rows, int* S, float* trailing, int cap_rows, int* n_trailing) {
    Q3_API_BEGIN(h)
    if (n_instruct < 0 || (n_instruct > 0 && !instruct_ids)) throw q3::Error("build_prompt_instruct: bad instruction");
    if (!prompt || !S || cap_prompt_rows < n_instruct + 16) throw q3::Error("build_prompt_instruct: the prompt buffer needs n_instruct + 16 rows");
    const size_t H = (size_t)h->e->c.hidden;
    if (n_instruct > 0) h->e->text_project(instruct_ids, n_instruct, prompt);
    int S0 = 0;
    h->e->build_prompt(ids, n_ids, lang, speaker, prompt + (size_t)n_instruct * H, &S0, trailing, cap_rows, n_trailing);
    *S = n_instruct + S0;
    return 0;
    Q3_API_END(h)
}

int q3tts_build_prompt_host(q3tts_engine* h, const int64_t* ids, int n_ids, int lang, const float* speaker,
                            float* prompt, int* S, float* trailing, int cap_rows, int* n_trailing) {
    Q3_API_BEGIN(h) h->e->build_prompt(ids, n_ids, lang, speaker, prompt, S, trailing, cap_rows, n_trailing); return 0; Q3_API_END(h)
}

int q3tts_build_prompt_open_host(q3tts_engine* h, const int64_t* ids, int n_ids, int lang, const float* speaker,
                                 float* prompt, int* S, float* trailing, int cap_rows, int* n_trailing) {
    Q3_API_BEGIN(h) h->e->build_prompt_open(ids, n_ids, lang, speaker, prompt, S, trailing, cap_rows, n_trailing); return 0; Q3_API_END(h)
}

int q3tts_slot_begin(q3tts_engine* h, int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                     const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos) {
    Q3_API_BEGIN(h) h->e->slot_begin(slot, prompt, S, trailing, n_trailing, *p, seed, stream_id, ignore_eos); return 0; Q3_API_END(h)
}
int q3tts_slot_begin_codes(q3tts_engine* h, int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                           const int64_t* prefix_codes, int n_prefix,
                           const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos) {
    Q3_API_BEGIN(h)
    if (!p) throw q3::Error("slot_begin_codes: null argument");
    Engine::SlotInit in;
    in.slot = slot; in.prompt = prompt; in.S = S; in.trailing = trailing; in.n_trailing = n_trailing; in.stream_id = stream_id;
    in.prefix = prefix_codes; in.n_prefix = n_prefix;
    h->e->slots_begin(&in, 1, *p, seed, ignore_eos);
    return 0;
    Q3_API_END(h)
}
// ---- shared prompt prefix (run_prefill, tts_onnx.cpp:615-665, once for many utterances): Engine::prefix_create / slots_begin_prefixed ----
int q3tts_prefix_create(q3tts_engine* h, const float* rows, int n_rows, int* prefix_id) {
    Q3_API_BEGIN(h)
    if (!prefix_id) throw q3::Error("prefix_create: null output");
    *prefix_id = h->e->prefix_create(rows, n_rows);
    return 0;
    Q3_API_END(h)
}
int q3tts_prefix_create_instruct(q3tts_engine* h, const int64_t* framed_ids, int n, int* prefix_id) {
    Q3_API_BEGIN(h)
    if (!prefix_id || !framed_ids) throw q3::Error("prefix_create_instruct: null argument");
    if (n < 1 || n >= h->e->max_ctx) throw q3::Error("prefix_create: 1 <= rows < max_ctx");
    std::vector<float> rows((size_t)n * (size_t)h->e->c.hidden);
    h->e->text_project(framed_ids, n, rows.data());
    *prefix_id = h->e->prefix_create(rows.data(), n);
    return 0;
    Q3_API_END(h)
}
int q3tts_prefix_info(q3tts_engine* h, int prefix_id, int* n_rows, int64_t* bytes) {
    Q3_API_BEGIN(h)
    const Engine::Prefix& pf = h->e->prefix_get(prefix_id);
    if (n_rows) *n_rows = pf.P;
    if (bytes) *bytes = pf.bytes;
    return 0;
    Q3_API_END(h)
}
int q3tts_prefix_release(q3tts_engine* h, int prefix_id) {
    Q3_API_BEGIN(h) h->e->prefix_release(prefix_id); return 0; Q3_API_END(h)
}
int q3tts_slot_begin_prefixed(q3tts_engine* h, int slot, int prefix_id, const float* prompt, int S, const float* trailing, int n_trailing,
                              const int64_t* prefix_codes, int n_prefix_frames, const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos) {
    Q3_API_BEGIN(h)
    if (!p) throw q3::Error("slot_begin_prefixed: null argument");
    Engine::SlotInit in;
    in.slot = slot; in.prompt = prompt; in.S = S; in.trailing = trailing; in.n_trailing = n_trailing; in.stream_id = stream_id;
    in.prefix = prefix_codes; in.n_prefix = n_prefix_frames; in.prefix_id = prefix_id;
    h->e->slots_begin_prefixed(&in, 1, *p, seed, ignore_eos);
    return 0;
    Q3_API_END(h)
}
int q3tts_slots_begin_prefixed(q3tts_engine* h, int n, const int32_t* slots, const int32_t* prefix_ids, const float* const* prompts, const int32_t* S,
                               const float* const* trailing, const int32_t* n_trailing, const q3tts_sampling* p, uint64_t seed,
                               const uint32_t* stream_ids, int ignore_eos) {
    Q3_API_BEGIN(h)
    if (n < 1) return 0;
    if (!p || !slots || !prompts || !S) throw q3::Error("slots_begin_prefixed: null argument");
    std::vector<Engine::SlotInit> in((size_t)n);
    for (int i = 0; i < n; ++i) {
        Engine::SlotInit& q = in[(size_t)i];
        q.slot = slots[i]; q.prompt = prompts[i]; q.S = S[i];
        q.n_trailing = n_trailing ? n_trailing[i] : 0; q.trailing = trailing && q.n_trailing > 0 ? trailing[i] : nullptr;
        if (q.n_trailing > 0 && !q.trailing) throw q3::Error("slots_begin_prefixed: trailing rows announced but not given");
        q.stream_id = stream_ids ? stream_ids[i] : (uint32_t)i;
        q.prefix_id = prefix_ids ? prefix_ids[i] : -1;
    }
    h->e->slots_begin_prefixed(in.data(), n, *p, seed, ignore_eos);
    return 0;
    Q3_API_END(h)
}
int q3tts_slots_begin_ragged(q3tts_engine* h, int n, const int32_t* slots, const int32_t* prefix_ids, const float* const* prompts, const int32_t* S,
                             const float* const* trailing, const int32_t* n_trailing, const int64_t* const* prefix_codes, const int32_t* n_prefix_frames,
                             const q3tts_sampling* p, uint64_t seed, const uint32_t* stream_ids, int ignore_eos) {
    Q3_API_BEGIN(h)
    if (n < 1) return 0;
    if (!p || !slots || !prompts || !S) throw q3::Error("slots_begin_ragged: null argument");
    std::vector<Engine::SlotInit> in((size_t)n);
    for (int i = 0; i < n; ++i) {
        Engine::SlotInit& q = in[(size_t)i];
        q.slot = slots[i]; q.prompt = prompts[i]; q.S = S[i];
        q.n_trailing = n_trailing ? n_trailing[i] : 0; q.trailing = trailing && q.n_trailing > 0 ? trailing[i] : nullptr;
        if (q.n_trailing > 0 && !q.trailing) throw q3::Error("slots_begin_ragged: trailing rows announced but not given");
        q.stream_id = stream_ids ? stream_ids[i] : (uint32_t)i;
        q.prefix_id = prefix_ids ? prefix_ids[i] : -1;
        q.n_prefix = n_prefix_frames ? n_prefix_frames[i] : 0;
        q.prefix = prefix_codes && q.n_prefix != 0 ? prefix_codes[i] : nullptr;
    }
    h->e->slots_begin_ragged(in.data(), n, *p, seed, ignore_eos);
    return 0;
    Q3_API_END(h)
}
int q3tts_decode_steps(q3tts_engine* h, int n_steps) {
    Q3_API_BEGIN(h) return h->e->decode_steps(n_steps); Q3_API_END(h)
}
int q3tts_slot_status(q3tts_engine* h, int slot, int* n_frames, int* finished) {
    Q3_API_BEGIN(h) h->e->slot_status(slot, n_frames, finished); return 0; Q3_API_END(h)
}
// ---- live text (Engine::slot_text_open / slots_text_append / slot_text_status; tts_onnx.cpp:531-536, :833-842) ----
int q3tts_slot_text_open(q3tts_engine* h, int slot) {
    Q3_API_BEGIN(h) h->e->slot_text_open(slot); return 0; Q3_API_END(h)
}
int q3tts_slot_text_append_host(q3tts_engine* h, int slot, const float* rows, int n_rows, int close) {
    Q3_API_BEGIN(h)
    if (n_rows < 0 || (n_rows > 0 && !rows)) throw q3::Error("text_append: bad arguments");
    const int32_t sl = slot, offsets[2] = { 0, n_rows };
    const uint8_t cl = close ? 1 : 0;
    if (n_rows > 0) h->e->slots_text_append(1, &sl, rows, nullptr, offsets, &cl);
    else h->e->slots_text_append(1, &sl, nullptr, nullptr, offsets, &cl);
    return 0;
    Q3_API_END(h)
}
int q3tts_slots_text_append_ids(q3tts_engine* h, int n, const int32_t* slots, const int64_t* ids, const int32_t* offsets, const uint8_t* close) {
    Q3_API_BEGIN(h)
    if (n < 0) throw q3::Error("text_append: bad arguments");
    h->e->slots_text_append(n, slots, nullptr, ids, offsets, close);
    return 0;
    Q3_API_END(h)
}
int q3tts_slot_text_status(q3tts_engine* h, int slot, int* n_text_rows, int* open, int* starved) {
    Q3_API_BEGIN(h) h->e->slot_text_status(slot, n_text_rows, open, starved); return 0; Q3_API_END(h)
}
int q3tts_slot_codes_host(q3tts_engine* h, int slot, int64_t* codes, int cap_frames) {
    Q3_API_BEGIN(h) h->e->slot_codes(slot, codes, cap_frames); return 0; Q3_API_END(h)
}
int q3tts_slot_logits_host(q3tts_engine* h, int slot, float* logits, float* last_hidden) {
    Q3_API_BEGIN(h) h->e->slot_logits(slot, logits, last_hidden); return 0; Q3_API_END(h)
}
int q3tts_slot_codec_decode_host(q3tts_engine* h, int slot, float* pcm, int64_t cap, int64_t* out_len) {
    Q3_API_BEGIN(h)
    const int64_t n = h->e->slot_codec_decode(slot, pcm, cap);
    if (out_len) *out_len = n;
    return 0;
    Q3_API_END(h)
}
int q3tts_kv_pool_info(q3tts_engine* h, int* page_tokens, int* total_pages, int* free_pages) {
    Q3_API_BEGIN(h)
    if (page_tokens) *page_tokens = 1 << h->e->talker.page_shift;
    if (total_pages) *total_pages = h->e->kv_total_pages();
    if (free_pages) *free_pages = h->e->kv_free_pages();
    return 0;
    Q3_API_END(h)
}

int q3tts_sched_stats(q3tts_engine* h, int64_t* admitted, int64_t* preempted, int* peak_live) {
    Q3_API_BEGIN(h)
    if (admitted) *admitted = h->e->sched_admitted;
    if (preempted) *preempted = h->e->sched_preempted;
    if (peak_live) *peak_live = h->e->sched_peak_live;
    return 0;
    Q3_API_END(h)
}

int q3tts_slot_release(q3tts_engine* h, int slot) {
    Q3_API_BEGIN(h) h->e->slot_release(slot); return 0; Q3_API_END(h)
}

// ---- the synthesize entries: each fills a q3::JobArgs by name and runs the offline or the streaming job (q3_job.h) ----
// what every entry passes under the same names: the voice's language, sampling, and where the results go
#define Q3_JOB_ARGS(a)                                                                                                             \
    q3::JobArgs a;                                                                                                                 \
    a.n_utt = n_utt; a.lang = lang; a.p = p; a.seed = seed; a.ignore_eos = ignore_eos;                                             \
    a.pcm_out = pcm_out; a.pcm_cap = pcm_cap; a.pcm_len = pcm_len; a.n_frames = n_frames; a.codes_out = codes_out;
static int run_job(q3tts_engine* h, q3::JobArgs& a, bool stream) {   // a streaming job takes the engine's sink and stages as they are now
    Q3_API_BEGIN(h)
    if (stream) { a.stages = h->stages; q3::job_stream(*h->e, a); }
    else q3::job_offline(*h->e, a);
    return 0;
    Q3_API_END(h)
}

// synthesize_tokens (reference src/tts_onnx.cpp:405-436) over a batch of independent utterances:
// waves of up to max_batch slots; prompt assembly -> prefill -> fused decode -> vocoder.
int q3tts_synthesize_batch_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                const q3tts_sampling* p, uint64_t seed, int ignore_eos,
                                float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames,
                                int64_t* codes_out) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets;
    return run_job(h, a, false);
}

int q3tts_synthesize_clone_batch_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                      const float* const* speakers, const q3tts_sampling* p, uint64_t seed, int ignore_eos,
                                      float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames,
                                      int64_t* codes_out) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers;
    return run_job(h, a, false);
}

int q3tts_synthesize_schedule_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames,
                                   int64_t* codes_out) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt;
    return run_job(h, a, false);
}

int q3tts_synthesize_prefixed_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   int chunk_frames, q3tts_audio_cb cb, void* user, const int32_t* prefix_ids) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt;
    a.prefix_ids = prefix_ids; a.chunk_frames = chunk_frames; a.cb = cb; a.user = user;
    return run_job(h, a, cb != nullptr);
}

int q3tts_synthesize_continue_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   const int64_t* prefix_codes, const int32_t* prefix_offsets) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt;
    a.prefix_codes = prefix_codes; a.prefix_offsets = prefix_offsets;
    return run_job(h, a, false);
}

int q3tts_synthesize_instruct_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   int chunk_frames, q3tts_audio_cb cb, void* user,
                                   const int64_t* instruct_ids, const int32_t* instruct_offsets) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt;
    a.instruct_ids = instruct_ids; a.instruct_offsets = instruct_offsets; a.chunk_frames = chunk_frames; a.cb = cb; a.user = user;
    return run_job(h, a, cb != nullptr);
}

// q3tts_synthesize_schedule_host with the audio delivered chunk by chunk (q3::job_stream)
int q3tts_synthesize_stream_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                 const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                 float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                 int chunk_frames, q3tts_audio_cb cb, void* user) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt; a.chunk_frames = chunk_frames; a.cb = cb; a.user = user;
    return run_job(h, a, true);
}
// The same loop behind teacher-forced frames (include/q3tts.h; tts_onnx.cpp:824-842, :759-776): forced begins, primed vocoder streams
int q3tts_synthesize_continue_stream_host(q3tts_engine* h, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                          const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                          float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                          const int64_t* prefix_codes, const int32_t* prefix_offsets,
                                          int chunk_frames, q3tts_audio_cb cb, void* user) {
    Q3_JOB_ARGS(a)
    a.ids = ids; a.offsets = offsets; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt;
    a.prefix_codes = prefix_codes; a.prefix_offsets = prefix_offsets; a.chunk_frames = chunk_frames; a.cb = cb; a.user = user;
    return run_job(h, a, true);
}
// The same loop with the texts pulled through a callback while the audio is generated (include/q3tts.h; tts_onnx.cpp:531-536, :833-842)
int q3tts_synthesize_live_host(q3tts_engine* h, int n_utt, q3tts_text_cb text_cb, void* text_user, int lang,
                               const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                               float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                               int chunk_frames, q3tts_audio_cb cb, void* user) {
    if (!text_cb) { if (h) h->err = "synthesize_live: null text callback"; return -1; }
    Q3_JOB_ARGS(a)
    a.text_cb = text_cb; a.text_user = text_user; a.speakers = speakers; a.max_new_per_utt = max_new_per_utt; a.chunk_frames = chunk_frames; a.cb = cb; a.user = user;
    return run_job(h, a, true);
}

int q3tts_read_wav_host(const char* path, float* out, int64_t cap, int64_t* n_samples, int32_t* sample_rate) {
    if (!path || !n_samples || !sample_rate) return -1;
    try {
        int sr = 0;
        const std::vector<float> a = q3::read_wav(path, &sr);
        if (a.empty()) return -1;
        *n_samples = (int64_t)a.size();
        *sample_rate = sr;
        for (int64_t i = 0; i < (int64_t)a.size() && i < cap && out; ++i) out[i] = a[(size_t)i];
        return 0;
    } catch (...) { return -1; }
}
int q3tts_read_wav_g711_host(const char* path, uint8_t* out, int64_t cap, int64_t* n_samples, int32_t* sample_rate, int* format) {
    if (!path || !n_samples || !sample_rate || !format) return -1;
    try {
        int sr = 0, fmt = 0;
        const std::vector<uint8_t> a = q3::read_wav_g711(path, &sr, &fmt);
        if (a.empty()) return -1;
        *n_samples = (int64_t)a.size();
        *sample_rate = sr;
        *format = fmt;
        if (out && cap > 0) memcpy(out, a.data(), (size_t)std::min<int64_t>(cap, (int64_t)a.size()));
        return 0;
    } catch (const std::invalid_argument&) { return -2; }
    catch (...) { return -1; }
}
int64_t q3tts_resample_host(const float* in, int64_t n, int32_t src_rate, int32_t dst_rate, float* out, int64_t cap) {
    if (n < 0 || (n > 0 && !in) || src_rate <= 0 || dst_rate <= 0) return -1;
    try {
        const std::vector<float> r = q3::resample_linear(std::vector<float>(in, in + n), src_rate, dst_rate);
        for (int64_t i = 0; i < (int64_t)r.size() && i < cap && out; ++i) out[i] = r[(size_t)i];
        return (int64_t)r.size();
    } catch (...) { return -1; }
}
int64_t q3tts_resample_stream_emitted(int32_t src_rate, int32_t dst_rate, int64_t n_received, int finish) {
    if (src_rate <= 0 || dst_rate <= 0 || n_received < 0) return -1;
    return q3::resample_stream_emitted(src_rate, dst_rate, n_received, finish != 0);
}
int q3tts_mel_host(const float* audio, int64_t n, float* mel, int64_t cap, int32_t* frames) {
    if (n < 0 || (n > 0 && !audio) || !frames) return -1;
    try {
        int f = 0;
        const std::vector<float> m = q3::log_mel(std::vector<float>(audio, audio + n), q3::MelSpec(), &f);
        *frames = f;
        if (m.empty()) return -1;
        if (mel) {
            if ((int64_t)m.size() > cap) return -1;
            memcpy(mel, m.data(), m.size() * sizeof(float));
        }
        return 0;
    } catch (...) { return -1; }
}
int q3tts_has_audio_encoder(q3tts_engine* h) { return h && h->e && h->e->has_audio_encoder() ? 1 : 0; }

int64_t q3tts_audio_encode_len(q3tts_engine* h, int64_t n_samples) {
    if (!h || !h->e) return -1;
    if (!h->e->has_audio_encoder()) { h->err = "model has no audio encoder"; return -1; }
    return h->e->audio_encode_len(n_samples);
}

int q3tts_audio_encode_batch_host(q3tts_engine* h, int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates,
                                  int64_t* const* codes_out, const int32_t* caps, int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!codes_out || !caps) throw q3::Error("audio encoder: NULL argument");
    h->e->audio_encode(n_clips, pcm, n_samples, sample_rates, codes_out, nullptr, caps, n_frames);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_encode_batch_latents_host(q3tts_engine* h, int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates,
                                          int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    h->e->audio_encode(n_clips, pcm, n_samples, sample_rates, codes_out, latents_out, caps, n_frames);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_encode_latents_host(q3tts_engine* h, const float* pcm24k, int64_t n_samples, float* latents, int64_t* codes_out, int cap_frames,
                                    int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    const int32_t rate = 24000, cap = cap_frames;
    int32_t nf = 0;
    h->e->audio_encode(1, &pcm24k, &n_samples, &rate, codes_out ? &codes_out : nullptr, latents ? &latents : nullptr, &cap, &nf);
    if (n_frames) *n_frames = nf;
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_encode_host(q3tts_engine* h, const float* pcm24k, int64_t n_samples, int64_t* codes_out, int cap_frames, int32_t* n_frames) {
    if (h && h->e && !codes_out) { h->err = "audio encoder: NULL argument"; return -1; }
    return q3tts_audio_encode_latents_host(h, pcm24k, n_samples, nullptr, codes_out, cap_frames, n_frames);
}

// ---- streamed audio -> codes (Engine::audio_stream_*) ----
int q3tts_audio_stream_begin(q3tts_engine* h, int64_t max_samples, int* stream_id) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!stream_id) throw q3::Error("audio stream: NULL argument");
    *stream_id = h->e->audio_stream_begin(max_samples);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_begin_rate(q3tts_engine* h, int32_t sample_rate, int format, int64_t max_samples, int* stream_id) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!stream_id) throw q3::Error("audio stream: NULL argument");
    *stream_id = h->e->audio_stream_begin(max_samples, sample_rate, format);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_format(q3tts_engine* h, int stream_id, int32_t* sample_rate, int* format) {
    Q3_API_BEGIN(h)
    int32_t fmt = 0;
    h->e->audio_stream_format(stream_id, sample_rate, &fmt);
    if (format) *format = fmt;
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_push_len(q3tts_engine* h, int stream_id, int64_t n_samples, int finish) {
    Q3_API_BEGIN(h)
    return (int)h->e->audio_stream_push_len(stream_id, n_samples, finish != 0);
    Q3_API_END(h)
}

int q3tts_audio_stream_push_batch_host(q3tts_engine* h, int n_streams, const int32_t* stream_ids, const float* const* pcm24k, const int64_t* n_samples,
                                       const int32_t* finish, int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!codes_out || !caps) throw q3::Error("audio stream push: NULL argument");
    h->e->audio_stream_push_batch(n_streams, stream_ids, (const void* const*)pcm24k, n_samples, finish, codes_out, latents_out, caps, n_frames, true);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_push_batch_any_host(q3tts_engine* h, int n_streams, const int32_t* stream_ids, const void* const* pcm, const int64_t* n_samples,
                                           const int32_t* finish, int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!codes_out || !caps) throw q3::Error("audio stream push: NULL argument");
    h->e->audio_stream_push_batch(n_streams, stream_ids, pcm, n_samples, finish, codes_out, latents_out, caps, n_frames, false);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_push_host(q3tts_engine* h, int stream_id, const float* pcm24k, int64_t n_samples, int finish, int64_t* codes_out, int cap_frames,
                                 int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!codes_out) throw q3::Error("audio stream push: NULL argument");
    const int32_t id = stream_id, fin = finish ? 1 : 0, cap = cap_frames;
    int32_t nf = 0;
    const void* p = pcm24k;
    h->e->audio_stream_push_batch(1, &id, &p, &n_samples, &fin, &codes_out, nullptr, &cap, &nf, true);
    if (n_frames) *n_frames = nf;
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_push_any_host(q3tts_engine* h, int stream_id, const void* pcm, int64_t n_samples, int finish, int64_t* codes_out, int cap_frames,
                                     int32_t* n_frames) {
    Q3_API_BEGIN(h)
    if (!h->e->has_audio_encoder()) throw q3::Error("model has no audio encoder");
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    if (!codes_out) throw q3::Error("audio stream push: NULL argument");
    const int32_t id = stream_id, fin = finish ? 1 : 0, cap = cap_frames;
    int32_t nf = 0;
    h->e->audio_stream_push_batch(1, &id, &pcm, &n_samples, &fin, &codes_out, nullptr, &cap, &nf, false);
    if (n_frames) *n_frames = nf;
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_info(q3tts_engine* h, int stream_id, int64_t* n_samples, int32_t* n_frames, int* finished, int64_t* bytes) {
    Q3_API_BEGIN(h)
    h->e->audio_stream_info(stream_id, n_samples, n_frames, finished, bytes);
    return 0;
    Q3_API_END(h)
}

int q3tts_audio_stream_end(q3tts_engine* h, int stream_id) {
    Q3_API_BEGIN(h)
    h->e->audio_stream_end(stream_id);
    return 0;
    Q3_API_END(h)
}

int q3tts_last_audio_encode_ms(q3tts_engine* h, float* ms) {
    if (!h || !h->e || !ms) return -1;
    *ms = h->e->last_audio_encode_ms;
    return 0;
}

int q3tts_test_audio_encoder_transformer_host(q3tts_engine* h, const float* rows, int n_rows, float* out) {
    Q3_API_BEGIN(h)
    if (!h->e->finalized) throw q3::Error("weights not finalized");
    h->e->enc_transformer_host(rows, n_rows, out);
    return 0;
    Q3_API_END(h)
}

int q3tts_has_speaker_encoder(q3tts_engine* h) { return h && h->e && h->e->has_speaker() ? 1 : 0; }
int q3tts_speaker_encoder_host(q3tts_engine* h, const float* mel, int frames, float* embed) {
    Q3_API_BEGIN(h) h->e->speaker_encode(mel, frames, embed); return 0; Q3_API_END(h)
}
int q3tts_extract_speaker_embedding_host(q3tts_engine* h, const char* wav_path, float* embed) {
    Q3_API_BEGIN(h)
    if (!h->e->has_speaker()) throw q3::Error("model has no speaker encoder");
    int sr = 0;
    std::vector<float> a = q3::read_wav(wav_path, &sr);
    if (a.empty()) throw q3::Error(std::string("Failed to read audio: ") + wav_path);
    // the header's 32-bit rate is untrusted: >= 2^31 reads as a negative int (a negative resampling ratio is undefined behaviour)
    if (sr <= 0 || sr > 768000) throw q3::Error(std::string("Failed to read audio: ") + wav_path + " (sample rate " + std::to_string((unsigned)sr) + " out of range)");
    if (sr != 24000) a = q3::resample_linear(a, sr, 24000);
    int frames = 0;
    const std::vector<float> m = q3::log_mel(a, q3::MelSpec(), &frames);
    if (m.empty()) throw q3::Error("Failed to extract mel spectrogram");
    h->e->speaker_encode(m.data(), frames, embed);
    return 0;
    Q3_API_END(h)
}

// ---- the same front end on the GPU, for audio already in memory (q3_speaker.cpp) ----
int64_t q3tts_resample_gpu_host(q3tts_engine* h, const float* in, int64_t n, int32_t src_rate, int32_t dst_rate, float* out, int64_t cap) {
    Q3_API_BEGIN(h) return h->e->resample_gpu(in, n, src_rate, dst_rate, out, cap); Q3_API_END(h)
}
int q3tts_mel_gpu_host(q3tts_engine* h, const float* audio, int64_t n, int32_t sample_rate, float* mel, int64_t cap, int32_t* frames) {
    Q3_API_BEGIN(h)
    int f = 0;
    const bool any = h->e->mel_gpu(audio, n, sample_rate, mel, cap, &f);
    *frames = f;
    if (!any) throw q3::Error("Failed to extract mel spectrogram");   // an empty clip, as q3tts_mel_host
    return 0;
    Q3_API_END(h)
}
int q3tts_speaker_embed_pcm_batch_host(q3tts_engine* h, int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates,
                                       float* embeds) {
    Q3_API_BEGIN(h) h->e->speaker_embed_pcm(n_clips, pcm, n_samples, sample_rates, embeds); return 0; Q3_API_END(h)
}

int q3tts_last_decode_ms(q3tts_engine* h, float* ms, int* steps) {
    Q3_API_BEGIN(h)
    if (ms) *ms = h->e->last_decode_ms;
    if (steps) *steps = h->e->last_decode_steps;
    return 0;
    Q3_API_END(h)
}
int q3tts_last_codec_ms(q3tts_engine* h, float* ms) {
    Q3_API_BEGIN(h) if (ms) *ms = h->e->last_codec_ms; return 0; Q3_API_END(h)
}
int q3tts_counters(q3tts_engine* h, double* dms, int64_t* dsteps, double* cms, int64_t* cframes, int reset) {
    Q3_API_BEGIN(h)
    if (dms) *dms = h->e->total_decode_ms;
    if (dsteps) *dsteps = h->e->total_decode_steps;
    if (cms) *cms = h->e->total_codec_ms;
    if (cframes) *cframes = h->e->total_codec_frames;
    if (reset) { h->e->total_decode_ms = 0; h->e->total_decode_steps = 0; h->e->total_codec_ms = 0; h->e->total_codec_frames = 0; }
    return 0;
    Q3_API_END(h)
}
int q3tts_codec_plane_stats(q3tts_engine* h, int* two_product, int* three_product) {
    Q3_API_BEGIN(h)
    h->e->codec_plane_stats(two_product, three_product);
    return 0;
    Q3_API_END(h)
}
int q3tts_prefill_profile(q3tts_engine* h, int n_slots, int n_rows, int reps, double* ms_per_pass) {
    Q3_API_BEGIN(h)
    if (!ms_per_pass) throw q3::Error("prefill_profile: null output");
    h->e->prefill_profile(n_slots, n_rows, reps, ms_per_pass);
    return 0;
    Q3_API_END(h)
}
int q3tts_stage_profile(q3tts_engine* h, int n_steps, double* out_ms) {
    Q3_API_BEGIN(h)
    if (!out_ms) throw q3::Error("stage_profile: null output");
    h->e->stage_profile(n_steps, out_ms);
    return 0;
    Q3_API_END(h)
}
// ---- batch-first device-pointer entry points ----
#define Q3_DEV_CALL(h, strm, body)                                       \
    Q3_API_BEGIN(h)                                                      \
    hipStream_t caller_ = (strm) ? (hipStream_t)(strm) : (h)->e->stream; \
    (h)->e->stream_join(caller_);                                        \
    body;                                                                \
    (h)->e->stream_fork(caller_);                                        \
    return 0;                                                            \
    Q3_API_END(h)
int q3tts_talker_prefill_dev(q3tts_engine* h, const float* embeds, int batch, int S, const int32_t* lens, float* logits_last, float* last_hidden, void* stream) {
    Q3_DEV_CALL(h, stream, h->e->talker_prefill_dev(embeds, batch, S, lens, logits_last, last_hidden))
}
int q3tts_talker_decode_dev(q3tts_engine* h, const float* embeds, int batch, const uint8_t* active_mask, float* logits, float* last_hidden, void* stream) {
    Q3_DEV_CALL(h, stream, h->e->talker_decode_dev(embeds, batch, active_mask, logits, last_hidden))
}
int q3tts_code_predictor_dev(q3tts_engine* h, const float* last_hidden, const int64_t* code0, int batch, const q3tts_sampling* p, uint64_t seed,
                             uint32_t stream_id0, uint32_t frame, int32_t* sub, void* stream) {
    if (!p) return -1;
    Q3_DEV_CALL(h, stream, h->e->code_predictor_dev(last_hidden, code0, batch, *p, seed, stream_id0, frame, sub))
}
int q3tts_sample_dev(q3tts_engine* h, const float* logits, int batch, int n, const q3tts_sampling* p, const float* u, int suppress, int64_t* ids, void* stream) {
    if (!p) return -1;
    Q3_DEV_CALL(h, stream, h->e->sample_dev(logits, batch, n, *p, u, suppress, ids))
}
int q3tts_sample_hist_dev(q3tts_engine* h, const float* logits, int batch, int n, const q3tts_sampling* p, const float* u, int suppress,
                          const int64_t* history, int hist_ld, const int32_t* hist_len, int64_t* ids, void* stream) {
    if (!p) return -1;
    Q3_DEV_CALL(h, stream, h->e->sample_hist_dev(logits, batch, n, *p, u, suppress, history, hist_ld, hist_len, ids))
}
int q3tts_measure_skip_frames(q3tts_engine* h, int n_frames) {
    Q3_API_BEGIN(h)
    h->e->measure_skip_frames(n_frames);
    return 0;
    Q3_API_END(h)
}
int q3tts_test_group_final_conv(q3tts_engine* h, float* sx_out, float* pcm_out, int64_t cap_floats, int32_t* T, int32_t* C, int32_t* nb) {
    Q3_API_BEGIN(h)
    int t = 0, c = 0, n = 0;
    h->e->codec_debug_group(sx_out, pcm_out, cap_floats, &t, &c, &n);
    if (T) *T = t; if (C) *C = c; if (nb) *nb = n;
    return 0;
    Q3_API_END(h)
}
int64_t q3tts_test_final_conv_partials(q3tts_engine* h, float* out, int64_t cap_floats) {
    if (!h || !h->e) return -1;
    try { return h->e->codec_debug_partials(out, cap_floats); } catch (...) { return -1; }
}
int q3tts_test_poison_workspace(q3tts_engine* h) {
    Q3_API_BEGIN(h)
    h->e->codec_poison();
    h->e->encoder_poison();
    return 0;
    Q3_API_END(h)
}
int q3tts_step_logits_host(q3tts_engine* h, int slot, float* out, int cols) {
    Q3_API_BEGIN(h)
    if (!out) throw q3::Error("step_logits: null output");
    h->e->step_logits(slot, out, cols);
    return 0;
    Q3_API_END(h)
}
int q3tts_decode_step_bytes(q3tts_engine* h, double* wb, double* kvb) {
    Q3_API_BEGIN(h) h->e->step_bytes(wb, kvb); return 0; Q3_API_END(h)
}

} // extern "C"

// ---- weight files -----------------------------------------------------------------------------
namespace {
const char kMagic[8] = { 'Q', '3', 'T', 'W', '0', '0', '0', '1' };
struct File {
    FILE* f;
    explicit File(const char* p, const char* mode) : f(fopen(p, mode)) {}
    ~File() { if (f) fclose(f); }
};
void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) throw q3::Error("weights file truncated"); }
void wr(FILE* f, const void* p, size_t n) { if (fwrite(p, 1, n, f) != n) throw q3::Error("weights file write failed"); }
void read_header(FILE* f, q3tts_config* cfg, uint32_t* n) {
    char magic[8];
    rd(f, magic, 8);
    if (memcmp(magic, kMagic, 8) != 0) throw q3::Error("not a Q3TW0001 weights file");
    uint32_t cfg_bytes = 0;
    rd(f, &cfg_bytes, 4);
    // files written before the speaker-encoder fields existed carry a shorter config: the missing tail reads as zero
    if (cfg_bytes > sizeof(q3tts_config) || cfg_bytes < offsetof(q3tts_config, spk_enc_dim)) throw q3::Error("weights file: config struct size mismatch");
    memset(cfg, 0, sizeof *cfg);
    rd(f, cfg, cfg_bytes);
    if (cfg->cp_hidden == cfg->hidden) cfg->cp_hidden = 0; // one spelling of "same width" (the engine normalises likewise)
    rd(f, n, 4);
}
} // namespace

extern "C" {

int q3tts_read_weights_config(const char* path, q3tts_config* out) {
    try {
        File fl(path, "rb");
        if (!fl.f) throw q3::Error(std::string("cannot open ") + path);
        uint32_t n = 0;
        read_header(fl.f, out, &n);
        return 0;
    } catch (const q3::Error& ex) { g_create_err = ex.msg; return -1; }
}

int q3tts_load_weights_file(q3tts_engine* h, const char* path) {
    Q3_API_BEGIN(h)
    h->e->check_unshared();
    File fl(path, "rb");
    if (!fl.f) throw q3::Error(std::string("cannot open ") + path);
    q3tts_config cfg;
    uint32_t n = 0;
    read_header(fl.f, &cfg, &n);
    if (memcmp(&cfg, &h->e->c, sizeof cfg) != 0) throw q3::Error("weights file was written for a different model config");
    std::vector<float> f32;
    std::vector<uint16_t> b16;
    // every registry tensor exactly once: storage is a bare hipMalloc, so a tensor the file does not carry would be synthesized from
    // uninitialised HBM (the reference refuses to start when a model file is missing, tts_onnx.cpp:91-107)
    std::vector<char> seen(h->e->tensors.size(), 0);
    for (uint32_t t = 0; t < n; ++t) {
        uint16_t nl = 0;
        rd(fl.f, &nl, 2);
        std::string name(nl, '\0');
        rd(fl.f, &name[0], nl);
        uint8_t dtype = 0;
        rd(fl.f, &dtype, 1);
        uint64_t numel = 0;
        rd(fl.f, &numel, 8);
        // the header is untrusted: size the buffers from the registry, not from the file
        const q3::Tensor& want = h->e->T(name);
        char& mark = seen[(size_t)h->e->tindex.at(name)];
        if (mark) throw q3::Error("weights file: tensor '" + name + "' appears twice");
        mark = 1;
        if ((uint64_t)want.numel != numel) throw q3::Error("weights file: tensor '" + name + "' has " + std::to_string(numel) + " elements, expected " + std::to_string(want.numel));
        f32.resize(numel);
        if (dtype == 0) rd(fl.f, f32.data(), numel * 4);
        else if (dtype == 1) {
            b16.resize(numel);
            rd(fl.f, b16.data(), numel * 2);
            for (uint64_t i = 0; i < numel; ++i) f32[i] = q3::bf16_to_f32(b16[i]);
        } else throw q3::Error("weights file: unknown dtype for " + name);
        h->e->set_tensor(name, f32.data(), (int64_t)numel);
    }
    {   // name every missing tensor at once (an importer with a wrong key prefix drops whole components)
        std::string missing;
        size_t n_missing = 0;
        for (size_t i = 0; i < seen.size(); ++i)
            if (!seen[i]) { if (n_missing++ < 24) missing += (missing.empty() ? "" : ", ") + h->e->tensors[i].name; }
        if (n_missing) throw q3::Error("weights file: " + std::to_string(n_missing) + " of " + std::to_string(seen.size()) + " tensors missing: " + missing + (n_missing > 24 ? ", ..." : ""));
    }
    h->e->finalize();
    return 0;
    Q3_API_END(h)
}

int q3tts_save_weights_file(q3tts_engine* h, const char* path) {
    Q3_API_BEGIN(h)
    File fl(path, "wb");
    if (!fl.f) throw q3::Error(std::string("cannot create ") + path);
    wr(fl.f, kMagic, 8);
    const uint32_t cfg_bytes = sizeof(q3tts_config), n = (uint32_t)h->e->tensors.size();
    wr(fl.f, &cfg_bytes, 4);
    wr(fl.f, &h->e->c, sizeof(q3tts_config));
    wr(fl.f, &n, 4);
    std::vector<float> f32;
    std::vector<uint16_t> b16;
    for (const q3::Tensor& t : h->e->tensors) {
        const uint16_t nl = (uint16_t)t.name.size();
        wr(fl.f, &nl, 2);
        wr(fl.f, t.name.data(), nl);
        const uint8_t dtype = t.bf16 ? 1 : 0;
        wr(fl.f, &dtype, 1);
        const uint64_t numel = (uint64_t)t.numel;
        wr(fl.f, &numel, 8);
        f32.resize(numel);
        h->e->get_tensor(t.name, f32.data(), t.numel);
        if (t.bf16) {
            b16.resize(numel);
            for (uint64_t i = 0; i < numel; ++i) b16[i] = q3::f32_to_bf16(f32[i]);
            wr(fl.f, b16.data(), numel * 2);
        } else wr(fl.f, f32.data(), numel * 4);
    }
    return 0;
    Q3_API_END(h)
}

// ---- text front end (host only) ----
struct q3tts_tokenizer {
    q3::BpeTokenizer t;
};

q3tts_tokenizer* q3tts_tokenizer_create(void) {
    try { return new q3tts_tokenizer(); } catch (...) { return nullptr; }
}
void q3tts_tokenizer_destroy(q3tts_tokenizer* t) { delete t; }
int q3tts_tokenizer_load_vocab(q3tts_tokenizer* t, const char* path) {
    if (!t || !path) return -1;
    try { return t->t.load_vocab(path) ? 0 : -1; } catch (...) { return -1; }
}
int q3tts_tokenizer_load_merges(q3tts_tokenizer* t, const char* path) {
    if (!t || !path) return -1;
    try { return t->t.load_merges(path) ? 0 : -1; } catch (...) { return -1; }
}
int q3tts_tokenizer_ready(const q3tts_tokenizer* t) { return t && t->t.ready() ? 1 : 0; }
int64_t q3tts_tokenize(const q3tts_tokenizer* t, const char* text, int64_t len, int32_t* ids, int64_t cap) {
    if (!t || len < 0 || (len > 0 && !text)) return -1;
    try {
        std::vector<int32_t> v;
        t->t.encode(text, (size_t)len, v);
        for (int64_t i = 0; i < (int64_t)v.size() && i < cap && ids; ++i) ids[i] = v[(size_t)i];
        return (int64_t)v.size();
    } catch (...) { return -1; }
}

} // extern "C"
