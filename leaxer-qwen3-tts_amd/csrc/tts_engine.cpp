// tts_engine.cpp — leaxer_qwen::TTSEngine over the C-ABI (include/q3tts.h).
#include "tts_engine.h"

#include <cmath>

#include <algorithm>
#include <climits>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>

#include "../../include/q3tts.h"

namespace leaxer_qwen {

Speaker parse_speaker(const std::string& name) { // reference src/tts_onnx.cpp:54-68: case-insensitive names
    std::string s;
    for (char ch : name) s.push_back((char)std::tolower((unsigned char)ch));
    static const struct { const char* n; Speaker v; } table[] = {
        { "serena", Speaker::Serena }, { "vivian", Speaker::Vivian }, { "uncle_fu", Speaker::Uncle_Fu },
        { "dylan", Speaker::Dylan }, { "eric", Speaker::Eric }, { "ryan", Speaker::Ryan }, { "aiden", Speaker::Aiden },
        { "ono_anna", Speaker::Ono_Anna }, { "sohee", Speaker::Sohee } };
    for (const auto& e : table) if (s == e.n) return e.v;
    return Speaker::None;
}

static int lang_index(Language l) { return l == Language::Auto ? 0 : (int)(language_to_codec_id(l) - config::LANG_ENGLISH) + 1; }

TTSEngine::TTSEngine(const std::string& model_dir, bool audio_encoder) {
    const char* env_b = std::getenv("Q3TTS_MAX_BATCH");
    max_batch_ = env_b ? std::max(1, std::atoi(env_b)) : 1;
    const int device = std::getenv("Q3TTS_DEVICE") ? std::atoi(std::getenv("Q3TTS_DEVICE")) : 0;
    const int max_ctx = config::MAX_NEW_TOKENS + 64;
    max_ctx_ = max_ctx;
    q3tts_config cfg;
    if (model_dir.rfind("synthetic:", 0) == 0 || model_dir.rfind("synthetic-1.7b:", 0) == 0) {   // seeded weights at the 0.6B / 1.7B dims
        const bool big = model_dir[9] == '-';
        q3tts_default_config(big ? "1.7b" : "0.6b", &cfg);
        if (audio_encoder) q3tts_config_enable_audio_encoder(&cfg);
        h_ = q3tts_create(&cfg, device, max_batch_, max_ctx, 0);
        if (!h_) { error_msg_ = q3tts_last_error(nullptr); return; }
        if (q3tts_fill_synthetic(h_, std::strtoull(model_dir.c_str() + (big ? 15 : 10), nullptr, 10)) != 0 || q3tts_finalize(h_) != 0) { error_msg_ = q3tts_last_error(h_); return; }
    } else {
        const std::string path = model_dir + "/model.q3w";
        if (q3tts_read_weights_config(path.c_str(), &cfg) != 0) { error_msg_ = std::string("Failed to load ") + path + ": " + q3tts_last_error(nullptr); return; }
        h_ = q3tts_create(&cfg, device, max_batch_, max_ctx, 0);
        if (!h_) { error_msg_ = q3tts_last_error(nullptr); return; }
        if (q3tts_load_weights_file(h_, path.c_str()) != 0) { error_msg_ = q3tts_last_error(h_); return; }
    }
    spk_dim_ = cfg.spk_enc_dim;
    cfg_hidden_ = cfg.hidden;
    n_groups_ = cfg.n_groups;
    model_dir_ = model_dir;
    if (!load_tokenizer(model_dir)) return;
    ready_ = true;
}

std::unique_ptr<TTSEngine> TTSEngine::share_weights(const TTSEngine& donor) {
    if (!donor.ready_ || !donor.h_) { std::cerr << "[TTSEngine] share_weights: the donor is not ready" << std::endl; return nullptr; }
    std::unique_ptr<TTSEngine> t(new TTSEngine());
    t->max_batch_ = donor.max_batch_; t->max_ctx_ = donor.max_ctx_;
    t->h_ = q3tts_create_sharing(donor.h_, donor.max_batch_, donor.max_ctx_, 0, 0);
    if (!t->h_) { std::cerr << "[TTSEngine] share_weights: " << q3tts_last_error(nullptr) << std::endl; return nullptr; }
    t->spk_dim_ = donor.spk_dim_; t->cfg_hidden_ = donor.cfg_hidden_; t->n_groups_ = donor.n_groups_;
    t->model_dir_ = donor.model_dir_;
    if (!t->load_tokenizer(t->model_dir_)) { std::cerr << "[TTSEngine] share_weights: " << t->error_msg_ << std::endl; return nullptr; }
    t->ready_ = true;
    return t;
}

bool TTSEngine::load_tokenizer(const std::string& model_dir) {
    // tokenizer files: where the reference looks (tts_onnx.cpp:110-121: <parent of model_dir>/models/
    // Qwen3-TTS-12Hz-0.6B-Base/{vocab.json,merges.txt}), then model_dir itself.  Present but unreadable is
    // an error, absent is a warning and text synthesis stays unavailable — as in the reference.
    namespace fs = std::filesystem;
    tok_ = q3tts_tokenizer_create();
    const fs::path ref_base = fs::path(model_dir).parent_path() / "models" / "Qwen3-TTS-12Hz-0.6B-Base";
    fs::path base = ref_base;
    std::error_code ec;
    if (!(fs::exists(base / "vocab.json", ec) && fs::exists(base / "merges.txt", ec)) && model_dir.rfind("synthetic:", 0) != 0)
        base = fs::path(model_dir);
    if (fs::exists(base / "vocab.json", ec) && fs::exists(base / "merges.txt", ec)) {
        if (!tok_ || q3tts_tokenizer_load_vocab(tok_, (base / "vocab.json").string().c_str()) != 0 ||
            q3tts_tokenizer_load_merges(tok_, (base / "merges.txt").string().c_str()) != 0) {
            error_msg_ = "Failed to load tokenizer";
            return false;
        }
    } else {
        std::cerr << "[TTSEngine] Warning: Tokenizer not found at " << ref_base << std::endl;
    }
    return true;
}

TTSEngine::~TTSEngine() {
    if (tok_) q3tts_tokenizer_destroy(tok_);
    if (h_) q3tts_destroy(h_);
}

bool TTSEngine::wrap_text(const std::string& text, std::vector<int64_t>& ids) const {
    // reference tts_onnx.cpp:243-259: [IM_START, ASSISTANT, TTS_BOS, ...text..., TTS_EOS, IM_END]
    if (!q3tts_tokenizer_ready(tok_)) {
        std::cerr << "[TTSEngine] Tokenizer not ready" << std::endl;
        return false;
    }
    const int64_t n = q3tts_tokenize(tok_, text.data(), (int64_t)text.size(), nullptr, 0);
    if (n < 0) return false;
    std::vector<int32_t> t((size_t)n);
    q3tts_tokenize(tok_, text.data(), (int64_t)text.size(), t.data(), n);
    ids = { config::IM_START, config::ASSISTANT, config::TTS_BOS };
    ids.insert(ids.end(), t.begin(), t.end());
    ids.push_back(config::TTS_EOS);
    ids.push_back(config::IM_END);
    return true;
}

std::vector<int32_t> TTSEngine::tokenize(const std::string& text) const {
    std::vector<int32_t> t;
    const int64_t n = q3tts_tokenize(tok_, text.data(), (int64_t)text.size(), nullptr, 0);
    if (n <= 0) return t;
    t.resize((size_t)n);
    q3tts_tokenize(tok_, text.data(), (int64_t)text.size(), t.data(), n);
    return t;
}

std::vector<float> TTSEngine::synthesize(const std::string& text, Language lang, const SamplingParams& params) {
    if (!ready_) return {};
    std::vector<int64_t> ids;
    if (!wrap_text(text, ids)) return {};
    return synthesize_tokens(ids, lang, params);
}

std::vector<std::vector<float>> TTSEngine::synthesize_batch(const std::vector<std::string>& texts, Language lang,
                                                            const SamplingParams& params) {
    std::vector<std::vector<int64_t>> ids(texts.size());
    if (!ready_) return std::vector<std::vector<float>>(texts.size());
    for (size_t i = 0; i < texts.size(); ++i)
        if (!wrap_text(texts[i], ids[i])) return std::vector<std::vector<float>>(texts.size());
    return synthesize_tokens_batch(ids, lang, params);
}

bool TTSEngine::has_speaker_encoder() const { return h_ && q3tts_has_speaker_encoder(h_); }

std::vector<float> TTSEngine::synthesize_clone(const std::string& text, const std::string& ref_audio_path, Language lang,
                                               const SamplingParams& params) { // reference tts_onnx.cpp:264-318
    if (!ready_) return {};
    if (!has_speaker_encoder()) {
        std::cerr << "[TTSEngine] Speaker encoder not available" << std::endl;
        return {};
    }
    const std::vector<float> spk = extract_speaker_embedding(ref_audio_path);
    if (spk.empty()) {
        std::cerr << "[TTSEngine] Failed to extract speaker embedding" << std::endl;
        return {};
    }
    std::vector<int64_t> ids;
    if (!wrap_text(text, ids)) return {};
    return synthesize_tokens_clone(ids, spk, lang, params);
}

std::vector<float> TTSEngine::synthesize_tokens_clone(const std::vector<int64_t>& token_ids, const std::vector<float>& speaker_embed,
                                                      Language lang, const SamplingParams& params) {
    if (!ready_) return {};
    if (!speaker_embed.empty() && (int)speaker_embed.size() != cfg_hidden_) {   // the row is spliced into the prompt as one talker-width embedding
        std::cerr << "[TTSEngine] Synthesis error: speaker embedding has " << speaker_embed.size() << " values, the model needs " << cfg_hidden_ << std::endl;
        return {};
    }
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    const int32_t offs[2] = { 0, (int32_t)token_ids.size() };
    const int64_t cap = (int64_t)params.max_new_tokens * 1920 + 1920;
    std::vector<float> pcm((size_t)cap);
    float* ptr = pcm.data();
    const float* spk = speaker_embed.empty() ? nullptr : speaker_embed.data();
    int64_t len = 0;
    int32_t frames = 0;
    if (q3tts_synthesize_clone_batch_host(h_, 1, token_ids.data(), offs, lang_index(lang), &spk, &sp, seed_, 0, &ptr, cap, &len, &frames, nullptr) != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    pcm.resize((size_t)std::min<int64_t>(len, cap));
    (void)apply_speed(pcm);
    return pcm;
}

std::vector<float> TTSEngine::synthesize_instruct(const std::string& text, const std::string& instruct, Language lang, const SamplingParams& params) {
    return synthesize_instruct(text, instruct, std::vector<float>(), lang, params);
}

std::vector<float> TTSEngine::synthesize_instruct(const std::string& text, const std::string& instruct, const std::vector<float>& speaker_embed,
                                                  Language lang, const SamplingParams& params) {
    if (!ready_) return {};
    std::vector<int64_t> ids;
    if (!wrap_text(text, ids)) return {};
    return synthesize_tokens_instruct(ids, instruct.empty() ? std::vector<int32_t>() : tokenize(instruct), speaker_embed, lang, params);
}

std::vector<float> TTSEngine::synthesize_tokens_instruct(const std::vector<int64_t>& token_ids, const std::vector<int32_t>& instruct_text_ids,
                                                         const std::vector<float>& speaker_embed, Language lang, const SamplingParams& params) {
    if (!ready_) return {};
    if (instruct_text_ids.empty()) return synthesize_tokens_clone(token_ids, speaker_embed, lang, params);
    if (!speaker_embed.empty() && (int)speaker_embed.size() != cfg_hidden_) {
        std::cerr << "[TTSEngine] Synthesis error: speaker embedding has " << speaker_embed.size() << " values, the model needs " << cfg_hidden_ << std::endl;
        return {};
    }
    std::vector<int64_t> framed((size_t)instruct_text_ids.size() + 5);
    if (q3tts_frame_instruct_ids(instruct_text_ids.data(), (int64_t)instruct_text_ids.size(), framed.data(), (int64_t)framed.size()) != (int64_t)framed.size()) return {};
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    // prompt rows: the instruction + at most 16; the frames that still fit the context behind them
    sp.max_new_tokens = std::min(sp.max_new_tokens, max_ctx_ - (int)framed.size() - 16);
    if (sp.max_new_tokens < 1) {
        std::cerr << "[TTSEngine] Synthesis error: the instruction does not fit the engine's context" << std::endl;
        return {};
    }
    const int32_t offs[2] = { 0, (int32_t)token_ids.size() }, ioffs[2] = { 0, (int32_t)framed.size() };
    const int64_t cap = (int64_t)sp.max_new_tokens * 1920 + 1920;
    std::vector<float> pcm((size_t)cap);
    float* ptr = pcm.data();
    const float* spk = speaker_embed.empty() ? nullptr : speaker_embed.data();
    int64_t len = 0;
    int32_t frames = 0;
    if (q3tts_synthesize_instruct_host(h_, 1, token_ids.data(), offs, lang_index(lang), &spk, &sp, nullptr, seed_, 0, &ptr, cap, &len, &frames, nullptr,
                                       0, nullptr, nullptr, framed.data(), ioffs) != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    pcm.resize((size_t)std::min<int64_t>(len, cap));
    (void)apply_speed(pcm);
    return pcm;
}

std::vector<float> TTSEngine::synthesize_tokens_continue(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes, Language lang,
                                                         const SamplingParams& params, std::vector<int64_t>* all_codes) {
    if (all_codes) all_codes->clear();
    if (!ready_) return {};
    const size_t G = (size_t)n_groups_;
    if (prefix_codes.size() % G != 0) {
        std::cerr << "[TTSEngine] Synthesis error: prefix codes are not whole frames of " << G << " ids" << std::endl;
        return {};
    }
    const int F0 = (int)(prefix_codes.size() / G);
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    sp.max_new_tokens = std::min(sp.max_new_tokens, max_ctx_ - F0 - 16);   // prompt rows: at most 16
    if (sp.max_new_tokens < 1) {
        std::cerr << "[TTSEngine] Synthesis error: the prefix does not fit the engine's context" << std::endl;
        return {};
    }
    const int32_t offs[2] = { 0, (int32_t)token_ids.size() }, poffs[2] = { 0, F0 };
    const int64_t cap = (int64_t)sp.max_new_tokens * 1920 + 1920;
    std::vector<float> pcm((size_t)cap);
    std::vector<int64_t> codes((size_t)(F0 + sp.max_new_tokens) * G);
    float* ptr = pcm.data();
    int64_t len = 0;
    int32_t frames = 0;
    if (q3tts_synthesize_continue_host(h_, 1, token_ids.data(), offs, lang_index(lang), nullptr, &sp, nullptr, seed_, 0, &ptr, cap, &len, &frames, codes.data(),
                                       F0 > 0 ? prefix_codes.data() : nullptr, F0 > 0 ? poffs : nullptr) != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    if (all_codes) all_codes->assign(codes.begin(), codes.begin() + (size_t)frames * G);
    pcm.resize((size_t)std::min<int64_t>(len, cap));
    (void)apply_speed(pcm);
    return pcm;
}

int TTSEngine::synthesize_tokens_continue_streaming(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes, Language lang,
                                                    const SamplingParams& params, int chunk_frames,
                                                    const std::function<bool(const float*, size_t, bool)>& on_audio, std::vector<int64_t>* all_codes) {
    if (all_codes) all_codes->clear();
    if (!ready_ || chunk_frames < 1 || !on_audio) return -1;
    const size_t G = (size_t)n_groups_;
    if (prefix_codes.size() % G != 0) {
        std::cerr << "[TTSEngine] Synthesis error: prefix codes are not whole frames of " << G << " ids" << std::endl;
        return -1;
    }
    const int F0 = (int)(prefix_codes.size() / G);
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    sp.max_new_tokens = std::min(sp.max_new_tokens, max_ctx_ - F0 - 16);   // prompt rows: at most 16
    if (sp.max_new_tokens < 1) {
        std::cerr << "[TTSEngine] Synthesis error: the prefix does not fit the engine's context" << std::endl;
        return -1;
    }
    const int32_t offs[2] = { 0, (int32_t)token_ids.size() }, poffs[2] = { 0, F0 };
    std::vector<int64_t> codes((size_t)(F0 + sp.max_new_tokens) * G);
    int32_t frames = 0;
    struct Ctx { const std::function<bool(const float*, size_t, bool)>* f; } ctx{ &on_audio };
    const q3tts_audio_cb cb = [](void* user, int, int, int, const float* pcm, int64_t n, int finished) -> int {
        return (*static_cast<Ctx*>(user)->f)(pcm, (size_t)n, finished != 0) ? 1 : 0;
    };
    if (sink_on()) sink_fn_ = [&](int, const void* pcm, int64_t n, int finished) { return on_audio((const float*)pcm, (size_t)n, finished != 0) ? 1 : 0; };
    const int rc = q3tts_synthesize_continue_stream_host(h_, 1, token_ids.data(), offs, lang_index(lang), nullptr, &sp, nullptr, seed_, 0, nullptr, 0, nullptr, &frames,
                                                         codes.data(), F0 > 0 ? prefix_codes.data() : nullptr, F0 > 0 ? poffs : nullptr, chunk_frames, cb, &ctx);
    sink_fn_ = nullptr;
    if (rc != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return -1;
    }
    if (all_codes) all_codes->assign(codes.begin(), codes.begin() + (size_t)frames * G);
    return frames;
}

std::vector<float> TTSEngine::synthesize_speaker(const std::string& text, Speaker, Language lang, const SamplingParams& params) {
    std::cerr << "[TTSEngine] Preset speakers require CustomVoice model (not yet supported)" << std::endl; // :327
    return synthesize(text, lang, params);
}

bool TTSEngine::set_output_format(int sample_rate, bool pcm16) { return set_output_encoding(sample_rate, pcm16 ? Q3TTS_PCM_S16 : Q3TTS_PCM_F32); }

bool TTSEngine::set_output_encoding(int sample_rate, int format) {
    if (!ready_) return false;
    if (sample_rate == config::SAMPLE_RATE && format == Q3TTS_PCM_F32) {
        (void)q3tts_engine_set_sink(h_, nullptr);
        out_rate_ = sample_rate; out_format_ = Q3TTS_PCM_F32;
        return true;
    }
    q3tts_sink sk;
    sk.sample_rate = sample_rate; sk.format = format; sk.user = this;
    sk.cb = [](void* user, int utt, int, int, const void* pcm, int64_t n, int finished) -> int {
        TTSEngine* self = static_cast<TTSEngine*>(user);
        return self->sink_fn_ ? self->sink_fn_(utt, pcm, n, finished) : 0;
    };
    if (q3tts_engine_set_sink(h_, &sk) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Output format: " << error_msg_ << std::endl;
        return false;
    }
    out_rate_ = sample_rate; out_format_ = format;
    return true;
}

bool TTSEngine::convert_output(const std::vector<float>& pcm24, std::vector<float>* f32, std::vector<int16_t>* s16) { return convert_output(pcm24, f32, s16, nullptr); }

bool TTSEngine::convert_output(const std::vector<float>& pcm24, std::vector<float>* f32, std::vector<int16_t>* s16, std::vector<uint8_t>* g711) {
    if (f32) f32->clear();
    if (s16) s16->clear();
    if (g711) g711->clear();
    const bool as_f32 = out_format_ == Q3TTS_PCM_F32, as_s16 = out_format_ == Q3TTS_PCM_S16;
    if (!ready_ || (as_f32 ? !f32 : as_s16 ? !s16 : !g711)) return false;
    if (!sink_on()) { *f32 = pcm24; return true; }
    int id = -1;
    auto fail = [&]() {
        std::cerr << "[TTSEngine] Output conversion error: " << q3tts_last_error(h_) << std::endl;
        if (id >= 0) (void)q3tts_pcm_sink_end(h_, id);
        if (f32) f32->clear();
        if (s16) s16->clear();
        if (g711) g711->clear();
        return false;
    };
    if (q3tts_pcm_sink_begin(h_, out_rate_, out_format_, &id) != 0) return fail();
    const size_t step = 1440000;   // the most one push takes
    size_t done = 0;
    do {
        const size_t m = std::min(step, pcm24.size() - done);
        const int64_t n_in = (int64_t)m;
        const uint8_t fin = done + m == pcm24.size() ? 1 : 0;
        const int64_t before = q3tts_sink_emitted(out_rate_, (int64_t)done, 0), after = q3tts_sink_emitted(out_rate_, (int64_t)(done + m), fin);
        if (before < 0 || after < before) return fail();
        const size_t have = as_f32 ? f32->size() : as_s16 ? s16->size() : g711->size(), want = have + (size_t)(after - before);
        if (as_f32) f32->resize(want); else if (as_s16) s16->resize(want); else g711->resize(want);
        const float* in = pcm24.data() + done;
        void* out = as_f32 ? (void*)(f32->data() + have) : as_s16 ? (void*)(s16->data() + have) : (void*)(g711->data() + have);
        int64_t len = 0;
        if (q3tts_pcm_sink_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &out, after - before, &len) != 0 || len != after - before) return fail();
        done += m;
    } while (done < pcm24.size());
    (void)q3tts_pcm_sink_end(h_, id);
    return true;
}

bool TTSEngine::set_speed(float speed) {
    if (!ready_) return false;
    const long S = std::lround(1000.0 * (double)speed);
    if (!(speed == speed) || S < 500 || S > 2000) {
        error_msg_ = "speed " + std::to_string(speed) + " is outside 0.5 .. 2.0";
        std::cerr << "[TTSEngine] Speed: " << error_msg_ << std::endl;
        return false;
    }
    if (q3tts_engine_set_speed(h_, (int32_t)S) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Speed: " << error_msg_ << std::endl;
        return false;
    }
    speed_ = (int)S;
    return true;
}

bool TTSEngine::stretch_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out) {
    const int64_t n_in = (int64_t)n;
    const uint8_t fin = finish ? 1 : 0;
    const int64_t before = q3tts_speed_emitted(speed_, (int64_t)received_before, 0), after = q3tts_speed_emitted(speed_, (int64_t)(received_before + n), fin);
    if (before < 0 || after < before) return false;
    const size_t have = out.size();
    out.resize(have + (size_t)(after - before));
    float* dst = out.data() + have;
    int64_t len = 0;
    return q3tts_speed_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &dst, after - before, &len, nullptr, nullptr) == 0 && len == after - before;
}

bool TTSEngine::set_pitch(float semitones) {
    if (!ready_) return false;
    const int32_t r = semitones == semitones ? q3tts_pitch_ratio(100.0 * (double)semitones) : -1;
    if (r < 0) {
        error_msg_ = "pitch " + std::to_string(semitones) + " semitones is outside -12 .. +12";
        std::cerr << "[TTSEngine] Pitch: " << error_msg_ << std::endl;
        return false;
    }
    if (q3tts_engine_set_pitch(h_, r) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Pitch: " << error_msg_ << std::endl;
        return false;
    }
    pitch_ = (int)r;
    return true;
}

bool TTSEngine::pitch_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out) {
    const int64_t n_in = (int64_t)n;
    const uint8_t fin = finish ? 1 : 0;
    const int64_t before = q3tts_pitch_emitted((int64_t)received_before, 0), after = q3tts_pitch_emitted((int64_t)(received_before + n), fin);
    if (before < 0 || after < before) return false;
    const size_t have = out.size();
    out.resize(have + (size_t)(after - before));
    float* dst = out.data() + have;
    int64_t len = 0;
    return q3tts_pitch_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &dst, after - before, &len) == 0 && len == after - before;
}

bool TTSEngine::apply_pitch(std::vector<float>& pcm24) {
    if (!ready_) return false;
    if (pitch_ == 1000 || pcm24.empty()) return true;
    int id = -1;
    std::vector<float> out;
    bool ok = q3tts_pitch_begin(h_, pitch_, &id) == 0;
    const size_t step = 1440000;   // the most one push takes
    for (size_t done = 0; ok && done < pcm24.size(); done += step) {
        const size_t m = std::min(step, pcm24.size() - done);
        ok = pitch_push(id, pcm24.data() + done, m, done + m == pcm24.size(), done, out);
    }
    if (!ok) std::cerr << "[TTSEngine] Pitch error: " << q3tts_last_error(h_) << std::endl;
    if (id >= 0) (void)q3tts_pitch_end(h_, id);
    if (ok) pcm24.swap(out); else pcm24.clear();
    return ok;
}

bool TTSEngine::set_tone(const char* spec) {
    if (!ready_) return false;
    q3tts_tone_section s[Q3TTS_TONE_MAX_SECTIONS];
    int32_t n = 0;
    if (q3tts_tone_parse(spec, s, &n) != 0) {
        error_msg_ = q3tts_tone_last_error();
        std::cerr << "[TTSEngine] Tone: " << error_msg_ << std::endl;
        return false;
    }
    if (q3tts_engine_set_tone(h_, n, s) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Tone: " << error_msg_ << std::endl;
        return false;
    }
    tone_n_ = n;
    tone_spec_ = spec;
    return true;
}

int TTSEngine::tone_begin(int* id) {
    q3tts_tone_section s[Q3TTS_TONE_MAX_SECTIONS];
    int32_t n = 0;
    if (q3tts_tone_parse(tone_spec_.c_str(), s, &n) != 0) return -1;   // set_tone accepted this spec
    return q3tts_tone_begin(h_, n, s, id);
}

void TTSEngine::clear_tone() {
    if (ready_) (void)q3tts_engine_set_tone(h_, 0, nullptr);
    tone_n_ = 0;
    tone_spec_.clear();
}

bool TTSEngine::tone_push(int id, const float* in, size_t n, bool finish, std::vector<float>& out) {   // the stage emits what it receives
    const int64_t n_in = (int64_t)n;
    const uint8_t fin = finish ? 1 : 0;
    const size_t have = out.size();
    out.resize(have + n);
    float* dst = out.data() + have;
    int64_t len = 0;
    return q3tts_tone_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &dst, n_in, &len) == 0 && len == n_in;
}

bool TTSEngine::apply_tone(std::vector<float>& pcm24) {
    if (!ready_) return false;
    if (tone_n_ == 0 || pcm24.empty()) return true;
    int id = -1;
    std::vector<float> out;
    bool ok = tone_begin(&id) == 0;
    const size_t step = 1440000;   // the most one push takes
    for (size_t done = 0; ok && done < pcm24.size(); done += step) {
        const size_t m = std::min(step, pcm24.size() - done);
        ok = tone_push(id, pcm24.data() + done, m, done + m == pcm24.size(), out);
    }
    if (!ok) std::cerr << "[TTSEngine] Tone error: " << q3tts_last_error(h_) << std::endl;
    if (id >= 0) (void)q3tts_tone_end(h_, id);
    if (ok) pcm24.swap(out); else pcm24.clear();
    return ok;
}

bool TTSEngine::set_loudness(float lufs, float range_db) {
    if (!ready_) return false;
    const long T = std::lround(10.0 * (double)lufs), R = std::lround(10.0 * (double)range_db);
    if (!(lufs == lufs) || T < -400 || T > -50) {
        error_msg_ = "loudness " + std::to_string(lufs) + " LUFS is outside -40 .. -5";
        std::cerr << "[TTSEngine] Loudness: " << error_msg_ << std::endl;
        return false;
    }
    if (!(range_db == range_db) || R < 0 || R > 400) {
        error_msg_ = "loudness range " + std::to_string(range_db) + " dB is outside 0 .. 40";
        std::cerr << "[TTSEngine] Loudness: " << error_msg_ << std::endl;
        return false;
    }
    if (q3tts_engine_set_loudness(h_, 1, (int32_t)T, (int32_t)R, 0) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Loudness: " << error_msg_ << std::endl;
        return false;
    }
    loud_ = true; loud_target_ = (int)T; loud_range_ = (int)R;
    return true;
}

void TTSEngine::clear_loudness() {
    if (ready_) (void)q3tts_engine_set_loudness(h_, 0, 0, 0, 0);
    loud_ = false;
}

bool TTSEngine::loudness_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out) {
    const int64_t n_in = (int64_t)n;
    const uint8_t fin = finish ? 1 : 0;
    const int64_t before = q3tts_loudness_emitted(loud_target_, (int64_t)received_before, 0), after = q3tts_loudness_emitted(loud_target_, (int64_t)(received_before + n), fin);
    if (before < 0 || after < before) return false;
    const size_t have = out.size();
    out.resize(have + (size_t)(after - before));
    float* dst = out.data() + have;
    int64_t len = 0;
    return q3tts_loudness_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &dst, after - before, &len, nullptr, nullptr, nullptr) == 0 && len == after - before;
}

bool TTSEngine::apply_loudness(std::vector<float>& pcm24) {
    if (!ready_) return false;
    if (!loud_ || pcm24.empty()) return true;
    int id = -1;
    std::vector<float> out;
    bool ok = q3tts_loudness_begin(h_, loud_target_, loud_range_, 0, &id) == 0;
    const size_t step = 1440000;   // the most one push takes
    for (size_t done = 0; ok && done < pcm24.size(); done += step) {
        const size_t m = std::min(step, pcm24.size() - done);
        ok = loudness_push(id, pcm24.data() + done, m, done + m == pcm24.size(), done, out);
    }
    if (!ok) std::cerr << "[TTSEngine] Loudness error: " << q3tts_last_error(h_) << std::endl;
    if (id >= 0) (void)q3tts_loudness_end(h_, id);
    if (ok) pcm24.swap(out); else pcm24.clear();
    return ok;
}

bool TTSEngine::set_level(float gain_db, float ceiling) {
    if (!ready_) return false;
    const long G = std::lround(10.0 * (double)gain_db), T = std::lround(1000.0 * (double)ceiling);
    if (!(gain_db == gain_db) || G < -600 || G > 400) {
        error_msg_ = "gain " + std::to_string(gain_db) + " dB is outside -60 .. +40";
        std::cerr << "[TTSEngine] Level: " << error_msg_ << std::endl;
        return false;
    }
    if (!(ceiling == ceiling) || T < 0 || T > 1000 || (ceiling > 0.0f && T == 0)) {
        error_msg_ = "ceiling " + std::to_string(ceiling) + " is outside 0.001 .. 1.0 (0: no limiter)";
        std::cerr << "[TTSEngine] Level: " << error_msg_ << std::endl;
        return false;
    }
    if (q3tts_engine_set_level(h_, (int32_t)G, (int32_t)T) != 0) {
        error_msg_ = q3tts_last_error(h_);
        std::cerr << "[TTSEngine] Level: " << error_msg_ << std::endl;
        return false;
    }
    gain_cb_ = (int)G; ceiling_ = (int)T;
    return true;
}

bool TTSEngine::level_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out) {
    const int64_t n_in = (int64_t)n;
    const uint8_t fin = finish ? 1 : 0;
    const int64_t before = q3tts_level_emitted(gain_cb_, ceiling_, (int64_t)received_before, 0), after = q3tts_level_emitted(gain_cb_, ceiling_, (int64_t)(received_before + n), fin);
    if (before < 0 || after < before) return false;
    const size_t have = out.size();
    out.resize(have + (size_t)(after - before));
    float* dst = out.data() + have;
    int64_t len = 0;
    return q3tts_level_push_batch_host(h_, 1, &id, &in, &n_in, &fin, &dst, after - before, &len) == 0 && len == after - before;
}

bool TTSEngine::apply_level(std::vector<float>& pcm24) {
    if (!ready_) return false;
    if ((gain_cb_ == 0 && ceiling_ == 0) || pcm24.empty()) return true;
    int id = -1;
    std::vector<float> out;
    bool ok = q3tts_level_begin(h_, gain_cb_, ceiling_, &id) == 0;
    const size_t step = 1440000;   // the most one push takes
    for (size_t done = 0; ok && done < pcm24.size(); done += step) {
        const size_t m = std::min(step, pcm24.size() - done);
        ok = level_push(id, pcm24.data() + done, m, done + m == pcm24.size(), done, out);
    }
    if (!ok) std::cerr << "[TTSEngine] Level error: " << q3tts_last_error(h_) << std::endl;
    if (id >= 0) (void)q3tts_level_end(h_, id);
    if (ok) pcm24.swap(out); else pcm24.clear();
    return ok;
}

// the whole clip through the pitch stage, the stretcher, the tone stage, the loudness stage and then the level stage (each only when set): every
// one-shot method ends here
bool TTSEngine::apply_speed(std::vector<float>& pcm24) {
    if (!ready_) return false;
    if (pcm24.empty()) return true;
    if (!apply_pitch(pcm24)) return false;
    if (speed_ == 1000) return apply_tone(pcm24) && apply_loudness(pcm24) && apply_level(pcm24);
    int id = -1;
    std::vector<float> out;
    bool ok = q3tts_speed_begin(h_, speed_, &id) == 0;
    const size_t step = 1440000;   // the most one push takes
    for (size_t done = 0; ok && done < pcm24.size(); done += step) {
        const size_t m = std::min(step, pcm24.size() - done);
        ok = stretch_push(id, pcm24.data() + done, m, done + m == pcm24.size(), done, out);
    }
    if (!ok) std::cerr << "[TTSEngine] Speed error: " << q3tts_last_error(h_) << std::endl;
    if (id >= 0) (void)q3tts_speed_end(h_, id);
    if (ok) pcm24.swap(out); else pcm24.clear();
    return ok && apply_tone(pcm24) && apply_loudness(pcm24) && apply_level(pcm24);
}

bool TTSEngine::has_audio_encoder() const { return h_ && q3tts_has_audio_encoder(h_) != 0; }

std::vector<int64_t> TTSEngine::encode_audio(const std::vector<float>& pcm, int sample_rate) {
    if (!ready_) return {};
    if (!has_audio_encoder()) { std::cerr << "[TTSEngine] model has no audio encoder" << std::endl; return {}; }
    if (pcm.empty() || sample_rate < 1) { std::cerr << "[TTSEngine] encode_audio: empty clip or bad sample rate" << std::endl; return {}; }
    const int64_t n24 = (int64_t)((double)pcm.size() * 24000.0 / sample_rate) + 1;
    const int64_t cap64 = q3tts_audio_encode_len(h_, n24);
    if (cap64 < 1 || cap64 > INT32_MAX) { std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; return {}; }
    std::vector<int64_t> codes((size_t)cap64 * (size_t)n_groups_);
    const float* clip = pcm.data();
    const int64_t n = (int64_t)pcm.size();
    const int32_t rate = sample_rate, cap = (int32_t)cap64;
    int64_t* out = codes.data();
    int32_t frames = 0;
    if (q3tts_audio_encode_batch_host(h_, 1, &clip, &n, &rate, &out, &cap, &frames) != 0) {
        std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    codes.resize((size_t)frames * (size_t)n_groups_);
    return codes;
}

int TTSEngine::audio_stream_begin(int64_t max_samples) { return audio_stream_begin(max_samples, 24000, false); }

int TTSEngine::audio_stream_begin(int64_t max_samples, int sample_rate, bool pcm16) {
    if (!ready_) return -1;
    int id = -1;
    if (q3tts_audio_stream_begin_rate(h_, sample_rate, pcm16 ? Q3TTS_PCM_S16 : Q3TTS_PCM_F32, max_samples, &id) != 0) { std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; return -1; }
    return id;
}

int TTSEngine::audio_stream_begin_encoded(int64_t max_samples, int sample_rate, int format) {
    if (!ready_) return -1;
    int id = -1;
    if (q3tts_audio_stream_begin_rate(h_, sample_rate, format, max_samples, &id) != 0) { std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; return -1; }
    return id;
}

std::vector<int64_t> TTSEngine::audio_stream_push(int id, const float* pcm, size_t n, bool finish, bool* ok) {
    return audio_stream_push_any(id, pcm, n, finish, ok, 0);
}

std::vector<int64_t> TTSEngine::audio_stream_push(int id, const int16_t* pcm, size_t n, bool finish, bool* ok) {
    return audio_stream_push_any(id, pcm, n, finish, ok, 1);
}

std::vector<int64_t> TTSEngine::audio_stream_push(int id, const uint8_t* pcm, size_t n, bool finish, bool* ok) {
    return audio_stream_push_any(id, pcm, n, finish, ok, 2);
}

std::vector<int64_t> TTSEngine::audio_stream_push_any(int id, const void* pcm, size_t n, bool finish, bool* ok, int kind) {
    if (ok) *ok = false;
    if (!ready_) return {};
    const bool pcm16 = kind != 0;   // below: anything but float goes through the entry that reads the stream's own format
    if (kind != 0) {   // int16 samples and G.711 bytes go to a stream begun for them only: the engine reads them in the stream's format
        int fmt = Q3TTS_PCM_F32;
        if (q3tts_audio_stream_format(h_, id, nullptr, &fmt) != 0) { std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; return {}; }
        const bool fits = kind == 1 ? fmt == Q3TTS_PCM_S16 : (fmt == Q3TTS_PCM_MULAW || fmt == Q3TTS_PCM_ALAW);
        if (!fits) { std::cerr << "[TTSEngine] audio stream " << id << " takes " << (fmt == Q3TTS_PCM_F32 ? "float samples" : fmt == Q3TTS_PCM_S16 ? "int16 samples" : "G.711 bytes") << ", not " << (kind == 1 ? "int16" : "G.711 bytes") << std::endl; return {}; }
    }
    const int frames = q3tts_audio_stream_push_len(h_, id, (int64_t)n, finish ? 1 : 0);
    if (frames < 0) { std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; return {}; }
    std::vector<int64_t> codes((size_t)std::max(frames, 1) * (size_t)n_groups_);
    int32_t got = 0;
    // the float entry refuses an int16 stream by name; the other one reads the samples in the stream's own format, so it gets int16 only
    const int rc = pcm16 ? q3tts_audio_stream_push_any_host(h_, id, pcm, (int64_t)n, finish ? 1 : 0, codes.data(), std::max(frames, 1), &got)
                         : q3tts_audio_stream_push_host(h_, id, (const float*)pcm, (int64_t)n, finish ? 1 : 0, codes.data(), std::max(frames, 1), &got);
    if (rc != 0) {
        std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    codes.resize((size_t)got * (size_t)n_groups_);
    if (ok) *ok = true;
    return codes;
}

void TTSEngine::audio_stream_end(int id) {
    if (ready_ && q3tts_audio_stream_end(h_, id) != 0) std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl;
}

static bool read_wav_file(const std::string& path, std::vector<float>& pcm, int32_t& rate) {
    int64_t n = 0;
    if (q3tts_read_wav_host(path.c_str(), nullptr, 0, &n, &rate) != 0 || n < 1) { std::cerr << "[TTSEngine] Failed to read audio: " << path << std::endl; return false; }
    pcm.resize((size_t)n);
    if (q3tts_read_wav_host(path.c_str(), pcm.data(), n, &n, &rate) != 0) { std::cerr << "[TTSEngine] Failed to read audio: " << path << std::endl; return false; }
    return true;
}

std::vector<int64_t> TTSEngine::encode_audio(const std::string& wav_path) {
    std::vector<float> pcm;
    int32_t rate = 0;
    if (!read_wav_file(wav_path, pcm, rate)) return {};
    return encode_audio(pcm, rate);
}

std::vector<float> TTSEngine::synthesize_clone_icl(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& ref_text_ids,
                                                   const std::string& ref_wav_path, Language lang, const SamplingParams& params,
                                                   std::vector<int64_t>* all_codes) {
    if (all_codes) all_codes->clear();
    std::vector<float> pcm;
    int32_t rate = 0;
    if (!read_wav_file(ref_wav_path, pcm, rate)) return {};
    return synthesize_clone_icl(token_ids, ref_text_ids, pcm, rate, lang, params, all_codes);
}

std::vector<float> TTSEngine::synthesize_clone_icl(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& ref_text_ids,
                                                   const std::vector<float>& ref_pcm, int ref_rate, Language lang, const SamplingParams& params,
                                                   std::vector<int64_t>* all_codes) {
    if (all_codes) all_codes->clear();
    if (!ready_ || token_ids.size() < 3) return {};
    const std::vector<int64_t> ref_codes = encode_audio(ref_pcm, ref_rate);
    if (ref_codes.empty()) return {};
    std::vector<int64_t> ids(token_ids.begin(), token_ids.begin() + 3);   // role ids, reference text, target text and tail
    ids.insert(ids.end(), ref_text_ids.begin(), ref_text_ids.end());
    ids.insert(ids.end(), token_ids.begin() + 3, token_ids.end());
    return synthesize_tokens_continue(ids, ref_codes, lang, params, all_codes);
}

std::vector<float> TTSEngine::extract_speaker_embedding(const std::string& audio_path) { // reference tts_onnx.cpp:331-365
    if (!has_speaker_encoder()) return {};
    std::vector<float> embed((size_t)spk_dim_);
    if (q3tts_extract_speaker_embedding_host(h_, audio_path.c_str(), embed.data()) != 0) {
        std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl; // "Failed to read audio: <path>" / "Failed to extract mel spectrogram"
        return {};
    }
    return embed;
}

std::vector<float> TTSEngine::extract_speaker_embedding(const std::vector<float>& pcm, int sample_rate) {
    if (!has_speaker_encoder()) return {};
    std::vector<float> embed((size_t)spk_dim_);
    const float* clip = pcm.data();
    const int64_t n = (int64_t)pcm.size();
    const int32_t rate = sample_rate;
    if (q3tts_speaker_embed_pcm_batch_host(h_, 1, &clip, &n, &rate, embed.data()) != 0) {
        std::cerr << "[TTSEngine] " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    return embed;
}

std::vector<std::vector<float>> TTSEngine::synthesize_tokens_batch(const std::vector<std::vector<int64_t>>& token_ids,
                                                                   Language lang, const SamplingParams& params) {
    std::vector<std::vector<float>> out(token_ids.size());
    if (!ready_ || token_ids.empty()) return out;
    q3tts_config cfg;
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    std::vector<int64_t> flat;
    std::vector<int32_t> offs(1, 0);
    for (const auto& t : token_ids) { flat.insert(flat.end(), t.begin(), t.end()); offs.push_back((int32_t)flat.size()); }
    // capacity: samples of max_new_tokens frames
    q3tts_default_config("0.6b", &cfg);
    const int64_t cap = (int64_t)params.max_new_tokens * 1920 + 1920;
    std::vector<float*> ptrs(token_ids.size());
    for (size_t i = 0; i < token_ids.size(); ++i) { out[i].resize((size_t)cap); ptrs[i] = out[i].data(); }
    std::vector<int64_t> lens(token_ids.size(), 0);
    std::vector<int32_t> frames(token_ids.size(), 0);
    const int rc = q3tts_synthesize_batch_host(h_, (int)token_ids.size(), flat.data(), offs.data(), lang_index(lang), &sp, seed_, 0,
                                               ptrs.data(), cap, lens.data(), frames.data(), nullptr);
    if (rc != 0) { // reference tts_onnx.cpp:432-435: log, return empty
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        for (auto& v : out) v.clear();
        return out;
    }
    for (size_t i = 0; i < out.size(); ++i) { out[i].resize((size_t)std::min<int64_t>(lens[i], cap)); (void)apply_speed(out[i]); }
    return out;
}

std::vector<std::vector<float>> TTSEngine::synthesize_tokens_batch_instruct_shared(const std::vector<std::vector<int64_t>>& token_ids,
                                                                                   const std::vector<int64_t>& framed_instruct_ids,
                                                                                   Language lang, const SamplingParams& params) {
    if (framed_instruct_ids.empty()) return synthesize_tokens_batch(token_ids, lang, params);
    std::vector<std::vector<float>> out(token_ids.size());
    if (!ready_ || token_ids.empty()) return out;
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    std::vector<int64_t> flat;
    std::vector<int32_t> offs(1, 0);
    for (const auto& t : token_ids) { flat.insert(flat.end(), t.begin(), t.end()); offs.push_back((int32_t)flat.size()); }
    auto fail = [&]() {   // reference tts_onnx.cpp:432-435: log, return empty
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        for (auto& v : out) v.clear();
        return out;
    };
    for (int b = 0; b < max_batch_; ++b) (void)q3tts_slot_release(h_, b);   // the prefix is prefilled in a free slot
    int pid = -1;
    if (q3tts_prefix_create_instruct(h_, framed_instruct_ids.data(), (int)framed_instruct_ids.size(), &pid) != 0) return fail();
    const int64_t cap = (int64_t)params.max_new_tokens * 1920 + 1920;
    std::vector<float*> ptrs(token_ids.size());
    for (size_t i = 0; i < token_ids.size(); ++i) { out[i].resize((size_t)cap); ptrs[i] = out[i].data(); }
    std::vector<int64_t> lens(token_ids.size(), 0);
    std::vector<int32_t> frames(token_ids.size(), 0), pids(token_ids.size(), pid);
    const int rc = q3tts_synthesize_prefixed_host(h_, (int)token_ids.size(), flat.data(), offs.data(), lang_index(lang), nullptr, &sp, nullptr, seed_, 0,
                                                  ptrs.data(), cap, lens.data(), frames.data(), nullptr, 0, nullptr, nullptr, pids.data());
    if (rc != 0) { (void)fail(); (void)q3tts_prefix_release(h_, pid); return out; }
    (void)q3tts_prefix_release(h_, pid);
    for (size_t i = 0; i < out.size(); ++i) { out[i].resize((size_t)std::min<int64_t>(lens[i], cap)); (void)apply_speed(out[i]); }
    return out;
}

int TTSEngine::synthesize_tokens_streaming(const std::vector<int64_t>& token_ids, Language lang, const SamplingParams& params, int chunk_frames,
                                           int left_context_frames, const std::function<void(const float*, size_t)>& on_audio) {
    if (!ready_ || chunk_frames < 1) return -1;
    q3tts_config cfg;
    q3tts_default_config("0.6b", &cfg);
    const int H = cfg_hidden_;
    std::vector<float> prompt((size_t)16 * H), trailing((size_t)1024 * H);
    int S = 0, nt = 0;
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    auto fail = [&]() { std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl; (void)q3tts_slot_release(h_, 0); return -1; };
    for (int b = 0; b < max_batch_; ++b) (void)q3tts_slot_release(h_, b);
    if (q3tts_build_prompt_host(h_, token_ids.data(), (int)token_ids.size(), lang_index(lang), nullptr, prompt.data(), &S, trailing.data(), 1024, &nt) != 0) return fail();
    if (q3tts_slot_begin(h_, 0, prompt.data(), S, trailing.data(), nt, &sp, seed_, 0, 0) != 0) return fail();
    std::vector<float> pcm((size_t)chunk_frames * 1920 + 1920);
    int done = 0;
    // with a speed the chunks pass a stretcher of this call's own; its tail leaves in one more chunk at the end
    int stretcher = -1;
    size_t received = 0;
    std::vector<float> fast;
    if (speed_ != 1000 && q3tts_speed_begin(h_, speed_, &stretcher) != 0) return fail();
    // with a pitch the chunks first pass a pitch stage of this call's own, ahead of the stretcher
    int shifter = -1;
    size_t shifted = 0;
    std::vector<float> low;
    if (pitch_ != 1000 && q3tts_pitch_begin(h_, pitch_, &shifter) != 0) {
        const int rc = fail();
        if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
        return rc;
    }
    // with a tone the stretcher's chunks pass a tone stage of this call's own, ahead of the loudness stage
    int equaliser = -1;
    std::vector<float> shaped;
    if (tone_n_ > 0 && tone_begin(&equaliser) != 0) {
        const int rc = fail();
        if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
        if (shifter >= 0) (void)q3tts_pitch_end(h_, shifter);
        return rc;
    }
    // with a loudness the stretcher's chunks pass a loudness stage of this call's own, ahead of the level stage
    int normaliser = -1;
    size_t normalised = 0;
    std::vector<float> even;
    if (loud_ && q3tts_loudness_begin(h_, loud_target_, loud_range_, 0, &normaliser) != 0) {
        const int rc = fail();
        if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
        if (shifter >= 0) (void)q3tts_pitch_end(h_, shifter);
        if (equaliser >= 0) (void)q3tts_tone_end(h_, equaliser);
        return rc;
    }
    // with a level the chunks (the stretcher's, when there is one) pass a level stage of this call's own in the same way
    int leveler = -1;
    size_t levelled = 0;
    std::vector<float> loud;
    if ((gain_cb_ != 0 || ceiling_ != 0) && q3tts_level_begin(h_, gain_cb_, ceiling_, &leveler) != 0) {
        const int rc = fail();
        if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
        if (shifter >= 0) (void)q3tts_pitch_end(h_, shifter);
        if (equaliser >= 0) (void)q3tts_tone_end(h_, equaliser);
        if (normaliser >= 0) (void)q3tts_loudness_end(h_, normaliser);
        return rc;
    }
    auto fail_s = [&]() {
        const int rc = fail();
        if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
        if (shifter >= 0) (void)q3tts_pitch_end(h_, shifter);
        if (equaliser >= 0) (void)q3tts_tone_end(h_, equaliser);
        if (normaliser >= 0) (void)q3tts_loudness_end(h_, normaliser);
        if (leveler >= 0) (void)q3tts_level_end(h_, leveler);
        return rc;
    };
    auto emit = [&](const float* p, size_t n, bool last) -> bool {   // a chunk at 24 kHz on its way out
        if (leveler < 0) { if (n > 0) on_audio(p, n); return true; }
        loud.clear();
        if (!level_push(leveler, p, n, last, levelled, loud)) return false;
        levelled += n;
        if (!loud.empty()) on_audio(loud.data(), loud.size());
        return true;
    };
    auto feed = [&](const float* p, size_t n, bool last) -> bool {   // a chunk from the vocoder: pitch stage, stretcher, tone stage, loudness stage, then emit
        if (shifter >= 0) {
            low.clear();
            if (!pitch_push(shifter, p, n, last, shifted, low)) return false;
            shifted += n;
            p = low.data(); n = low.size();
        }
        if (stretcher >= 0) {
            fast.clear();
            if (!stretch_push(stretcher, p, n, last, received, fast)) return false;
            received += n;
            p = fast.data(); n = fast.size();
        }
        if (equaliser >= 0) {
            shaped.clear();
            if (!tone_push(equaliser, p, n, last, shaped)) return false;
            p = shaped.data(); n = shaped.size();
        }
        if (normaliser >= 0) {
            even.clear();
            if (!loudness_push(normaliser, p, n, last, normalised, even)) return false;
            normalised += n;
            p = even.data(); n = even.size();
        }
        return emit(p, n, last && leveler >= 0);
    };
    for (;;) {
        const int want = std::min(chunk_frames, params.max_new_tokens - done);
        const int active = want > 0 ? q3tts_decode_steps(h_, want) : 0;
        if (active < 0) return fail_s();
        int nf = 0, fin = 0;
        if (q3tts_slot_status(h_, 0, &nf, &fin) != 0) return fail_s();
        if (nf > done) {
            int64_t n = 0;
            const int ctx = left_context_frames < 0 ? nf : left_context_frames;
            if (q3tts_slot_codec_decode_range_host(h_, 0, done, nf, ctx, pcm.data(), (int64_t)pcm.size(), &n) != 0) return fail_s();
            const size_t got = (size_t)std::min<int64_t>(n, (int64_t)pcm.size());
            if (!feed(pcm.data(), got, false)) return fail_s();
            done = nf;
        }
        if (active == 0 || want <= 0) break;
    }
    if ((shifter >= 0 || stretcher >= 0 || equaliser >= 0 || normaliser >= 0 || leveler >= 0) && !feed(pcm.data(), 0, true)) return fail_s();   // the stages' tails, in their order
    if (shifter >= 0) (void)q3tts_pitch_end(h_, shifter);
    if (stretcher >= 0) (void)q3tts_speed_end(h_, stretcher);
    if (equaliser >= 0) (void)q3tts_tone_end(h_, equaliser);
    if (normaliser >= 0) (void)q3tts_loudness_end(h_, normaliser);
    if (leveler >= 0) (void)q3tts_level_end(h_, leveler);
    (void)q3tts_slot_release(h_, 0);
    return done;
}

std::vector<int> TTSEngine::synthesize_tokens_batch_streaming(const std::vector<std::vector<int64_t>>& token_ids, Language lang, const SamplingParams& params,
                                                              int chunk_frames, const std::function<bool(int, const float*, size_t, bool)>& on_audio) {
    return synthesize_tokens_batch_streaming(token_ids, lang, params, chunk_frames, on_audio, nullptr);
}

// utterance u's frames out of a scheduler entry's codes_out [n_utt][max_new][n_groups]
static void split_codes(const std::vector<int64_t>& all, const std::vector<int32_t>& frames, int max_new, int G, std::vector<std::vector<int64_t>>* codes) {
    if (!codes) return;
    codes->assign(frames.size(), std::vector<int64_t>());
    for (size_t u = 0; u < frames.size(); ++u)
        (*codes)[u].assign(all.begin() + (ptrdiff_t)(u * (size_t)max_new * G), all.begin() + (ptrdiff_t)((u * (size_t)max_new + (size_t)frames[u]) * G));
}

std::vector<int> TTSEngine::synthesize_tokens_live(int n_utt, const std::function<bool(int, std::vector<int64_t>&, bool&)>& text_source, Language lang,
                                                   const SamplingParams& params, int chunk_frames,
                                                   const std::function<bool(int, const float*, size_t, bool)>& on_audio,
                                                   std::vector<std::vector<int64_t>>* codes) {
    if (!ready_ || n_utt < 1 || chunk_frames < 1 || !on_audio || !text_source) return {};
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    std::vector<int32_t> frames((size_t)n_utt, 0);
    struct Ctx { const std::function<bool(int, const float*, size_t, bool)>* f; const std::function<bool(int, std::vector<int64_t>&, bool&)>* t;
                 std::vector<std::vector<int64_t>> backlog; std::vector<char> closed; } ctx{ &on_audio, &text_source, {}, {} };
    ctx.backlog.resize((size_t)n_utt); ctx.closed.assign((size_t)n_utt, 0);
    const q3tts_audio_cb cb = [](void* user, int utt, int, int, const float* pcm, int64_t n, int finished) -> int {
        return (*static_cast<Ctx*>(user)->f)(utt, pcm, (size_t)n, finished != 0) ? 1 : 0;
    };
    const q3tts_text_cb tcb = [](void* user, int utt, int64_t* ids, int cap, int32_t* n, int32_t* closed) -> int {
        Ctx& c = *static_cast<Ctx*>(user);
        std::vector<int64_t>& bl = c.backlog[(size_t)utt];
        if (bl.empty() && !c.closed[(size_t)utt]) {
            bool cl = false;
            if (!(*c.t)(utt, bl, cl)) return 1;
            c.closed[(size_t)utt] = cl ? 1 : 0;
        }
        const size_t m = std::min(bl.size(), (size_t)std::max(cap, 0));   // what does not fit this poll goes out at the next
        std::copy(bl.begin(), bl.begin() + (ptrdiff_t)m, ids);
        bl.erase(bl.begin(), bl.begin() + (ptrdiff_t)m);
        *n = (int32_t)m;
        *closed = bl.empty() && c.closed[(size_t)utt] ? 1 : 0;
        return 0;
    };
    std::vector<int64_t> all;
    if (codes) all.assign((size_t)n_utt * (size_t)params.max_new_tokens * (size_t)n_groups_, 0);
    if (sink_on()) sink_fn_ = [&](int utt, const void* pcm, int64_t n, int finished) { return on_audio(utt, (const float*)pcm, (size_t)n, finished != 0) ? 1 : 0; };
    const int rc = q3tts_synthesize_live_host(h_, n_utt, tcb, &ctx, lang_index(lang), nullptr, &sp, nullptr, seed_, 0,
                                              nullptr, 0, nullptr, frames.data(), codes ? all.data() : nullptr, chunk_frames, cb, &ctx);
    sink_fn_ = nullptr;
    if (rc != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    split_codes(all, frames, params.max_new_tokens, n_groups_, codes);
    return std::vector<int>(frames.begin(), frames.end());
}

std::vector<int> TTSEngine::synthesize_tokens_batch_streaming(const std::vector<std::vector<int64_t>>& token_ids, Language lang, const SamplingParams& params,
                                                              int chunk_frames, const std::function<bool(int, const float*, size_t, bool)>& on_audio,
                                                              std::vector<std::vector<int64_t>>* codes) {
    if (!ready_ || token_ids.empty() || chunk_frames < 1 || !on_audio) return {};
    q3tts_sampling sp{ params.temperature, params.top_p, params.top_k, params.repetition_penalty, params.max_new_tokens };
    std::vector<int64_t> flat;
    std::vector<int32_t> offs(1, 0);
    for (const auto& t : token_ids) { flat.insert(flat.end(), t.begin(), t.end()); offs.push_back((int32_t)flat.size()); }
    std::vector<int32_t> frames(token_ids.size(), 0);
    struct Ctx { const std::function<bool(int, const float*, size_t, bool)>* f; } ctx{ &on_audio };
    const q3tts_audio_cb cb = [](void* user, int utt, int, int, const float* pcm, int64_t n, int finished) -> int {
        return (*static_cast<Ctx*>(user)->f)(utt, pcm, (size_t)n, finished != 0) ? 1 : 0;
    };
    std::vector<int64_t> all;
    if (codes) all.assign(token_ids.size() * (size_t)params.max_new_tokens * (size_t)n_groups_, 0);
    if (sink_on()) sink_fn_ = [&](int utt, const void* pcm, int64_t n, int finished) { return on_audio(utt, (const float*)pcm, (size_t)n, finished != 0) ? 1 : 0; };
    const int rc = q3tts_synthesize_stream_host(h_, (int)token_ids.size(), flat.data(), offs.data(), lang_index(lang), nullptr, &sp, nullptr, seed_, 0,
                                                nullptr, 0, nullptr, frames.data(), codes ? all.data() : nullptr, chunk_frames, cb, &ctx);
    sink_fn_ = nullptr;
    if (rc != 0) {
        std::cerr << "[TTSEngine] Synthesis error: " << q3tts_last_error(h_) << std::endl;
        return {};
    }
    split_codes(all, frames, params.max_new_tokens, n_groups_, codes);
    return std::vector<int>(frames.begin(), frames.end());
}

std::vector<float> TTSEngine::synthesize_tokens(const std::vector<int64_t>& token_ids, Language lang, const SamplingParams& params) {
    if (!ready_) return {};
    auto r = synthesize_tokens_batch({ token_ids }, lang, params);
    return r.empty() ? std::vector<float>() : std::move(r[0]);
}

} // namespace leaxer_qwen
