// tts_engine.h — the reference's public surface (leaxer_qwen::TTSEngine, reference src/tts_onnx.h:
// 29-105, 118-164, 230-238) re-implemented over libq3tts_hip.so.  Same namespace, type names, method
// names, argument meaning and error behaviour (errors never throw: is_ready()/get_error(), empty
// vector on a failed synthesis, messages on stderr prefixed "[TTSEngine]"), so a program written
// against the reference header compiles against this one.
#ifndef LEAXER_QWEN_TTS_ENGINE_H
#define LEAXER_QWEN_TTS_ENGINE_H

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct q3tts_engine;
struct q3tts_tokenizer;

namespace leaxer_qwen {

namespace config { // reference src/tts_onnx.h:29-70
constexpr int HIDDEN_SIZE = 1024, NUM_LAYERS = 28, NUM_KV_HEADS = 8, HEAD_DIM = 128, VOCAB_SIZE = 3072;
constexpr int NUM_CODE_GROUPS = 16, SUBCODE_VOCAB_SIZE = 2048;
constexpr int64_t TTS_BOS = 151672, TTS_EOS = 151673, TTS_PAD = 151671;
constexpr int64_t IM_START = 151644, IM_END = 151645, ASSISTANT = 77091;
constexpr int64_t CODEC_BOS = 2149, CODEC_EOS = 2150, CODEC_PAD = 2148, CODEC_THINK = 2154, CODEC_NOTHINK = 2155;
constexpr int64_t CODEC_THINK_BOS = 2156, CODEC_THINK_EOS = 2157;
constexpr int64_t LANG_ENGLISH = 2050, LANG_CHINESE = 2051, LANG_JAPANESE = 2052, LANG_KOREAN = 2053;
constexpr int MAX_NEW_TOKENS = 2048;
constexpr float DEFAULT_TEMPERATURE = 0.8f, DEFAULT_TOP_P = 0.95f;
constexpr int DEFAULT_TOP_K = 50;
constexpr int SAMPLE_RATE = 24000;
} // namespace config

enum class Language { Auto, English, Chinese, Japanese, Korean };
enum class Speaker { None, Serena, Vivian, Uncle_Fu, Dylan, Eric, Ryan, Aiden, Ono_Anna, Sohee };
Speaker parse_speaker(const std::string& name);

struct SamplingParams {
    float temperature = config::DEFAULT_TEMPERATURE;
    float top_p = config::DEFAULT_TOP_P;
    int top_k = config::DEFAULT_TOP_K;
    float repetition_penalty = 1.0f; // on the first codebook's ids an utterance has emitted (include/q3tts.h: q3tts_sampling); 1 = off.  The reference declares it and never reads it
    int max_new_tokens = config::MAX_NEW_TOKENS;
};

class TTSEngine {
public:
    // model_dir: a directory holding `model.q3w` (see q3tts_save_weights_file / tools/pack_weights.py),
    // or the literal "synthetic:<seed>" for seeded random 0.6B weights (benchmarks, smoke tests).
    // vocab.json + merges.txt are looked up where the reference looks (<parent of model_dir>/models/
    // Qwen3-TTS-12Hz-0.6B-Base/, tts_onnx.cpp:110-112), then in model_dir.
    // audio_encoder: a synthetic: model is created with the 12 Hz tokenizer's encoder enabled (q3tts_config_enable_audio_encoder); a
    // weight file has it when it carries the enc.* tensors, whatever this says
    explicit TTSEngine(const std::string& model_dir, bool audio_encoder = false);
    ~TTSEngine();
    TTSEngine(const TTSEngine&) = delete;
    TTSEngine& operator=(const TTSEngine&) = delete;
    // A second ready engine on the donor's GPU over the same model directory's tokenizer and the donor's weights, held, not copied
    // (q3tts_create_sharing): one engine per worker thread costs one set of weights.  Slots, KV cache, streams and every setting
    // (seed, output format, speed, level, pitch, loudness: at their defaults) are its own.  Null, with the reason on stderr, on failure.
    static std::unique_ptr<TTSEngine> share_weights(const TTSEngine& donor);

    std::vector<float> synthesize(const std::string& text, Language lang = Language::Auto,
                                  const SamplingParams& params = SamplingParams());
    std::vector<float> synthesize_clone(const std::string& text, const std::string& ref_audio_path,
                                        Language lang = Language::Auto, const SamplingParams& params = SamplingParams());
    std::vector<float> synthesize_speaker(const std::string& text, Speaker speaker, Language lang = Language::Auto,
                                          const SamplingParams& params = SamplingParams());
    std::vector<float> synthesize_tokens(const std::vector<int64_t>& token_ids, Language lang = Language::Auto,
                                         const SamplingParams& params = SamplingParams());
    std::vector<float> extract_speaker_embedding(const std::string& audio_path);
    // the same for reference audio already in memory (mono samples at sample_rate): resampling, log-mel and encoder all run on the GPU
    std::vector<float> extract_speaker_embedding(const std::vector<float>& pcm, int sample_rate);

    // batch extension: independent utterances share one decode loop (one result per utterance)
    std::vector<std::vector<float>> synthesize_tokens_batch(const std::vector<std::vector<int64_t>>& token_ids,
                                                            Language lang = Language::Auto,
                                                            const SamplingParams& params = SamplingParams());
    std::vector<std::vector<float>> synthesize_batch(const std::vector<std::string>& texts, Language lang = Language::Auto,
                                                     const SamplingParams& params = SamplingParams());
    // streaming extension: `on_audio` receives each chunk's samples as soon as its frames exist (exactly the
    // samples the whole-utterance decode would return for them when left_context_frames covers the history; < 0 = all of it).
    // Returns the number of frames generated, -1 on error.
    int synthesize_tokens_streaming(const std::vector<int64_t>& token_ids, Language lang, const SamplingParams& params, int chunk_frames,
                                    int left_context_frames, const std::function<void(const float*, size_t)>& on_audio);
    // the same for a batch: every chunk_frames steps each utterance with new audio gets on_audio(utt, pcm, n, finished) — its tail with
    // finished = true, once and last; more utterances than slots queue.  A true return from on_audio cancels the job.  Returns the
    // frames generated per utterance (empty on error).
    std::vector<int> synthesize_tokens_batch_streaming(const std::vector<std::vector<int64_t>>& token_ids, Language lang, const SamplingParams& params,
                                                       int chunk_frames, const std::function<bool(int, const float*, size_t, bool)>& on_audio);
    // codes (optional): utterance u's frames, [frames][n_groups] flattened
    std::vector<int> synthesize_tokens_batch_streaming(const std::vector<std::vector<int64_t>>& token_ids, Language lang, const SamplingParams& params,
                                                       int chunk_frames, const std::function<bool(int, const float*, size_t, bool)>& on_audio,
                                                       std::vector<std::vector<int64_t>>* codes);
    // live text extension (q3tts_synthesize_live_host): the same delivery for n_utt texts that arrive while their audio is generated.
    // text_source(utt, ids, closed) is polled between decode chunks while the utterance's text is open: it appends new ids to `ids`
    // (possibly none; the utterance's first ids are the role ids, as token_ids above) and sets closed once no more will come; a false
    // return cancels the job.  An utterance whose next frame has no text yet stalls and gets no audio that turn.
    std::vector<int> synthesize_tokens_live(int n_utt, const std::function<bool(int, std::vector<int64_t>&, bool&)>& text_source, Language lang,
                                            const SamplingParams& params, int chunk_frames,
                                            const std::function<bool(int, const float*, size_t, bool)>& on_audio,
                                            std::vector<std::vector<int64_t>>* codes = nullptr);
    void set_seed(uint64_t seed) { seed_ = seed; }
    // ids of `text` from the loaded tokenizer (reference io::tokenize, src/io/tokenizer.h:22)
    std::vector<int32_t> tokenize(const std::string& text) const;

    // clone with a ready speaker embedding (what synthesize_clone does after extract_speaker_embedding)
    std::vector<float> synthesize_tokens_clone(const std::vector<int64_t>& token_ids, const std::vector<float>& speaker_embed,
                                               Language lang = Language::Auto, const SamplingParams& params = SamplingParams());
    // Voice instructions (the reference README's roadmap row "Voice instructions (--instruct), 1.7B-VoiceDesign: Planned"; these sit
    // beside the reference's methods).  `instruct` is tokenised with the loaded vocab, framed as a chat turn (q3tts_frame_instruct_ids:
    // [HINT], unpinned) and its projected rows go in front of the prompt (q3tts_build_prompt_instruct_host).  The speaker_embed overload
    // combines it with voice clone (--ref + --instruct).  An empty instruction is plain synthesis.  max_new_tokens is lowered where
    // prompt + max_new_tokens would pass the engine's context.
    std::vector<float> synthesize_instruct(const std::string& text, const std::string& instruct, Language lang = Language::Auto,
                                           const SamplingParams& params = SamplingParams());
    std::vector<float> synthesize_instruct(const std::string& text, const std::string& instruct, const std::vector<float>& speaker_embed,
                                           Language lang = Language::Auto, const SamplingParams& params = SamplingParams());
    // the same over ids: token_ids framed as synthesize_tokens takes them, instruct_text_ids the instruction's text ids (framed here)
    std::vector<float> synthesize_tokens_instruct(const std::vector<int64_t>& token_ids, const std::vector<int32_t>& instruct_text_ids,
                                                  const std::vector<float>& speaker_embed, Language lang = Language::Auto,
                                                  const SamplingParams& params = SamplingParams());
    // A batch read in one designed voice: the instruction (already framed ids, q3tts_frame_instruct_ids) is prefilled ONCE as a shared
    // prompt prefix (include/q3tts.h: q3tts_prefix_create_instruct) and every utterance is begun behind a copy of its KV rows
    // (q3tts_synthesize_prefixed_host); the prefix is released when the job is done.  An empty instruction is synthesize_tokens_batch.
    std::vector<std::vector<float>> synthesize_tokens_batch_instruct_shared(const std::vector<std::vector<int64_t>>& token_ids,
                                                                            const std::vector<int64_t>& framed_instruct_ids,
                                                                            Language lang = Language::Auto,
                                                                            const SamplingParams& params = SamplingParams());
    // Continue from codes (include/q3tts.h: q3tts_synthesize_continue_host; beside the reference's methods).  prefix_codes holds recorded
    // frames, n_groups() ids each, frame-major: the utterance is generated as if these had been its first frames (the previous sentence
    // of a document with its text in token_ids, the reference codes of an in-context clone, an utterance to resume), and the returned
    // samples are those of the NEW frames only — they join the prefix's own audio without a seam.  all_codes (optional) receives prefix
    // + new frames.  An empty prefix is synthesize_tokens.  max_new_tokens is lowered where prompt + prefix + max_new_tokens would pass
    // the engine's context.
    std::vector<float> synthesize_tokens_continue(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes,
                                                  Language lang = Language::Auto, const SamplingParams& params = SamplingParams(),
                                                  std::vector<int64_t>* all_codes = nullptr);
    // The same with the new audio delivered while it is generated (include/q3tts.h: q3tts_synthesize_continue_stream_host; the shape of
    // synthesize_tokens_batch_streaming for one utterance): every chunk_frames steps on_audio(pcm, n, finished) receives the samples of
    // the new frames generated since the previous call — the prefix is history, never decoded to audio — the tail with finished = true,
    // once and last; a true return cancels.  Returns the frames generated (prefix included), -1 on error.
    int synthesize_tokens_continue_streaming(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& prefix_codes, Language lang,
                                             const SamplingParams& params, int chunk_frames,
                                             const std::function<bool(const float*, size_t, bool)>& on_audio,
                                             std::vector<int64_t>* all_codes = nullptr);
    // Audio -> codes (include/q3tts.h: q3tts_audio_encode_batch_host; [HINT] the 12 Hz tokenizer's encoder, beside the reference's
    // methods): mono samples at sample_rate -> frames of n_groups() ids, frame-major — what synthesize_tokens_continue takes.  Empty on error.
    std::vector<int64_t> encode_audio(const std::vector<float>& pcm, int sample_rate);
    std::vector<int64_t> encode_audio(const std::string& wav_path);
    // Audio -> codes while the audio arrives (include/q3tts.h: q3tts_audio_stream_begin / _push_host / _end; [HINT] as encode_audio):
    // a stream takes mono samples at its source's rate (24 kHz unless begun otherwise; float, or int16 when begun with pcm16) in
    // pushes of any size (at most 60 s each) and returns the frames each push completes; the concatenation is bit-identical to
    // encode_audio of the concatenated samples at that rate (int16 v is the float v / 32768).  max_samples: the most of its own
    // samples the stream will take (0: 60 s; at most one hour).  audio_stream_begin returns the stream id, -1 on error; a failed
    // push returns no frames and sets *ok = false when ok is given.
    int audio_stream_begin(int64_t max_samples = 0);
    int audio_stream_begin(int64_t max_samples, int sample_rate /* 24000: the overload above */, bool pcm16 = false);
    std::vector<int64_t> audio_stream_push(int id, const float* pcm, size_t n, bool finish = false, bool* ok = nullptr);
    std::vector<int64_t> audio_stream_push(int id, const int16_t* pcm, size_t n, bool finish = false, bool* ok = nullptr);   // streams begun with pcm16
    // the same for a source in any Q3TTS_PCM_* format; Q3TTS_PCM_MULAW / _ALAW streams take G.711 bytes through the uint8_t overload
    int audio_stream_begin_encoded(int64_t max_samples, int sample_rate, int format);
    std::vector<int64_t> audio_stream_push(int id, const uint8_t* pcm, size_t n, bool finish = false, bool* ok = nullptr);
    void audio_stream_end(int id);
    // In-context voice clone ([HINT]): the reference audio is encoded, the text becomes reference text +
    // target text (ref_text_ids go between token_ids' three role ids and its text) and the utterance is continued behind the
    // reference's codes; the returned samples are the target's only.  Exactly encode_audio + synthesize_tokens_continue.
    std::vector<float> synthesize_clone_icl(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& ref_text_ids,
                                            const std::vector<float>& ref_pcm, int ref_rate, Language lang = Language::Auto,
                                            const SamplingParams& params = SamplingParams(), std::vector<int64_t>* all_codes = nullptr);
    std::vector<float> synthesize_clone_icl(const std::vector<int64_t>& token_ids, const std::vector<int64_t>& ref_text_ids,
                                            const std::string& ref_wav_path, Language lang = Language::Auto,
                                            const SamplingParams& params = SamplingParams(), std::vector<int64_t>* all_codes = nullptr);
    // Output format (include/q3tts.h: q3tts_engine_set_sink, q3tts_pcm_sink_*; beside the reference's methods, which deliver 24 kHz
    // float only).  While a format other than 24 000 Hz float is set, the scheduler's streaming methods
    // (synthesize_tokens_batch_streaming, synthesize_tokens_live, synthesize_tokens_continue_streaming) deliver their chunks at
    // sample_rate (4 000 .. 192 000), band-limited on the GPU; the finishing chunk carries the resampler's tail.  With pcm16 the
    // pointer a callback receives addresses int16_t samples (cast it; n still counts samples).  set_output_format(24000, false) is
    // the default again.  false (and get_error()) for a rate the engine refuses.  The non-streaming methods keep returning 24 kHz
    // float: convert_output brings a whole clip to the set format in one push + finish of the same resampler (exactly one of
    // f32 / s16 is filled, by the format; at 24 000 Hz float f32 is the input).
    bool set_output_format(int sample_rate, bool pcm16 = false);
    int output_rate() const { return out_rate_; }
    bool output_pcm16() const { return out_format_ == 1; }
    bool convert_output(const std::vector<float>& pcm24, std::vector<float>* f32, std::vector<int16_t>* s16);
    // The same with any Q3TTS_PCM_* format (0 float, 1 int16, 2 mu-law, 3 A-law): Q3TTS_PCM_MULAW / _ALAW deliver G.711 bytes (include/q3tts.h "G.711": the byte of the
    // int16 the pcm16 format gives), one uint8_t per sample in the callbacks' pointer and in convert_output's g711.
    // set_output_format(rate, pcm16) is set_output_encoding(rate, pcm16 ? Q3TTS_PCM_S16 : Q3TTS_PCM_F32).
    bool set_output_encoding(int sample_rate, int format);
    int output_encoding() const { return out_format_; }
    bool convert_output(const std::vector<float>& pcm24, std::vector<float>* f32, std::vector<int16_t>* s16, std::vector<uint8_t>* g711);
    // Speaking rate (include/q3tts.h: q3tts_engine_set_speed, q3tts_speed_*; the reference has no speed control).  speed 1.25 makes
    // every synthesize* method's audio 25 % faster at the same pitch (WSOLA on the GPU); the engine works in permille,
    // S = round(1000 * speed), 500 .. 2000, and 1.0 is no stage at all.  The scheduler's streaming methods stretch inside their
    // streams (ahead of the output format's resampler; the finishing chunk carries the tail), synthesize_tokens_streaming through a
    // stretcher of its own behind the chunks, the one-shot methods run the stage over the whole clip (apply_speed).  false (and
    // get_error(), naming the range) for a speed the engine refuses.
    bool set_speed(float speed);
    int speed_permille() const { return speed_; }
    bool apply_speed(std::vector<float>& pcm24);   // the whole clip through the stage, in place; speed 1.0 leaves it as it is; then apply_level
    // Output level (include/q3tts.h: q3tts_engine_set_level, q3tts_level_*; the reference has no volume control).  gain_db decibels of
    // gain, rounded to centibels (-60 .. +40); ceiling the limiter's linear ceiling, rounded to permille (0: gain only; otherwise 0.001 ..
    // 1.0); (0, 0) is no stage at all.  The stage stands behind the stretcher and ahead of the sink on every path that honours
    // set_speed, in the same way: inside the scheduler's streaming pushes, as a stage of its own behind synthesize_tokens_streaming's
    // chunks, over the whole clip in the one-shot methods (apply_level, which apply_speed calls last).  false (and get_error(), naming
    // the range) for values the engine refuses.
    bool set_level(float gain_db, float ceiling);
    int gain_centibels() const { return gain_cb_; }
    int ceiling_permille() const { return ceiling_; }
    bool apply_level(std::vector<float>& pcm24);   // the whole clip through the stage, in place; (0, 0) leaves it as it is
    // Loudness (include/q3tts.h: q3tts_engine_set_loudness, q3tts_loudness_*; the reference has no loudness control).  lufs: the
    // target, -40 .. -5 (rounded to 0.1); range_db: the largest boost or cut, 0 .. 40.  A BS.1770 meter and a gain that moves towards the
    // target by at most 1 dB per 100 ms, on the GPU between the stretcher and the level stage, on every path that honours set_speed, in
    // the same way (apply_loudness, which apply_speed calls before apply_level).  The stage delivers 100 ms late; the last call of a
    // streaming method carries its tail.  false (and get_error(), naming the range) for a value the engine refuses.
    bool set_loudness(float lufs, float range_db = 20.0f);
    void clear_loudness();                            // no stage again
    bool has_loudness() const { return loud_; }
    bool apply_loudness(std::vector<float>& pcm24);   // the whole clip through the stage, in place; no stage leaves it as it is
    // Tone (include/q3tts.h: q3tts_engine_set_tone, q3tts_tone_*; the reference has no equaliser).  spec: a preset's name (telephone,
    // rumble, presence, warm; unheard and untuned) or sections "kind:Hz[:dB]:Q" separated by commas, as q3tts_tone_parse reads them.  A
    // cascade of 1 .. 8 biquads on the GPU between the stretcher and the loudness stage, on every path that honours set_speed, in the
    // same way (apply_tone, which apply_speed calls before apply_loudness).  No latency.  false (and get_error(), naming the field) for
    // a spec the engine refuses.
    bool set_tone(const char* spec);
    void clear_tone();                            // no stage again
    bool has_tone() const { return tone_n_ > 0; }
    bool apply_tone(std::vector<float>& pcm24);   // the whole clip through the stage, in place; no stage leaves it as it is
    // Pitch (include/q3tts.h: q3tts_engine_set_pitch, q3tts_pitch_*; the reference has no pitch control).  semitones -12 .. +12; the
    // engine works in permille, r = round(1000 * 2^(semitones / 12)), and 0 semitones is no stage at all.  TD-PSOLA on the GPU: the
    // fundamental moves, the spectral envelope stays.  The stage stands first behind the vocoder on every path that honours set_speed,
    // in the same way: inside the scheduler's streaming pushes, as a stage of its own ahead of synthesize_tokens_streaming's
    // stretcher, over the whole clip in the one-shot methods (apply_pitch, which apply_speed calls first).  false (and get_error(),
    // naming the range) for a value the engine refuses.
    bool set_pitch(float semitones);
    int pitch_permille() const { return pitch_; }
    bool apply_pitch(std::vector<float>& pcm24);   // the whole clip through the stage, in place; 0 semitones leaves it as it is
    bool has_audio_encoder() const;
    int n_groups() const { return n_groups_; }
    bool has_speaker_encoder() const; // true when the weight file carries the spk.* tensors (reference: speaker_encoder.onnx present)
    bool is_ready() const { return ready_; }
    const std::string& get_error() const { return error_msg_; }

private:
    TTSEngine() = default;                              // share_weights fills it in
    bool load_tokenizer(const std::string& model_dir);  // false: present but unreadable (error_msg_ set); absent is a warning
    std::string model_dir_;
    bool wrap_text(const std::string& text, std::vector<int64_t>& ids) const;
    std::vector<int64_t> audio_stream_push_any(int id, const void* pcm, size_t n, bool finish, bool* ok, int kind);   // kind: 0 float, 1 int16, 2 G.711 bytes
    q3tts_engine* h_ = nullptr;
    q3tts_tokenizer* tok_ = nullptr;
    bool ready_ = false;
    std::string error_msg_;
    uint64_t seed_ = 0;
    int max_batch_ = 1;
    int spk_dim_ = 0;
    int cfg_hidden_ = 1024;
    int max_ctx_ = 0;
    int n_groups_ = config::NUM_CODE_GROUPS;
    int out_rate_ = config::SAMPLE_RATE;
    int out_format_ = 0;   // Q3TTS_PCM_F32 (include/q3tts.h)
    std::function<int(int, const void*, int64_t, int)> sink_fn_;   // the running streaming call's delivery, while an output format is set
    int speed_ = 1000;
    int gain_cb_ = 0, ceiling_ = 0;
    int pitch_ = 1000;
    bool loud_ = false;
    int loud_target_ = -160, loud_range_ = 200;
    int tone_n_ = 0;
    std::string tone_spec_;   // the spec set_tone accepted; this header stands alone (no q3tts.h), so the sections are formed from it where a stage begins
    int tone_begin(int* id);  // a tone stage of this engine's spec (q3tts_tone_begin's return)
    bool tone_push(int id, const float* in, size_t n, bool finish, std::vector<float>& out);
    bool loudness_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out);
    bool pitch_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out);
    bool level_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out);
    // one push of a stretcher of this engine: out receives the push's samples (appended)
    bool stretch_push(int id, const float* in, size_t n, bool finish, size_t received_before, std::vector<float>& out);
    bool sink_on() const { return out_rate_ != config::SAMPLE_RATE || out_format_ != 0; }
};

inline int64_t language_to_codec_id(Language lang) { // reference src/tts_onnx.h:230-238
    switch (lang) {
    case Language::English: return config::LANG_ENGLISH;
    case Language::Chinese: return config::LANG_CHINESE;
    case Language::Japanese: return config::LANG_JAPANESE;
    case Language::Korean: return config::LANG_KOREAN;
    default: return 0;
    }
}

} // namespace leaxer_qwen
#endif
