// leaxer-tts — command line of the MI355X engine.  Flag set of the reference CLI
// (reference src/main_onnx.cpp:60-77, 99-124): -m -p -o --lang --ref --temp --top-k --top-p --max-tokens -h, plus --rep-penalty (an extension),
// unknown flags ignored, 16-bit mono WAV at 24 kHz (clip to [-1,1], truncate x*32767).  Additions:
// --tokens "id,id,..." (pre-tokenised text between TTS_BOS and TTS_EOS, bypassing vocab.json/merges.txt),
// --seed N, --instruct TEXT / --instruct-tokens "id,id,..." (a voice instruction in front of the prompt: the reference README's roadmap
// row "Voice instructions (--instruct)"; combines with --ref), --save-codes FILE / --continue-codes FILE (with --tokens: write the
// utterance's codec frames, one per line; generate behind recorded frames — the WAV then holds the new audio only),
// --encode WAV --save-codes FILE (audio -> codes with the 12 Hz tokenizer's encoder, nothing else; --encode-chunk MS pushes the file MS
// milliseconds at a time through one encoder stream opened at the file's own rate: the same codes, and no 60 s limit), --ref WAV with --ref-text TEXT /
// --out-format pcm16|mulaw|alaw (G.711 bytes from the engine's sink, WAV format tags 7 / 6; --encode and --ref with --ref-text also read such files),
// --ref-tokens "id,id,..." (in-context clone: the reference's codes and text in front of the utterance; --ref alone stays the x-vector clone).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/q3tts.h"
#include "tts_engine.h"

using namespace leaxer_qwen;

static bool put(FILE* f, const void* p, size_t n) { return fwrite(p, 1, n, f) == n; }

static int save_wav16(const char* path, const std::vector<float>& audio, uint32_t rate) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    const uint32_t data = (uint32_t)(audio.size() * 2), riff = 36 + data, fmt = 16, bytes_per_s = rate * 2;
    const uint16_t pcm = 1, ch = 1, align = 2, bits = 16;
    bool ok = put(f, "RIFF", 4) && put(f, &riff, 4) && put(f, "WAVEfmt ", 8) && put(f, &fmt, 4) && put(f, &pcm, 2) && put(f, &ch, 2) &&
              put(f, &rate, 4) && put(f, &bytes_per_s, 4) && put(f, &align, 2) && put(f, &bits, 2) && put(f, "data", 4) && put(f, &data, 4);
    std::vector<int16_t> s(audio.size());
    for (size_t i = 0; i < audio.size(); ++i) {
        float v = audio[i] > 1.0f ? 1.0f : (audio[i] < -1.0f ? -1.0f : audio[i]);
        s[i] = (int16_t)(v * 32767.0f);
    }
    ok = ok && put(f, s.data(), s.size() * 2);
    fclose(f);
    return ok ? 0 : -1;
}

// the same file from samples that already are int16 (--out-rate: the engine's sink converted them on the GPU, by the rule above)
static int save_wav16_raw(const char* path, const std::vector<int16_t>& s, uint32_t rate) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    const uint32_t data = (uint32_t)(s.size() * 2), riff = 36 + data, fmt = 16, bytes_per_s = rate * 2;
    const uint16_t pcm = 1, ch = 1, align = 2, bits = 16;
    bool ok = put(f, "RIFF", 4) && put(f, &riff, 4) && put(f, "WAVEfmt ", 8) && put(f, &fmt, 4) && put(f, &pcm, 2) && put(f, &ch, 2) &&
              put(f, &rate, 4) && put(f, &bytes_per_s, 4) && put(f, &align, 2) && put(f, &bits, 2) && put(f, "data", 4) && put(f, &data, 4);
    ok = ok && put(f, s.data(), s.size() * 2);
    fclose(f);
    return ok ? 0 : -1;
}

// G.711 (--out-format mulaw / alaw): the sink's bytes as they came.  WAVE_FORMAT_MULAW (7) / WAVE_FORMAT_ALAW (6): an 18-byte fmt
// chunk (cbSize 0), a fact chunk with the sample count, the data chunk padded to an even length (the pad byte counts in the RIFF
// size, not in the data size).
static int save_wav_g711(const char* path, const std::vector<uint8_t>& s, uint32_t rate, int format) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    const uint32_t data = (uint32_t)s.size(), pad = data & 1u, riff = 4 + (8 + 18) + (8 + 4) + (8 + data + pad), fmt = 18, fact = 4, bytes_per_s = rate;
    const uint16_t tag = format == Q3TTS_PCM_MULAW ? 7 : 6, ch = 1, align = 1, bits = 8, cb = 0;
    const uint8_t zero = 0;
    bool ok = put(f, "RIFF", 4) && put(f, &riff, 4) && put(f, "WAVEfmt ", 8) && put(f, &fmt, 4) && put(f, &tag, 2) && put(f, &ch, 2) &&
              put(f, &rate, 4) && put(f, &bytes_per_s, 4) && put(f, &align, 2) && put(f, &bits, 2) && put(f, &cb, 2) &&
              put(f, "fact", 4) && put(f, &fact, 4) && put(f, &data, 4) && put(f, "data", 4) && put(f, &data, 4);
    ok = ok && put(f, s.data(), s.size()) && (!pad || put(f, &zero, 1));
    fclose(f);
    return ok ? 0 : -1;
}

static void usage(const char* prog) {
    printf("Usage: %s [options]\n\nQwen3-TTS synthesis on MI355X (HIP)\n\nOptions:\n", prog);
    printf("  -m, --model DIR       model directory holding model.q3w, or synthetic:<seed> / synthetic-1.7b:<seed> (required)\n");
    printf("  -p, --prompt TEXT     text to synthesize (needs vocab.json + merges.txt, see README)\n");
    printf("      --tokens IDS      comma-separated text token ids (framed as IM_START ASSISTANT TTS_BOS ids TTS_EOS IM_END)\n");
    printf("  -o, --output PATH     output WAV file (default: output.wav)\n");
    printf("  --lang LANG           auto, en, zh, ja, ko (default: auto)\n");
    printf("  --instruct TEXT       voice instruction placed in front of the prompt (tokenised with the loaded vocab; combines with --ref)\n");
    printf("  --instruct-tokens IDS comma-separated text token ids of the instruction (for synthetic: models, like --tokens)\n");
    printf("  --save-codes FILE     with --tokens: write the utterance's codec frames, one frame per line (--continue-codes frames included)\n");
    printf("  --continue-codes FILE with --tokens: generate behind the recorded frames of FILE (as --save-codes writes them); the WAV holds the new audio only\n");
    printf("  --ref PATH            reference audio for voice clone (WAV; resampled to 24 kHz, ECAPA speaker encoder on the GPU)\n");
    printf("  --ref-text TEXT       with --ref: in-context clone instead — the reference is encoded to codes and continued, TEXT is what it says\n");
    printf("  --ref-tokens IDS      the same with the reference text as comma-separated token ids (for synthetic: models, with --tokens)\n");
    printf("                        (--encode and --ref with --ref-text / --ref-tokens also read G.711 WAVs, mu-law or A-law, 8 bits mono: their bytes go through an encoder stream as they are)\n");
    printf("  --encode PATH         encode a WAV to codec frames with the audio encoder and write them to --save-codes FILE; nothing is synthesized\n");
    printf("  --encode-chunk MS     with --encode: push the file MS milliseconds at a time through one encoder stream (the stream runs at the file's own rate: the same codes; files over 60 s encode)\n");
    printf("  --temp FLOAT          temperature (default: 0.8; 0 samples at T=1 like the reference, use --top-k 1 for greedy)\n");
    printf("  --top-k N             top-k (default: 50)\n  --top-p FLOAT         top-p (default: 0.95)\n");
    printf("  --rep-penalty FLOAT   repetition penalty on the first codebook's ids (default: 1.0 = off; not a flag of the reference CLI)\n");
    printf("  --max-tokens N        max codec frames (default: 2048)\n  --seed N              sampling seed (default: 0)\n");
    printf("  --stream-chunk N      with --tokens: decode audio every N frames while generating (same samples as the one-shot decode);\n");
    printf("                        combines with --continue-codes and with --ref + --ref-text / --ref-tokens (the prefix is history, never decoded)\n");
    printf("  --out-rate R          write the WAV at R Hz (4000 .. 192000; default 24000): band-limited resampling on the GPU, in the stream's sink with --stream-chunk\n");
    printf("  --out-format F        sample format of the WAV: pcm16 (default), mulaw or alaw (G.711, 8 bits: WAV format tags 7 / 6), encoded on the GPU in the sink; composes with --out-rate (a telephone line: --out-rate 8000), --stream-chunk and the stage flags\n");
    printf("  --speed X             speaking rate (0.5 .. 2.0; default 1.0): X times as fast at the same pitch, WSOLA time stretch on the GPU; composes with --out-rate and --stream-chunk\n");
    printf("  --pitch ST            pitch shift in semitones (-12 .. +12; default 0): the fundamental moves, the formants stay, TD-PSOLA on the GPU ahead of --speed; composes with --speed, --gain, --limit and --out-rate\n");
    printf("  --eq SPEC             tone: a preset (telephone, rumble, presence, warm; unheard and untuned) or up to 8 sections kind:Hz[:dB]:Q separated by commas, kind one of hp, lp, ls, hs, peak, e.g. hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707; biquads in double on the GPU behind --speed and ahead of --loudness; no latency; composes with every stage flag, --out-rate and --out-format\n");
    printf("  --loudness LUFS       programme loudness to aim for (-40 .. -5; default: none): a BS.1770 meter and a gain that follows it by at most 1 dB per 100 ms, on the GPU behind --speed and ahead of --gain / --limit; 100 ms latency; composes with --pitch, --speed, --gain, --limit and --out-rate\n");
    printf("  --loudness-range DB   with --loudness: the largest boost or cut (0 .. 40; default 20)\n");
    printf("  --gain DB             output gain in decibels (-60 .. +40, rounded to 0.1 dB; default 0), applied on the GPU behind --speed and ahead of --out-rate\n");
    printf("  --limit X             look-ahead limiter behind the gain: no sample leaves the stage above X (0.001 .. 1.0, rounded to 0.001; default: none), 5.3 ms look-ahead\n");
    printf("  --feed K              with --stream-chunk: hand the text to the engine K tokens at a time while it generates (live text; same codes, and with --save-codes the same samples as without --feed)\n  -h, --help\n");
}

// a WAV file as mono float at its own rate for --encode-chunk: the encoder stream is opened at that rate and resamples on the GPU as
// plain --encode does, so a file of any rate gives both the same codes
static bool read_wav_mono(const std::string& path, std::vector<float>& pcm, int32_t& rate) {
    int64_t n = 0;
    if (q3tts_read_wav_host(path.c_str(), nullptr, 0, &n, &rate) != 0 || n < 1) return false;
    pcm.resize((size_t)n);
    return q3tts_read_wav_host(path.c_str(), pcm.data(), n, &n, &rate) == 0;
}

// a G.711 WAV (which read_wav_mono refuses) as its bytes: 0, or -1 when it is none either, or -2 (said on stderr) when it is stereo
static int read_wav_g711_file(const std::string& path, std::vector<uint8_t>& bytes, int32_t& rate, int& format) {
    int64_t n = 0;
    const int rc = q3tts_read_wav_g711_host(path.c_str(), nullptr, 0, &n, &rate, &format);
    if (rc == -2) fprintf(stderr, "Error: %s is a stereo G.711 file: only mono G.711 is read\n", path.c_str());
    if (rc != 0 || n < 1) return rc != 0 ? rc : -1;
    bytes.resize((size_t)n);
    return q3tts_read_wav_g711_host(path.c_str(), bytes.data(), n, &n, &rate, &format) == 0 ? 0 : -1;
}

// the bytes of a G.711 file through one encoder stream opened at the file's rate and format, `step` samples per push (0: whole-file
// pushes of at most the 60 s a push holds); empty on error
static std::vector<int64_t> encode_g711(TTSEngine& engine, const std::vector<uint8_t>& bytes, int32_t rate, int format, size_t step) {
    std::vector<int64_t> codes;
    const int id = engine.audio_stream_begin_encoded((int64_t)bytes.size(), rate, format);
    if (id < 0) return codes;
    const size_t most = (size_t)60 * (size_t)rate;
    step = step == 0 ? most : std::min(step, most);
    bool ok = true;
    for (size_t i = 0; ok && i < bytes.size(); i += step) {
        const size_t m = std::min(step, bytes.size() - i);
        const std::vector<int64_t> part = engine.audio_stream_push(id, bytes.data() + i, m, i + m == bytes.size(), &ok);
        codes.insert(codes.end(), part.begin(), part.end());
    }
    engine.audio_stream_end(id);
    if (!ok) codes.clear();
    return codes;
}

// one frame per line, the same number of integers on every line (blanks or commas between them); false with a message on stderr
static bool read_codes_file(const std::string& path, std::vector<int64_t>& codes, size_t& per_frame) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { fprintf(stderr, "Error: cannot read codes file: %s\n", path.c_str()); return false; }
    std::string line;
    per_frame = 0;
    int lineno = 0, ch = 0;
    while (ch != EOF) {
        line.clear();
        while ((ch = fgetc(f)) != EOF && ch != '\n') line.push_back((char)ch);
        ++lineno;
        size_t n = 0;
        const char* q = line.c_str();
        for (;;) {
            while (*q == ' ' || *q == '\t' || *q == ',' || *q == '\r') ++q;
            if (!*q) break;
            char* end = nullptr;
            const long long v = strtoll(q, &end, 10);
            if (end == q) { fprintf(stderr, "Error: %s line %d: not an integer: %s\n", path.c_str(), lineno, q); fclose(f); return false; }
            codes.push_back((int64_t)v);
            ++n;
            q = end;
        }
        if (n == 0) continue;
        if (per_frame == 0) per_frame = n;
        else if (n != per_frame) { fprintf(stderr, "Error: %s line %d: %zu codes, the lines before have %zu\n", path.c_str(), lineno, n, per_frame); fclose(f); return false; }
    }
    fclose(f);
    return true;
}

static bool write_codes_file(const std::string& path, const std::vector<int64_t>& codes, size_t per_frame) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) return false;
    for (size_t i = 0; i < codes.size(); ++i) fprintf(f, "%lld%c", (long long)codes[i], (i + 1) % per_frame == 0 ? '\n' : ' ');
    return fclose(f) == 0;
}

static Language lang_of(const std::string& s) {
    if (s == "en" || s == "english") return Language::English;
    if (s == "zh" || s == "chinese") return Language::Chinese;
    if (s == "ja" || s == "japanese") return Language::Japanese;
    if (s == "ko" || s == "korean") return Language::Korean;
    return Language::Auto;
}

// -p TEXT as --tokens frames its ids: IM_START ASSISTANT TTS_BOS <ids of the tokenizer> TTS_EOS IM_END; false with a message on stderr
static bool frame_prompt(const TTSEngine& engine, const std::string& prompt, std::vector<int64_t>& ids) {
    const std::vector<int32_t> t = engine.tokenize(prompt);
    if (t.empty()) { fprintf(stderr, "Error: the text has no tokens (-p needs vocab.json + merges.txt)\n"); return false; }
    ids = { config::IM_START, config::ASSISTANT, config::TTS_BOS };
    ids.insert(ids.end(), t.begin(), t.end());
    ids.push_back(config::TTS_EOS);
    ids.push_back(config::IM_END);
    return true;
}

int main(int argc, char** argv) {
    std::string model, prompt, tokens, output = "output.wav", lang = "auto", ref, instruct, instruct_tokens, save_codes, continue_codes, encode, ref_text, ref_tokens, out_format = "pcm16";
    bool have_prompt = false;
    SamplingParams sp;
    uint64_t seed = 0;
    int stream_chunk = 0, feed = 0, encode_chunk = 0, out_rate = config::SAMPLE_RATE;
    bool have_encode_chunk = false;
    double speed = 1.0, gain_db = 0.0, limit = 0.0, pitch_st = 0.0, loudness = 0.0, loudness_range = 20.0;
    bool have_loudness = false;
    std::string eq;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;
        if (a == "-h" || a == "--help") { usage(argv[0]); return 0; }
        else if ((a == "-m" || a == "--model") && more) model = argv[++i];
        else if ((a == "-p" || a == "--prompt") && more) { prompt = argv[++i]; have_prompt = true; }
        else if (a == "--tokens" && more) tokens = argv[++i];
        else if ((a == "-o" || a == "--output") && more) output = argv[++i];
        else if (a == "--lang" && more) lang = argv[++i];
        else if (a == "--ref" && more) ref = argv[++i];
        else if (a == "--ref-text" && more) ref_text = argv[++i];
        else if (a == "--ref-tokens" && more) ref_tokens = argv[++i];
        else if (a == "--encode" && more) encode = argv[++i];
        else if (a == "--encode-chunk" && more) { encode_chunk = atoi(argv[++i]); have_encode_chunk = true; }
        else if (a == "--instruct" && more) instruct = argv[++i];
        else if (a == "--instruct-tokens" && more) instruct_tokens = argv[++i];
        else if (a == "--save-codes" && more) save_codes = argv[++i];
        else if (a == "--continue-codes" && more) continue_codes = argv[++i];
        else if (a == "--temp" && more) sp.temperature = (float)atof(argv[++i]);
        else if (a == "--top-k" && more) sp.top_k = atoi(argv[++i]);
        else if (a == "--top-p" && more) sp.top_p = (float)atof(argv[++i]);
        else if (a == "--rep-penalty" && more) sp.repetition_penalty = (float)atof(argv[++i]);
        else if (a == "--max-tokens" && more) sp.max_new_tokens = atoi(argv[++i]);
        else if (a == "--seed" && more) seed = strtoull(argv[++i], nullptr, 10);
        else if (a == "--stream-chunk" && more) stream_chunk = atoi(argv[++i]);
        else if (a == "--feed" && more) feed = atoi(argv[++i]);
        else if (a == "--out-rate" && more) out_rate = atoi(argv[++i]);
        else if (a == "--out-format" && more) out_format = argv[++i];
        else if (a == "--speed" && more) speed = atof(argv[++i]);
        else if (a == "--pitch" && more) pitch_st = atof(argv[++i]);
        else if (a == "--eq" && more) eq = argv[++i];
        else if (a == "--loudness" && more) { loudness = atof(argv[++i]); have_loudness = true; }
        else if (a == "--loudness-range" && more) loudness_range = atof(argv[++i]);
        else if (a == "--gain" && more) gain_db = atof(argv[++i]);
        else if (a == "--limit" && more) limit = atof(argv[++i]);
    }
    const bool icl = !ref_text.empty() || !ref_tokens.empty();
    if (out_format != "pcm16" && out_format != "mulaw" && out_format != "alaw") {
        fprintf(stderr, "Error: --out-format %s is none of pcm16, mulaw, alaw\n", out_format.c_str());
        return 1;
    }
    const int out_g711 = out_format == "mulaw" ? Q3TTS_PCM_MULAW : (out_format == "alaw" ? Q3TTS_PCM_ALAW : 0);   // 0: pcm16
    if (have_encode_chunk && (encode.empty() || encode_chunk < 1)) {
        fprintf(stderr, "Error: --encode-chunk MS (MS >= 1) goes with --encode\nUsage: %s -m MODEL --encode WAV --encode-chunk MS --save-codes FILE\n", argv[0]);
        return 1;
    }
    if (!encode.empty()) {   // audio -> codes, nothing else
        if (model.empty() || save_codes.empty()) { fprintf(stderr, "Error: --encode needs --model and --save-codes FILE\n"); return 1; }
        TTSEngine enc_engine(model, true);
        if (!enc_engine.is_ready()) { fprintf(stderr, "Error: %s\n", enc_engine.get_error().c_str()); return 1; }
        if (!enc_engine.has_audio_encoder()) { fprintf(stderr, "Error: model has no audio encoder\n"); return 1; }
        std::vector<int64_t> codes;
        std::vector<float> pcm; int32_t rate = 0;
        std::vector<uint8_t> g711; int g711_format = 0;
        if (!read_wav_mono(encode, pcm, rate) || pcm.empty()) {   // not a file the reader takes: a G.711 file goes through a stream of its own format
            pcm.clear();
            const int rc = read_wav_g711_file(encode, g711, rate, g711_format);
            if (rc == -2) return 1;
            if (rc != 0) g711.clear();
        }
        if (!g711.empty()) {
            codes = encode_g711(enc_engine, g711, rate, g711_format, have_encode_chunk ? std::max<size_t>((size_t)((int64_t)encode_chunk * rate / 1000), 1) : 0);
        } else if (have_encode_chunk) {   // the file through one encoder stream sized to it, encode_chunk ms per push
            if (pcm.empty()) { fprintf(stderr, "Error: failed to read %s\n", encode.c_str()); return 1; }
            const int id = enc_engine.audio_stream_begin((int64_t)pcm.size(), rate);
            if (id < 0) { fprintf(stderr, "Error: encoding failed\n"); return 1; }
            // encode_chunk ms of the file's own samples, at least one, at most the 60 s a push holds
            const size_t step = std::min<size_t>(std::max<size_t>((size_t)((int64_t)encode_chunk * rate / 1000), 1), (size_t)60 * (size_t)rate);
            bool ok = true;
            for (size_t i = 0; ok && i < pcm.size(); i += step) {
                const size_t m = std::min(step, pcm.size() - i);
                const std::vector<int64_t> part = enc_engine.audio_stream_push(id, pcm.data() + i, m, i + m == pcm.size(), &ok);
                codes.insert(codes.end(), part.begin(), part.end());
            }
            enc_engine.audio_stream_end(id);
            if (!ok) codes.clear();
        } else codes = enc_engine.encode_audio(encode);
        if (codes.empty()) { fprintf(stderr, "Error: encoding failed\n"); return 1; }
        if (!write_codes_file(save_codes, codes, (size_t)enc_engine.n_groups())) { fprintf(stderr, "Error: failed to write %s\n", save_codes.c_str()); return 1; }
        printf("Encoded %zu frames\nCodes saved to: %s\n", codes.size() / (size_t)enc_engine.n_groups(), save_codes.c_str());
        return 0;
    }
    if (icl && (ref.empty() || !instruct.empty() || !instruct_tokens.empty() || !continue_codes.empty() || (!ref_tokens.empty() && tokens.empty()))) {
        fprintf(stderr, "Error: --ref-text / --ref-tokens go with --ref (without --instruct, --continue-codes; --ref-tokens with --tokens)\n");
        return 1;
    }
    if (model.empty() || (!have_prompt && tokens.empty())) {
        fprintf(stderr, "Error: --model and --prompt (or --tokens) are required\n");
        usage(argv[0]);
        return 1;
    }
    if (feed != 0 && (feed < 1 || stream_chunk < 1 || !ref.empty() || !instruct.empty() || !instruct_tokens.empty() || !continue_codes.empty())) {
        fprintf(stderr, "Error: --feed K (K >= 1) needs --stream-chunk (without --ref, --instruct, --continue-codes)\n");
        return 1;
    }
    std::vector<int64_t> prefix;
    size_t prefix_groups = 0;
    if (!save_codes.empty() || !continue_codes.empty()) {
        if (tokens.empty() || (!ref.empty() && !icl) || !instruct.empty() || !instruct_tokens.empty()) {
            fprintf(stderr, "Error: --save-codes / --continue-codes go with --tokens (without --instruct, and without --ref unless --ref-text / --ref-tokens make it an in-context clone)\n");
            return 1;
        }
        if (!continue_codes.empty()) {
            if (!read_codes_file(continue_codes, prefix, prefix_groups)) return 1;
            printf("Continue from: %s (%zu frames of %zu codes)\n", continue_codes.c_str(), prefix_groups ? prefix.size() / prefix_groups : 0, prefix_groups);
        }
    }
    struct stat stbuf;
    if (model.rfind("synthetic:", 0) != 0 && model.rfind("synthetic-1.7b:", 0) != 0 && stat(model.c_str(), &stbuf) != 0) {
        fprintf(stderr, "Error: model directory not found: %s\n", model.c_str());
        return 1;
    }
    printf("Model: %s\n", model.c_str());
    if (have_prompt) printf("Text: %s\n", prompt.c_str());
    if (!ref.empty()) printf("Reference: %s\n", ref.c_str());
    printf("Language: %s\nOutput: %s\n\n", lang.c_str(), output.c_str());

    if (!eq.empty()) {   // a spec that cannot be read is refused before the model is loaded
        q3tts_tone_section sections[Q3TTS_TONE_MAX_SECTIONS]; int32_t n_sections = 0;
        if (q3tts_tone_parse(eq.c_str(), sections, &n_sections) != 0) { fprintf(stderr, "Error: --eq %s: %s\n", eq.c_str(), q3tts_tone_last_error()); return 1; }
    }
    TTSEngine engine(model, icl);
    if (!engine.is_ready()) { fprintf(stderr, "Error: %s\n", engine.get_error().c_str()); return 1; }
    engine.set_seed(seed);
    // --out-rate: the engine delivers int16 at that rate (the streaming paths through their sink, whole clips through convert_output
    // below); 24000 leaves everything as it is.  --out-format mulaw / alaw: the sink delivers G.711 bytes instead, at 24000 too (the
    // format-only sink).  The chunks' samples are collected in audio16 / audio8.
    const bool resample_out = out_rate != config::SAMPLE_RATE;
    const bool sink_out = resample_out || out_g711 != 0;
    if (sink_out && !engine.set_output_encoding(out_rate, out_g711 ? out_g711 : Q3TTS_PCM_S16)) {
        if (resample_out) fprintf(stderr, "Error: --out-rate %d: %s\n", out_rate, engine.get_error().c_str());
        else fprintf(stderr, "Error: --out-format %s: %s\n", out_format.c_str(), engine.get_error().c_str());
        return 1;
    }
    // --speed: S = round(1000 X) permille; 1000 is no stage (the bytes written without the flag)
    const long speed_permille = std::lround(1000.0 * speed);
    if (!(speed == speed) || speed_permille < 500 || speed_permille > 2000) { fprintf(stderr, "Error: --speed %g is outside 0.5 .. 2.0\n", speed); return 1; }
    const bool sped = speed_permille != 1000;
    if (sped && !engine.set_speed((float)speed)) { fprintf(stderr, "Error: --speed %g: %s\n", speed, engine.get_error().c_str()); return 1; }
    // --pitch: r = round(1000 2^(ST / 12)) permille; 0 semitones is no stage (the bytes written without the flag)
    if (!(pitch_st == pitch_st) || pitch_st < -12.0 || pitch_st > 12.0) { fprintf(stderr, "Error: --pitch %g is outside -12 .. +12\n", pitch_st); return 1; }
    if (pitch_st != 0.0 && !engine.set_pitch((float)pitch_st)) { fprintf(stderr, "Error: --pitch %g: %s\n", pitch_st, engine.get_error().c_str()); return 1; }
    // --eq: a preset or sections; without the flag there is no stage (the bytes written before)
    if (!eq.empty() && !engine.set_tone(eq.c_str())) { fprintf(stderr, "Error: --eq %s: %s\n", eq.c_str(), engine.get_error().c_str()); return 1; }
    // --loudness / --loudness-range: tenths of a LUFS and centibels; without the flag there is no stage (the bytes written before)
    if (have_loudness && !engine.set_loudness((float)loudness, (float)loudness_range)) {
        fprintf(stderr, "Error: --loudness %g --loudness-range %g: %s\n", loudness, loudness_range, engine.get_error().c_str());
        return 1;
    }
    // --gain / --limit: centibels and permille; neither given is no stage (the bytes written without the flags)
    if ((gain_db != 0.0 || limit != 0.0) && !engine.set_level((float)gain_db, (float)limit)) {
        fprintf(stderr, "Error: --gain %g --limit %g: %s\n", gain_db, limit, engine.get_error().c_str());
        return 1;
    }
    std::vector<int16_t> audio16;
    std::vector<uint8_t> audio8;
    printf("Synthesizing...\n");
    std::vector<float> audio;
    bool streamed16 = false;
    auto have_audio = [&]() { return !audio.empty() || !audio16.empty() || !audio8.empty(); };
    auto take = [&](const float* p, size_t n) {   // a streaming chunk: float at 24 kHz, or the sink's int16 / G.711 bytes behind the same pointer
        if (!sink_out) { audio.insert(audio.end(), p, p + n); return; }
        if (out_g711) {
            const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
            audio8.insert(audio8.end(), q, q + n);
        } else {
            const int16_t* q = reinterpret_cast<const int16_t*>(p);
            audio16.insert(audio16.end(), q, q + n);
        }
        streamed16 = true;
    };
    // --ref with --ref-text / --ref-tokens: a G.711 reference (which the reader refuses) is encoded through a stream of its own format
    std::vector<int64_t> g711_ref_codes;
    if (icl) {
        int64_t probe = 0; int32_t rate = 0;
        if (q3tts_read_wav_host(ref.c_str(), nullptr, 0, &probe, &rate) != 0 || probe < 1) {
            std::vector<uint8_t> g711; int g711_format = 0;
            const int rc = read_wav_g711_file(ref, g711, rate, g711_format);
            if (rc == -2) return 1;
            if (rc == 0 && !g711.empty()) {
                if (!engine.has_audio_encoder()) { fprintf(stderr, "Error: model has no audio encoder\n"); return 1; }
                g711_ref_codes = encode_g711(engine, g711, rate, g711_format, 0);
                if (g711_ref_codes.empty()) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
            }
        }
    }
    if (!ref.empty() && !icl) {
        if (!engine.has_speaker_encoder()) { fprintf(stderr, "Error: speaker encoder not available for voice clone\n"); return 1; }
    }
    std::vector<int64_t> ids;
    if (!tokens.empty()) {
        ids = { config::IM_START, config::ASSISTANT, config::TTS_BOS };
        for (char* tok = strtok(&tokens[0], ", "); tok; tok = strtok(nullptr, ", ")) ids.push_back(strtoll(tok, nullptr, 10));
        ids.push_back(config::TTS_EOS);
        ids.push_back(config::IM_END);
    }
    if (icl) {   // in-context clone: the reference's codes (audio encoder) and text in front of the utterance
        if (!engine.has_audio_encoder()) { fprintf(stderr, "Error: model has no audio encoder\n"); return 1; }
        std::vector<int64_t> rids;
        if (!ref_tokens.empty())
            for (char* tok = strtok(&ref_tokens[0], ", "); tok; tok = strtok(nullptr, ", ")) rids.push_back(strtoll(tok, nullptr, 10));
        else for (int32_t t : engine.tokenize(ref_text)) rids.push_back(t);
        if (rids.empty()) { fprintf(stderr, "Error: the reference text has no tokens (--ref-text needs vocab.json + merges.txt)\n"); return 1; }
        if (ids.empty() && !frame_prompt(engine, prompt, ids)) return 1;   // -p: the framing of --tokens around the tokenised text
        std::vector<int64_t> all;
        if (stream_chunk > 0) {   // the same clone delivered in chunks: encode, frame the ids as synthesize_clone_icl does, continue behind the codes
            const std::vector<int64_t> ref_codes = g711_ref_codes.empty() ? engine.encode_audio(ref) : g711_ref_codes;
            if (ref_codes.empty() || ids.size() < 3) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
            std::vector<int64_t> tids(ids.begin(), ids.begin() + 3);
            tids.insert(tids.end(), rids.begin(), rids.end());
            tids.insert(tids.end(), ids.begin() + 3, ids.end());
            size_t chunks = 0;
            const int nf = engine.synthesize_tokens_continue_streaming(tids, ref_codes, lang_of(lang), sp, stream_chunk, [&](const float* p, size_t n, bool) {
                if (n > 0 && chunks++ == 0) printf("First %.2f seconds of audio ready\n", (float)n / out_rate);
                take(p, n);
                return false;
            }, &all);
            if (nf < 0) { audio.clear(); audio16.clear(); audio8.clear(); }
            else printf("Streamed %d new frames in %zu chunks\n", nf - (int)(ref_codes.size() / (size_t)engine.n_groups()), chunks);
        } else if (!g711_ref_codes.empty() && ids.size() >= 3) {   // what synthesize_clone_icl does behind its own encode
            std::vector<int64_t> tids(ids.begin(), ids.begin() + 3);
            tids.insert(tids.end(), rids.begin(), rids.end());
            tids.insert(tids.end(), ids.begin() + 3, ids.end());
            audio = engine.synthesize_tokens_continue(tids, g711_ref_codes, lang_of(lang), sp, &all);
        } else audio = engine.synthesize_clone_icl(ids, rids, ref, lang_of(lang), sp, &all);
        const size_t G = (size_t)engine.n_groups();
        if (have_audio()) printf("In-context clone: %zu reference text tokens, %zu frames in all\n", rids.size(), all.size() / G);
        if (have_audio() && !save_codes.empty()) {
            if (!write_codes_file(save_codes, all, G)) { fprintf(stderr, "Error: failed to write %s\n", save_codes.c_str()); return 1; }
            printf("Codes saved to: %s\n", save_codes.c_str());
        }
    } else if (!instruct.empty() || !instruct_tokens.empty()) {   // a voice instruction in front of the prompt, with or without a cloned voice
        std::vector<int32_t> ins;
        if (!instruct_tokens.empty())
            for (char* tok = strtok(&instruct_tokens[0], ", "); tok; tok = strtok(nullptr, ", ")) ins.push_back((int32_t)strtol(tok, nullptr, 10));
        else ins = engine.tokenize(instruct);
        if (ins.empty()) { fprintf(stderr, "Error: the instruction has no tokens (--instruct needs vocab.json + merges.txt)\n"); return 1; }
        std::vector<float> spk;
        if (!ref.empty()) {
            spk = engine.extract_speaker_embedding(ref);
            if (spk.empty()) { fprintf(stderr, "[TTSEngine] Failed to extract speaker embedding\n"); return 1; }
        }
        printf("Instruction: %zu tokens\n", ins.size());
        if (!ids.empty()) audio = engine.synthesize_tokens_instruct(ids, ins, spk, lang_of(lang), sp);
        else if (!instruct_tokens.empty()) { fprintf(stderr, "Error: --instruct-tokens goes with --tokens\n"); return 1; }
        else audio = engine.synthesize_instruct(prompt, instruct, spk, lang_of(lang), sp);
    } else if (!ref.empty() && !ids.empty()) {
        const std::vector<float> spk = engine.extract_speaker_embedding(ref);
        if (spk.empty()) { fprintf(stderr, "[TTSEngine] Failed to extract speaker embedding\n"); }
        else audio = engine.synthesize_tokens_clone(ids, spk, lang_of(lang), sp);
    } else if (!ref.empty()) {
        audio = engine.synthesize_clone(prompt, ref, lang_of(lang), sp);
    } else if (stream_chunk > 0 && !continue_codes.empty()) {   // behind recorded frames, the new audio in chunks
        if (!prefix.empty() && prefix_groups != (size_t)engine.n_groups()) {
            fprintf(stderr, "Error: %s has %zu codes per frame, the model has %d\n", continue_codes.c_str(), prefix_groups, engine.n_groups());
            return 1;
        }
        std::vector<int64_t> all;
        size_t chunks = 0;
        const size_t G = (size_t)engine.n_groups();
        const int nf = engine.synthesize_tokens_continue_streaming(ids, prefix, lang_of(lang), sp, stream_chunk, [&](const float* p, size_t n, bool) {
            if (n > 0 && chunks++ == 0) printf("First %.2f seconds of audio ready\n", (float)n / out_rate);
            take(p, n);
            return false;
        }, &all);
        if (nf < 0) { audio.clear(); audio16.clear(); audio8.clear(); }
        else printf("Frames: %zu recorded + %zu new, streamed in %zu chunks\n", prefix.size() / G, all.size() / G - prefix.size() / G, chunks);
        if (have_audio() && !save_codes.empty()) {
            if (!write_codes_file(save_codes, all, G)) { fprintf(stderr, "Error: failed to write %s\n", save_codes.c_str()); return 1; }
            printf("Codes saved to: %s\n", save_codes.c_str());
        }
    } else if (stream_chunk > 0 && (feed > 0 || !save_codes.empty())) {
        // the batch scheduler's delivery for one utterance; --feed: its ids reach the engine K at a time, one piece per poll (live text)
        if (ids.empty() && !frame_prompt(engine, prompt, ids)) return 1;   // -p: the framing of --tokens around the tokenised text
        size_t chunks = 0, given = 0, polls = 0;
        auto on_audio = [&](int, const float* p, size_t n, bool) {
            if (n > 0 && chunks++ == 0) printf("First %.2f seconds of audio ready\n", (float)n / out_rate);
            take(p, n);
            return false;
        };
        std::vector<std::vector<int64_t>> codes;
        std::vector<int> nf;
        if (feed > 0) {
            nf = engine.synthesize_tokens_live(1, [&](int, std::vector<int64_t>& out, bool& closed) {
                const size_t m = std::min((size_t)feed, ids.size() - given);
                out.insert(out.end(), ids.begin() + (std::ptrdiff_t)given, ids.begin() + (std::ptrdiff_t)(given + m));
                given += m; ++polls;
                closed = given == ids.size();
                return true;
            }, lang_of(lang), sp, stream_chunk, on_audio, save_codes.empty() ? nullptr : &codes);
        } else nf = engine.synthesize_tokens_batch_streaming({ ids }, lang_of(lang), sp, stream_chunk, on_audio, &codes);
        if (nf.empty()) { audio.clear(); audio16.clear(); audio8.clear(); }
        else {
            printf("Streamed %d frames in %zu chunks\n", nf[0], chunks);
            if (feed > 0) printf("Text fed in %zu pieces of up to %d tokens\n", polls, feed);
        }
        if (!nf.empty() && !save_codes.empty()) {
            if (!write_codes_file(save_codes, codes[0], (size_t)engine.n_groups())) { fprintf(stderr, "Error: failed to write %s\n", save_codes.c_str()); return 1; }
            printf("Codes saved to: %s\n", save_codes.c_str());
        }
    } else if (!ids.empty() && stream_chunk > 0 && resample_out) {   // the same through the scheduler, whose streams carry the sink
        size_t chunks = 0;
        const std::vector<int> nf = engine.synthesize_tokens_batch_streaming({ ids }, lang_of(lang), sp, stream_chunk, [&](int, const float* p, size_t n, bool) {
            if (n > 0 && chunks++ == 0) printf("First %.2f seconds of audio ready\n", (float)n / out_rate);
            take(p, n);
            return false;
        });
        if (nf.empty()) { audio16.clear(); audio8.clear(); }
        else printf("Streamed %d frames in %zu chunks of %d frames\n", nf[0], chunks, stream_chunk);
    } else if (!ids.empty() && stream_chunk > 0) {   // chunks of audio as their frames are generated; the file holds their concatenation
        size_t chunks = 0;
        const int nf = engine.synthesize_tokens_streaming(ids, lang_of(lang), sp, stream_chunk, -1, [&](const float* p, size_t n) {
            if (chunks++ == 0) printf("First %.2f seconds of audio ready\n", (float)n / out_rate);
            audio.insert(audio.end(), p, p + n);   // 24 kHz float whatever the output format (here the rate is 24000): converted below
        });
        if (nf < 0) { audio.clear(); audio16.clear(); }
        else printf("Streamed %d frames in %zu chunks\n", nf, chunks);
    } else if (!ids.empty() && (!save_codes.empty() || !continue_codes.empty())) {
        if (!prefix.empty() && prefix_groups != (size_t)engine.n_groups()) {
            fprintf(stderr, "Error: %s has %zu codes per frame, the model has %d\n", continue_codes.c_str(), prefix_groups, engine.n_groups());
            return 1;
        }
        std::vector<int64_t> all;
        audio = engine.synthesize_tokens_continue(ids, prefix, lang_of(lang), sp, &all);
        const size_t G = (size_t)engine.n_groups();
        if (have_audio()) printf("Frames: %zu recorded + %zu new\n", prefix.size() / G, all.size() / G - prefix.size() / G);
        if (have_audio() && !save_codes.empty()) {
            if (!write_codes_file(save_codes, all, G)) { fprintf(stderr, "Error: failed to write %s\n", save_codes.c_str()); return 1; }
            printf("Codes saved to: %s\n", save_codes.c_str());
        }
    } else if (!ids.empty()) {
        audio = engine.synthesize_tokens(ids, lang_of(lang), sp);
    } else audio = engine.synthesize(prompt, lang_of(lang), sp);
    if (sink_out) {
        if (!streamed16) {   // a whole clip at 24 kHz: one push + finish through the resampler the streams use
            if (audio.empty()) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
            if (!engine.convert_output(audio, nullptr, &audio16, &audio8)) { fprintf(stderr, "Error: %s conversion failed\n", resample_out ? "--out-rate" : "--out-format"); return 1; }
        }
        if (out_g711) {
            if (audio8.empty()) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
            printf("Generated %.2f seconds of audio\n", (float)audio8.size() / out_rate);
            if (save_wav_g711(output.c_str(), audio8, (uint32_t)out_rate, out_g711) != 0) { fprintf(stderr, "Error: failed to write WAV\n"); return 1; }
            printf("Saved to: %s\n", output.c_str());
            return 0;
        }
        if (audio16.empty()) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
        printf("Generated %.2f seconds of audio\n", (float)audio16.size() / out_rate);
        if (save_wav16_raw(output.c_str(), audio16, (uint32_t)out_rate) != 0) { fprintf(stderr, "Error: failed to write WAV\n"); return 1; }
        printf("Saved to: %s\n", output.c_str());
        return 0;
    }
    if (audio.empty()) { fprintf(stderr, "Error: synthesis failed\n"); return 1; }
    printf("Generated %.2f seconds of audio\n", (float)audio.size() / config::SAMPLE_RATE);
    if (save_wav16(output.c_str(), audio, config::SAMPLE_RATE) != 0) { fprintf(stderr, "Error: failed to write WAV\n"); return 1; }
    printf("Saved to: %s\n", output.c_str());
    return 0;
}
