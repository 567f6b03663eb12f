// q3_audio.h — reference-audio front end of the voice-clone path: RIFF/WAVE reader,
// linear resampler and the 128-bin log-mel extractor whose output feeds the speaker encoder.
// Behavioural contract = reference src/io/wav_reader.cpp:28-164 and src/io/mel.cpp:13-236 as driven by
// TTSEngine::extract_speaker_embedding (src/tts_onnx.cpp:331-365).  Host code: one clip per utterance,
// microseconds to milliseconds of work.
#ifndef Q3_AUDIO_H
#define Q3_AUDIO_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace q3 {

// mono float samples in [-1, 1); empty on any failure (as the reference).  *sample_rate is set on success.
std::vector<float> read_wav(const std::string& path, int* sample_rate);
// The bytes of a G.711 WAV (format tag 7 mu-law / 6 A-law, 8 bits, mono), which read_wav returns nothing for; *format is set to
// Q3TTS_PCM_MULAW (2) / Q3TTS_PCM_ALAW (3).  A G.711 file with more than one channel throws std::invalid_argument naming it; anything
// else (another tag, other bits, no file) gives an empty result.  read_wav itself is the reference's reader and stays as it is.
std::vector<uint8_t> read_wav_g711(const std::string& path, int* sample_rate, int* format);
std::vector<float> resample_linear(const std::vector<float>& audio, int src_rate, int dst_rate);
// resample_linear over audio that is still arriving: the number of output samples a stream at src_rate has emitted in all once it
// holds n_received samples.  finish: resample_linear's own length.  Otherwise the largest count whose every output i (a) has both
// taps inside the received samples unclamped, floor(i / ratio) + 1 <= n_received - 1, and (b) lies below
// (size_t)((double)n_received * ratio): whatever the final length n >= n_received, resample_linear produces it.  Monotone in
// n_received, never above the finished length of a longer clip; equal rates: n_received.  Host-only, pure.
int64_t resample_stream_emitted(int src_rate, int dst_rate, int64_t n_received, bool finish);
// the raw samples a stream keeps behind its last one for the outputs it holds back: ceil(src_rate / dst_rate) + 1
inline int resample_stream_carry(int src_rate, int dst_rate) { return (src_rate + dst_rate - 1) / dst_rate + 1; }

// ---- the output side: band-limited polyphase resampler from 24 kHz to a sink's rate ----
// Plan for sink rate R (kSinkMinRate .. kSinkMaxRate): g = gcd(R, 24000), L = R / g, M = 24000 / g; output j sits at input position
// j * M / L.  s = min(1, R / 24000), half-width H = 16 / s input samples, half = ceil(H), taps = 2 * half, cut-off f = 0.92 * s.
// Row p, tap t: d = (t - half + 1) - p / L; h = f sinc(f d) I0(10 sqrt(1 - (d / H)^2)) / I0(10) for |d| < H, else 0; each row is formed
// in double, divided by its own sum (DC gain exactly 1 per phase) and rounded to float.  R == 24000: L = M = 1, half = taps = 0, no
// table (pass-through).  sink_plan throws std::invalid_argument naming the rate when it is out of range or its table would exceed kSinkMaxTable floats.
constexpr int kSinkMinRate = 4000, kSinkMaxRate = 192000;
constexpr int64_t kSinkMaxTable = (int64_t)1 << 22;
struct SinkPlan { int rate = 24000, L = 1, M = 1, half = 0, taps = 0; std::vector<float> table; /* [L][taps] */ };
void sink_plan_dims(int rate, SinkPlan* plan);   // everything but the table (and the same refusals)
SinkPlan sink_plan(int rate);
// outputs a sink at `rate` has emitted in all after n_received samples at 24 kHz: unfinished max(0, ceil((n - half) L / M)) — exactly the
// outputs whose last tap kc + half <= n - 1 has arrived — finished ceil(n L / M).  rate 24000: n.  Pure integer arithmetic.
int64_t sink_emitted(const SinkPlan& dims, int64_t n_received, bool finished);
// input samples a sink carries from push to push: 2 * half + ceil(M / L)
inline int sink_carry(const SinkPlan& d) { return d.taps == 0 ? 0 : 2 * d.half + (d.M + d.L - 1) / d.L; }

// ---- speaking rate: WSOLA time stretch at 24 kHz (the arithmetic is fixed in include/q3tts.h) ----
// Frame length N, synthesis hop Hs, search tolerance D; speed S in permille (kSpeedMin .. kSpeedMax, 1000: no stage).  Analysis
// position a_m = floor(m Hs S / 1000).  Everything here is 64-bit integer arithmetic and independent of the offsets the search picks.
constexpr int kSpeedN = 720, kSpeedHs = 360, kSpeedD = 240;
constexpr int kSpeedMin = 500, kSpeedMax = 2000;
constexpr int kSpeedCarry = 2 * kSpeedD + kSpeedN + 2 * kSpeedHs;   // 1920: strict upper bound of the samples a stretcher carries
void speed_check(int speed);   // throws std::invalid_argument naming the speed when it is outside kSpeedMin .. kSpeedMax
inline int64_t speed_pos(int speed, int64_t m) { return m * kSpeedHs * speed / 1000; }
// frame m is ready once need(m) = max(a_m + D + N, a_{m-1} + D + Hs + N) samples have been received (second term for m >= 1)
inline int64_t speed_need(int speed, int64_t m) {
    const int64_t a = speed_pos(speed, m) + kSpeedD + kSpeedN;
    return m >= 1 ? std::max(a, speed_pos(speed, m - 1) + kSpeedD + kSpeedHs + kSpeedN) : a;
}
// frames a stretcher has completed after n_received samples: unfinished #{m : need(m) <= n}, finished ceil(ceil(1000 n / S) / Hs)
int64_t speed_frames(int speed, int64_t n_received, bool finished);
// outputs it has emitted in all: unfinished Hs * frames, finished ceil(1000 n / S)
int64_t speed_emitted(int speed, int64_t n_received, bool finished);
// the window w[i] = 0.5 - 0.5 cos(2 pi i / N), formed in double and rounded to float (kSpeedN entries)
std::vector<float> speed_window();

// ---- output level: gain and look-ahead limiter at 24 kHz (the arithmetic is fixed in include/q3tts.h) ----
// gain in centibels (kLevelGainMin .. kLevelGainMax), ceiling in permille (0: gain only; 1 .. 1000: limiter at T = (float)(ceiling /
// 1000.0)); (0, 0) is no stage.  Look-ahead window W = kLevelW samples; a limiter carries the last kLevelCarry = 2 W - 2 values of v.
constexpr int kLevelGainMin = -600, kLevelGainMax = 400, kLevelW = 128, kLevelCarry = 2 * kLevelW - 2;
void level_check(int gain_cb, int ceiling_permille);   // throws std::invalid_argument naming the value that is out of range
float level_gain(int gain_cb);                         // 10^(gain_cb / 200), formed in double and rounded to float
inline float level_ceiling(int ceiling_permille) { return (float)((double)ceiling_permille / 1000.0); }
// outputs a stage has emitted in all after n_received samples: gain only n; limiter unfinished max(0, n - (W - 1)), finished n
inline int64_t level_emitted(int ceiling_permille, int64_t n_received, bool finished) {
    return ceiling_permille == 0 || finished ? n_received : std::max<int64_t>(0, n_received - (kLevelW - 1));
}

// ---- pitch: TD-PSOLA shift of the fundamental at 24 kHz (the arithmetic is fixed in include/q3tts.h) ----
// Ratio r in permille (kPitchMin .. kPitchMax, 1000: no stage).  Periods kPitchPmin .. kPitchPmax, an unvoiced mark's kPitchPu, the
// search template's half-width kPitchW.  A search at mark a reads x[a - W, a + kPitchReach): lags Pmin - 1 .. Pmax + 1 of a 2 W window.
// A synthesis mark at t is placed once kPitchGate samples from t on have arrived (its analysis mark lies at most Pmax / 2 behind t);
// output k is final once every mark up to k + Pmax is placed, so kPitchLA = Pmax + kPitchGate - 1.  Synthesis positions carry
// kPitchFrac fraction bits.  The two constants most likely to want tuning on real voices are kPitchVoiced2 and kPitchOctave2
// (squared correlations: 0.5 and 0.9), used by k_psola and restated in tests/pitch_ref.py.
constexpr int kPitchMin = 500, kPitchMax = 2000;
constexpr int kPitchPmin = 48, kPitchPmax = 400, kPitchPu = 120, kPitchW = 240;
constexpr int kPitchLags = kPitchPmax - kPitchPmin + 3;                  // 355 scores: lags Pmin - 1 .. Pmax + 1
constexpr int kPitchReach = kPitchW + kPitchPmax + 1;                    // 641
constexpr int kPitchRegion = kPitchW + kPitchReach;                      // 881 samples of one search
constexpr int kPitchGate = kPitchPmax / 2 + kPitchReach;                 // 841
constexpr int kPitchLA = kPitchPmax + kPitchGate - 1;                    // 1240 samples, 51.7 ms
constexpr int kPitchFrac = 20;
constexpr float kPitchVoiced2 = 0.25f, kPitchOctave2 = 0.81f, kPitchFloor = 0.0625f;
constexpr int kPitchRing = 1024;                                         // the two output accumulators beyond the last emitted sample (at most kPitchLA - kPitchGate + kPitchPmax = 799 are live)
constexpr int kPitchCarry = 2560;                                        // input samples a stage carries (at most 2 Pmax + kPitchGate + 2 Pmax - 1 = 2440 can be read again)
constexpr int kPitchStateWords = 8;                                      // int64: a_cur, P_cur, v_cur, has_next, P_next, v_next, s, marks placed
constexpr int kPitchHalfFloats = kPitchCarry + 2 * kPitchRing + 2 * kPitchStateWords;   // one half of a stage's allocation
void pitch_check(int ratio);   // throws std::invalid_argument naming the ratio when it is outside kPitchMin .. kPitchMax
int pitch_ratio(double cents); // round(1000 * 2^(cents / 1200)), in double
// outputs a stage has emitted in all after n_received samples: unfinished max(0, n - kPitchLA), finished n.  Independent of every period.
inline int64_t pitch_emitted(int64_t n_received, bool finished) { return finished ? n_received : std::max<int64_t>(0, n_received - kPitchLA); }
// the windows: for P = Pmin .. Pmax the 2 P values 0.5 - 0.5 cos(pi m / P), formed in double and rounded to float, P after P
constexpr int pitch_window_offset(int P) { return P * (P - 1) - kPitchPmin * (kPitchPmin - 1); }
constexpr int kPitchWindowFloats = (kPitchPmax + 1) * kPitchPmax - kPitchPmin * (kPitchPmin - 1);   // 158 144
std::vector<float> pitch_windows();

// ---- loudness: BS.1770 meter and normaliser at 24 kHz (the arithmetic is fixed in include/q3tts.h) ----
// target in tenths of a LUFS (kLoudTargetMin .. kLoudTargetMax; 0: meter only), range in centibels (0 .. kLoudRangeMax), start gain in
// centibels (kLoudStartMin .. kLoudStartMax).  A sub-block is kLoudBlock samples (100 ms); four of them are the standard's 400 ms block.
// A window of four counts from kLoudGate on: floor(9600 2^32 10^((-70 + 0.691) / 10)); kLoudNorm = 9600 2^32 turns a window's integer
// energy into a mean square.  A stage's half: kLoudStateWords 8-byte words (six doubles of filter history x[k-1], x[k-2], u[k-1],
// u[k-2], v[k-1], v[k-2]; then int64 E_{b-1}, E_{b-2}, E_{b-3}, the open sub-block's sum, A, N; then G's bits) and kLoudBlock floats of
// input not yet emitted.
constexpr int kLoudTargetMin = -400, kLoudTargetMax = -50, kLoudRangeMax = 400, kLoudStartMin = -400, kLoudStartMax = 400;
constexpr int kLoudBlock = 2400;
constexpr int64_t kLoudGate = 4834272;
constexpr double kLoudNorm = 41231686041600.0;
constexpr float kLoudUp = (float)1.1220184543019633, kLoudDn = (float)0.8912509381337456;   // (float)10^(1/20), (float)10^(-1/20)
constexpr int kLoudStateWords = 16;
constexpr size_t kLoudHalfBytes = (size_t)kLoudStateWords * 8 + (size_t)kLoudBlock * sizeof(float);
void loudness_check(int target_dlufs, int range_cb, int start_cb);   // throws std::invalid_argument naming the value that is out of range
// the two biquads at `rate`: out = { b0, b1, b2, a1, a2 } of the shelf, then of the high-pass (the header's formulas, in double)
void loudness_coeffs(int rate, double out[10]);
// outputs a stage has emitted in all after n_received samples: meter only n; else unfinished kLoudBlock floor(n / kLoudBlock), finished n
inline int64_t loudness_emitted(int target_dlufs, int64_t n_received, bool finished) {
    return target_dlufs == 0 || finished ? n_received : kLoudBlock * (n_received / kLoudBlock);
}
// LUFS of n sub-block energies: mode 0 momentary (the last four), 1 short-term (the last thirty), 2 integrated (absolute gate, then the
// relative gate at -10 LU).  -inf when the span is not there or nothing passes the gates.
double loudness_lufs(const int64_t* E, int64_t n, int mode);

// ---- tone: a cascade of 1 .. kToneMaxSections biquads at 24 kHz (the arithmetic is fixed in include/q3tts.h) ----
// A section is { kind, freq_hz, gain_cb, q_permille }, all integers (q3tts_tone_section has the same layout).  The coefficients are the
// RBJ Audio-EQ-Cookbook forms in double, normalised by a0: w0 = 2 pi f / 24000, alpha = sin(w0) / (2 Q), A = 10^(gain_cb / 400).  A
// stage carries two doubles per signal (the input and each section's output): kToneStateDoubles per half at the most.  It emits what
// it receives: no latency, nothing held back, nothing flushed.
constexpr int kToneMaxSections = 8, kToneHighpass = 1, kToneLowpass = 2, kToneLowshelf = 3, kToneHighshelf = 4, kTonePeak = 5;
constexpr int kToneFreqMin = 20, kToneFreqMax = 11000, kToneGainMax = 240, kToneQMin = 100, kToneQMax = 10000;
constexpr int kToneStateDoubles = 2 * (kToneMaxSections + 1);
constexpr int kToneSegment = 2048;   // samples k_tone stages through LDS at a time (tests/test_gpu_tone.py reads it here to cut pushes around it)
struct ToneSection { int32_t kind, freq_hz, gain_cb, q_permille; };
// throws std::invalid_argument naming the field, the section's index and the value that is out of range (n outside 1 .. 8 as well)
void tone_check(int n, const ToneSection* sections);
// out[j] = { b0, b1, b2, a1, a2 } of section j at 24 kHz; the sections must have passed tone_check
void tone_coeffs(int n, const ToneSection* sections, double (*out)[5]);
// sections from a spec string: a preset's name (telephone, rumble, presence, warm) or comma-separated kind:Hz[:dB]:Q with kind one of
// hp, lp, ls, hs, peak (dB only, and always, for ls, hs and peak).  Throws std::invalid_argument naming what it could not read; the
// values are range-checked by tone_check.
std::vector<ToneSection> tone_parse(const std::string& spec);

struct MelSpec { // the settings of tts_onnx.cpp:347-354
    int sample_rate = 24000, n_fft = 1024, hop = 256, win = 1024, n_mels = 128;
    float fmin = 0.0f, fmax = 12000.0f;
};
// the tables of the extractor (window, FFT twiddles, bit reversal, triangle corners), computed once per MelSpec.  The GPU front end
// (k_logmel, q3_speaker_kernels.hip) uploads exactly these, so the two implementations cannot drift.
struct MelPlan {
    MelSpec spec;
    int n = 0, bins = 0;              // FFT length (power of two >= n_fft), kept bins
    std::vector<float> window;
    std::vector<float> tw_re, tw_im;  // exp(-2 pi i k / n), k < n/2
    std::vector<uint32_t> rev;
    std::vector<int> lo, mid, hi;     // triangle corners per mel band
};
MelPlan make_plan(const MelSpec& spec);
// log-mel, layout [n_mels][frames] like the reference's MelExtractor::extract; *frames receives the frame count
std::vector<float> log_mel(const std::vector<float>& audio, const MelSpec& spec, int* frames);

} // namespace q3
#endif
