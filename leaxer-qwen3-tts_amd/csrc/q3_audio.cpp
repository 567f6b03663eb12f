// q3_audio.cpp — see q3_audio.h.
#include "q3_audio.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace q3 {

// ---------------------------------------------------------------------------------------------
// RIFF/WAVE (reference wav_reader.cpp:28-143).  Chunks are walked in file order; "fmt " supplies
// format tag / channels / rate / bits, the LAST "data" chunk supplies the samples, everything else is
// skipped by its size (no pad-byte handling, as the reference).  A data chunk that runs past the end of
// the file is zero-filled to its declared size.  Accepted: PCM 8 (unsigned) / 16 / 24 / 32 bit and
// 32-bit IEEE float; channels are averaged.
// ---------------------------------------------------------------------------------------------
namespace {
struct File {
    FILE* f;
    explicit File(const char* p) : f(fopen(p, "rb")) {}
    ~File() { if (f) fclose(f); }
    bool get(void* dst, size_t n) { return fread(dst, 1, n, f) == n; }
};
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | p[1] << 8); }
} // namespace

std::vector<float> read_wav(const std::string& path, int* sample_rate) {
    File fl(path.c_str());
    if (!fl.f) return {};
    uint8_t hdr[12];
    if (!fl.get(hdr, 4) || memcmp(hdr, "RIFF", 4) != 0) return {};
    (void)fl.get(hdr + 4, 4); // RIFF size: not used
    if (!fl.get(hdr + 8, 4) || memcmp(hdr + 8, "WAVE", 4) != 0) return {};

    unsigned tag = 0, channels = 0, bits = 0;
    uint32_t rate = 0;
    std::vector<uint8_t> data;
    for (;;) {
        uint8_t ch[8];
        if (!fl.get(ch, 4) || !fl.get(ch + 4, 4)) break;
        const uint32_t size = le32(ch + 4);
        if (memcmp(ch, "fmt ", 4) == 0) {
            uint8_t fm[16] = { 0 };
            const size_t got = fread(fm, 1, 16, fl.f);
            // fields that were not read keep their previous value, like a sequence of unchecked freads
            if (got >= 2) tag = le16(fm);
            if (got >= 4) channels = le16(fm + 2);
            if (got >= 8) rate = le32(fm + 4);
            if (got >= 16) bits = le16(fm + 14);
            if (size > 16) fseek(fl.f, (long)(size - 16), SEEK_CUR);
        } else if (memcmp(ch, "data", 4) == 0) {
            try {
                data.assign((size_t)size, 0);
            } catch (...) { return {}; }
            if (size) (void)!fread(data.data(), 1, (size_t)size, fl.f);
        } else {
            fseek(fl.f, (long)size, SEEK_CUR);
        }
        if (feof(fl.f)) break;
    }
    if (tag != 1 && tag != 3) return {};
    if (!channels || !rate || !bits) return {};
    const size_t width = bits / 8;
    if (!width) return {};
    *sample_rate = (int)rate;

    const size_t n = data.size() / (channels * width);
    std::vector<float> out;
    out.reserve(n);
    const uint8_t* p = data.data();
    for (size_t i = 0; i < n; ++i) {
        float acc = 0.0f;
        for (unsigned c = 0; c < channels; ++c, p += width) {
            if (tag == 3) {
                if (bits == 32) { float v; memcpy(&v, p, 4); acc += v; }
            } else if (bits == 16) {
                acc += (float)(int16_t)le16(p) / 32768.0f;
            } else if (bits == 24) {
                int32_t v = (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
                if (v & 0x800000) v -= 0x1000000;
                acc += (float)v / 8388608.0f;
            } else if (bits == 32) {
                acc += (float)(int32_t)le32(p) / 2147483648.0f;
            } else if (bits == 8) {
                acc += (float)((int)p[0] - 128) / 128.0f;
            }
        }
        out.push_back(acc / (float)channels);
    }
    return out;
}

// G.711 WAVs (format tag 7 mu-law / 6 A-law, 8 bits, mono), which read_wav returns nothing for: the bytes as they lie, for an encoder
// stream of that format.  [HINT] no counterpart in the reference.  Chunks are walked with their pad bytes; the last "data" chunk
// supplies the bytes, cut where the file ends (a zero byte is not silence in either law).
std::vector<uint8_t> read_wav_g711(const std::string& path, int* sample_rate, int* format) {
    File fl(path.c_str());
    if (!fl.f) return {};
    uint8_t hdr[12];
    if (!fl.get(hdr, 12) || memcmp(hdr, "RIFF", 4) != 0 || memcmp(hdr + 8, "WAVE", 4) != 0) return {};
    unsigned tag = 0, channels = 0, bits = 0;
    uint32_t rate = 0;
    bool have_fmt = false;
    std::vector<uint8_t> data;
    for (;;) {
        uint8_t ch[8];
        if (!fl.get(ch, 8)) break;
        const uint32_t size = le32(ch + 4);
        if (memcmp(ch, "fmt ", 4) == 0) {
            uint8_t fm[16];
            if (size < 16 || !fl.get(fm, 16)) return {};
            tag = le16(fm); channels = le16(fm + 2); rate = le32(fm + 4); bits = le16(fm + 14);
            have_fmt = true;
            if (fseek(fl.f, (long)(size - 16) + (long)(size & 1), SEEK_CUR) != 0) break;
        } else if (memcmp(ch, "data", 4) == 0) {
            if (size > (uint32_t)1 << 30) return {};
            data.assign((size_t)size, 0);
            data.resize(size ? fread(data.data(), 1, (size_t)size, fl.f) : 0);
            if (size & 1) (void)fseek(fl.f, 1, SEEK_CUR);
        } else if (fseek(fl.f, (long)size + (long)(size & 1), SEEK_CUR) != 0) {
            break;
        }
    }
    if (!have_fmt || (tag != 6 && tag != 7) || bits != 8 || !rate || rate > 0x7FFFFFFFu) return {};
    if (channels != 1)
        throw std::invalid_argument("read_wav_g711: " + path + " has " + std::to_string(channels) + " channels: stereo G.711 is not read, only mono");
    *sample_rate = (int)rate;
    *format = tag == 7 ? 2 /* Q3TTS_PCM_MULAW */ : 3 /* Q3TTS_PCM_ALAW */;
    return data;
}

// ---------------------------------------------------------------------------------------------
// Linear-interpolation resampler (reference wav_reader.cpp:145-164): out[i] samples the input at
// i * src/dst, positions and weights in double, floor(n * dst/src) output samples, no anti-alias filter.
// ---------------------------------------------------------------------------------------------
std::vector<float> resample_linear(const std::vector<float>& a, int src_rate, int dst_rate) {
    if (src_rate == dst_rate || a.empty()) return a;
    const double ratio = (double)dst_rate / src_rate;
    const size_t n_out = (size_t)((double)a.size() * ratio);
    std::vector<float> out(n_out);
    const size_t last = a.size() - 1;
    for (size_t i = 0; i < n_out; ++i) {
        const double pos = (double)i / ratio;
        const size_t k = (size_t)pos;
        const double w = pos - (double)k;
        out[i] = (float)((double)a[k] * (1.0 - w) + (double)a[std::min(k + 1, last)] * w);
    }
    return out;
}

// The same resampler while the clip is still arriving (q3_audio.h).  Positions are resample_linear's own expression on absolute
// indices, (double)i / ratio, so the count agrees with what the one-shot reads; the estimate is corrected by stepping on that
// expression, never trusted.
int64_t resample_stream_emitted(int src_rate, int dst_rate, int64_t n, bool finish) {
    if (n <= 0 || src_rate < 1 || dst_rate < 1) return 0;
    if (src_rate == dst_rate) return n;
    const double ratio = (double)dst_rate / src_rate;
    const int64_t len = (int64_t)(size_t)((double)(size_t)n * ratio);   // resample_linear's n_out for a clip of n samples
    if (finish) return len;
    if (n < 2) return 0;
    auto tap = [&](int64_t i) { return (int64_t)(size_t)((double)(size_t)i / ratio); };   // output i reads samples tap(i) and tap(i) + 1
    int64_t e = (int64_t)((double)(n - 1) * ratio);            // about the first output whose upper tap has not arrived
    while (e > 0 && tap(e - 1) > n - 2) --e;
    while (tap(e) <= n - 2) ++e;
    return std::min(e, len);
}

// ---- sink plans (q3_audio.h) ----
static double bessel_i0(double x) {   // power series: converges fast for the |x| <= 10 used here
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}
void sink_plan_dims(int rate, SinkPlan* plan) {
    if (rate < kSinkMinRate || rate > kSinkMaxRate)
        throw std::invalid_argument("pcm sink: sample rate " + std::to_string(rate) + " is outside " + std::to_string(kSinkMinRate) + " .. " + std::to_string(kSinkMaxRate));
    SinkPlan d;
    d.rate = rate;
    if (rate != 24000) {
        int a = rate, b = 24000;
        while (b) { const int t = a % b; a = b; b = t; }
        d.L = rate / a; d.M = 24000 / a;
        // half = ceil(16 / s) = ceil(16 * 24000 / R) below 24 kHz, in integers
        d.half = rate >= 24000 ? 16 : (int)((16LL * 24000 + rate - 1) / rate);
        d.taps = 2 * d.half;
        if ((int64_t)d.L * d.taps > kSinkMaxTable)
            throw std::invalid_argument("pcm sink: sample rate " + std::to_string(rate) + " needs a table of " + std::to_string((int64_t)d.L * d.taps) + " floats (" +
                        std::to_string(d.L) + " phases x " + std::to_string(d.taps) + " taps), more than " + std::to_string(kSinkMaxTable));
    }
    *plan = d;
}
SinkPlan sink_plan(int rate) {
    SinkPlan d;
    sink_plan_dims(rate, &d);
    if (d.taps == 0) return d;
    const double pi = 3.14159265358979323846;
    const double s = rate >= 24000 ? 1.0 : (double)rate / 24000.0, H = 16.0 / s, f = 0.92 * s, i0b = bessel_i0(10.0);
    d.table.assign((size_t)d.L * d.taps, 0.f);
    std::vector<double> row((size_t)d.taps);
    for (int p = 0; p < d.L; ++p) {
        double sum = 0.0;
        for (int t = 0; t < d.taps; ++t) {
            const double x = (double)(t - d.half + 1) - (double)p / (double)d.L;
            double h = 0.0;
            if (std::fabs(x) < H) {
                const double fx = f * x, r = x / H;
                const double sinc = fx == 0.0 ? 1.0 : std::sin(pi * fx) / (pi * fx);
                h = f * sinc * bessel_i0(10.0 * std::sqrt(1.0 - r * r)) / i0b;
            }
            row[(size_t)t] = h;
            sum += h;
        }
        for (int t = 0; t < d.taps; ++t) d.table[(size_t)p * d.taps + t] = (float)(row[(size_t)t] / sum);
    }
    return d;
}
int64_t sink_emitted(const SinkPlan& d, int64_t n, bool finished) {
    if (n <= 0) return 0;
    if (d.taps == 0) return n;
    const int64_t m = finished ? n : n - d.half;
    if (m <= 0) return 0;
    return (m * d.L + d.M - 1) / d.M;
}

// ---- speaking rate (q3_audio.h) ----
void speed_check(int speed) {
    if (speed < kSpeedMin || speed > kSpeedMax)
        throw std::invalid_argument("speed: " + std::to_string(speed) + " permille is outside " + std::to_string(kSpeedMin) + " .. " + std::to_string(kSpeedMax));
}
int64_t speed_frames(int speed, int64_t n, bool finished) {
    if (n <= 0) return 0;
    if (finished) return ((n * 1000 + speed - 1) / speed + kSpeedHs - 1) / kSpeedHs;
    // need(m) <= a_m + Hs + D + N <= m Hs S / 1000 + Hs + D + N, so every m up to m0 is ready; need(m) >= a_m + D + N > m Hs S / 1000 - 1
    // + D + N, so the walk from m0 ends within 1000 / S + 2 steps
    const int64_t slack = n - (kSpeedHs + kSpeedD + kSpeedN);
    int64_t m = slack >= 0 ? slack * 1000 / ((int64_t)kSpeedHs * speed) : 0;
    if (speed_need(speed, m) > n) return 0;   // only m == 0 can come here
    while (speed_need(speed, m) <= n) ++m;
    return m;
}
int64_t speed_emitted(int speed, int64_t n, bool finished) {
    if (n <= 0) return 0;
    return finished ? (n * 1000 + speed - 1) / speed : kSpeedHs * speed_frames(speed, n, false);
}
std::vector<float> speed_window() {
    std::vector<float> w((size_t)kSpeedN);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < kSpeedN; ++i) w[(size_t)i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)kSpeedN));
    return w;
}

// ---- output level (q3_audio.h) ----
void level_check(int gain_cb, int ceiling) {
    if (gain_cb < kLevelGainMin || gain_cb > kLevelGainMax)
        throw std::invalid_argument("level: gain " + std::to_string(gain_cb) + " centibels is outside " + std::to_string(kLevelGainMin) + " .. " + std::to_string(kLevelGainMax));
    if (ceiling < 0 || ceiling > 1000)
        throw std::invalid_argument("level: ceiling " + std::to_string(ceiling) + " permille is outside 0 .. 1000");
}
float level_gain(int gain_cb) { return (float)std::pow(10.0, (double)gain_cb / 200.0); }

// ---- pitch (q3_audio.h) ----
void pitch_check(int ratio) {
    if (ratio < kPitchMin || ratio > kPitchMax)
        throw std::invalid_argument("pitch: " + std::to_string(ratio) + " permille is outside " + std::to_string(kPitchMin) + " .. " + std::to_string(kPitchMax));
}
int pitch_ratio(double cents) { return (int)std::llround(1000.0 * std::pow(2.0, cents / 1200.0)); }
std::vector<float> pitch_windows() {
    std::vector<float> w((size_t)kPitchWindowFloats);
    const double pi = 3.14159265358979323846;
    for (int P = kPitchPmin; P <= kPitchPmax; ++P)
        for (int m = 0; m < 2 * P; ++m) w[(size_t)(pitch_window_offset(P) + m)] = (float)(0.5 - 0.5 * std::cos(pi * (double)m / (double)P));
    return w;
}

// ---- loudness (q3_audio.h) ----
void loudness_check(int target, int range, int start) {
    if (target != 0 && (target < kLoudTargetMin || target > kLoudTargetMax))
        throw std::invalid_argument("loudness: target " + std::to_string(target) + " tenths of a LUFS is outside " + std::to_string(kLoudTargetMin) + " .. " + std::to_string(kLoudTargetMax) + " (0: meter only)");
    if (range < 0 || range > kLoudRangeMax)
        throw std::invalid_argument("loudness: range " + std::to_string(range) + " centibels is outside 0 .. " + std::to_string(kLoudRangeMax));
    if (start < kLoudStartMin || start > kLoudStartMax)
        throw std::invalid_argument("loudness: start gain " + std::to_string(start) + " centibels is outside " + std::to_string(kLoudStartMin) + " .. " + std::to_string(kLoudStartMax));
}
void loudness_coeffs(int rate, double out[10]) {
    const double pi = 3.14159265358979323846;
    {   // the shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double KQ = K / Q, K2 = K * K, a0 = 1.0 + KQ + K2;
        out[0] = (Vh + Vb * KQ + K2) / a0; out[1] = 2.0 * (K2 - Vh) / a0; out[2] = (Vh - Vb * KQ + K2) / a0;
        out[3] = 2.0 * (K2 - 1.0) / a0; out[4] = (1.0 - KQ + K2) / a0;
    }
    {   // the high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)rate);
        const double KQ = K / Q, K2 = K * K, a0 = 1.0 + KQ + K2;
        out[5] = 1.0; out[6] = -2.0; out[7] = 1.0;
        out[8] = 2.0 * (K2 - 1.0) / a0; out[9] = (1.0 - KQ + K2) / a0;
    }
}
double loudness_lufs(const int64_t* E, int64_t n, int mode) {
    const double ninf = -std::numeric_limits<double>::infinity();
    auto lufs = [&](double mean_square) { return mean_square > 0.0 ? -0.691 + 10.0 * std::log10(mean_square) : ninf; };
    if (mode == 0 || mode == 1) {   // the last 4 / 30 sub-blocks, ungated
        const int64_t span = mode == 0 ? 4 : 30;
        if (n < span) return ninf;
        double s = 0.0;
        for (int64_t b = n - span; b < n; ++b) s += (double)E[b];
        return lufs(s / ((double)span * (double)kLoudBlock * 4294967296.0));
    }
    // integrated: windows of four at 75 % overlap; the absolute gate; the relative gate 10 LU below the mean of what passed it
    double sum_abs = 0.0; int64_t n_abs = 0;
    for (int64_t b = 3; b < n; ++b) {
        const int64_t W = E[b - 3] + E[b - 2] + E[b - 1] + E[b];
        if (W >= kLoudGate) { sum_abs += (double)W / kLoudNorm; ++n_abs; }
    }
    if (n_abs == 0) return ninf;
    const double rel = 0.1 * (sum_abs / (double)n_abs);
    double sum_rel = 0.0; int64_t n_rel = 0;
    for (int64_t b = 3; b < n; ++b) {
        const int64_t W = E[b - 3] + E[b - 2] + E[b - 1] + E[b];
        const double z = (double)W / kLoudNorm;
        if (W >= kLoudGate && z > rel) { sum_rel += z; ++n_rel; }
    }
    return n_rel == 0 ? ninf : lufs(sum_rel / (double)n_rel);
}

// ---- tone (q3_audio.h) ----
static const char* const kToneFields[4] = { "kind", "freq_hz", "gain_cb", "q_permille" };
static std::invalid_argument tone_refusal(int j, int field, int64_t v, const std::string& why) {
    return std::invalid_argument("tone: section " + std::to_string(j) + " " + kToneFields[field] + " " + std::to_string(v) + " " + why);
}
void tone_check(int n, const ToneSection* s) {
    if (n < 1 || n > kToneMaxSections) throw std::invalid_argument("tone: " + std::to_string(n) + " sections is outside 1 .. " + std::to_string(kToneMaxSections));
    if (!s) throw std::invalid_argument("tone: NULL argument");
    for (int j = 0; j < n; ++j) {
        if (s[j].kind < kToneHighpass || s[j].kind > kTonePeak) throw tone_refusal(j, 0, s[j].kind, "is none of high-pass (1), low-pass (2), low shelf (3), high shelf (4), peak (5)");
        if (s[j].freq_hz < kToneFreqMin || s[j].freq_hz > kToneFreqMax) throw tone_refusal(j, 1, s[j].freq_hz, "Hz is outside " + std::to_string(kToneFreqMin) + " .. " + std::to_string(kToneFreqMax));
        if (s[j].gain_cb < -kToneGainMax || s[j].gain_cb > kToneGainMax) throw tone_refusal(j, 2, s[j].gain_cb, "centibels is outside " + std::to_string(-kToneGainMax) + " .. " + std::to_string(kToneGainMax));
        if (s[j].gain_cb != 0 && s[j].kind <= kToneLowpass) throw tone_refusal(j, 2, s[j].gain_cb, "centibels must be 0 for a high-pass or a low-pass");
        if (s[j].q_permille < kToneQMin || s[j].q_permille > kToneQMax) throw tone_refusal(j, 3, s[j].q_permille, "is outside " + std::to_string(kToneQMin) + " .. " + std::to_string(kToneQMax));
    }
}
void tone_coeffs(int n, const ToneSection* s, double (*out)[5]) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < n; ++j) {
        const double w0 = 2.0 * pi * (double)s[j].freq_hz / 24000.0, cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * ((double)s[j].q_permille / 1000.0));
        const double A = std::pow(10.0, (double)s[j].gain_cb / 400.0);
        double b0, b1, b2, a0, a1, a2;
        switch (s[j].kind) {
        case kToneHighpass: b0 = (1.0 + cw) / 2.0; b1 = -(1.0 + cw); b2 = b0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case kToneLowpass:  b0 = (1.0 - cw) / 2.0; b1 = 1.0 - cw; b2 = b0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case kTonePeak:     b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A; a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A; break;
        case kToneLowshelf: {
            const double sq = 2.0 * std::sqrt(A) * alpha, p = A + 1.0, m = A - 1.0;
            b0 = A * ((p - m * cw) + sq); b1 = 2.0 * A * (m - p * cw); b2 = A * ((p - m * cw) - sq);
            a0 = (p + m * cw) + sq; a1 = -2.0 * (m + p * cw); a2 = (p + m * cw) - sq; break; }
        default: {          // kToneHighshelf
            const double sq = 2.0 * std::sqrt(A) * alpha, p = A + 1.0, m = A - 1.0;
            b0 = A * ((p + m * cw) + sq); b1 = -2.0 * A * (m + p * cw); b2 = A * ((p + m * cw) - sq);
            a0 = (p - m * cw) + sq; a1 = 2.0 * (m - p * cw); a2 = (p - m * cw) - sq; break; }
        }
        out[j][0] = b0 / a0; out[j][1] = b1 / a0; out[j][2] = b2 / a0; out[j][3] = a1 / a0; out[j][4] = a2 / a0;
    }
}
// The presets have never been heard: no checkpoint exists, so they are textbook starting points, untuned.
static const struct { const char* name; const char* spec; } kTonePresets[] = {
    { "telephone", "hp:300:0.707,hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707,lp:3400:0.707" },
    { "rumble", "hp:80:0.707" },
    { "presence", "peak:3000:+4:0.9,hs:8000:+2:0.707" },
    { "warm", "ls:200:+3:0.707,hs:6000:-4:0.707" },
};
std::vector<ToneSection> tone_parse(const std::string& spec_in) {
    std::string spec = spec_in;
    for (const auto& p : kTonePresets) if (spec == p.name) spec = p.spec;
    if (spec.empty()) throw std::invalid_argument("tone: empty spec (a preset: telephone, rumble, presence, warm; or kind:Hz[:dB]:Q sections separated by commas)");
    // a number in a field: the whole field must be one; scaled and rounded to the integer the stage takes
    auto number = [](const std::string& f, int j, const char* what, double scale) -> int32_t {
        char* end = nullptr;
        const double v = f.empty() ? 0.0 : std::strtod(f.c_str(), &end);
        if (f.empty() || !end || *end != '\0' || !(v > -1e6 && v < 1e6)) throw std::invalid_argument("tone: section " + std::to_string(j) + " " + what + " '" + f + "' is no number");
        return (int32_t)std::llround(v * scale);
    };
    std::vector<ToneSection> out;
    size_t pos = 0;
    for (int j = 0; pos <= spec.size(); ++j) {
        const size_t comma = std::min(spec.find(',', pos), spec.size());
        const std::string sec = spec.substr(pos, comma - pos);
        pos = comma + 1;
        std::vector<std::string> f;
        for (size_t a = 0; a <= sec.size();) { const size_t c = std::min(sec.find(':', a), sec.size()); f.push_back(sec.substr(a, c - a)); a = c + 1; }
        ToneSection s{ 0, 0, 0, 0 };
        s.kind = f[0] == "hp" ? kToneHighpass : f[0] == "lp" ? kToneLowpass : f[0] == "ls" ? kToneLowshelf : f[0] == "hs" ? kToneHighshelf : f[0] == "peak" ? kTonePeak : 0;
        if (s.kind == 0) throw std::invalid_argument("tone: section " + std::to_string(j) + " kind '" + f[0] + "' is none of hp, lp, ls, hs, peak");
        const bool gained = s.kind > kToneLowpass;
        if (f.size() != (gained ? 4u : 3u)) throw std::invalid_argument("tone: section " + std::to_string(j) + " '" + sec + "' is not " + (gained ? "kind:Hz:dB:Q" : "kind:Hz:Q"));
        s.freq_hz = number(f[1], j, "freq_hz", 1.0);
        if (gained) s.gain_cb = number(f[2], j, "gain_cb", 10.0);
        s.q_permille = number(f.back(), j, "q_permille", 1000.0);
        out.push_back(s);
    }
    tone_check((int)out.size(), out.data());
    return out;
}

// ---------------------------------------------------------------------------------------------
// log-mel (reference mel.cpp:13-80 filterbank, :182-236 framing).  NOT librosa's: symmetric Hann
// window, no centre padding, frames = (n - win)/hop + 1 (one zero-padded frame for shorter clips),
// power spectrum, HTK mel scale, triangle corners snapped to FFT bins floor((n_fft+1) f / sr) with
// integer-bin slopes, natural log of (energy + 1e-10).  The corner bins come out of single-precision
// arithmetic in the reference; the same precision is used here so the corners land on the same bins.
// ---------------------------------------------------------------------------------------------
namespace {

float hz_to_mel(float hz) { return 2595.0f * log10f(1.0f + hz / 700.0f); }
float mel_to_hz(float m) { return 700.0f * (powf(10.0f, m / 2595.0f) - 1.0f); }

} // namespace

MelPlan make_plan(const MelSpec& s) {
    MelPlan p;
    p.spec = s;
    p.n = 1;
    while (p.n < s.n_fft) p.n <<= 1;
    p.bins = s.n_fft / 2 + 1;
    p.window.resize((size_t)s.win);
    for (int i = 0; i < s.win; ++i) p.window[(size_t)i] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * i / (s.win - 1))));
    p.tw_re.resize((size_t)p.n / 2);
    p.tw_im.resize((size_t)p.n / 2);
    for (int k = 0; k < p.n / 2; ++k) {
        p.tw_re[(size_t)k] = (float)cos(-2.0 * M_PI * k / p.n);
        p.tw_im[(size_t)k] = (float)sin(-2.0 * M_PI * k / p.n);
    }
    int lg = 0;
    while ((1 << lg) < p.n) ++lg;
    p.rev.resize((size_t)p.n);
    for (int i = 0; i < p.n; ++i) {
        uint32_t r = 0;
        for (int b = 0; b < lg; ++b) r |= (uint32_t)((i >> b) & 1) << (lg - 1 - b);
        p.rev[(size_t)i] = r;
    }
    const float m_lo = hz_to_mel(s.fmin), m_hi = hz_to_mel(s.fmax);
    std::vector<int> corner((size_t)s.n_mels + 2);
    for (int i = 0; i < s.n_mels + 2; ++i) {
        const float mel = m_lo + (m_hi - m_lo) * i / (s.n_mels + 1);
        const float hz = mel_to_hz(mel);
        corner[(size_t)i] = std::min((int)floorf((s.n_fft + 1) * hz / s.sample_rate), p.bins - 1);
    }
    p.lo.assign(corner.begin(), corner.end() - 2);
    p.mid.assign(corner.begin() + 1, corner.end() - 1);
    p.hi.assign(corner.begin() + 2, corner.end());
    return p;
}

namespace {

// in-place decimation-in-time radix-2 FFT on bit-reversed input
void fft_pow2(const MelPlan& p, float* re, float* im) {
    const int n = p.n;
    for (int len = 2; len <= n; len <<= 1) {
        const int half = len >> 1, step = n / len;
        for (int base = 0; base < n; base += len) {
            for (int k = 0; k < half; ++k) {
                const float wr = p.tw_re[(size_t)(k * step)], wi = p.tw_im[(size_t)(k * step)];
                float& ar = re[base + k];
                float& ai = im[base + k];
                float& br = re[base + k + half];
                float& bi = im[base + k + half];
                const float tr = wr * br - wi * bi, ti = wr * bi + wi * br;
                br = ar - tr; bi = ai - ti;
                ar += tr; ai += ti;
            }
        }
    }
}

} // namespace

std::vector<float> log_mel(const std::vector<float>& audio, const MelSpec& spec, int* frames_out) {
    *frames_out = 0;
    if (audio.empty()) return {};
    const MelPlan p = make_plan(spec);
    const long n_audio = (long)audio.size();
    const int frames = n_audio < spec.win ? 1 : (int)((n_audio - spec.win) / spec.hop + 1);
    std::vector<float> out((size_t)spec.n_mels * (size_t)frames);
    std::vector<float> re((size_t)p.n), im((size_t)p.n), power((size_t)p.bins);
    for (int t = 0; t < frames; ++t) {
        const long start = (long)t * spec.hop;
        std::fill(im.begin(), im.end(), 0.0f);
        for (int i = 0; i < p.n; ++i) {
            const long src = start + i;
            const float v = (i < spec.win && i < spec.n_fft && src < n_audio) ? audio[(size_t)src] * p.window[(size_t)i] : 0.0f;
            re[p.rev[(size_t)i]] = v;
        }
        fft_pow2(p, re.data(), im.data());
        const int kept = std::min(p.bins, p.n / 2 + 1);
        for (int k = 0; k < kept; ++k) power[(size_t)k] = re[(size_t)k] * re[(size_t)k] + im[(size_t)k] * im[(size_t)k];
        for (int k = kept; k < p.bins; ++k) power[(size_t)k] = 0.0f;
        for (int m = 0; m < spec.n_mels; ++m) {
            const int a = p.lo[(size_t)m], b = p.mid[(size_t)m], c = p.hi[(size_t)m];
            float e = 0.0f;
            for (int k = a; k < b; ++k) e += (float)(k - a) / (float)(b - a) * power[(size_t)k];
            for (int k = b; k < c; ++k) e += (float)(c - k) / (float)(c - b) * power[(size_t)k];
            out[(size_t)m * (size_t)frames + (size_t)t] = logf(e + 1e-10f);
        }
    }
    *frames_out = frames;
    return out;
}

} // namespace q3
