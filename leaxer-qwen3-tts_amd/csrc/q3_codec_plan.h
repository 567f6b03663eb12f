// q3_codec_plan.h — the host arithmetic of the vocoder's decode paths (q3_codec.cpp: codec_run, codec_pre_batch, the single and the
// batched push, priming; Engine::codec_decode_range_dev): the decoder's length formula, the frames the stages behind the pre-transformer
// look back, the cut of a push's own samples out of its window's, the batched push's grouping, the bump arenas' byte counts and the
// staging of host codes with the one refusal of a bad code.  No HIP in here: tests/test_cpu_codec_plan.py drives this header from a
// plain g++ harness.  The reference decodes a whole utterance in one run_vocoder call (src/tts_onnx.cpp:759-776) and has none of this.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/q3tts.h"

namespace q3 {

// ---- lengths ----
// samples of F frames (q3tts_codec_decode_len): the ConvNeXt stages multiply, each decoder block's transposed conv (k = 2 r, stride r) trims
inline int64_t codec_decode_len(const q3tts_config& c, int F) {
    int64_t T = F;
    for (int s = 0; s < c.cd_n_up; ++s) T *= c.cd_up_ratios[s];
    for (int i = 0; i < c.cd_n_blocks; ++i) {
        const int r = c.cd_up_rates[i], k = 2 * r, pad = k - r;
        const int left = c.cd_tconv_trim == 0 ? pad : 0;
        T = (T - 1) * r + k - left - pad;
    }
    return T;
}
inline int64_t codec_len_of(const q3tts_config& c, int n) { return n <= 0 ? 0 : codec_decode_len(c, n); }   // L(n), L(0) = 0
inline int64_t codec_up_front(const q3tts_config& c) {   // rows per frame behind the ConvNeXt stages
    int64_t up = 1;
    for (int i = 0; i < c.cd_n_up; ++i) up *= c.cd_up_ratios[i];
    return up;
}
inline int64_t codec_samples_per_frame(const q3tts_config& c) {
    int64_t up = codec_up_front(c);
    for (int i = 0; i < c.cd_n_blocks; ++i) up *= c.cd_up_rates[i];
    return up;
}

// frames the stages behind the pre-transformer look back, from the config: rows of lookback at each layer's rate / rows per frame
inline int codec_stage_b_context(const q3tts_config& c) {
    double frames = 0.0, rate = 1.0;
    for (int s = 0; s < c.cd_n_up; ++s) { rate *= c.cd_up_ratios[s]; frames += 6.0 / rate; }            // ConvNeXt: depthwise causal k7 at the stage's output rate
    frames += 6.0 / rate;                                                                                    // conv_in k7
    for (int i = 0; i < c.cd_n_blocks; ++i) {
        frames += 1.0 / rate;                                                                                // transposed conv k = 2 r: one input row back
        rate *= c.cd_up_rates[i];
        frames += 6.0 * (1 + 3 + 9) / rate;                                                                  // three 7-tap convs, dilations 1, 3, 9
    }
    frames += 6.0 / rate;                                                                                    // conv_out k7
    return (int)frames + 3;                                                                                  // + margin for the transposed convs' trimming
}

// ---- the window cut: frames [a0, a0 + n) decoded as the tail of the window [a0 - ctx, a0 + n) own n_own of its samples, from `first` ----
struct CodecCut {
    int64_t first = 0, n_own = 0;
    // against the window's decoded length: a window that ends with the frames ends with their samples; a shorter sequence of a padded
    // group (fills == false) only has to hold them
    bool matches(int64_t n_win, bool fills = true) const { return first >= 0 && (fills ? first + n_own == n_win : first + n_own <= n_win); }
};
inline CodecCut codec_window_cut(const q3tts_config& c, int a0, int n, int ctx) {
    CodecCut k;
    k.first = codec_len_of(c, a0) - codec_samples_per_frame(c) * (a0 - ctx);
    k.n_own = codec_len_of(c, a0 + n) - codec_len_of(c, a0);
    return k;
}

// ---- the batched push's grouping ----
// order: left-context length min(n_done, ctxB) descending, mature streams (the common case) first, ties in call order
template <class LeftCtx>
void codec_push_order(std::vector<int>& live, LeftCtx left_ctx) {
    std::stable_sort(live.begin(), live.end(), [&](int x, int y) { return left_ctx(x) > left_ctx(y); });
}
// groups [i0, i1) of equal left context over the ordered streams, cut so that a group's conv decoder stays inside ~16 GB of workspace
// (4.7 MB per frame at 0.6B dims); Tw: rows of the group's longest window
struct CodecGroup { int i0 = 0, i1 = 0, Tw = 0; };
template <class Ctx, class New>
std::vector<CodecGroup> codec_push_groups(int g, Ctx ctx, New n_new) {
    std::vector<CodecGroup> groups;
    for (int i0 = 0; i0 < g;) {
        int i1 = i0, Tw = 0;
        while (i1 < g && ctx(i1) == ctx(i0)) {
            const int Tw1 = std::max(Tw, ctx(i1) + n_new(i1));
            if (i1 > i0 && (int64_t)(i1 - i0 + 1) * Tw1 * 4700000 > ((int64_t)16 << 30)) break;
            Tw = Tw1; ++i1;
        }
        groups.push_back(CodecGroup{ i0, i1, Tw });
        i0 = i1;
    }
    return groups;
}

// ---- workspace: 256-byte bump arenas ----
inline size_t codec_bytes_of(size_t nfloat) { return (nfloat * sizeof(float) + 255) & ~(size_t)255; }
struct CodecBump {   // base == nullptr: a planning pass, which only counts
    char* base = nullptr; size_t off = 0;
    float* operator()(size_t nfloat) { float* p = base ? (float*)(base + off) : nullptr; off += codec_bytes_of(nfloat); return p; }
};
constexpr size_t CODEC_KSLAB_FLOATS = (size_t)32 * 128 * 4096;   // split-K partial sums of the short pre-transformer / ConvNeXt GEMMs
// the pre-transformer's six row buffers (h, hn, att | qkv | up, gate) and the slab
inline size_t codec_pre_bytes(const q3tts_config& c, size_t rows) {
    return codec_bytes_of(rows * c.cd_hidden) * 3 + codec_bytes_of(rows * 3 * c.cd_hidden) + codec_bytes_of(rows * c.cd_ffn) * 2 + codec_bytes_of(CODEC_KSLAB_FLOATS);
}
inline size_t codec_scratch_kv_bytes(const q3tts_config& c, size_t n, size_t P) { return codec_bytes_of(n * c.cd_heads * P * c.cd_head_dim) * 2; }   // K and V, [n][head][P][d]
inline size_t codec_upsample_bytes(const q3tts_config& c, size_t rows) {   // per stage: y, ln (hidden each) and the 4x wide hidden, at the stage's output rate
    size_t need = 0;
    for (int s = 0; s < c.cd_n_up; ++s) { rows *= (size_t)c.cd_up_ratios[s]; need += codec_bytes_of(rows * c.cd_hidden) * 2 + codec_bytes_of(rows * 4 * c.cd_hidden); }
    return need;
}
inline size_t codec_batch_arena_bytes(const q3tts_config& c, size_t n, size_t Fp, size_t P, bool with_upsampling) {   // codec_pre_batch
    return codec_pre_bytes(c, n * Fp) + codec_scratch_kv_bytes(c, n, P) + (with_upsampling ? codec_upsample_bytes(c, n * Fp) : 0);
}
inline size_t codec_stream_arena_bytes(const q3tts_config& c, size_t T) { return codec_pre_bytes(c, T); }               // the single push
inline size_t codec_sbatch_push_bytes(const q3tts_config& c, size_t T, size_t back_rows) {                              // the batched push: + the largest group's window
    return codec_pre_bytes(c, T) + codec_bytes_of(back_rows * c.cd_hidden) + codec_upsample_bytes(c, back_rows);
}
inline size_t codec_sbatch_prime_bytes(const q3tts_config& c, size_t g, size_t Fp, size_t Ps) { return codec_pre_bytes(c, g * Fp) + codec_scratch_kv_bytes(c, g, Ps); }

// ---- host codes: checked against the codebook and narrowed; the first bad one is refused, with the library's one text for it ----
template <class Err>
void stage_codes(const int64_t* codes, size_t n, int codebook, int32_t* dst) {
    for (size_t i = 0; i < n; ++i) {
        if (codes[i] < 0 || codes[i] >= codebook) throw Err("codec_decode: code out of range");
        dst[i] = (int32_t)codes[i];
    }
}

} // namespace q3
