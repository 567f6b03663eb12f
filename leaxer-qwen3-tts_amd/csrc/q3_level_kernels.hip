// q3_level_kernels.hip — k_level, the output-level stage (LevelDesc, q3_common.h): gain and look-ahead limiter on 24 kHz
// float PCM between the stretcher and the sink.  [HINT] no counterpart in the reference, whose dead wav_writer.cpp peak-normalises a
// whole clip, which a streaming engine cannot do.
//
// A workgroup owns a tile of kLevelTile outputs of one stage (blockIdx.y: the stage, blockIdx.x: the tile; workgroups past a stage's
// last tile leave at once).  Output k reads v[k - 127 .. k + 127], so the tile stages kLevelTile + 254 values of v in LDS and forms r
// beside them; the 128-wide minimum is seven doubling passes between two LDS rows (w_{2s}[i] = min(w_s[i], w_s[i + s]): consecutive
// lanes, consecutive banks); each thread then quantises five consecutive minima (stride 5: odd, no bank conflict), the block's prefix
// sum is a wave scan by __shfl_up plus one LDS word per wave, and the window sum is the difference of two prefix entries.  min and the
// integer sum are order-free and every fp32 operation is a single rounded one (the library is built with -ffp-contract=off and without
// fast-math: the division is hipcc's default, correctly rounded), so a sample's bits do not depend on the tile it fell into.
#include "q3_audio.h"
#include "q3_common.h"

namespace q3 {

constexpr int kLevelThreads = 256;
constexpr int kLevelSpan = kLevelTile + kLevelCarry;        // 1278: v and r of a tile, from k0 - 127
constexpr int kLevelQ = kLevelTile + kLevelW - 1;           // 1151: m and q of a tile, from k0 - 127
constexpr int kLevelPer = (kLevelQ + kLevelThreads - 1) / kLevelThreads;   // 5 values of q per thread
static_assert(kLevelTile == 4 * kLevelThreads, "a thread writes four consecutive outputs");
static_assert(kLevelW == 128 && kLevelCarry == 254, "the doubling passes below build a 128-wide window");

// v[k] of the stage, from its carry or from the push's new samples: both addresses clamped, both loads issued, then selected; zero
// outside [0, n_total) (k_pcm_sink's discipline)
__device__ __forceinline__ float level_v(const LevelDesc& d, int64_t k) {
    int64_t jn = k - d.n_before, jc = k - (d.n_before - kLevelCarry);
    const bool is_new = jn >= 0, inside = k >= 0 && k < d.n_total;
    const int64_t last_new = d.n_new > 0 ? d.n_new - 1 : 0;
    jn = jn < 0 ? 0 : (jn > last_new ? last_new : jn);
    jc = jc < 0 ? 0 : (jc > kLevelCarry - 1 ? kLevelCarry - 1 : jc);
    const float vn = d.g * d.x_new[jn];
    const float vc = d.carry_in[jc];
    const float v = is_new ? vn : vc;
    return inside ? v : 0.0f;
}

// four consecutive outputs of a thread: one 16-byte store where all four exist (out + o is 16-byte aligned: the host packs a call's
// outputs at multiples of 64 floats and o is a multiple of 4)
__device__ __forceinline__ void level_store4(float* out, int o, int n_out, const float (&y)[4]) {
    if (o + 4 <= n_out) *reinterpret_cast<float4*>(out + o) = make_float4(y[0], y[1], y[2], y[3]);
    else for (int j = 0; j < 4; ++j) if (o + j < n_out) out[o + j] = y[j];
}

__global__ __launch_bounds__(kLevelThreads) void k_level(const LevelDesc* descs) {
    __shared__ float vs[kLevelSpan];
    __shared__ float ra[kLevelSpan];
    __shared__ float rb[kLevelSpan];
    __shared__ int ps[kLevelQ + 1];
    __shared__ int wsum[kLevelThreads / 64];
    const LevelDesc d = descs[blockIdx.y];
    const int tiles = level_tiles(d.n_out);
    if ((int)blockIdx.x >= tiles) return;
    const int tid = threadIdx.x;
    const int o0 = (int)blockIdx.x * kLevelTile;          // the tile's first output within the push
    const int o = o0 + 4 * tid;                           // this thread's first
    float y[4];
    if (!d.limit) {                                       // gain only: out0 == n_before, one product
        for (int j = 0; j < 4; ++j) {
            const int i = o + j < d.n_new ? o + j : (d.n_new > 0 ? d.n_new - 1 : 0);
            y[j] = d.g * d.x_new[i];
        }
        level_store4(d.out, o, d.n_out, y);
        return;
    }
    const float T = d.T;
    const int64_t k0 = d.out0 + o0 - (kLevelW - 1);       // absolute index of vs[0]
    for (int s = tid; s < kLevelSpan; s += kLevelThreads) {
        const float v = level_v(d, k0 + s);
        const float a = __builtin_fabsf(v);
        vs[s] = v;
        ra[s] = a > T ? T / a : 1.0f;
    }
    __syncthreads();
    // w_1 = r; w_{2s}[i] = min(w_s[i], w_s[i + s]) is defined for i < kLevelSpan - 2 s + 1; w_128 ends up in rb (seven passes)
    float* src = ra;
    float* dst = rb;
    for (int step = 1; step < kLevelW; step <<= 1) {
        for (int s = tid; s < kLevelSpan - 2 * step + 1; s += kLevelThreads) dst[s] = __builtin_fminf(src[s], src[s + step]);
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
    const float* m = src;
    // q and its exclusive prefix sum ps[i] = q[0] + .. + q[i - 1]
    int qv[kLevelPer];
    int sum = 0;
#pragma unroll
    for (int j = 0; j < kLevelPer; ++j) {
        const int i = kLevelPer * tid + j;
        qv[j] = i < kLevelQ ? (int)__builtin_floorf(m[i] * 65536.0f) : 0;
        sum += qv[j];
    }
    const int lane = tid & 63, wave = tid >> 6;
    int inc = sum;
    for (int sh = 1; sh < 64; sh <<= 1) {
        const int up = __shfl_up(inc, sh, 64);
        if (lane >= sh) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    if (tid == 0) ps[0] = 0;
#pragma unroll
    for (int j = 0; j < kLevelPer; ++j) {
        const int i = kLevelPer * tid + j;
        run += qv[j];
        if (i < kLevelQ) ps[i + 1] = run;
    }
    __syncthreads();
    // output o0 + p: S = q[p] + .. + q[p + 127] (<= 2^23, exact as a float), s = S 2^-23, y = clamp(v s)
    const int p = 4 * tid;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s = (float)(ps[p + j + kLevelW] - ps[p + j]) * 1.1920928955078125e-07f;
        const float t = vs[p + j + kLevelW - 1] * s;
        y[j] = __builtin_fminf(__builtin_fmaxf(t, -T), T);
    }
    level_store4(d.out, o, d.n_out, y);
    // the stage's last workgroup: the next carry, v[n_total - 254 .. n_total)
    if (d.keep > 0 && (int)blockIdx.x == tiles - 1)
        for (int s = tid; s < kLevelCarry; s += kLevelThreads) d.carry_out[s] = level_v(d, d.n_total - kLevelCarry + s);
}

void launch_level(const LevelDesc* tab, int n, int max_tiles, hipStream_t s) {
    if (n < 1 || n > 65535) throw Error("level: 1..65535 stages per launch");
    if (max_tiles < 1) throw Error("level: a launch has at least one tile");
    hipLaunchKernelGGL(k_level, dim3((unsigned)max_tiles, (unsigned)n), dim3(kLevelThreads), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
