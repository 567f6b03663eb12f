// q3_speed_kernels.hip — k_wsola, the speaking-rate stage (SpeedDesc, q3_common.h): WSOLA time stretch of 24 kHz float PCM
// between the vocoder and the sink.  [HINT] no counterpart in the reference, which has no speed control.
//
// Frames of one stretcher depend on each other through the chosen position p_{m-1}, so one workgroup owns one stretcher and walks its
// ready frames in order; the parallelism is the 2 D + 1 = 481 lags of a frame's search (one thread each) and the stretchers side by
// side (blockIdx.x).  Per frame the search region x[a_m - D .. a_m + D + N) (1200 floats) and the template (720 floats) are staged in
// LDS once; thread `lag` reads region[lag + i] — consecutive lanes, consecutive banks — and the template element is a broadcast.  The
// arithmetic is the header's, in its order: four accumulators over i mod 4, every product and add rounded to fp32 (the library is built
// with -ffp-contract=off), c = (s0 + s1) + (s2 + s3), arg-max with (value descending, lag ascending) as the order.
#include "q3_audio.h"
#include "q3_common.h"

namespace q3 {

constexpr int kWsolaThreads = 512;
constexpr int kWsolaLags = 2 * kSpeedD + 1;            // 481
constexpr int kWsolaRegion = kSpeedN + 2 * kSpeedD;    // 1200

// sample k of the stretcher, from its carry or from the push's new samples: both addresses clamped, both loads issued, then selected;
// zero outside [0, n_total) (k_pcm_sink's discipline)
__device__ __forceinline__ float wsola_sample(const SpeedDesc& d, int64_t k) {
    int64_t jn = k - d.n_before, jc = k - d.carry_abs0;
    const bool is_new = jn >= 0, inside = k >= 0 && k < d.n_total;
    const int64_t last_new = d.n_new > 0 ? d.n_new - 1 : 0, last_c = d.n_before - d.carry_abs0 > 0 ? d.n_before - d.carry_abs0 - 1 : 0;
    jn = jn < 0 ? 0 : (jn > last_new ? last_new : jn);
    jc = jc < 0 ? 0 : (jc > last_c ? last_c : jc);
    const float vn = d.x_new[jn];
    const float vc = d.carry_in[jc];
    const float v = is_new ? vn : vc;
    return inside ? v : 0.0f;
}

// (c, lag) is better than (c2, lag2): larger value, the smaller lag among equals
__device__ __forceinline__ bool wsola_better(float c, int lag, float c2, int lag2) { return c > c2 || (c == c2 && lag < lag2); }

__global__ __launch_bounds__(kWsolaThreads) void k_wsola(const SpeedDesc* descs) {
    __shared__ float region[kWsolaRegion];
    __shared__ float tmpl[kSpeedN];
    __shared__ float red_c[kWsolaThreads / 64];
    __shared__ int red_lag[kWsolaThreads / 64];
    const SpeedDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    const int wi = tid < kSpeedHs ? tid : 0;               // threads below Hs write the block: their two window values
    const float w_new = d.win[wi], w_old = d.win[kSpeedHs + wi];
    const int64_t p_state = d.state_in[0];
    int64_t p_prev = d.frame0 == 0 ? -(int64_t)kSpeedHs : p_state;
    for (int f = 0; f < d.n_frames; ++f) {
        const int64_t a = (d.frame0 + f) * kSpeedHs * d.speed / 1000;
        for (int s = tid; s < kWsolaRegion; s += kWsolaThreads) region[s] = wsola_sample(d, a - kSpeedD + s);
        for (int s = tid; s < kSpeedN; s += kWsolaThreads) tmpl[s] = wsola_sample(d, p_prev + kSpeedHs + s);
        __syncthreads();
        float c = -__builtin_inff();
        int lag = tid;
        if (tid < kWsolaLags) {
            const float* x = region + tid;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            for (int i = 0; i < kSpeedN; i += 4) {
                s0 = s0 + tmpl[i] * x[i];
                s1 = s1 + tmpl[i + 1] * x[i + 1];
                s2 = s2 + tmpl[i + 2] * x[i + 2];
                s3 = s3 + tmpl[i + 3] * x[i + 3];
            }
            c = (s0 + s1) + (s2 + s3);
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const float c2 = __shfl_xor(c, o, 64);
            const int lag2 = __shfl_xor(lag, o, 64);
            if (wsola_better(c2, lag2, c, lag)) { c = c2; lag = lag2; }
        }
        if ((tid & 63) == 0) { red_c[tid >> 6] = c; red_lag[tid >> 6] = lag; }
        __syncthreads();
        c = red_c[0]; lag = red_lag[0];
        for (int w = 1; w < kWsolaThreads / 64; ++w)
            if (wsola_better(red_c[w], red_lag[w], c, lag)) { c = red_c[w]; lag = red_lag[w]; }
        lag = lag < 0 ? 0 : (lag > kWsolaLags - 1 ? kWsolaLags - 1 : lag);   // a NaN input cannot move the block's reads out of the region
        // x[p_m + i] = region[lag + i]
        const int o = f * kSpeedHs + tid;
        if (tid < kSpeedHs && o < d.n_out) d.out[o] = (w_old * tmpl[tid]) + (w_new * region[lag + tid]);
        if (tid == 0) d.offs[f] = lag - kSpeedD;
        p_prev = a + (lag - kSpeedD);
        __syncthreads();   // before the next frame's staging overwrites region / tmpl / red_*
    }
    for (int s = tid; s < d.keep; s += kWsolaThreads) d.carry_out[s] = wsola_sample(d, d.keep_abs0 + s);
    if (tid == 0) { d.state_out[0] = p_prev; d.state_out[1] = d.frame0 + d.n_frames; }
}

void launch_wsola(const SpeedDesc* tab, int n, hipStream_t s) {
    if (n < 1 || n > 65535) throw Error("speed: 1..65535 stretchers per launch");
    hipLaunchKernelGGL(k_wsola, dim3(n), dim3(kWsolaThreads), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
