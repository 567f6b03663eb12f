// q3_loudness_kernels.hip — k_loudness, the loudness stage (LoudDesc, q3_common.h): a BS.1770 K-weighted meter with an
// exact integer energy measure and a slewed gain towards a target, for 24 kHz float PCM between the stretcher and the level stage.
// [HINT] no counterpart in the reference, whose wav_writer.cpp peak normalisation is dead code and needs the whole clip.
//
// The two biquads are recursive: u[k] needs u[k-1].  What does not recur is parallel — the feed-forward part ff = (b0 x[k] + b1 x[k-1])
// + b2 x[k-2] of either biquad, the energy quanta q[k], their integer sum and the output ramp run one sample per thread — and only the
// two-operation chain u[k] = (ff - a2 u[k-2]) - a1 u[k-1] is walked by one lane over a segment that lies in LDS.  One workgroup owns one
// stage of the push (blockIdx.x) and cuts the push's samples into segments that end at sub-block edges (at most kLoudBlock samples), so
// a sub-block's E is complete when its last segment is summed; the gain step follows, then the sub-block's samples leave with the
// ramp.  The arithmetic is the header's, in its order, every operation rounded once (the library is built with -ffp-contract=off):
// the samples, energies and gains depend on the input and the parameters alone, never on how the audio was cut into pushes.
#include "q3_audio.h"
#include "q3_common.h"

namespace q3 {

constexpr int kLoudThreads = 256;
constexpr int kLoudSampleOff = kLoudStateWords * 8;   // bytes: where a half's carried input begins

// sample k of the stage, from its carry or from the push's new samples: both addresses clamped, both loads issued, then selected
// (k_psola's discipline).  The carry holds [carry0, n_before), carry0 the open sub-block's first sample.
__device__ __forceinline__ float loud_sample(const LoudDesc& d, int64_t carry0, int64_t k) {
    int64_t jn = k - d.n_before, jc = k - carry0;
    const bool is_new = jn >= 0;
    const int64_t last_new = d.n_new > 0 ? d.n_new - 1 : 0;
    jn = jn < 0 ? 0 : (jn > last_new ? last_new : jn);
    jc = jc < 0 ? 0 : (jc > kLoudBlock - 1 ? kLoudBlock - 1 : jc);
    const float vn = d.x_new[jn];
    const float vc = ((const float*)(d.half_in + kLoudSampleOff))[jc];
    return is_new ? vn : vc;
}

__global__ __launch_bounds__(kLoudThreads) void k_loudness(const LoudDesc* descs) {
    __shared__ double bx[kLoudBlock + 2];      // a segment's x behind its two samples of history; later the second biquad's ff and v
    __shared__ double bu[kLoudBlock + 2];      // the first biquad's ff, then u, behind its history
    __shared__ long long red[kLoudThreads];
    __shared__ double hist[6];                 // x[k-1], x[k-2], u[k-1], u[k-2], v[k-1], v[k-2] at the next segment's first sample
    __shared__ long long acc[6];               // E_{b-1}, E_{b-2}, E_{b-3}, the open sub-block's sum, A, N
    __shared__ float gs[2];                    // G_{b-1}, G_b of the sub-block that just closed; gs[1] is the current gain
    const LoudDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    const bool meter = d.meter != 0;
    const int64_t blocks0 = d.n_before / kLoudBlock;          // sub-blocks closed before this push
    const int64_t carry0 = blocks0 * kLoudBlock;              // the open sub-block's first sample: the carry's, and a normaliser's first output
    if (tid == 0) {
        const double* hd = (const double*)d.half_in;
        const long long* hi = (const long long*)d.half_in + 6;
        const float g_in = *(const float*)(d.half_in + 12 * 8);
        for (int i = 0; i < 6; ++i) { const double h = hd[i]; const long long a = hi[i]; hist[i] = d.first ? 0.0 : h; acc[i] = d.first ? 0 : a; }
        gs[0] = gs[1] = d.first ? d.g_start : g_in;
    }
    if (meter) for (int i = tid; i < d.n_out && i < d.n_new; i += kLoudThreads) d.out[i] = d.x_new[i];   // a meter hands its input on
    __syncthreads();
    const double b0 = d.c[0], b1 = d.c[1], b2 = d.c[2], a1 = d.c[3], a2 = d.c[4];
    const double c0 = d.c[5], c1 = d.c[6], c2 = d.c[7], e1 = d.c[8], e2 = d.c[9];
    int64_t pos = d.n_before;
    while (pos < d.n_total) {
        const int64_t edge = (pos / kLoudBlock + 1) * kLoudBlock;
        const int64_t end = edge < d.n_total ? edge : d.n_total;
        const int len = (int)(end - pos);                      // 1 .. kLoudBlock
        const float* xs = d.x_new + (pos - d.n_before);
        for (int i = tid; i < len; i += kLoudThreads) bx[i + 2] = (double)xs[i];
        if (tid == 0) { bx[0] = hist[1]; bx[1] = hist[0]; bu[0] = hist[3]; bu[1] = hist[2]; }
        __syncthreads();
        for (int i = tid; i < len; i += kLoudThreads) bu[i + 2] = (b0 * bx[i + 2] + b1 * bx[i + 1]) + b2 * bx[i];
        __syncthreads();
        if (tid == 0) {                                        // the first biquad's recursion, in place
            double u1 = bu[1], u2 = bu[0];
#pragma unroll 8
            for (int i = 0; i < len; ++i) { const double u = (bu[i + 2] - a2 * u2) - a1 * u1; bu[i + 2] = u; u2 = u1; u1 = u; }
            hist[0] = bx[len + 1]; hist[1] = bx[len]; hist[2] = u1; hist[3] = u2;
            bx[0] = hist[5]; bx[1] = hist[4];                  // bx becomes the second biquad's: v's history in front
        }
        __syncthreads();
        for (int i = tid; i < len; i += kLoudThreads) bx[i + 2] = (c0 * bu[i + 2] + c1 * bu[i + 1]) + c2 * bu[i];
        __syncthreads();
        if (tid == 0) {                                        // the second biquad's recursion, in place
            double v1 = bx[1], v2 = bx[0];
#pragma unroll 8
            for (int i = 0; i < len; ++i) { const double v = (bx[i + 2] - e2 * v2) - e1 * v1; bx[i + 2] = v; v2 = v1; v1 = v; }
            hist[4] = v1; hist[5] = v2;
        }
        __syncthreads();
        long long s = 0;                                       // q = floor(min(z, 4) 2^32): an integer, so the sum is exact in any order
        for (int i = tid; i < len; i += kLoudThreads) {
            const double v = bx[i + 2], z = v * v;
            s += (long long)__builtin_floor((z < 4.0 ? z : 4.0) * 4294967296.0);
        }
        red[tid] = s;
        __syncthreads();
        for (int o = kLoudThreads / 2; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        const bool closes = end == edge;
        if (tid == 0) {
            const long long E = acc[3] + red[0];
            if (!closes) acc[3] = E;
            else {
                const int64_t b = edge / kLoudBlock - 1;       // the sub-block's absolute number
                long long A = acc[4], N = acc[5];
                if (b >= 3) {
                    const long long W = ((acc[2] + acc[1]) + acc[0]) + E;
                    if (W >= kLoudGate) { A += W; N += 1; }
                }
                const float Gp = gs[1];
                float T = Gp;
                if (N > 0 && !meter) {
                    const double P = (double)A / ((double)N * kLoudNorm);
                    double g = __builtin_sqrt(d.pt / P);
                    g = g < d.r_lo ? d.r_lo : (g > d.r_hi ? d.r_hi : g);
                    T = (float)g;
                }
                const float lo = Gp * kLoudDn, hi = Gp * kLoudUp;
                float G = T > lo ? T : lo;
                G = G < hi ? G : hi;
                acc[2] = acc[1]; acc[1] = acc[0]; acc[0] = E; acc[3] = 0; acc[4] = A; acc[5] = N;
                gs[0] = Gp; gs[1] = G;
                const int64_t j = b - blocks0;
                if (j >= 0 && j < d.n_blocks) { d.energies[j] = E; d.gains[j] = G; }
            }
        }
        __syncthreads();
        if (closes && !meter) {                                // the sub-block's samples, ramped from G_{b-1} to G_b
            const int64_t k0 = edge - kLoudBlock;
            const float Gp = gs[0], dG = gs[1] - gs[0];
            for (int i = tid; i < kLoudBlock; i += kLoudThreads) {
                const float x = loud_sample(d, carry0, k0 + i);
                const float g = Gp + dG * ((float)i / 2400.0f);
                const int64_t o = k0 + i - carry0;
                if (o >= 0 && o < d.n_out) d.out[o] = x * g;
            }
        }
        pos = end;
    }
    __syncthreads();
    const int64_t open0 = d.n_total / kLoudBlock * kLoudBlock;   // the open sub-block after this push
    const int n_open = (int)(d.n_total - open0);
    if (d.finish) {
        if (!meter) {                                          // the last, partial sub-block at the last gain, unramped
            const float G = gs[1];
            for (int i = tid; i < n_open; i += kLoudThreads) {
                const int64_t o = open0 + i - carry0;
                const float x = loud_sample(d, carry0, open0 + i);
                if (o >= 0 && o < d.n_out) d.out[o] = x * G;
            }
        }
        return;
    }
    if (!meter) {
        float* keep = (float*)(d.half_out + kLoudSampleOff);
        for (int i = tid; i < n_open; i += kLoudThreads) keep[i] = loud_sample(d, carry0, open0 + i);
    }
    if (tid == 0) {
        double* hd = (double*)d.half_out;
        long long* hi = (long long*)d.half_out + 6;
        for (int i = 0; i < 6; ++i) { hd[i] = hist[i]; hi[i] = acc[i]; }
        *(float*)(d.half_out + 12 * 8) = gs[1];
    }
}

void launch_loudness(const LoudDesc* tab, int n, hipStream_t s) {
    if (n < 1 || n > 65535) throw Error("loudness: 1..65535 stages per launch");
    hipLaunchKernelGGL(k_loudness, dim3(n), dim3(kLoudThreads), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
