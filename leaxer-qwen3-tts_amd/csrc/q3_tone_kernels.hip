// q3_tone_kernels.hip — k_tone, the tone stage (ToneDesc, q3_common.h): a cascade of 1 .. 8 biquads in double on 24 kHz
// float PCM between the stretcher and the loudness stage.  [HINT] no counterpart in the reference, which has no equaliser.
//
// Every section is recursive and needs the section before it, so walking them one after another (k_loudness's way) would cost n
// serial passes.  Here the cascade is a systolic pipeline across the lanes of one wave: lane j owns section j + 1 (its five
// coefficients, its input's last two samples and its output's), and at step t it filters sample t - j, whose input lane j - 1 produced
// at step t - 1 and hands over with a DPP move one lane to the right inside the row of 16 (lane 0 takes the sample from LDS instead:
// the move leaves a row's first lane what it had).  A push of m samples takes m + n - 1 steps whatever n is.  Lanes behind the last
// section run along and are never read.  Each section performs the header's operations in the header's order, every one a rounded fp64
// operation (the library is built with -ffp-contract=off), so the samples equal the sequential cascade's bit for bit and depend on
// the input and the sections alone, never on how the audio was cut into pushes or segments.
//
// One workgroup of one wave owns one stage of the push (blockIdx.x).  The push's samples pass through LDS in segments of kToneSegment:
// widened to double in parallel, filtered by the pipeline, which is not drained between segments (lane j simply runs j samples
// behind), and narrowed and stored in parallel.  Only the pipeline's first n - 1 steps and the n - 1 steps behind the push's last
// sample have idle lanes; they (and a segment's last few steps) run the guarded form of the step, everything between runs the
// plain one, eight steps to a block so that the LDS reads are issued ahead of the chain that needs them.
#include "q3_audio.h"
#include "q3_common.h"

namespace q3 {

constexpr int kToneThreads = 64;
constexpr int kTonePad = kToneMaxSections;   // steps a segment can run past its samples (the drain: at most n - 1)

// the value lane - 1 holds in v; a row's first lane keeps own (row_shr:1, bound_ctrl off: an invalid source leaves the old value)
__device__ __forceinline__ double tone_from_left(double own, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(own), __double2loint(v), 0x111, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(own), __double2hiint(v), 0x111, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// steps [i, i_end) of a segment in the guarded form: a lane whose sample k0 + i lies outside the push computes and keeps nothing
__device__ __forceinline__ void tone_guarded(int& i, int i_end, int k0, int n_new, bool tail, const double* xs, double* ys, double b0, double b1, double b2,
                                             double a1, double a2, double& in1, double& in2, double& out1, double& out2, double& y) {
    for (; i < i_end; ++i) {
        const int k = k0 + i;
        const bool live = k >= 0 && k < n_new;
        const double u = tone_from_left(xs[i], y);
        const double ff = (b0 * u + b1 * in1) + b2 * in2;
        y = (ff - a2 * out2) - a1 * out1;
        in2 = live ? in1 : in2; in1 = live ? u : in1;
        out2 = live ? out1 : out2; out1 = live ? y : out1;
        if (tail && live) ys[i] = y;
    }
}

__global__ __launch_bounds__(kToneThreads) void k_tone(const ToneDesc* descs) {
    __shared__ double xs[kToneSegment + kTonePad];   // a segment's input, zeros behind it for the drain
    __shared__ double ys[kToneSegment + kTonePad];   // step i's output of the last section: sample seg0 + i - (n - 1)
    const ToneDesc& d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = d.n_sections, n_new = d.n_new;
    const int j = lane & 15;                          // the lane's delay in samples
    const int jc = j < n ? j : n - 1;                 // its section, clamped: the lanes behind the last one repeat it
    const bool tail = lane == n - 1;                  // the lane whose output leaves
    const double b0 = d.c[jc][0], b1 = d.c[jc][1], b2 = d.c[jc][2], a1 = d.c[jc][3], a2 = d.c[jc][4];
    const double* si = d.state_in + 2 * jc;
    const double h0 = si[0], h1 = si[1], h2 = si[2], h3 = si[3];
    const bool first = d.first != 0;
    double in1 = first ? 0.0 : h0, in2 = first ? 0.0 : h1;     // the section's input: its last sample, the one before
    double out1 = first ? 0.0 : h2, out2 = first ? 0.0 : h3;   // the section's output likewise
    double y = 0.0;                                   // what the lane hands to its right neighbour
    const float* x = d.x_new;
    float* out = d.out;

    for (int seg0 = 0; seg0 < n_new; seg0 += kToneSegment) {
        const int len = n_new - seg0 < kToneSegment ? n_new - seg0 : kToneSegment;
        const int steps = len + (seg0 + len == n_new ? n - 1 : 0);   // the push's last segment drains the pipeline
        for (int i = lane; i < len; i += kToneThreads) xs[i] = (double)x[seg0 + i];
        for (int i = len + lane; i < steps; i += kToneThreads) xs[i] = 0.0;
        __syncthreads();
        int i = 0;
        const int ramp = n - 1 - seg0;                // steps of this segment before lane n - 1 has a sample
        tone_guarded(i, ramp < 0 ? 0 : (ramp < steps ? ramp : steps), seg0 - j, n_new, tail, xs, ys, b0, b1, b2, a1, a2, in1, in2, out1, out2, y);
        for (; i + 8 <= len; i += 8) {                // steps n - 1 <= t < n_new, eight at a time: every section has a sample
            double xv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) xv[q] = xs[i + q];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const double u = tone_from_left(xv[q], y);
                const double ff = (b0 * u + b1 * in1) + b2 * in2;
                y = (ff - a2 * out2) - a1 * out1;
                in2 = in1; in1 = u; out2 = out1; out1 = y;
                if (tail) ys[i + q] = y;
            }
        }
        tone_guarded(i, steps, seg0 - j, n_new, tail, xs, ys, b0, b1, b2, a1, a2, in1, in2, out1, out2, y);
        __syncthreads();
        for (int s = lane; s < steps; s += kToneThreads) {
            const int k = seg0 + s - (n - 1);
            if (k >= 0 && k < n_new) out[k] = (float)ys[s];
        }
        __syncthreads();
    }
    double* so = d.state_out;
    if (lane < n) { so[2 * lane] = in1; so[2 * lane + 1] = in2; }
    if (tail) { so[2 * n] = out1; so[2 * n + 1] = out2; }
}

void launch_tone(const ToneDesc* tab, int n, hipStream_t s) {
    if (n < 1 || n > 65535) throw Error("tone: 1..65535 stages per launch");
    hipLaunchKernelGGL(k_tone, dim3(n), dim3(kToneThreads), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
