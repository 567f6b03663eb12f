// q3_pitch_kernels.hip — k_psola, the pitch stage (PitchDesc, q3_common.h): TD-PSOLA shift of the fundamental of 24 kHz
// float PCM, the first stage behind the vocoder.  [HINT] no counterpart in the reference, which has no pitch control.
//
// Marks of one stage depend on each other (an analysis mark lies one period behind the last, a synthesis mark one scaled period), so
// one workgroup owns one stage and walks its marks in order; the parallelism is the 355 lags of a period search (one thread each) and
// the stages side by side (blockIdx.x).  Per search the region x[a - W, a + W + Pmax + 1) (881 floats, the template is its first 480)
// is staged in LDS once; thread `lag` reads region[lag + i] — consecutive lanes, consecutive banks — against a broadcast template
// element.  The arithmetic is the header's, in its order: four accumulators over i mod 4 for each of the three sums, every product and
// add rounded to fp32 (the library is built with -ffp-contract=off), score = num |num| / (E_t E_lag), the smallest local maximum within
// kPitchOctave2 of the best.  The two output accumulators live in an LDS ring of 1 024 entries: a grain is added at its absolute
// index mod 1 024, and what no later mark can reach (everything below t - Pmax) is divided, written and cleared before the next grain.
#include "q3_audio.h"
#include "q3_common.h"

namespace q3 {

constexpr int kPsolaThreads = 512;
static_assert(kPitchRing % kPsolaThreads == 0, "a thread must meet the same ring entries on every round of a flush");
static_assert(kPitchLags <= kPsolaThreads && 2 * kPitchPmax <= kPitchRing, "one lag per thread, one grain inside the ring");

// sample k of the stage, from its carry or from the push's new samples: both addresses clamped, both loads issued, then selected;
// zero outside [0, n_total) (k_pcm_sink's discipline)
__device__ __forceinline__ float psola_sample(const PitchDesc& d, int64_t k) {
    int64_t jn = k - d.n_before, jc = k - d.carry_abs0;
    const bool is_new = jn >= 0, inside = k >= 0 && k < d.n_total;
    const int64_t last_new = d.n_new > 0 ? d.n_new - 1 : 0;
    int64_t last_c = d.n_before - d.carry_abs0 - 1;
    last_c = last_c < 0 ? 0 : (last_c > kPitchCarry - 1 ? kPitchCarry - 1 : last_c);
    jn = jn < 0 ? 0 : (jn > last_new ? last_new : jn);
    jc = jc < 0 ? 0 : (jc > last_c ? last_c : jc);
    const float vn = d.x_new[jn];
    const float vc = d.half_in[jc];
    const float v = is_new ? vn : vc;
    return inside ? v : 0.0f;
}

__device__ __forceinline__ int psola_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the analysis mark at a: its period, and whether it is voiced.  Every thread calls it with the same a and returns the same pair.  A
// mark whose windows leave the known signal is unvoiced and costs nothing.
__device__ __forceinline__ int psola_search(const PitchDesc& d, int64_t a, float* region, float* sc, float* red_f, int* red_i, int tid, int& voiced) {
    voiced = 0;
    if (a < kPitchW || a + kPitchReach > d.n_total) return kPitchPu;
    for (int s = tid; s < kPitchRegion; s += kPsolaThreads) region[s] = psola_sample(d, a - kPitchW + s);
    __syncthreads();
    float score = -__builtin_inff();
    if (tid < kPitchLags) {
        const float* x = region + (kPitchPmin - 1) + tid;
        float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, n3 = 0.0f, e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, e3 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
        for (int i = 0; i < 2 * kPitchW; i += 4) {
            const float ta = region[i], tb = region[i + 1], tc = region[i + 2], td = region[i + 3];
            const float xa = x[i], xb = x[i + 1], xc = x[i + 2], xd = x[i + 3];
            n0 = n0 + ta * xa; n1 = n1 + tb * xb; n2 = n2 + tc * xc; n3 = n3 + td * xd;
            e0 = e0 + xa * xa; e1 = e1 + xb * xb; e2 = e2 + xc * xc; e3 = e3 + xd * xd;
            t0 = t0 + ta * ta; t1 = t1 + tb * tb; t2 = t2 + tc * tc; t3 = t3 + td * td;
        }
        const float num = (n0 + n1) + (n2 + n3), el = (e0 + e1) + (e2 + e3), et = (t0 + t1) + (t2 + t3);
        const float den = et * el;
        score = den > 0.0f ? (num * __builtin_fabsf(num)) / den : 0.0f;
    }
    sc[tid] = score;
    __syncthreads();
    // a candidate is a lag Pmin .. Pmax whose score is not below either neighbour's (a NaN score is no candidate)
    const float below = sc[tid > 0 ? tid - 1 : 0], above = sc[tid < kPsolaThreads - 1 ? tid + 1 : kPsolaThreads - 1];
    const bool cand = tid >= 1 && tid <= kPitchLags - 2 && score >= below && score >= above;
    float c = cand ? score : -__builtin_inff();
    for (int o = 32; o >= 1; o >>= 1) { const float c2 = __shfl_xor(c, o, 64); c = c2 > c ? c2 : c; }
    if ((tid & 63) == 0) red_f[tid >> 6] = c;
    __syncthreads();
    float best = red_f[0];
    for (int w = 1; w < kPsolaThreads / 64; ++w) best = red_f[w] > best ? red_f[w] : best;
    const float thr = kPitchOctave2 * best;
    int q = cand && score >= thr ? tid : kPsolaThreads;
    for (int o = 32; o >= 1; o >>= 1) { const int q2 = __shfl_xor(q, o, 64); q = q2 < q ? q2 : q; }
    if ((tid & 63) == 0) red_i[tid >> 6] = q;
    __syncthreads();
    q = red_i[0];
    for (int w = 1; w < kPsolaThreads / 64; ++w) q = red_i[w] < q ? red_i[w] : q;
    q = psola_clamp(q, 1, kPitchLags - 2);   // a NaN input cannot move a period out of Pmin .. Pmax
    voiced = best >= kPitchVoiced2 ? 1 : 0;
    return voiced ? kPitchPmin - 1 + q : kPitchPu;
}

__global__ __launch_bounds__(kPsolaThreads) void k_psola(const PitchDesc* descs) {
    __shared__ float region[kPitchRegion];
    __shared__ float sc[kPsolaThreads];
    __shared__ float acc[kPitchRing];
    __shared__ float wsm[kPitchRing];
    __shared__ float red_f[kPsolaThreads / 64];
    __shared__ int red_i[kPsolaThreads / 64];
    const PitchDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    const bool first = d.first != 0;
    const float* acc_in = d.half_in + kPitchCarry;
    const float* wsm_in = acc_in + kPitchRing;
    const int64_t* st_in = (const int64_t*)(wsm_in + kPitchRing);
    for (int m = tid; m < kPitchRing; m += kPsolaThreads) {
        const float va = acc_in[m], vw = wsm_in[m];
        const int idx = (int)((d.out0 + m) & (kPitchRing - 1));
        acc[idx] = first ? 0.0f : va;
        wsm[idx] = first ? 0.0f : vw;
    }
    const int64_t s0 = st_in[0], s1 = st_in[1], s2 = st_in[2], s3 = st_in[3], s4 = st_in[4], s5 = st_in[5], s6 = st_in[6], s7 = st_in[7];
    int64_t a_cur = first ? 0 : s0;
    int P_cur = first ? kPitchPu : psola_clamp((int)s1, kPitchPmin, kPitchPmax);
    int v_cur = first ? 0 : (s2 != 0);
    int has_next = first ? 0 : (s3 != 0);
    int P_next = first ? kPitchPu : psola_clamp((int)s4, kPitchPmin, kPitchPmax);
    int v_next = first ? 0 : (s5 != 0);
    int64_t s = first ? 0 : s6;
    int64_t marks = first ? 0 : s7;
    const int ratio = psola_clamp(d.ratio, kPitchMin, kPitchMax);
    const int64_t e_after = d.out0 + d.n_out;
    int64_t flushed = d.out0;
    __syncthreads();
    // outputs [flushed, upto) are final: no later mark reaches them
    auto flush = [&](int64_t upto) {
        upto = upto > e_after ? e_after : upto;
        for (int64_t k = flushed + tid; k < upto; k += kPsolaThreads) {
            const int idx = (int)(k & (kPitchRing - 1));
            const float a = acc[idx], w = wsm[idx];
            d.out[k - d.out0] = a / (w > kPitchFloor ? w : kPitchFloor);
            acc[idx] = 0.0f; wsm[idx] = 0.0f;
        }
        flushed = upto > flushed ? upto : flushed;
        __syncthreads();
    };
    for (;;) {
        const int64_t t = s >> kPitchFrac;
        const bool ready = d.finish ? t < d.n_total + kPitchPmax : t + kPitchGate <= d.n_total;
        if (!ready) break;
        while (a_cur + P_cur <= t) {   // the last analysis mark at or before t
            if (!has_next) P_next = psola_search(d, a_cur + P_cur, region, sc, red_f, red_i, tid, v_next);
            a_cur += P_cur; P_cur = P_next; v_cur = v_next; has_next = 0;
        }
        int64_t a_g = a_cur;
        int P_g = P_cur, v_g = v_cur;
        if (a_cur + P_cur - t <= t - a_cur) {   // the next one is nearer, or as near: the later of two
            if (!has_next) { P_next = psola_search(d, a_cur + P_cur, region, sc, red_f, red_i, tid, v_next); has_next = 1; }
            a_g = a_cur + P_cur; P_g = P_next; v_g = v_next;
        }
        flush(t - kPitchPmax);
        const float* win = d.win + pitch_window_offset(P_g);
        for (int m = tid; m < 2 * P_g; m += kPsolaThreads) {
            const int64_t k = t - P_g + m;
            const float xv = psola_sample(d, a_g - P_g + m);
            const float w = win[m];
            if (k >= flushed && k < flushed + kPitchRing) {
                const int idx = (int)(k & (kPitchRing - 1));
                acc[idx] = acc[idx] + w * xv;
                wsm[idx] = wsm[idx] + w;
            }
        }
        __syncthreads();
        s += v_g ? (((int64_t)P_g * 1000) << kPitchFrac) / ratio : (int64_t)P_g << kPitchFrac;
        ++marks;
    }
    flush(e_after);
    float* acc_out = d.half_out + kPitchCarry;
    float* wsm_out = acc_out + kPitchRing;
    for (int m = tid; m < kPitchRing; m += kPsolaThreads) {
        const int idx = (int)((e_after + m) & (kPitchRing - 1));
        acc_out[m] = acc[idx];
        wsm_out[m] = wsm[idx];
    }
    for (int i = tid; i < d.keep; i += kPsolaThreads) d.half_out[i] = psola_sample(d, d.keep_abs0 + i);
    if (tid == 0) {
        int64_t* st = (int64_t*)(wsm_out + kPitchRing);
        st[0] = a_cur; st[1] = P_cur; st[2] = v_cur; st[3] = has_next; st[4] = P_next; st[5] = v_next; st[6] = s; st[7] = marks;
    }
}

void launch_psola(const PitchDesc* tab, int n, hipStream_t s) {
    if (n < 1 || n > 65535) throw Error("pitch: 1..65535 stages per launch");
    hipLaunchKernelGGL(k_psola, dim3(n), dim3(kPsolaThreads), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
