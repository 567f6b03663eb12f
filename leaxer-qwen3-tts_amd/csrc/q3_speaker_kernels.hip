// q3_speaker_kernels.hip — kernels of the ECAPA-TDNN speaker encoder (voice-clone path, SURVEY.md 8f-2;
// the reference runs speaker_encoder.onnx through ORT, src/tts_onnx.cpp:367-403).  One pass per reference
// clip (not per frame): ~5 MFLOP per mel frame, so these are plain fp32 FMA kernels with LDS-staged input
// tiles — the work is far below anything worth an MFMA pipeline.  Activations are time-major [T][C]; a batch of clips is stored
// clip after clip along time with a table of (row offset, T) per clip (SpkClip).  The file also holds the GPU audio front end of the
// same path (k_resample_linear, k_logmel: the arithmetic of q3_audio.cpp).
#include "q3_common.h"

namespace q3 {

// "same" Conv1d with reflect padding: y[t][co] = act(b[co] + sum_{ci,j} W[j][ci][co] * in[reflect(t + (j - k/2) dil)][ci]),
// in = x (+ x2).  Tile: 64 output channels x 16 time steps per workgroup, 32 input channels per LDS stage.
// With a clip table (blockIdx.z = clip) the tile grid starts at each clip's own t = 0 and reflect padding stays inside the clip, so a
// clip's arithmetic does not depend on what else is in the batch; workgroups past the clip's last frame exit.
__global__ __launch_bounds__(256) void k_spk_conv(SpkConvArgs a) {
    __shared__ float xs[5][16][33];
    const int co = blockIdx.x * 64 + (threadIdx.x & 63), tg = threadIdx.x >> 6;
    const int t0 = blockIdx.y * 16, half = a.k / 2;
    if (a.clips) {
        const SpkClip cl = a.clips[blockIdx.z];
        if (t0 >= cl.T) return;
        a.T = cl.T;
        if (a.x_channel_major) { a.x += (size_t)cl.row_off * a.Cin; a.ldx = cl.T; }
        else a.x += (size_t)cl.row_off * a.ldx;
        if (a.x2) a.x2 += (size_t)cl.row_off * a.ldx2;
        a.y += (size_t)cl.row_off * a.ldy;
    }
    float acc[4] = { 0.f, 0.f, 0.f, 0.f };
    for (int c0 = 0; c0 < a.Cin; c0 += 32) {
        for (int e = threadIdx.x; e < a.k * 512; e += 256) {
            const int c = e & 31, tt = (e >> 5) & 15, j = e >> 9;
            const int t = t0 + tt;
            float v = 0.f;
            if (t < a.T && c0 + c < a.Cin) {
                int src = t + (j - half) * a.dil;
                src = src < 0 ? -src : (src >= a.T ? 2 * (a.T - 1) - src : src);
                v = a.x_channel_major ? a.x[(size_t)(c0 + c) * a.ldx + src] : a.x[(size_t)src * a.ldx + c0 + c];
                if (a.x2) v += a.x2[(size_t)src * a.ldx2 + c0 + c];
            }
            xs[j][tt][c] = v;
        }
        __syncthreads();
        if (co < a.Cout) {
            const int cn = a.Cin - c0 < 32 ? a.Cin - c0 : 32;
            for (int c = 0; c < cn; ++c)
                for (int j = 0; j < a.k; ++j) {
                    const float w = a.W[((size_t)j * a.Cin + c0 + c) * a.Cout + co];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = fmaf(w, xs[j][tg * 4 + q][c], acc[q]);
                }
        }
        __syncthreads();
    }
    if (co >= a.Cout) return;
    const float b = a.bias[co];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = t0 + tg * 4 + q;
        if (t >= a.T) continue;
        float v = acc[q] + b;
        if (a.act >= 1) v = v > 0.f ? v : 0.f;
        if (a.act == 2) v = tanhf(v);
        a.y[(size_t)t * a.ldy + co] = v;
    }
}

// torch Conv1d weight [Cout][Cin][k] -> [k][Cin][Cout]
__global__ void k_spk_repack(const float* w, float* out, int cout, int cin, int k) {
    const size_t n = (size_t)cout * cin * k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % cout), ci = (int)((i / cout) % cin), j = (int)(i / ((size_t)cout * cin));
        out[i] = w[((size_t)co * cin + ci) * k + j];
    }
}

// per-channel reductions over time; 64 channels x 4 time lanes per workgroup, fixed combination order
template <typename F>
static __device__ __forceinline__ float col_reduce(int T, int tl, F f, float (*red)[64], int cl, bool is_max) {
    float s = is_max ? -INFINITY : 0.f;
    for (int t = tl; t < T; t += 4) { const float v = f(t); s = is_max ? fmaxf(s, v) : s + v; }
    red[tl][cl] = s;
    __syncthreads();
    const float r = is_max ? fmaxf(fmaxf(red[0][cl], red[1][cl]), fmaxf(red[2][cl], red[3][cl])) : ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    __syncthreads();
    return r;
}

// mean[c] (and, if sd != null, sqrt(max(mean of squared deviations, 1e-12))) of x[T][ld]
// clips != null: blockIdx.y = clip, rows [row_off, row_off + T) of x, mean / sd rows [clip][C]
__global__ __launch_bounds__(256) void k_spk_colstats(const float* x, int ld, int T, int C, float* mean, float* sd, const SpkClip* clips) {
    __shared__ float red[4][64];
    if (clips) {
        const SpkClip cl = clips[blockIdx.y];
        T = cl.T;
        x += (size_t)cl.row_off * ld;
        mean += (size_t)blockIdx.y * C;
        if (sd) sd += (size_t)blockIdx.y * C;
    }
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, ch = blockIdx.x * 64 + cl;
    const int cc = ch < C ? ch : C - 1;
    const float mu = col_reduce(T, tl, [&](int t) { return x[(size_t)t * ld + cc]; }, red, cl, false) / (float)T;
    float var = 0.f;
    if (sd) var = col_reduce(T, tl, [&](int t) { const float d = x[(size_t)t * ld + cc] - mu; return d * d; }, red, cl, false) / (float)T;
    if (ch < C && tl == 0) {
        mean[ch] = mu;
        if (sd) sd[ch] = sqrtf(var > 1e-12f ? var : 1e-12f);
    }
}

// squeeze-excitation gate + block residual: h[t][c] = y[t][c] * sigmoid(g[c]) + h[t][c]; the same value goes to cat[t][c]
__global__ void k_spk_se_gate(const float* y, const float* g, float* h, float* cat, int ld_cat, int T, int C, const SpkClip* clips) {
    if (clips) {   // blockIdx.y = clip, gate row [clip][C]
        const SpkClip cl = clips[blockIdx.y];
        T = cl.T;
        y += (size_t)cl.row_off * C; h += (size_t)cl.row_off * C; cat += (size_t)cl.row_off * ld_cat;
        g += (size_t)blockIdx.y * C;
    }
    const size_t n = (size_t)T * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t t = i / C;
        const float v = y[i] * (1.0f / (1.0f + expf(-g[c]))) + h[i];
        h[i] = v;
        cat[t * ld_cat + c] = v;
    }
}

// attention input of the pooling layer: rows [x[t] | mean | sd]  (C each)
__global__ void k_spk_asp_input(const float* x, const float* mean, const float* sd, float* out, int T, int C, const SpkClip* clips) {
    if (clips) {   // blockIdx.y = clip, mean / sd rows [clip][C]
        const SpkClip cl = clips[blockIdx.y];
        T = cl.T;
        x += (size_t)cl.row_off * C; out += (size_t)cl.row_off * 3 * C;
        mean += (size_t)blockIdx.y * C; sd += (size_t)blockIdx.y * C;
    }
    const size_t n = (size_t)T * 3 * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % (3 * C));
        const size_t t = i / (3 * C);
        out[i] = c < C ? x[t * C + c] : (c < 2 * C ? mean[c - C] : sd[c - 2 * C]);
    }
}

// attentive statistics: per channel, softmax over time of the scores s[T][C], then the weighted mean and standard
// deviation of x[T][C]; out[c] = mean, out[C + c] = sd
__global__ __launch_bounds__(256) void k_spk_asp_pool(const float* s, const float* x, int T, int C, float* out, const SpkClip* clips) {
    __shared__ float red[4][64];
    if (clips) {   // blockIdx.y = clip, out rows [clip][2 C]
        const SpkClip cl = clips[blockIdx.y];
        T = cl.T;
        s += (size_t)cl.row_off * C; x += (size_t)cl.row_off * C;
        out += (size_t)blockIdx.y * 2 * C;
    }
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, ch = blockIdx.x * 64 + cl;
    const int cc = ch < C ? ch : C - 1;
    const float mx = col_reduce(T, tl, [&](int t) { return s[(size_t)t * C + cc]; }, red, cl, true);
    const float den = col_reduce(T, tl, [&](int t) { return expf(s[(size_t)t * C + cc] - mx); }, red, cl, false);
    const float mu = col_reduce(T, tl, [&](int t) { return expf(s[(size_t)t * C + cc] - mx) / den * x[(size_t)t * C + cc]; }, red, cl, false);
    const float var = col_reduce(T, tl, [&](int t) { const float d = x[(size_t)t * C + cc] - mu; return expf(s[(size_t)t * C + cc] - mx) / den * d * d; }, red, cl, false);
    if (ch < C && tl == 0) {
        out[ch] = mu;
        out[C + ch] = sqrtf(var > 1e-12f ? var : 1e-12f);
    }
}

// ---------------------------------------------------------------------------------------------
// Audio front end of the clone path on the GPU: the arithmetic of q3_audio.cpp, many clips per launch.
// ---------------------------------------------------------------------------------------------

// q3::resample_linear element for element: position and weight in double, two products and a sum in double, one rounding to float
// (the library is built with -ffp-contract=off, so these are the host's IEEE operations and the samples are the host's bits)
__global__ __launch_bounds__(256) void k_resample_linear(const float* raw, float* rs, const SpkClip* clips) {
    const SpkClip cl = clips[blockIdx.y];
    if (cl.src_rate == cl.dst_rate) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cl.n_rs) return;
    const float* a = raw + cl.in_off;
    const double ratio = (double)cl.dst_rate / cl.src_rate;
    const double pos = (double)i / ratio;
    int k = (int)pos;
    if (k > cl.n_in - 1) k = cl.n_in - 1;   // never taken for i < floor(n_in * ratio); keeps the load inside the clip whatever the table says
    const double w = pos - (double)k;
    const int k1 = k + 1 < cl.n_in - 1 ? k + 1 : cl.n_in - 1;
    rs[cl.rs_off + i] = (float)((double)a[k] * (1.0 - w) + (double)a[k1] * w);
}

// k_resample_linear for encoder streams: the clip is still arriving, so a sample is either in the stream's carry or among the push's
// new ones.  Both addresses are clamped into their buffers and both loads issued; the value is selected afterwards.
__device__ __forceinline__ float rs_stream_sample(const EncRsStream& d, const char* staged_new, int64_t k) {
    int64_t jn = k - d.n_before, jc = k - d.carry_abs0;
    const bool is_new = jn >= 0;
    const int64_t last_new = d.n_new > 0 ? d.n_new - 1 : 0, last_c = d.n_before - d.carry_abs0 > 0 ? d.n_before - d.carry_abs0 - 1 : 0;
    jn = jn < 0 ? 0 : (jn > last_new ? last_new : jn);
    jc = jc < 0 ? 0 : (jc > last_c ? last_c : jc);
    float vn;   // the staging buffer always holds at least one padded element; the format is the stream's (uniform over blockIdx.y)
    if (d.format == Q3TTS_PCM_F32) vn = ((const float*)staged_new)[jn];
    else if (d.format == Q3TTS_PCM_S16) vn = (float)((const int16_t*)staged_new)[jn] / 32768.0f;
    else vn = (float)g711_dec(d.format, ((const uint8_t*)staged_new)[jn]) / 32768.0f;
    const float vc = d.carry_in[jc];
    return is_new ? vn : vc;
}
__global__ __launch_bounds__(256) void k_stream_resample_linear(const char* staged, float* x24, const EncRsStream* tab) {
    const EncRsStream d = tab[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.n_out + d.keep) return;
    const char* snew = staged + d.in_off;
    if (t >= d.n_out) {   // the next carry: the last `keep` samples the stream has
        const int j = t - d.n_out;
        d.carry_out[j] = rs_stream_sample(d, snew, d.n_total - d.keep + j);
        return;
    }
    const int64_t i = d.out0 + t, last = d.n_total - 1;
    const double ratio = 24000.0 / d.src_rate;
    const double pos = (double)i / ratio;
    int64_t k = (int64_t)pos;
    if (k > last) k = last;   // never taken for an output the host rule emits; keeps the taps inside the stream whatever the table says
    const double w = pos - (double)k;
    const int64_t k1 = k + 1 < last ? k + 1 : last;
    x24[d.x24_off + t] = (float)((double)rs_stream_sample(d, snew, k) * (1.0 - w) + (double)rs_stream_sample(d, snew, k1) * w);
}

// One frame per workgroup: window -> the host's radix-2 decimation-in-time FFT (same butterflies, same twiddle table, so the same
// roundings) -> power -> one lane per mel band sums its triangle in the host's order -> logf(e + 1e-10f).  The complex frame lives in
// LDS; index i is stored at i + i / 32, which spreads the stride-2 .. stride-32 accesses of the first five stages over the banks.
#define MEL_IX(i) ((i) + ((i) >> 5))
__global__ __launch_bounds__(256) void k_logmel(const float* raw, const float* rs, const SpkClip* clips, MelTablesDev tb, float* mel) {
    __shared__ float re[1024 + 32], im[1024 + 32], wr_s[512], wi_s[512];
    const SpkClip cl = clips[blockIdx.y];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= cl.T) return;
    const bool as_is = cl.src_rate == cl.dst_rate;
    const float* a = as_is ? raw + cl.in_off : rs + cl.rs_off;
    const int n_audio = as_is ? cl.n_in : cl.n_rs, start = t * 256;
    for (int i = tid; i < 1024; i += 256) {
        const int src = start + i;
        re[MEL_IX(tb.rev[i])] = src < n_audio ? a[src] * tb.window[i] : 0.0f;
        im[MEL_IX(i)] = 0.0f;
    }
    for (int i = tid; i < 512; i += 256) { wr_s[i] = tb.tw_re[i]; wi_s[i] = tb.tw_im[i]; }
    __syncthreads();
    for (int lg = 0; lg < 10; ++lg) {   // half = 1 << lg, len = 2 half, twiddle step = 512 >> lg
        const int half = 1 << lg;
        for (int b = tid; b < 512; b += 256) {
            const int k = b & (half - 1), i0 = ((b >> lg) << (lg + 1)) + k;
            const int i = MEL_IX(i0), j = MEL_IX(i0 + half);
            const float wr = wr_s[k << (9 - lg)], wi = wi_s[k << (9 - lg)];
            const float ar = re[i], ai = im[i], br = re[j], bi = im[j];
            const float tr = wr * br - wi * bi, ti = wr * bi + wi * br;
            re[j] = ar - tr; im[j] = ai - ti;
            re[i] = ar + tr; im[i] = ai + ti;
        }
        __syncthreads();
    }
    for (int k = tid; k <= 512; k += 256) {   // power spectrum over the kept bins, in place of re[]
        const int i = MEL_IX(k);
        re[i] = re[i] * re[i] + im[i] * im[i];
    }
    __syncthreads();
    if (tid < 128) {
        const int lo = tb.lo[tid], mid = tb.mid[tid], hi = tb.hi[tid];
        float e = 0.0f;
        for (int k = lo; k < mid; ++k) e += (float)(k - lo) / (float)(mid - lo) * re[MEL_IX(k)];
        for (int k = mid; k < hi; ++k) e += (float)(hi - k) / (float)(hi - mid) * re[MEL_IX(k)];
        mel[(size_t)cl.row_off * 128 + (size_t)tid * cl.T + t] = logf(e + 1e-10f);
    }
}
#undef MEL_IX

void launch_spk_conv(const SpkConvArgs& a, hipStream_t s) {
    if (a.k < 1 || a.k > 5 || !(a.k & 1)) throw Error("speaker conv: kernel size must be 1, 3 or 5");
    const int shortest = a.clips ? a.min_T : a.T;
    if (a.T < 1 || shortest < 1 || (a.k > 1 && (a.k / 2) * a.dil >= shortest)) throw Error("speaker conv: reflect padding needs more frames");
    if (a.clips && (a.n_clips < 1 || a.n_clips > 65535)) throw Error("speaker conv: 1..65535 clips per launch");
    if ((a.T + 15) / 16 > 65535) throw Error("speaker conv: more than 65535 x 16 rows in one launch");
    hipLaunchKernelGGL(k_spk_conv, dim3((a.Cout + 63) / 64, (a.T + 15) / 16, a.clips ? a.n_clips : 1), dim3(256), 0, s, a);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_spk_repack(const float* w, float* out, int cout, int cin, int k, hipStream_t s) {
    const size_t n = (size_t)cout * cin * k;
    hipLaunchKernelGGL(k_spk_repack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, w, out, cout, cin, k);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_spk_colstats(const float* x, int ld, int T, int C, float* mean, float* sd, hipStream_t s, const SpkClip* clips, int n_clips) {
    hipLaunchKernelGGL(k_spk_colstats, dim3((C + 63) / 64, clips ? n_clips : 1), dim3(256), 0, s, x, ld, T, C, mean, sd, clips);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_spk_se_gate(const float* y, const float* g, float* h, float* cat, int ld_cat, int T, int C, hipStream_t s, const SpkClip* clips, int n_clips) {
    const size_t n = (size_t)T * C;
    hipLaunchKernelGGL(k_spk_se_gate, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192), clips ? n_clips : 1), dim3(256), 0, s, y, g, h, cat, ld_cat, T, C, clips);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_spk_asp_input(const float* x, const float* mean, const float* sd, float* out, int T, int C, hipStream_t s, const SpkClip* clips, int n_clips) {
    const size_t n = (size_t)T * 3 * C;
    hipLaunchKernelGGL(k_spk_asp_input, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192), clips ? n_clips : 1), dim3(256), 0, s, x, mean, sd, out, T, C, clips);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_spk_asp_pool(const float* sc, const float* x, int T, int C, float* out, hipStream_t s, const SpkClip* clips, int n_clips) {
    hipLaunchKernelGGL(k_spk_asp_pool, dim3((C + 63) / 64, clips ? n_clips : 1), dim3(256), 0, s, sc, x, T, C, out, clips);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_resample_linear(const float* raw, float* rs, const SpkClip* clips, int n_clips, int max_n_rs, hipStream_t s) {
    if (n_clips < 1 || n_clips > 65535 || max_n_rs < 1) throw Error("resample: 1..65535 clips with at least one output sample");
    hipLaunchKernelGGL(k_resample_linear, dim3((max_n_rs + 255) / 256, n_clips), dim3(256), 0, s, raw, rs, clips);
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_resample_linear_streams(const void* staged, float* x24, const EncRsStream* tab, int n, int max_work, hipStream_t s) {
    if (n < 1 || n > 65535 || max_work < 1) throw Error("stream resample: 1..65535 streams with at least one output or carry sample");
    hipLaunchKernelGGL(k_stream_resample_linear, dim3((max_work + 255) / 256, n), dim3(256), 0, s, (const char*)staged, x24, tab);
}

void launch_logmel(const float* raw, const float* rs, const SpkClip* clips, int n_clips, int max_T, const MelTablesDev& tb, float* mel, hipStream_t s) {
    if (n_clips < 1 || n_clips > 65535 || max_T < 1) throw Error("log-mel: 1..65535 clips with at least one frame");
    hipLaunchKernelGGL(k_logmel, dim3(max_T, n_clips), dim3(256), 0, s, raw, rs, clips, tb, mel);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
