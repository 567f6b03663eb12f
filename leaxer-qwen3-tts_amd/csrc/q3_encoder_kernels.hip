// q3_encoder_kernels.hip — kernels of the 12 Hz speech tokenizer's encoder (audio -> codes; q3_encoder.cpp), gfx950.
// Network [HINT: transformers MimiModel.encode]: SEANet encoder (causal convs) -> transformer at 25 Hz -> stride-2 conv -> split
// residual VQ.  Everything is fp32: the encoder runs once per clip and its output is integer decisions, so precision comes first.
// Activations are time-major rows [T][C], clip after clip; every kernel that looks across time takes the clip from the grid
// (EncSpan tables) and stays inside it, so a clip's arithmetic does not depend on what else is in the batch.
#include <limits.h>

#include <algorithm>
#include <cstdint>

#include "q3_common.h"

namespace q3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static __device__ __forceinline__ float enc_elu(float v) { return v > 0.f ? v : expm1f(v); }
static __device__ __forceinline__ float enc_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// ------------------------------------------------------------------------------------------------
// k_enc_conv_mfma — strided / dilated causal Conv1d as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain per
// output).  Workgroup tile: 64 output rows x 64 output channels, K walked as (tap) x (32 input channels); 4 waves, one 32 x 32
// accumulator block each.  The k = 1 linear layers of the transformer are the same kernel with one tap.
// Bounds: every global load is guarded by (row inside the clip, channel < Cin / Cout); rows past the clip's T_out are staged as
// zeros and never stored.  An output's sum runs over (tap, ci) in one fixed order whatever its tile, so results are reproducible
// across batch compositions.
// ------------------------------------------------------------------------------------------------
#define ET_M 64
#define ET_N 64
#define ET_K 32
#define ET_LD 33   // padded LDS row: ds_read_b32 of a column is conflict-free

// HIST (streamed pushes): the span is one stream's new rows; an input row before the chunk comes from the stream's
// carry ring (EncHist), resolved per staged row.  The K walk, the MFMA order, the epilogue and every guard are the one-shot's, so an
// output has the bits the one-shot gives it.  HIST = false compiles to the kernel as it was.
// Row `src` (chunk-local, already shifted) of a stream's input: chunk row, carry-ring row, or nullptr (a zero row).  Every returned
// pointer is inside the chunk's T rows or the ring's cap rows whatever the table holds.
static __device__ __forceinline__ const float* enc_hist_row(const EncHist& hs, const float* in, int T, int src, int replicate, int Cin) {
    if (replicate && src > T - 1) src = T - 1;       // finishing push: the last row repeated
    if (src >= T) return nullptr;                    // finishing push: zeros complete the last output
    int abs_row = hs.n_in + src;
    if (replicate && abs_row < 0) abs_row = 0;       // the stream's first row repeated
    if (abs_row < 0) return nullptr;
    if (abs_row >= hs.n_in) return in + (size_t)(abs_row - hs.n_in) * Cin;
    if (hs.cap < 1 || hs.n_in - abs_row > hs.cap) return nullptr;
    return hs.carry + (size_t)(abs_row % hs.cap) * Cin;
}

template <bool HIST>
static __device__ __forceinline__ void enc_conv_mfma_body(const EncConvArgs& a, const EncHist* hist) {
    __shared__ float As[ET_M][ET_LD];
    __shared__ float Bs[ET_N][ET_LD];
    const EncSpan si = a.sin[blockIdx.z], so = a.sout[blockIdx.z];
    EncHist hs;
    if constexpr (HIST) hs = hist[blockIdx.z];
    const int t0 = blockIdx.x * ET_M, co0 = blockIdx.y * ET_N;
    if (t0 >= so.T) return;   // whole workgroup: no barrier has been passed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const float* in = a.in + (size_t)si.off * a.Cin;
    const bool vec = (a.Cin & 3) == 0;

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    const int srow = tid >> 3, scol = (tid & 7) * 4;   // rows srow and srow + 32, 4 channels each
    for (int tap = 0; tap < a.taps; ++tap) {
        const float* Wt = a.W + (size_t)tap * a.Cout * a.Cin;
        for (int ci0 = 0; ci0 < a.Cin; ci0 += ET_K) {
            const int ci = ci0 + scol;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = srow + 32 * h;
                const int t = t0 + r;
                int src = t * a.stride - a.pad_left + tap * a.dil;
                bool ok = t < so.T;
                const float* prow = nullptr;
                if constexpr (HIST) {
                    if (ok) prow = enc_hist_row(hs, in, si.T, src + hs.shift, a.replicate, a.Cin);
                    ok = prow != nullptr;
                } else {
                    if (a.replicate) src = src < 0 ? 0 : (src > si.T - 1 ? si.T - 1 : src);
                    else ok = ok && src >= 0 && src < si.T;
                }
                float v[4] = { 0.f, 0.f, 0.f, 0.f };
                if (ok) {
                    const float* p = (HIST ? prow : in + (size_t)src * a.Cin) + ci;
                    if (vec) {
                        if (ci < a.Cin) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (ci + e < a.Cin) v[e] = p[e];
                    }
                    if (a.elu_in) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = enc_elu(v[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) As[r][scol + e] = v[e];
                const int co = co0 + r;
                float w[4] = { 0.f, 0.f, 0.f, 0.f };
                if (co < a.Cout) {
                    const float* p = Wt + (size_t)co * a.Cin + ci;
                    if (vec) {
                        if (ci < a.Cin) { const float4 q = *reinterpret_cast<const float4*>(p); w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (ci + e < a.Cin) w[e] = p[e];
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) Bs[r][scol + e] = w[e];
            }
            __syncthreads();
            const float* ap = &As[wr * 32 + (lane & 31)][lane >> 5];
            const float* bp = &Bs[wc * 32 + (lane & 31)][lane >> 5];
#pragma unroll
            for (int kk = 0; kk < ET_K / 2; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * 2], bp[kk * 2], acc, 0, 0, 0);
            __syncthreads();
        }
    }

    // D[row][col]: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int co = co0 + wc * 32 + (lane & 31);
    if (co >= a.Cout) return;
    const float bias = a.bias ? a.bias[co] : 0.f;
    const float sc = a.scale ? a.scale[co] : 1.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int t = t0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (t >= so.T) continue;
        float v = acc[reg] + bias;
        if (a.act == 1) v = enc_gelu(v);
        if (a.scale) v = sc * v;
        const size_t o = (size_t)(so.off + t) * a.Cout + co;
        if (a.res) v = a.res[o] + v;
        a.out[o] = v;
    }
}
__global__ __launch_bounds__(256) void k_enc_conv_mfma(EncConvArgs a) { enc_conv_mfma_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void k_enc_conv_mfma_hist(EncConvArgs a, const EncHist* hist) { enc_conv_mfma_body<true>(a, hist); }

// The 1-channel first conv (24 kHz samples -> enc_filters channels): VALU work, 64 output rows per workgroup, the clip's samples of
// the tile's window in LDS.  Window = 63 * stride + (taps - 1) * dil + 1 <= 1024 samples (launch_enc_conv checks).
template <bool HIST>
static __device__ __forceinline__ void enc_conv_c1_body(const EncConvArgs& a, const EncHist* hist) {
    __shared__ float xs[1024];
    const EncSpan si = a.sin[blockIdx.z], so = a.sout[blockIdx.z];
    const int t0 = blockIdx.x * 64;
    if (t0 >= so.T) return;
    const int win = 63 * a.stride + (a.taps - 1) * a.dil + 1;
    const int base = t0 * a.stride - a.pad_left;
    for (int i = threadIdx.x; i < win; i += 256) {
        int src = base + i;
        float v = 0.f;
        if constexpr (HIST) {
            const EncHist hs = hist[blockIdx.z];
            const float* p = enc_hist_row(hs, a.in + (size_t)si.off, si.T, src + hs.shift, a.replicate, 1);
            if (p) v = *p;
        } else {
            if (a.replicate) src = src < 0 ? 0 : (src > si.T - 1 ? si.T - 1 : src);
            if (src >= 0 && src < si.T) v = a.in[(size_t)si.off + src];
        }
        xs[i] = a.elu_in ? enc_elu(v) : v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * a.Cout; i += 256) {
        const int r = i / a.Cout, co = i - r * a.Cout, t = t0 + r;
        if (t >= so.T) continue;
        float acc = 0.f;
        for (int tap = 0; tap < a.taps; ++tap) acc += a.W[(size_t)tap * a.Cout + co] * xs[r * a.stride + tap * a.dil];
        float v = acc + (a.bias ? a.bias[co] : 0.f);
        if (a.act == 1) v = enc_gelu(v);
        if (a.scale) v = a.scale[co] * v;
        const size_t o = (size_t)(so.off + t) * a.Cout + co;
        if (a.res) v = a.res[o] + v;
        a.out[o] = v;
    }
}
__global__ __launch_bounds__(256) void k_enc_conv_c1(EncConvArgs a) { enc_conv_c1_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void k_enc_conv_c1_hist(EncConvArgs a, const EncHist* hist) { enc_conv_c1_body<true>(a, hist); }

static void enc_launch_conv(const EncConvArgs& a, const EncHist* hist, hipStream_t s) {
    if (!a.in || !a.out || !a.W || !a.sin || !a.sout) throw Error("encoder conv: NULL argument");
    if (a.n_clips < 1 || a.n_clips > 65535 || a.max_T_out < 1) throw Error("encoder conv: 1..65535 clips with at least one output row");
    if (a.Cin < 1 || a.Cout < 1 || a.taps < 1 || a.dil < 1 || a.stride < 1) throw Error("encoder conv: bad shape");
    const int tiles = (a.max_T_out + 63) / 64;
    if (a.Cin == 1) {
        if (63 * a.stride + (a.taps - 1) * a.dil + 1 > 1024) throw Error("encoder conv: the 1-channel kernel covers windows of up to 1024 samples");
        if (hist) hipLaunchKernelGGL(k_enc_conv_c1_hist, dim3(tiles, 1, a.n_clips), dim3(256), 0, s, a, hist);
        else hipLaunchKernelGGL(k_enc_conv_c1, dim3(tiles, 1, a.n_clips), dim3(256), 0, s, a);
    } else {
        const int ny = (a.Cout + ET_N - 1) / ET_N;
        if (ny > 65535) throw Error("encoder conv: too many output channels");
        if (hist) hipLaunchKernelGGL(k_enc_conv_mfma_hist, dim3(tiles, ny, a.n_clips), dim3(256), 0, s, a, hist);
        else hipLaunchKernelGGL(k_enc_conv_mfma, dim3(tiles, ny, a.n_clips), dim3(256), 0, s, a);
    }
    Q3_HIP_CHECK(hipGetLastError());
}
void launch_enc_conv(const EncConvArgs& a, hipStream_t s) { enc_launch_conv(a, nullptr, s); }
void launch_enc_conv_hist(const EncConvArgs& a, const EncHist* hist, hipStream_t s) {
    if (!hist) throw Error("encoder conv: NULL history table");
    enc_launch_conv(a, hist, s);
}

// ------------------------------------------------------------------------------------------------
// LayerNorm rows with bias (torch.nn.LayerNorm: biased variance, two passes): one wave per row
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_enc_layernorm(const float* x, const float* w, const float* b, float eps, int rows, int C, float* out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    float s = 0.f;
    for (int i = lane; i < C; i += 64) s += xr[i];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int i = lane; i < C; i += 64) { const float d = xr[i] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    float* o = out + (size_t)row * C;
    for (int i = lane; i < C; i += 64) o[i] = (xr[i] - mean) * rstd * w[i] + b[i];
}
void launch_enc_layernorm(const float* x, const float* w, const float* b, float eps, int rows, int C, float* out, hipStream_t s) {
    if (rows < 1 || C < 1) throw Error("encoder layernorm: bad shape");
    hipLaunchKernelGGL(k_enc_layernorm, dim3((rows + 3) / 4), dim3(256), 0, s, x, w, b, eps, rows, C, out);
    Q3_HIP_CHECK(hipGetLastError());
}

// rotate-half RoPE on the q and k thirds of qkv rows, position = row index inside the clip (tables made in double on the host)
template <bool HIST>
static __device__ __forceinline__ void enc_rope_body(float* qkv, const float* cs, const float* sn, int max_pos, int heads, int d, const EncSpan* spans, const EncHist* hist) {
    const EncSpan sp = spans[blockIdx.y];
    const int half = d >> 1, per_row = 2 * heads * half;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)sp.T * per_row) return;
    const int t = (int)(i / per_row), r = (int)(i - (int64_t)t * per_row);
    const int which = r / (heads * half), hh = (r - which * heads * half) / half, j = r % half;
    int pos = t;
    if constexpr (HIST) pos += hist[blockIdx.y].n_in;   // the row's absolute index in its stream
    pos = pos < max_pos ? pos : max_pos - 1;            // the host refuses clips (and sizes streams) so that nothing reaches this
    float* p = qkv + (size_t)(sp.off + t) * (3 * heads * d) + (size_t)which * heads * d + (size_t)hh * d;
    const float c = cs[(size_t)pos * half + j], sv = sn[(size_t)pos * half + j];
    const float x1 = p[j], x2 = p[j + half];
    p[j] = x1 * c - x2 * sv;
    p[j + half] = x2 * c + x1 * sv;
}
__global__ __launch_bounds__(256) void k_enc_rope(float* qkv, const float* cs, const float* sn, int max_pos, int heads, int d, const EncSpan* spans) {
    enc_rope_body<false>(qkv, cs, sn, max_pos, heads, d, spans, nullptr);
}
__global__ __launch_bounds__(256) void k_enc_rope_hist(float* qkv, const float* cs, const float* sn, int max_pos, int heads, int d, const EncSpan* spans, const EncHist* hist) {
    enc_rope_body<true>(qkv, cs, sn, max_pos, heads, d, spans, hist);
}
void launch_enc_rope(float* qkv, const float* cs, const float* sn, int max_pos, int heads, int d, const EncSpan* spans, int n_clips, int max_T, hipStream_t s,
                     const EncHist* hist) {
    if (n_clips < 1 || n_clips > 65535 || max_T < 1 || max_pos < 1) throw Error("encoder rope: bad shape");
    const int64_t per_clip = (int64_t)max_T * heads * d;
    const dim3 grid((unsigned)((per_clip + 255) / 256), n_clips);
    if (hist) hipLaunchKernelGGL(k_enc_rope_hist, grid, dim3(256), 0, s, qkv, cs, sn, max_pos, heads, d, spans, hist);
    else hipLaunchKernelGGL(k_enc_rope, grid, dim3(256), 0, s, qkv, cs, sn, max_pos, heads, d, spans);
    Q3_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Causal sliding-window attention inside a clip: row t attends to rows (t - window, t].  One wave per (row, head): the lanes take
// the window's keys (each a full q . k dot product), the scores go through LDS, then the lanes take the output dims.  window <= 1024
// and d <= 128 (launch check); every load is inside the clip's rows by construction (j0 >= 0, j0 + n - 1 = t < T).
// ------------------------------------------------------------------------------------------------
#define EA_WMAX 1024
// HIST (streamed pushes): row t of the chunk is absolute row P + t of its stream; a key before the chunk comes from the layer's
// K/V ring ([window - 1][2 AO]: rotated K, then V; absolute row r in slot r mod (window - 1)).  The lane <-> jj mapping, the per-lane
// running sums, wave_sum and the sequential jj loop of P.V are the one-shot's, so the sums come out in the same order.  Ring rows read
// are absolute rows [P - (window - 1), P) that exist (>= 0): slots < window - 1 by the modulo.
template <bool HIST>
static __device__ __forceinline__ void enc_attn_body(const float* qkv, float* out, int heads, int d, int window, float scale, const EncSpan* spans, const EncHist* hist) {
    __shared__ float sc[4][EA_WMAX];
    __shared__ float qs[4][128];
    const EncSpan sp = spans[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * 4 + wave;
    const int t = (int)(task / heads), h = (int)(task % heads);
    const bool valid = t < sp.T;
    const int AO = heads * d, ld = 3 * AO;
    int P = 0; const float* ring = nullptr; const int cap = window - 1;
    if constexpr (HIST) { P = hist[blockIdx.y].n_in; ring = hist[blockIdx.y].carry; }
    const int pa = P + t;   // absolute row; j0 is absolute too
    const int j0 = valid ? (pa - window + 1 > 0 ? pa - window + 1 : 0) : 0, n = valid ? pa - j0 + 1 : 0;
    const float* base = qkv + (size_t)sp.off * ld;   // the chunk's row 0 (absolute row P): indexed by r - P for absolute rows r >= P
    if (valid) for (int i = lane; i < d; i += 64) qs[wave][i] = base[(size_t)t * ld + (size_t)h * d + i];
    __syncthreads();
    float m = -INFINITY;
    for (int jj = lane; jj < n; jj += 64) {
        const int r = j0 + jj;
        const float* kr;
        if (HIST && r < P) kr = ring + (size_t)(r % cap) * (2 * AO) + (size_t)h * d;
        else kr = base + (size_t)(r - P) * ld + AO + (size_t)h * d;
        float s = 0.f;
        for (int i = 0; i < d; i += 2) { const float2 kv = *reinterpret_cast<const float2*>(kr + i); s += qs[wave][i] * kv.x; s += qs[wave][i + 1] * kv.y; }
        s *= scale;
        sc[wave][jj] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    float l = 0.f;
    for (int jj = lane; jj < n; jj += 64) { const float p = expf(sc[wave][jj] - m); sc[wave][jj] = p; l += p; }
    l = wave_sum(l);
    __syncthreads();
    if (!valid) return;
    const int n_ring = HIST ? (P - j0 > 0 ? (P - j0 < n ? P - j0 : n) : 0) : 0;   // the first n_ring keys lie before the chunk
    for (int i = lane; i < d; i += 64) {
        float acc = 0.f;
        if constexpr (HIST) {
            if (n_ring > 0) {
                int slot = j0 % cap;
                for (int jj = 0; jj < n_ring; ++jj) {
                    acc += sc[wave][jj] * ring[(size_t)slot * (2 * AO) + AO + (size_t)h * d + i];
                    if (++slot == cap) slot = 0;
                }
            }
        }
        const float* vr = base + (size_t)(j0 + n_ring - P) * ld + 2 * AO + (size_t)h * d + i;
        for (int jj = n_ring; jj < n; ++jj) acc += sc[wave][jj] * vr[(size_t)(jj - n_ring) * ld];
        out[(size_t)(sp.off + t) * AO + (size_t)h * d + i] = acc / l;
    }
}
__global__ __launch_bounds__(256) void k_enc_attn(const float* qkv, float* out, int heads, int d, int window, float scale, const EncSpan* spans) {
    enc_attn_body<false>(qkv, out, heads, d, window, scale, spans, nullptr);
}
__global__ __launch_bounds__(256) void k_enc_attn_hist(const float* qkv, float* out, int heads, int d, int window, float scale, const EncSpan* spans, const EncHist* hist) {
    enc_attn_body<true>(qkv, out, heads, d, window, scale, spans, hist);
}
void launch_enc_attn(const float* qkv, float* out, int heads, int d, int window, float scale, const EncSpan* spans, int n_clips, int max_T, hipStream_t s,
                     const EncHist* hist) {
    if (n_clips < 1 || n_clips > 65535 || max_T < 1 || heads < 1) throw Error("encoder attention: bad shape");
    if (window < 1 || window > EA_WMAX || d < 2 || d > 128 || (d & 1)) throw Error("encoder attention: built for windows of up to 1024 rows and even head dims of up to 128");
    const int64_t tasks = (int64_t)max_T * heads;
    const dim3 grid((unsigned)((tasks + 3) / 4), n_clips);
    if (hist) hipLaunchKernelGGL(k_enc_attn_hist, grid, dim3(256), 0, s, qkv, out, heads, d, window, scale, spans, hist);
    else hipLaunchKernelGGL(k_enc_attn, grid, dim3(256), 0, s, qkv, out, heads, d, window, scale, spans);
    Q3_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// k_enc_carry_copy — a push's rows into the streams' carry rings, every stream of the push in one launch (blockIdx.y = table entry).
// Row i < rows of src (row stride src_ld floats) goes to ring slot (slot0 + i) mod cap, `width` floats.  The host passes at most cap
// rows per entry (the launcher's table is the host's; the kernel clamps rows to cap all the same), so no two rows of an entry share a
// slot, and a ring is only ever written from workspace rows: nothing moves inside a ring, whatever the push's size.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_enc_carry_copy(const EncCarryCopy* tab) {
    const EncCarryCopy c = tab[blockIdx.y];
    if (c.cap < 1 || c.width < 1) return;
    const int rows = c.rows < c.cap ? c.rows : c.cap;
    const bool vec = !((c.width | c.src_ld) & 3) && !(((uintptr_t)c.src | (uintptr_t)c.dst) & 15);
    const int per_row = vec ? c.width >> 2 : c.width;
    const int64_t total = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / per_row), e = (int)(i - (int64_t)r * per_row);
        const int slot = (int)(((int64_t)c.slot0 + r) % c.cap);
        if (vec) reinterpret_cast<float4*>(c.dst + (size_t)slot * c.width)[e] = reinterpret_cast<const float4*>(c.src + (size_t)r * c.src_ld)[e];
        else c.dst[(size_t)slot * c.width + e] = c.src[(size_t)r * c.src_ld + e];
    }
}
void launch_enc_carry_copy(const EncCarryCopy* tab, int n, int64_t max_floats, hipStream_t s) {
    if (!tab || n < 1 || n > 65535 || max_floats < 1) throw Error("encoder carry copy: bad table");
    const int64_t blocks = std::min<int64_t>((max_floats / 4 + 255) / 256 + 1, 1024);
    hipLaunchKernelGGL(k_enc_carry_copy, dim3((unsigned)blocks, n), dim3(256), 0, s, tab);
    Q3_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// k_rvq_encode — split residual VQ.  A workgroup owns RV_TF = 8 frames: both input projections (thread = output dim, the projection
// row read once for the 8 frames), then the level loop: thread = codebook row(s), the row read once and its squared distance to the 8
// residuals accumulated side by side (direct differences, no |a|^2 + |b|^2 - 2ab), per-thread running minimum (ascending rows, strict
// <), then a tree reduction per frame with the lower index winning a tie; the residual loses the chosen row.
// Tile size: a level's table (2 MB at 2048 x 256) is read once per workgroup, i.e. once per 8 frames, from L2: 8 keeps the 24
// per-thread accumulators / minima in registers without spilling, and a 10 s clip still spreads over 16 workgroups.  Whether 16
// frames per workgroup (half the L2 traffic, half the workgroups) is faster has not been measured.
// Dynamic LDS: residuals [2][8][D] floats + reduction scratch [8][256] (float, int).
// ------------------------------------------------------------------------------------------------
#define RV_TF 8
__global__ __launch_bounds__(256) void k_rvq_encode(const float* lat, int rows, int H, const float* proj_sem, const float* proj_ac, const float* books,
                                                    int G, int CB, int D, int32_t* codes) {
    extern __shared__ __attribute__((aligned(16))) float rv_lds[];
    float* res = rv_lds;                                  // [2][RV_TF][D]
    float* red_v = rv_lds + 2 * RV_TF * D;                // [RV_TF][256]
    int* red_i = (int*)(red_v + RV_TF * 256);             // [RV_TF][256]
    const int tid = threadIdx.x, row0 = blockIdx.x * RV_TF;
    const int nf = rows - row0 < RV_TF ? rows - row0 : RV_TF;   // >= 1 by the grid
    for (int q = 0; q < 2; ++q) {
        const float* P = q == 0 ? proj_sem : proj_ac;
        for (int dd = tid; dd < D; dd += 256) {
            float acc[RV_TF];
#pragma unroll
            for (int f = 0; f < RV_TF; ++f) acc[f] = 0.f;
            const float* pr = P + (size_t)dd * H;
            for (int hh = 0; hh < H; hh += 4) {
                const float4 w = *reinterpret_cast<const float4*>(pr + hh);
#pragma unroll
                for (int f = 0; f < RV_TF; ++f) {
                    if (f < nf) {
                        const float4 x = *reinterpret_cast<const float4*>(lat + (size_t)(row0 + f) * H + hh);
                        acc[f] += w.x * x.x; acc[f] += w.y * x.y; acc[f] += w.z * x.z; acc[f] += w.w * x.w;
                    }
                }
            }
#pragma unroll
            for (int f = 0; f < RV_TF; ++f) res[(q * RV_TF + f) * D + dd] = acc[f];
        }
    }
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        float* R = res + (g == 0 ? 0 : RV_TF * D);
        const float* book = books + (size_t)g * CB * D;
        float best[RV_TF]; int bidx[RV_TF];
#pragma unroll
        for (int f = 0; f < RV_TF; ++f) { best[f] = INFINITY; bidx[f] = INT_MAX; }
        for (int cb = tid; cb < CB; cb += 256) {
            float acc[RV_TF];
#pragma unroll
            for (int f = 0; f < RV_TF; ++f) acc[f] = 0.f;
            const float* er = book + (size_t)cb * D;
            for (int dd = 0; dd < D; dd += 4) {
                const float4 e = *reinterpret_cast<const float4*>(er + dd);
#pragma unroll
                for (int f = 0; f < RV_TF; ++f) {
                    const float4 r = *reinterpret_cast<const float4*>(R + f * D + dd);
                    const float d0 = r.x - e.x, d1 = r.y - e.y, d2 = r.z - e.z, d3 = r.w - e.w;
                    acc[f] += d0 * d0; acc[f] += d1 * d1; acc[f] += d2 * d2; acc[f] += d3 * d3;
                }
            }
#pragma unroll
            for (int f = 0; f < RV_TF; ++f) if (acc[f] < best[f]) { best[f] = acc[f]; bidx[f] = cb; }
        }
#pragma unroll
        for (int f = 0; f < RV_TF; ++f) { red_v[f * 256 + tid] = best[f]; red_i[f * 256 + tid] = bidx[f]; }
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int f = 0; f < RV_TF; ++f) {
                    const float v1 = red_v[f * 256 + tid + s], v0 = red_v[f * 256 + tid];
                    const int i1 = red_i[f * 256 + tid + s], i0 = red_i[f * 256 + tid];
                    if (v1 < v0 || (v1 == v0 && i1 < i0)) { red_v[f * 256 + tid] = v1; red_i[f * 256 + tid] = i1; }
                }
            }
            __syncthreads();
        }
        if (tid < nf) {
            const int id = red_i[tid * 256];
            codes[(size_t)(row0 + tid) * G + g] = id < CB ? id : 0;
        }
        for (int o = tid; o < RV_TF * D; o += 256) {
            const int f = o / D, dd = o - f * D;
            const int id = red_i[f * 256];
            if (id < CB) R[o] -= book[(size_t)id * D + dd];
        }
        __syncthreads();
    }
}
void launch_rvq_encode(const float* lat, int rows, int H, const float* proj_sem, const float* proj_ac, const float* books, int G, int CB, int D,
                       int32_t* codes, hipStream_t s) {
    if (rows < 1 || G < 1 || CB < 1) throw Error("rvq encode: bad shape");
    if (H < 4 || (H & 3) || D < 4 || (D & 3)) throw Error("rvq encode: hidden and codebook dims must be multiples of 4");
    const size_t lds = ((size_t)2 * RV_TF * D + (size_t)2 * RV_TF * 256) * sizeof(float);
    if (lds > 64 * 1024) throw Error("rvq encode: codebook dim too large for the residual tile in LDS");
    hipLaunchKernelGGL(k_rvq_encode, dim3((rows + RV_TF - 1) / RV_TF), dim3(256), lds, s, lat, rows, H, proj_sem, proj_ac, books, G, CB, D, codes);
    Q3_HIP_CHECK(hipGetLastError());
}

} // namespace q3
