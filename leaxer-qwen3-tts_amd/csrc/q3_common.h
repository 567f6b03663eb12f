// q3_common.h — shared declarations of libq3tts_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/q3tts.h"

typedef uint16_t bf16_t; // raw bf16 bits

#define Q3_HIP_CHECK(expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) throw q3::Error(std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

namespace q3 {

struct Error {
    std::string msg;
    explicit Error(std::string m) : msg(std::move(m)) {}
};

// A/B knobs of the measurement scripts and the test suite (Q3TTS_SEAM, Q3TTS_GEMM3_LA, Q3TTS_CONV_NO_PEEL, Q3TTS_ATTN_STREAM_*, ...; the
// full list is in INTEGRATION.md).  knob() answers like getenv() ONLY while at least one engine created with Q3TTS_FLAG_TEST_HOOKS is
// alive in the process, and nullptr otherwise: a stray environment variable cannot change which kernels a production engine launches.
// Read at every use (no caching): a test may flip a knob between two calls.  Defined in q3_engine.cpp.
const char* knob(const char* name);
struct KnobScope {   // member of Engine: holds the process-wide count of hook-enabled engines for the engine's lifetime
    bool on = false;
    void enable();
    ~KnobScope();
};

// fp32 -> bf16, round-to-nearest-even (inputs are finite weights)
inline bf16_t f32_to_bf16(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    return (bf16_t)u;
}
inline float bf16_to_f32(bf16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// G.711 (include/q3tts.h "G.711"): the laws on int16, integers only, shared by the host helpers and the kernels
// (pcm_sink_store, rs_stream_sample).  floor(log2 m) is 31 - clz(m); m >= 132 (mu-law) and a >= 32 (A-law) where it is taken.
__host__ __device__ inline int g711_log2(uint32_t v) { return 31 - __builtin_clz(v); }
__host__ __device__ inline uint8_t g711_mulaw_enc(int16_t s) {
    const int32_t mag = s < 0 ? -(int32_t)s : (int32_t)s;
    const uint32_t m = (uint32_t)(mag > 32635 ? 32635 : mag) + 132u;
    const int e = g711_log2(m) - 7;
    const uint32_t mant = (m >> (e + 3)) & 15u;
    return (uint8_t)(~((s < 0 ? 0x80u : 0u) | ((uint32_t)e << 4) | mant) & 0xFFu);
}
__host__ __device__ inline uint8_t g711_alaw_enc(int16_t s) {
    const int32_t mag = s < 0 ? -(int32_t)s : (int32_t)s;
    const uint32_t a = (uint32_t)(mag > 32767 ? 32767 : mag) >> 3;
    const int e = a < 32u ? 0 : g711_log2(a) - 4;
    const uint32_t mant = a < 32u ? a >> 1 : (a >> e) & 15u;
    return (uint8_t)(((s >= 0 ? 0x80u : 0u) | ((uint32_t)e << 4) | mant) ^ 0x55u);
}
__host__ __device__ inline int16_t g711_mulaw_dec(uint8_t b) {
    const uint32_t u = ~(uint32_t)b & 0xFFu;
    const int e = (int)(u >> 4) & 7;
    const int32_t m = (int32_t)((((u & 15u) << 3) + 132u) << e) - 132;
    return (int16_t)(u & 0x80u ? -m : m);
}
__host__ __device__ inline int16_t g711_alaw_dec(uint8_t b) {
    const uint32_t x = (uint32_t)b ^ 0x55u;
    const int e = (int)(x >> 4) & 7;
    const uint32_t mant = x & 15u;
    const int32_t m = e == 0 ? (int32_t)((mant << 4) + 8u) : (int32_t)(((mant << 4) + 0x108u) << (e - 1));
    return (int16_t)(x & 0x80u ? m : -m);
}
__host__ __device__ inline uint8_t g711_enc(int format, int16_t s) { return format == Q3TTS_PCM_MULAW ? g711_mulaw_enc(s) : g711_alaw_enc(s); }
__host__ __device__ inline int16_t g711_dec(int format, uint8_t b) { return format == Q3TTS_PCM_MULAW ? g711_mulaw_dec(b) : g711_alaw_dec(b); }
inline bool pcm_format_known(int format) { return format >= Q3TTS_PCM_F32 && format <= Q3TTS_PCM_ALAW; }
inline bool pcm_format_g711(int format) { return format == Q3TTS_PCM_MULAW || format == Q3TTS_PCM_ALAW; }
// bytes of one sample in a Q3TTS_PCM_* format
inline size_t pcm_format_bytes(int format) { return format == Q3TTS_PCM_F32 ? 4 : (format == Q3TTS_PCM_S16 ? 2 : 1); }
inline const char* pcm_format_name(int format) {
    return format == Q3TTS_PCM_F32 ? "float (Q3TTS_PCM_F32)" : format == Q3TTS_PCM_S16 ? "int16 (Q3TTS_PCM_S16)"
         : format == Q3TTS_PCM_MULAW ? "mu-law (Q3TTS_PCM_MULAW)" : "A-law (Q3TTS_PCM_ALAW)";
}

// ------------------------------------------------------------------------------------------------
// kernel argument blocks + launchers (q3_decode_kernels.hip)
// ------------------------------------------------------------------------------------------------

enum GemvEpi { EPI_STORE = 0, EPI_RESIDUAL = 1, EPI_SWIGLU = 2, EPI_BIAS = 3, EPI_BIAS_SILU = 4, EPI_SLAB = 5, EPI_SLAB2 = 6 };

// out[m][n] = epi( sum_k xin[m][k] * W[n][k] ),  W row-major bf16 [N][K] (nn.Linear.weight layout)
struct GemvArgs {
    const bf16_t* W = nullptr;   // [N][K]
    const bf16_t* W2 = nullptr;  // EPI_SWIGLU: up_proj rows (W = gate_proj)
    const float* x = nullptr;    // [M][ldx]
    int ldx = 0;
    const float* gamma = nullptr; // non-null: fused RMSNorm of x rows (gamma[K], eps)
    float eps = 0.f;
    float* xn_out = nullptr;      // optional: normalised rows written by block 0 (ld_xn)
    int ld_xn = 0;
    const float* bias = nullptr;  // EPI_BIAS / EPI_BIAS_SILU
    const float* res = nullptr;   // EPI_RESIDUAL (may alias out)
    int ldres = 0;
    float* out = nullptr;
    int ldo = 0;
    int M = 0, N = 0, K = 0;
    int epi = EPI_STORE;
    bool nt = false;              // non-temporal weight loads (streamed-once weights)
    bool xlds = true;             // fast path, rows as they lie in memory: each wave loads a quarter of the activation rows (and of gamma), the workgroup
                                  // shares them through LDS; false: every wave loads them whole (Q3TTS_GEMV_XLDS=0, the A/B knob).  Same bits.
    // optional: x rows are the combination of split-T attention partials (o_proj prologue)
    const float* po = nullptr;    // [(row*heads + h)*S + s][d] un-normalised sum(p*v)
    const float* pm = nullptr;    // [(row*heads + h)*S + s] running max
    const float* pl = nullptr;    // [(row*heads + h)*S + s] running sum
    int pS = 0, pchunk = 0, pn_new = 1, pslot_offset = 0, pheads = 0, pd = 0;
    const int* ppos_dev = nullptr;
    int ppos_scalar = 0;
    // optional (gate/up, fast path): the activation rows are x + the o_proj partial rows of the 8 kv heads, psum[(h * M + m) * K + k],
    // summed in kv-head order; every workgroup stores its slice of that sum to xmid [M][K] (the down projection's residual)
    const float* psum = nullptr;
    float* xmid = nullptr;
    bool psum_lead = true;        // psum launches: x, the partial rows and gamma (one 16-byte unit per thread, shared through LDS) are issued ahead of the
                                  // weight loads; false: behind them, gamma whole in every wave (Q3TTS_GEMV_PSUM_LEAD=0, the A/B knob).  Same bits.
};
void launch_gemv(const GemvArgs& a, hipStream_t s);
bool gemv_fast_path(const GemvArgs& a); // single-pass kernel available (M <= 2, K in {1024,2048,3072})
bool gemv16_ok(const GemvArgs& a);        // 3..16 rows on the matrix cores, same contract (q3_gemm_kernels.hip); launch_gemv picks it
void launch_gemv16(const GemvArgs& a, hipStream_t s);
// Fragment-packed copies of the bf16 weight matrices for the matrix-core decode kernels (k_gemv16, k_gemm3; round 5).  The B operand of
// v_mfma_f32_16x16x32_bf16 wants lane (r16, q) to hold row n0 + r16, k = 32 s + 8 q .. + 7: read from the row-major [N][K] matrix that is
// 16 rows x 64 bytes per load instruction — sixteen half-used 128-byte lines.  The packed copy stores, for every (16-row tile t, k-step s),
// the 64 lanes' 16 bytes back to back: P[((t K/32 + s) 64 + lane) 8 + e] = W[min(16 t + (lane & 15), N - 1)][32 s + 8 (lane >> 4) + e], so a
// load instruction is ONE contiguous KB (eight whole lines).  Same values into the same registers: results are bit-identical.  The kernels
// find the copy through a process-wide registry keyed by the row-major pointer (engines register at finalize, unregister when destroyed);
// Q3TTS_PACKED_W=0 (A/B knob) ignores it.
void launch_pack_mfma_b(const bf16_t* W, bf16_t* P, int N, int K, hipStream_t s);
size_t packed_mfma_b_elems(int N, int K);
void register_packed_weight(const bf16_t* W, const bf16_t* P);
void unregister_packed_weight(const bf16_t* W);
const bf16_t* find_packed_weight(const bf16_t* W);   // nullptr: none (or the knob says no)

// Decode-time attention over a paged fp32 KV cache with the new tokens' q/k-norm + RoPE + append fused.
struct AttnArgs {
    const float* qkv = nullptr; // [nb*n_new][ld_qkv]: q heads | k heads | v heads (raw projections)
    int ld_qkv = 0;
    // deferred RMSNorm of the projection's input (split-K seam, GemmArgs::seam): the raw q / k / v sums are scaled by
    // 1 / sqrt(sum_t ssq_in[row][t] / ssq_K + ssq_eps) before anything else.  Null: the input planes were normalised.
    const float* ssq_in = nullptr; int ssq_nt = 0, ssq_K = 0; float ssq_eps = 0.f;
    int qkv_nslab = 1; size_t qkv_slab_stride = 0; // > 1: qkv is the sum of that many split-K partial slabs
    float* out = nullptr;       // [nb*n_new][nq*d]
    int ld_out = 0;
    float* kcache = nullptr;    // [page][layer][kvh][page_tokens][d]
    float* vcache = nullptr;
    bool kv_bf16 = false;       // the caches hold bf16 (2 bytes per element, same element layout); rounded on append, fp32 math
    bool kv_round = false;      // fp32 caches holding bf16-ROUNDED values (Q3TTS_FLAG_KV_ROUND_BF16): what kv_bf16 computes, without the 16-bit storage
    const int* page_table = nullptr; // [slot][pages_per_slot]
    int pages_per_slot = 0, page_shift = 0;
    bool identity_pages = false;     // page_table[slot][i] == slot * pages_per_slot + i by construction (code predictor): kernels may skip the table
    int layer = 0, n_layers = 0;
    const float* q_norm = nullptr; // [d] or null
    const float* k_norm = nullptr;
    float eps = 0.f;
    const float* rope_cos = nullptr; // [max_pos][d/2]
    const float* rope_sin = nullptr;
    const int* pos_dev = nullptr;    // per-slot position of new token 0 (device) or null -> pos_scalar
    int pos_scalar = 0;
    int slot_offset = 0, nb = 0, n_new = 0;
    const int* slot_map = nullptr; // optional: batch row bi belongs to slot slot_map[bi] instead of slot_offset + bi (prefill of scattered slots)
    int nq = 0, nkv = 0, d = 0;
    float scale = 0.f;
    int window = 0;
    int new_from_raw = 1; // 1: new tokens' K/V come from qkv (and are appended); 0: everything is in the cache, q pre-roped
    // split-T mode: n_splits workgroups per (kv head, new token, row), each over `chunk` tokens, write
    // un-normalised partials instead of `out`; combined by the o_proj GEMV prologue or launch_attn_combine
    int n_splits = 1, chunk = 1 << 30;
    float* po = nullptr; float* pm = nullptr; float* pl = nullptr;
    // optional (hi, lo) bf16 plane outputs of launch_attn_combine for the MFMA GEMM path
    bf16_t* oh = nullptr; bf16_t* ol = nullptr; int ldp = 0;
    // 1: k_attn_stream — the batched step's long-context kernel (one new token per row, d = 128, splits on page boundaries, K/V walked in
    // a two-deep register ring); the engine asks for it where the launch is bound by the KV bytes it streams
    int stream = 0;
    // launch_attn_prefill's segment form (ragged prefill): the chunk's n_new rows belong to n_seg segments.  Device tables of ints:
    // seg [n_seg][4] = {slot, cache position of the segment's first row, first row in the chunk, n_rows}, row_seg [n_new] = row -> segment,
    // tiles [n_tiles][2] = {segment, first row of the tile within the segment}.  Null: the one-slot / group forms.
    const int* seg = nullptr; const int* row_seg = nullptr; const int* tiles = nullptr; int n_seg = 0, n_tiles = 0;
};
void launch_attn(const AttnArgs& a, hipStream_t s);
// code-predictor attention + o_proj (+ residual) for one utterance: see k_cp_attn_oproj
struct CpAttnOprojArgs {
    const float* qkv = nullptr; int ld_qkv = 0; // [n_new][ld_qkv] raw q | k | v projections
    float* kc = nullptr; float* vc = nullptr;    // this (slot, layer)'s cache rows: [nkv][page_tokens][d]
    int page_tokens = 0;
    int base = 0;                                // tokens already cached = position of new row 0
    const float* q_norm = nullptr; const float* k_norm = nullptr; float eps = 0.f;
    const float* rope_cos = nullptr; const float* rope_sin = nullptr;
    float scale = 0.f;
    int nq = 0, nkv = 0, d = 0;
    const bf16_t* W = nullptr; int K = 0, N = 0; // o_proj [N][K]
    float* x = nullptr; int ldx = 0;             // residual stream rows [n_new][ldx], updated in place
    bool lead = true;                            // launch_cp_attn_kvh: the attention's operands are issued ahead of the o_proj weight loads; false: the
                                                 // weights first (Q3TTS_CP_KVH_LEAD=0, the A/B knob).  Same bits.
};
bool cp_attn_oproj_ok(const CpAttnOprojArgs& a, int n_new);
void launch_cp_attn_oproj(const CpAttnOprojArgs& a, int n_new, hipStream_t s);
// o_proj split by kv head (b = 1): one fp32 partial row per (kv head, row) into part[(h * n_new + m) * N], x left as it is; the gate/up
// GEMV adds them (GemvArgs::psum).  The predictor's attention + o_proj (same shapes as cp_attn_oproj_ok), and the talker's split-T merge +
// o_proj (a COMB GemvArgs of one row)
void launch_cp_attn_kvh(const CpAttnOprojArgs& a, int n_new, float* part, hipStream_t s);
bool oproj_kvh_ok(const GemvArgs& a);
void launch_oproj_kvh(const GemvArgs& a, float* part, hipStream_t s);
void launch_attn_combine(const AttnArgs& a, hipStream_t s); // partials -> a.out
// Long-prompt prefill (run_prefill, reference tts_onnx.cpp:615-665, past 16 rows): a chunk of n_new <= 128 rows of ONE slot (nb = 1, slot =
// slot_offset) at the host-known position pos_scalar.  Two launches: the rows' K / V appended (k_attn's prologue, same rounding point),
// then causal attention of every row over cache tokens [0, pos_scalar + its index] read from the cache alone.  n_splits = 1: normalised
// rows (out) and / or planes (oh, ol).  Group form (slots begun behind a shared prefix): nb members of n_new <= 16 rows, nb * n_new <= 128,
// member bi in slot slot_map[bi] (slot_offset + bi without a map) at its own base pos_dev[bi] (device); pos_scalar then carries the
// largest of those bases for the launch's bounds check.  Segment form (a.seg non-null, ragged prefill): nb = 1, the n_new <= 128 rows
// are cut into segments of any lengths, slots and bases (AttnArgs::seg); a tile of query rows never straddles two segments, so the
// per-row arithmetic is the one-slot form's and a chunk of one segment gives its bits.  The caller (host) vouches that every segment
// fits its slot's pages; the kernels skip one that does not.
void launch_attn_prefill(const AttnArgs& a, hipStream_t s);
bool attn_prefill_seg_ok(int d, int nq, int nkv);   // the segment form is built for these dims
int attn_prefill_tile_rows(int nq, int nkv);        // TQ: query rows per tile (16, or 8 for GQA groups of 3-4)
// dst row i = src row idx[i] (device indices): the rows a ragged chunk hands to the codec head
void launch_gather_rows_f32(const float* src, int lds, const int* idx_dev, int n, float* dst, int ldd, int cols, hipStream_t s);
// KV rows of positions [0, P) between a slot's pages and a compact store [layer][kvh][P][d] (k_kv_prefix_copy)
struct KvPrefixCopyArgs {
    void* kcache = nullptr; void* vcache = nullptr;   // [page][layer][kvh][64][d], either element type
    void* kstore = nullptr; void* vstore = nullptr;   // [layer][kvh][P][d], the same element type
    const int* page_table = nullptr; int pages_per_slot = 0;
    const int* slots = nullptr; int n_dst = 1;         // scatter: the destination slots (device); gather: null, one source slot0
    int slot0 = 0, scatter = 0;
    int n_lk = 0;                                      // n_layers * n_kv_heads
    int P = 0, row16 = 0;                              // positions; 16-byte units per token row
};
void launch_kv_prefix_copy(const KvPrefixCopyArgs& a, hipStream_t s);

// Skinny-M bf16-MFMA GEMM (q3_gemm_kernels.hip): activations as (hi, lo) bf16 planes, fp32 accumulate
struct GemmArgs {
    const bf16_t* W = nullptr;   // [N][K]
    const bf16_t* W2 = nullptr;  // EPI_SWIGLU: up_proj rows
    const bf16_t* xh = nullptr;  // [M][ldx] hi plane
    const bf16_t* xl = nullptr;  // [M][ldx] lo plane
    int ldx = 0;
    const float* res = nullptr; int ldres = 0;
    const float* bias = nullptr;
    float* out = nullptr; int ldo = 0;        // fp32 output (may be null when only planes are wanted)
    float* out2 = nullptr;                    // EPI_SLAB2: slabs of the W2 product
    bf16_t* oh = nullptr; bf16_t* ol = nullptr; int ldp = 0; // optional plane outputs (input of the next GEMM)
    int M = 0, N = 0, K = 0, epi = EPI_STORE;
    int slab_rows = 0;   // EPI_SLAB / EPI_SLAB2: rows per slab (0 = M); launch_gemm2 sets it when it cuts M into 128-row blocks
    bool nt = false;     // non-temporal weight loads (weights this step reads once: the talker's)
    bool w_packed = false;      // W / W2 point at fragment-packed copies (set by launch_gemm3 from the registry)
    bool plain_slabs = false;   // A/B knob Q3TTS_GEMM_PLAIN_SLABS: k_gemm3's slabs as plain stores instead of write-through (sc1)
    // ---- split-K seam (k_gemm3 only): the slabs are reduced INSIDE the launch by the K-slice workgroups of a column tile themselves
    // (sc1 slab stores, a flag per slice, slice s < 16-row-chunk count owns chunk s once every flag is set), instead of by a k_finish* launch.
    // seam 1: x += sum(slabs); planes = split(gamma * x) — NOT normalised: the consumer applies 1/rms from the per-(row, tile) sums of
    //         squares written to ssq_out (deferred RMSNorm, as k_gemv16 does);
    // seam 2: planes = split(silu(r * sum(gate slabs)) * (r * sum(up slabs))), r = 1/rms of the INPUT planes' rows from ssq_in.
    int seam = 0;
    unsigned* seam_cnt = nullptr;                    // one 64-byte line per (column tile, row block): words 0..11 slice flags, 12..15 abandoned-chunk marks
    const unsigned* seam_gen = nullptr;              // the step's generation (bumped once per step by the first sampler): every word a launch writes carries it,
                                                     // so nothing is ever reset and a copy of the line left over from an earlier step can never read as set
    int seam_spin = 512;                             // polls an owner makes before it abandons its chunk (~0.7 us each)
    float* sx = nullptr; int sldx = 0;               // seam 1: residual stream rows, updated in place
    const float* sgamma = nullptr;                   // seam 1: the consumer's RMSNorm gain
    float* ssq_out = nullptr; int ssq_nt = 0;        // seam 1: [M][ssq_nt] partial sums of squares, one per 64-column tile
    const float* ssq_in = nullptr; int ssq_in_nt = 0; float seps = 0.f;   // seam 2 (K = this GEMM's K): the input rows' partial sums of squares
};
void launch_gemm2(const GemmArgs& a, int ksplit, int nw, hipStream_t s); // EPI_SLAB: out = slabs [ksplit][M][ldo]
bool gemm_seam_ok(const GemmArgs& a, int ksplit);                        // the in-launch split-K reduction (GemmArgs::seam) covers this launch
void launch_finish(float* x, int ldx, const float* slab, int nslab, size_t slab_stride, int ld_slab, const float* gamma, float eps,
                   int rows, int K, bf16_t* oh, bf16_t* ol, int ldp, float* xn_out, int ld_xn, hipStream_t s);
void launch_finish_swiglu(const float* gs, const float* us, int nslab, size_t slab_stride, int rows, int N,
                          bf16_t* oh, bf16_t* ol, int ldp, hipStream_t s);

struct SlotState { // device-resident per-slot generation state
    int32_t n_frames;     // frames recorded so far
    int32_t finished;     // 1 after EOS / max_frames
    int32_t active;       // slot armed
    int32_t prompt_len;
    int32_t trailing_len;
    int32_t max_frames;
    int32_t top_k;
    int32_t ignore_eos;
    float temperature, top_p;
    uint32_t stream_id;
    float rep_penalty;    // repetition penalty on code0 (group 0 sampler); 0 and 1 = off
    uint64_t seed;
    int32_t prefix_len;   // rows of a shared prompt prefix in front of the prompt (0: none): the talker position is prefix_len + prompt_len + frame
    uint32_t text_open;   // 0: frames at or beyond trailing_len take tts_pad; 1: more text may arrive (live text), the slot stalls there instead
};                        // 64 bytes: read by the sampler as four 16-byte loads
static_assert(sizeof(SlotState) == 64, "SlotState must be 64 bytes");

struct SampleArgs {
    const float* logits = nullptr; // [nb][ld]
    int ld = 0, V = 0, nb = 0;
    int nslab = 1; size_t slab_stride = 0; // > 1: the logits are the sum of that many split-K partial slabs (batched predictor heads), summed in slab order
    int sup_begin = 0, sup_end = 0, eos_id = -1; // suppress [sup_begin,sup_end) except eos_id (group 0 only)
    int group = 0, n_groups = 0;
    SlotState* st = nullptr;       // [nb]; null -> standalone mode (params below, token_out)
    float temperature = 1.f, top_p = 1.f;
    int top_k = 0;
    float u = 0.f;
    const float* u_dev = nullptr;   // standalone mode, optional: row b draws with u_dev[b] instead of u (q3tts_sample_dev)
    int suppress = 0;
    int64_t* token_out = nullptr;
    // repetition penalty (group 0 / standalone rows only; both null -> the sampler instantiation without the penalty step).
    // generation mode: seen = per-slot bitmaps of the code0 ids the utterance has emitted, [nb][seen_ld] words, seen_ld >= ceil(V / 32);
    // the sampler reads row b, penalises by SlotState::rep_penalty and sets the bit of the id it records.
    // standalone mode: hist = ids already used, [nb][hist_ld] (ids outside [0, V) are ignored), hist_len[b] of them valid; rep_penalty.
    uint32_t* seen = nullptr; int seen_ld = 0;
    const int64_t* hist = nullptr; int hist_ld = 0; const int32_t* hist_len = nullptr;
    float rep_penalty = 1.f;
    // fused epilogue (generation mode)
    const bf16_t* embed = nullptr; // [V][H] embedding table of the sampled codebook
    int H = 0;
    float* x_next = nullptr;       // row b*ld_xnext: embedding of the sampled token (next predictor input)
    int ld_xnext = 0;
    float* sum = nullptr;          // [nb][H] running fp32 sum of the frame's 16 embeddings
    float* x_talk = nullptr;       // [nb][H], last group only: sum + text row | tts_pad
    const float* trailing = nullptr; // [nb][max_trailing][H]
    int max_trailing = 0;
    const float* tts_pad = nullptr;  // [H]
    int32_t* codes = nullptr;      // [nb][max_frames_cap][n_groups]
    int max_frames_cap = 0;
    int32_t* talker_pos = nullptr; // [nb], last group only: position of the token the talker decodes next
    // optional (batched step with the split-K seam): the sampler also prepares the NEXT predictor pass's input planes, so that the pass
    // needs no RMSNorm launch in front of its first projection — (hi, lo) planes of gamma0 * row (NOT normalised: deferred RMSNorm) and
    // the row's sum of squares in ssq_out[row * ssq_nt + 0] (the other ssq_nt - 1 partials zero).  Row of utterance b: b * pl_row_mul +
    // pl_row_add.  lh (group 0 only): the talker's last_hidden rows [nb][ld_lh], which pass 0 takes as row b * 2.
    bf16_t* pl_h = nullptr; bf16_t* pl_l = nullptr; int pl_ldp = 0;
    const float* gamma0 = nullptr;
    float* ssq_out = nullptr; int ssq_nt = 0;
    int pl_row_mul = 1, pl_row_add = 0;
    const float* lh = nullptr; int ld_lh = 0;
    unsigned* step_gen = nullptr;  // group 0 only: the step's generation counter (split-K seam flags), bumped by workgroup 0
    // optional (one-slot engines, groups 1 .. n_groups - 2): the next predictor pass's layer-0 QKV projection, looked up instead of
    // computed — qkv_tab [V][qkv_n] is this group's slab of Engine::cp_qkv_tab, row `token` is copied to qkv_out [qkv_n]
    const float* qkv_tab = nullptr; float* qkv_out = nullptr; int qkv_n = 0;
};
void launch_sample(const SampleArgs& a, hipStream_t s);

// Frames that were not sampled here -> the talker input rows the sampler's fused epilogue would have left in x_talk for them (reference
// tts_onnx.cpp:824-842): row i = codec_embed[code0] + cp_embed[0][sub0] + ... + cp_embed[n_groups - 2][sub_last] (fp32, in that order)
// + the text row of frame frame0 + i.  One workgroup per frame of ONE slot.  Optionally the launch also records the frames as the
// sampler does: the ids as int32 into codes_out [n][n_groups] and the code0 bits into the slot's repetition-penalty bitmap.
struct FrameRowsArgs {
    const int64_t* codes = nullptr;  // [n][n_groups] (device), validated by the caller; the kernel clamps them all the same
    int n = 0, n_groups = 0, H = 0;
    const bf16_t* embed0 = nullptr; int V0 = 0;       // codec_embed_w [V0][H]
    const bf16_t* embed_sub[31] = {}; int SV = 0;     // cp_embed_w[g - 1] [SV][H]; launch_frame_rows points the unused entries at the last table
    const float* trailing = nullptr; // [.][H]: row i is the text row of frame frame0 + i (read while frame0 + i < trailing_len)
    int frame0 = 0, trailing_len = 0;
    const float* tts_pad = nullptr;  // [H]
    float* out = nullptr; int ldo = 0;
    int32_t* codes_out = nullptr;    // optional
    uint32_t* seen = nullptr;        // optional: the slot's bitmap row, >= ceil(V0 / 32) words
};
void launch_frame_rows(FrameRowsArgs a, hipStream_t s);

void launch_gather_rows_bf16(const bf16_t* table, int H, const int64_t* ids_dev, int n, float* out, int ldo, hipStream_t s);
void launch_fill_synth(void* dst, int is_bf16, int64_t n, uint64_t key, float mean, float stddev, hipStream_t s);
void launch_bf16_to_f32(const bf16_t* src, float* dst, int64_t n, hipStream_t s);
void launch_copy_rows(const float* src, int lds, float* dst, int ldd, int rows, int cols, hipStream_t s);
// rows whose flag is 0 are skipped (flags: device ints, one per row)
void launch_copy_rows_masked(const float* src, int lds, float* dst, int ldd, int rows, int cols, const int* flags_dev, hipStream_t s);
void launch_bump_u32(unsigned* counter, hipStream_t s);   // *counter += 1 (the split-K seam's step generation outside the fused step)
void launch_count_active(const SlotState* st, int nb, int32_t* out, hipStream_t s);

// Live text (reference tts_onnx.cpp:531-536 builds the trailing block once; :833-842 reads row `frame` of it): new text rows of n slots
// go behind the rows each slot already holds, in one launch.  desc: n records of 8 ints {slot, src0, n_rows, dst0, close, 0, 0, 0} —
// rows [src0, src0 + n_rows) of `rows` ([.][H], end to end) land in trailing[slot][dst0 .. dst0 + n_rows); with close the tts_eos row
// follows them; then SlotState::trailing_len = dst0 + n_rows + close and text_open = !close.  Rows at or past max_trailing are dropped
// (the caller validates; the kernel never writes outside the slot's block).
struct TextScatterArgs {
    const float* rows = nullptr; const int32_t* desc = nullptr; int n = 0, max_rows = 0;   // max_rows: the largest n_rows + close of the call
    float* trailing = nullptr; int max_trailing = 0, H = 0, n_slots = 0;
    const float* tts_eos = nullptr;
    SlotState* st = nullptr;
};
void launch_text_scatter(const TextScatterArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// codec decoder launchers (q3_codec_kernels.hip)
// ------------------------------------------------------------------------------------------------
struct ConvArgs { // out[t][co] = epi(bias[co] + sum_{tap,ci} W[tap][co][ci] * in[src_t(t,tap)][ci])
    const float* in = nullptr; int T_in = 0, C_in = 0;
    float* out = nullptr;      int T_out = 0, C_out = 0; // out may be null when only out2 is wanted
    const float* W = nullptr;  // [taps][C_out][C_in] fp32
    const bf16_t* Wh = nullptr; const bf16_t* Wl = nullptr; // optional (hi, lo) fp16 planes of W * 2^k: selects the split-precision MFMA kernel
    float w_scale_inv = 1.0f;                                  // 2^-k
    bool w_lo_zero = false, w2_lo_zero = false;                // the lo plane of W (W2) is identically zero: two matrix-core products instead of three, exact
    const float* bias = nullptr;
    int taps = 1, dil = 1;
    int transposed = 0, stride = 1, left = 0; // transposed: out index jo = m*stride + phase - left
    int act = 0;                 // 0 none, 1 GELU(erf), 2 SiLU, applied to (acc + bias)
    const float* mul = nullptr;  // optional elementwise multiplier after act (SwiGLU up branch)
    const float* res_scale = nullptr; // optional per-channel scale (LayerScale / ConvNeXt gamma)
    const float* res = nullptr;  // optional residual (same shape as out, may alias out)
    int clamp = 0;               // clamp to [-1, 1]
    float* out2 = nullptr;       // optional second output: SnakeBeta(value) for the NEXT layer
    const float* snake_alpha = nullptr;
    const float* snake_beta = nullptr;
    bool in_planes = false, out2_planes = false;   // `in` / `out2` hold, per 4 channels, 4 hi + 4 lo fp16 halves in place of the 4 floats (k_conv_split; see ConvKArgs)
    const float* snake_pre = nullptr;   // [2][C_out]: exp(alpha) | 1 / (exp(beta) + 1e-9), launch_snake_pre (split-precision path)
    float* slab = nullptr; size_t slab_floats = 0; // optional scratch for split-K partial sums of short 1-tap GEMMs ([slice][T_out][C_out])
    // fused residual unit (96-channel decoder block): out = res + bias2 + W2 . snake_mid(bias + W . in) — the 7-tap conv, the SnakeBeta
    // between, the 1x1 conv and the residual add in ONE launch; the intermediate never leaves the CU.  W2 = the 1x1 conv's [1][C_out][C_out]
    const float* W2 = nullptr; const bf16_t* W2h = nullptr; const bf16_t* W2l = nullptr; float w2_scale_inv = 1.0f;
    // Round 5, line-friendly copies of the weight planes (same values; launch_repack_planes_cm / launch_pack_w2_frags at finalize):
    // Whc = the (hi, lo) planes CHUNK-major, [plane][tap][C_in / 32][C_out][32]: a workgroup's weight tile of one (tap, 32-channel chunk)
    // is contiguous (96 rows x 64 B = 6 KB) instead of 96 separate 64-byte row pieces — k_conv_split's 32-wide-chunk kernels stage it with
    // whole-line loads (the 128-wide-chunk kernels of the short GEMMs keep the row-major planes: their rows are 256 B already);
    // W2fh / W2fl = the fused unit's 96 x 96 second conv in MFMA B-fragment order, [k-step][32-column block][lane][8]: the unit's weight
    // fragments come straight from global memory, one contiguous KB per load instead of 32 rows x 32 bytes.
    const bf16_t* Whc = nullptr; const bf16_t* W2fh = nullptr; const bf16_t* W2fl = nullptr;
    const float* bias2 = nullptr; const float* mid_alpha = nullptr; const float* mid_beta = nullptr; const float* mid_pre = nullptr;
    int batch = 1;               // independent sequences of the same shape: sequence u at in + u * in_ustride, out / out2 / res / mul at + u * T_out * C_out
    size_t in_ustride = 0;       // floats between the sequences' inputs (0: T_in * C_in, i.e. densely packed)
};
void launch_conv(const ConvArgs& a, hipStream_t s);
void cout1_debug_buffer(const float** p, size_t* n);   // experiment hook (Q3TTS_COUT1_PACKED=2)
void launch_split_planes(const float* w, bf16_t* hi, bf16_t* lo, size_t n, float scale, hipStream_t s);
void launch_snake_pre(const float* alpha, const float* beta, float* pre /* [2][C] */, int C, hipStream_t s);
void launch_repack_planes_cm(const bf16_t* planes /* [2][taps][cout][cin] */, bf16_t* out /* [2][taps][cin/32][cout][32] */, int taps, int cout, int cin, size_t plane_elems, hipStream_t s);
void launch_pack_w2_frags(const bf16_t* plane /* [C][C] */, bf16_t* out /* [C/16][C/32][64][8] */, int C, hipStream_t s);
void launch_absmax(const float* w, size_t n, unsigned* out, hipStream_t s);
void launch_or_mag16(const bf16_t* p, size_t n, unsigned* out /* |= magnitude bits */, hipStream_t s);
void launch_repack_conv(const float* w, float* out, int cin, int cout, int k, int transposed, hipStream_t s);
void launch_code_embed_mean(const float* table, const int32_t* codes, int F, int G, int codebook, int C, float* out, hipStream_t s,
                            int n_utt = 1, size_t codes_stride = 0, const int* perm = nullptr);
void launch_rmsnorm_rows(const float* x, const float* w, float eps, int rows, int C, float* out, hipStream_t s);
void launch_rope_store(float* qkv, int ld, int T, int nq, int nkv, int d, const float* cs, const float* sn,
                       float* kc, float* vc, int P, hipStream_t s, int n_utt = 1);
void launch_dwconv_ln(const float* x, int T, int C, const float* dw_w, const float* dw_b, const float* ln_w,
                      const float* ln_b, float* out, hipStream_t s, int rows_per_utt = 0);

// ---- batched carried-state push (Engine::codec_stream_push_batch): n new frames for each of g streams in one set of launches ----
// Activation rows are packed [stream][its new frames]; a table of these descriptors, uploaded once per push, tells every kernel that
// looks at a position or at a stream's own buffers where stream blockIdx.z (or .y) lives.  Grids cover the longest n; workgroups
// beyond a stream's n exit.
struct CodecStreamDesc {
    float* kv = nullptr;              // the stream's sliding K / V buffer [layer][k | v][head][P][d]
    float* hpost = nullptr;           // its kept transformer output rows [h_cap][hidden]
    const int32_t* codes = nullptr;   // the new frames' codes [n][groups] (device)
    int32_t P = 0;                    // rows per (layer, k | v, head) block of kv
    int32_t k0 = 0, h0 = 0;           // first new row in kv / in hpost
    int32_t a0 = 0;                   // absolute position of the first new frame (RoPE)
    int32_t n = 0, row_off = 0;       // new frames, first packed row
    int32_t ctx = 0, blk = 0;         // stages behind the transformer: kept rows in front of the new ones, sequence index in its group's block
};
void launch_code_embed_mean_streams(const float* table, const CodecStreamDesc* descs, int g, int n_max, int G, int codebook, int C, float* out, hipStream_t s);
void launch_rope_store_streams(float* qkv, int ld, const CodecStreamDesc* descs, int g, int n_max, int layer, int nq, int nkv, int d,
                               const float* cs, const float* sn, hipStream_t s);
// sliding-window attention of the packed rows over each stream's own cache (q roped, K / V stored: after launch_rope_store_streams)
void launch_attn_streams(const float* qkv, int ld_qkv, float* out, int ld_out, const CodecStreamDesc* descs, int g, int n_max, int layer,
                         int heads, int d, int window, float scale, hipStream_t s);
bool attn_streams_windowed(int heads, int d, int window, int ld_qkv, int ld_out);   // launch_attn_streams covers these dims (k_attn_win's sibling); others keep k_attn, stream by stream
void launch_rmsnorm_rows_streams(const float* x, const float* w, float eps, const CodecStreamDesc* descs, int g, int n_max, int C, hipStream_t s);   // row -> hpost[h0 + t]
// out [g][Tw][C]: sequence blk = the stream's hpost rows [h0 - ctx, h0 + n), zeros behind them
void launch_gather_stream_rows(const CodecStreamDesc* descs, int g, int Tw, int C, float* out, hipStream_t s);
// ---- priming (Engine::codec_stream_prime_batch): the tails a stream keeps, out of the whole-utterance layout into the streams' own buffers ----
// The descriptors read here: kv, hpost, P (the stream's own), n (frames primed), row_off (first of its rows [stream][Fp]), blk (its scratch
// K / V block).  Sources are the scratch K / V of one layer ([stream][head][Ps][d], after launch_rope_store) and the normalised output rows;
// a stream's buffers are only written: rows [0, min(n, keep)) of layer `layer`'s K and V, rows [0, min(n, ctx)) of hpost.  n == 0: untouched.
void launch_prime_kv_tails(const float* kc, const float* vc, int Ps, const CodecStreamDesc* descs, int g, int layer, int nkv, int d, int keep, hipStream_t s);
void launch_prime_row_tails(const float* h, const CodecStreamDesc* descs, int g, int C, int ctx, hipStream_t s);

// ---- PCM sinks (q3_codec.cpp): 24 kHz float PCM -> the sink's rate and format, band-limited, with carried state ----
// One sink of one push.  The samples the sink has are its carry (the last `n_before - carry_abs0` samples before this push) followed
// by the push's n_new samples at x_new (device; the vocoder's PCM where it lies, or staged host samples).  Output i of the launch is the
// sink's absolute output j = out0 + i: kc = floor(j M / L), p = (j M) mod L, y = sum_t tab[p][t] * x[kc - half + 1 + t], t ascending in
// fp32, x[k] = 0 for k < 0 and k >= n_total (which only a finishing push reaches).  taps == 0 (24 kHz): y[j] = x[j].  The result is
// written to out[i] as float, as int16 by the CLI's rule (clip to [-1, 1], (int16_t)(v * 32767.0f)), or as the G.711 byte of that int16.  Threads [n_out, n_out + keep)
// write the sink's next carry, the last `keep` samples of (carry, new), into carry_out: the other of the sink's two carry buffers.
struct PcmSinkDesc {
    const float* carry_in = nullptr; float* carry_out = nullptr;
    const float* x_new = nullptr;       // n_new samples (never null: a push without samples points at the carry)
    const float* tab = nullptr;         // [L][taps] on the device
    void* out = nullptr;                // n_out samples in the sink's format
    int64_t carry_abs0 = 0;             // absolute index of carry_in[0]
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push
    int64_t out0 = 0;                   // absolute index of the first new output
    int32_t n_new = 0, n_out = 0, keep = 0;   // keep == 0: the carry stays
    int32_t L = 1, M = 1, half = 0, taps = 0, format = 0;   // format: Q3TTS_PCM_* of `out`
    int32_t tab_lds = 0;                // the table's rows are staged in LDS (pcm_sink_tab_in_lds)
};
constexpr int kPcmSinkLdsX = 256 * 6 + 192 + 8;      // inputs of 256 outputs at the lowest rate (M / L <= 6, taps <= 192)
constexpr int kPcmSinkLdsTab = 12288;                // floats of table (rows padded to an odd stride) kept in LDS
inline int pcm_sink_tab_stride(int taps) { return taps | 1; }
inline bool pcm_sink_tab_in_lds(int L, int taps) { return taps > 0 && (int64_t)L * pcm_sink_tab_stride(taps) <= kPcmSinkLdsTab; }
void launch_pcm_sinks(const PcmSinkDesc* tab /* device, [n] */, int n, int max_work /* largest n_out + keep */, bool any_tab_lds, hipStream_t s);

// ---- speaking rate (q3_speed.cpp): WSOLA time stretch of 24 kHz float PCM, with carried state ----
// One stretcher of one push.  Its samples are, as for a sink, the carry ([carry_abs0, n_before)) followed by the push's n_new samples at
// x_new; x[k] = 0 for k < 0 and k >= n_total.  The launch's workgroup walks frames frame0 .. frame0 + n_frames - 1 in order (frame m:
// a_m = floor(m Hs S / 1000), template t[i] = x[p_{m-1} + Hs + i], c(delta) = (s0 + s1) + (s2 + s3) over the 2 D + 1 lags, s_q the fp32
// sum of t[i] x[a_m + delta + i] over i = q mod 4 ascending; the largest c wins, the smallest delta among equals; p_m = a_m + delta_m;
// y[m Hs + i] = w[Hs + i] t[i] + w[i] x[p_m + i]) and writes out[0 .. n_out) (n_out <= n_frames Hs: the last block of a finished
// stretcher is cut), offs[f] = delta of frame frame0 + f, the next carry x[keep_abs0 .. keep_abs0 + keep) into carry_out, and
// state_out = { p of the last frame, frame0 + n_frames }.  p_{frame0 - 1} is state_in[0] (frame0 == 0: -Hs).
struct SpeedDesc {
    const float* carry_in = nullptr; float* carry_out = nullptr;
    const float* x_new = nullptr;       // n_new samples (never null: a push without samples points at the carry)
    const float* win = nullptr;         // the window, kSpeedN floats on the device
    float* out = nullptr;               // n_out samples
    int32_t* offs = nullptr;            // n_frames offsets
    const int64_t* state_in = nullptr; int64_t* state_out = nullptr;   // { p, frames done }
    int64_t carry_abs0 = 0;             // absolute index of carry_in[0]
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push
    int64_t frame0 = 0;                 // the first frame of this push
    int64_t keep_abs0 = 0;              // absolute index of carry_out[0]
    int32_t n_new = 0, n_frames = 0, n_out = 0, keep = 0, speed = 1000;
};
void launch_wsola(const SpeedDesc* tab /* device, [n] */, int n, hipStream_t s);

// ---- output level (q3_level.cpp): gain and look-ahead limiter on 24 kHz float PCM, with carried state ----
// One stage of one push.  v[k] = g x[k]: for k < n_before the carry holds it (carry_in[j] = v[n_before - kLevelCarry + j]; entries of
// negative k are never read), for n_before <= k < n_total it is g * x_new[k - n_before]; v[k] = 0 (so r[k] = 1) for k < 0 and k >=
// n_total, which only a finishing push reaches.  Output i of the launch is the stage's absolute sample out0 + i.  limit == 0: y = v.
// limit != 0: the header's r, 128-wide minimum, quantisation, 128-wide integer sum, product and clamp; the stage's last workgroup
// writes v[n_total - kLevelCarry .. n_total) into carry_out, the other of the stage's two carry buffers (keep == 0: the carry stays).
struct LevelDesc {
    const float* carry_in = nullptr; float* carry_out = nullptr;
    const float* x_new = nullptr;       // n_new samples (never null: a push without samples points at the carry)
    float* out = nullptr;               // n_out samples
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push
    int64_t out0 = 0;                   // absolute index of the first new output
    int32_t n_new = 0, n_out = 0, limit = 0, keep = 0;
    float g = 1.0f, T = 1.0f;
};
constexpr int kLevelTile = 1024;        // outputs of one workgroup
constexpr int level_tiles(int64_t n_out) { return n_out <= 0 ? 1 : (int)((n_out + kLevelTile - 1) / kLevelTile); }
void launch_level(const LevelDesc* tab /* device, [n] */, int n, int max_tiles, hipStream_t s);

// ---- pitch (q3_pitch.cpp): TD-PSOLA shift of the fundamental of 24 kHz float PCM, with carried state ----
// One stage of one push.  Its samples are the carry ([carry_abs0, n_before)) followed by the push's n_new samples at x_new; x[k] = 0 for
// k < 0 and k >= n_total.  half_in / half_out: the two halves of the stage's allocation, each kPitchCarry floats of input, kPitchRing
// floats of grain sum and kPitchRing of window sum (entry m belongs to output out0 + m, resp. out0 + n_out + m), then kPitchStateWords
// int64 of mark state.  The launch's workgroup places every synthesis mark whose gate has arrived (t + kPitchGate <= n_total; finish: t
// < n_total + Pmax), writes out[0 .. n_out) (outputs out0 ..), the next carry x[keep_abs0 .. keep_abs0 + keep) and the state into
// half_out.  first: the stage has received nothing yet, so accumulators and state start from their initial values, not from half_in.
struct PitchDesc {
    const float* half_in = nullptr; float* half_out = nullptr;
    const float* x_new = nullptr;       // n_new samples (never null: a push without samples points at the carry)
    const float* win = nullptr;         // the windows, kPitchWindowFloats floats on the device
    float* out = nullptr;               // n_out samples
    int64_t carry_abs0 = 0;             // absolute index of the carried input's first sample
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push
    int64_t out0 = 0;                   // absolute index of the first new output
    int64_t keep_abs0 = 0;              // absolute index of the next carry's first sample
    int32_t n_new = 0, n_out = 0, keep = 0, ratio = 1000, finish = 0, first = 0;
};
void launch_psola(const PitchDesc* tab /* device, [n] */, int n, hipStream_t s);

// ---- loudness (q3_loudness.cpp): BS.1770 meter and normaliser of 24 kHz float PCM, with carried state ----
// One stage of one push.  half_in / half_out: the two halves of the stage's allocation (q3_audio.h: kLoudHalfBytes each: the state words,
// then the input of the open sub-block, samples [kLoudBlock floor(n_before / kLoudBlock), n_before)).  The launch's workgroup filters
// the push's n_new samples at x_new, adds their energy to the open sub-block and closes every sub-block that ends at or before n_total:
// its E and G go to energies[j] / gains[j] (j counts the push's sub-blocks, n_blocks in all) and, when the stage is no meter, its
// kLoudBlock ramped samples to out.  finish: the samples of the last, partial sub-block follow at the last gain.  A meter's out is the
// push's input.  first: the stage has received nothing yet, so its state starts from zeros and g_start, not from half_in.
struct LoudDesc {
    const char* half_in = nullptr; char* half_out = nullptr;
    const float* x_new = nullptr;       // n_new samples (never null: a push without samples points at the carry)
    float* out = nullptr;               // n_out samples
    int64_t* energies = nullptr; float* gains = nullptr;   // n_blocks each
    double c[10] = {};                  // loudness_coeffs(24000)
    double pt = 0.0, r_lo = 1.0, r_hi = 1.0;   // PT = 10^((target / 10 + 0.691) / 10); 1 / R and R
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push
    float g_start = 1.0f;               // G_-1
    int32_t n_new = 0, n_out = 0, n_blocks = 0, meter = 0, finish = 0, first = 0;
};
void launch_loudness(const LoudDesc* tab /* device, [n] */, int n, hipStream_t s);

// ---- tone (q3_tone.cpp): a cascade of 1 .. 8 biquads on 24 kHz float PCM, with carried state ----
// One stage of one push.  state_in / state_out: the two halves of the stage's allocation, (n_sections + 1) * 2 doubles each: signal s
// (0: the input, s: section s's output) keeps its last sample at [2 s] and the one before at [2 s + 1].  The launch's wave filters the
// push's n_new >= 1 samples at x_new into out (as many) and writes the state behind them into state_out.  first: the stage has received
// nothing yet, so its history is zero, not state_in.
struct ToneDesc {
    const double* state_in = nullptr; double* state_out = nullptr;
    const float* x_new = nullptr;       // n_new samples
    float* out = nullptr;               // n_new samples
    double c[8][5] = {};                // tone_coeffs: b0 b1 b2 a1 a2 of each section
    int32_t n_new = 0, n_sections = 0, first = 0, pad = 0;
};
void launch_tone(const ToneDesc* tab /* device, [n] */, int n, hipStream_t s);


// ---- speaker encoder + GPU audio front end of the clone path (q3_speaker_kernels.hip) ----
// One reference clip of a batch.  Activations of a batch lie clip after clip along time ([sum T][C]); every kernel that looks across
// time takes the clip from the grid and stays inside [row_off, row_off + T).
struct SpkClip {
    int32_t in_off = 0, n_in = 0;       // the caller's samples in the raw-audio buffer
    int32_t src_rate = 0, dst_rate = 0; // equal: the clip is used as it is
    int32_t rs_off = 0, n_rs = 0;       // resampled samples (n_rs == n_in, rs_off unused, when the rates are equal)
    int32_t row_off = 0, T = 0;         // mel frames / activation rows
};
struct SpkConvArgs {
    const float* x = nullptr; int ldx = 0;   // [T][ldx] time-major (or [Cin][ldx] when x_channel_major)
    const float* x2 = nullptr; int ldx2 = 0; // optional second input added to x before the convolution
    int x_channel_major = 0;
    int T = 0, Cin = 0, Cout = 0, k = 1, dil = 1;
    int act = 0;                              // 0 none, 1 ReLU, 2 tanh(ReLU)
    const float* W = nullptr;                 // [k][Cin][Cout]
    const float* bias = nullptr;
    float* y = nullptr; int ldy = 0;
    // batch of clips (blockIdx.z): x, x2, y are the batch's buffers, T the longest clip (grid), min_T the shortest (reflect padding);
    // channel-major input is [Cin][T of the clip] per clip, clip after clip
    const SpkClip* clips = nullptr; int n_clips = 1, min_T = 0;
};
void launch_spk_conv(const SpkConvArgs& a, hipStream_t s);
void launch_spk_repack(const float* w, float* out, int cout, int cin, int k, hipStream_t s);
// clips == null: one clip of T rows.  Otherwise T is the longest clip and the per-clip vectors (mean, sd, gate, pooled) are [clip][C].
void launch_spk_colstats(const float* x, int ld, int T, int C, float* mean, float* sd, hipStream_t s, const SpkClip* clips = nullptr, int n_clips = 1);
void launch_spk_se_gate(const float* y, const float* g, float* h, float* cat, int ld_cat, int T, int C, hipStream_t s, const SpkClip* clips = nullptr, int n_clips = 1);
void launch_spk_asp_input(const float* x, const float* mean, const float* sd, float* out, int T, int C, hipStream_t s, const SpkClip* clips = nullptr, int n_clips = 1);
void launch_spk_asp_pool(const float* scores, const float* x, int T, int C, float* out, hipStream_t s, const SpkClip* clips = nullptr, int n_clips = 1);

// linear resampler of q3::resample_linear for the clips whose rates differ: rs[rs_off + i], i < n_rs, from raw[in_off ..]
void launch_resample_linear(const float* raw, float* rs, const SpkClip* clips, int n_clips, int max_n_rs, hipStream_t s);
// The same resampler for audio that is still arriving (encoder streams, q3_encoder.cpp).  One stream of one push:
// the samples the stream has are its carry (floats, the last `n_before - carry_abs0` samples before this push) followed by the
// push's n_new staged samples (float, int16 converted as (float)v / 32768.0f, or G.711 bytes decoded to that int16).  Output i of the launch is the stream's absolute
// output out0 + i: position, taps and weight from that absolute index in double, as q3::resample_linear forms them; the upper tap
// is clamped to n_total - 1, which only a finishing push reaches.  All indices are 64-bit: an hour at 384 kHz is 1.38e9 samples.
// The launch also writes the stream's next carry, the last `keep` samples of (carry, new), into carry_out: the other of the
// stream's two carry buffers, never the one being read.
struct EncRsStream {
    const float* carry_in = nullptr; float* carry_out = nullptr;
    int64_t carry_abs0 = 0;             // absolute index of carry_in[0]
    int64_t n_before = 0, n_total = 0;  // samples received before / with this push (n_before = absolute index of the first new sample)
    int64_t out0 = 0;                   // absolute index of the first new output
    int64_t in_off = 0;                 // byte offset of the new samples in the staging buffer (a multiple of 4)
    int32_t n_new = 0, n_out = 0, keep = 0;   // keep == 0: the carry stays (a push without samples)
    int32_t x24_off = 0;                // first new output in the push's 24 kHz buffer
    int32_t src_rate = 0, format = 0;   // format: Q3TTS_PCM_* of the staged samples
};
void launch_resample_linear_streams(const void* staged, float* x24, const EncRsStream* tab /* device, [n] */, int n, int max_work /* largest n_out + keep */, hipStream_t s);
// log-mel of q3::log_mel for the clone path's MelSpec (n_fft = win = 1024, hop 256, 128 bands): mel + 128 * row_off is the clip's [128][T]
struct MelTablesDev {
    const float *window = nullptr, *tw_re = nullptr, *tw_im = nullptr;   // [1024], [512], [512]
    const uint32_t* rev = nullptr;                                       // [1024]
    const int32_t *lo = nullptr, *mid = nullptr, *hi = nullptr;          // [128] triangle corners
};
void launch_logmel(const float* raw, const float* rs, const SpkClip* clips, int n_clips, int max_T, const MelTablesDev& tb, float* mel, hipStream_t s);


// ---- audio encoder of the 12 Hz tokenizer (q3_encoder_kernels.hip): fp32 throughout ----
// Activations are time-major rows, clip after clip.  One clip at one rate level: its first row in the level's buffer and its rows.
struct EncSpan { int32_t off = 0, T = 0; };
// out[t][co] = res[t][co] + scale[co] * act(bias[co] + sum_{tap, ci} W[tap][co][ci] * f(in[t * stride - pad_left + tap * dil][ci])),
// f = ELU when elu_in; rows outside [0, T_in) are zeros, or the clip's first / last row when replicate.  blockIdx.z = clip: the tile
// grid starts at each clip's own t = 0 and no tap leaves the clip, so a clip's arithmetic does not depend on the rest of the batch.
struct EncConvArgs {
    const float* in = nullptr; float* out = nullptr;      // [rows][Cin], [rows][Cout]
    const float* W = nullptr;                             // [taps][Cout][Cin]
    const float* bias = nullptr; const float* scale = nullptr; const float* res = nullptr;   // optional; res [rows][Cout] may alias out
    int Cin = 0, Cout = 0, taps = 1, dil = 1, stride = 1, pad_left = 0;
    int replicate = 0, elu_in = 0, act = 0;               // act 1: exact (erf) GELU
    const EncSpan* sin = nullptr; const EncSpan* sout = nullptr; int n_clips = 0, max_T_out = 0;
};
void launch_enc_conv(const EncConvArgs& a, hipStream_t s);      // Cin == 1: VALU kernel; otherwise implicit GEMM on the fp32 matrix cores
// Streamed pushes (q3_encoder.cpp).  One stream at one launch: the span holds the stream's NEW rows only, and what lies
// before them comes from the stream's carry ring: `cap` rows of the launch's input width, absolute input row r in slot r mod cap.
// n_in = input rows the stream had before this push (the chunk's row 0 is absolute row n_in); shift = chunk-local input row that
// output row 0's stride origin falls on (n_out * stride - n_in, <= 0).  A conv reads src = t * stride + shift - pad_left + tap * dil:
// src >= 0 is a chunk row, src < 0 absolute row n_in + src from the ring, rows before the stream's start are zeros (its first row
// when replicate) and rows past the chunk are zeros (its last row when replicate): the one-shot's edges, met only at a stream's
// first and finishing pushes.  RoPE and attention read n_in as the chunk's first absolute row and carry as the layer's K/V ring
// ([window - 1][2 * heads * d]: rotated K, then V).
struct EncHist { const float* carry = nullptr; int32_t n_in = 0, shift = 0, cap = 0, pad_ = 0; };
void launch_enc_conv_hist(const EncConvArgs& a, const EncHist* hist /* device, [n_clips] */, hipStream_t s);
// rows [0, rows) of src (row stride src_ld floats, `width` floats each) into ring slots (slot0 + i) mod cap of dst; rows <= cap
struct EncCarryCopy { const float* src = nullptr; float* dst = nullptr; int32_t rows = 0, width = 0, src_ld = 0, slot0 = 0, cap = 0, pad_ = 0; };
void launch_enc_carry_copy(const EncCarryCopy* tab /* device, [n] */, int n, int64_t max_floats /* largest rows * width */, hipStream_t s);
void launch_enc_layernorm(const float* x, const float* w, const float* b, float eps, int rows, int C, float* out, hipStream_t s);
// q and k of qkv [rows][3 * heads * d] rotated in place (rotate-half RoPE) at each row's position inside its clip; cs / sn [max_pos][d / 2]
// hist (streamed pushes): position = hist[clip].n_in + row
void launch_enc_rope(float* qkv, const float* cs, const float* sn, int max_pos, int heads, int d, const EncSpan* spans, int n_clips, int max_T, hipStream_t s,
                     const EncHist* hist = nullptr);
// causal sliding-window attention inside each clip: row i sees rows (i - window, i]; out [rows][heads * d]
// hist (streamed pushes): keys before the chunk come from hist[clip].carry, the layer's K/V ring
void launch_enc_attn(const float* qkv, float* out, int heads, int d, int window, float scale, const EncSpan* spans, int n_clips, int max_T, hipStream_t s,
                     const EncHist* hist = nullptr);
// split residual VQ: per frame both input projections ([D][H] each), then level g = 0 on the semantic residual and levels 1 .. G - 1 on the
// acoustic one: nearest row of books[g] [CB][D] by direct squared distance (lowest index on a tie), residual -= that row.  codes [rows][G]
void launch_rvq_encode(const float* lat, int rows, int H, const float* proj_sem, const float* proj_ac, const float* books, int G, int CB, int D,
                       int32_t* codes, hipStream_t s);

} // namespace q3
