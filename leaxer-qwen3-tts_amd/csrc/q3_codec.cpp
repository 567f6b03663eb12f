// q3_codec.cpp — orchestration of the 12 Hz codec decoder on the GPU: the reference's
// run_vocoder / tokenizer12hz_decode.onnx session (src/tts_onnx.cpp:759-776).  [HINT] architecture:
// transformers Qwen3OmniMoeCode2Wav (modeling_qwen3_omni_moe.py:3180-3697), pinned by
// tests/golden/hf_code2wav.npz.  Whole-utterance decode like the reference (tts_onnx.cpp:430):
// with 288 GB of HBM the largest activation (F=2048: 3.9 M samples x 96 ch fp32 = 1.5 GB) needs no
// chunking.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "q3_engine.h"

namespace q3 {

struct PackedConv { const float* w = nullptr; const float* b = nullptr; int cin = 0, cout = 0, k = 0; };
struct SnakeP { const float *alpha = nullptr, *beta = nullptr; int C = 0; };

// The weight half: a function of the checkpoint (and of Q3TTS_FLAG_FP32_CODEC, which decides whether the planes exist) alone.  It lives
// in the engine's WeightSet; every holder's CodecW reads it through references of the same names.
struct CodecWeights {
    struct Layer { const float *in_norm, *post_norm, *qkv, *o, *gate, *up, *down, *attn_scale, *mlp_scale; };
    std::vector<Layer> layers;
    const float *norm = nullptr, *code_embed = nullptr;
    struct Up { PackedConv tconv; const float *dw_w, *dw_b, *ln_w, *ln_b, *pw1_w, *pw1_b, *pw2_w, *pw2_b, *gamma; };
    std::vector<Up> up;
    PackedConv conv_in, conv_out;
    struct Res { SnakeP a1, a2; PackedConv c1, c2; };
    struct Block { SnakeP act; PackedConv tconv; Res res[3]; };
    std::vector<Block> blocks;
    SnakeP snake_out;
    std::vector<float*> packed; // owned
    // (hi, lo) bf16 planes of every conv / linear weight, keyed by the fp32 pointer the layer list holds (owned)
    // lo_zero: the weight is exact in fp16 (bf16- / fp16-origin): two products instead of three.  cm: the same planes chunk-major
    // ([plane][tap][C_in / 32][C_out][32], ConvArgs::Whc; null when C_in is not a multiple of 32); fh / fl: a 96 x 96 second conv of a
    // fused residual unit in B-fragment order (ConvArgs::W2fh / W2fl; one allocation)
    struct Planes { bf16_t* hi; bf16_t* lo; float scale_inv; bool lo_zero; bf16_t* cm = nullptr; bf16_t* fh = nullptr; bf16_t* fl = nullptr; };
    int n_lo_zero = 0, n_lo_used = 0;
    std::unordered_map<const float*, Planes> planes;
    // SnakeBeta constants [2][C] (exp(alpha) | 1 / (exp(beta) + 1e-9)) keyed by the alpha pointer (owned; split-precision path only)
    std::unordered_map<const float*, float*> snake_pre;
    int64_t bytes = 0;   // HBM of the owned copies (counted in the set's bytes)
};

void codec_weights_free(CodecWeights* w) {
    if (!w) return;
    for (float* p : w->packed) (void)hipFree(p);
    for (auto& kv : w->planes) {
        (void)hipFree(kv.second.hi);   // lo lives in the same allocation
        if (kv.second.cm) (void)hipFree(kv.second.cm);
        if (kv.second.fh) (void)hipFree(kv.second.fh);   // fl lives in the same allocation
    }
    for (auto& kv : w->snake_pre) (void)hipFree(kv.second);
    delete w;
}

// The run-time half, one per engine: lanes, arenas, pinned buffers, RoPE tables, streams.
struct CodecW {
    using Layer = CodecWeights::Layer; using Up = CodecWeights::Up; using Res = CodecWeights::Res; using Block = CodecWeights::Block; using Planes = CodecWeights::Planes;
    explicit CodecW(const CodecWeights& w)
        : layers(w.layers), norm(w.norm), code_embed(w.code_embed), up(w.up), conv_in(w.conv_in), conv_out(w.conv_out), blocks(w.blocks),
          snake_out(w.snake_out), n_lo_zero(w.n_lo_zero), n_lo_used(w.n_lo_used), planes(w.planes), snake_pre(w.snake_pre) {}
    const std::vector<Layer>& layers;
    const float* const& norm; const float* const& code_embed;
    const std::vector<Up>& up;
    const PackedConv &conv_in, &conv_out;
    const std::vector<Block>& blocks;
    const SnakeP& snake_out;
    const int &n_lo_zero, &n_lo_used;
    const std::unordered_map<const float*, Planes>& planes;
    const std::unordered_map<const float*, float*>& snake_pre;
    // run-time workspace: one bump arena per codec stream (lane 0 = the engine's own stream)
    static constexpr int NLANE = 32;   // capacity; `nlane` of them are used (Q3TTS_CODEC_LANES)
    int nlane = 9;                      // lane 0 = the engine's stream (synchronous entry points), the others decode asynchronously
    char* arena[NLANE] = {}; size_t arena_bytes[NLANE] = {};
    hipStream_t lane_stream[NLANE] = {};
    float* pinned[NLANE] = {}; size_t pinned_floats[NLANE] = {};
    float *rope_cos = nullptr, *rope_sin = nullptr; int rope_P = 0;
    int* page_table = nullptr;
    // asynchronous per-utterance decodes over the side lanes: result parked in the lane's pinned buffer until the lane is drained
    struct Item { float* user; int64_t n, cap, off; int64_t* len; };   // off: float offset of the utterance's samples in the lane's pinned buffer
    struct Pending { std::vector<Item> items; int frames = 0; bool busy = false; };
    Pending pend[NLANE];
    int32_t* job_codes = nullptr; size_t job_codes_n = 0;
    const float* dbg_sx = nullptr; const float* dbg_pcm = nullptr; int dbg_T = 0, dbg_C = 0, dbg_nb = 0;   // test hook: the last batched group's final conv
    char* batch_arena = nullptr; size_t batch_arena_bytes = 0;   // batched pre-transformer of a job (codec_pre_batch)
    int* batch_pages = nullptr; size_t batch_pages_n = 0;          // identity page table, one cache block per utterance   // codes of a scheduler job's finished utterances, [utterance][max_new][groups]
    hipEvent_t lane_done[NLANE] = {};
    hipEvent_t fork = nullptr, win0 = nullptr, win1 = nullptr;
    bool window_open = false, win0_recorded = false;
    int rr = 0;
    int submits = 0, fail_at_submit = 0;   // fault injection for the tests: the fail_at_submit-th submit of a job throws
    // carried-state streaming decode (Engine::codec_stream_*): per stream the pre-transformer's K / V rows of every layer ([layer][k | v]
    // [head][P][d]) and its output rows [cap][hidden]; work buffers of one push in a grow-only arena of their own
    // Both are SLIDING buffers (round 5; they used to hold every position up to the stream's capacity: 268 MB of K / V per stream at
    // max_ctx 2112).  kv: [layer][k | v][head][P][d] with P = pow2 >= 2 (window - 1) + the largest push so far; `kv_rows` rows are stored,
    // the last of them position n_done - 1; when a push would not fit, the newest window - 1 rows move to the front (the only ones a
    // later query can reach).  hpost: [h_cap][hidden], `h_rows` stored, the newest codec_stage_b_context() rows kept the same way.
    // stage: the stream's stages by Engine::StageKind, in the order its audio passes them (ids of Engine::stages[k]; -1: none, all -1:
    // the stream delivers 24 kHz float); delivered: a push has returned samples
    struct Stream { bool used = false; int cap = 0, P = 0, pshift = 0, n_done = 0, kv_rows = 0, h_cap = 0, h_rows = 0; float* kv = nullptr; float* hpost = nullptr;
                    int stage[Engine::SK_N] = { -1, -1, -1, -1, -1, -1 }; bool delivered = false;
                    const char* has() const {   // what the float entries refuse the stream by; nullptr: no stage
                        return stage[Engine::SK_SINK] >= 0 ? " has a sink" : stage[Engine::SK_SPEED] >= 0 ? " has a speed" : stage[Engine::SK_LEVEL] >= 0 ? " has a level" : stage[Engine::SK_PITCH] >= 0 ? " has a pitch"
                             : stage[Engine::SK_LOUD] >= 0 ? " has a loudness" : stage[Engine::SK_TONE] >= 0 ? " has a tone" : nullptr; } };
    std::vector<Stream> streams;
    char* stream_arena = nullptr; size_t stream_arena_bytes = 0;
    std::vector<int> slot_stream;          // slot -> stream id (-1: none): q3tts_slot_codec_decode_range_host's implicit stream
    // batched push (Engine::codec_stream_push_batch): work buffers of all streams' new rows and of one group's window behind the
    // transformer, the descriptor table of a push (host copy + device), the host codes' staging area; all grow-only
    char* sbatch_arena = nullptr; size_t sbatch_arena_bytes = 0;
    CodecStreamDesc* sbatch_desc = nullptr; size_t sbatch_desc_n = 0;
    std::vector<CodecStreamDesc> sbatch_desc_h;
    int32_t* sbatch_codes = nullptr; size_t sbatch_codes_n = 0;
};

void Engine::codec_free() {
    if (!codec) return;
    for (int i = 0; i < CodecW::NLANE; ++i) {
        if (codec->arena[i]) (void)hipFree(codec->arena[i]);
        if (codec->pinned[i]) (void)hipHostFree(codec->pinned[i]);
        if (codec->lane_done[i]) (void)hipEventDestroy(codec->lane_done[i]);
        if (i > 0 && codec->lane_stream[i] && !null_stream) (void)hipStreamDestroy(codec->lane_stream[i]);
    }
    for (hipEvent_t ev : { codec->fork, codec->win0, codec->win1 }) if (ev) (void)hipEventDestroy(ev);
    if (codec->job_codes) (void)hipFree(codec->job_codes);
    if (codec->batch_arena) (void)hipFree(codec->batch_arena);
    if (codec->batch_pages) (void)hipFree(codec->batch_pages);
    if (codec->rope_cos) (void)hipFree(codec->rope_cos);
    if (codec->rope_sin) (void)hipFree(codec->rope_sin);
    if (codec->page_table) (void)hipFree(codec->page_table);
    for (auto& s : codec->streams) { if (s.kv) (void)hipFree(s.kv); if (s.hpost) (void)hipFree(s.hpost); }
    if (codec->stream_arena) (void)hipFree(codec->stream_arena);
    if (codec->sbatch_arena) (void)hipFree(codec->sbatch_arena);
    if (codec->sbatch_desc) (void)hipFree(codec->sbatch_desc);
    if (codec->sbatch_codes) (void)hipFree(codec->sbatch_codes);
    delete codec;
    codec = nullptr;
}

void Engine::codec_plane_stats(int* two_product, int* three_product) const {
    if (two_product) *two_product = codec ? codec->n_lo_zero : 0;
    if (three_product) *three_product = codec ? codec->n_lo_used : 0;
}

void Engine::codec_finalize() {
    codec_free();
    if (ws.codec) { ws.add_bytes(-ws.codec->bytes); codec_weights_free(ws.codec); ws.codec = nullptr; }
    ws.codec = new CodecWeights;
    CodecWeights& W = *ws.codec;
    auto fp = [&](const std::string& n) { return (const float*)T(n).dev; };
    auto pack = [&](const std::string& prefix, int cin, int cout, int k, bool transposed) {
        float* out = (float*)ws.take((size_t)cin * cout * k * sizeof(float), W.bytes);
        W.packed.push_back(out);
        launch_repack_conv(fp(prefix + ".w"), out, cin, cout, k, transposed ? 1 : 0, stream);
        PackedConv p; p.w = out; p.b = fp(prefix + ".b"); p.cin = cin; p.cout = cout; p.k = k;
        return p;
    };
    auto snake = [&](const std::string& prefix) { SnakeP s; s.alpha = fp(prefix + ".alpha"); s.beta = fp(prefix + ".beta"); s.C = (int)T(prefix + ".alpha").numel; return s; };
    const int CH = c.cd_hidden, D = c.cd_decoder_dim;
    for (int i = 0; i < c.cd_layers; ++i) {
        const std::string p = "cd.layers." + std::to_string(i) + ".";
        CodecWeights::Layer L;
        L.in_norm = fp(p + "input_norm"); L.post_norm = fp(p + "post_norm"); L.qkv = fp(p + "q_proj"); L.o = fp(p + "o_proj");
        L.gate = fp(p + "gate_proj"); L.up = fp(p + "up_proj"); L.down = fp(p + "down_proj");
        L.attn_scale = fp(p + "attn_scale"); L.mlp_scale = fp(p + "mlp_scale");
        W.layers.push_back(L);
    }
    W.norm = fp("cd.norm"); W.code_embed = fp("cd.code_embed");
    for (int s = 0; s < c.cd_n_up; ++s) {
        const std::string p = "cd.up." + std::to_string(s) + ".";
        CodecWeights::Up u;
        u.tconv = pack(p + "tconv", CH, CH, c.cd_up_ratios[s], true);
        u.dw_w = fp(p + "cnx.dw.w"); u.dw_b = fp(p + "cnx.dw.b"); u.ln_w = fp(p + "cnx.ln.w"); u.ln_b = fp(p + "cnx.ln.b");
        u.pw1_w = fp(p + "cnx.pw1.w"); u.pw1_b = fp(p + "cnx.pw1.b"); u.pw2_w = fp(p + "cnx.pw2.w"); u.pw2_b = fp(p + "cnx.pw2.b");
        u.gamma = fp(p + "cnx.gamma");
        W.up.push_back(u);
    }
    W.conv_in = pack("cd.dec.conv_in", CH, D, 7, false);
    for (int i = 0; i < c.cd_n_blocks; ++i) {
        const int cin = D >> i, cout = D >> (i + 1), r = c.cd_up_rates[i];
        const std::string p = "cd.dec.blocks." + std::to_string(i) + ".";
        CodecWeights::Block B;
        B.act = snake(p + "snake");
        B.tconv = pack(p + "tconv", cin, cout, 2 * r, true);
        for (int u = 0; u < 3; ++u) {
            const std::string q = p + "res." + std::to_string(u) + ".";
            B.res[u].a1 = snake(q + "act1"); B.res[u].a2 = snake(q + "act2");
            B.res[u].c1 = pack(q + "conv1", cout, cout, 7, false);
            B.res[u].c2 = pack(q + "conv2", cout, cout, 1, false);
        }
        W.blocks.push_back(B);
    }
    W.snake_out = snake("cd.dec.snake_out");
    W.conv_out = pack("cd.dec.conv_out", D >> c.cd_n_blocks, 1, 7, false);
    if (!(flags & Q3TTS_FLAG_FP32_CODEC)) { // fp16 hi/lo planes for the split-precision matrix-core path
        unsigned* amax_d = (unsigned*)dmalloc(sizeof(unsigned));
        auto split = [&](const float* w, size_t n, int taps = 0, int cout = 0, int cin = 0) {
            if (!w || W.planes.count(w)) return;
            // power-of-two pre-scale: largest |w| lands in [2^11, 2^12) so the low plane of ordinary weights stays normal
            unsigned bits = 0;
            Q3_HIP_CHECK(hipMemsetAsync(amax_d, 0, sizeof(unsigned), stream));
            launch_absmax(w, n, amax_d, stream);
            Q3_HIP_CHECK(hipMemcpyAsync(&bits, amax_d, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            sync();
            float amax;
            memcpy(&amax, &bits, sizeof amax);
            int e = 0;
            if (amax > 0.f && std::isfinite(amax)) (void)frexpf(amax, &e);   // amax = m * 2^e, m in [0.5, 1)
            // k <= 126: 2^k (the pre-scale) and 2^-k (the epilogue's acc_scale) both finite and normal.  A tensor whose largest magnitude is
            // below 2^-115 would ask for more (2^k = inf: planes of inf / nan); it keeps 2^126 and sits lower in the planes instead, at
            // an absolute resolution of 2^-150, beyond fp32's own.  e <= 128, so k >= -116 needs no bound.
            const int k = amax > 0.f ? std::min(12 - e, 126) : 0;
            bf16_t *hi = nullptr, *lo = nullptr;   // one allocation, lo right behind hi: k_conv_split addresses both planes as base + 32-bit offset
            const size_t np = (n + 7) / 8 * 8;
            hi = (bf16_t*)ws.take(2 * np * sizeof(bf16_t), W.bytes);
            lo = hi + np;
            launch_split_planes(w, hi, lo, n, ldexpf(1.0f, k), stream);
            unsigned lo_bits = 0;
            Q3_HIP_CHECK(hipMemsetAsync(amax_d, 0, sizeof(unsigned), stream));
            launch_or_mag16(lo, n, amax_d, stream);
            Q3_HIP_CHECK(hipMemcpyAsync(&lo_bits, amax_d, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            sync();
            CodecWeights::Planes pl{ hi, lo, ldexpf(1.0f, -k), lo_bits == 0 };
            if (taps > 0 && cin % 32 == 0 && (size_t)taps * cout * cin == n) {   // the chunk-major copy for the 32-wide-chunk kernels
                pl.cm = (bf16_t*)ws.take(2 * np * sizeof(bf16_t), W.bytes);
                launch_repack_planes_cm(hi, pl.cm, taps, cout, cin, np, stream);
            }
            if (taps == 1 && cout == 96 && cin == 96) {                           // a fused unit's second conv: B fragments
                pl.fh = (bf16_t*)ws.take(2 * n * sizeof(bf16_t), W.bytes);
                pl.fl = pl.fh + n;
                launch_pack_w2_frags(hi, pl.fh, 96, stream);
                launch_pack_w2_frags(lo, pl.fl, 96, stream);
            }
            W.planes[w] = pl;
            (lo_bits == 0 ? W.n_lo_zero : W.n_lo_used) += 1;
        };
        const size_t FFn = (size_t)c.cd_ffn;
        for (const CodecW::Layer& L : W.layers) {
            split(L.qkv, (size_t)3 * CH * CH, 1, 3 * CH, CH); split(L.o, (size_t)CH * CH, 1, CH, CH);
            split(L.gate, FFn * CH, 1, (int)FFn, CH); split(L.up, FFn * CH, 1, (int)FFn, CH); split(L.down, FFn * CH, 1, CH, (int)FFn);
        }
        for (const CodecW::Up& u : W.up) {
            split(u.tconv.w, (size_t)u.tconv.cin * u.tconv.cout * u.tconv.k, u.tconv.k, u.tconv.cout, u.tconv.cin);
            split(u.pw1_w, (size_t)4 * CH * CH, 1, 4 * CH, CH); split(u.pw2_w, (size_t)4 * CH * CH, 1, CH, 4 * CH);
        }
        auto pc = [&](const PackedConv& p) { split(p.w, (size_t)p.cin * p.cout * p.k, p.k, p.cout, p.cin); };
        pc(W.conv_in);
        for (const CodecW::Block& B : W.blocks) { pc(B.tconv); for (int u = 0; u < 3; ++u) { pc(B.res[u].c1); pc(B.res[u].c2); } }
        auto pre = [&](const SnakeP& sp) {   // exp(alpha), 1 / (exp(beta) + 1e-9) once per activation instead of once per 32-row block of every launch
            if (!sp.alpha || !sp.beta || sp.C <= 0 || W.snake_pre.count(sp.alpha)) return;
            float* d = (float*)ws.take((size_t)2 * sp.C * sizeof(float), W.bytes);
            launch_snake_pre(sp.alpha, sp.beta, d, sp.C, stream);
            W.snake_pre[sp.alpha] = d;
        };
        for (const CodecW::Block& B : W.blocks) { pre(B.act); for (int u = 0; u < 3; ++u) { pre(B.res[u].a1); pre(B.res[u].a2); } }
        pre(W.snake_out);
    }
    sync();
    codec_runtime_init();
}

void Engine::codec_runtime_init() {
    codec_free();
    if (!ws.codec) throw Error("codec decoder not finalized");
    codec = new CodecW(*ws.codec);
    CodecW& W = *codec;
    if (const char* ev = getenv("Q3TTS_CODEC_LANES")) W.nlane = std::max(1, std::min((int)CodecW::NLANE, atoi(ev)));
    W.lane_stream[0] = stream;
    for (int i = 1; i < W.nlane; ++i) {
        if (null_stream) W.lane_stream[i] = nullptr;
        else {
            int lo = 0, hi = 0;
            Q3_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            Q3_HIP_CHECK(hipStreamCreateWithPriority(&W.lane_stream[i], hipStreamNonBlocking, lo));
        }
    }
    int zero = 0;
    Q3_HIP_CHECK(hipMalloc((void**)&W.page_table, sizeof(int)));
    Q3_HIP_CHECK(hipMemcpy(W.page_table, &zero, sizeof(int), hipMemcpyHostToDevice));
    sync();
}

static int tconv_out_len(const q3tts_config& c, int T, int k, int s, int* left_out) {
    const int pad = k - s, left = c.cd_tconv_trim == 0 ? pad : 0;
    if (left_out) *left_out = left;
    return (T - 1) * s + k - left - pad;
}

// RoPE tables of the codec's pre-transformer for positions [0, P), oracle formula (fp32 libm); grow-only, shared by every lane and stream
void Engine::codec_rope_tables(int P) {
    CodecW& W = *codec;
    if (W.rope_P >= P) return;
    const int HD = c.cd_head_dim;
    for (int i = 0; i < W.nlane; ++i) Q3_HIP_CHECK(hipStreamSynchronize(W.lane_stream[i])); // tables may be in use
    const int half = HD / 2;
    std::vector<float> cs((size_t)P * half), sn((size_t)P * half);
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < half; ++i) {
            const float inv = 1.0f / powf(c.cd_rope_theta, (float)(2 * i) / (float)HD);
            const float ang = (float)p * inv;
            cs[(size_t)p * half + i] = cosf(ang); sn[(size_t)p * half + i] = sinf(ang);
        }
    // the old tables are freed by regrow (every lane drained above); rope_P counts again once both new ones are filled
    size_t cap = 0;
    W.rope_P = 0;
    regrow(W.rope_cos, cap, cs.size(), 1, true);
    regrow(W.rope_sin, cap, sn.size(), 1, true);
    Q3_HIP_CHECK(hipMemcpy(W.rope_cos, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
    Q3_HIP_CHECK(hipMemcpy(W.rope_sin, sn.data(), sn.size() * sizeof(float), hipMemcpyHostToDevice));
    W.rope_P = P;
}

// ------------------------------------------------------------------------------------------------
// What the five decode paths share: the conv launcher, the attention arguments, the pre-transformer's layer loop and the
// workspace rule.  A path keeps what differs: its rows, the order it carves its arena in, its K / V store and attention, the code
// embedding in front of the loop and the final norm behind it.
// ------------------------------------------------------------------------------------------------
// Every conv / linear launch: the weight's (hi, lo, cm) planes, the SnakeBeta constants and the caller's split-K slab are attached here.
// plan: codec_run's sizing pass, which launches nothing; batch: sequences per launch of its conv decoder
struct ConvLauncher {
    const CodecW& W; float* slab; hipStream_t stream; int batch = 1; bool plan = false;
    void operator()(ConvArgs a) const {
        if (plan) return;
        a.slab = slab; a.slab_floats = CODEC_KSLAB_FLOATS; a.batch = batch;
        const auto it = W.planes.find(a.W);
        if (it != W.planes.end()) { a.Wh = it->second.hi; a.Wl = it->second.lo; a.Whc = it->second.cm; a.w_scale_inv = it->second.scale_inv; a.w_lo_zero = it->second.lo_zero; }
        if (a.snake_alpha) { const auto sp = W.snake_pre.find(a.snake_alpha); if (sp != W.snake_pre.end()) a.snake_pre = sp->second; }
        if (a.mid_alpha) { const auto sp = W.snake_pre.find(a.mid_alpha); if (sp != W.snake_pre.end()) a.mid_pre = sp->second; }
        launch_conv(a, stream);
    }
};

// The vocoder's windowed attention over one layer's roped, stored K / V ([block][head][2^page_shift][d], one block per sequence through
// page_table): nb sequences of n_new rows each, the first of them at cache row pos_scalar
static AttnArgs codec_attn_args(const q3tts_config& c, const float* qkv, float* out, float* kc, float* vc, const int* page_table, int page_shift, int pos_scalar, int nb, int n_new) {
    AttnArgs a;
    a.qkv = qkv; a.ld_qkv = 3 * c.cd_hidden; a.out = out; a.ld_out = c.cd_hidden; a.kcache = kc; a.vcache = vc;
    a.page_table = page_table; a.pages_per_slot = 1; a.page_shift = page_shift; a.layer = 0; a.n_layers = 1;
    a.pos_scalar = pos_scalar; a.slot_offset = 0; a.nb = nb; a.n_new = n_new; a.nq = c.cd_heads; a.nkv = c.cd_heads; a.d = c.cd_head_dim;
    a.scale = 1.0f / sqrtf((float)c.cd_head_dim); a.window = c.cd_window; a.new_from_raw = 0;
    return a;
}

// The pre-transformer's layers over T rows of h, in place: RMSNorm, QKV GEMM, store_and_attend(l), o_proj with residual scale, RMSNorm,
// up, gate . up, down with residual scale.  store_and_attend(l) is the caller's launches between the QKV GEMM and o_proj (RoPE + K / V
// store of qkvb's rows, attention into att): the only thing that differs per path.  The six row buffers are the caller's; nothing is allocated.
struct PreBufs { float *h, *hn, *att, *qkvb, *ub, *gb; };
template <class StoreAttend>
static void pre_transformer_layers(const q3tts_config& c, const CodecW& W, int T, const PreBufs& b, const ConvLauncher& conv, StoreAttend&& store_and_attend, hipStream_t stream) {
    const int CH = c.cd_hidden, FF = c.cd_ffn;
    auto gemm = [&](const float* in, int Cin, const float* Wm, int Cout, float* out) {
        ConvArgs a; a.in = in; a.T_in = T; a.C_in = Cin; a.out = out; a.T_out = T; a.C_out = Cout; a.W = Wm;
        return a;
    };
    for (int l = 0; l < c.cd_layers; ++l) {
        const CodecW::Layer& L = W.layers[l];
        launch_rmsnorm_rows(b.h, L.in_norm, c.cd_rms_eps, T, CH, b.hn, stream);
        conv(gemm(b.hn, CH, L.qkv, 3 * CH, b.qkvb));
        store_and_attend(l);
        { ConvArgs a = gemm(b.att, CH, L.o, CH, b.h); a.res_scale = L.attn_scale; a.res = b.h; conv(a); }
        launch_rmsnorm_rows(b.h, L.post_norm, c.cd_rms_eps, T, CH, b.hn, stream);
        conv(gemm(b.hn, CH, L.up, FF, b.ub));
        { ConvArgs a = gemm(b.hn, CH, L.gate, FF, b.gb); a.act = 2; a.mul = b.ub; conv(a); }
        { ConvArgs a = gemm(b.gb, FF, L.down, CH, b.h); a.res_scale = L.mlp_scale; a.res = b.h; conv(a); }
    }
}

// Engine::regrow's order (free, null and zero capacity, allocate, set capacity) for a lane's pinned staging buffer.  No drain: the caller
// has drained the lane, so no copy into the old buffer is in flight.
static void regrow_pinned(float*& p, size_t& cap, size_t n) {
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    Q3_HIP_CHECK(hipHostMalloc((void**)&p, n * sizeof(float)));
    cap = n;
}

// identity page table of the whole-utterance layouts, one scratch cache block per sequence: [0, n); [n_cap, 2 n_cap): codec_pre_batch's
// perm area.  The capacity counts only once the identity is in the new buffer.
static void codec_identity_pages(Engine& e, int n) {
    CodecW& W = *e.codec;
    if (W.batch_pages_n >= (size_t)n) return;
    size_t cap = 0;
    W.batch_pages_n = 0;
    e.regrow(W.batch_pages, cap, (size_t)n, 2);
    std::vector<int> idt((size_t)n);
    for (int i = 0; i < n; ++i) idt[(size_t)i] = i;
    Q3_HIP_CHECK(hipMemcpy(W.batch_pages, idt.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    W.batch_pages_n = cap;
}

int64_t Engine::codec_run(const int32_t* codes_dev, int F, float** pcm_dev, int lane, const float* h_in, int h_stage, int nbatch, size_t h_ustride) {
    if (!codec) throw Error("codec decoder not finalized");
    CodecW& W = *codec;
    if (lane < 0 || lane >= W.nlane) throw Error("codec: bad lane");
    hipStream_t stream = W.lane_stream[lane]; // shadows the engine stream for every launch below
    if (nbatch < 1 || (nbatch > 1 && !(h_in && h_stage == 2))) throw Error("codec: a batched decode starts from codec_pre_batch's upsampled rows");
    const size_t nbz = (size_t)nbatch;   // sequences per launch of the conv decoder (rows [sequence][T] everywhere)
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim, FF = c.cd_ffn, D = c.cd_decoder_dim;
    if (NH * HD != CH) throw Error("codec: heads*head_dim must equal hidden");
    int P = 1, pshift = 0;
    while (P < F) { P <<= 1; ++pshift; }
    codec_rope_tables(P);

    int64_t n_pcm = 0;
    float* pcm = nullptr;
    for (int pass = 0; pass < 2; ++pass) { // pass 0 sizes the arena, pass 1 launches
        const bool plan = pass == 0;
        CodecBump take{ plan ? nullptr : W.arena[lane] };
        float* kslab = take(CODEC_KSLAB_FLOATS);
        const ConvLauncher conv{ W, kslab, stream, nbatch, plan };
        auto gemm = [&](const float* in, int T, int Cin, const float* Wm, const float* bias, int Cout, float* out) {
            ConvArgs a; a.in = in; a.T_in = T; a.C_in = Cin; a.out = out; a.T_out = T; a.C_out = Cout; a.W = Wm; a.bias = bias;
            return a;
        };
        // ---- code embedding mean + pre-transformer ----
        float* h = take((size_t)F * CH);
        float* hn = take((size_t)F * CH);
        float* qkvb = take((size_t)F * 3 * CH);
        float* att = take((size_t)F * CH);
        float* ub = take((size_t)F * FF);
        float* gb = take((size_t)F * FF);
        float* kc = take((size_t)NH * P * HD);
        float* vc = take((size_t)NH * P * HD);
        if (!plan && !h_in) {   // h_in: the pre-transformer of this utterance already ran (codec_pre_batch, a push)
            launch_code_embed_mean(W.code_embed, codes_dev, F, c.n_groups, c.cd_codebook, CH, h, stream);
            pre_transformer_layers(c, W, F, PreBufs{ h, hn, att, qkvb, ub, gb }, conv, [&](int) {
                launch_rope_store(qkvb, 3 * CH, F, NH, NH, HD, W.rope_cos, W.rope_sin, kc, vc, P, stream);
                launch_attn(codec_attn_args(c, qkvb, att, kc, vc, W.page_table, pshift, 0, 1, F), stream);
            }, stream);
            launch_rmsnorm_rows(h, W.norm, c.cd_rms_eps, F, CH, h, stream);
        }
        // ---- ConvNeXt upsampling stages ----
        float* cur = h_in ? const_cast<float*>(h_in) : h;
        int Tc = F;
        if (h_in && h_stage == 2)   // the ConvNeXt upsampling stages ran in codec_pre_batch too
            for (int s = 0; s < c.cd_n_up; ++s) Tc = tconv_out_len(c, Tc, c.cd_up_ratios[s], c.cd_up_ratios[s], nullptr);
        for (int s = 0; s < (h_in && h_stage == 2 ? 0 : c.cd_n_up); ++s) {
            const CodecW::Up& U = W.up[s];
            const int f = c.cd_up_ratios[s];
            int left = 0;
            const int To = tconv_out_len(c, Tc, f, f, &left);
            float* y = take((size_t)To * CH);
            float* ln = take((size_t)To * CH);
            float* a4 = take((size_t)To * 4 * CH);
            { ConvArgs a; a.in = cur; a.T_in = Tc; a.C_in = CH; a.out = y; a.T_out = To; a.C_out = CH; a.W = U.tconv.w; a.bias = U.tconv.b;
              a.taps = f; a.transposed = 1; a.stride = f; a.left = left; conv(a); }
            if (!plan) launch_dwconv_ln(y, To, CH, U.dw_w, U.dw_b, U.ln_w, U.ln_b, ln, stream);
            { ConvArgs a = gemm(ln, To, CH, U.pw1_w, U.pw1_b, 4 * CH, a4); a.act = 1; conv(a); }
            { ConvArgs a = gemm(a4, To, 4 * CH, U.pw2_w, U.pw2_b, CH, y); a.res_scale = U.gamma; a.res = y; conv(a); }
            cur = y; Tc = To;
        }
        // ---- SnakeBeta decoder: conv_in, 4 x (snake, transposed conv, 3 residual units), snake, conv_out ----
        // SnakeBeta outputs travel between the decoder's convs as (hi, lo) fp16 pairs (ConvArgs::in_planes / out2_planes): the producer's
        // epilogue splits each element once, the consumers stage it without converting.  Needs every decoder conv on the split-precision
        // path with 96-multiple widths (0.6B / 1.7B: 1536 .. 96); the last activation feeds the fp32 C_out = 1 conv and stays fp32.
        const bool fp32_act = knob("Q3TTS_CONV_FP32_ACT") != nullptr || knob("Q3TTS_CONV_GENERIC_EPILOGUE") != nullptr;   // A/B switches
        bool act_planes = !fp32_act && !W.planes.empty() && CH % 32 == 0 && W.planes.count(W.conv_in.w) && !W.snake_pre.empty();
        for (int i = 0, Cw = D; i <= c.cd_n_blocks; ++i, Cw /= 2) act_planes = act_planes && Cw % 96 == 0;
        for (const CodecW::Block& B : W.blocks) {
            act_planes = act_planes && W.planes.count(B.tconv.w);
            for (int u = 0; u < 3; ++u) act_planes = act_planes && W.planes.count(B.res[u].c1.w) && W.planes.count(B.res[u].c2.w);
        }
        float* x = take(nbz * Tc * D);
        float* sx = take(nbz * Tc * D);
        { ConvArgs a; a.in = cur; a.T_in = Tc; a.C_in = CH; a.out = x; a.T_out = Tc; a.C_out = D; a.W = W.conv_in.w; a.bias = W.conv_in.b; a.taps = 7;
          a.in_ustride = nbatch > 1 ? h_ustride : 0;   // the batched front pads every utterance to the job's longest; a group runs at its own longest
          a.out2 = sx; a.snake_alpha = W.blocks[0].act.alpha; a.snake_beta = W.blocks[0].act.beta; a.out2_planes = act_planes; conv(a); }
        int C = D;
        static const int dil[3] = { 1, 3, 9 };
        for (int i = 0; i < c.cd_n_blocks; ++i) {
            const CodecW::Block& B = W.blocks[i];
            const int r = c.cd_up_rates[i], Co = C / 2;
            int left = 0;
            const int To = tconv_out_len(c, Tc, 2 * r, r, &left);
            float* nx = take(nbz * To * Co);
            float* ns = take(nbz * To * Co);
            float* nt = take(nbz * To * Co);
            { ConvArgs a; a.in = sx; a.T_in = Tc; a.C_in = C; a.out = nx; a.T_out = To; a.C_out = Co; a.W = B.tconv.w; a.bias = B.tconv.b;
              a.taps = 2 * r; a.transposed = 1; a.stride = r; a.left = left; a.in_planes = act_planes;
              a.out2 = ns; a.snake_alpha = B.res[0].a1.alpha; a.snake_beta = B.res[0].a1.beta; a.out2_planes = act_planes; conv(a); }
            for (int u = 0; u < 3; ++u) {
                const CodecW::Res& R = B.res[u];
                const SnakeP nxt = u < 2 ? B.res[u + 1].a1 : (i + 1 < c.cd_n_blocks ? W.blocks[i + 1].act : W.snake_out);
                const bool nxt_planes = act_planes && !(u == 2 && i + 1 == c.cd_n_blocks);   // the very last activation feeds the fp32 conv_out
                // 96-channel block: the whole residual unit (7-tap conv, SnakeBeta, 1x1 conv, + x) in one launch — the intermediate stays in
                // the CU (k_conv_split<..., F2>): 4 activation passes through HBM instead of 6, one launch instead of two.  The unit reads
                // snake(x) with a tap halo reaching into its neighbours' rows, so the next layer's snake(x') goes to the OTHER buffer
                // (ns <-> nt); x itself is updated in place (every element is read and written by the same thread).
                const auto p2 = W.planes.find(R.c2.w);
                if (Co == 96 && p2 != W.planes.end() && W.planes.count(R.c1.w) && !knob("Q3TTS_NO_FUSED_RES")) {
                    ConvArgs a; a.in = ns; a.T_in = To; a.C_in = Co; a.out = nx; a.T_out = To; a.C_out = Co; a.W = R.c1.w; a.bias = R.c1.b;
                    a.taps = 7; a.dil = dil[u]; a.mid_alpha = R.a2.alpha; a.mid_beta = R.a2.beta;
                    a.W2 = R.c2.w; a.W2h = p2->second.hi; a.W2l = p2->second.lo; a.W2fh = p2->second.fh; a.W2fl = p2->second.fl; a.w2_scale_inv = p2->second.scale_inv; a.w2_lo_zero = p2->second.lo_zero; a.bias2 = R.c2.b;
                    a.res = nx; a.out2 = nt; a.snake_alpha = nxt.alpha; a.snake_beta = nxt.beta;
                    a.in_planes = act_planes; a.out2_planes = nxt_planes;
                    conv(a);
                    std::swap(ns, nt);
                    continue;
                }
                { ConvArgs a; a.in = ns; a.T_in = To; a.C_in = Co; a.out = nullptr; a.T_out = To; a.C_out = Co; a.W = R.c1.w; a.bias = R.c1.b;
                  a.taps = 7; a.dil = dil[u]; a.out2 = nt; a.snake_alpha = R.a2.alpha; a.snake_beta = R.a2.beta;
                  a.in_planes = act_planes; a.out2_planes = act_planes; conv(a); }
                { ConvArgs a; a.in = nt; a.T_in = To; a.C_in = Co; a.out = nx; a.T_out = To; a.C_out = Co; a.W = R.c2.w; a.bias = R.c2.b;
                  a.taps = 1; a.res = nx; a.out2 = ns; a.snake_alpha = nxt.alpha; a.snake_beta = nxt.beta;
                  a.in_planes = act_planes; a.out2_planes = nxt_planes; conv(a); }
            }
            x = nx; sx = ns; Tc = To; C = Co;
        }
        pcm = take(nbz * Tc);
        { ConvArgs a; a.in = sx; a.T_in = Tc; a.C_in = C; a.out = pcm; a.T_out = Tc; a.C_out = 1; a.W = W.conv_out.w; a.bias = W.conv_out.b;
          a.taps = 7; a.clamp = 1; conv(a); }
        if (!plan && nbatch > 1) { W.dbg_sx = sx; W.dbg_pcm = pcm; W.dbg_T = Tc; W.dbg_C = C; W.dbg_nb = nbatch; }
        n_pcm = Tc;
        if (plan && take.off > W.arena_bytes[lane]) {
            Q3_HIP_CHECK(hipStreamSynchronize(stream));   // the lane's stream, not the engine's
            W.dbg_sx = W.dbg_pcm = nullptr;               // they may point into the arena that goes
            regrow(W.arena[lane], W.arena_bytes[lane], take.off, 1, true);
        }
    }
    *pcm_dev = pcm;
    return n_pcm;
}


// ConvNeXt upsampling stages over row blocks [sequence][*per] (T rows in all): the transposed convs have kernel == stride (every input row
// expands on its own), the depthwise causal conv stops at each sequence's first row, the pointwise layers are plain GEMMs.  take(n)
// hands out n floats of the caller's arena, conv(a) launches with the caller's slab and weight planes.  Shared by codec_pre_batch (whole
// utterances) and the batched push (the streams' windows).  *per leaves as the rows per sequence of the result.
static float* upsample_blocks(const q3tts_config& c, const CodecW& W, float* cur, int T, int* per, CodecBump& take, const ConvLauncher& conv, hipStream_t stream) {
    const int CH = c.cd_hidden;
    int Tc = T;
    for (int s2 = 0; s2 < c.cd_n_up; ++s2) {
        const CodecW::Up& U = W.up[s2];
        const int f = c.cd_up_ratios[s2];
        if (U.tconv.k != f) throw Error("codec: batched upsampling needs kernel == stride");
        const int To = Tc * f;
        float* y = take((size_t)To * CH);
        float* ln = take((size_t)To * CH);
        float* a4 = take((size_t)To * 4 * CH);
        { ConvArgs a; a.in = cur; a.T_in = Tc; a.C_in = CH; a.out = y; a.T_out = To; a.C_out = CH; a.W = U.tconv.w; a.bias = U.tconv.b;
          a.taps = f; a.transposed = 1; a.stride = f; a.left = 0; conv(a); }
        *per *= f;
        launch_dwconv_ln(y, To, CH, U.dw_w, U.dw_b, U.ln_w, U.ln_b, ln, stream, *per);
        { ConvArgs a; a.in = ln; a.T_in = To; a.C_in = CH; a.out = a4; a.T_out = To; a.C_out = 4 * CH; a.W = U.pw1_w; a.bias = U.pw1_b; a.act = 1; conv(a); }
        { ConvArgs a; a.in = a4; a.T_in = To; a.C_in = 4 * CH; a.out = y; a.T_out = To; a.C_out = CH; a.W = U.pw2_w; a.bias = U.pw2_b; a.res_scale = U.gamma; a.res = y; conv(a); }
        cur = y; Tc = To;
    }
    return cur;
}

// ------------------------------------------------------------------------------------------------
// Pre-transformer of a whole job in one pass: the utterances' frames are laid out as [utterance][Fp] rows (Fp = the longest, shorter
// ones padded: attention is causal, so padding rows never reach a real one), every linear layer is ONE matrix-core GEMM over all rows
// (weights streamed once, full grids) instead of one short GEMM per utterance, attention runs with the utterance as its batch
// dimension.  Returns the normalised hidden rows [n][Fp][cd_hidden] (valid until the next call); codes: [n][codes_stride_frames][groups].
// ------------------------------------------------------------------------------------------------
const float* Engine::codec_pre_batch(const int32_t* codes_dev, int codes_stride_frames, int n, int Fp, bool with_upsampling, int* rows_per_utt_out,
                                     const int* perm_host) {
    if (!codec) throw Error("codec decoder not finalized");
    CodecW& W = *codec;
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim, FF = c.cd_ffn;
    int P = 1, pshift = 0;
    while (P < Fp) { P <<= 1; ++pshift; }
    if (W.rope_P < P) throw Error("codec_pre_batch: RoPE tables not prepared");
    const size_t rows = (size_t)n * Fp;
    const size_t need = codec_batch_arena_bytes(c, (size_t)n, (size_t)Fp, (size_t)P, with_upsampling);
    if (W.batch_arena_bytes < need) regrow(W.batch_arena, W.batch_arena_bytes, need);
    codec_identity_pages(*this, n);   // [0, n): identity page table; [n_cap, 2 n_cap): the job's utterance order (perm)
    const int* perm_d = nullptr;
    if (perm_host) {   // row block y of every buffer holds utterance perm[y] (the scheduler sorts by length so that decoder groups pad little)
        Q3_HIP_CHECK(hipMemcpyAsync(W.batch_pages + W.batch_pages_n, perm_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
        perm_d = W.batch_pages + W.batch_pages_n;
    }
    CodecBump take{ W.batch_arena };
    float* h = take(rows * CH);
    float* hn = take(rows * CH);
    float* att = take(rows * CH);
    float* qkvb = take(rows * 3 * CH);
    float* ub = take(rows * FF);
    float* gb = take(rows * FF);
    float* kc = take((size_t)n * NH * P * HD);
    float* vc = take((size_t)n * NH * P * HD);
    const ConvLauncher conv{ W, take(CODEC_KSLAB_FLOATS), stream };
    const int T = (int)rows;
    if (!W.win0_recorded) { Q3_HIP_CHECK(hipEventRecord(W.win0, stream)); W.win0_recorded = true; }   // the vocoder window starts here
    launch_code_embed_mean(W.code_embed, codes_dev, Fp, c.n_groups, c.cd_codebook, CH, h, stream, n, (size_t)codes_stride_frames * c.n_groups, perm_d);
    pre_transformer_layers(c, W, T, PreBufs{ h, hn, att, qkvb, ub, gb }, conv, [&](int) {
        launch_rope_store(qkvb, 3 * CH, Fp, NH, NH, HD, W.rope_cos, W.rope_sin, kc, vc, P, stream, n);
        launch_attn(codec_attn_args(c, qkvb, att, kc, vc, W.batch_pages, pshift, 0, n, Fp), stream);
    }, stream);
    launch_rmsnorm_rows(h, W.norm, c.cd_rms_eps, T, CH, h, stream);
    if (rows_per_utt_out) *rows_per_utt_out = Fp;
    if (!with_upsampling) return h;
    int per = Fp;
    float* cur = upsample_blocks(c, W, h, T, &per, take, conv, stream);
    if (rows_per_utt_out) *rows_per_utt_out = per;
    return cur;
}

// ------------------------------------------------------------------------------------------------
// Vocoder side of the scheduler (q3tts_synthesize_schedule_host).  A slot that finishes copies its codes into the job's buffer on the
// engine stream (codec_stash) and is free at once; when the decode queue has run dry the utterances are vocoded over the side lanes
// (codec_async_submit_dev / codec_async_drain), their small-grid kernels overlapping each other.  Vocoding while other slots still
// decode was measured and dropped: the conv kernels own whole CUs and stream gigabytes through L2 / MALL, so every decode step of the
// latency-bound chain got 12 % longer and the job 10 % slower than with the two phases back to back (profiles/r01_negative_results.txt).
// ------------------------------------------------------------------------------------------------
// Forget every queued vocoder result without delivering it: after a failure inside the vocoder phase the pending items still hold the
// failed job's host pointers (pcm_out rows, pcm_len entries), which a later job's drain must never write through.
void Engine::codec_async_abort() {
    if (!codec) return;
    CodecW& W = *codec;
    for (int i = 0; i < W.nlane; ++i) {
        if (i > 0 && W.lane_stream[i]) (void)hipStreamSynchronize(W.lane_stream[i]);
        W.pend[i].items.clear();
        W.pend[i].frames = 0;
        W.pend[i].busy = false;
    }
    if (stream || null_stream) (void)hipStreamSynchronize(stream);
    W.window_open = false; W.win0_recorded = false;
    W.submits = 0;
}

void Engine::codec_async_prepare(int max_frames, int n_utt) {
    if (!codec) throw Error("codec decoder not finalized");
    CodecW& W = *codec;
    codec_async_abort();   // a previous job that failed mid-way must not leak its pending items into this one
    // fault injection for the tests (tests/test_gpu_edges.py): only an engine created with Q3TTS_FLAG_TEST_HOOKS reads the variable, so a
    // stray environment setting cannot fail a production job
    const char* fv = (flags & Q3TTS_FLAG_TEST_HOOKS) ? getenv("Q3TTS_TEST_FAIL_VOCODER_SUBMIT") : nullptr;
    W.fail_at_submit = fv ? atoi(fv) : 0;
    int P = 1;
    while (P < max_frames) P <<= 1;
    if (W.rope_P < P) {   // grow the shared RoPE tables before any lane is in flight
        int32_t* tmp = nullptr; float* dummy = nullptr;
        Q3_HIP_CHECK(hipMalloc((void**)&tmp, (size_t)max_frames * c.n_groups * sizeof(int32_t)));
        Q3_HIP_CHECK(hipMemset(tmp, 0, (size_t)max_frames * c.n_groups * sizeof(int32_t)));
        codec_run(tmp, max_frames, &dummy, 0);
        sync();
        (void)hipFree(tmp);
    }
    const size_t need = (size_t)n_utt * max_frames * c.n_groups;
    if (W.job_codes_n < need) regrow(W.job_codes, W.job_codes_n, need);
    W.rr = 0;   // a job's first utterances always land on the same lanes (their arenas are already sized)
    W.win0_recorded = false;
    if (!W.fork) { Q3_HIP_CHECK(hipEventCreateWithFlags(&W.fork, hipEventDisableTiming)); Q3_HIP_CHECK(hipEventCreate(&W.win0)); Q3_HIP_CHECK(hipEventCreate(&W.win1)); }
}

// slot's first nf frames -> row `utt` of the job buffer (stride = row_frames frames); ordered on the engine stream, so the slot may be re-armed next
const int32_t* Engine::codec_stash(int slot, int nf, int utt, int row_frames) {
    CodecW& W = *codec;
    const int G = c.n_groups;
    int32_t* dst = W.job_codes + (size_t)utt * row_frames * G;
    if (nf > 0) Q3_HIP_CHECK(hipMemcpyAsync(dst, codes_d + (size_t)slot * max_frames_cap * G, (size_t)nf * G * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    return dst;
}

// host codes [n_utt][row_frames][n_groups] -> the job buffer (after codec_async_prepare(row_frames, n_utt)); returns once they are in HBM
void Engine::codec_job_upload(const int32_t* host, int n_utt, int row_frames) {
    CodecW& W = *codec;
    const size_t n = (size_t)n_utt * row_frames * c.n_groups;
    if (n > W.job_codes_n) throw Error("codec_job_upload: job buffer not prepared");
    Q3_HIP_CHECK(hipMemcpyAsync(W.job_codes, host, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    sync();
}

const int32_t* Engine::codec_job_codes(int utt, int row_frames) { return codec->job_codes + (size_t)utt * row_frames * c.n_groups; }

void Engine::codec_async_drain_lane(int lane) {
    CodecW& W = *codec;
    CodecW::Pending& p = W.pend[lane];
    if (!p.busy) return;
    Q3_HIP_CHECK(hipStreamSynchronize(W.lane_stream[lane]));
    for (const CodecW::Item& it : p.items) {
        const int64_t m = std::min(it.n, it.cap);
        if (it.user && m > 0) memcpy(it.user, W.pinned[lane] + it.off, (size_t)m * sizeof(float));
        if (it.len) *it.len = it.n;
    }
    total_codec_frames += p.frames;
    p.items.clear();
    p.busy = false;
}

void Engine::codec_async_submit_dev(const int32_t* codes_dev, int nf, float* user_pcm, int64_t cap, int64_t* len_out, const float* h_in, int h_stage) {
    CodecW& W = *codec;
    if (len_out) *len_out = 0;
    if (nf <= 0) return;   // the reference returns an empty vector when no frame was generated (tts_onnx.cpp:418)
    const int lane = W.nlane > 1 ? 1 + (W.rr++ % (W.nlane - 1)) : 0;
    codec_async_drain_lane(lane);
    if (W.fail_at_submit > 0 && ++W.submits == W.fail_at_submit) throw Error("vocoder submit failed (injected by Q3TTS_TEST_FAIL_VOCODER_SUBMIT)");
    if (!W.window_open) {   // the lanes start behind everything the engine stream has queued (the stashed codes among it)
        if (!W.win0_recorded) { Q3_HIP_CHECK(hipEventRecord(W.win0, stream)); W.win0_recorded = true; }
        Q3_HIP_CHECK(hipEventRecord(W.fork, stream));
        for (int i = 1; i < W.nlane; ++i) Q3_HIP_CHECK(hipStreamWaitEvent(W.lane_stream[i], W.fork, 0));
        W.window_open = true;
    }
    if (!W.lane_done[lane]) Q3_HIP_CHECK(hipEventCreateWithFlags(&W.lane_done[lane], hipEventDisableTiming));
    hipStream_t ls = W.lane_stream[lane];
    float* pcm_d = nullptr;
    const int64_t n = codec_run(codes_dev, nf, &pcm_d, lane, h_in, h_stage);
    const int64_t m = std::min(n, cap);
    if ((size_t)m > W.pinned_floats[lane]) regrow_pinned(W.pinned[lane], W.pinned_floats[lane], (size_t)m);
    if (m > 0) Q3_HIP_CHECK(hipMemcpyAsync(W.pinned[lane], pcm_d, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, ls));
    Q3_HIP_CHECK(hipEventRecord(W.lane_done[lane], ls));
    CodecW::Pending& p = W.pend[lane];
    p.items.assign(1, CodecW::Item{ user_pcm, n, cap, 0, len_out });
    p.frames = nf; p.busy = true;
}

// ------------------------------------------------------------------------------------------------
// Streaming decode with CARRIED state (the reference decodes the whole utterance in one run_vocoder call,
// /root/reference/src/tts_onnx.cpp:759-776, :430).  The decoder is causal.  Its only long memory is the pre-transformer (8 layers of
// 72-frame sliding-window attention: 568 frames of receptive field): a stream keeps every layer's K / V rows and the transformer's
// output rows, so a push of n new frames runs the transformer on n rows (positions n_done .. n_done + n, attention over the cached
// window) instead of over the history.  Everything behind it — ConvNeXt upsampling, the conv decoder — looks back a few frames only
// (stage_b_context: depthwise k7 convs, the 2r-tap transposed convs, three 7-tap dilated convs per block): it is decoded over the
// window [n_done - context, n_done + n) of the kept transformer rows and the new frames' samples are cut out, exactly as the windowed
// range decode does for the whole network.  Work per push: O(n + context), exact (same kernels as the one-shot decode on the same rows;
// only the GEMM tile shapes a short launch picks differ).
// ------------------------------------------------------------------------------------------------
int Engine::codec_stage_b_context() const { return q3::codec_stage_b_context(c); }

int Engine::codec_stream_begin(int max_frames) {
    if (!codec) throw Error("codec decoder not finalized");
    if (max_frames < 1 || max_frames > (1 << 20)) throw Error("codec_stream_begin: max_frames out of range");
    CodecW& W = *codec;
    int sid = -1;
    for (size_t i = 0; i < W.streams.size(); ++i) if (!W.streams[i].used) { sid = (int)i; break; }
    if (sid < 0) { W.streams.emplace_back(); sid = (int)W.streams.size() - 1; }
    CodecW::Stream& S = W.streams[(size_t)sid];
    // buffers sized for pushes of up to 64 frames (16.8 MB of K / V + 0.4 MB of rows at 0.6B dims, whatever max_frames is); a larger
    // push grows them (codec_stream_fit).  Kept across streams: begin / end of a pooled stream allocate nothing.
    S.kv_rows = 0; S.h_rows = 0;                       // nothing of the buffers' previous stream is kept
    codec_stream_fit(sid, std::min(max_frames, 64));
    S.cap = max_frames;
    S.used = true; S.n_done = 0; S.delivered = false;
    for (int& id : S.stage) id = -1;
    int P = 1;
    while (P < max_frames) P <<= 1;
    codec_rope_tables(P);   // positions are absolute in the RoPE tables (grow-only, shared)
    return sid;
}

// make room for a push of n frames: K / V rows [kv_rows, kv_rows + n) and hpost rows [h_rows, h_rows + n) exist afterwards, the rows a
// later query / the stages behind the transformer still need are kept (moved to the front of the buffer, or into a larger one)
void Engine::codec_stream_fit(int sid, int n) {
    CodecW& W = *codec;
    CodecW::Stream& S = W.streams[(size_t)sid];
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim;
    const int keep = std::max(c.cd_window - 1, 0), ctx = codec_stage_b_context();
    const size_t blocks = (size_t)c.cd_layers * 2 * NH;   // (layer, k | v, head) row blocks of P rows each
    if (S.kv == nullptr || S.kv_rows + n > S.P) {
        const int keepN = std::min(keep, S.kv_rows);
        if (S.kv == nullptr || 2 * keep + n > S.P) {       // grow (or first allocation): P rows so that an in-place move never overlaps
            int P = 64, pshift = 6;
            while (P < 2 * keep + n) { P <<= 1; ++pshift; }
            float* nk = nullptr;
            Q3_HIP_CHECK(hipMalloc((void**)&nk, blocks * P * HD * sizeof(float)));
            if (S.kv && keepN > 0)
                Q3_HIP_CHECK(hipMemcpy2DAsync(nk, (size_t)P * HD * sizeof(float), S.kv + (size_t)(S.kv_rows - keepN) * HD, (size_t)S.P * HD * sizeof(float),
                                              (size_t)keepN * HD * sizeof(float), blocks, hipMemcpyDeviceToDevice, stream));
            if (S.kv) { sync(); (void)hipFree(S.kv); }
            S.kv = nk; S.P = P; S.pshift = pshift;
        } else if (keepN > 0) {                            // kv_rows > P - n >= 2 keep: source rows [kv_rows - keepN, kv_rows) lie behind the destination rows [0, keepN)
            Q3_HIP_CHECK(hipMemcpy2DAsync(S.kv, (size_t)S.P * HD * sizeof(float), S.kv + (size_t)(S.kv_rows - keepN) * HD, (size_t)S.P * HD * sizeof(float),
                                          (size_t)keepN * HD * sizeof(float), blocks, hipMemcpyDeviceToDevice, stream));
        }
        S.kv_rows = keepN;
    }
    if (S.hpost == nullptr || S.h_rows + n > S.h_cap) {
        const int ctxN = std::min(ctx, S.h_rows);
        if (S.hpost == nullptr || 2 * ctx + n > S.h_cap) {
            const int cap = 2 * ctx + std::max(n, 64);
            float* nh = nullptr;
            Q3_HIP_CHECK(hipMalloc((void**)&nh, (size_t)cap * CH * sizeof(float)));
            if (S.hpost && ctxN > 0)
                Q3_HIP_CHECK(hipMemcpyAsync(nh, S.hpost + (size_t)(S.h_rows - ctxN) * CH, (size_t)ctxN * CH * sizeof(float), hipMemcpyDeviceToDevice, stream));
            if (S.hpost) { sync(); (void)hipFree(S.hpost); }
            S.hpost = nh; S.h_cap = cap;
        } else if (ctxN > 0) {                             // h_rows > h_cap - n >= 2 ctx: no overlap
            Q3_HIP_CHECK(hipMemcpyAsync(S.hpost, S.hpost + (size_t)(S.h_rows - ctxN) * CH, (size_t)ctxN * CH * sizeof(float), hipMemcpyDeviceToDevice, stream));
        }
        S.h_rows = ctxN;
    }
}

static CodecW::Stream& open_stream(CodecW* W, int sid, const char* fn) {   // the open stream behind an id, or fn's refusal
    if (!W || sid < 0 || sid >= (int)W->streams.size() || !W->streams[(size_t)sid].used) throw Error(std::string(fn) + ": no such stream");
    return W->streams[(size_t)sid];
}

void Engine::codec_stream_end(int sid) {
    CodecW::Stream& S = open_stream(codec, sid, "codec_stream_end");
    S.used = false;        // buffers are kept for the next stream of this size
    S.n_done = 0;
    for (int k = 0; k < SK_N; ++k) {
        if (S.stage[k] >= 0) stages[k]->end(S.stage[k]);
        S.stage[k] = -1;
    }
}

// The setters: the stream must not have delivered a sample; `make` begins the new stage or returns -1 for the "no stage" values, and a
// refusal of it comes before the old stage goes.
static void stream_set_stage(Engine& e, int sid, const char* fn, int kind, const std::function<int()>& make) {
    CodecW::Stream& S = open_stream(e.codec, sid, fn);
    if (S.delivered) throw Error(std::string(fn) + ": stream " + std::to_string(sid) + " has already delivered samples");
    const int id = make();
    if (S.stage[kind] >= 0) e.stages[kind]->end(S.stage[kind]);
    S.stage[kind] = id;
}

void Engine::codec_stream_set_level(int sid, int gain_cb, int ceiling) {
    stream_set_stage(*this, sid, "codec_stream_set_level", SK_LEVEL, [&] {
        try { level_check(gain_cb, ceiling); } catch (const std::invalid_argument& ex) { throw Error(std::string("codec_stream_set_level: ") + ex.what()); }
        return gain_cb == 0 && ceiling == 0 ? -1 : level.begin(gain_cb, ceiling);
    });
}

void Engine::codec_stream_set_pitch(int sid, int ratio) {
    stream_set_stage(*this, sid, "codec_stream_set_pitch", SK_PITCH, [&] { return ratio == 1000 ? -1 : pitch.begin(ratio); });
}

void Engine::codec_stream_set_loudness(int sid, int target, int range, int start) {   // every value is a stage (target 0: a meter)
    stream_set_stage(*this, sid, "codec_stream_set_loudness", SK_LOUD, [&] {
        try { loudness_check(target, range, start); } catch (const std::invalid_argument& ex) { throw Error(std::string("codec_stream_set_loudness: ") + ex.what()); }
        return loud.begin(target, range, start);
    });
}

void Engine::codec_stream_set_tone(int sid, int n, const ToneSection* sections) {
    stream_set_stage(*this, sid, "codec_stream_set_tone", SK_TONE, [&] {
        if (n == 0) return -1;
        try { tone_check(n, sections); } catch (const std::invalid_argument& ex) { throw Error(std::string("codec_stream_set_tone: ") + ex.what()); }
        return tone.begin(n, sections);
    });
}

void Engine::codec_stream_set_speed(int sid, int speed_permille) {
    stream_set_stage(*this, sid, "codec_stream_set_speed", SK_SPEED, [&] { return speed_permille == 1000 ? -1 : speed.begin(speed_permille); });
}

void Engine::codec_stream_set_sink(int sid, int rate, int format) {
    stream_set_stage(*this, sid, "codec_stream_set_sink", SK_SINK, [&] {
        if (!pcm_format_known(format)) throw Error("codec_stream_set_sink: format " + std::to_string(format) + " is neither Q3TTS_PCM_F32 nor Q3TTS_PCM_S16, nor Q3TTS_PCM_MULAW (2) or Q3TTS_PCM_ALAW (3)");
        return rate == 24000 && format == Q3TTS_PCM_F32 ? -1 : sink.begin(rate, format);
    });
}

int Engine::codec_stream_frames(int sid) const {
    return open_stream(codec, sid, "codec_stream").n_done;
}

// n new frames (codes_dev: int32 [n][n_groups] on the device) -> the samples they own, *pcm_dev pointing into the engine's decode arena
// (valid until the next decode on the engine's stream); returns the sample count
int64_t Engine::codec_stream_push_dev(int sid, const int32_t* codes_dev, int n, float** pcm_dev) {
    CodecW::Stream& S = open_stream(codec, sid, "codec_stream_push");
    CodecW& W = *codec;
    if (n < 1) throw Error("codec_stream_push: no frames");
    if (S.has()) throw Error("codec_stream_push: stream " + std::to_string(sid) + S.has() + ": push it through the batched entry that takes any format");
    if (S.n_done + n > S.cap) throw Error("codec_stream_push: more frames than the stream was opened for");
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim, FF = c.cd_ffn;
    const int a0 = S.n_done, b0 = a0 + n, T = n;
    codec_stream_fit(sid, n);
    const int k0 = S.kv_rows, h0 = S.h_rows;   // where this push's rows go in the sliding buffers (position a0 = K / V row k0 = hpost row h0)
    const size_t need = codec_stream_arena_bytes(c, (size_t)T);
    if (W.stream_arena_bytes < need) regrow(W.stream_arena, W.stream_arena_bytes, need);
    CodecBump take{ W.stream_arena };
    float* h = take((size_t)T * CH);
    float* hn = take((size_t)T * CH);
    float* att = take((size_t)T * CH);
    float* qkvb = take((size_t)T * 3 * CH);
    float* ub = take((size_t)T * FF);
    float* gb = take((size_t)T * FF);
    const ConvLauncher conv{ W, take(CODEC_KSLAB_FLOATS), stream };
    // ---- the pre-transformer on the new rows: positions [a0, b0), keys / values of earlier frames from the stream's caches ----
    const int half = HD / 2;
    const size_t layer_kv = (size_t)NH * S.P * HD;
    launch_code_embed_mean(W.code_embed, codes_dev, T, c.n_groups, c.cd_codebook, CH, h, stream);
    pre_transformer_layers(c, W, T, PreBufs{ h, hn, att, qkvb, ub, gb }, conv, [&](int l) {
        float* kc = S.kv + (size_t)l * 2 * layer_kv;
        float* vc = kc + layer_kv;
        // row t of this push is position a0 + t: the tables and the cache rows start there
        launch_rope_store(qkvb, 3 * CH, T, NH, NH, HD, W.rope_cos + (size_t)a0 * half, W.rope_sin + (size_t)a0 * half, kc + (size_t)k0 * HD, vc + (size_t)k0 * HD, S.P, stream);
        // pos_scalar = k0: cache rows are addressed relative to the sliding buffer; every row a window can reach is in it (RoPE is already applied, absolute)
        launch_attn(codec_attn_args(c, qkvb, att, kc, vc, W.page_table, S.pshift, k0, 1, T), stream);
    }, stream);
    launch_rmsnorm_rows(h, W.norm, c.cd_rms_eps, T, CH, S.hpost + (size_t)h0 * CH, stream);
    // ---- everything behind the transformer over the window [sB, b0) of its kept output rows ----
    const int sB = std::max(0, a0 - codec_stage_b_context());   // h0 >= a0 - sB: codec_stream_fit keeps that many rows
    const CodecCut cut = codec_window_cut(c, a0, n, a0 - sB);
    float* pcm_d = nullptr;
    if (h0 < a0 - sB) throw Error("codec_stream_push: the kept transformer rows do not cover the look-back window");
    const int64_t n_win = codec_run(nullptr, b0 - sB, &pcm_d, 0, S.hpost + (size_t)(h0 - (a0 - sB)) * CH, 1);
    if (!cut.matches(n_win)) throw Error("codec_stream_push: window arithmetic does not match the decoder length formula");
    S.n_done = b0; S.kv_rows = k0 + n; S.h_rows = h0 + n; S.delivered = S.delivered || cut.n_own > 0;
    if (pcm_dev) *pcm_dev = pcm_d + cut.first;
    return cut.n_own;
}

int64_t Engine::codec_stream_push_host(int sid, const int64_t* codes, int n, float* pcm, int64_t cap) {
    if (n < 1) throw Error("codec_stream_push: no frames");
    std::vector<int32_t> tmp((size_t)n * c.n_groups);
    stage_codes<Error>(codes, tmp.size(), c.cd_codebook, tmp.data());
    if (n > max_frames_cap) throw Error("codec_stream_push: more frames in one push than the engine's frame capacity");
    Q3_HIP_CHECK(hipMemcpyAsync(codes_scratch_d, tmp.data(), tmp.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    float* pcm_d = nullptr;
    CodecTimed t(*this);
    const int64_t n_own = codec_stream_push_dev(sid, codes_scratch_d, n, &pcm_d);
    t.stop();
    return t.deliver(pcm_d, n_own, pcm, cap, n);
}

// ------------------------------------------------------------------------------------------------
// Batched push: n new frames for each of g streams in ONE set of launches per layer (a server with 64 live callers otherwise makes 64
// latency-bound pushes back to back every chunk: ~10 small launches per layer each, on grids of a handful of workgroups).  Rows are packed
// [stream][its new frames] (ragged n), every linear layer is one GEMM over all rows — weights streamed once — and the kernels that look
// at a position or at a stream's own buffers (code gather, RoPE + cache store, windowed attention, the final norm's scatter into hpost)
// find them in a descriptor table uploaded once per push (CodecStreamDesc).  Stream state stays where codec_stream_fit keeps it: the
// table carries pointers, so streams of different P mix freely and keep / move / grow work per stream as before.
// Behind the transformer the streams' windows [kept rows | new rows] are gathered into [g][Tw][hidden] blocks, upsampled together
// (upsample_blocks) and decoded with codec_run(nbatch = g).  A stream younger than codec_stage_b_context() frames has a shorter left
// context — its window starts at the utterance's first row, where the causal convs see nothing, not a neighbour's rows — so streams are
// grouped by left-context length; inside a group shorter pushes are right-padded with zero rows (exact: every layer is causal).
// Everything runs on the engine's stream, serially with the decode chain (vocoding beside decoding costs every decode step 12 %:
// profiles/r01_negative_results.txt).  PCM goes to the callers' host buffers; the call returns once it is there.
// ------------------------------------------------------------------------------------------------
void Engine::codec_stream_push_batch(StreamPush* ps, int g_all) {
    if (!codec) throw Error("codec decoder not finalized");
    CodecW& W = *codec;
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim, FF = c.cd_ffn;
    if (NH * HD != CH) throw Error("codec: heads*head_dim must equal hidden");
    // ---- every argument is checked before any stream's buffers are touched ----
    std::vector<int> live;
    for (int i = 0; i < g_all; ++i) {
        StreamPush& q = ps[i];
        q.n_own = 0;
        if (q.sid < 0 || q.sid >= (int)W.streams.size() || !W.streams[(size_t)q.sid].used) throw Error("codec_stream_push_batch: no such stream");
        for (int k = 0; k < i; ++k) if (ps[k].sid == q.sid) throw Error("codec_stream_push_batch: stream listed twice");
        if (q.n < 0) throw Error("codec_stream_push_batch: negative frame count");
        if (W.streams[(size_t)q.sid].n_done + q.n > W.streams[(size_t)q.sid].cap) throw Error("codec_stream_push_batch: more frames than the stream was opened for");
        if (q.n > 0 && !q.codes_dev) throw Error("codec_stream_push_batch: null codes");
        if (q.n > 0) live.push_back(i);
    }
    // streams with stages: their pushes' lengths by the host rules (which refuse a finished or full stage), before anything moves.  A
    // stage's input is the push of the stream's nearest earlier stage, or the vocoder's; only the last one delivers to the caller.
    std::vector<StagePush> sp[SK_N];             // sp[k][i] belongs to ps[i]; id == -1: stream i has no stage of kind k
    size_t st_out[SK_N] = {}, st_offs[SK_N] = {};
    int st_n[SK_N] = {}, st_any = 0;
    for (int k = 0; k < SK_N; ++k) sp[k].assign((size_t)g_all, StagePush());
    for (int i = 0; i < g_all; ++i) {
        const StreamPush& q = ps[i];
        const CodecW::Stream& S = W.streams[(size_t)q.sid];
        int64_t n24 = codec_len_of(c, S.n_done + q.n) - codec_len_of(c, S.n_done);
        int last = -1;
        for (int k = 0; k < SK_N; ++k) {
            if (S.stage[k] < 0) continue;
            StagePush& v = sp[k][(size_t)i];
            v.id = S.stage[k]; v.n_new = n24; v.finish = q.finish;
            st_out[k] += stages[k]->plan(v); st_offs[k] += (size_t)v.n_frames;
            ++st_n[k]; ++st_any;
            n24 = v.n_out; last = k;
        }
        if (last < 0) {
            if (q.finish) throw Error("codec_stream_push_batch: finish on stream " + std::to_string(q.sid) + ", which has no sink");
            continue;
        }
        sp[last][(size_t)i].out_host = q.pcm; sp[last][(size_t)i].cap = q.cap;
    }
    for (int k = 0; k < SK_N; ++k) if (st_n[k] > 0) stages[k]->reserve(st_n[k], st_out[k], st_offs[k]);
    auto prev_stage = [&](int k, int i) { do --k; while (k >= 0 && sp[k][(size_t)i].id < 0); return k; };   // stream i's nearest stage ahead of kind k; -1: the vocoder
    std::vector<StagePush> run[SK_N];            // per kind the pushes of one launch, and where each came from
    std::vector<int> src[SK_N];
    auto run_stages = [&]() {                    // at most one launch per kind, in the stages' order
        for (int k = 0; k < SK_N; ++k) {
            if (run[k].empty()) continue;
            stages[k]->launch(run[k].data(), (int)run[k].size());
            for (size_t j = 0; j < run[k].size(); ++j) { sp[k][(size_t)src[k][j]] = run[k][j]; ps[src[k][j]].n_own = run[k][j].n_out; }
            run[k].clear(); src[k].clear();
            for (int m = k + 1; m < SK_N; ++m) for (size_t j = 0; j < run[m].size(); ++j) {   // the stage behind this one reads its output where it lies
                const int i = src[m][j];
                if (prev_stage(m, i) != k) continue;
                if (run[m][j].n_new != sp[k][(size_t)i].n_out)
                    throw Error(std::string("codec_stream_push_batch: a ") + stages[m]->noun + "'s input length does not match its " + stages[k]->noun + "'s push");
                run[m][j].x_dev = sp[k][(size_t)i].out_dev;
            }
        }
    };
    auto commit_stages = [&]() {
        for (int k = 0; k < SK_N; ++k) for (int i = 0; i < g_all; ++i) if (sp[k][(size_t)i].id >= 0) stages[k]->commit(&sp[k][(size_t)i], 1);
    };
    auto queue_stages = [&](int i, const float* x_dev) -> bool {   // stream i's stages join the next launches; x_dev feeds the first of them
        bool any = false;
        for (int k = 0; k < SK_N; ++k) {
            if (sp[k][(size_t)i].id < 0) continue;
            run[k].push_back(sp[k][(size_t)i]); src[k].push_back(i);
            run[k].back().x_dev = x_dev;         // behind another stage: replaced by that stage's output in run_stages
            any = true;
        }
        return any;
    };
    auto finish_idle = [&]() -> bool {   // streams that finish without new frames: each stage's tail, in the stages' order
        bool any = false;
        for (int i = 0; i < g_all; ++i) if (ps[i].n == 0 && ps[i].finish && queue_stages(i, nullptr)) any = true;
        return any;
    };
    const int g = (int)live.size();
    if (g == 0) {   // no frames anywhere: only stages that finish have something to deliver
        if (!finish_idle()) return;
        run_stages();
        sync();
        commit_stages();
        return;
    }
    if (g > 65535) throw Error("codec_stream_push_batch: at most 65535 streams per call");
    const int ctxB = codec_stage_b_context();
    codec_push_order(live, [&](int x) { return std::min(W.streams[(size_t)ps[x].sid].n_done, ctxB); });   // mature streams (the common case) first
    std::vector<CodecStreamDesc>& D = W.sbatch_desc_h;
    D.assign((size_t)g, CodecStreamDesc());
    int T = 0, n_max = 0;
    for (int i = 0; i < g; ++i) {
        const StreamPush& q = ps[live[(size_t)i]];
        codec_stream_fit(q.sid, q.n);
        const CodecW::Stream& S = W.streams[(size_t)q.sid];
        CodecStreamDesc& d = D[(size_t)i];
        d.kv = S.kv; d.hpost = S.hpost; d.codes = q.codes_dev; d.P = S.P; d.k0 = S.kv_rows; d.h0 = S.h_rows; d.a0 = S.n_done; d.n = q.n; d.row_off = T;
        d.ctx = std::min(S.n_done, ctxB);
        if (d.k0 + d.n > S.P || d.h0 + d.n > S.h_cap) throw Error("codec_stream_push_batch: the stream's buffers do not hold the push");
        if (d.h0 < d.ctx) throw Error("codec_stream_push_batch: the kept transformer rows do not cover the look-back window");
        if (W.rope_P < d.a0 + d.n) throw Error("codec_stream_push_batch: RoPE tables not prepared");
        T += q.n; n_max = std::max(n_max, q.n);
    }
    const std::vector<CodecGroup> groups = codec_push_groups(g, [&](int i) { return D[(size_t)i].ctx; }, [&](int i) { return D[(size_t)i].n; });
    size_t back_rows = 0;   // rows of the largest group's gathered block
    for (const CodecGroup& G : groups) {
        for (int i = G.i0; i < G.i1; ++i) D[(size_t)i].blk = i - G.i0;
        back_rows = std::max(back_rows, (size_t)(G.i1 - G.i0) * G.Tw);
    }
    // ---- workspace ----
    const size_t need = codec_sbatch_push_bytes(c, (size_t)T, back_rows);
    if (W.sbatch_arena_bytes < need) regrow(W.sbatch_arena, W.sbatch_arena_bytes, need);
    if (W.sbatch_desc_n < (size_t)g) regrow(W.sbatch_desc, W.sbatch_desc_n, std::max((size_t)64, (size_t)g));
    Q3_HIP_CHECK(hipMemcpyAsync(W.sbatch_desc, D.data(), (size_t)g * sizeof(CodecStreamDesc), hipMemcpyHostToDevice, stream));
    CodecBump take{ W.sbatch_arena };
    float* h = take((size_t)T * CH);
    float* hn = take((size_t)T * CH);
    float* att = take((size_t)T * CH);
    float* qkvb = take((size_t)T * 3 * CH);
    float* ub = take((size_t)T * FF);
    float* gb = take((size_t)T * FF);
    const ConvLauncher conv{ W, take(CODEC_KSLAB_FLOATS), stream };
    float* win = take(back_rows * CH);
    const size_t off_back = take.off;
    Q3_HIP_CHECK(hipEventRecord(ev0, stream));
    // ---- the pre-transformer on all streams' new rows ----
    const CodecStreamDesc* dd = W.sbatch_desc;
    const bool win_attn = attn_streams_windowed(NH, HD, c.cd_window, 3 * CH, CH);
    launch_code_embed_mean_streams(W.code_embed, dd, g, n_max, c.n_groups, c.cd_codebook, CH, h, stream);
    pre_transformer_layers(c, W, T, PreBufs{ h, hn, att, qkvb, ub, gb }, conv, [&](int l) {
        launch_rope_store_streams(qkvb, 3 * CH, dd, g, n_max, l, NH, NH, HD, W.rope_cos, W.rope_sin, stream);
        if (win_attn) launch_attn_streams(qkvb, 3 * CH, att, CH, dd, g, n_max, l, NH, HD, c.cd_window, 1.0f / sqrtf((float)HD), stream);
        else for (int i = 0; i < g; ++i) {   // head sizes k_attn_win does not take (tiny configs): k_attn, exactly the single push's launch
            const CodecStreamDesc& d = D[(size_t)i];
            float* kc = d.kv + (size_t)l * 2 * NH * d.P * HD;
            launch_attn(codec_attn_args(c, qkvb + (size_t)d.row_off * 3 * CH, att + (size_t)d.row_off * CH, kc, kc + (size_t)NH * d.P * HD, W.page_table,
                                        W.streams[(size_t)ps[live[(size_t)i]].sid].pshift, d.k0, 1, d.n), stream);
        }
    }, stream);
    launch_rmsnorm_rows_streams(h, W.norm, c.cd_rms_eps, dd, g, n_max, CH, stream);
    // ---- everything behind the transformer, one group of equal left context at a time ----
    const bool batchable = codec_batchable();
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const CodecGroup& G = groups[gi];
        const int gk = G.i1 - G.i0;
        launch_gather_stream_rows(dd + G.i0, gk, G.Tw, CH, win, stream);
        take.off = off_back;
        int per = G.Tw;
        const float* hup = upsample_blocks(c, W, win, gk * G.Tw, &per, take, conv, stream);
        const size_t ustride = (size_t)per * CH;
        const bool last_group = gi + 1 == groups.size();
        auto deliver = [&](int i, const float* pcm_seq, int64_t Tp) {   // stream i's own samples out of its window's
            const CodecStreamDesc& d = D[(size_t)i];
            StreamPush& q = ps[live[(size_t)i]];
            const CodecCut cut = codec_window_cut(c, d.a0, d.n, d.ctx);
            const int64_t first = cut.first, n_own = cut.n_own;
            if (!cut.matches(Tp, d.ctx + d.n == G.Tw)) throw Error("codec_stream_push_batch: window arithmetic does not match the decoder length formula");
            q.n_own = n_own;
            int k0 = 0;
            while (k0 < SK_N && sp[k0][(size_t)live[(size_t)i]].id < 0) ++k0;
            if (k0 < SK_N) {   // through its stages, each in the group's one launch of its kind (run_stages), from where the samples lie
                if (sp[k0][(size_t)live[(size_t)i]].n_new != n_own)
                    throw Error(std::string("codec_stream_push_batch: a ") + stages[k0]->noun + "'s input length does not match the decoder length formula");
                (void)queue_stages(live[(size_t)i], pcm_seq + first);
                return;
            }
            const int64_t m = std::min(n_own, q.cap);
            if (m > 0 && q.pcm) Q3_HIP_CHECK(hipMemcpyAsync(q.pcm, pcm_seq + first, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, stream));
        };
        if (batchable && gk > 1) {   // the conv decoder of the whole group in one set of launches
            float* pcm_d = nullptr;
            const int64_t Tp = codec_run(nullptr, G.Tw, &pcm_d, 0, hup, 2, gk, ustride);
            if (last_group) Q3_HIP_CHECK(hipEventRecord(ev1, stream));
            for (int i = G.i0; i < G.i1; ++i) deliver(i, pcm_d + (size_t)(i - G.i0) * Tp, Tp);
            run_stages();
        } else {                     // one stream in the group, or a decoder the batched conv kernels do not cover: sequence by sequence
            for (int i = G.i0; i < G.i1; ++i) {
                float* pcm_d = nullptr;
                const int64_t Tp = codec_run(nullptr, G.Tw, &pcm_d, 0, hup + (size_t)(i - G.i0) * ustride, 2);
                if (last_group && i + 1 == G.i1) Q3_HIP_CHECK(hipEventRecord(ev1, stream));
                deliver(i, pcm_d, Tp);
                run_stages();   // before the next sequence's decode reuses the lane's workspace
            }
        }
    }
    (void)finish_idle();
    run_stages();
    if (st_any > 0) Q3_HIP_CHECK(hipEventRecord(ev1, stream));   // the push's time includes its stages
    sync();
    Q3_HIP_CHECK(hipEventElapsedTime(&last_codec_ms, ev0, ev1));
    total_codec_ms += last_codec_ms; total_codec_frames += T;
    for (int i = 0; i < g; ++i) {   // the streams advance only now: a failure above leaves every one of them where it was
        const CodecStreamDesc& d = D[(size_t)i];
        const StreamPush& q = ps[live[(size_t)i]];
        CodecW::Stream& S = W.streams[(size_t)q.sid];
        S.n_done = d.a0 + d.n; S.kv_rows = d.k0 + d.n; S.h_rows = d.h0 + d.n;
        S.delivered = S.delivered || q.n_own > 0;
        for (int k = 0; k < SK_N; ++k) S.delivered = S.delivered || (S.stage[k] >= 0 && sp[k][(size_t)live[(size_t)i]].n_new > 0);
    }
    commit_stages();
}

// host codes: stream s receives frames codes[frame_offsets[s] .. frame_offsets[s + 1]); validated as a whole before anything moves
void Engine::codec_stream_push_batch_host(int n_streams, const int32_t* sids, const int64_t* codes, const int32_t* frame_offsets, float* const* pcm_out,
                                          int64_t cap, int64_t* pcm_len, const uint8_t* finish, bool float_only) {
    if (!codec) throw Error("codec decoder not finalized");
    if (n_streams < 0) throw Error("codec_stream_push_batch: negative stream count");
    if (n_streams == 0) return;
    if (!sids || !frame_offsets) throw Error("codec_stream_push_batch: null argument");
    if (cap < 0) throw Error("codec_stream_push_batch: negative pcm_cap");
    CodecW& W = *codec;
    const int G = c.n_groups;
    if (frame_offsets[0] != 0) throw Error("codec_stream_push_batch: frame_offsets must start at 0");
    for (int i = 0; i < n_streams; ++i)
        if (frame_offsets[i + 1] < frame_offsets[i]) throw Error("codec_stream_push_batch: frame_offsets must not decrease");
    const size_t total = (size_t)frame_offsets[n_streams] * G;
    if (total > 0 && !codes) throw Error("codec_stream_push_batch: null codes");
    std::vector<int32_t> tmp(total);
    stage_codes<Error>(codes, total, c.cd_codebook, tmp.data());
    std::vector<StreamPush> ps((size_t)n_streams);
    for (int i = 0; i < n_streams; ++i) {   // the checks codec_stream_push_batch repeats, made here before the staging buffer may grow
        ps[(size_t)i].sid = sids[i]; ps[(size_t)i].n = frame_offsets[i + 1] - frame_offsets[i];
        ps[(size_t)i].pcm = pcm_out ? pcm_out[i] : nullptr; ps[(size_t)i].cap = cap;
        ps[(size_t)i].finish = finish && finish[i];
        if (float_only && sids[i] >= 0 && sids[i] < (int)W.streams.size() && W.streams[(size_t)sids[i]].used && W.streams[(size_t)sids[i]].has())
            throw Error("codec_stream_push_batch: stream " + std::to_string(sids[i]) + W.streams[(size_t)sids[i]].has() + ": the float entry serves streams without one");
        if (pcm_len) pcm_len[i] = 0;
    }
    if (W.sbatch_codes_n < total || !W.sbatch_codes) regrow(W.sbatch_codes, W.sbatch_codes_n, std::max(total, (size_t)1));
    if (total > 0) Q3_HIP_CHECK(hipMemcpyAsync(W.sbatch_codes, tmp.data(), total * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    for (int i = 0; i < n_streams; ++i) ps[(size_t)i].codes_dev = W.sbatch_codes + (size_t)frame_offsets[i] * G;
    try { codec_stream_push_batch(ps.data(), n_streams); } catch (...) { try { sync(); } catch (...) { } throw; }   // tmp must outlive the upload
    if (pcm_len) for (int i = 0; i < n_streams; ++i) pcm_len[i] = ps[(size_t)i].n_own;
}

// For every listed slot: the frames generated since the slot's previous streaming call, through the slot's implicit stream (the one
// slot_codec_stream_range uses: the two interleave), all slots in batched passes.  The codes are read where the sampler wrote them.
void Engine::slots_codec_decode_new(int n_slots, const int32_t* slots, float* const* pcm_out, int64_t cap, int64_t* pcm_len, int32_t* frame_begin, int32_t* frame_end,
                                   const int32_t* frame_limit, const int32_t* final_frames) {
    if (!codec) throw Error("codec decoder not finalized");
    if (n_slots < 0) throw Error("slots_codec_decode_new: negative slot count");
    if (n_slots == 0) return;
    if (!slots) throw Error("slots_codec_decode_new: null argument");
    if (cap < 0) throw Error("slots_codec_decode_new: negative pcm_cap");
    CodecW& W = *codec;
    for (int i = 0; i < n_slots; ++i) {
        if (slots[i] < 0 || slots[i] >= B) throw Error("slot out of range");
        for (int k = 0; k < i; ++k) if (slots[k] == slots[i]) throw Error("slots_codec_decode_new: slot listed twice");
    }
    std::vector<SlotState> st;
    slots_state(B, st);
    if ((int)W.slot_stream.size() < B) W.slot_stream.assign((size_t)B, -1);
    std::vector<StreamPush> ps((size_t)n_slots);
    for (int i = 0; i < n_slots; ++i) {
        const int slot = slots[i];
        int nf = st[(size_t)slot].active ? std::min(st[(size_t)slot].n_frames, max_frames_cap) : 0;
        int sid = W.slot_stream[(size_t)slot];
        // frame_limit (the live-text scheduler): frames past it wait for a later call; never below what the stream has already pushed
        if (frame_limit && sid >= 0 && W.streams[(size_t)sid].used && W.streams[(size_t)sid].n_done <= nf) nf = std::min(nf, std::max(frame_limit[i], W.streams[(size_t)sid].n_done));
        else if (frame_limit) nf = std::min(nf, std::max(frame_limit[i], 0));
        if (sid < 0 || !W.streams[(size_t)sid].used || W.streams[(size_t)sid].n_done > nf) {   // first call of the utterance, or a restart
            if (sid >= 0 && W.streams[(size_t)sid].used) codec_stream_end(sid);
            sid = codec_stream_begin(max_frames_cap);
            W.slot_stream[(size_t)slot] = sid;
        }
        // the scheduler's stages: a stream that has delivered nothing yet takes them (a primed stream included: they start from silence)
        const SlotStages& ss = slot_stages;
        const int* have = W.streams[(size_t)sid].stage;
        if (!W.streams[(size_t)sid].delivered) {
            if (ss.pitch > 0 && ss.pitch != 1000 && have[SK_PITCH] < 0) codec_stream_set_pitch(sid, ss.pitch);
            if (ss.sink_rate > 0 && have[SK_SINK] < 0) codec_stream_set_sink(sid, ss.sink_rate, ss.sink_format);
            if (ss.speed > 0 && ss.speed != 1000 && have[SK_SPEED] < 0) codec_stream_set_speed(sid, ss.speed);
            if (ss.tone_n > 0 && have[SK_TONE] < 0) codec_stream_set_tone(sid, ss.tone_n, ss.tone);
            if (ss.loud != 0 && have[SK_LOUD] < 0) codec_stream_set_loudness(sid, ss.loud_target, ss.loud_range, ss.loud_start);
            if ((ss.gain_cb != 0 || ss.ceiling != 0) && have[SK_LEVEL] < 0) codec_stream_set_level(sid, ss.gain_cb, ss.ceiling);
        }
        const int a = W.streams[(size_t)sid].n_done;
        StreamPush& q = ps[(size_t)i];
        q.sid = sid; q.n = nf - a; q.codes_dev = codes_d + ((size_t)slot * max_frames_cap + a) * c.n_groups;
        q.pcm = pcm_out ? pcm_out[i] : nullptr; q.cap = cap;
        q.finish = W.streams[(size_t)sid].has() && final_frames && final_frames[i] >= 0 && nf >= final_frames[i];
        if (frame_begin) frame_begin[i] = a;
        if (frame_end) frame_end[i] = nf;
        if (pcm_len) pcm_len[i] = 0;
    }
    codec_stream_push_batch(ps.data(), n_slots);
    if (pcm_len) for (int i = 0; i < n_slots; ++i) pcm_len[i] = ps[(size_t)i].n_own;
}

// ------------------------------------------------------------------------------------------------
// Priming: g open streams that hold no frames yet are put into the state a push of their first n frames would leave, without the audio.
// A stream needs very little of its past: the last window - 1 rotated K / V rows of every pre-transformer layer (all a later query can
// reach) and the last codec_stage_b_context() output rows (all the stages behind the transformer look back).  So only the
// pre-transformer runs, in codec_pre_batch's whole-utterance layout — rows [stream][Fp], Fp the longest n, shorter ones padded with zero
// rows (causal attention: padding never reaches a real row), scratch K / V [stream][head][Ps][d] per layer, every linear layer one
// GEMM over all rows, attention with the stream as its batch dimension: the launch count does not depend on g — and two copy kernels
// move the tails to the front of the streams' own buffers (k_prime_kv_tails after each layer's RoPE + store, k_prime_row_tails after the
// final norm), found through a descriptor table uploaded once.  The conv decoder and the upsampling stages do not run, and the streams'
// buffers keep the size codec_stream_begin gave them (a push of n frames grows them to hold n more rows, for good).
// Workspace: the batched push's arena and descriptor table (engine stream only, like the push).
// ------------------------------------------------------------------------------------------------
void Engine::codec_stream_prime_batch(const StreamPush* ps, int g_all) {
    if (!codec) throw Error("codec decoder not finalized");
    CodecW& W = *codec;
    const int CH = c.cd_hidden, NH = c.cd_heads, HD = c.cd_head_dim, FF = c.cd_ffn;
    if (NH * HD != CH) throw Error("codec: heads*head_dim must equal hidden");
    if (g_all < 0) throw Error("codec_stream_prime_batch: negative stream count");
    const int keep = std::max(c.cd_window - 1, 0), ctxB = codec_stage_b_context();
    // ---- every argument is checked before anything moves ----
    std::vector<int> live;
    int Fp = 0;
    for (int i = 0; i < g_all; ++i) {
        const StreamPush& q = ps[i];
        if (q.sid < 0 || q.sid >= (int)W.streams.size() || !W.streams[(size_t)q.sid].used) throw Error("codec_stream_prime_batch: no such stream");
        for (int k = 0; k < i; ++k) if (ps[k].sid == q.sid) throw Error("codec_stream_prime_batch: stream listed twice");
        const CodecW::Stream& S = W.streams[(size_t)q.sid];
        if (S.n_done != 0) throw Error("codec_stream_prime_batch: stream already has frames");
        if (q.n < 0) throw Error("codec_stream_prime_batch: negative frame count");
        if (q.n > S.cap) throw Error("codec_stream_prime_batch: more frames than the stream was opened for");
        if (q.n > 0 && !q.codes_dev) throw Error("codec_stream_prime_batch: null codes");
        // the tails land at the front of what codec_stream_begin allocated: they must fit it as it is
        if (q.n > 0 && (!S.kv || !S.hpost || std::min(q.n, keep) > S.P || std::min(q.n, ctxB) > S.h_cap)) throw Error("codec_stream_prime_batch: the stream's buffers do not hold the kept rows");
        if (q.n > 0) { live.push_back(i); Fp = std::max(Fp, q.n); }
    }
    const int g = (int)live.size();
    if (g == 0) return;
    if (g > 65535) throw Error("codec_stream_prime_batch: at most 65535 streams per call");
    if ((int64_t)g * Fp > (int64_t)1 << 24) throw Error("codec_stream_prime_batch: more than 2^24 padded rows in one call");
    int Ps = 1, pshift = 0;
    while (Ps < Fp) { Ps <<= 1; ++pshift; }
    codec_rope_tables(Ps);   // positions [0, Fp): the padded length
    std::vector<CodecStreamDesc>& D = W.sbatch_desc_h;
    D.assign((size_t)g, CodecStreamDesc());
    for (int i = 0; i < g; ++i) {
        const StreamPush& q = ps[live[(size_t)i]];
        const CodecW::Stream& S = W.streams[(size_t)q.sid];
        CodecStreamDesc& d = D[(size_t)i];
        d.kv = S.kv; d.hpost = S.hpost; d.codes = q.codes_dev; d.P = S.P; d.k0 = 0; d.h0 = 0; d.a0 = 0; d.n = q.n; d.row_off = i * Fp;
        d.ctx = std::min(q.n, ctxB); d.blk = i;
    }
    // ---- workspace ----
    const size_t rows = (size_t)g * Fp;
    const int T = (int)rows;
    const size_t need = codec_sbatch_prime_bytes(c, (size_t)g, (size_t)Fp, (size_t)Ps);
    if (W.sbatch_arena_bytes < need) regrow(W.sbatch_arena, W.sbatch_arena_bytes, need);
    if (W.sbatch_desc_n < (size_t)g) regrow(W.sbatch_desc, W.sbatch_desc_n, std::max((size_t)64, (size_t)g));
    codec_identity_pages(*this, g);   // one scratch cache block per stream
    Q3_HIP_CHECK(hipMemcpyAsync(W.sbatch_desc, D.data(), (size_t)g * sizeof(CodecStreamDesc), hipMemcpyHostToDevice, stream));
    CodecBump take{ W.sbatch_arena };
    float* h = take(rows * CH);
    float* hn = take(rows * CH);
    float* att = take(rows * CH);
    float* qkvb = take(rows * 3 * CH);
    float* ub = take(rows * FF);
    float* gb = take(rows * FF);
    float* kc = take((size_t)g * NH * Ps * HD);
    float* vc = take((size_t)g * NH * Ps * HD);
    const ConvLauncher conv{ W, take(CODEC_KSLAB_FLOATS), stream };
    Q3_HIP_CHECK(hipEventRecord(ev0, stream));
    const CodecStreamDesc* dd = W.sbatch_desc;
    Q3_HIP_CHECK(hipMemsetAsync(h, 0, rows * CH * sizeof(float), stream));   // padding rows: zeros through every layer
    launch_code_embed_mean_streams(W.code_embed, dd, g, Fp, c.n_groups, c.cd_codebook, CH, h, stream);
    pre_transformer_layers(c, W, T, PreBufs{ h, hn, att, qkvb, ub, gb }, conv, [&](int l) {
        launch_rope_store(qkvb, 3 * CH, Fp, NH, NH, HD, W.rope_cos, W.rope_sin, kc, vc, Ps, stream, g);
        launch_prime_kv_tails(kc, vc, Ps, dd, g, l, NH, HD, keep, stream);
        launch_attn(codec_attn_args(c, qkvb, att, kc, vc, W.batch_pages, pshift, 0, g, Fp), stream);
    }, stream);
    launch_rmsnorm_rows(h, W.norm, c.cd_rms_eps, T, CH, hn, stream);
    launch_prime_row_tails(hn, dd, g, CH, ctxB, stream);
    Q3_HIP_CHECK(hipEventRecord(ev1, stream));
    sync();
    Q3_HIP_CHECK(hipEventElapsedTime(&last_codec_ms, ev0, ev1));
    for (int i = 0; i < g; ++i) {   // the streams advance only now: a failure above leaves every one of them where it was
        const CodecStreamDesc& d = D[(size_t)i];
        CodecW::Stream& S = W.streams[(size_t)ps[live[(size_t)i]].sid];
        S.n_done = d.n; S.kv_rows = std::min(d.n, keep); S.h_rows = d.ctx;
    }
}

// host codes: stream s is primed with frames codes[frame_offsets[s] .. frame_offsets[s + 1]); validated as a whole before anything moves
void Engine::codec_stream_prime_batch_host(int n_streams, const int32_t* sids, const int64_t* codes, const int32_t* frame_offsets) {
    if (!codec) throw Error("codec decoder not finalized");
    if (n_streams < 0) throw Error("codec_stream_prime_batch: negative stream count");
    if (n_streams == 0) return;
    if (!sids || !frame_offsets) throw Error("codec_stream_prime_batch: null argument");
    CodecW& W = *codec;
    const int G = c.n_groups;
    if (frame_offsets[0] != 0) throw Error("codec_stream_prime_batch: frame_offsets must start at 0");
    for (int i = 0; i < n_streams; ++i)
        if (frame_offsets[i + 1] < frame_offsets[i]) throw Error("codec_stream_prime_batch: frame_offsets must not decrease");
    const size_t total = (size_t)frame_offsets[n_streams] * G;
    if (total > 0 && !codes) throw Error("codec_stream_prime_batch: null codes");
    std::vector<int32_t> tmp(total);
    stage_codes<Error>(codes, total, c.cd_codebook, tmp.data());
    std::vector<StreamPush> ps((size_t)n_streams);
    for (int i = 0; i < n_streams; ++i) {   // the checks codec_stream_prime_batch repeats, made here before the staging buffer may grow
        ps[(size_t)i].sid = sids[i]; ps[(size_t)i].n = frame_offsets[i + 1] - frame_offsets[i];
        if (sids[i] < 0 || sids[i] >= (int)W.streams.size() || !W.streams[(size_t)sids[i]].used) throw Error("codec_stream_prime_batch: no such stream");
        for (int k = 0; k < i; ++k) if (sids[k] == sids[i]) throw Error("codec_stream_prime_batch: stream listed twice");
        if (W.streams[(size_t)sids[i]].n_done != 0) throw Error("codec_stream_prime_batch: stream already has frames");
        if (ps[(size_t)i].n > W.streams[(size_t)sids[i]].cap) throw Error("codec_stream_prime_batch: more frames than the stream was opened for");
    }
    if (W.sbatch_codes_n < total) regrow(W.sbatch_codes, W.sbatch_codes_n, total);
    if (total > 0) Q3_HIP_CHECK(hipMemcpyAsync(W.sbatch_codes, tmp.data(), total * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    for (int i = 0; i < n_streams; ++i) ps[(size_t)i].codes_dev = W.sbatch_codes + (size_t)frame_offsets[i] * G;
    try { codec_stream_prime_batch(ps.data(), n_streams); } catch (...) { try { sync(); } catch (...) { } throw; }   // tmp must outlive the upload
    sync();
}

// The listed slots' implicit streams are restarted and primed with the slots' first n_frames[i] frames, read where the sampler (or the
// forced begin) wrote them: slots_codec_decode_new then starts at frame n_frames[i] with those frames as history.
void Engine::slots_codec_prime(int n_slots, const int32_t* slots, const int32_t* n_frames) {
    if (!codec) throw Error("codec decoder not finalized");
    if (n_slots < 0) throw Error("slots_codec_prime: negative slot count");
    if (n_slots == 0) return;
    if (!slots || !n_frames) throw Error("slots_codec_prime: null argument");
    CodecW& W = *codec;
    std::vector<SlotState> st;
    slots_state(B, st);
    for (int i = 0; i < n_slots; ++i) {
        if (slots[i] < 0 || slots[i] >= B) throw Error("slot out of range");
        for (int k = 0; k < i; ++k) if (slots[k] == slots[i]) throw Error("slots_codec_prime: slot listed twice");
        const SlotState& s = st[(size_t)slots[i]];
        const int have = s.active ? std::min(s.n_frames, max_frames_cap) : 0;
        if (n_frames[i] < 0 || n_frames[i] > have) throw Error("slots_codec_prime: slot " + std::to_string(slots[i]) + ": more frames than the slot holds");
    }
    if ((int)W.slot_stream.size() < B) W.slot_stream.assign((size_t)B, -1);
    std::vector<StreamPush> ps((size_t)n_slots);
    for (int i = 0; i < n_slots; ++i) {
        const int slot = slots[i];
        int sid = W.slot_stream[(size_t)slot];
        if (sid >= 0 && W.streams[(size_t)sid].used) codec_stream_end(sid);
        sid = codec_stream_begin(max_frames_cap);
        W.slot_stream[(size_t)slot] = sid;
        ps[(size_t)i].sid = sid; ps[(size_t)i].n = n_frames[i];
        ps[(size_t)i].codes_dev = codes_d + (size_t)slot * max_frames_cap * c.n_groups;
    }
    codec_stream_prime_batch(ps.data(), n_slots);
}

void Engine::codec_stream_info(int sid, int* n_done, int* kv_capacity_rows, int64_t* bytes) const {
    if (!codec || sid < 0 || sid >= (int)codec->streams.size() || !codec->streams[(size_t)sid].used) throw Error("codec_stream: no such stream");
    const CodecW::Stream& S = codec->streams[(size_t)sid];
    if (n_done) *n_done = S.n_done;
    if (kv_capacity_rows) *kv_capacity_rows = S.P;
    if (bytes) *bytes = (int64_t)((size_t)c.cd_layers * 2 * c.cd_heads * S.P * c.cd_head_dim * sizeof(float) + (size_t)S.h_cap * c.cd_hidden * sizeof(float));
}

// the implicit stream behind q3tts_slot_codec_decode_range_host: consecutive exact ranges of a slot ([0, b1), [b1, b2), ...) are pushes
int64_t Engine::slot_codec_stream_range(int slot, int a, int b, float* pcm, int64_t cap) {
    CodecW& W = *codec;
    if ((int)W.slot_stream.size() < B) W.slot_stream.assign((size_t)B, -1);
    int sid = W.slot_stream[(size_t)slot];
    if (sid < 0 || !W.streams[(size_t)sid].used || W.streams[(size_t)sid].n_done > a) {   // first range of the utterance, or a restart
        if (sid >= 0 && W.streams[(size_t)sid].used) codec_stream_end(sid);
        sid = codec_stream_begin(max_frames_cap);
        W.slot_stream[(size_t)slot] = sid;
    }
    const int32_t* codes = codes_d + (size_t)slot * max_frames_cap * c.n_groups;
    CodecW::Stream& S = W.streams[(size_t)sid];
    if (S.n_done < a) codec_stream_push_dev(sid, codes + (size_t)S.n_done * c.n_groups, a - S.n_done, nullptr);   // frames nobody asked the audio of
    float* pcm_d = nullptr;
    CodecTimed t(*this);
    const int64_t n_own = codec_stream_push_dev(sid, codes + (size_t)a * c.n_groups, b - a, &pcm_d);
    t.stop();
    return t.deliver(pcm_d, n_own, pcm, cap, b - a);
}
void Engine::slot_codec_stream_reset(int slot) {
    if (!codec) return;
    CodecW& W = *codec;
    if (slot < 0 || slot >= (int)W.slot_stream.size()) return;
    const int sid = W.slot_stream[(size_t)slot];
    if (sid >= 0 && W.streams[(size_t)sid].used) codec_stream_end(sid);
    W.slot_stream[(size_t)slot] = -1;
}

// Test hook (Q3TTS_FLAG_TEST_HOOKS engines): every byte of the vocoder's reusable workspace — lane arenas, the batched front's arena,
// the streaming arena, the pinned PCM staging buffers, the job's code rows — becomes 0xFF (NaN as fp32 and as fp16), so a decode that
// reads anything it did not write in the same call shows up as NaN instead of as yesterday's plausible samples.
void Engine::codec_poison() {
    if (!(flags & Q3TTS_FLAG_TEST_HOOKS)) throw Error("codec_poison needs Q3TTS_FLAG_TEST_HOOKS");
    if (!codec) return;
    CodecW& W = *codec;
    for (int i = 0; i < W.nlane; ++i) Q3_HIP_CHECK(hipStreamSynchronize(W.lane_stream[i]));
    W.dbg_sx = W.dbg_pcm = nullptr;   // the last batched group's rows are gone with everything else
    for (int i = 0; i < CodecW::NLANE; ++i) {
        if (W.arena[i]) Q3_HIP_CHECK(hipMemset(W.arena[i], 0xFF, W.arena_bytes[i]));
        if (W.pinned[i]) memset(W.pinned[i], 0xFF, W.pinned_floats[i] * sizeof(float));
    }
    if (W.batch_arena) Q3_HIP_CHECK(hipMemset(W.batch_arena, 0xFF, W.batch_arena_bytes));
    if (W.stream_arena) Q3_HIP_CHECK(hipMemset(W.stream_arena, 0xFF, W.stream_arena_bytes));
    if (W.sbatch_arena) Q3_HIP_CHECK(hipMemset(W.sbatch_arena, 0xFF, W.sbatch_arena_bytes));
    if (W.sbatch_desc) Q3_HIP_CHECK(hipMemset(W.sbatch_desc, 0xFF, W.sbatch_desc_n * sizeof(CodecStreamDesc)));   // uploaded anew by every push
    if (W.sbatch_codes) Q3_HIP_CHECK(hipMemset(W.sbatch_codes, 0xFF, W.sbatch_codes_n * sizeof(int32_t)));
    if (W.job_codes) Q3_HIP_CHECK(hipMemset(W.job_codes, 0xFF, W.job_codes_n * sizeof(int32_t)));   // -1: clamped to code 0 by the gather, never out of the table
    Q3_HIP_CHECK(hipDeviceSynchronize());
}

// Test hook: input rows [nb][T][C] and output [nb][T] of the last batched group's final conv, as they lie in the lane's arena now
void Engine::codec_debug_group(float* sx_out, float* pcm_out, int64_t cap_floats, int* T, int* C, int* nb) {
    if (!(flags & Q3TTS_FLAG_TEST_HOOKS)) throw Error("codec_debug_group needs Q3TTS_FLAG_TEST_HOOKS");
    CodecW& W = *codec;
    *T = W.dbg_T; *C = W.dbg_C; *nb = W.dbg_nb;
    if (!W.dbg_sx || !W.dbg_pcm) throw Error("codec_debug_group: no batched group's rows to read (none has run, or its lane's workspace was regrown or poisoned since)");
    Q3_HIP_CHECK(hipDeviceSynchronize());
    const int64_t n = (int64_t)W.dbg_nb * W.dbg_T * W.dbg_C;
    if (sx_out && n <= cap_floats) Q3_HIP_CHECK(hipMemcpy(sx_out, W.dbg_sx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (pcm_out) Q3_HIP_CHECK(hipMemcpy(pcm_out, W.dbg_pcm, (size_t)W.dbg_nb * W.dbg_T * sizeof(float), hipMemcpyDeviceToHost));
}
int64_t Engine::codec_debug_partials(float* out, int64_t cap_floats) {
    const float* p = nullptr; size_t n = 0;
    cout1_debug_buffer(&p, &n);
    if (out && p && (int64_t)n <= cap_floats) { Q3_HIP_CHECK(hipDeviceSynchronize()); Q3_HIP_CHECK(hipMemcpy(out, p, n * sizeof(float), hipMemcpyDeviceToHost)); }
    return (int64_t)n;
}

bool Engine::codec_batchable() const {
    if (!codec || codec->planes.empty()) return false;                     // exact-fp32 codec: no split-precision planes
    const int D = c.cd_decoder_dim, OD = D >> c.cd_n_blocks;
    if (c.cd_hidden % 32 || OD % 32 || OD < 32) return false;             // every channel count of the decoder is then a multiple of 32
    if ((size_t)(128 + 6) * (OD + 1) * sizeof(float) > 60 * 1024) return false;   // last conv (C_out = 1) in LDS
    for (int i = 0; i < c.cd_n_blocks; ++i) if (c.cd_up_rates[i] < 1) return false;
    return true;
}

// The conv decoder of g consecutive utterances of codec_pre_batch's output in ONE set of launches (rows [utterance][Tp] in every layer; the
// kernels' row tiles never straddle utterances, and causality keeps the padding out of the real samples): h_group = the group's upsampled
// rows (h_ustride floats apart), Fg = frames of the group's longest utterance.  Each utterance's sample count comes from its own frame count.
void Engine::codec_async_submit_group(const float* h_group, size_t h_ustride, int Fg, int g, const int* nf, float* const* user_pcm, int64_t cap, int64_t* const* len_out) {
    CodecW& W = *codec;
    // a group's launches fill the chip on their own: two lanes are enough to overlap one group's tail with the next one's start (and each
    // lane owns a group-sized arena)
    const int lane = W.nlane > 1 ? 1 + (W.rr++ % std::min(W.nlane - 1, 2)) : 0;
    codec_async_drain_lane(lane);
    if (W.fail_at_submit > 0 && ++W.submits == W.fail_at_submit) throw Error("vocoder submit failed (injected by Q3TTS_TEST_FAIL_VOCODER_SUBMIT)");
    if (!W.window_open) {
        if (!W.win0_recorded) { Q3_HIP_CHECK(hipEventRecord(W.win0, stream)); W.win0_recorded = true; }
        Q3_HIP_CHECK(hipEventRecord(W.fork, stream));
        for (int i = 1; i < W.nlane; ++i) Q3_HIP_CHECK(hipStreamWaitEvent(W.lane_stream[i], W.fork, 0));
        W.window_open = true;
    }
    if (!W.lane_done[lane]) Q3_HIP_CHECK(hipEventCreateWithFlags(&W.lane_done[lane], hipEventDisableTiming));
    hipStream_t ls = W.lane_stream[lane];
    if (lane != 0) {   // this group's rows come from the batched pass just queued on the engine stream (a later block than the window's first)
        Q3_HIP_CHECK(hipEventRecord(W.fork, stream));
        Q3_HIP_CHECK(hipStreamWaitEvent(ls, W.fork, 0));
    }
    float* pcm_d = nullptr;
    const int64_t Tp = codec_run(nullptr, Fg, &pcm_d, lane, h_group, 2, g, h_ustride);   // padded samples per utterance (Fg = the group's longest)
    CodecW::Pending& p = W.pend[lane];
    p.items.clear();
    int64_t total = 0;
    int frames = 0;
    for (int u = 0; u < g; ++u) {
        const int64_t n = codec_len_of(c, nf[u]);
        p.items.push_back(CodecW::Item{ user_pcm ? user_pcm[u] : nullptr, n, cap, total, len_out ? len_out[u] : nullptr });
        total += std::min(n, cap);
        frames += std::max(nf[u], 0);
    }
    if ((size_t)total > W.pinned_floats[lane]) regrow_pinned(W.pinned[lane], W.pinned_floats[lane], (size_t)total);
    for (int u = 0; u < g; ++u) {
        const CodecW::Item& it = p.items[(size_t)u];
        const int64_t m = std::min(it.n, it.cap);
        if (m > 0) Q3_HIP_CHECK(hipMemcpyAsync(W.pinned[lane] + it.off, pcm_d + (size_t)u * Tp, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, ls));
    }
    Q3_HIP_CHECK(hipEventRecord(W.lane_done[lane], ls));
    p.frames = frames; p.busy = true;
}

// the engine stream waits for every lane's queued work (no host synchronisation): what it launches next may overwrite what the lanes read
void Engine::codec_lanes_join() {
    if (!codec) return;
    CodecW& W = *codec;
    for (int i = 1; i < W.nlane; ++i)
        if (W.pend[i].busy && W.lane_done[i]) Q3_HIP_CHECK(hipStreamWaitEvent(stream, W.lane_done[i], 0));
}

void Engine::codec_async_drain() {
    if (!codec) return;
    CodecW& W = *codec;
    if (!W.window_open) return;
    for (int i = 0; i < W.nlane; ++i)
        if (W.pend[i].busy && i != 0) Q3_HIP_CHECK(hipStreamWaitEvent(stream, W.lane_done[i], 0));
    Q3_HIP_CHECK(hipEventRecord(W.win1, stream));
    for (int i = 0; i < W.nlane; ++i) codec_async_drain_lane(i);
    sync();
    float ms = 0.f;
    Q3_HIP_CHECK(hipEventElapsedTime(&ms, W.win0, W.win1));
    total_codec_ms += ms; last_codec_ms = ms;
    W.window_open = false; W.win0_recorded = false;
}

} // namespace q3
