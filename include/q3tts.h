/*
 * q3tts.h — C-ABI of libq3tts_hip.so: the MI355X (gfx950) replacement for the seven ONNX Runtime
 * sessions of leaxer-ai/leaxer-qwen3-tts.
 *
 * The reference has no plugin/FFI layer; its narrowest seam is the private run_* family of
 * TTSEngine (reference src/tts_onnx.h:196-212, src/tts_onnx.cpp:545-776), each a named-tensor
 * ONNX Runtime Session::Run over host vectors.  Every entry point below cites the run_* call it
 * replaces.  Conventions: int return (0 ok, <0 error; message via q3tts_last_error), no exceptions
 * cross the ABI, plain pointers and sizes only.  "_host" entry points take HOST pointers exactly
 * like the reference's run_* (inputs caller-owned, outputs copied out); the batched generation
 * entry points keep everything (KV cache, logits, codes) resident in HBM.  A handle is not
 * thread-safe: one in-flight call per handle, like one TTSEngine (tts_onnx.h:182-186).
 */
#ifndef Q3TTS_H
#define Q3TTS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Model dimensions.  The reference hard-codes the 0.6B talker dims (tts_onnx.h:31-37); the rest
 * are properties of the opaque graphs ([HINT]).  Runtime-configurable so the
 * same library serves the 1.7B export and the tiny test configs. */
typedef struct q3tts_config {
    int32_t hidden, n_layers, n_heads, n_kv_heads, head_dim, ffn, vocab;
    float rope_theta, rms_eps;
    int32_t cp_layers, cp_heads, cp_kv_heads, cp_head_dim, cp_ffn, n_groups, sub_vocab;
    float cp_rope_theta, cp_rms_eps;
    int32_t text_vocab, text_hidden;
    int32_t cd_codebook, cd_hidden, cd_layers, cd_heads, cd_head_dim, cd_ffn, cd_window;
    float cd_rope_theta, cd_rms_eps;
    int32_t cd_n_up;
    int32_t cd_up_ratios[4];
    int32_t cd_decoder_dim;
    int32_t cd_n_blocks;
    int32_t cd_up_rates[8];
    int32_t cd_tconv_trim; /* 0: trim k-s on both sides, 1: right side only */
    int32_t codec_eos, suppress_begin, suppress_end; /* tts_onnx.h:51, tts_onnx.cpp:803-807 */
    /* speaker encoder of the clone path (speaker_encoder.onnx, tts_onnx.cpp:367-403): ECAPA-TDNN, channel plan
     * (C, C, C, C, 3C), kernels (5,3,3,3,1), dilations (1,2,3,4,1).  spk_enc_dim == 0: no speaker encoder
     * (has_speaker_encoder() false, as when the reference finds no speaker_encoder.onnx). */
    int32_t spk_enc_dim, spk_mel, spk_channels, spk_scale, spk_se, spk_att;
    /* width of the code predictor's layers; 0 (or == hidden): the talker's width, as in the 0.6B export.  Otherwise (1.7B: hidden 2048,
     * cp_hidden 1024) every predictor input row passes through cp.proj (Linear + bias, [HINT] Qwen3-TTS small_to_mtp_projection) first;
     * the predictor's code embeddings stay talker-wide.  The code_predictor session contract (tts_onnx.cpp:734-757) is unchanged. */
    int32_t cp_hidden;
    /* audio encoder of the 12 Hz speech tokenizer (audio -> codes; [HINT] transformers MimiModel.encode, the first n_groups quantizers):
     * SEANet encoder (causal convs: enc_kernel taps 1 -> enc_filters; per ratio a residual block of enc_res_kernel and 1 taps, then a
     * conv of 2 x ratio taps, stride ratio, doubling the channels; enc_last_kernel taps -> enc_hidden), a transformer of enc_layers
     * layers at that rate (LayerNorm, RoPE, causal window enc_window, LayerScale, GELU MLP), a stride-2 conv of 4 taps with replicate
     * padding, and a split residual VQ (1 semantic + n_groups - 1 acoustic levels of enc_codebook rows x enc_vq_dim).  enc_ratios is in
     * encoder order (first stage first).  enc_hidden == 0: no audio encoder (q3tts_has_audio_encoder() false, no enc.* tensor). */
    int32_t enc_hidden, enc_filters, enc_n_ratios;
    int32_t enc_ratios[4];
    int32_t enc_kernel, enc_res_kernel, enc_last_kernel;
    int32_t enc_layers, enc_heads, enc_head_dim, enc_ffn, enc_window;
    int32_t enc_vq_dim, enc_codebook;
    float enc_rope_theta, enc_norm_eps;
} q3tts_config;

/* SamplingParams, reference src/tts_onnx.h:99-105.  The reference declares repetition_penalty and never reads it; here it is the
 * standard logits processor (transformers RepetitionPenaltyLogitsProcessor) on the FIRST codebook: for every code0 id the utterance
 * has emitted so far (frames 0 .. n-1 of this utterance; the prompt contributes nothing, an id seen many times counts once) the raw
 * fp32 logit becomes x > 0 ? x / p : x * p — before the special-token suppression, temperature, top-k and top-p.  The 15 sub-codes
 * (other codebooks, a separate predictor) are not penalised.  1.0 and 0.0 (a zero-initialised struct) switch it off: the output is
 * then bit-identical to an engine without the field.  0 < p < 1 rewards repeats.  A negative or non-finite value is refused by every
 * entry point that starts a generation or samples with a history ("repetition_penalty must be positive").  It applies in the fused
 * generation (q3tts_slot_begin + q3tts_decode_steps, q3tts_synthesize_*) and in q3tts_sample_hist_*; q3tts_sample_host / _dev and
 * q3tts_code_predictor_dev have no code0 history and ignore it. */
typedef struct q3tts_sampling {
    float temperature, top_p;
    int32_t top_k;
    float repetition_penalty;
    int32_t max_new_tokens;
} q3tts_sampling;

typedef struct q3tts_engine q3tts_engine;

/* flags for q3tts_create */
#define Q3TTS_FLAG_NO_GRAPH 1u   /* launch the decode step eagerly instead of replaying a hipGraph */
#define Q3TTS_FLAG_NO_FUSED_CP 2u /* b = 1: keep code-predictor attention and o_proj as separate launches (A/B testing) */
#define Q3TTS_FLAG_KV_BF16 8u     /* talker KV cache in bf16: K / V rows rounded to bf16 (round-to-nearest-even) where they enter the cache, fp32 attention
                                   * math on the rounded rows — half the cache bytes of the default fp32 cache (which mirrors the reference's fp32
                                   * KVCache, src/tts_onnx.h:108-115).  The CPU oracle has the same switch; rounding being a discontinuity, two implementations
                                   * agree to ~4e-3 on logits in this mode (2e-5 with fp32 caches), ids to the first sub-noise decision. */
#define Q3TTS_FLAG_KV_ROUND_BF16 16u /* test aid: fp32 KV storage holding the bf16-ROUNDED rows — the arithmetic of Q3TTS_FLAG_KV_BF16 without its 16-bit storage;
                                     * the two modes must agree bit for bit (tests/test_gpu_full.py), which pins the bf16 load / store / convert path */
#define Q3TTS_FLAG_TEST_HOOKS 32u  /* honour the fault-injection environment hooks of the test suite (Q3TTS_TEST_FAIL_VOCODER_SUBMIT); without it they are ignored */
#define Q3TTS_FLAG_RAGGED_PREFILL 64u /* scheduler: the utterances of an admission look that are begun on their own today (instructed, continued,
                                       * behind a shared prefix with more than 16 rows of their own) are begun with ONE q3tts_slots_begin_ragged call.
                                       * Opt-in: without it every entry point keeps its launches and its bits */
#define Q3TTS_FLAG_FP32_CODEC 4u  /* codec decoder on the exact-fp32 matrix-core path instead of the fp16 (hi, lo) split-operand path */

/* ---- lifecycle (replaces TTSEngine ctor / load_model, tts_onnx.cpp:84-232) ---- */
int q3tts_default_config(const char* name /* "0.6b" | "1.7b" */, q3tts_config* out);
/* q3tts_default_config leaves the audio encoder off; this fills in the 12 Hz tokenizer's encoder dimensions ([HINT], unpinned: the Mimi
 * encoder of transformers — 64 filters, ratios 4 5 6 8, hidden 512, 8 layers of 8 x 64 heads, ffn 2048, window 250, 2048 x 256
 * codebooks).  The other fields are left as they are.  0 on success, -1 for a NULL pointer. */
int q3tts_config_enable_audio_encoder(q3tts_config* cfg);
q3tts_engine* q3tts_create(const q3tts_config* cfg, int device, int max_batch, int max_ctx, uint32_t flags);
/* The same with a bounded KV page pool.  The talker's cache (the reference's KVCache, tts_onnx.h:108-115, grown by one token per run_decode)
 * is a pool of 64-token pages; a slot takes pages for prompt + max_new_tokens when it is armed (q3tts_slot_begin / the scheduler) or as its
 * context grows (q3tts_talker_prefill_host / q3tts_talker_decode_host) and returns them at q3tts_slot_release.  kv_pool_tokens = 0 sizes the
 * pool for max_batch x max_ctx (q3tts_create); a smaller pool admits as many utterances as fit — q3tts_slot_begin fails with "KV page pool
 * exhausted" and arms nothing; the scheduler (q3tts_synthesize_*) keeps the rest queued.  There, with ignore_eos (lengths known) an
 * utterance is admitted when prompt + cap fit; otherwise slots grow page by page as they generate, so utterances that stop early never
 * hold the pages of their cap, and when the pool runs dry the youngest running utterance is preempted and generated again later. */
q3tts_engine* q3tts_create_pooled(const q3tts_config* cfg, int device, int max_batch, int max_ctx, int64_t kv_pool_tokens, uint32_t flags);
int q3tts_kv_pool_info(q3tts_engine* e, int* page_tokens, int* total_pages, int* free_pages);
/* One set of weights for several engines on a GPU (the reference loads its sessions once per TTSEngine, tts_onnx.cpp:91-107; a server
 * with one handle per worker thread would otherwise hold one copy per handle).  A new engine on the donor's GPU with the donor's config,
 * holding the donor's finalized weights (registry and everything finalize derives from it: packed copies, codec planes, repacked
 * convs, codebooks, the layer-0 QKV table) instead of a copy.  Slots, KV pool, workspaces, streams, graphs, codec / encoder streams
 * and stages are its own; it is ready at once (no q3tts_finalize).  The KV flags, NO_GRAPH, NO_FUSED_CP, RAGGED_PREFILL and TEST_HOOKS
 * may differ from the donor's; Q3TTS_FLAG_FP32_CODEC must not (it selects a different derived layout).  May be called while the donor
 * generates on another thread: neither the donor's stream nor its workspaces are touched.  NULL, with q3tts_last_error(NULL), when the
 * donor is NULL or not finalized, when that flag differs, or on any argument q3tts_create_pooled refuses.
 * While more than one engine holds a set, q3tts_set_tensor_host, q3tts_fill_synthetic and q3tts_load_weights_file fail on every holder
 * ("weights are shared by N engines") and q3tts_finalize returns 0 and does nothing; the read-only calls work on every holder.  Holders
 * may be destroyed in any order, also while another one generates; the last q3tts_destroy frees the weights. */
q3tts_engine* q3tts_create_sharing(q3tts_engine* donor, int max_batch, int max_ctx, int64_t kv_pool_tokens, uint32_t flags);
/* bytes of HBM the engine's weight set holds (registry + derived copies), how many engines hold that set, and how many bytes of weights
 * or derived weight copies this engine owns outside the shared set (0 when everything applicable is shared).  Any pointer may be NULL. */
int q3tts_weights_info(q3tts_engine* e, int64_t* shared_bytes, int* holders, int64_t* private_weight_bytes);
/* The last q3tts_synthesize_* call on this engine: utterances admitted to a slot (re-admissions count), utterances preempted because the
 * pool ran dry (each is generated again from its prompt: same RNG stream, same codes), most utterances running at once. */
int q3tts_sched_stats(q3tts_engine* e, int64_t* admitted, int64_t* preempted, int* peak_live);
void q3tts_destroy(q3tts_engine* e);
const char* q3tts_last_error(q3tts_engine* e); /* e may be NULL: error of the last failed create */

/* ---- weights: tensors by name (names = the oracle's / DESIGN.md section 3) ---- */
/* The registry a config implies, without an engine (host-only, no GPU needed): what a checkpoint converter must provide.
 * kind: 0 matrix / conv weight, 1 norm weight, 2 bias, 3 LayerScale / gamma, 4 SnakeBeta alpha / beta. */
int q3tts_config_num_tensors(const q3tts_config* cfg);
int q3tts_config_tensor_info(const q3tts_config* cfg, int index, char* name, int name_cap, int64_t* shape4, int* ndim, int* kind);
int q3tts_num_tensors(q3tts_engine* e);
int q3tts_tensor_info(q3tts_engine* e, int index, char* name, int name_cap, int64_t* shape4, int* ndim);
int q3tts_set_tensor_host(q3tts_engine* e, const char* name, const float* data, int64_t numel);
int q3tts_get_tensor_host(q3tts_engine* e, const char* name, float* out, int64_t numel);
/* seeded on-device synthetic weights (integer hash -> Irwin-Hall normal, bf16-representable) */
int q3tts_fill_synthetic(q3tts_engine* e, uint64_t seed);
/* call after the last set_tensor / fill: builds RoPE tables, packed conv weights, tts_pad row */
int q3tts_finalize(q3tts_engine* e);

/* Weight files ("Q3TW0001": config + named tensors, fp32 or bf16 payloads; written by
 * q3tts_save_weights_file or tools/pack_weights.py).  This is what TTSEngine(model_dir) loads in
 * place of the reference's seven .onnx files (tts_onnx.cpp:91-107). */
int q3tts_read_weights_config(const char* path, q3tts_config* out);
int q3tts_load_weights_file(q3tts_engine* e, const char* path);   /* set_tensor for every entry + finalize */
int q3tts_save_weights_file(q3tts_engine* e, const char* path);

/* ---- session-shaped entry points, host I/O, one per reference run_* ---- */
/* The talker input row of a finished frame, tts_onnx.cpp:824-842: codes[n][n_groups] -> out[n][hidden], row i = codec_embed[code0] +
 * cp_embed[0][sub0] + ... + cp_embed[n_groups-2][sub_last], accumulated in fp32 in that order, + the text row of frame frame0 + i:
 * trailing[frame0 + i] when that index is < n_trailing, else the tts_pad row.  This is exactly what the fused generation loop feeds the
 * talker after sampling that frame (bit for bit: the result is determined by the order of the adds), made by one launch on the device
 * instead of 16 embedding round trips per frame.  code0 in [0, vocab), sub-codes in [0, sub_vocab); n <= max_ctx per call. */
int q3tts_frame_rows_host(q3tts_engine* e, const int64_t* codes, int n, int frame0, const float* trailing, int n_trailing, float* out);
/* run_text_project, tts_onnx.cpp:545-559: ids[n] -> out[n][hidden] */
int q3tts_text_project_host(q3tts_engine* e, const int64_t* ids, int n, float* out);
/* run_codec_embed / run_codec_embed_batch, tts_onnx.cpp:561-590 */
int q3tts_codec_embed_host(q3tts_engine* e, const int64_t* ids, int n, float* out);
/* run_code_predictor_embed, tts_onnx.cpp:592-613 */
int q3tts_cp_embed_host(q3tts_engine* e, int64_t id, int generation_step, float* out);
/* run_prefill, tts_onnx.cpp:615-665: embeds[S][hidden] -> logits[S][vocab], last_hidden[hidden]; 1 <= S <= max_ctx; either output
 * may be NULL.  The KV cache of `slot` is reset and stays device-resident (replaces KVCache, tts_onnx.h:108-115).  Up to 16 rows (the
 * reference's own prompt is 8-10) take one pass; a longer prompt — an instruction or any other prefix in front of it — is walked in
 * chunks of up to 128 rows, each attending causally over what the chunks before it left in the cache.  `logits`, when given, still
 * receives all S rows; with logits == NULL the codec head runs on the last row only. */
int q3tts_talker_prefill_host(q3tts_engine* e, int slot, const float* embeds, int S, float* logits, float* last_hidden);
/* run_decode, tts_onnx.cpp:667-732: one token appended to `slot` */
int q3tts_talker_decode_host(q3tts_engine* e, int slot, const float* embed, float* logits, float* last_hidden);
/* run_code_predictor, tts_onnx.cpp:734-757: seq[n][hidden], head #generation_step on the last row */
int q3tts_code_predictor_host(q3tts_engine* e, const float* seq, int n, int generation_step, float* logits);
/* run_vocoder, tts_onnx.cpp:759-776: codes[F][n_groups] (frame-major) -> pcm; *out_len = lengths[0].
 * One call decodes at most ~5500 frames (7 minutes: a decoder activation must stay below 4 GB, the conv kernels address it with 32-bit
 * offsets); longer utterances go through q3tts_codec_decode_chunked_host. */
int q3tts_codec_decode_host(q3tts_engine* e, const int64_t* codes, int F, float* pcm, int64_t cap, int64_t* out_len);
int64_t q3tts_codec_decode_len(const q3tts_config* cfg, int F);
/* run_vocoder for a whole job in one call (the reference calls run_vocoder once per utterance, tts_onnx.cpp:418-432 / :759-776; this is the
 * vocoder phase of q3tts_synthesize_schedule_host on its own): utterance u's codes are codes[frame_offsets[u] .. frame_offsets[u+1])
 * frames of n_groups ids each.  Utterances of similar length share one batched pass, the rest go one at a time over the side lanes;
 * pcm_out[u] receives up to pcm_cap samples, pcm_len[u] the utterance's sample count (q3tts_codec_decode_len of its frames; 0 for an
 * utterance without frames).  Each result equals q3tts_codec_decode_host of the same utterance to fp32 rounding; ids outside
 * [0, codebook) and utterances beyond the engine's frame capacity are rejected like there. */
int q3tts_codec_decode_batch_host(q3tts_engine* e, int n_utt, const int64_t* codes, const int32_t* frame_offsets, float* const* pcm_out,
                                  int64_t pcm_cap, int64_t* pcm_len);
/* the same with both ends in HBM: codes_dev int32 [F][n_groups] and pcm_dev float [cap] are DEVICE pointers on the engine's GPU (any
 * allocator: hipMalloc, a torch tensor's data_ptr); values outside [0, codebook) are clamped.  Returns after the work has completed. */
int q3tts_codec_decode_dev(q3tts_engine* e, const int32_t* codes_dev, int F, float* pcm_dev, int64_t cap, int64_t* out_len);
/* the engine's HIP stream as an opaque pointer (hipStream_t): every launch of this handle is ordered on it, so a host application can
 * record events on / wait for it instead of relying on the blocking entry points */
void* q3tts_stream(q3tts_engine* e);
/* Streaming / chunked decode (the reference decodes the whole utterance in one run_vocoder call, tts_onnx.cpp:430).
 * The decoder is causal: frames [a, b) own the samples [L(a), L(b)) of the full decode (L = q3tts_codec_decode_len, L(0) = 0), and
 * they are final as soon as frame b-1 exists.  With left_context >= a (exact mode) the call runs on a carried-state stream (below):
 * O(b - a) work, and the concatenation over chunks equals the whole-utterance decode.  A smaller left_context decodes the window
 * [a - left_context, b) instead and returns those samples: bounded memory of the past at the price of a truncated history (the
 * pre-transformer looks back 72 frames per layer, 568 in all). */
int q3tts_codec_decode_chunked_host(q3tts_engine* e, const int64_t* codes, int F, int chunk_frames, int left_context, float* pcm, int64_t cap,
                                    int64_t* out_len);
/* Streaming decode with CARRIED state (round 4): a stream keeps the pre-transformer's K / V rows of every layer and its output rows, so a
 * push of n new frames costs O(n + a few frames of conv look-back) instead of a decode of the history.  The concatenation of the pushes
 * equals q3tts_codec_decode_host of all the frames to fp32 rounding (<= 2e-5 asserted in tests/test_gpu_codec.py, ~1e-6 measured): the
 * arithmetic is the same, but a short push picks other GEMM tile shapes / split-K and, under 128 rows, k_attn instead of k_attn_win, so
 * sums associate differently.  max_frames bounds the stream's length (and sizes the shared RoPE tables), NOT its memory: the state is a
 * sliding buffer of the last window - 1 = 71 K / V rows per layer and the last 12 output rows plus room for the largest push so far
 * (round 5; 16.8 MB of K / V + 0.4 MB of rows per stream at 0.6B dims for pushes of up to 114 frames, whatever max_frames is; a larger push
 * grows it once).  A stream's buffers are kept when it ends and reused by the next stream; they are freed with the engine.
 * q3tts_codec_decode_chunked_host with left_context >= F and q3tts_slot_codec_decode_range_host with left_context >= frame_begin run on
 * such a stream by themselves (one per slot, created at the slot's first exact range). */
int q3tts_codec_stream_begin(q3tts_engine* e, int max_frames, int* stream_id);
/* codes[n_frames][n_groups] of the NEXT n_frames frames of the stream -> the samples those frames own (*out_len of them) */
int q3tts_codec_stream_push_host(q3tts_engine* e, int stream_id, const int64_t* codes, int n_frames, float* pcm, int64_t cap, int64_t* out_len);
int q3tts_codec_stream_end(q3tts_engine* e, int stream_id);
/* the same for frames of a slot that is still generating: call after q3tts_decode_steps has produced frame_end frames.  Behind
 * q3tts_slot_begin_codes the slot's frames start with the prefix: (slot, n_prefix, n_frames, left_context >= n_prefix) returns the new
 * frames' samples with the prefix as history — the audio that joins what the prefix's own decode ended with, without a seam. */
int q3tts_slot_codec_decode_range_host(q3tts_engine* e, int slot, int frame_begin, int frame_end, int left_context, float* pcm, int64_t cap,
                                       int64_t* out_len);
/* run_vocoder (tts_onnx.cpp:759-776) for the NEXT frames of many carried-state streams at once — the reference decodes one whole
 * utterance per call.  Stream stream_ids[s] receives frames codes[frame_offsets[s] .. frame_offsets[s+1]) (n_groups ids each) and
 * pcm_out[s] the samples they own (up to pcm_cap; pcm_len[s] their count).  All streams' new rows go through the pre-transformer in ONE
 * set of launches per layer (each at its own position, over its own sliding K / V buffer), their windows through the conv decoder as one
 * batch per left-context length: the launch count does not depend on n_streams.  Every result equals the single pushes' to fp32 rounding.
 * A stream without frames is left untouched (pcm_len[s] = 0).  Everything is validated before any stream advances — ids distinct and
 * open, offsets non-decreasing from 0, codes inside the codebook, no stream beyond its max_frames: on error no stream has moved. */
int q3tts_codec_stream_push_batch_host(q3tts_engine* e, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets,
                                       float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len);
/* run_vocoder (tts_onnx.cpp:759-776) over what the listed slots have generated since their previous streaming call, in batched passes:
 * slot slots[i] gets the samples of its frames [frame_begin[i], frame_end[i]) (frame_end = the slot's frame count now; an empty range
 * gives pcm_len[i] = 0).  Runs on the slot's implicit stream — the one q3tts_slot_codec_decode_range_host uses in exact mode, so the two
 * may alternate on a slot — and reads the codes where the sampler left them: they never leave HBM.  Slots must be distinct. */
int q3tts_slots_codec_decode_new_host(q3tts_engine* e, int n_slots, const int32_t* slots, float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len,
                                      int32_t* frame_begin, int32_t* frame_end);
/* run_vocoder (tts_onnx.cpp:759-776) carries no state; a carried-state stream that continues behind frames whose audio nobody wants
 * needs their state, not their samples.  PRIMING puts g open streams that hold no frames yet into the state a push of their first
 * n_s = frame_offsets[s + 1] - frame_offsets[s] frames (codes as in the batched push) would leave: the pre-transformer alone runs over
 * all streams' rows in one set of launches per layer (padded [stream][longest] rows, scratch K / V), and two copy kernels move the
 * tails a stream keeps — the last min(n_s, window - 1) rotated K / V rows of every layer, the last min(n_s, look-back) output rows —
 * to the front of the stream's own buffers.  The conv decoder and the upsampling stages do not run, no sample is produced, and the
 * stream's buffers stay as q3tts_codec_stream_begin sized them whatever n_s is.  The next push continues at frame n_s and equals the
 * push behind a pushed history to fp32 rounding (the bound of the pushes themselves).  n_s == 0 leaves a stream untouched.  Everything
 * is validated before anything moves — ids distinct and open, "stream already has frames", offsets non-decreasing from 0, codes inside
 * the codebook, no n_s beyond the stream's max_frames.  q3tts_last_codec_ms reports the call's device time. */
int q3tts_codec_stream_prime_batch_host(q3tts_engine* e, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets);
/* run_vocoder (tts_onnx.cpp:759-776) would decode these frames again with every call; here the slots' implicit streams (the ones
 * q3tts_slots_codec_decode_new_host uses) are restarted and primed with the slots' first n_frames[i] frames, read from the slots' code
 * buffers in HBM; the next q3tts_slots_codec_decode_new_host call starts at frame n_frames[i].  n_frames[i] <= the slot's frame count;
 * slots distinct.  For a slot begun behind a prefix (q3tts_slot_begin_codes): n_frames[i] = n_prefix delivers the new frames only. */
int q3tts_slots_codec_prime(q3tts_engine* e, int n_slots, const int32_t* slots, const int32_t* n_frames);
/* state of a carried-state stream (run_vocoder, tts_onnx.cpp:759-776, keeps none): frames pushed or primed so far, K / V rows the
 * sliding buffer can hold (P), bytes of the stream's K / V and row buffers; any output may be NULL */
int q3tts_codec_stream_info(q3tts_engine* e, int stream_id, int* n_done, int* kv_capacity_rows, int64_t* bytes);
/* ---- the same sessions, batch-first, on DEVICE pointers ----
 * For a host application that keeps embeddings, logits and ids in HBM: no PCIe round trip per call.  Row b of a call is slot b of the
 * engine (batch <= max_batch).  Tensors (float / id buffers) are device pointers on the engine's GPU, any allocator; control arrays
 * (`lens`, `active_mask`) are host pointers.  `stream` is the caller's hipStream_t (NULL: the engine's own stream, q3tts_stream): the
 * engine's stream first waits for everything the caller has enqueued on it, and the caller's stream is made to wait for the call's
 * work — the call is ordered inside the caller's stream like a kernel launch.  The calls that track positions on the host
 * (prefill / decode / code_predictor) return after their launches have completed; q3tts_sample_dev returns at once.
 * Per-slot state is shared with the "_host" entry points and the fused generation (positions, KV cache, the armed logits row). */
/* run_prefill, tts_onnx.cpp:615-665: embeds[batch][S][hidden] (row block b: lens[b] <= S <= max_ctx rows; lens NULL = S for all) ->
 * logits_last[batch][vocab] (the last prompt row's, all the reference consumes, :797-798), last_hidden[batch][hidden]; either may be NULL.
 * Consecutive slots with equal lengths share one pass through the layers; a slot on its own takes q3tts_talker_prefill_host's launches, and a slot with lens[b] > 16 its chunked
 * long-prompt path, one slot at a time. */
int q3tts_talker_prefill_dev(q3tts_engine* e, const float* embeds, int batch, int S, const int32_t* lens, float* logits_last, float* last_hidden, void* stream);
/* run_decode, tts_onnx.cpp:667-732: embeds[batch][hidden] -> logits[batch][vocab], last_hidden[batch][hidden]; one token appended to every
 * slot whose active_mask[b] != 0 (NULL: all).  Masked rows keep the batch's shape and leave outputs, position and slot state untouched. */
int q3tts_talker_decode_dev(q3tts_engine* e, const float* embeds, int batch, const uint8_t* active_mask, float* logits, float* last_hidden, void* stream);
/* predict_subcodes, tts_onnx.cpp:851-872, fused: last_hidden[batch][hidden] + code0[batch] (int64, as the reference holds ids) ->
 * sub[batch][n_groups - 1] int32: 15 KV-cached run_code_predictor passes (:734-757) with sample_token (:878-950) on device; row b draws
 * sub-code j with q3tts_rng_uniform(seed, stream_id0 + b, frame, j + 1), the fused generation loop's draw for that utterance and frame. */
int q3tts_code_predictor_dev(q3tts_engine* e, const float* last_hidden, const int64_t* code0, int batch, const q3tts_sampling* p, uint64_t seed,
                             uint32_t stream_id0, uint32_t frame, int32_t* sub, void* stream);
/* sample_token, tts_onnx.cpp:878-950, for a batch: logits[batch][n], u[batch] (uniforms in [0,1), one per row) -> ids[batch] int64 */
int q3tts_sample_dev(q3tts_engine* e, const float* logits, int batch, int n, const q3tts_sampling* p, const float* u, int suppress, int64_t* ids, void* stream);
/* sample_token, tts_onnx.cpp:878-905, on device; u in [0,1) replaces the mt19937 draw.
 * suppress != 0 applies the special-token suppression of tts_onnx.cpp:803-807 first. */
int q3tts_sample_host(q3tts_engine* e, const float* logits, int n, const q3tts_sampling* p, float u, int suppress, int64_t* token);
/* the same with p->repetition_penalty applied to the ids in history[0 .. n_history) first (duplicates count once, ids outside [0, n)
 * are ignored): what the fused loop's code0 sampler computes for an utterance that has emitted those ids */
int q3tts_sample_hist_host(q3tts_engine* e, const float* logits, int n, const q3tts_sampling* p, float u, int suppress,
                           const int64_t* history, int n_history, int64_t* token);
/* batch form on DEVICE pointers (see q3tts_sample_dev; returns at once): history[batch][hist_ld] int64, hist_len[batch] int32 (row b
 * uses its first hist_len[b] <= hist_ld ids) */
int q3tts_sample_hist_dev(q3tts_engine* e, const float* logits, int batch, int n, const q3tts_sampling* p, const float* u, int suppress,
                          const int64_t* history, int hist_ld, const int32_t* hist_len, int64_t* ids, void* stream);
float q3tts_rng_uniform(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t group);

/* ---- host logic of the path, mirrored (build_prompt_embeddings, tts_onnx.cpp:442-539) ---- */
/* lang: 0 Auto, 1 English, 2 Chinese, 3 Japanese, 4 Korean.  prompt[<=16][hidden], *S rows;
 * trailing[cap_rows][hidden] receives trailing_text_hidden_, *n_trailing its row count. */
int q3tts_build_prompt_host(q3tts_engine* e, const int64_t* ids, int n_ids, int lang, const float* speaker,
                            float* prompt, int* S, float* trailing, int cap_rows, int* n_trailing);
/* q3tts_build_prompt_host for a text whose end is not known (live text; tts_onnx.cpp:531-536 / :833-842): ids[0..2] are the role,
 * ids[3] the first text id, every later id becomes a trailing row — none is held back as the chat template's tail, no tts_eos row is
 * added, *n_trailing = n_ids - 4 (n_ids >= 4).  The prompt rows equal q3tts_build_prompt_host's for any whole text with the same first
 * four ids, bit for bit.  Begin a slot with the result, then q3tts_slot_text_open. */
int q3tts_build_prompt_open_host(q3tts_engine* e, const int64_t* ids, int n_ids, int lang, const float* speaker,
                                 float* prompt, int* S, float* trailing, int cap_rows, int* n_trailing);
/* Voice instructions — the reference README's roadmap row "Voice instructions (--instruct), 1.7B-VoiceDesign: Planned".  The prompt of
 * build_prompt_embeddings (tts_onnx.cpp:442-539) with an instruction in front of it: rows 0 .. n_instruct-1 of prompt[cap_prompt_rows][hidden]
 * are text_project(instruct_ids) (run_text_project, :541-559), the rest is exactly what q3tts_build_prompt_host produces; *S = n_instruct +
 * its row count (needs cap_prompt_rows >= n_instruct + 16).  n_instruct == 0 gives that prompt unchanged.  The caller supplies the
 * instruction already framed (q3tts_frame_instruct_ids): this entry does not know the chat template. */
int q3tts_build_prompt_instruct_host(q3tts_engine* e, const int64_t* ids, int n_ids, int lang, const float* speaker,
                                     const int64_t* instruct_ids, int n_instruct,
                                     float* prompt, int cap_prompt_rows, int* S, float* trailing, int cap_rows, int* n_trailing);
/* [HINT], unpinned.  Frames a tokenised instruction as a chat turn: <|im_start|>user\n ... <|im_end|>\n, i.e.
 * [151644, 872, 198] + text_ids + [151645, 198] — the upstream Qwen3-TTS instruct template as recalled; the reference has not implemented
 * it (README roadmap) and no VoiceDesign checkpoint was available to confirm it.  Should a checkpoint show another template, these five
 * constants are the only thing to change.  Host-only: needs no engine and no GPU.  Returns the framed length n + 5 and writes
 * min(n + 5, cap) ids (out may be NULL with cap = 0 to size); -1 on a bad argument. */
int64_t q3tts_frame_instruct_ids(const int32_t* text_ids, int64_t n, int64_t* out, int64_t cap);

/* ---- fused, batched generation (generate_codes + predict_subcodes, tts_onnx.cpp:782-872) ---- */
/* Admit an utterance into `slot`: uploads prompt + trailing rows, runs prefill, arms the slot.
 * stream_id selects the RNG stream; ignore_eos keeps EOS suppressed (fixed-length benchmark mode). */
int q3tts_slot_begin(q3tts_engine* e, int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                     const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos);
/* Continue from codes (tts_onnx.cpp:824-842 is the arithmetic of a frame's row; the reference itself can only start at frame 0).
 * q3tts_slot_begin with prefix_codes[n_prefix][n_groups] teacher-forced behind the prompt: the slot is left in the state q3tts_slot_begin
 * with the same arguments would have after generating exactly these as its first n_prefix frames — the talker's KV rows, the
 * repetition penalty's code0 history, the frame index behind the text rows (trailing[frame], then tts_pad) and the RNG draws
 * (q3tts_rng_uniform(seed, stream_id, frame, group)), and the slot's code buffer, which the vocoder reads for left context.  The
 * forced frames cost a chunked prefill (the weights streamed once per 128 rows) instead of one decode step each.  n_prefix == 0 is
 * q3tts_slot_begin, bit for bit.  p->max_new_tokens counts NEW frames; q3tts_slot_status, q3tts_slot_codes_host and
 * q3tts_slot_codec_decode_host then see n_prefix + new frames.  Refused before anything is reserved or armed: n_prefix < 0,
 * S + n_prefix + max_new_tokens > max_ctx, a code0 outside [0, vocab) or inside [suppress_begin, suppress_end) (EOS included: a
 * recorded frame never holds it), a sub-code outside [0, sub_vocab) — the message names frame and group.  KV pages are taken for
 * S + n_prefix + max_new_tokens; a pool that cannot hold them fails with "KV page pool exhausted" and arms nothing.
 * Uses: the next sentence of a document conditioned on the previous one's text and codes; in-context voice clone from reference codes
 * + reference text ([HINT], INTEGRATION.md section 5c: how upstream frames that prompt is unpinned, the arithmetic is verified, its
 * effect on audio is not: no checkpoint was available); resuming an utterance from its codes on another engine. */
int q3tts_slot_begin_codes(q3tts_engine* e, int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                           const int64_t* prefix_codes, int n_prefix,
                           const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos);
/* Advance every armed slot by n_steps frames (one hipGraph replay per frame).  Returns the number
 * of slots still active, <0 on error. */
int q3tts_decode_steps(q3tts_engine* e, int n_steps);
int q3tts_slot_status(q3tts_engine* e, int slot, int* n_frames, int* finished);

/* ---- live text: append text to a generating slot, stall when starved ----
 * The reference builds an utterance's trailing text block once (tts_onnx.cpp:531-536) and frame f's talker input row reads row f of it
 * and nothing else (:833-842), tts_pad beyond its end.  A slot therefore only has to be ONE text row ahead of its frame counter: an
 * open slot whose next frame has no row yet does not take tts_pad, it stalls — the step leaves it exactly as it was (codes, frame
 * counter, logits, KV rows) — and goes on, bit for bit as if it had held the whole text from the start, once the row is there.
 * q3tts_decode_steps keeps its meaning (its return counts stalled slots as active); a stalled slot never reaches max_frames on its own,
 * so a caller that feeds text looks at q3tts_slot_text_status.
 * Every call validates everything before anything moves: on error no slot has changed. */
/* Opens the slot's text (tts_onnx.cpp:531-536: the block is no longer final).  After any q3tts_slot_begin* variant (plain, codes, prefixed,
 * ragged member) and before the slot's first step; refused once the slot has stepped.  q3tts_decode_steps then fails, naming the
 * slot, while an open slot that has not stepped holds no row for its first frame (:833-842 reads it in that very step).
 * A slot begun behind teacher-forced frames must already hold those frames' text rows at its begin (they were read there): the open
 * is refused when it holds fewer rows than forced frames. */
int q3tts_slot_text_open(q3tts_engine* e, int slot);
/* n_rows projected rows [n_rows][hidden] (q3tts_text_project_host's) go behind the slot's text rows (the block of tts_onnx.cpp:531-536); close = 1
 * puts the tts_eos row behind them (:535) and ends the text: from then on frames beyond it take tts_pad (:833-842).  n_rows == 0 with
 * close = 1 just closes.  Errors: "not armed", "text already closed", "text too long for the trailing buffer". */
int q3tts_slot_text_append_host(q3tts_engine* e, int slot, const float* rows, int n_rows, int close);
/* The same for n distinct slots from token ids (tts_onnx.cpp:531-536 projects them into the block; :833-842 reads them): slot slots[i] takes
 * ids[offsets[i] .. offsets[i + 1]), close (optional) [n].  One text_project pass over all the ids on the device and one scatter launch,
 * whatever n.  Further errors: "duplicate slots", "text id out of range [0, text_vocab)". */
int q3tts_slots_text_append_ids(q3tts_engine* e, int n, const int32_t* slots, const int64_t* ids, const int32_t* offsets, const uint8_t* close);
/* n_text_rows: text rows the slot holds (tts_onnx.cpp:531-536, the tts_eos row included once closed); open; starved = open and
 * n_frames >= n_text_rows (:833-842 would need a row that has not arrived).  Any output may be NULL. */
int q3tts_slot_text_status(q3tts_engine* e, int slot, int* n_text_rows, int* open, int* starved);
/* codes[cap_frames][n_groups], int64 like the reference (tts_onnx.cpp:421-427) */
int q3tts_slot_codes_host(q3tts_engine* e, int slot, int64_t* codes, int cap_frames);
/* run_decode's outputs (tts_onnx.cpp:714-719) as the fused path holds them for the slot: logits[vocab] the slot's next code0 will be
 * sampled from and last_hidden[hidden] the code predictor's first input row (either may be NULL).  For teacher-forced parity checks
 * of the batched step; the data never leaves HBM in normal operation. */
int q3tts_slot_logits_host(q3tts_engine* e, int slot, float* logits, float* last_hidden);
/* vocoder over the slot's device-resident codes */
int q3tts_slot_codec_decode_host(q3tts_engine* e, int slot, float* pcm, int64_t cap, int64_t* out_len);
int q3tts_slot_release(q3tts_engine* e, int slot);

/* synthesize_tokens (tts_onnx.cpp:405-436) for a batch: utterance u has token ids
 * ids[offsets[u] .. offsets[u+1]).  pcm_out[u] receives up to pcm_cap samples, pcm_len[u] the
 * sample count, n_frames[u] the frames generated; codes_out (optional) [n_utt][max_new][n_groups]. */
int q3tts_synthesize_batch_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                const q3tts_sampling* p, uint64_t seed, int ignore_eos,
                                float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames,
                                int64_t* codes_out);

/* ---- voice-clone front end ---- */
/* synthesize_tokens with one speaker embedding per utterance spliced before CODEC_BOS (synthesize_clone,
 * tts_onnx.cpp:264-318; splice :481-498).  speakers[u] = [hidden] floats or NULL; speakers == NULL is
 * q3tts_synthesize_batch_host. */
int q3tts_synthesize_clone_batch_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                      const float* const* speakers, const q3tts_sampling* p, uint64_t seed, int ignore_eos,
                                      float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames,
                                      int64_t* codes_out);
/* The scheduler behind both: n_utt may exceed max_batch — utterances queue for the slots, a slot that finishes is re-armed with the
 * next one (continuous batching) while its codes are vocoded on a side stream.  max_new_per_utt (NULL: p->max_new_tokens for all) caps
 * each utterance separately: with ignore_eos it fixes ragged lengths for benchmarks.  Results do not depend on
 * the schedule (RNG stream = utterance index). */
int q3tts_synthesize_schedule_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out);
/* q3tts_synthesize_schedule_host that delivers audio while it generates (the reference returns an utterance's samples from one
 * run_vocoder call at its end, tts_onnx.cpp:759-776 / :430).  The loop: advance the live slots chunk_frames steps; decode every slot's
 * new frames in batched passes (q3tts_slots_codec_decode_new_host's); call cb once per utterance that has new audio — pcm holds the
 * samples of frames [frame_begin, frame_end) and is valid during the call only.  A finished slot delivers its tail with finished = 1,
 * exactly once and as that utterance's last call (n_samples may be 0), and is re-armed from the queue.  The vocoder passes run between the
 * decode chunks on the engine's stream, not beside them.  Codes, n_frames and (pcm_out non-NULL) the concatenated PCM are returned as by
 * the schedule entry.  A non-zero return from cb ends the job with the error "cancelled by callback" and releases the slots.
 * On a pooled engine (q3tts_create_pooled) an utterance is admitted only when prompt + cap fit the pool: there is no on-demand growth
 * and no preemption here, because audio that has been delivered cannot be taken back. */
typedef int (*q3tts_audio_cb)(void* user, int utt, int frame_begin, int frame_end, const float* pcm, int64_t n_samples, int finished);
int q3tts_synthesize_stream_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                 const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                 float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                 int chunk_frames, q3tts_audio_cb cb, void* user);
/* q3tts_synthesize_stream_host (same audio callback, same outputs, no preemption) for texts that arrive while their audio is generated:
 * a pull callback takes the place of ids / offsets (tts_onnx.cpp:531-536 builds the text block from the whole text; :833-842 reads
 * one row of it per frame, which is all a slot has to be ahead).  text_cb is called on the caller's thread between decode chunks, for
 * utterance u while its text is open: write up to cap new ids, set *n (0: nothing yet) and *closed (1: no more text will come).  A
 * non-zero return cancels the job ("cancelled by callback").  A callback with nothing to give should block or sleep: when every live
 * slot is starved and nothing can be admitted the loop polls again at once.
 * The ids of an utterance are those of the other entries: 3 role ids, the text, and the chat template's two-id tail, which every
 * entry drops (tts_onnx.cpp:531: text_end = n - 2) — the last two ids received are therefore held back until the text is closed.
 * An utterance is queued from the start and admitted once it holds 5 usable ids (role, first text id, the row of frame 0) or is
 * closed with at least 4 ids.  Admission keeps the queue order (RNG stream and slot use as in the stream entry): an utterance
 * whose text has not arrived yet holds back the ones queued behind it, ready or not.  Per loop turn: poll every open utterance (live or queued), admit, append the new ids of all live slots
 * in ONE q3tts_slots_text_append_ids call, decode chunk_frames steps, vocode and deliver the new frames.  A stalled slot has an empty
 * frame range and gets no audio callback that turn.  Codes and frame counts equal q3tts_synthesize_stream_host's on the same ids. */
typedef int (*q3tts_text_cb)(void* user, int utt, int64_t* ids, int cap, int32_t* n, int32_t* closed);
int q3tts_synthesize_live_host(q3tts_engine* e, int n_utt, q3tts_text_cb text_cb, void* text_user, int lang,
                               const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                               float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                               int chunk_frames, q3tts_audio_cb cb, void* user);
/* The scheduler entries with a voice instruction per utterance (README roadmap row "--instruct"): instruct_ids / instruct_offsets
 * [n_utt + 1] give utterance u the framed instruction ids [instruct_offsets[u], instruct_offsets[u + 1]); an empty range means none, and
 * instruct_ids == NULL none for any.  An instructed utterance's prompt is q3tts_build_prompt_instruct_host's and is prefilled on its own
 * (long-prompt path); the others share their pass as before.  cb != NULL: q3tts_synthesize_stream_host's delivery; cb == NULL:
 * q3tts_synthesize_schedule_host (chunk_frames and user are ignored).  One implementation behind all three; results do not depend on the
 * schedule (RNG stream = utterance index). */
int q3tts_synthesize_instruct_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   int chunk_frames, q3tts_audio_cb cb, void* user,
                                   const int64_t* instruct_ids, const int32_t* instruct_offsets);
/* q3tts_synthesize_schedule_host with teacher-forced frames per utterance (tts_onnx.cpp:824-842; q3tts_slot_begin_codes is the begin):
 * prefix_codes / prefix_offsets [n_utt + 1], in FRAMES, give utterance u the frames [prefix_offsets[u], prefix_offsets[u + 1]) of
 * prefix_codes[.][n_groups]; an empty range means none, and prefix_codes == NULL none for any.  A prefixed utterance is begun on its own
 * (like an instructed one); a preempted one is re-admitted through the same forced begin.  n_frames[u] and codes_out cover prefix + new
 * frames: codes_out (optional) is [n_utt][P + max_new_tokens][n_groups], P the longest prefix of the job.  pcm_out[u] receives only
 * the samples the NEW frames own, out of the decode of all the utterance's frames (the decoder is causal: that slice is exact, and it
 * joins the prefix's own audio without a seam), pcm_len[u] their count.  An utterance without a prefix gets what
 * q3tts_synthesize_schedule_host gives it, bit for bit.  Non-streaming only: delivery through a q3tts_audio_cb with a prefix is not
 * implemented here (q3tts_synthesize_continue_stream_host is the streaming entry). */
int q3tts_synthesize_continue_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   const int64_t* prefix_codes, const int32_t* prefix_offsets);
/* q3tts_synthesize_stream_host with teacher-forced frames per utterance (tts_onnx.cpp:824-842 is a frame's row, :759-776 the vocoder
 * the chunks stand for): q3tts_synthesize_continue_host's arguments, in its order, then the stream entry's chunk_frames / cb / user.
 * A prefixed utterance is begun through the continue entry's forced begin (on its own, or as a member of the one ragged begin under
 * Q3TTS_FLAG_RAGGED_PREFILL), so its codes equal that entry's bit for bit; the fresh prefixed slots of an admission look are primed in
 * one q3tts_slots_codec_prime call before the first decode chunk, so only the new frames are ever vocoded.  cb's frame_begin /
 * frame_end count the utterance's frames with the prefix included: an utterance's first call has frame_begin == n_prefix.  pcm_out /
 * pcm_len hold the new frames' samples only; n_frames and codes_out ([n_utt][P + max_new_tokens][n_groups]) are the continue entry's.
 * Admission as in the stream entry (prompt + prefix frames + cap must fit, no preemption).  An utterance with an empty prefix range
 * gets what q3tts_synthesize_stream_host gives it, bit for bit; prefix_codes == NULL is that entry. */
int q3tts_synthesize_continue_stream_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                          const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                          float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                          const int64_t* prefix_codes, const int32_t* prefix_offsets,
                                          int chunk_frames, q3tts_audio_cb cb, void* user);
/* ---- shared prompt prefix: run_prefill (tts_onnx.cpp:615-665) once for rows that many utterances have in front of their prompts ----
 * A prefix is n_rows talker input rows (an instruction's text_project rows, say), 1 <= n_rows < max_ctx, prefilled once in a borrowed
 * free slot; the K / V rows of its positions are kept on the engine in a compact store.  Slots begun behind it get a COPY of those rows
 * in their own pages (no page is shared: a slot owns pages for prefix + prompt + frames like any slot) and only their own rows are
 * prefilled, at base position n_rows; causality makes that exact (the rows of positions [0, P) depend on rows [0, P) alone).  Up to 64
 * prefixes are live at a time; ids are never reused.  Nothing is changed when a call fails (no free slot, pool too small, 65th prefix). */
int q3tts_prefix_create(q3tts_engine* e, const float* rows, int n_rows, int* prefix_id);   /* run_prefill, tts_onnx.cpp:615-665 */
/* text_project (tts_onnx.cpp:615-665 consumes its rows) of framed instruction ids (q3tts_frame_instruct_ids), then q3tts_prefix_create */
int q3tts_prefix_create_instruct(q3tts_engine* e, const int64_t* framed_ids, int n, int* prefix_id);
/* n_rows and the bytes of the store: n_rows x n_layers x n_kv_heads x head_dim x 2 (K and V) x element size (4, or 2 with Q3TTS_FLAG_KV_BF16) */
int q3tts_prefix_info(q3tts_engine* e, int prefix_id, int* n_rows, int64_t* bytes);
/* frees the store; refused while a running q3tts_synthesize_prefixed_host job uses the prefix (its callback may try) */
int q3tts_prefix_release(q3tts_engine* e, int prefix_id);
/* q3tts_slot_begin / q3tts_slot_begin_codes behind prefix prefix_id (-1: none, then exactly those entries; run_prefill,
 * tts_onnx.cpp:615-665, for the prompt's rows at base P).  P + S + n_prefix_frames + max_new_tokens <= max_ctx.  The slot's frames,
 * status and codes are as without a prefix; its context starts at P + S (+ n_prefix_frames). */
int q3tts_slot_begin_prefixed(q3tts_engine* e, int slot, int prefix_id, const float* prompt, int S, const float* trailing, int n_trailing,
                              const int64_t* prefix_codes, int n_prefix_frames, const q3tts_sampling* p, uint64_t seed, uint32_t stream_id, int ignore_eos);
/* n slots at once (run_prefill, tts_onnx.cpp:615-665, batched): everything is validated first (ids live, lengths, slots distinct), pages
 * are reserved all or nothing, each prefix is copied into its slots in one launch, and members with equal S <= 16 share one pass through
 * the talker (up to 128 rows, each member at its own base; a member with prefix_ids[i] == -1 sits at base 0).  Members with S > 16, and
 * engines whose dims are not multiples of 128, are begun one at a time.  prefix_ids == NULL or all -1: q3tts_slot_begin's launches. */
int q3tts_slots_begin_prefixed(q3tts_engine* e, int n, const int32_t* slots, const int32_t* prefix_ids, const float* const* prompts, const int32_t* S,
                               const float* const* trailing, const int32_t* n_trailing, const q3tts_sampling* p, uint64_t seed,
                               const uint32_t* stream_ids, int ignore_eos);
/* Ragged begin (run_prefill, tts_onnx.cpp:615-665, and the frame loop's talker input rows, :824-842, for many slots at once): the
 * n-slot form of q3tts_slot_begin_prefixed.  Member i is slot slots[i] behind prefix prefix_ids[i] (NULL or -1: none) with an own
 * prompt of ANY S[i] and n_prefix_frames[i] teacher-forced frames prefix_codes[i][.][n_groups] (either array NULL: none; an entry may be
 * NULL where its count is 0).  Everything is validated first (q3tts_slot_begin_prefixed's checks and messages, slots distinct), KV pages
 * are reserved all or nothing, and on failure no slot is armed and no page moves.  The members' rows (prompt rows, then the forced
 * frames' rows) are laid end to end in call order and cut into chunks of 128 rows; a chunk may hold rows of many slots, a member that does
 * not fit the rest of a chunk continues in the next.  One pass through the talker per chunk; the codec head runs on each member's last
 * row.  Each slot is left exactly as q3tts_slot_begin_prefixed leaves it (frames, status, codes, context, RNG stream).
 * Exact (bit for bit): n == 1 against q3tts_slot_begin_prefixed; the same call twice; Q3TTS_FLAG_KV_BF16 against
 * Q3TTS_FLAG_KV_ROUND_BF16; engines whose dims are not multiples of 128 and calls of fewer than 12 rows (members begun one at a time).
 * Within 2e-4 of the reference arithmetic (4e-3 with the bf16 cache), not bit-identical: a member of a multi-member call against the same
 * member begun alone — the projections see a different row count, as in every batched path here. */
int q3tts_slots_begin_ragged(q3tts_engine* e, int n, const int32_t* slots, const int32_t* prefix_ids, const float* const* prompts, const int32_t* S,
                             const float* const* trailing, const int32_t* n_trailing,
                             const int64_t* const* prefix_codes /* entries may be NULL */, const int32_t* n_prefix_frames,
                             const q3tts_sampling* p, uint64_t seed, const uint32_t* stream_ids, int ignore_eos);
/* q3tts_synthesize_instruct_host with prefix_ids[n_utt] (-1: none) in place of the instruction ranges (run_prefill, tts_onnx.cpp:615-665,
 * per utterance only for its own rows): utterance u's prompt is q3tts_build_prompt_host's, begun behind prefix prefix_ids[u].  Utterances
 * admitted in the same look with equal S share their pass; a preempted utterance is re-admitted through the same prefixed begin; the
 * job's prefixes cannot be released while it runs.  cb as in q3tts_synthesize_instruct_host.  Results do not depend on the schedule
 * (RNG stream = utterance index). */
int q3tts_synthesize_prefixed_host(q3tts_engine* e, int n_utt, const int64_t* ids, const int32_t* offsets, int lang,
                                   const float* const* speakers, const q3tts_sampling* p, const int32_t* max_new_per_utt, uint64_t seed, int ignore_eos,
                                   float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, int32_t* n_frames, int64_t* codes_out,
                                   int chunk_frames, q3tts_audio_cb cb, void* user, const int32_t* prefix_ids);
/* io::read_wav (src/io/wav_reader.h:13, wav_reader.cpp:28-143): mono float samples; -1 when the reference
 * returns an empty vector.  Call with out == NULL to learn *n_samples. */
int q3tts_read_wav_host(const char* path, float* out, int64_t cap, int64_t* n_samples, int32_t* sample_rate);
/* The bytes of a G.711 WAV (format tag 7 mu-law / 6 A-law, 8 bits, mono), which q3tts_read_wav_host refuses: *format is
 * Q3TTS_PCM_MULAW (2) / Q3TTS_PCM_ALAW (3), the bytes are what an encoder stream of that format takes.  -2 for a G.711 file with more
 * than one channel (stereo is not read), -1 for anything else.  Sizing call: out NULL. */
int q3tts_read_wav_g711_host(const char* path, uint8_t* out, int64_t cap, int64_t* n_samples, int32_t* sample_rate, int* format);
/* io::resample (wav_reader.cpp:145-164): linear interpolation; returns the output length */
int64_t q3tts_resample_host(const float* in, int64_t n, int32_t src_rate, int32_t dst_rate, float* out, int64_t cap);
/* io::resample over audio that is still arriving: the output samples a stream at src_rate has emitted IN ALL once it holds n_received
 * samples.  finish != 0: q3tts_resample_host's length.  finish == 0: the largest count whose every output i has both taps received
 * unclamped, floor(i / ratio) + 1 <= n_received - 1, and lies below (size_t)((double)n_received * ratio), ratio = dst_rate / src_rate
 * in double: whatever the final length, io::resample produces it.  Equal rates: n_received.  A push's length is the difference of
 * two calls.  Host-only, no engine; -1 for a rate < 1 or n_received < 0. */
int64_t q3tts_resample_stream_emitted(int32_t src_rate, int32_t dst_rate, int64_t n_received, int finish);
/* MelExtractor::extract with the settings of tts_onnx.cpp:347-354 (24 kHz, n_fft = win = 1024, hop 256, 128 HTK
 * mels, 0-12 kHz, log power): mel[128][*frames].  Call with mel == NULL to learn *frames. */
int q3tts_mel_host(const float* audio, int64_t n, float* mel, int64_t cap, int32_t* frames);
/* has_speaker_encoder (tts_onnx.h:172) */
int q3tts_has_speaker_encoder(q3tts_engine* e);
/* run_speaker_encoder (tts_onnx.cpp:367-403): mel[128][frames] (MelExtractor layout) -> embed[spk_enc_dim], on the GPU */
int q3tts_speaker_encoder_host(q3tts_engine* e, const float* mel, int frames, float* embed);
/* extract_speaker_embedding (tts_onnx.cpp:331-365): wav -> 24 kHz -> mel -> speaker encoder */
int q3tts_extract_speaker_embedding_host(q3tts_engine* e, const char* wav_path, float* embed);
/* The same front end on the GPU for reference audio that is already in memory (mono float samples, any rate; callers mix channels
 * down as read_wav does).  Each call stages its audio in one pinned copy, runs on the engine's stream in a workspace the engine owns
 * (grow-only, freed by q3tts_destroy; at most about 1 GiB per group of clips, larger batches are processed group after group) and
 * ends with one stream synchronisation.  -1 with q3tts_last_error on failure; nothing is written to the outputs then. */
/* io::resample (wav_reader.cpp:145-164) on the GPU: the same samples as q3tts_resample_host, bit for bit; returns the output length
 * and writes min(length, cap) samples when out != NULL */
int64_t q3tts_resample_gpu_host(q3tts_engine* e, const float* in, int64_t n, int32_t src_rate, int32_t dst_rate, float* out, int64_t cap);
/* resample to 24 kHz (when sample_rate != 24000) + MelExtractor::extract on the GPU: mel[128][*frames]; mel == NULL only sizes.
 * Needs finalized weights.  Differs from q3tts_mel_host by the rounding of logf only; -1 for an empty clip, as q3tts_mel_host. */
int q3tts_mel_gpu_host(q3tts_engine* e, const float* audio, int64_t n, int32_t sample_rate, float* mel, int64_t cap, int32_t* frames);
/* extract_speaker_embedding (tts_onnx.cpp:331-365) for n_clips clips at once: embeds[n_clips][spk_enc_dim].  Every clip needs 5 to
 * 16384 mel frames (about 0.1 s to 175 s); an error names the clip index.  A clip's embedding does not depend on the rest of the
 * batch, nor on how the batch was split into workspace groups. */
int q3tts_speaker_embed_pcm_batch_host(q3tts_engine* e, int n_clips, const float* const* pcm, const int64_t* n_samples,
                                       const int32_t* sample_rates, float* embeds);

/* ---- audio -> codes: the 12 Hz speech tokenizer's encoder ([HINT], unpinned: transformers MimiModel.encode; the arithmetic is verified
 * against it, its effect on audio is not: no checkpoint was available) ----
 * The producer of what q3tts_slot_begin_codes consumes (tts_onnx.cpp:824-842 is the arithmetic of a frame's row; the reference has no
 * encoder).  All of it runs in fp32 on the GPU in a workspace the engine owns (grow-only, freed by q3tts_destroy).  A clip holds at most
 * 1 440 000 samples at 24 kHz (60 s) and, at another rate, 23 040 000 samples before resampling; a batch is processed in consecutive groups of at most 2 880 000 samples.  An engine whose config
 * has enc_hidden == 0 answers "model has no audio encoder". */
int q3tts_has_audio_encoder(q3tts_engine* e);
/* frames of a clip of n_samples samples at 24 kHz: ceil(n / samples per frame) through the convs' own padding rule; host-only.
 * -1 without an encoder or for n_samples < 1. */
int64_t q3tts_audio_encode_len(q3tts_engine* e, int64_t n_samples);
/* pcm24k[n_samples] (mono, 24 kHz) -> codes_out[*n_frames][n_groups] int64, the layout q3tts_slot_codes_host returns and
 * q3tts_slot_begin_codes takes.  cap_frames < the clip's frames is refused. */
int q3tts_audio_encode_host(q3tts_engine* e, const float* pcm24k, int64_t n_samples, int64_t* codes_out, int cap_frames, int32_t* n_frames);
/* n_clips clips at once, each at its own rate (clips not at 24 kHz go through the GPU resampler of q3tts_resample_gpu_host first): one
 * set of launches per group, padding never crosses a clip boundary, and every clip's codes are bit-identical to encoding it alone.
 * codes_out[i] receives n_frames[i] x n_groups ids (caps[i] frames of room). */
int q3tts_audio_encode_batch_host(q3tts_engine* e, int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates,
                                  int64_t* const* codes_out, const int32_t* caps, int32_t* n_frames);
/* Parity aid: the rows the quantiser sees, latents[*n_frames][enc_hidden] (the stride-2 conv's output), and optionally the codes. */
int q3tts_audio_encode_latents_host(q3tts_engine* e, const float* pcm24k, int64_t n_samples, float* latents, int64_t* codes_out, int cap_frames,
                                    int32_t* n_frames);
/* Parity aid: q3tts_audio_encode_batch_host that also returns each clip's latents, latents_out[i][n_frames[i]][enc_hidden] (caps[i] frames of
 * room; codes_out or latents_out may be NULL, and so may single entries) */
int q3tts_audio_encode_batch_latents_host(q3tts_engine* e, int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates,
                                          int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames);
/* Parity aid (engines created with Q3TTS_FLAG_TEST_HOOKS): the encoder's transformer alone on rows[n_rows][enc_hidden] -> out, same shape */
int q3tts_test_audio_encoder_transformer_host(q3tts_engine* e, const float* rows, int n_rows, float* out);

/* ---- audio -> codes while the audio arrives: carried-state pushes of many streams ([HINT], as the encoder above; beside the reference's
 * clone front end tts_onnx.cpp:331-365, which has no encoder) ----
 * A stream takes mono samples at the source's own rate (1 .. 384 000 Hz) as float or int16, in pushes of any size, and returns the
 * codes of the frames each push completes.  No caller has to resample first, or convert: a stream that is not 24 kHz float resamples on the GPU
 * on the way in (io::resample's arithmetic on absolute sample indices; it carries its last ceil(rate / 24000) + 1 samples).
 * Promise: the codes (and latents) of a stream begun at rate R, however its samples were cut into pushes and whatever streams of
 * whatever rates and formats shared its calls, are bit-identical to q3tts_audio_encode_batch_host of the concatenated audio at rate
 * R (q3tts_audio_encode_host at 24 kHz); int16 samples v are the float audio v / 32768.0f, q3tts_read_wav_host's conversion.
 * An unfinished stream that holds N samples has fed the encoder E = q3tts_resample_stream_emitted(R, 24000, N, 0) samples at 24 kHz:
 * output i is emitted once (1) both its taps have arrived, floor(i / ratio) + 1 <= N - 1, and (2) i < floor(N * ratio), so that the
 * one-shot of any longer clip produces it (ratio = 24000.0 / R, in double).  Latency: floor(E / samples per frame) frames have been
 * returned, at most one 24 kHz sample behind real time (at 24 kHz float E = N: none).  The finishing push emits what
 * io::resample's clamped right edge adds and returns the 0 or 1 frames the one-shot's right edge completes.
 * State per stream lives in device buffers of its own (per conv k - 1 input rows, per transformer layer window - 1 K and V rows;
 * q3tts_audio_stream_info reports the bytes), kept by q3tts_audio_stream_end for the next begin and freed by q3tts_destroy.
 * At most 1024 streams are open at a time.  q3tts_last_audio_encode_ms covers pushes too. */
/* A new stream that will take at most max_samples samples (0: 1 440 000 = 60 s; at most 86 400 000 = one hour).  A stream longer than
 * any before it regrows the RoPE tables (the same double-precision formula: existing rows keep their bits) and synchronises for it. */
int q3tts_audio_stream_begin(q3tts_engine* e, int64_t max_samples, int* stream_id);
/* The same for a source at sample_rate (1 .. 384 000; anything else is refused with the value) whose samples are float
 * (Q3TTS_PCM_F32), int16 (Q3TTS_PCM_S16) or G.711 bytes (Q3TTS_PCM_MULAW / _ALAW, below).  max_samples counts the stream's OWN samples: 0 = 60 s at its rate, at most one hour.
 * q3tts_audio_stream_begin is this at 24 000 / Q3TTS_PCM_F32. */
#define Q3TTS_PCM_F32 0
#define Q3TTS_PCM_S16 1
/* ---- G.711 (ITU-T G.711; RTP payload types 0 and 8, WAV format tags 7 and 6) ----
 * Two more sample formats for the encoder streams (in) and the sinks (out): one uint8_t per sample, mu-law or A-law.  Both laws are
 * defined on the int16 the engine already makes, as sign-magnitude codes: enc(-s) == enc(s) ^ 0x80 for s in 1 .. 32767 (not the
 * `pcm >> 2` of a negative two's-complement value that some C libraries use).
 * Out (sinks): s = (int16_t)(clip(y, -1, 1) * 32767.0f), the int16 rule above, unchanged; the byte is enc(s).
 *   mu-law enc(s): m = min(|s|, 32635) + 132 (|s| in 32 bits); e = floor(log2 m) - 7 (0 .. 7, by count-leading-zeros: integers only,
 *     no table); mant = (m >> (e + 3)) & 15; byte = ~((s < 0 ? 0x80 : 0) | e << 4 | mant) & 0xFF.  Silence is 0xFF.
 *   A-law enc(s): a = min(|s|, 32767) >> 3; a < 32: e = 0, mant = a >> 1; otherwise e = floor(log2 a) - 4 (1 .. 7), mant = (a >> e) & 15;
 *     byte = ((s >= 0 ? 0x80 : 0) | e << 4 | mant) ^ 0x55.  Silence is 0xD5.
 * In (encoder streams): the byte decodes to an int16 s and the sample is (float)s / 32768.0f, the int16 ingest rule.
 *   mu-law dec(b): u = ~b & 0xFF; e = (u >> 4) & 7; mant = u & 15; m = (((mant << 3) + 132) << e) - 132; s = u & 0x80 ? -m : m.  Range +-32124.
 *   A-law dec(b): x = b ^ 0x55; e = (x >> 4) & 7; mant = x & 15; m = e == 0 ? (mant << 4) + 8 : ((mant << 4) + 0x108) << (e - 1);
 *     s = x & 0x80 ? m : -m.  Range +-32256.
 * enc(dec(b)) == b for every byte except mu-law 0x7F (negative zero, which re-encodes as 0xFF).
 * Sample counts, push limits, max_samples, q3tts_sink_emitted and q3tts_resample_stream_emitted do not depend on the format. */
#define Q3TTS_PCM_MULAW 2
#define Q3TTS_PCM_ALAW 3
/* Host only, no engine: the same inline functions the kernels use.  n samples; -1 for a format other than Q3TTS_PCM_MULAW / _ALAW,
 * n < 0 or a NULL pointer with n > 0. */
int q3tts_g711_encode_host(int format, const int16_t* in, int64_t n, uint8_t* out);
int q3tts_g711_decode_host(int format, const uint8_t* in, int64_t n, int16_t* out);
int q3tts_audio_stream_begin_rate(q3tts_engine* e, int32_t sample_rate, int format, int64_t max_samples, int* stream_id);
/* the rate and format a stream was begun with (either pointer may be NULL) */
int q3tts_audio_stream_format(q3tts_engine* e, int stream_id, int32_t* sample_rate, int* format);
/* host-only: frames the next push of n_samples (finish 0/1) to this stream would return; -1 when that push would be refused */
int q3tts_audio_stream_push_len(q3tts_engine* e, int stream_id, int64_t n_samples, int finish);
/* n_samples >= 0 more samples; finish != 0 ends the stream's audio (zeros / the repeated last row complete the last frame, as in the
 * one-shot).  codes_out[*n_frames][n_groups] int64 in q3tts_audio_encode_host's layout: the NEW frames only.  n_samples == 0 without
 * finish does nothing; finish on a stream that never got a sample returns 0 frames.  A push holds at most 60 s of the stream's own
 * samples (1 440 000 at 24 kHz).  n_samples counts the stream's own samples; this entry serves float streams of any rate and
 * refuses an int16 or G.711 stream by name. */
int q3tts_audio_stream_push_host(q3tts_engine* e, int stream_id, const float* pcm24k, int64_t n_samples, int finish,
                                 int64_t* codes_out, int cap_frames, int32_t* n_frames);
/* the same with the samples read in the stream's own format: float for Q3TTS_PCM_F32, int16_t for Q3TTS_PCM_S16 (staged as int16,
 * half the upload, and converted on the GPU), uint8_t for Q3TTS_PCM_MULAW / _ALAW (staged as bytes, a quarter, decoded on the GPU) */
int q3tts_audio_stream_push_any_host(q3tts_engine* e, int stream_id, const void* pcm, int64_t n_samples, int finish,
                                     int64_t* codes_out, int cap_frames, int32_t* n_frames);
/* Many streams in one call: one set of launches per group of at most 2 880 000 new samples, whatever the number of streams, and each
 * stream's result is what pushing it alone gives.  The call is validated completely before any stream moves (ids distinct, open and
 * not finished; sizes; each stream's total within its max_samples; caps[i] frames of room): a call refused by these checks leaves every
 * stream where it was.  (A HIP error is another matter: streams advance group by group, so after one in a later group of a call of
 * more than 2 880 000 new samples the streams of earlier groups have moved; end every stream of such a call.)  finish NULL: no stream finishes.  latents_out (NULL ok, and so may single entries) is the parity aid of
 * q3tts_audio_encode_batch_latents_host: latents_out[i][n_frames[i]][enc_hidden].
 * The float entry serves Q3TTS_PCM_F32 streams of any rate and refuses an int16 or G.711 stream by name. */
int q3tts_audio_stream_push_batch_host(q3tts_engine* e, int n_streams, const int32_t* stream_ids, const float* const* pcm24k,
                                       const int64_t* n_samples, const int32_t* finish /* NULL: none */,
                                       int64_t* const* codes_out, float* const* latents_out /* NULL ok: parity aid */,
                                       const int32_t* caps, int32_t* n_frames);
/* q3tts_audio_stream_push_batch_host with pcm[i] read in stream i's own format; streams of different rates and formats may share a
 * call (groups are cut by new 24 kHz samples and by at most 23 040 000 samples to resample) */
int q3tts_audio_stream_push_batch_any_host(q3tts_engine* e, int n_streams, const int32_t* stream_ids, const void* const* pcm,
                                           const int64_t* n_samples, const int32_t* finish /* NULL: none */,
                                           int64_t* const* codes_out, float* const* latents_out /* NULL ok: parity aid */,
                                           const int32_t* caps, int32_t* n_frames);
/* samples received (at the stream's own rate), frames returned, finished 0/1 and the bytes of the stream's device state (any pointer may be NULL) */
int q3tts_audio_stream_info(q3tts_engine* e, int stream_id, int64_t* n_samples, int32_t* n_frames, int* finished, int64_t* bytes);
/* closes the stream (finished or not); its id and buffers serve a later q3tts_audio_stream_begin */
int q3tts_audio_stream_end(q3tts_engine* e, int stream_id);

/* ---- audio out at the sink's rate: carried-state band-limited resampler ([HINT] no counterpart in the reference, whose main.cpp writes
 * 24 kHz only) ----
 * Everything above delivers 24 kHz float.  A sink delivers the same audio at its own rate R (4 000 .. 192 000 Hz) as float
 * (Q3TTS_PCM_F32), int16 (Q3TTS_PCM_S16) or G.711 bytes (Q3TTS_PCM_MULAW / _ALAW: the byte of that int16, "G.711" above), resampled on the GPU between the vocoder and the device -> host copy, all streams of a push
 * in one launch.  24 000 / Q3TTS_PCM_F32 is "no sink": no launch, the same bytes as before.
 * The resampler: g = gcd(R, 24000), L = R / g, M = 24000 / g; output j sits at input position j M / L.  s = min(1, R / 24000), half-width
 * H = 16 / s input samples, half = ceil(H), taps = 2 half, cut-off f = 0.92 s.  Table row p (0 <= p < L), tap t: d = (t - half + 1) - p / L,
 * h = f sinc(f d) I0(10 sqrt(1 - (d / H)^2)) / I0(10) for |d| < H, else 0 (sinc(x) = sin(pi x) / (pi x)); each row is formed in double,
 * divided by its own sum and rounded to float.  Output j: kc = floor(j M / L), p = (j M) mod L, y[j] = sum_t tab[p][t] x[kc - half + 1 + t]
 * with t ascending in fp32 (unfused), x[k] = 0 for k < 0 and, once the sink is finished, for k >= n.  A sample's bits depend on its
 * absolute index alone: never on how the audio was cut into pushes or on which sinks shared a launch.
 * A sink that has received N samples and is not finished has emitted E(N) = max(0, ceil((N - half) L / M)) outputs: those whose last
 * tap kc + half <= N - 1 has arrived (latency: half input samples; 0.67 ms at >= 24 kHz, 2 ms at 8 kHz, 4 ms at 4 kHz).  Finished, it has
 * emitted ceil(n L / M).  A push delivers E(after) - E(before).  R = 24000: no filter, no latency, E(N) = N.
 * int16 is the CLI's rule (save_wav16): clip to [-1, 1], then (int16_t)(v * 32767.0f), truncating; converted on the GPU.
 * Known limit: a primed stream's sink (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts from silence,
 * x[k] = 0 for k < 0, so behind a prefix the first `half` input samples' worth of output differs from a resample of prefix +
 * continuation.  At 24 kHz the seam stays exact. */
/* Host only, no engine.  The plan for `rate`: any output pointer may be NULL; table (NULL ok) receives the L * taps floats the device
 * uses when cap >= L * taps.  -1 for a rate outside 4 000 .. 192 000 or one whose table would exceed 2^22 floats (191 999: L = 191 999);
 * q3tts_sink_last_error() then names the rate (thread-local, valid until the thread's next sink_plan / sink_emitted call). */
int q3tts_sink_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* half, int32_t* taps, float* table, int64_t cap);
const char* q3tts_sink_last_error(void);
/* Host only: outputs a sink at `rate` has emitted in all after n_received samples at 24 kHz (finished != 0: the whole clip's
 * ceil(n L / M)).  -1 for a rate q3tts_sink_plan refuses or n_received < 0. */
int64_t q3tts_sink_emitted(int32_t rate, int64_t n_received, int finished);
/* Sinks on their own: the stage by itself, fed 24 kHz float from the host.  A sink accepts at most one hour of input (86 400 000
 * samples), a push at most 1 440 000.  At most 4096 sinks are open at a time (vocoder streams' sinks included). */
int q3tts_pcm_sink_begin(q3tts_engine* e, int32_t sample_rate, int format, int* sink_id);
/* n sinks (distinct, open, not finished), sink i given n_in[i] >= 0 more samples pcm24[i]; finish[i] != 0 (finish NULL: none) flushes
 * the tail with this push and closes the sink's audio (n_in[i] == 0 allowed).  out[i] is float*, int16_t* or uint8_t* by the sink's format,
 * with room for cap_samples; out_len[i] is the push's length by the rule above (min(out_len, cap_samples) samples are written).  The call
 * is validated completely before any sink moves.  n_in[i] == 0 without finish leaves the sink as it was. */
int q3tts_pcm_sink_push_batch_host(q3tts_engine* e, int n, const int32_t* sink_ids, const float* const* pcm24, const int64_t* n_in,
                                   const uint8_t* finish, void* const* out, int64_t cap_samples, int64_t* out_len);
int q3tts_pcm_sink_end(q3tts_engine* e, int sink_id);
/* Vocoder streams.  A stream delivers through a sink from its first sample on: refused, by name, once the stream has delivered a
 * sample.  24 000 / Q3TTS_PCM_F32 takes the sink away again. */
int q3tts_codec_stream_set_sink(q3tts_engine* e, int stream_id, int32_t sample_rate, int format);
/* q3tts_codec_stream_push_batch_host with pcm_out[s] read in stream s's format (float without a sink) and pcm_cap / pcm_len counted in
 * its samples.  finish[s] != 0 (NULL: none; only for streams with a sink) flushes the sink's tail with this push; a push of 0 frames
 * with finish is allowed.  The float entries keep serving streams without a sink and refuse a stream with one by name. */
int q3tts_codec_stream_push_batch_any_host(q3tts_engine* e, int n_streams, const int32_t* stream_ids, const int64_t* codes, const int32_t* frame_offsets,
                                           void* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len, const uint8_t* finish);
/* The scheduler: one setter for the four streaming entries (q3tts_synthesize_stream_host, _live_host, _instruct_host with a callback,
 * _continue_stream_host).  While a sink is set they deliver through sink->cb in the sink's format (pcm is float*, int16_t* or, for G.711, uint8_t*), their
 * own cb argument may be NULL, and a non-NULL pcm_out is refused by name.  The finished = 1 call carries the flushed tail, so an
 * utterance's calls add up to ceil(n24 L / M) samples; pcm_len counts the sink's samples.  Codes, frame counts and RNG use are
 * untouched.  sink == NULL: none.  The struct is copied. */
typedef int (*q3tts_audio_any_cb)(void* user, int utt, int frame_begin, int frame_end, const void* pcm, int64_t n_samples, int finished);
typedef struct { int32_t sample_rate; int32_t format; q3tts_audio_any_cb cb; void* user; } q3tts_sink;
int q3tts_engine_set_sink(q3tts_engine* e, const q3tts_sink* sink);

/* ---- speaking rate: carried-state WSOLA time stretch ([HINT] no counterpart in the reference, which has no speed control; DESIGN.md
 * 4m) ----
 * A speed S, an integer in permille (500 .. 2000), makes the audio S / 1000 times as fast at the same pitch: waveform-similarity
 * overlap-add (Verhelst & Roelands 1993) with a fixed synthesis hop, on the GPU between the vocoder and the sink, all stretchers of a push
 * in one launch.  S = 1000 is "no stage": no launch, the same bytes as before (the stretcher is not the identity there, so 1000 bypasses it).
 * Constants at 24 kHz: frame N = 720, synthesis hop Hs = 360, search tolerance D = 240 (2 D + 1 = 481 lags).  Window w[i] = 0.5 - 0.5 cos(2 pi i
 * / N), formed in double and rounded to float (w[i] + w[i + Hs] = 1).  Positions are 64-bit integers: a_m = floor(m Hs S / 1000); the chosen
 * segment start p_m = a_m + delta_m with delta_m in [-D, D]; p_{-1} = -Hs; x[k] = 0 for k < 0 and, once the stretcher is finished with n
 * samples, for k >= n.  Frame m >= 0: template t[i] = x[p_{m-1} + Hs + i], 0 <= i < N; for each lag c(delta) = (s0 + s1) + (s2 + s3) with
 * s_q = sum of t[i] x[a_m + delta + i] over i = q (mod 4), i ascending, every product and add rounded to fp32, unfused; delta_m is the lag
 * with the largest c, the smallest delta among equals; y[m Hs + i] = (w[Hs + i] t[i]) + (w[i] x[p_m + i]) for 0 <= i < Hs: two fp32 products
 * and one fp32 add.  So the output is a function of the input and S alone: never of how the audio was cut into pushes or of which
 * stretchers shared a launch.
 * Frame m is ready after R received samples when need(m) <= R, need(m) = max(a_m + D + N, a_{m-1} + D + Hs + N) (second term for m >= 1):
 * integers only, independent of every delta.  Unfinished, a stretcher has emitted E(R) = Hs #{m : need(m) <= R}; finished with n samples,
 * T = ceil(1000 n / S): ceil(T / Hs) frames, the last block cut to T.  A push delivers E(after) - E(before).  Latency: at most N + D + Hs
 * input samples (55 ms).  The stretcher carries its input from a_{F-1} - D on (F: the next frame; fewer than 2 D + N + 2 Hs = 1920 floats),
 * p_{F-1} and the frame counter, in two alternating buffers of its own.
 * Known limit: a primed stream's stretcher (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts from
 * silence, x[k] = 0 for k < 0, like its sink: the first frame's template is zero, not the prefix's last samples. */
/* Host only, no engine.  Outputs a stretcher at speed_permille has emitted in all after n_received samples (finished != 0: the whole
 * clip's ceil(1000 n / S)).  -1 for a speed outside 500 .. 2000 or n_received < 0; q3tts_speed_last_error() then names the value
 * (thread-local, valid until the thread's next speed_emitted / speed_window call).  1000 is answered by the same rule. */
int64_t q3tts_speed_emitted(int32_t speed_permille, int64_t n_received, int finished);
const char* q3tts_speed_last_error(void);
/* Host only: the window the device uses, 720 floats; -1 when table is NULL or cap < 720. */
int q3tts_speed_window(float* table, int64_t cap);
/* Stretchers on their own: the stage by itself, fed 24 kHz float from the host.  A stretcher accepts at most one hour of input
 * (86 400 000 samples), a push at most 1 440 000.  At most 4096 stretchers are open at a time (vocoder streams' included).  1000 is
 * refused: it is no stage. */
int q3tts_speed_begin(q3tts_engine* e, int32_t speed_permille, int* id);
/* n stretchers (distinct, open, not finished), stretcher i given n_in[i] >= 0 more samples pcm24[i]; finish[i] != 0 (finish NULL: none)
 * flushes the tail with this push and closes the stretcher's audio (n_in[i] == 0 allowed).  out[i] has room for cap_samples floats;
 * out_len[i] is the push's length by the rule above (min(out_len, cap_samples) samples are written).  offsets_out (NULL ok) and
 * offsets_out[i] (NULL ok): room for cap_samples / 360 + 1 offsets, receives the delta of every frame the push completed; n_offsets[i]
 * (NULL ok): how many those are.  The call is validated completely before any stretcher moves.  n_in[i] == 0 without finish leaves the
 * stretcher as it was; a push that completes no frame still updates the carry. */
int q3tts_speed_push_batch_host(q3tts_engine* e, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len,
                                int32_t* const* offsets_out, int64_t* n_offsets);
int q3tts_speed_end(q3tts_engine* e, int id);
/* Vocoder streams.  A stream delivers time-stretched from its first sample on: refused, by name, once the stream has delivered a
 * sample.  1000 takes the stage away again.  q3tts_codec_stream_push_batch_any_host serves such streams: the stretcher runs on the
 * push's PCM where it lies, and its output feeds the stream's sink in the same push when it has one (the sink's input length is the
 * stretcher's push length); finish[s] flushes the stretcher first, then the sink, and is allowed on a stream with a speed and no
 * sink.  The float entries refuse a stream with a speed by name, as they refuse one with a sink. */
int q3tts_codec_stream_set_speed(q3tts_engine* e, int stream_id, int32_t speed_permille);
/* The scheduler: one setter for the four streaming entries, beside q3tts_engine_set_sink.  With a sink set, delivery goes through
 * the sink's callback in the sink's format; without one, through the entry's own float callback (a non-NULL pcm_out then receives the
 * stretched audio).  The finished = 1 call carries the flushed tail, so an utterance's calls add up to ceil(1000 n24 / S) samples at
 * 24 kHz.  Codes, frame counts and RNG use are untouched.  1000: none. */
int q3tts_engine_set_speed(q3tts_engine* e, int32_t speed_permille);

/* ---- output level: carried-state gain and look-ahead limiter ([HINT] no counterpart in the reference, which has no volume control; its
 * dead wav_writer.cpp peak-normalises a whole clip, which a streaming engine cannot do) ----
 * A third stage at 24 kHz between the stretcher and the sink: vocoder -> stretcher -> level -> sink, on the GPU, all stages of a push in
 * one launch.  Parameters: gain_cb, integer centibels, -600 .. +400; ceiling_permille, 0 = gain only, 1 .. 1000 = limiter at
 * T = (float)(ceiling / 1000.0).  (0, 0) is "no stage": no launch, the same bytes as before.
 * Gain: g = 10^(gain_cb / 200), formed in double and rounded to float (q3tts_level_gain returns the very value the device uses).
 * Gain only (ceiling 0): y[k] = g x[k], one fp32 product; no latency, E(R) = R.
 * Limiter, look-ahead window W = 128 samples (5.3 ms):
 *   1. v[k] = g x[k], a[k] = |v[k]|;
 *   2. r[k] = (a[k] > T) ? T / a[k] : 1.0f, a correctly rounded fp32 division;
 *   3. r[k] = 1 for k < 0 and, once the stage is finished with n samples, for k >= n;
 *   4. m[k] = min(r[k], .., r[k + 127]);
 *   5. q[k] = (int32)floor(m[k] * 65536.0f), in [0, 65536];
 *   6. S[k] = q[k] + q[k - 1] + .. + q[k - 127], an integer <= 2^23, exact in any order;
 *   7. s[k] = (float)S[k] * 2^-23, exact;
 *   8. y[k] = min(max(v[k] * s[k], -T), T): one fp32 product, then the clamp.
 * Every fp32 operation is a single rounded operation and the minimum and the integer sum are order-free, so a sample's bits depend on
 * its absolute index, the input and the parameters alone: never on how the audio was cut into pushes, on which stages shared a launch
 * or on how the kernel tiles its work.  Every q in S[k] comes from a window that contains k, so s[k] <= r[k] and |y[k]| <= T; where no
 * sample within +-127 of k exceeds T, s[k] = 1 exactly and y[k] = v[k] bit for bit.
 * A limiter that has received R samples and is not finished has emitted E(R) = max(0, R - 127) outputs; finished with n samples, n.  A
 * push delivers E(after) - E(before).  It carries the last 254 values of v in two alternating buffers of its own, and its counters.
 * Non-finite input: the formulas apply as written.
 * Known limits: a primed stream's level stage (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts from
 * r = 1 history, like its sink and its stretcher start from silence; the sink's band-limited resampling behind the limiter can
 * overshoot T slightly, and the int16 conversion's clip stays behind it. */
/* Host only, no engine.  g for gain_cb; -1.0f for a gain outside -600 .. +400 (q3tts_level_last_error() then names the value;
 * thread-local, valid until the thread's next level_gain / level_emitted call). */
float q3tts_level_gain(int32_t gain_cb);
/* Host only: outputs a stage with these parameters has emitted in all after n_received samples.  -1 for parameters out of range or
 * n_received < 0.  (0, 0) is answered by the same rule. */
int64_t q3tts_level_emitted(int32_t gain_cb, int32_t ceiling_permille, int64_t n_received, int finished);
const char* q3tts_level_last_error(void);
/* Level stages on their own: the stage by itself, fed 24 kHz float from the host.  A stage accepts at most one hour of input
 * (86 400 000 samples), a push at most 1 440 000.  At most 4096 stages are open at a time (vocoder streams' included).  (0, 0) is
 * refused: it is no stage. */
int q3tts_level_begin(q3tts_engine* e, int32_t gain_cb, int32_t ceiling_permille, int* id);
/* n stages (distinct, open, not finished), stage i given n_in[i] >= 0 more samples pcm24[i]; finish[i] != 0 (finish NULL: none) flushes
 * the tail with this push and closes the stage's audio (n_in[i] == 0 allowed).  out[i] has room for cap_samples floats; out_len[i] is
 * the push's length by the rule above (min(out_len, cap_samples) samples are written).  The call is validated completely before any
 * stage moves.  n_in[i] == 0 without finish leaves the stage as it was; a push that emits nothing still updates the carry. */
int q3tts_level_push_batch_host(q3tts_engine* e, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len);
int q3tts_level_end(q3tts_engine* e, int id);
/* Vocoder streams.  A stream delivers through a level stage from its first sample on: refused, by name, once the stream has delivered
 * a sample.  (0, 0) takes the stage away again.  q3tts_codec_stream_push_batch_any_host serves such streams: the stage reads the push's
 * PCM (or its stretcher's output) where it lies and feeds the stream's sink in the same push when it has one; finish[s] flushes the
 * stretcher, then the level stage, then the sink, and is allowed on a stream with a level stage and no sink.  The float entries refuse
 * a stream with a level stage by name. */
int q3tts_codec_stream_set_level(q3tts_engine* e, int stream_id, int32_t gain_cb, int32_t ceiling_permille);
/* The scheduler: one setter for the four streaming entries, beside q3tts_engine_set_sink / q3tts_engine_set_speed.  The finished = 1
 * call carries the limiter's tail, so an utterance's calls add up to the length they have without the stage.  Codes, frame counts
 * and RNG use are untouched.  (0, 0): none. */
int q3tts_engine_set_level(q3tts_engine* e, int32_t gain_cb, int32_t ceiling_permille);

/* ---- pitch: carried-state TD-PSOLA shift of the fundamental ([HINT] no counterpart in the reference, which has no pitch control;
 * DESIGN.md 4o) ----
 * The FIRST stage behind the vocoder at 24 kHz: vocoder -> pitch -> stretcher -> level -> sink, on the GPU, all stages of a push in one
 * launch.  It delivers the same audio at the same length with the fundamental multiplied by r / 1000 and the spectral envelope left
 * where it is (time-domain pitch-synchronous overlap-add; Moulines & Charpentier 1990).  r: integer permille, 500 .. 2000.  1000 is "no
 * stage": no launch, the same bytes as before.
 * Constants: Pmin = 48, Pmax = 400, Pu = 120, W = 240; VOICED2 = 0.25f, OCTAVE2 = 0.81f (squared correlations 0.5 and 0.9);
 * FLOOR = 0.0625f; synthesis positions carry F = 20 fraction bits.  x[k] = 0 for k < 0 and, once the stage is finished with n
 * samples, for k >= n.
 * Analysis marks: a_0 = 0, a_{j+1} = a_j + P_j.  Mark j is searched when a_j >= W and a_j + W + Pmax + 1 <= n (while the stage is not
 * finished a mark is only looked at once that much has arrived); otherwise it is unvoiced.  The search, with t[i] = x[a_j - W + i],
 * i = 0 .. 479, for every lag L = 47 .. 401:
 *   num(L) = (s0 + s1) + (s2 + s3), s_q the fp32 sum of t[i] * x[a_j - W + L + i] over i = q mod 4 ascending (product rounded, then added);
 *   E_lag(L) likewise of x[a_j - W + L + i]^2, E_t likewise of t[i]^2;  den = E_t * E_lag;
 *   score(L) = den > 0 ? (num * |num|) / den : 0, a correctly rounded fp32 division.
 * A candidate is a lag 48 .. 400 with score(L) >= score(L - 1) and score(L) >= score(L + 1).  best = the largest candidate score
 * (no candidate: unvoiced).  The mark is voiced when best >= VOICED2; then P_j = the SMALLEST candidate with score >= OCTAVE2 * best
 * (one fp32 product).  An unvoiced mark has P_j = Pu.  Mark 0 is unvoiced (a_0 < W).
 * Synthesis marks: s_0 = 0 in 64-bit fixed point, t_i = s_i >> F.  Mark i takes the analysis mark j nearest to t_i, the later of two
 * equally near, and s_{i+1} = s_i + ((P_j * 1000) << F) / r (integer division) when that mark is voiced, s_i + (P_j << F) when not.
 * Marks are placed for t_i < n + Pmax.
 * Grains: mark i adds, for m = 0 .. 2 P_j - 1 and k = t_i - P_j + m >= 0, acc[k] = acc[k] + h[m] * x[a_j - P_j + m] (product rounded,
 * then added) and wsum[k] = wsum[k] + h[m], with h[m] = (float)(0.5 - 0.5 cos(pi m / P_j)) formed in double (a table per P, built on
 * the host).  Grains are added in mark order.  y[k] = acc[k] / (wsum[k] > FLOOR ? wsum[k] : FLOOR) for 0 <= k < n.
 * Every fp32 operation is a single rounded operation in a fixed order, so a sample's bits depend on the input, r and its absolute index
 * alone: never on how the audio was cut into pushes or on which stages shared a launch.  Unvoiced audio (every mark at hop Pu, windows
 * summing to 1) comes out as it went in up to the rounding of sum(h x) / sum(h).
 * Host rule: a synthesis mark at t is placed once t + GATE samples have arrived, GATE = Pmax / 2 + W + Pmax + 1 = 841 (its analysis mark
 * lies at most Pmax / 2 behind t and is searched over W + Pmax + 1 samples); output k is final once every mark up to k + Pmax is placed.
 * So a stage that has received R samples and is not finished has emitted E(R) = max(0, R - LA), LA = Pmax + GATE - 1 = 1240 (51.7 ms);
 * finished with n samples, n.  A push delivers E(after) - E(before).  The stage carries its last 2 560 input samples, the 1 024
 * entries of acc and wsum beyond the last emitted sample and eight words of mark state in two alternating halves of its own.
 * Non-finite input: the formulas apply as written (a comparison with a NaN is false); periods and indices stay in their ranges.
 * Known limits: a primed stream's pitch stage (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts from
 * silence, like the other stages.  VOICED2 and OCTAVE2 are untuned on real voices. */
/* Host only, no engine.  round(1000 * 2^(cents / 1200)) in double; -1 for cents outside -1200 .. +1200 or not finite
 * (q3tts_pitch_last_error() then says so; thread-local, valid until the thread's next pitch_ratio / pitch_emitted call). */
int32_t q3tts_pitch_ratio(double cents);
/* Host only: outputs a stage has emitted in all after n_received samples (the rule does not depend on r).  -1 for n_received < 0. */
int64_t q3tts_pitch_emitted(int64_t n_received, int finished);
const char* q3tts_pitch_last_error(void);
/* Pitch stages on their own: the stage by itself, fed 24 kHz float from the host.  A stage accepts at most one hour of input
 * (86 400 000 samples), a push at most 1 440 000.  At most 4096 stages are open at a time (vocoder streams' included).  1000 is
 * refused: it is no stage. */
int q3tts_pitch_begin(q3tts_engine* e, int32_t ratio_permille, int* id);
/* As q3tts_level_push_batch_host: n stages (distinct, open, not finished), validated completely before any stage moves. */
int q3tts_pitch_push_batch_host(q3tts_engine* e, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len);
int q3tts_pitch_end(q3tts_engine* e, int id);
/* Vocoder streams.  A stream delivers through a pitch stage from its first sample on: refused, by name, once the stream has delivered
 * a sample.  1000 takes the stage away again.  q3tts_codec_stream_push_batch_any_host serves such streams: the stage reads the push's
 * PCM where it lies and feeds the stream's later stages in the same push; finish[s] flushes pitch, stretcher, level, sink in that
 * order and is allowed on a stream with a pitch stage and no sink.  The float entries refuse a stream with a pitch stage by name. */
int q3tts_codec_stream_set_pitch(q3tts_engine* e, int stream_id, int32_t ratio_permille);
/* The scheduler: one setter for the four streaming entries, beside q3tts_engine_set_sink / _speed / _level.  The finished = 1 call
 * carries the stage's tail, so an utterance's calls add up to the length they have without the stage.  Codes, frame counts and RNG
 * use are untouched.  1000: none. */
int q3tts_engine_set_pitch(q3tts_engine* e, int32_t ratio_permille);

/* ---- loudness: carried-state BS.1770 meter and normaliser ([HINT] no counterpart in the reference, whose wav_writer.cpp peak
 * normalisation is dead code and needs the whole clip) ----
 * A stage between the stretcher and the level stage at 24 kHz: vocoder -> pitch -> stretcher -> loudness -> level -> sink, on the GPU,
 * all stages of a push in one launch.  It measures programme loudness as ITU-R BS.1770-4 does and, given a target, moves a gain towards
 * it by at most 1 dB per 100 ms; a boost is caught by the limiter behind it.
 * Parameters: target_dlufs, the target in tenths of a LUFS, -400 .. -50, or 0: meter only.  range_cb, the largest boost or cut in
 * centibels, 0 .. 400; R = 10^(range_cb / 200).  start_cb, the gain before anything is measured, -400 .. 400;
 * G_-1 = (float)10^(start_cb / 200) (a caller that served this voice before passes the last gain it was told).  There is no "no stage"
 * value: not setting the stage is "no stage".  (0, ., .) is meter only: y[k] = x[k] bit for bit, E(R) = R, no latency, and the
 * measurement is still produced (its G_b stay G_-1).
 * 1. K-weighting at fs = 24 000, in double: two biquads re-derived from BS.1770's analogue prototype by the bilinear transform.
 *    Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *    Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b = ((Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0),
 *    a = (2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0).  High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = (1, -2, 1), a as
 *    above with this K and Q.  At 48 000 the formulas give the BS.1770-4 table to 9e-16.
 * 2. Recursion: x[k] widened exactly to double; ff = (b0 x[k] + b1 x[k-1]) + b2 x[k-2], u[k] = (ff - a2 u[k-2]) - a1 u[k-1], every
 *    operation one rounded fp64 operation in this order; the second biquad has the same shape on u and gives v.  History is zero before
 *    sample 0.  The library is built with -ffp-contract=off, so these are the host's IEEE operations.
 * 3. Energy: z = v[k] v[k], q[k] = (int64)floor((z < 4.0 ? z : 4.0) 2^32).  Sub-block b covers samples [2400 b, 2400 b + 2400);
 *    E_b = sum of its q: an integer sum, exact in any order, below 2^46.
 * 4. Gate: for b >= 3, W_b = E_{b-3} + E_{b-2} + E_{b-1} + E_b, the standard's 400 ms block at 75 % overlap.  W_b counts when
 *    W_b >= 4834272 = floor(9600 2^32 10^((-70 + 0.691) / 10)).  A = the sum of the counted W, N their number (A stays below 2^63 over
 *    the one hour a stage accepts).  The -10 LU relative gate is not applied on the device; q3tts_loudness_lufs applies it.
 * 5. Gain after sub-block b: N = 0 or meter only: T = G_{b-1}.  Otherwise P = (double)A / ((double)N 41231686041600.0),
 *    d = sqrt(PT / P) with PT = 10^((target_dlufs / 10 + 0.691) / 10) formed once on the host, d clamped to [1 / R, R] in double (1 / R
 *    one division on the host), T = (float)d.  Slew, 1 dB per sub-block: G_b = min(max(T, G_{b-1} DN), G_{b-1} UP),
 *    UP = (float)10^(1/20), DN = (float)10^(-1/20), fp32 products.  Division, sqrt and int -> double are correctly rounded.
 * 6. Output: for k in sub-block b, i = k - 2400 b: y[k] = x[k] (G_{b-1} + (G_b - G_{b-1}) ((float)i / 2400.0f)), each operation one
 *    rounded fp32 operation.  Samples of a final partial sub-block: y[k] = x[k] G of the last complete one, unramped.
 * 7. Host rule: a stage that has received R samples and is not finished has emitted E(R) = 2400 floor(R / 2400); finished with n
 *    samples, n.  A push delivers E(after) - E(before).  The latency is 100 ms: what a causal measurement costs.
 * 8. Carry, in two alternating halves: six doubles of filter history; E of the last three sub-blocks and the running sum of the open
 *    one; A, N and G; the fewer than 2400 input samples not yet emitted.
 * So samples, energies and gains depend on the input and the parameters alone: never on how the audio was cut into pushes or on which
 * stages shared a launch.  Non-finite input: the formulas apply as written (z < 4.0 is false for a NaN, so its q is 4 2^32).
 * Known limits: a primed stream's loudness stage (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts
 * from zero history and start_cb, like the other stages start from silence. */
#define Q3TTS_LOUDNESS_MOMENTARY 0   /* the last window of four sub-blocks (400 ms) */
#define Q3TTS_LOUDNESS_SHORT_TERM 1  /* the last thirty sub-blocks (3 s) */
#define Q3TTS_LOUDNESS_INTEGRATED 2  /* BS.1770: windows of four, the absolute gate (W >= 4834272), then the relative gate 10 LU below their mean */
/* Host only, no engine.  The ten doubles { b0, b1, b2, a1, a2 } of the shelf, then of the high-pass, by the formulas above at `rate`
 * (8000 .. 384000); at 24 000 the very doubles the device uses.  -1 outside the range (q3tts_loudness_last_error() then says so;
 * thread-local, valid until the thread's next loudness_coeffs / _emitted / _lufs call). */
int q3tts_loudness_coeffs(int32_t rate, double out[10]);
/* Host only: outputs a stage has emitted in all after n_received samples (of the parameters only target_dlufs == 0 matters).  -1 for
 * n_received < 0 or a target out of range, which the message names. */
int64_t q3tts_loudness_emitted(int32_t target_dlufs, int64_t n_received, int finished);
/* Host only: LUFS of n sub-block energies E_b as a push reports them, -0.691 + 10 log10(mean square).  -inf when the span has not
 * arrived yet or nothing passes the gates; NaN for a bad argument (q3tts_loudness_last_error()). */
double q3tts_loudness_lufs(const int64_t* E, int64_t n, int mode);
const char* q3tts_loudness_last_error(void);
/* Loudness stages on their own: the stage by itself, fed 24 kHz float from the host.  A stage accepts at most one hour of input
 * (86 400 000 samples), a push at most 1 440 000.  At most 4096 stages are open at a time (vocoder streams' included).  A value out of
 * range is refused with the value named. */
int q3tts_loudness_begin(q3tts_engine* e, int32_t target_dlufs, int32_t range_cb, int32_t start_cb, int* id);
/* As q3tts_level_push_batch_host: n stages (distinct, open, not finished), validated completely before any stage moves.  Optional
 * report (as the stretcher's offsets_out): energies_out[i] and gains_out[i] (either NULL ok; n_in[i] / 2400 + 1 entries each) receive
 * E_b and G_b of the sub-blocks push i completed, n_blocks[i] (NULL ok) their number. */
int q3tts_loudness_push_batch_host(q3tts_engine* e, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                                   const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len,
                                   int64_t* const* energies_out, float* const* gains_out, int64_t* n_blocks);
int q3tts_loudness_end(q3tts_engine* e, int id);
/* Vocoder streams.  A stream delivers through a loudness stage from its first sample on: refused, by name, once the stream has
 * delivered a sample.  q3tts_codec_stream_push_batch_any_host serves such streams: the stage reads its input where the stage in front
 * left it and feeds the stream's later stages in the same push; finish[s] flushes pitch, stretcher, loudness, level, sink in that order
 * and is allowed on a stream with a loudness stage and no sink.  The float entries refuse a stream with a loudness stage by name. */
int q3tts_codec_stream_set_loudness(q3tts_engine* e, int stream_id, int32_t target_dlufs, int32_t range_cb, int32_t start_cb);
/* The scheduler: one setter for the four streaming entries, beside q3tts_engine_set_sink / _speed / _level / _pitch.  enabled 0 takes
 * the stage away (the other arguments are not looked at).  The finished = 1 call carries the stage's tail, so an utterance's calls add
 * up to the length they have without the stage.  Codes, frame counts and RNG use are untouched; the callback's signature stays. */
int q3tts_engine_set_loudness(q3tts_engine* e, int enabled, int32_t target_dlufs, int32_t range_cb, int32_t start_cb);

/* ---- tone: carried-state parametric equaliser ([HINT] no counterpart in the reference, which has no equaliser) ----
 * A stage between the stretcher and the loudness stage at 24 kHz, so that the meter measures what is heard and the limiter stands
 * behind anything that can boost.  With it the order of the six stages is
 *   vocoder -> pitch -> stretcher -> tone -> loudness -> level -> sink
 * on the GPU, all tone stages of a push in one launch.  A stage is a cascade of n = 1 .. 8 biquad sections, each one of
 * { kind, freq_hz, gain_cb, q_permille }: kind high-pass, low-pass, low shelf, high shelf or peak; freq_hz 20 .. 11000; gain_cb
 * -240 .. +240 in 0.1 dB steps (must be 0 for a high- or low-pass); q_permille 100 .. 10000 (Q 0.1 .. 10).  There is no "no stage"
 * value: no sections is no stage, no launch, and the bytes delivered without one.  A value out of range is refused with the field,
 * the section's index and the value named.
 * 1. Coefficients, in double on the host, the RBJ Audio-EQ-Cookbook forms: w0 = 2 pi freq_hz / 24000, c = cos(w0),
 *    alpha = sin(w0) / (2 Q), Q = q_permille / 1000, A = 10^(gain_dB / 40) = 10^(gain_cb / 400).
 *    High-pass: b = ((1 + c) / 2, -(1 + c), (1 + c) / 2), a = (1 + alpha, -2 c, 1 - alpha).
 *    Low-pass:  b = ((1 - c) / 2, 1 - c, (1 - c) / 2), a as the high-pass's.
 *    Peak:      b = (1 + alpha A, -2 c, 1 - alpha A), a = (1 + alpha / A, -2 c, 1 - alpha / A).
 *    Shelves, with s = 2 sqrt(A) alpha, p = A + 1, m = A - 1:
 *    low shelf  b = (A ((p - m c) + s), 2 A (m - p c), A ((p - m c) - s)), a = ((p + m c) + s, -2 (m + p c), (p + m c) - s);
 *    high shelf b = (A ((p + m c) + s), -2 A (m + p c), A ((p + m c) - s)), a = ((p - m c) + s, 2 (m - p c), (p - m c) - s).
 *    Each of b0 b1 b2 a1 a2 is divided by a0.  q3tts_tone_coeffs returns the very doubles the device uses; a restatement takes them
 *    from there, so that nothing rests on two maths libraries agreeing in the last bit.
 * 2. Recursion, the loudness stage's biquad repeated: s_0[k] = (double)x[k]; for section j = 1 .. n:
 *    ff = (b0 s_{j-1}[k] + b1 s_{j-1}[k-1]) + b2 s_{j-1}[k-2], s_j[k] = (ff - a2 s_j[k-2]) - a1 s_j[k-1]; y[k] = (float)s_n[k].
 *    Every operation is one rounded IEEE fp64 operation in this order (the library is built with -ffp-contract=off); nothing is rounded
 *    to float between sections; all history is zero before sample 0; subnormals are kept (gradual underflow) in the fp64 arithmetic and
 *    in the final conversion, which rounds to nearest even.
 * 3. Host rule: a stage that has received N samples has emitted N.  No latency, no look-ahead; finish flushes nothing, and a push of 0
 *    samples with finish is allowed.
 * 4. Carry, in two alternating halves: two doubles per signal s_0 .. s_n, (n + 1) * 2 in all.
 * So a sample's bits depend on its absolute index, the input and the sections alone: never on how the audio was cut into pushes or on
 * which stages shared a launch.  Non-finite input: the formulas apply as written (a NaN stays in the history).
 * Known limits: a primed stream's tone stage (q3tts_codec_stream_prime_batch_host, q3tts_synthesize_continue_stream_host) starts from
 * zero history, like the other stages start from silence.  The sections of a stage cannot change while it runs. */
#define Q3TTS_TONE_HIGHPASS 1
#define Q3TTS_TONE_LOWPASS 2
#define Q3TTS_TONE_LOWSHELF 3
#define Q3TTS_TONE_HIGHSHELF 4
#define Q3TTS_TONE_PEAK 5
#define Q3TTS_TONE_MAX_SECTIONS 8
typedef struct { int32_t kind, freq_hz, gain_cb, q_permille; } q3tts_tone_section;
/* Host only, no engine.  out[j] = { b0, b1, b2, a1, a2 } of section j by the formulas above.  -1 for n outside 1 .. 8 or a value out
 * of range (q3tts_tone_last_error() then names it; thread-local, valid until the thread's next tone_coeffs / tone_parse call). */
int q3tts_tone_coeffs(int32_t n, const q3tts_tone_section* sections, double (*out)[5]);
/* Host only: the sections of a spec string, at most 8 into out, their number into *n.  A spec is a preset's name (telephone, rumble,
 * presence, warm) or sections separated by commas, kind:Hz:Q for hp and lp, kind:Hz:dB:Q for ls, hs and peak, as in
 * "hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707".  dB is rounded to 0.1, Q to 0.001.  -1 for what it cannot read or what is out of range
 * (q3tts_tone_last_error()).  The presets are unheard and untuned: no checkpoint exists yet. */
int q3tts_tone_parse(const char* spec, q3tts_tone_section* out, int32_t* n);
const char* q3tts_tone_last_error(void);
/* Tone stages on their own: the stage by itself, fed 24 kHz float from the host.  A stage accepts at most one hour of input
 * (86 400 000 samples), a push at most 1 440 000.  At most 4096 stages are open at a time (vocoder streams' included). */
int q3tts_tone_begin(q3tts_engine* e, int32_t n, const q3tts_tone_section* sections, int* id);
/* As q3tts_level_push_batch_host: n stages (distinct, open, not finished), validated completely before any stage moves; out_len[i]
 * is n_in[i]. */
int q3tts_tone_push_batch_host(q3tts_engine* e, int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in,
                               const uint8_t* finish, float* const* out, int64_t cap_samples, int64_t* out_len);
int q3tts_tone_end(q3tts_engine* e, int id);
/* Vocoder streams.  A stream delivers through a tone stage from its first sample on: refused, by name, once the stream has delivered
 * a sample.  n = 0 takes the stage away again.  q3tts_codec_stream_push_batch_any_host serves such streams: the stage reads its input
 * where the stage in front left it and feeds the stream's later stages in the same push; finish[s] is allowed on a stream with a tone
 * stage and no sink.  The float entries refuse a stream with a tone stage by name. */
int q3tts_codec_stream_set_tone(q3tts_engine* e, int stream_id, int32_t n, const q3tts_tone_section* sections);
/* The scheduler: one setter for the four streaming entries, beside q3tts_engine_set_sink / _speed / _level / _pitch / _loudness.
 * n = 0 takes the stage away.  Lengths, codes, frame counts and RNG use are untouched; the callback's signature stays. */
int q3tts_engine_set_tone(q3tts_engine* e, int32_t n, const q3tts_tone_section* sections);

/* ---- text front end: the reference's byte-level BPE tokenizer ---- */
/* Replaces leaxer_qwen::io::load_vocab / load_merges / is_tokenizer_ready / tokenize (reference
 * src/io/tokenizer.h:13-22, src/io/tokenizer.cpp:538-561) with the same ids for the same files and text.
 * The reference keeps one process-global tokenizer; here it is a handle (host-only, no GPU work).
 * load_* return 0 on success, -1 on failure (the reference's `false`).  q3tts_tokenize writes up to
 * `cap` ids and returns the number of ids the text produces (call with cap=0 to size the buffer). */
typedef struct q3tts_tokenizer q3tts_tokenizer;
q3tts_tokenizer* q3tts_tokenizer_create(void);
void q3tts_tokenizer_destroy(q3tts_tokenizer* t);
int q3tts_tokenizer_load_vocab(q3tts_tokenizer* t, const char* vocab_json_path);
int q3tts_tokenizer_load_merges(q3tts_tokenizer* t, const char* merges_txt_path);
int q3tts_tokenizer_ready(const q3tts_tokenizer* t);
int64_t q3tts_tokenize(const q3tts_tokenizer* t, const char* text, int64_t len, int32_t* ids, int64_t cap);

/* ---- measurement hooks (bench.py) ---- */
/* device time in ms of the last q3tts_decode_steps call, from HIP events on the engine's stream */
int q3tts_last_decode_ms(q3tts_engine* e, float* ms, int* steps);
/* device time in ms of the last q3tts_audio_encode_* or q3tts_audio_stream_push_* call (uploads and launches of all its groups, HIP events on the engine's stream) */
int q3tts_last_audio_encode_ms(q3tts_engine* e, float* ms);
/* device time in ms of the last codec decode */
int q3tts_last_codec_ms(q3tts_engine* e, float* ms);
/* accumulated device time since the last reset: decode steps (HIP events around the graph
 * replays, on the engine's stream) and codec decodes */
int q3tts_counters(q3tts_engine* e, double* decode_ms, int64_t* decode_steps, double* codec_ms, int64_t* codec_frames, int reset);
/* Codec decoder (run_vocoder's graph, /root/reference/src/tts_onnx.cpp:759-776): how many of its conv / linear weight tensors are exact
 * in fp16 after the power-of-two pre-scale (every bf16- or fp16-origin tensor) and therefore run two matrix-core products per fp32
 * product, and how many keep a non-zero lo plane and run three.  Both 0 under Q3TTS_FLAG_FP32_CODEC. */
int q3tts_codec_plane_stats(q3tts_engine* e, int* two_product, int* three_product);
/* Per-stage device time of the decode step: runs n_steps EAGER steps of the armed slots (they advance like q3tts_decode_steps) with HIP
 * events at the stage boundaries.  out_ms[0] sampler (n_groups launches), [1] code predictor (layer passes + heads; predict_subcodes,
 * tts_onnx.cpp:851-872), [2] talker decode (layers + codec head; run_decode :667-732), [3] their sum — milliseconds per step. */
int q3tts_stage_profile(q3tts_engine* e, int n_steps, double* out_ms /* [4] */);
/* Device time of the prefill stage (run_prefill, tts_onnx.cpp:615-665): `reps` batched prefill passes of slots 0..n_slots-1 (all free)
 * over n_rows synthetic prompt rows each, already in HBM — the launches a job's equal-length prompts take (groups of up to 128 rows
 * share one pass over the talker's weights) — with HIP events around each pass; *ms_per_pass = mean device milliseconds.  The slots
 * are released again.  bench.py's stages.prefill.  n_slots == 1 also takes n_rows up to max_ctx: the chunked long-prompt prefill
 * (tools/prefill_long_bench.py). */
int q3tts_prefill_profile(q3tts_engine* e, int n_slots, int n_rows, int reps, double* ms_per_pass);
/* Measurement aid (engines created with Q3TTS_FLAG_TEST_HOOKS only): every armed slot jumps n_frames ahead without generating them — frame
 * counters and talker positions advance, the skipped frames' codes are zero and the talker's KV cache is refilled with seeded synthetic rows.
 * What the slots emit afterwards is numerically meaningless; the decode step streams a context of the requested depth, which is what the
 * rocprofv3 passes over run_decode's attention (tts_onnx.cpp:667-732) at 1000-2000 tokens of context need (tools/ctx_bench.py). */
int q3tts_measure_skip_frames(q3tts_engine* e, int n_frames);
/* Test hook (engines created with Q3TTS_FLAG_TEST_HOOKS only): fills the vocoder's reusable workspace (lane arenas, batched-front arena,
 * streaming arena, pinned PCM staging, the job's code rows) with 0xFF bytes = NaN, so that a later decode which reads anything it did
 * not write itself produces NaN instead of plausible stale samples (tests/test_gpu_codec_stress.py).  The audio encoder's grow-only
 * workspace is filled the same way: an encoder stream's state (rings, resampler carry) lives outside it and must not notice. */
int q3tts_test_poison_workspace(q3tts_engine* e);
/* Test hook (Q3TTS_FLAG_TEST_HOOKS engines): the last batched vocoder group's final conv as it lies in its lane's workspace — input rows
 * sx_out[nb][T][C] (cap_floats >= nb*T*C, else skipped) and output pcm_out[nb][T]; either may be NULL.  tools/vocoder_stress.py uses it to
 * tell a wrong input from a wrong conv when a job's PCM differs from the utterance's own decode. */
/* ... and, when the A/B knob Q3TTS_COUT1_PACKED=2 selected the dumping variant of that conv, the per-row per-tap partial sums each tile's
 * output phase read from LDS: out[tile][256][8]; returns the float count (call with out == NULL to size). */
int64_t q3tts_test_final_conv_partials(q3tts_engine* e, float* out, int64_t cap_floats);
int q3tts_test_group_final_conv(q3tts_engine* e, float* sx_out, float* pcm_out, int64_t cap_floats, int32_t* T, int32_t* C, int32_t* nb);
/* Parity aid: ONE eager decode step of the armed slots (they advance like q3tts_decode_steps(1)) that also returns, for `slot`, the
 * logits row each of the frame's n_groups decisions was sampled from — out[n_groups][cols], cols >= max(vocab, sub_vocab); row 0 the
 * code0 logits (run_decode's output, before suppression), row j the code predictor's logits for sub-code j-1 (run_code_predictor,
 * tts_onnx.cpp:734-757).  Lets a test compare every head of the fused step with the oracle at a chosen frame. */
int q3tts_step_logits_host(q3tts_engine* e, int slot, float* out, int cols);
/* algorithmic bytes one decode step streams (weights + KV at the slots' current contexts) */
int q3tts_decode_step_bytes(q3tts_engine* e, double* weight_bytes, double* kv_bytes);

#ifdef __cplusplus
}
#endif
#endif
