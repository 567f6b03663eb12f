// q3_engine.h — the device-resident engine behind the C-ABI (include/q3tts.h).
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "q3_audio.h"
#include "q3_begin_plan.h"
#include "q3_codec_plan.h"
#include "q3_common.h"
#include "q3_kvpool.h"
#include "q3_stage.h"
#include "q3_weight_share.h"

namespace q3 {

enum TensorKind { TK_W = 0, TK_NORM = 1, TK_BIAS = 2, TK_SCALE = 3, TK_SNAKE = 4 };

struct Tensor {
    std::string name;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
    int kind = TK_W;
    bool bf16 = false;  // storage: bf16 for talker / predictor / text matrices, fp32 otherwise
    void* dev = nullptr; // may point into a fused parent allocation (qkv)
    int64_t numel = 0;
    float synth_std = 0.02f;
};

struct TensorSpec { // registry entry without storage
    std::string name;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0, kind = TK_W;
    bool bf16 = false;
    int fuse = 0;           // 1/2/3: q/k/v of a layer, allocated as one block
    float synth_std = 0.02f;
};
std::vector<TensorSpec> tensor_specs(const q3tts_config& c); // host-only
bool enc_config_ok(const q3tts_config& c);                   // the audio encoder's dims are ones the registry and the kernels cover

struct DecLayerW { // one decoder layer, bf16 matrices
    const float *in_norm = nullptr, *post_norm = nullptr, *q_norm = nullptr, *k_norm = nullptr;
    const bf16_t *qkv = nullptr, *o = nullptr, *gate = nullptr, *up = nullptr, *down = nullptr;
};
struct DecStack {
    int H = 0, L = 0, nq = 0, nkv = 0, d = 0, ffn = 0;
    float eps = 0.f;
    std::vector<DecLayerW> layers;
    float *kc = nullptr, *vc = nullptr; // paged cache (fp32, or bf16 behind the same pointers when kv_bf16)
    bool kv_bf16 = false, kv_round = false;
    int* page_table = nullptr;
    int pages_per_slot = 0, page_shift = 0;
    bool identity_pages = false;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    bool nt = false; // weights streamed once per step -> non-temporal loads
    int n_splits = 1, chunk = 1 << 30; // split-T attention
    int n_splits_stream = 0, chunk_stream = 0; // k_attn_stream's splits (batched step, long contexts): whole pages, 256 tokens by default
    float *po = nullptr, *pm = nullptr, *pl = nullptr; // attention partials [rows][nq][n_splits]([d])
};

struct CodecW; // q3_codec.cpp: the vocoder's run-time part (lanes, arenas, streams); reads its weights through CodecWeights
struct CodecWeights; // q3_codec.cpp: layer list, repacked convs, (hi, lo) planes and their chunk-major / fragment copies, SnakeBeta constants
struct SpeakerW; // q3_speaker.cpp: the speaker encoder's repacked convs (weights only)
struct SpkFront; // q3_speaker.cpp: the clone front end's workspace; its mel tables are the set's
struct EncoderW; // q3_encoder.cpp: the audio encoder's run-time part (RoPE tables, workspace, streams)
struct EncWeights; // q3_encoder.cpp: repacked convs, layer pointers, codebooks
void codec_weights_free(CodecWeights* w);
void speaker_weights_free(SpeakerW* w);
void encoder_weights_free(EncWeights* w);

// Everything that is a function of the checkpoint alone ("The weight set"): the registry and every copy finalize derives
// from it.  Immutable once published; engines created by q3tts_create_sharing hold the donor's set instead of a copy.  The last holder's
// destruction frees the HBM.  Nothing in it is sized by max_batch or max_ctx, and nothing in it is written while an engine runs, except
// the layer-0 QKV table, which the first holder it applies to adds once (ShareBook::build_once).
struct WeightSet : ShareBook {
    explicit WeightSet(int dev) : device(dev) {}
    ~WeightSet();
    WeightSet(const WeightSet&) = delete;
    WeightSet& operator=(const WeightSet&) = delete;
    int device;
    std::vector<Tensor> tensors;
    std::unordered_map<std::string, int> tindex;
    std::vector<void*> allocs;                 // the registry's storage, tts_pad / tts_eos, the speaker encoder's repacked convs
    bool ready = false;                        // Engine::finalized: the derived copies match the registry
    std::vector<std::pair<const bf16_t*, bf16_t*>> packed_w;   // fragment-packed bf16 copies, registered under their row-major pointers
    CodecWeights* codec = nullptr;
    SpeakerW* spk = nullptr;
    EncWeights* enc = nullptr;
    void* mel_tables_d = nullptr;              // the log-mel front end's tables (q3_speaker.cpp: front_finalize)
    float *tts_pad_d = nullptr, *tts_eos_d = nullptr;
    float* cp_qkv_tab = nullptr; int64_t cp_qkv_tab_bytes = 0;   // Engine::cp_qkv_tab
    void* dmalloc(size_t bytes);               // counted in bytes, freed with the set
    void* take(size_t bytes, int64_t& tally);  // a derived copy's allocation: counted in bytes and in the piece's own tally
    void drop(int64_t& tally) { add_bytes(-tally); tally = 0; }   // the piece was freed
    int64_t packed_bytes = 0, mel_bytes = 0;
    void free_packed();                        // the packed copies and the table (re-finalize, destruction)
};

class Engine {
public:
    // kv_pool_tokens: capacity of the talker's KV page pool in tokens (0: max_batch x max_ctx, every slot can reach max_ctx at once)
    // shared non-null: the engine holds that (published) set instead of allocating a registry, and comes up finalized (bind_shared)
    Engine(const q3tts_config& cfg, int device, int max_batch, int max_ctx, uint32_t flags, int64_t kv_pool_tokens = 0,
           std::shared_ptr<WeightSet> shared = nullptr);
    ~Engine();

    // ---- talker KV page pool: 64-token pages handed to slots on demand (page 0 is a scratch page every unowned table entry points at,
    // so masked rows of unarmed / released slots keep writing somewhere harmless).  Host-side free list; the device sees only the table.
    int kv_total_pages() const { return kv.total; }
    int kv_free_pages() const { return kv.free_count; }
    int kv_pages_for(int tokens) const { return kv.pages_for(tokens); }
    int kv_slot_pages(int slot) const { return kv.slot_pages(slot); }
    void kv_reserve(int slot, int tokens, bool exact);   // the slot owns pages for positions [0, tokens): grows (and with `exact` shrinks) to that
    void kv_upload_row(int slot);                        // after KvPool changed a slot's table row behind the engine's back (scheduler policy)
    void kv_release(int slot);

    KnobScope knob_scope;                      // first member: counts this engine among the hook-enabled ones until it is destroyed (also when the constructor throws)
    q3tts_config c;
    int device, B, max_ctx;
    KvPool kv;                                 // q3_kvpool.h: free list, per-slot pages, host mirror of talker.page_table
    int64_t sched_admitted = 0, sched_preempted = 0; int sched_peak_live = 0;   // the last scheduler call (q3tts_sched_stats)
    uint32_t flags;
    hipStream_t stream = nullptr;
    bool null_stream = false;
    std::string err;

    // ---- weights: the set's, through references, so that every reader keeps its spelling ----
    SetHold<WeightSet> hold;
    WeightSet& ws;
    std::vector<Tensor>& tensors;
    std::unordered_map<std::string, int>& tindex;
    bool& finalized;
    std::vector<void*> allocs;                 // this engine's own workspaces (nothing derived from the checkpoint)
    void check_unshared() const;               // set_tensor / fill_synthetic / load_weights: refused while another engine holds the set
    void bind_weights();                       // this engine's pointer views into the registry (DecStack layers, heads, embeddings)
    void bind_shared();                        // a sharer's construction: views + run-time parts on a published set, + the table if it is the first it applies to
    int64_t private_weight_bytes() const { return 0; }   // derived copies this engine owns outside the set: none
    Tensor& T(const std::string& n);
    void set_tensor(const std::string& name, const float* data, int64_t n);
    void get_tensor(const std::string& name, float* out, int64_t n);
    void fill_synthetic(uint64_t seed);
    void finalize();

    // ---- session-shaped ops (host I/O) ----
    void text_project(const int64_t* ids, int n, float* out);
    void codec_embed(const int64_t* ids, int n, float* out);
    void cp_embed(int64_t id, int step, float* out);
    void talker_prefill(int slot, const float* embeds, int S, float* logits, float* last_hidden);
    void prefill_rows_in_xp(int slot, int S);   // run_prefill's device work for the S rows in xp (shared by the host and the device-pointer entry)
    // ---- long prompts (S > 16: an instruction or any other long prefix in front of the reference's 8-10 rows) ----
    // The prompt is walked in chunks of prefill_chunk <= 128 rows: run_layers(nb = 1, n_new = chunk, pos_scalar = base) with
    // launch_attn_prefill in place of k_attn, in a 128-row workspace of its own (allocated by the first long prefill, freed with the
    // engine; rows_max and every short-prompt launch stay as they are).  x: the S prompt rows on the device, overwritten.  logits_host
    // non-null: the codec head runs on every row and the S rows land there; otherwise on the last row only.  Arms the slot like
    // prefill_rows_in_xp and leaves the last row's logits / normalised hidden row at long_last_logits / long_last_hidden.
    // base0 > 0 (a slot begun behind a shared prefix): the rows take positions [base0, base0 + S) behind cache rows [0, base0) that are
    // already in the slot's pages; prompt_len stays S, the talker position becomes base0 + S.
    void prefill_rows_long(int slot, float* x, int S, float* logits_host, int base0 = 0);
    void long_ws_ensure();                      // the 128-row workspace (allocated once)
    float* long_rows(int S);                    // device staging for S prompt rows (grow-only)
    struct LongWs { float *qkv = nullptr, *attn = nullptr, *act = nullptr, *slab = nullptr, *gu_slab = nullptr, *qkv_slab = nullptr, *hn = nullptr, *logits = nullptr;
                    bf16_t *p0h = nullptr, *p0l = nullptr, *p1h = nullptr, *p1l = nullptr; int rows = 0; } lws;
    void long_ws_swap();                        // exchanges run_layers' row workspaces (and ws_rows) with lws
    // a pass in the long workspace with the chunk attention (prefill_rows_long, the prefixed group, the ragged chunks); leaves no segment tables behind
    struct LongWsScope { Engine& e; explicit LongWsScope(Engine& en) : e(en) { e.long_ws_swap(); e.chunk_attn = true; } ~LongWsScope() { e.seg_attn = nullptr; e.chunk_attn = false; e.long_ws_swap(); } };
    float* long_x_d = nullptr; size_t long_x_rows = 0;
    const float *long_last_logits = nullptr, *long_last_hidden = nullptr;
    int prefill_chunk = 128;                    // Q3TTS_PREFILL_CHUNK (16..128) at engine creation: A/B knob, lets a test cross chunk boundaries at a short prompt
    bool chunk_attn = false;                    // prefill_rows_long -> run_layers: the attention launch is launch_attn_prefill
    int ws_rows = 0;                            // rows the slab workspaces in use are laid out for (rows_max; 128 inside a long prefill)
    void talker_decode(int slot, const float* embed, float* logits, float* last_hidden);
    void code_predictor(const float* seq, int n, int step, float* logits);
    void sample(const float* logits, int n, const q3tts_sampling& p, float u, int suppress, int64_t* tok);
    void sample_hist(const float* logits, int n, const q3tts_sampling& p, float u, int suppress, const int64_t* hist, int n_hist, int64_t* tok);   // + repetition penalty over the ids in hist
    void build_prompt(const int64_t* ids, int n_ids, int lang, const float* speaker, float* prompt, int* S,
                      float* trailing, int cap_rows, int* n_trailing);
    void build_prompts(const int64_t* ids, const int32_t* offsets, int n_utt, int lang, const float* const* speakers,
                       float* prompts, int* S_out, float* trailing, const size_t* toff, int* nt_out, bool open_text = false);
    int64_t* proj_ids_d = nullptr; float* proj_out_d = nullptr; size_t proj_cap = 0;   // text_project staging (grow-only)
    std::vector<int64_t> proj_ids_h;
    int64_t codec_decode_host(const int64_t* codes, int F, float* pcm, int64_t cap);
    int64_t codec_decode_dev(const int32_t* codes_dev, int F, float* pcm_dev, int64_t cap);
    // exact chunked / streaming decode: samples owned by frames [a, b), decoded from the window [a - left_context, b)
    int64_t codec_decode_range_dev(const int32_t* codes_dev, int a, int b, int left_context, float* pcm, int64_t cap);
    int64_t slot_codec_decode_range(int slot, int a, int b, int left_context, float* pcm, int64_t cap);
    int64_t codec_decode_chunked_host(const int64_t* codes, int F, int chunk, int left_context, float* pcm, int64_t cap);
    // streaming decode with carried state (q3_codec.cpp): a stream keeps the pre-transformer's K / V rows and output rows, a push decodes
    // n new frames in O(n + stage_b_context) work, exactly
    void codec_debug_group(float* sx_out, float* pcm_out, int64_t cap_floats, int* T, int* C, int* nb);
    int64_t codec_debug_partials(float* out, int64_t cap_floats);
    void codec_poison();                                // test hook: the vocoder's reusable workspace filled with NaN bytes
    int codec_stream_begin(int max_frames);
    void codec_stream_fit(int sid, int n);              // room for a push of n frames in the stream's sliding K / V and row buffers
    int64_t codec_stream_push_dev(int sid, const int32_t* codes_dev, int n, float** pcm_dev);
    int64_t codec_stream_push_host(int sid, const int64_t* codes, int n, float* pcm, int64_t cap);
    void codec_stream_end(int sid);
    int codec_stream_frames(int sid) const;
    int codec_stage_b_context() const;          // frames the stages behind the pre-transformer look back
    int64_t slot_codec_stream_range(int slot, int a, int b, float* pcm, int64_t cap);
    // batched push: n new frames (device codes) for each of g distinct streams in one set of launches; n == 0 leaves a stream untouched.
    // PCM lands in the callers' host buffers (min(n_own, cap) samples); validated as a whole before any stream advances
    struct StreamPush { int sid = -1; const int32_t* codes_dev = nullptr; int n = 0; float* pcm = nullptr; int64_t cap = 0; int64_t n_own = 0;
                        bool finish = false; /* a stream with a sink: flush its tail with this push (n == 0 allowed) */ };
    void codec_stream_push_batch(StreamPush* ps, int g);
    // finish[i] (optional): stream i's sink flushes its tail with this push.  float_only: a stream with a sink is refused (pcm_out is
    // read as float); otherwise pcm_out[i] is read in the stream's sink's format and cap / pcm_len count its samples
    void codec_stream_push_batch_host(int n_streams, const int32_t* sids, const int64_t* codes, const int32_t* frame_offsets, float* const* pcm_out,
                                      int64_t cap, int64_t* pcm_len, const uint8_t* finish = nullptr, bool float_only = true);
    void slots_codec_decode_new(int n_slots, const int32_t* slots, float* const* pcm_out, int64_t cap, int64_t* pcm_len, int32_t* frame_begin, int32_t* frame_end,
                                const int32_t* frame_limit = nullptr,    // frame_limit[i] (optional): decode slot i's frames below it only
                                const int32_t* final_frames = nullptr);  // final_frames[i] >= 0 (optional): the utterance ends at that frame count; the push that reaches it flushes the slot's sink
    // priming: g open streams without frames take the state a push of their first n frames would leave — pre-transformer only, the K / V
    // and output-row tails copied into the streams' buffers, which keep the size codec_stream_begin gave them (StreamPush: sid, codes_dev, n)
    void codec_stream_prime_batch(const StreamPush* ps, int g);
    void codec_stream_prime_batch_host(int n_streams, const int32_t* sids, const int64_t* codes, const int32_t* frame_offsets);
    void slots_codec_prime(int n_slots, const int32_t* slots, const int32_t* n_frames);
    void codec_stream_info(int sid, int* n_done, int* kv_capacity_rows, int64_t* bytes) const;
    void slot_codec_stream_reset(int slot);
    void codec_rope_tables(int P);

    // ---- carried-state stages behind the vocoder: 24 kHz float on the device in, the stage's samples out ----
    // Six kinds in one fixed order: the pitch stage (q3_pitch.cpp, 4o), the stretcher (q3_speed.cpp, 4m), the tone stage (q3_tone.cpp,
    // 4r), the loudness stage (q3_loudness.cpp, 4p), the level stage (q3_level.cpp, 4n), the PCM sink (q3_pcm_sink.cpp, 4l).  Stage (q3_stage.cpp) is what they share: a call reserves once (the only
    // place the workspaces may grow, before anything is enqueued), launches once per set of stages whose input is ready, and commits
    // after the stream's sync.
    enum StageKind { SK_PITCH = 0, SK_SPEED = 1, SK_TONE = 2, SK_LOUD = 3, SK_LEVEL = 4, SK_SINK = 5, SK_N = 6 };
    static constexpr int kMaxStages = 4096;                          // of a kind, open at the same time (vocoder streams' included)
    static constexpr int64_t kStageMaxPush = 1440000;                // one push of a standalone entry: 60 s
    // x_dev: n_new samples on the device; out_host (NULL ok): min(n_out, cap) samples in the stage's output format land there;
    // offs_host (NULL ok, the stretcher's and the loudness stage's): min(n_frames, offs_cap) per-frame words.  n_out, n_frames, out_dev / offs_dev (the push's
    // output on the device, valid until the call's next reserve) and desc are set by plan and launch
    struct StagePush { int id = -1; const float* x_dev = nullptr; int64_t n_new = 0; bool finish = false; void* out_host = nullptr; int64_t cap = 0;
                       int32_t* offs_host = nullptr; int64_t offs_cap = 0; int64_t n_out = 0, n_frames = 0;
                       const float* out_dev = nullptr; const int32_t* offs_dev = nullptr; int desc = -1; };
    struct DevBuf { char* p = nullptr; size_t cap = 0; };           // a grow-only device workspace; cap in elements
    void ws_grow(DevBuf& b, size_t want, size_t el);                 // syncs and reallocates (64 elements at least) when b holds fewer than want
    struct Stage {
        Engine& e;
        const char *name, *noun, *count_noun;                        // the refusals' words: "level", "level stage", "stage"
        bool has_offs = false;                                       // the kind keeps per-frame words (the stretcher's offsets, the loudness stage's report)
        Stage(Engine& en, const char* nm, const char* nn, const char* cn) : e(en), name(nm), noun(nn), count_noun(cn) {}
        virtual ~Stage() {}
        // ---- what a kind supplies ----
        virtual void end(int id) = 0; virtual void free_all() = 0;   // free_all: the kind's own allocations (ws_free is the shared part)
        virtual int64_t push_len(int id, int64_t n_new, bool finish) const = 0;   // host-only: samples that push would deliver; throws when it would be refused
        virtual size_t out_el(int id) const { return sizeof(float); }             // bytes per delivered sample
        virtual bool idle(StagePush& q) const { return q.n_new == 0 && q.n_out == 0; }   // an empty push: the carry stays, nothing is emitted
        virtual size_t desc_size() const = 0; virtual const void* desc_at(size_t i) const = 0;
        virtual void desc_reset(size_t n) = 0;                       // the call's host descriptors: never resized during the call (uploads read them until the sync)
        virtual bool fill(StagePush& q, size_t di, char* out, int32_t* offs) = 0;   // descriptor di of a live push; false drops it
        virtual void issue(size_t d0, int n_live) = 0;               // the kind's launch over uploaded descriptors [d0, d0 + n_live)
        virtual void commit_one(const StagePush& q) = 0;             // counters advance, carries flip by the kind's rule
        // ---- what they share (q3_stage.cpp) ----
        DevBuf desc, out, in, offs;                                  // descriptors, packed outputs (bytes), a standalone entry's staged input (floats), the stretcher's frame offsets
        size_t desc_n = 0, desc_used = 0, out_used = 0, offs_used = 0;   // descriptors the call reserved; what its launches have taken
        static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // a push's share of the packed output
        size_t plan(StagePush& q) const;                             // sets n_out (and n_frames) of a push about to be reserved, returns its output bytes; throws like push_len
        void reserve(int n_total, size_t out_bytes_total, size_t offs_total = 0);   // once per call, before anything is enqueued
        void launch(StagePush* ps, int n);                           // one descriptor upload + one launch + the device -> host copies; no stage moves
        void commit(const StagePush* ps, int n) { for (int i = 0; i < n; ++i) commit_one(ps[i]); }   // after the sync
        void push_batch_host(int n, const int32_t* ids, const float* const* pcm24, const int64_t* n_in, const uint8_t* finish,
                             void* const* out_host, int64_t cap, int64_t* out_len, int32_t* const* offsets_out = nullptr, int64_t* n_offsets = nullptr);
        void ws_free();
    };
    template <class Desc, class Slot> struct StageOf : Stage {   // a kind's typed halves: its host descriptors and its table (q3_stage.h)
        StageOf(Engine& en, const char* nm, const char* nn, const char* cn, const char* none) : Stage(en, nm, nn, cn), tab{ nm, nn, none, kMaxStages, {} } {}
        StageTable<Slot, Error> tab;
        std::vector<Desc> desc_h;
        void end(int id) override { tab.end(id); }
        size_t desc_size() const override { return sizeof(Desc); }
        void desc_reset(size_t n) override { desc_h.assign(n, Desc()); }
        const void* desc_at(size_t i) const override { return &desc_h[i]; }
    };

    // the pitch stage.  mem: its own allocation, two halves of kPitchHalfFloats floats (carried input, the two output accumulators, the
    // mark state).  carry_abs0: absolute index of the first carried sample.  The host rule needs nothing from the device.
    struct Shifter : StageSlot { int ratio = 1000; int64_t carry_abs0 = 0; float* mem = nullptr; };
    struct PitchStage : StageOf<PitchDesc, Shifter> {
        explicit PitchStage(Engine& en) : StageOf(en, "pitch", "pitch stage", "stage", "no such pitch stage") {}
        float* win_d = nullptr;                                      // the windows: a host table, built once and uploaded
        int begin(int ratio);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } pitch{*this};
    // the stretcher.  mem: its own allocation, [2][kSpeedCarry] floats of carry followed by [2][2] int64 of state { p, frames }.
    // carry_abs0: absolute index of the first carried sample; frames: completed (the host rule's count, which the device's state repeats)
    struct Stretcher : StageSlot { int speed = 1000; int64_t frames = 0, carry_abs0 = 0; float* mem = nullptr; };
    struct SpeedStage : StageOf<SpeedDesc, Stretcher> {
        explicit SpeedStage(Engine& en) : StageOf(en, "speed", "stretcher", "stretcher", "no such stretcher") { has_offs = true; }
        float* win_d = nullptr;                                      // the window: a host table, built once and uploaded
        int begin(int speed);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        bool idle(StagePush& q) const override;                      // sets n_frames, the frames the push would complete
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } speed{*this};
    // the tone stage: a cascade of n biquads.  c: their coefficients, formed once at begin.  mem: its own allocation, two halves of
    // kToneStateDoubles doubles (two per signal).  The host rule is the identity.
    struct Equaliser : StageSlot { int n = 0; double c[kToneMaxSections][5] = {}; double* mem = nullptr; };
    struct ToneStage : StageOf<ToneDesc, Equaliser> {
        explicit ToneStage(Engine& en) : StageOf(en, "tone", "tone stage", "stage", "no such tone stage") {}
        int begin(int n, const ToneSection* sections);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } tone{*this};
    // the loudness stage: BS.1770 meter and normaliser.  mem: its own allocation, two halves of kLoudHalfBytes (state words, then the
    // open sub-block's input).  pt, r_lo, r_hi, g_start: formed once on the host from the parameters.  A push's n_frames is four words
    // per sub-block it closes: its int64 energies, then its float gains.  The host rule needs nothing from the device.
    struct Normaliser : StageSlot { int target = 0; double pt = 0.0, r_lo = 1.0, r_hi = 1.0; float g_start = 1.0f; char* mem = nullptr; };
    struct LoudStage : StageOf<LoudDesc, Normaliser> {
        explicit LoudStage(Engine& en) : StageOf(en, "loudness", "loudness stage", "stage", "no such loudness stage") { has_offs = true; loudness_coeffs(24000, coeffs); }
        double coeffs[10];                                           // the two biquads at 24 kHz
        int begin(int target_dlufs, int range_cb, int start_cb);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        bool idle(StagePush& q) const override;                      // sets n_frames, four words per sub-block the push would close
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } loud{*this};
    // the level stage: gain and look-ahead limiter.  mem: a limiter's own allocation, [2][kLevelCarry] floats of carry (the last 254
    // values of v); a gain-only stage (ceiling 0) carries nothing.  The host rule needs nothing from the device.
    struct Leveler : StageSlot { int gain_cb = 0, ceiling = 0; float* mem = nullptr; };
    struct LevelStage : StageOf<LevelDesc, Leveler> {
        explicit LevelStage(Engine& en) : StageOf(en, "level", "level stage", "stage", "no such level stage") {}
        int begin(int gain_cb, int ceiling);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } level{*this};
    // the PCM sink.  carry: [2][kPcmSinkCarry] floats in the sink's own allocation.  carry_abs0: absolute index of the first carried sample
    static constexpr int kPcmSinkCarry = 256;                        // floats per carry buffer (2 * half + ceil(M / L) <= 198)
    struct SinkPlanDev { SinkPlan plan; float* tab_d = nullptr; };
    struct PcmSink : StageSlot { int rate = 24000, format = 0; const SinkPlanDev* plan = nullptr; int64_t carry_abs0 = 0; float* carry = nullptr; };
    struct SinkStage : StageOf<PcmSinkDesc, PcmSink> {
        explicit SinkStage(Engine& en) : StageOf(en, "pcm sink", "sink", "sink", "no such sink") {}
        std::map<int, SinkPlanDev> plans;                            // by rate: built once, uploaded, kept (node addresses are stable)
        const SinkPlanDev& plan_for(int rate);
        int begin(int rate, int format);
        void free_all() override;
        int64_t push_len(int id, int64_t n_new, bool finish) const override;
        size_t out_el(int id) const override { return pcm_format_bytes(tab.get(id).format); }
        bool fill(StagePush& q, size_t di, char* out, int32_t* offs) override;
        void issue(size_t d0, int n_live) override; void commit_one(const StagePush& q) override;
    } sink{*this};
    Stage* const stages[SK_N] = { &pitch, &speed, &tone, &loud, &level, &sink };         // by StageKind: the order a stream's audio passes them in

    // vocoder streams: a stream delivers its audio through the stages it has (codec_stream_push_batch; behind a sink StreamPush::pcm is read as
    // the sink's format, n_own counts its samples).  Refused once the stream has delivered a sample.  1000, (0, 0), 24 000 Hz float: no stage.
    void codec_stream_set_pitch(int sid, int ratio);
    void codec_stream_set_speed(int sid, int speed);
    void codec_stream_set_tone(int sid, int n, const ToneSection* sections);   // n == 0: no stage
    void codec_stream_set_loudness(int sid, int target_dlufs, int range_cb, int start_cb);
    void codec_stream_set_level(int sid, int gain_cb, int ceiling);
    void codec_stream_set_sink(int sid, int rate, int format);
    // the scheduler's stages (q3tts_engine_set_sink / _speed / _level / _pitch / _loudness / _tone): slots' implicit streams begin with them.
    // Zeros: none (loud: whether there is a loudness stage at all, since target 0 is a meter)
    struct SlotStages { int sink_rate = 0, sink_format = 0, speed = 0, gain_cb = 0, ceiling = 0, pitch = 0, loud = 0, loud_target = 0, loud_range = 0, loud_start = 0,
                        tone_n = 0; ToneSection tone[kToneMaxSections] = {}; } slot_stages;

    // ---- batch-first session ops on DEVICE pointers (include/q3tts.h "_dev" entry points): row b <-> slot b ----
    // caller stream: the engine's stream first waits for what the caller has enqueued, the caller's stream then waits for the call's work
    void stream_join(hipStream_t caller);
    void stream_fork(hipStream_t caller);
    void talker_prefill_dev(const float* embeds, int nb, int S, const int32_t* lens, float* logits_last, float* last_hidden);
    void talker_decode_dev(const float* embeds, int nb, const uint8_t* active, float* logits, float* last_hidden);
    void code_predictor_dev(const float* last_hidden, const int64_t* code0, int nb, const q3tts_sampling& p, uint64_t seed, uint32_t stream0,
                            uint32_t frame, int32_t* sub);
    void sample_dev(const float* logits, int nb, int V, const q3tts_sampling& p, const float* u, int suppress, int64_t* ids);
    void sample_hist_dev(const float* logits, int nb, int V, const q3tts_sampling& p, const float* u, int suppress, const int64_t* hist, int hist_ld,
                         const int32_t* hist_len, int64_t* ids);
    static float checked_penalty(const q3tts_sampling& p);   // throws unless repetition_penalty is 0 (off) or a positive finite factor
    void dev_scratch(int nb);                  // lazily allocated workspaces of the four calls above
    float* dev_logits_d = nullptr; int* dev_flags_d = nullptr; int32_t* dev_pos_d = nullptr; int32_t* dev_pos_dummy_d = nullptr;
    SlotState* dev_st_d = nullptr; int32_t* dev_codes_d = nullptr;
    hipEvent_t ev_join = nullptr, ev_fork = nullptr;
    void predictor_passes(int nb, const SampleArgs& s0, bool sp0, bool spn, const std::function<void()>& mark);

    // ---- fused generation: beginning utterances in slots (q3_begin.cpp) ----
    // Three entries, because which prompts share a pass decides the bits: slots_begin (equal-length groups in xp), slots_begin_prefixed
    // (groups at per-member bases in the long workspace) and slots_begin_ragged (segments over 128-row chunks).  Their refusals, the
    // quantities derived from a member, the grouping rule and what differs between the entries are in ONE place, q3_begin_plan.h; what
    // surrounds their launches is the helpers below, each written once.
    struct SlotInit { int slot = 0; const float* prompt = nullptr; int S = 0; const float* trailing = nullptr; int n_trailing = 0; uint32_t stream_id = 0;
                      int max_frames = 0; /* 0: the call's max_new_tokens */
                      int kv_tokens = 0;  /* KV pages reserved now, in tokens; 0: prompt + max_frames (the slot never needs more) */
                      // Teacher-forced frames behind the prompt (continue from codes): prefix[n_prefix][n_groups] on the host.  The slot is
                      // left as if it had generated exactly these as its first n_prefix frames; max_frames and max_new_tokens count the
                      // frames behind them.  Such a slot is begun on its own (slots_begin with n == 1), like any long prompt.
                      const int64_t* prefix = nullptr; int n_prefix = 0;
                      int prefix_id = -1; /* slots_begin_prefixed: the shared prompt prefix in front of the prompt (-1: none) */ };
    void slots_begin(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos); // batched prefill of equal-length prompts
    void slot_begin(int slot, const float* prompt, int S, const float* trailing, int n_trailing,
                    const q3tts_sampling& p, uint64_t seed, uint32_t stream_id, int ignore_eos);
    void slot_begin_forced(const SlotInit& q, const q3tts_sampling& p, uint64_t seed, int ignore_eos, float rep_penalty, int base = 0);   // the path for n_prefix > 0, one slot (base: rows of a shared prefix in front)
    // run_layers' MFMA condition on a stack's dims (the rows are the caller's: M >= mfma_min_rows): the slab GEMMs tile H, nq * d and ffn by 128
    static bool mfma_dims_ok(const DecStack& W) { return W.H % 128 == 0 && (W.nq * W.d) % 128 == 0 && W.ffn % 128 == 0 && W.H <= 4096; }
    BeginLimits begin_limits() const { return BeginLimits{B, max_ctx, max_trailing, max_frames_cap, rows_max, mfma_min_rows, mfma_dims_ok(talker)}; }
    std::vector<BeginMember> begin_members(BeginEntry e, const SlotInit* in, int n, int max_new);   // the members' views, checked by the entry's rules (throws)
    void kv_reserve_set(const BeginMember* m, int n, int max_new);                 // KV pages (begin_tokens) for the whole set, all or nothing
    void prefix_fan_out(const SlotInit* in, int n);                                // each prefix's rows into the pages of its slots
    void scatter_last_rows(const float* logits_row, const float* hidden_row, int slot);   // -> logits_t[slot], x_cp[slot]
    void stage_slot_inputs(const SlotInit& q);                                     // trailing rows up, code0 history cleared
    // the only writer of the armed SlotState (P: prefix rows in front).  stage_inputs == false: the caller staged them in front of frame_rows_launch
    void arm_slot(const SlotInit& q, int P, float rep_penalty, const q3tts_sampling& p, uint64_t seed, int ignore_eos, bool stage_inputs);
    // ---- shared prompt prefix (run_prefill, tts_onnx.cpp:615-665, once for many utterances) ----
    // A prefix is P talker input rows prefilled once in a borrowed slot; their K / V rows are kept in a compact store
    // [layer][kvh][P][head_dim] per cache (the cache's element type).  slots_begin_prefixed copies the store into each slot's own pages
    // (no page is shared) and prefills only the utterance's rows at base P: members that begin_groups puts in one group share one pass
    // through the layers (launch_attn_prefill's group form at per-member bases, up to 128 rows), the rest go one at a time through
    // prefill_rows_long(base0 = P).  Every prefix_id == -1: exactly slots_begin.
    struct Prefix { int P = 0; void* k = nullptr; void* v = nullptr; int64_t bytes = 0; int users = 0; };
    std::unordered_map<int, Prefix> prefixes;   // live prefixes by id (ids are never reused)
    int prefix_next_id = 0;
    static constexpr int kMaxPrefixes = 64;
    int prefix_create(const float* rows, int P);
    void prefix_release(int id);
    const Prefix& prefix_get(int id) const;     // throws on an unknown or released id
    void prefix_pin(int id, int delta);         // a running job holds its prefixes: prefix_release refuses them
    void slots_begin_prefixed(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos);
    void kv_prefix_copy(const Prefix& pf, const int* slots_dev, int n_dst, int slot0, bool scatter);
    float* grp_x_d = nullptr; int* grp_pos_d = nullptr;   // a prefixed group's rows [128][H] and per-member bases [128]
    // ---- ragged prefill: rows of many slots, with any lengths, bases and forced frames, share 128-row chunks ----
    // Members as in slots_begin_prefixed (optional prefix_id, own prompt of any S, optional forced frames).  Everything is validated
    // and the KV pages reserved (all or nothing) before anything is armed; the members' rows are staged contiguously in call order,
    // cut into chunks of prefill_chunk rows (a member that does not fit the rest of a chunk continues in the next one at base + rows
    // done) and every chunk takes ONE run_layers pass in the long workspace with the segment form of the chunk attention; the final
    // norm + codec head run on the rows that end a member.  n == 1, and whatever begin_ragged_one_at_a_time names (dims, the segment
    // kernels' instantiations, fewer than mfma_min_rows rows), begin their members one at a time (slots_begin_prefixed with n = 1).
    void slots_begin_ragged(const SlotInit* in, int n, const q3tts_sampling& p, uint64_t seed, int ignore_eos);
    struct SegMember { int slot = 0, base = 0, rows = 0; };
    struct SegChunk { int row0 = 0, rows = 0, n_seg = 0, n_tiles = 0, n_last = 0;      // rows [row0, row0 + rows) of the staged sequence
                      size_t seg = 0, row_seg = 0, tiles = 0, last = 0;                 // offsets (ints) of the chunk's tables in seg_tab_d
                      std::vector<int> last_member; };                                 // the members whose last row is in the chunk, in row order
    // cuts the members' rows into chunks, builds every chunk's tables in seg_tab_h and uploads them in one copy (the stream is
    // synchronised first: the previous call's upload may still read seg_tab_h)
    void seg_tables_build(const std::vector<SegMember>& members, std::vector<SegChunk>& chunks);
    std::vector<int32_t> seg_tab_h; int32_t* seg_tab_d = nullptr; size_t seg_tab_cap = 0;
    struct SegAttn { const int* seg = nullptr; const int* row_seg = nullptr; const int* tiles = nullptr; int n_seg = 0, n_tiles = 0; };
    const SegAttn* seg_attn = nullptr;          // slots_begin_ragged / prefill_rows_long -> run_layers: the chunk attention's segment tables
    float* rag_x_d = nullptr; size_t rag_x_rows = 0;   // the staged rows of a ragged call (grow-only)
    float* rag_rows(size_t rows);
    float *rag_last_x_d = nullptr, *rag_last_hn_d = nullptr;   // a chunk's member-ending rows [128][H] before / after the final norm
    bool prefill_seg = false;                   // Q3TTS_PREFILL_SEG=1 at creation (hook engines): prefill_rows_long issues its chunks through the segment kernels as one segment (A/B knob, tests' pin)
    int64_t ragged_passes = 0;                  // run_layers passes issued by slots_begin_ragged's chunk path (diagnostic, tools/ragged_prefill_bench.py)
    // forced-begin validation of recorded frames: code0 in [0, vocab) outside [suppress_begin, suppress_end) (a recorded frame never holds
    // EOS), sub-codes in [0, sub_vocab); strict == false (frame_rows): code0 anywhere in [0, vocab).  The error names frame and group.
    void check_frame_codes(const int64_t* codes, int n, bool strict) const;
    // rows of n given frames (FrameRowsArgs) on the engine's stream: codes from the host, everything else on the device
    void frame_rows_launch(const int64_t* codes, int n, int frame0, const float* trailing_dev, int trailing_len, float* out_dev,
                           int32_t* codes_out, uint32_t* seen);
    void frame_rows(const int64_t* codes, int n, int frame0, const float* trailing, int n_trailing, float* out);   // session-shaped, host I/O
    int64_t* frame_codes_d = nullptr; size_t frame_codes_cap = 0;   // staging of the given frames' ids (grow-only)
    float* frame_text_d = nullptr; size_t frame_text_rows = 0;      // frame_rows: the text rows it reads (grow-only)
    // ---- live text: the trailing block of reference tts_onnx.cpp:531-536 grows while the slot generates ----
    // Frame f reads text row f only (:833-842), so a slot needs to be one row ahead of its frame counter.  An open slot
    // (SlotState::text_open) whose next frame has no row yet stalls in the sampler for that step and changes nothing; appends are
    // stream-ordered between steps.  Every call validates everything before anything moves.
    void slot_text_open(int slot);   // after any begin, before the slot's first step
    // rows != null: n == 1, `rows` holds offsets[1] - offsets[0] projected rows [.][hidden] on the host; else ids [offsets[n]] go
    // through ONE text_project pass on the device.  One k_text_scatter launch for all n slots either way.
    void slots_text_append(int n, const int32_t* slots, const float* rows, const int64_t* ids, const int32_t* offsets, const uint8_t* close);
    void slot_text_status(int slot, int* n_text_rows, int* open, int* starved);
    void text_project_dev(const int64_t* ids, int n);   // text_project up to the copy back: rows [n][hidden] left in proj_out_d (stream-ordered)
    void proj_reserve(size_t rows);
    void check_text_and_mark_stepped(int nb);            // every stepping entry, before its launches: refuses an open slot without the row of its first frame, then marks the armed slots as stepped; an open slot that has not stepped since its begin needs the row of its first frame
    void build_prompt_open(const int64_t* ids, int n_ids, int lang, const float* speaker, float* prompt, int* S, float* trailing, int cap_rows, int* n_trailing);
    float* tts_eos_d = nullptr;      // text_project(TTS_EOS): the row build_prompts puts behind a whole text (:535)
    int32_t* text_desc_d = nullptr;  // k_text_scatter records [B][8]
    std::vector<uint8_t> stepped_h;  // per slot: stepped since its begin (host mirror; a stalled step of a fresh slot would overwrite its armed logits)
    int decode_steps(int n_steps);
    void slot_status(int slot, int* n_frames, int* finished);
    void slot_codes(int slot, int64_t* codes, int cap_frames);
    void slot_logits(int slot, float* logits, float* last_hidden);
    int64_t slot_codec_decode(int slot, float* pcm, int64_t cap);
    void slot_release(int slot);
    void step_bytes(double* wbytes, double* kvbytes);
    void measure_skip_frames(int n);                    // measurement aid: armed slots jump n frames ahead over a synthetic KV cache
    void pack_mfma_weights();                           // fragment-packed copies of the projection matrices for k_gemv16 / k_gemm3 (finalize)
    void free_packed_weights();
    std::vector<std::pair<const bf16_t*, bf16_t*>>& packed_w;
    void prefill_profile(int nb, int S, int reps, double* ms_per_pass);   // device time of a batched prefill pass (diagnostic)
    void stage_profile(int n_steps, double* out_ms4);   // eager steps with events at the stage boundaries (diagnostic)
    // one EAGER step of the armed slots that also keeps, for slot `slot`, the logits row every one of the frame's n_groups decisions was
    // sampled from (out: [n_groups][cols], cols >= max(vocab, sub_vocab)); the slots advance like decode_steps(1)
    void step_logits(int slot, float* out, int cols);
    float* trace_d = nullptr; int trace_slot = 0, trace_cols = 0;
    std::vector<hipEvent_t> stage_ev;

    float last_decode_ms = 0.f;
    int last_decode_steps = 0;
    float last_codec_ms = 0.f;
    double total_decode_ms = 0.0, total_codec_ms = 0.0;
    int64_t total_decode_steps = 0, total_codec_frames = 0;

    // ---- codec decoder (q3_codec.cpp) ----
    CodecW* codec = nullptr;
    void codec_finalize();                      // the set's CodecWeights (again), then codec_runtime_init
    void codec_runtime_init();                  // this engine's CodecW over ws.codec: lanes, page table
    void codec_plane_stats(int* two_product, int* three_product) const;   // weight tensors on the 2-product (lo plane empty) / 3-product split path
    // returns the sample count; h_in: this utterance's rows from codec_pre_batch (h_stage 1: after the pre-transformer, 2: after the upsampling stages too)
    int64_t codec_run(const int32_t* codes_dev, int F, float** pcm_dev, int lane = 0, const float* h_in = nullptr, int h_stage = 1, int nbatch = 1, size_t h_ustride = 0);
    void codec_async_submit_group(const float* h_group, size_t h_ustride, int Fg, int g, const int* nf, float* const* user_pcm, int64_t cap, int64_t* const* len_out);
    bool codec_batchable() const;   // every conv of the decoder takes the split-precision path (the batched kernels)
    const float* codec_pre_batch(const int32_t* codes_dev, int codes_stride_frames, int n, int Fp, bool with_upsampling, int* rows_per_utt_out,
                                 const int* perm_host = nullptr);
    // vocoder side of the scheduler: stash a finished slot's codes, vocode the job's utterances over the side lanes at the end
    void codec_async_prepare(int max_frames, int n_utt);
    const int32_t* codec_stash(int slot, int nf, int utt, int row_frames);
    const int32_t* codec_job_codes(int utt, int row_frames);
    void codec_job_upload(const int32_t* host, int n_utt, int row_frames);
    void codec_async_submit_dev(const int32_t* codes_dev, int nf, float* user_pcm, int64_t cap, int64_t* len_out, const float* h_in = nullptr, int h_stage = 1);
    void codec_async_drain_lane(int lane);
    void codec_async_drain();
    void codec_async_abort();   // drop every pending vocoder result (error path: their host pointers belong to a failed job)
    void codec_lanes_join();
    void slots_state(int nb, std::vector<SlotState>& out);
    void codec_free();

    // ---- speaker encoder of the clone path (q3_speaker.cpp) ----
    SpeakerW* spk = nullptr;
    bool has_speaker() const { return c.spk_enc_dim > 0; }
    void speaker_finalize();
    void speaker_free();
    // mel [spk_mel][frames] (the reference MelExtractor layout) on the host -> embedding [spk_enc_dim] on the host
    void speaker_encode(const float* mel, int frames, float* out);
    // GPU front end for audio already in memory (mono float, any rate).  Each call stages its clips in one pinned copy, runs on the
    // engine's stream in the engine-owned workspace (grow-only, freed with the engine) and ends with one stream sync.
    SpkFront* spkf = nullptr;
    void front_finalize();                      // the log-mel tables of q3_audio.cpp's make_plan, uploaded once per set
    // q3::resample_linear on the GPU, bit for bit; returns the output length, writes min(length, cap) samples when out != null
    int64_t resample_gpu(const float* in, int64_t n, int src_rate, int dst_rate, float* out, int64_t cap);
    // resample to 24 kHz (when sample_rate != 24000) + q3::log_mel: mel [128][*frames]; mel == null only sizes.  false: no frame (empty clip)
    bool mel_gpu(const float* audio, int64_t n, int sample_rate, float* mel, int64_t cap, int* frames);
    // n_clips clips -> out [n_clips][spk_enc_dim]; a clip's embedding does not depend on the rest of the batch
    void speaker_embed_pcm(int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* rates, float* out);

    // ---- audio encoder of the 12 Hz tokenizer (q3_encoder.cpp): audio -> codes, fp32 throughout ----
    EncoderW* enc = nullptr;
    bool has_audio_encoder() const { return c.enc_hidden > 0; }
    void encoder_finalize();                                  // the set's EncWeights (again), then encoder_runtime_init
    void encoder_runtime_init();                              // this engine's EncoderW over ws.enc: RoPE tables; streams and workspace grow later
    void encoder_free();
    void encoder_poison();                                    // test hook: NaN bytes over the encoder's workspace (stream state lives outside it)
    static constexpr int64_t kEncMaxClipSamples = 1440000;    // 60 s at 24 kHz: one clip
    static constexpr int64_t kEncMaxRawSamples = 23040000;    // a clip (and a group's clips together) at another rate: samples to resample (60 s at 384 kHz, 92 MB)
    static constexpr int64_t kEncMaxGroupSamples = 2880000;   // a batch is processed in consecutive groups of at most this many samples
    int64_t audio_encode_len(int64_t n24) const;              // frames of a clip of n24 samples at 24 kHz (the convs' own ceil rule)
    // n_clips clips (mono float, any rate) -> codes [frames][n_groups] int64 and / or latents [frames][enc_hidden] per clip (either array
    // or entry may be null); caps[i] = frames of room in clip i's buffers.  One set of launches per group; a clip's result does not
    // depend on the rest of the batch.  Validates everything before the first byte moves.
    void audio_encode(int n_clips, const float* const* pcm, const int64_t* n_samples, const int32_t* rates, int64_t* const* codes_out,
                      float* const* latents_out, const int32_t* caps, int32_t* n_frames);
    float last_audio_encode_ms = 0.f;                         // device time of the last audio_encode / audio_stream_push_batch call: uploads + launches of all its groups
    void enc_transformer_host(const float* rows, int n_rows, float* out);   // parity aid: the transformer alone
    // ---- streamed audio -> codes: carried-state pushes, bit-identical to audio_encode of the concatenated audio ----
    static constexpr int64_t kEncMaxStreamSamples = 86400000; // one hour at 24 kHz: a stream's max_samples
    static constexpr int kEncMaxStreams = 1024;               // open at the same time
    static constexpr int kEncMaxStreamRate = 384000;          // the rate kEncMaxRawSamples is worded for; a stream's carry is then 17 samples at most
    // A stream at sample_rate (1 .. kEncMaxStreamRate) in format Q3TTS_PCM_F32 / _S16 (other than 24 kHz float it resamples
    // on the way in, bit-identical to audio_encode at that rate).  max_samples counts the stream's own samples: 0 = 60 s, at most one
    // hour.  Regrows the RoPE tables when the stream can have more rows (syncs)
    int audio_stream_begin(int64_t max_samples, int sample_rate = 24000, int format = Q3TTS_PCM_F32);
    int64_t audio_stream_push_len(int id, int64_t n_samples, bool finish) const;   // host-only: frames that push of the stream's own samples would return
    // n streams (distinct, open, not finished), each given n_samples[i] >= 0 more samples of its own rate and format (finish[i]: the
    // stream's last push, right edge as the one-shot's) -> the NEW frames' codes [frames][n_groups] / latents [frames][enc_hidden].
    // Everything is validated before any stream moves; one set of launches per group of streams whatever their number, rates and
    // formats.  float_only: the caller's samples are float, an int16 stream is refused.
    void audio_stream_push_batch(int n, const int32_t* ids, const void* const* pcm, const int64_t* n_samples, const int32_t* finish,
                                 int64_t* const* codes_out, float* const* latents_out, const int32_t* caps, int32_t* n_frames, bool float_only = false);
    void audio_stream_info(int id, int64_t* n_samples, int32_t* n_frames, int* finished, int64_t* bytes) const;   // n_samples: received, at the stream's own rate
    void audio_stream_format(int id, int32_t* sample_rate, int32_t* format) const;
    void audio_stream_end(int id);                            // the stream's buffers stay for the next begin; freed in encoder_free
    void enc_calibrate_synthetic(uint64_t seed);              // fill_synthetic: codebooks at the scale of the projected latents

    // ---- internals ----
    DecStack talker, cp;
    const float* talker_norm = nullptr; const bf16_t* codec_head = nullptr; const bf16_t* codec_embed_w = nullptr;
    const bf16_t *text_embed = nullptr, *fc1_w = nullptr, *fc2_w = nullptr; const float *fc1_b = nullptr, *fc2_b = nullptr;
    const float* cp_norm = nullptr;
    const bf16_t* cp_proj_w = nullptr; const float* cp_proj_b = nullptr; // talker width -> predictor width (1.7B), null when equal
    float* x_cpp = nullptr;                                               // projected predictor input rows [<= rows_max][cp_width]
    int cp_width() const { return c.cp_hidden > 0 ? c.cp_hidden : c.hidden; }
    bool cp_projected() const { return cp_width() != c.hidden; }
    float* cp_project(float* rows, int ld, int M);
    std::vector<const bf16_t*> cp_head, cp_embed_w;

    int rows_max = 0, max_trailing = 0, max_frames_cap = 0;
    // rows from which a projection takes the split-K slab GEMM (k_gemm3 with the in-launch seam, 5 launches per layer; k_gemm2 + finish
    // kernels, 8 launches, where the seam does not apply).  Below it the GEMV-family contract holds (5 launches per layer): 1-2 rows
    // single-pass GEMV, 3..11 rows k_gemv16 on the matrix cores.  Crossover measured with the seam (round 3): b=8 3.76 (gemv16) vs 3.87 ms,
    // b=12 3.99 vs 3.89, b=16 4.22 vs 3.93; it was 17 rows with the finish launches.
    int mfma_min_rows = 12;
    float *x_talk = nullptr, *qkv = nullptr, *attn = nullptr, *act = nullptr, *logits_t = nullptr, *logits_cp = nullptr;
    float *x_cp = nullptr, *x_cp1 = nullptr, *sum = nullptr, *xp = nullptr, *hn = nullptr, *logits_p = nullptr;
    // `sum` [B][H] is more than step scratch since live text: row b must keep the running embedding sum of slot b's last sampled frame
    // from one step to the next (and across other slots' begins), because the last sampler of a STALLED slot rebuilds the slot's talker
    // input row from it (k_sample).  Only k_sample (rows of slots that sample) and the `_dev` predictor session write it; do not reuse
    // it as a workspace.  x_talk, by contrast, does not survive a step (run_layers works in place on it).
    float *trailing_d = nullptr, *tts_pad_d = nullptr, *text_tmp = nullptr, *text_tmp2 = nullptr;
    int64_t* ids_d = nullptr;
    bf16_t *pl0h = nullptr, *pl0l = nullptr, *pl1h = nullptr, *pl1l = nullptr; // (hi, lo) activation planes for the MFMA GEMM path
    int ldp = 0;
    float* slab_d = nullptr; // split-K partial sums [ks][rows][H]
    float* gu_slab_d = nullptr;  // gate | up split-K partial sums, 2 x [<=4][rows][ffn]
    float* cp_logit_slab_d = nullptr; // split-K partial sums of the batched predictor heads [4][B][sub_vocab]: the sampler sums them
    float* qkv_slab_d = nullptr; // split-K partial sums of the QKV projection [<=4][rows][QKV]
    // o_proj split by kv head (b = 1, both stacks): the 8 heads' partial rows [8][<= 2 rows][H] that the gate/up GEMV adds to x, and the sum
    // x + o_proj [<= 2][H] it leaves for the down projection's residual operand
    float *oproj_part_d = nullptr, *xmid_d = nullptr;
    // Layer-0 QKV rows of predictor passes 1 .. n_groups - 2 at b = 1, looked up instead of computed.  The input row of such a pass is
    // cp_embed_w[g - 1][code], so W_qkv[0] . RMSNorm(in_norm[0])(row) depends on the weights and (g, code) alone: cp_qkv_tab
    // [n_groups - 2][sub_vocab][QKV] fp32 (470 MB at 0.6B dims) holds every such row, made at finalize by the very GEMV launch the step
    // would issue (qkv_gemv_args: bit-identical).  The sampler of group g copies row (g, code) into qkv (SampleArgs::qkv_tab) and
    // announces it through qkv_in_ready; run_layers then starts the pass at its attention launch.  Built only by engines of one or two
    // slots whose predictor takes the fused b = 1 path (cp_qkv_table_applies); wider engines keep the GEMV when they drain to one slot.
    // The table is the set's (WeightSet::cp_qkv_tab): built at most once, by the first holder it applies to, on that holder's stream,
    // and published after its launches completed; this member is the engine's view of it (null where the table does not apply).
    float* cp_qkv_tab = nullptr;
    bool cp_qkv_table_on = true;   // Q3TTS_CP_QKV_TABLE=0 at engine creation: no table, the GEMV is launched (A/B knob, tests' second path)
    bool qkv_in_ready = false;     // predictor_passes -> run_layers: the sampler in front already wrote layer 0's qkv row
    bool cp_qkv_table_applies() const;
    void build_cp_qkv_table();
    void free_cp_qkv_table();      // drops this engine's view and the captured graphs: an nb = 1 graph has the table's address baked in
    GemvArgs qkv_gemv_args(const DecStack& W, int l, const float* x, int ldx, float* out, int M) const;   // a layer's QKV projection on the GEMV path
    bool gemv_xlds = true;       // Q3TTS_GEMV_XLDS=0 at engine creation: GemvArgs::xlds of this engine's GEMV launches (A/B knob, tests' second path; same bits)
    bool gemv_psum_lead = true;  // Q3TTS_GEMV_PSUM_LEAD=0 at engine creation: GemvArgs::psum_lead of this engine's gate/up launches behind a kv-head-split o_proj (A/B knob, tests' second path; same bits)
    bool cp_kvh_lead = true;     // Q3TTS_CP_KVH_LEAD=0 at engine creation: CpAttnOprojArgs::lead of this engine's k_cp_attn_kvh launches (A/B knob, tests' second path; same bits)
    void gemv(GemvArgs g) const { g.xlds = gemv_xlds; g.psum_lead = gemv_psum_lead; launch_gemv(g, stream); }
    bool kvh_oproj = true;       // Q3TTS_KVH_OPROJ=0 at engine creation: o_proj keeps the whole K in one launch (k_cp_attn_oproj / COMB GEMV; A/B knob, tests' second path)
    // split-K seam of the batched step (GemmArgs::seam): arrival / claim counters, one region per seam launch of the step (generation-valued words:
    // never reset), and the per-(row, 64-column tile) sums of squares behind the two residual seams of a layer
    unsigned* seam_cnt_d = nullptr; size_t seam_cnt_words = 0, seam_cnt_used = 0;
    unsigned* seam_gen_d = nullptr;   // the step generation the flag words carry (bumped by the step's first sampler launch)
    float *ssq_a_d = nullptr, *ssq_b_d = nullptr;
    bool seam_step = false;      // inside record_step: run_layers may fold the finish launches into the GEMMs
    bool seam_on = true;         // Q3TTS_SEAM=0 at engine creation keeps the finish launches (the A/B knob and the tests' second path)
    bool attn_stream = true;         // Q3TTS_ATTN_STREAM=0 at engine creation: the batched step's long-context attention stays on k_attn (A/B knob, tests' second path)
    bool attn_stream_one = true;     // Q3TTS_ATTN_STREAM_ONE=0: the one-split case (contexts <= 512 at >= 256 (row, kv head) pairs) back on k_attn (A/B knob): b=64 x 256 frames 4.67 -> 4.59 ms per step with it
    bool attn_keep_splits = false;   // Q3TTS_ATTN_KEEP_SPLITS at engine creation: the batched step keeps split-T attention + the combine launch (A/B knob, tests' second path)
    int seam_spin = 512;         // Q3TTS_SEAM_SPIN: polls (~0.7 us each) before an owner abandons its chunk to whoever sees the tile complete (1 forces that rescue path in the tests).  A fast-path seam completes within a few polls; the bound only matters when the launch's workgroups are not co-resident (vocoder lanes, other engines, a CU mask): 512 keeps a stalled owner off its CU after ~0.35 ms instead of round 3's ~2.9 ms
    int32_t* codes_d = nullptr;
    int32_t* codes_scratch_d = nullptr;
    int32_t* talker_pos_d = nullptr;
    int* slot_map_d = nullptr;      // [128] slots of a batched prefill over scattered slots
    float* logits_g = nullptr;      // [128][vocab] its head output before the scatter
    uint32_t* seen_d = nullptr; int seen_ld = 0;   // [B][seen_ld] bitmaps of the code0 ids each slot's utterance has emitted (repetition penalty)
    int64_t* hist_d = nullptr; size_t hist_cap = 0; // sample_hist staging (grow-only): the history ids, then their count
    SlotState* st_d = nullptr;
    std::vector<SlotState> st_h;
    int32_t* active_d = nullptr;
    int32_t* active_h = nullptr; // pinned
    int64_t* tok_d = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::unordered_map<int, hipGraphExec_t> graphs; // keyed by nb

    void* dmalloc(size_t bytes);
    // a grow-only staging buffer's regrow to n x el elements (cap counts n): the stream drains first, since the old buffer may be in flight, unless the caller just did
    template <class T> void regrow(T*& p, size_t& cap, size_t n, size_t el = 1, bool drained = false) {
        if (!drained) sync();
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        Q3_HIP_CHECK(hipMalloc((void**)&p, n * el * sizeof(T)));
        cap = n;
    }
    // final_gamma != null (MFMA path only): the last layer's finish kernel also applies the stack's final RMSNorm,
    // leaving (hi, lo) planes of the normalised rows in pl0 (+ fp32 rows in final_xn); returns true in that case
    bool run_layers(const DecStack& W, float* x, int ldx, int nb, int n_new, int slot_offset, const int* pos_dev, int pos_scalar,
                    const float* final_gamma = nullptr, float final_eps = 0.f, float* final_xn = nullptr, int final_ld_xn = 0,
                    const int* slot_map = nullptr);   // slot_map (device, nb ints): row group bi belongs to slot slot_map[bi]
    void record_step(int nb);
    bool seam_applies(const DecStack& W, int M, float* x, int ldx, bool has_slot_map) const;   // run_layers folds the finish launches of this stack pass into its GEMMs
    bool planes_in_ready = false;   // record_step -> run_layers: the sampler already wrote planes0 (gamma0 * rows) + their sums of squares (ssq_b_d)
    // returns the number of split-K slabs `out` was written as (1: plain rows).  slab_out non-null: the caller's consumer can sum slabs
    // ([nslab][M][ldo] at slab_out), which lets a 17..128-row head split K over 4x the workgroups
    int head_proj(const bf16_t* Wm, const float* x, int ldx, const float* gamma, float eps, float* xn_out, int ld_xn,
                  float* out, int ldo, int M, int N, int K, bool nt, bool planes_ready = false, int plane_row0 = 0, int plane_row_stride = 1,
                  float* slab_out = nullptr);
    int nb_in_use() const;
    void sync();
};

// A timed vocoder entry on the engine's stream: the constructor records ev0 in front of the entry's launches, stop() records ev1 behind
// them, deliver() copies the first min(n, cap) samples out, drains the stream and adds the time and the frames to the totals.  A failure
// anywhere before that leaves last_codec_ms and the totals as they were.
struct CodecTimed {
    Engine& e;
    explicit CodecTimed(Engine& en) : e(en) { Q3_HIP_CHECK(hipEventRecord(e.ev0, e.stream)); }
    void stop() { Q3_HIP_CHECK(hipEventRecord(e.ev1, e.stream)); }
    int64_t deliver(const float* src, int64_t n, float* dst, int64_t cap, int frames, hipMemcpyKind kind = hipMemcpyDeviceToHost) {
        const int64_t m = std::min(n, cap);
        if (m > 0 && dst) Q3_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)m * sizeof(float), kind, e.stream));
        e.sync();
        Q3_HIP_CHECK(hipEventElapsedTime(&e.last_codec_ms, e.ev0, e.ev1));
        e.total_codec_ms += e.last_codec_ms; e.total_codec_frames += frames;
        return n;
    }
};

} // namespace q3
