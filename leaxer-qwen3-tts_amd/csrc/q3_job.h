// q3_job.h — the job layer above the engine: what the q3tts_synthesize_* entries of q3_capi.cpp run.  A job is a batch of utterances that
// queue for the engine's slots; job_offline generates them all and vocodes at the end, job_stream delivers the audio chunk by chunk.
// Throws q3::Error; the extern "C" surface stays in q3_capi.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "q3_engine.h"

namespace q3 {

// The scheduler's stage settings, as the q3tts_engine_set_* entries leave them (each at its "none" value until set)
struct StageSettings {
    q3tts_sink sink = { 0, 0, nullptr, nullptr };   // q3tts_engine_set_sink (sample_rate 0: none)
    int32_t speed = 1000;                           // q3tts_engine_set_speed (1000: none)
    int32_t gain_cb = 0, ceiling = 0;               // q3tts_engine_set_level ((0, 0): none)
    int32_t pitch = 1000;                           // q3tts_engine_set_pitch (1000: none)
    bool loud = false;                              // q3tts_engine_set_loudness / _clear_loudness
    int32_t loud_target = 0, loud_range = 0, loud_start = 0;
    int32_t tone_n = 0;                             // q3tts_engine_set_tone (0: none)
    ToneSection tone[kToneMaxSections] = {};
};

// Everything a q3tts_synthesize_* entry passes, by name; what an entry does not have stays absent.
struct JobArgs {
    int n_utt = 0;
    const int64_t* ids = nullptr; const int32_t* offsets = nullptr;      // the texts, or
    q3tts_text_cb text_cb = nullptr; void* text_user = nullptr;          // their source (q3tts_synthesize_live_host)
    int lang = 0; const float* const* speakers = nullptr;
    const q3tts_sampling* p = nullptr; const int32_t* max_new_per_utt = nullptr; uint64_t seed = 0; int ignore_eos = 0;
    float* const* pcm_out = nullptr; int64_t pcm_cap = 0; int64_t* pcm_len = nullptr; int32_t* n_frames = nullptr; int64_t* codes_out = nullptr;
    const int64_t* instruct_ids = nullptr; const int32_t* instruct_offsets = nullptr;   // q3tts_synthesize_instruct_host
    const int32_t* prefix_ids = nullptr;                                                // q3tts_synthesize_prefixed_host
    const int64_t* prefix_codes = nullptr; const int32_t* prefix_offsets = nullptr;     // q3tts_synthesize_continue_host / _continue_stream_host
    // streaming only: the chunk cadence, the audio callback, the engine's sink and stages
    int chunk_frames = 0; q3tts_audio_cb cb = nullptr; void* user = nullptr;
    StageSettings stages;
};

void job_offline(Engine& e, const JobArgs& a);   // q3tts_synthesize_schedule_host and the entries built on it
void job_stream(Engine& e, const JobArgs& a);    // q3tts_synthesize_stream_host and the entries built on it

// The vocoder phase of a job: utterance u's codes are row u of the engine's job buffer (Engine::codec_job_codes, stride row_frames frames),
// got_frames[u] of them valid.  Shared by job_offline and q3tts_codec_decode_batch_host.
void vocoder_job(Engine& e, int n_utt, const std::vector<int32_t>& got_frames, int row_frames, float* const* pcm_out, int64_t pcm_cap, int64_t* pcm_len);

} // namespace q3
