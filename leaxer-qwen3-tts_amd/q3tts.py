"""ctypes binding of libq3tts_hip.so (C-ABI: include/q3tts.h).

Host-side mirror of the reference's TTSEngine run_* family (reference src/tts_onnx.h:196-212) plus
the batched generation entry points.  There is NO CPU fallback: if the HIP library is missing or
no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("Q3TTS_LIB") or os.path.join(_HERE, "libq3tts_hip.so")   # Q3TTS_LIB: kernel experiments (tools/)

_CFG_FIELDS = [
    ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32),
    ("head_dim", C.c_int32), ("ffn", C.c_int32), ("vocab", C.c_int32),
    ("rope_theta", C.c_float), ("rms_eps", C.c_float),
    ("cp_layers", C.c_int32), ("cp_heads", C.c_int32), ("cp_kv_heads", C.c_int32), ("cp_head_dim", C.c_int32),
    ("cp_ffn", C.c_int32), ("n_groups", C.c_int32), ("sub_vocab", C.c_int32),
    ("cp_rope_theta", C.c_float), ("cp_rms_eps", C.c_float),
    ("text_vocab", C.c_int32), ("text_hidden", C.c_int32),
    ("cd_codebook", C.c_int32), ("cd_hidden", C.c_int32), ("cd_layers", C.c_int32), ("cd_heads", C.c_int32),
    ("cd_head_dim", C.c_int32), ("cd_ffn", C.c_int32), ("cd_window", C.c_int32),
    ("cd_rope_theta", C.c_float), ("cd_rms_eps", C.c_float),
    ("cd_n_up", C.c_int32), ("cd_up_ratios", C.c_int32 * 4),
    ("cd_decoder_dim", C.c_int32), ("cd_n_blocks", C.c_int32), ("cd_up_rates", C.c_int32 * 8),
    ("cd_tconv_trim", C.c_int32),
    ("codec_eos", C.c_int32), ("suppress_begin", C.c_int32), ("suppress_end", C.c_int32),
    ("spk_enc_dim", C.c_int32), ("spk_mel", C.c_int32), ("spk_channels", C.c_int32), ("spk_scale", C.c_int32),
    ("spk_se", C.c_int32), ("spk_att", C.c_int32),
    ("cp_hidden", C.c_int32),
    # audio encoder of the 12 Hz tokenizer (enc_hidden == 0: none); enc_ratios in encoder order
    ("enc_hidden", C.c_int32), ("enc_filters", C.c_int32), ("enc_n_ratios", C.c_int32), ("enc_ratios", C.c_int32 * 4),
    ("enc_kernel", C.c_int32), ("enc_res_kernel", C.c_int32), ("enc_last_kernel", C.c_int32),
    ("enc_layers", C.c_int32), ("enc_heads", C.c_int32), ("enc_head_dim", C.c_int32), ("enc_ffn", C.c_int32), ("enc_window", C.c_int32),
    ("enc_vq_dim", C.c_int32), ("enc_codebook", C.c_int32),
    ("enc_rope_theta", C.c_float), ("enc_norm_eps", C.c_float),
]


class Config(C.Structure):
    _fields_ = _CFG_FIELDS

    def to_dict(self):
        d = {}
        for n, _ in _CFG_FIELDS:
            if n.startswith("enc_") and self.enc_hidden == 0:
                continue   # no audio encoder: the enc_* fields (all 0) are left out.  The oracle keeps its own shorter mirror of the struct and
                #            existing tests compare the two dicts, so an encoder-less config must serialise as it did before; from_dict puts the zeros back
            v = getattr(self, n)
            d[n] = list(v) if hasattr(v, "__len__") else v
        return d

    @classmethod
    def from_dict(cls, d):
        c = cls()
        for n, t in _CFG_FIELDS:
            v = d[n] if n in d or not (n.startswith("spk_") or n == "cp_hidden" or n.startswith("enc_")) else 0
            if hasattr(t, "_length_"):
                v = v or []
                arr = t()
                for i, x in enumerate(v):
                    arr[i] = x
                setattr(c, n, arr)
            else:
                setattr(c, n, v)
        return c


class Sampling(C.Structure):
    """SamplingParams, reference src/tts_onnx.h:99-105."""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
                ("repetition_penalty", C.c_float), ("max_new_tokens", C.c_int32)]

    def __init__(self, temperature=0.8, top_p=0.95, top_k=50, repetition_penalty=1.0, max_new_tokens=2048):
        super().__init__(temperature, top_p, top_k, repetition_penalty, max_new_tokens)


FLAG_NO_GRAPH = 1
FLAG_NO_FUSED_CP = 2
FLAG_FP32_CODEC = 4
FLAG_KV_ROUND_BF16 = 16   # test aid: fp32 KV storage of the bf16-rounded rows (must equal FLAG_KV_BF16 bit for bit)
FLAG_RAGGED_PREFILL = 64   # the scheduler begins the long prompts / forced begins of an admission look with one slots_begin_ragged call
FLAG_TEST_HOOKS = 32   # the engine honours the test suite's fault-injection environment hooks
FLAG_KV_BF16 = 8   # talker KV cache in bf16 (rounded on append, fp32 math); the oracle has the same switch (Oracle(kv_bf16=True))

# every symbol include/q3tts.h declares
EXPORTS = [
    "q3tts_default_config", "q3tts_create", "q3tts_create_pooled", "q3tts_kv_pool_info", "q3tts_sched_stats", "q3tts_destroy", "q3tts_last_error", "q3tts_num_tensors",
    "q3tts_tensor_info", "q3tts_set_tensor_host", "q3tts_get_tensor_host", "q3tts_fill_synthetic", "q3tts_finalize",
    "q3tts_text_project_host", "q3tts_codec_embed_host", "q3tts_cp_embed_host", "q3tts_talker_prefill_host",
    "q3tts_talker_decode_host", "q3tts_code_predictor_host", "q3tts_codec_decode_host", "q3tts_codec_decode_batch_host", "q3tts_codec_decode_len",
    "q3tts_sample_host", "q3tts_rng_uniform", "q3tts_build_prompt_host", "q3tts_slot_begin", "q3tts_decode_steps",
    "q3tts_slot_status", "q3tts_slot_codes_host", "q3tts_slot_codec_decode_host", "q3tts_slot_release",
    "q3tts_synthesize_batch_host", "q3tts_last_decode_ms", "q3tts_last_codec_ms", "q3tts_decode_step_bytes",
    "q3tts_codec_decode_dev", "q3tts_stream", "q3tts_counters", "q3tts_stage_profile", "q3tts_prefill_profile", "q3tts_codec_plane_stats", "q3tts_measure_skip_frames", "q3tts_test_poison_workspace", "q3tts_test_group_final_conv", "q3tts_test_final_conv_partials", "q3tts_codec_stream_begin", "q3tts_codec_stream_push_host", "q3tts_codec_stream_end", "q3tts_talker_prefill_dev", "q3tts_talker_decode_dev", "q3tts_code_predictor_dev", "q3tts_sample_dev", "q3tts_config_num_tensors", "q3tts_config_tensor_info", "q3tts_read_weights_config", "q3tts_load_weights_file", "q3tts_save_weights_file",
    "q3tts_tokenizer_create", "q3tts_tokenizer_destroy", "q3tts_tokenizer_load_vocab", "q3tts_tokenizer_load_merges",
    "q3tts_tokenizer_ready", "q3tts_tokenize",
    "q3tts_synthesize_clone_batch_host", "q3tts_synthesize_schedule_host", "q3tts_read_wav_host", "q3tts_resample_host", "q3tts_mel_host",
    "q3tts_has_speaker_encoder", "q3tts_speaker_encoder_host", "q3tts_extract_speaker_embedding_host",
    "q3tts_resample_gpu_host", "q3tts_mel_gpu_host", "q3tts_speaker_embed_pcm_batch_host",
    "q3tts_codec_decode_chunked_host", "q3tts_slot_codec_decode_range_host", "q3tts_slot_logits_host", "q3tts_step_logits_host",
    "q3tts_sample_hist_host", "q3tts_sample_hist_dev",
    "q3tts_codec_stream_push_batch_host", "q3tts_slots_codec_decode_new_host", "q3tts_synthesize_stream_host",
    "q3tts_build_prompt_instruct_host", "q3tts_frame_instruct_ids", "q3tts_synthesize_instruct_host",
    "q3tts_frame_rows_host", "q3tts_slot_begin_codes", "q3tts_synthesize_continue_host",
    "q3tts_prefix_create", "q3tts_prefix_create_instruct", "q3tts_prefix_info", "q3tts_prefix_release",
    "q3tts_slot_begin_prefixed", "q3tts_slots_begin_prefixed", "q3tts_slots_begin_ragged", "q3tts_synthesize_prefixed_host",
    "q3tts_slot_text_open", "q3tts_slot_text_append_host", "q3tts_slots_text_append_ids", "q3tts_slot_text_status",
    "q3tts_build_prompt_open_host", "q3tts_synthesize_live_host",
    "q3tts_config_enable_audio_encoder", "q3tts_has_audio_encoder", "q3tts_audio_encode_len", "q3tts_audio_encode_host",
    "q3tts_audio_stream_begin", "q3tts_audio_stream_push_len", "q3tts_audio_stream_push_host", "q3tts_audio_stream_push_batch_host",
    "q3tts_audio_stream_info", "q3tts_audio_stream_end",
    "q3tts_audio_stream_begin_rate", "q3tts_audio_stream_format", "q3tts_audio_stream_push_any_host", "q3tts_audio_stream_push_batch_any_host",
    "q3tts_resample_stream_emitted",
    "q3tts_audio_encode_batch_host", "q3tts_audio_encode_latents_host", "q3tts_audio_encode_batch_latents_host", "q3tts_last_audio_encode_ms", "q3tts_test_audio_encoder_transformer_host",
    "q3tts_codec_stream_prime_batch_host", "q3tts_slots_codec_prime", "q3tts_codec_stream_info", "q3tts_synthesize_continue_stream_host",
    "q3tts_sink_plan", "q3tts_sink_last_error", "q3tts_sink_emitted", "q3tts_pcm_sink_begin", "q3tts_pcm_sink_push_batch_host", "q3tts_pcm_sink_end",
    "q3tts_codec_stream_set_sink", "q3tts_codec_stream_push_batch_any_host", "q3tts_engine_set_sink",
    "q3tts_g711_encode_host", "q3tts_g711_decode_host", "q3tts_read_wav_g711_host",
    "q3tts_speed_emitted", "q3tts_speed_last_error", "q3tts_speed_window", "q3tts_speed_begin", "q3tts_speed_push_batch_host", "q3tts_speed_end",
    "q3tts_codec_stream_set_speed", "q3tts_engine_set_speed",
    "q3tts_level_gain", "q3tts_level_emitted", "q3tts_level_last_error", "q3tts_level_begin", "q3tts_level_push_batch_host", "q3tts_level_end",
    "q3tts_codec_stream_set_level", "q3tts_engine_set_level",
    "q3tts_pitch_ratio", "q3tts_pitch_emitted", "q3tts_pitch_last_error", "q3tts_pitch_begin", "q3tts_pitch_push_batch_host", "q3tts_pitch_end",
    "q3tts_codec_stream_set_pitch", "q3tts_engine_set_pitch",
    "q3tts_loudness_coeffs", "q3tts_loudness_emitted", "q3tts_loudness_lufs", "q3tts_loudness_last_error", "q3tts_loudness_begin",
    "q3tts_loudness_push_batch_host", "q3tts_loudness_end", "q3tts_codec_stream_set_loudness", "q3tts_engine_set_loudness",
    "q3tts_tone_coeffs", "q3tts_tone_parse", "q3tts_tone_last_error", "q3tts_tone_begin", "q3tts_tone_push_batch_host", "q3tts_tone_end",
    "q3tts_codec_stream_set_tone", "q3tts_engine_set_tone",
    "q3tts_create_sharing", "q3tts_weights_info",
]

# q3tts_audio_cb: int (*)(void* user, int utt, int frame_begin, int frame_end, const float* pcm, int64_t n_samples, int finished)
AUDIO_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int64, C.c_int)
# q3tts_audio_any_cb: the same with const void* pcm, read in the sink's format
AUDIO_ANY_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int)


class Sink(C.Structure):   # q3tts_sink
    _fields_ = [("sample_rate", C.c_int32), ("format", C.c_int32), ("cb", AUDIO_ANY_CB), ("user", C.c_void_p)]


# q3tts_text_cb: int (*)(void* user, int utt, int64_t* ids, int cap, int32_t* n, int32_t* closed)
TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python leaxer-qwen3-tts_amd/build.py` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    L.q3tts_default_config.argtypes = [C.c_char_p, C.POINTER(Config)]
    L.q3tts_create.restype = vp
    L.q3tts_create.argtypes = [C.POINTER(Config), i32, i32, i32, C.c_uint32]
    L.q3tts_create_pooled.restype = vp
    L.q3tts_create_pooled.argtypes = [C.POINTER(Config), i32, i32, i32, C.c_int64, C.c_uint32]
    L.q3tts_kv_pool_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.q3tts_create_sharing.restype = vp
    L.q3tts_create_sharing.argtypes = [vp, i32, i32, C.c_int64, C.c_uint32]
    L.q3tts_weights_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]
    L.q3tts_sched_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    L.q3tts_destroy.argtypes = [vp]
    L.q3tts_last_error.restype = C.c_char_p
    L.q3tts_last_error.argtypes = [vp]
    L.q3tts_num_tensors.argtypes = [vp]
    L.q3tts_tensor_info.argtypes = [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i32)]
    L.q3tts_set_tensor_host.argtypes = [vp, C.c_char_p, vp, i64]
    L.q3tts_get_tensor_host.argtypes = [vp, C.c_char_p, vp, i64]
    L.q3tts_fill_synthetic.argtypes = [vp, C.c_uint64]
    L.q3tts_finalize.argtypes = [vp]
    L.q3tts_text_project_host.argtypes = [vp, vp, i32, vp]
    L.q3tts_codec_embed_host.argtypes = [vp, vp, i32, vp]
    L.q3tts_cp_embed_host.argtypes = [vp, i64, i32, vp]
    L.q3tts_talker_prefill_host.argtypes = [vp, i32, vp, i32, vp, vp]
    L.q3tts_talker_decode_host.argtypes = [vp, i32, vp, vp, vp]
    L.q3tts_code_predictor_host.argtypes = [vp, vp, i32, i32, vp]
    L.q3tts_codec_decode_host.argtypes = [vp, vp, i32, vp, i64, C.POINTER(i64)]
    L.q3tts_codec_decode_batch_host.argtypes = [vp, i32, vp, vp, vp, i64, vp]
    L.q3tts_codec_decode_len.restype = i64
    L.q3tts_codec_decode_len.argtypes = [C.POINTER(Config), i32]
    L.q3tts_sample_host.argtypes = [vp, vp, i32, C.POINTER(Sampling), f32, i32, C.POINTER(i64)]
    L.q3tts_rng_uniform.restype = f32
    L.q3tts_rng_uniform.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.q3tts_build_prompt_host.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.q3tts_build_prompt_instruct_host.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.q3tts_frame_instruct_ids.restype = i64
    L.q3tts_frame_instruct_ids.argtypes = [vp, i64, vp, i64]
    L.q3tts_synthesize_instruct_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp,
                                                 i32, AUDIO_CB, vp, vp, vp]
    L.q3tts_slot_begin.argtypes = [vp, i32, vp, i32, vp, i32, C.POINTER(Sampling), C.c_uint64, C.c_uint32, i32]
    L.q3tts_slot_begin_codes.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, C.POINTER(Sampling), C.c_uint64, C.c_uint32, i32]
    L.q3tts_frame_rows_host.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.q3tts_synthesize_continue_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp, vp, vp]
    L.q3tts_synthesize_continue_stream_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp, vp, vp,
                                                        i32, AUDIO_CB, vp]
    L.q3tts_codec_stream_prime_batch_host.argtypes = [vp, i32, vp, vp, vp]
    L.q3tts_slots_codec_prime.argtypes = [vp, i32, vp, vp]
    L.q3tts_codec_stream_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.q3tts_prefix_create.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.q3tts_prefix_create_instruct.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.q3tts_prefix_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i64)]
    L.q3tts_prefix_release.argtypes = [vp, i32]
    L.q3tts_slot_begin_prefixed.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, C.POINTER(Sampling), C.c_uint64, C.c_uint32, i32]
    L.q3tts_slots_begin_prefixed.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, C.POINTER(Sampling), C.c_uint64, vp, i32]
    L.q3tts_slots_begin_ragged.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Sampling), C.c_uint64, vp, i32]
    L.q3tts_synthesize_prefixed_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp,
                                                 i32, AUDIO_CB, vp, vp]
    L.q3tts_decode_steps.argtypes = [vp, i32]
    L.q3tts_slot_text_open.argtypes = [vp, i32]
    L.q3tts_slot_text_append_host.argtypes = [vp, i32, vp, i32, i32]
    L.q3tts_slots_text_append_ids.argtypes = [vp, i32, vp, vp, vp, vp]
    L.q3tts_slot_text_status.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.q3tts_build_prompt_open_host.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.q3tts_synthesize_live_host.argtypes = [vp, i32, TEXT_CB, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp,
                                             i32, AUDIO_CB, vp]
    L.q3tts_slot_status.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.q3tts_slot_codes_host.argtypes = [vp, i32, vp, i32]
    L.q3tts_slot_codec_decode_host.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
    L.q3tts_slot_release.argtypes = [vp, i32]
    L.q3tts_slot_logits_host.argtypes = [vp, i32, vp, vp]
    L.q3tts_step_logits_host.argtypes = [vp, i32, vp, i32]
    L.q3tts_synthesize_batch_host.argtypes = [vp, i32, vp, vp, i32, C.POINTER(Sampling), C.c_uint64, i32,
                                              vp, i64, vp, vp, vp]
    L.q3tts_last_decode_ms.argtypes = [vp, C.POINTER(f32), C.POINTER(i32)]
    L.q3tts_last_codec_ms.argtypes = [vp, C.POINTER(f32)]
    L.q3tts_stage_profile.argtypes = [vp, i32, C.POINTER(C.c_double)]
    L.q3tts_codec_plane_stats.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.q3tts_counters.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i64), i32]
    L.q3tts_decode_step_bytes.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.q3tts_read_weights_config.argtypes = [C.c_char_p, C.POINTER(Config)]
    L.q3tts_load_weights_file.argtypes = [vp, C.c_char_p]
    L.q3tts_save_weights_file.argtypes = [vp, C.c_char_p]
    L.q3tts_synthesize_clone_batch_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), C.c_uint64, i32, vp, i64, vp, vp, vp]
    L.q3tts_synthesize_schedule_host.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(Sampling), vp, C.c_uint64, i32, vp, i64, vp, vp, vp]
    L.q3tts_read_wav_host.argtypes = [C.c_char_p, vp, i64, C.POINTER(i64), C.POINTER(C.c_int32)]
    L.q3tts_resample_host.restype = i64
    L.q3tts_resample_host.argtypes = [vp, i64, i32, i32, vp, i64]
    L.q3tts_mel_host.argtypes = [vp, i64, vp, i64, C.POINTER(C.c_int32)]
    L.q3tts_has_speaker_encoder.argtypes = [vp]
    L.q3tts_speaker_encoder_host.argtypes = [vp, vp, i32, vp]
    L.q3tts_extract_speaker_embedding_host.argtypes = [vp, C.c_char_p, vp]
    L.q3tts_resample_gpu_host.restype = i64
    L.q3tts_resample_gpu_host.argtypes = [vp, vp, i64, i32, i32, vp, i64]
    L.q3tts_mel_gpu_host.argtypes = [vp, vp, i64, i32, vp, i64, C.POINTER(C.c_int32)]
    L.q3tts_speaker_embed_pcm_batch_host.argtypes = [vp, i32, vp, vp, vp, vp]
    L.q3tts_config_enable_audio_encoder.argtypes = [C.POINTER(Config)]
    L.q3tts_has_audio_encoder.argtypes = [vp]
    L.q3tts_audio_encode_len.restype = i64
    L.q3tts_audio_encode_len.argtypes = [vp, i64]
    L.q3tts_audio_encode_host.argtypes = [vp, vp, i64, vp, i32, C.POINTER(C.c_int32)]
    L.q3tts_audio_encode_batch_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.q3tts_audio_encode_batch_latents_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.q3tts_last_audio_encode_ms.argtypes = [vp, C.POINTER(f32)]
    L.q3tts_audio_stream_begin.argtypes = [vp, i64, C.POINTER(C.c_int)]
    L.q3tts_audio_stream_push_len.argtypes = [vp, i32, i64, i32]
    L.q3tts_audio_stream_push_host.argtypes = [vp, i32, vp, i64, i32, vp, i32, C.POINTER(C.c_int32)]
    L.q3tts_audio_stream_push_batch_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.q3tts_audio_stream_info.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.q3tts_audio_stream_end.argtypes = [vp, i32]
    L.q3tts_audio_stream_begin_rate.argtypes = [vp, i32, i32, i64, C.POINTER(C.c_int)]
    L.q3tts_audio_stream_format.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
    L.q3tts_audio_stream_push_any_host.argtypes = [vp, i32, vp, i64, i32, vp, i32, C.POINTER(C.c_int32)]
    L.q3tts_audio_stream_push_batch_any_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.q3tts_resample_stream_emitted.argtypes = [i32, i32, i64, i32]
    L.q3tts_resample_stream_emitted.restype = i64
    L.q3tts_audio_encode_latents_host.argtypes = [vp, vp, i64, vp, vp, i32, C.POINTER(C.c_int32)]
    L.q3tts_test_audio_encoder_transformer_host.argtypes = [vp, vp, i32, vp]
    L.q3tts_codec_decode_chunked_host.argtypes = [vp, vp, i32, i32, i32, vp, i64, C.POINTER(i64)]
    L.q3tts_slot_codec_decode_range_host.argtypes = [vp, i32, i32, i32, i32, vp, i64, C.POINTER(i64)]
    L.q3tts_tokenizer_create.restype = vp
    L.q3tts_tokenizer_create.argtypes = []
    L.q3tts_tokenizer_destroy.restype = None
    L.q3tts_tokenizer_destroy.argtypes = [vp]
    L.q3tts_tokenizer_load_vocab.argtypes = [vp, C.c_char_p]
    L.q3tts_tokenizer_load_merges.argtypes = [vp, C.c_char_p]
    L.q3tts_tokenizer_ready.argtypes = [vp]
    L.q3tts_tokenize.restype = i64
    L.q3tts_tokenize.argtypes = [vp, C.c_char_p, i64, C.POINTER(C.c_int32), i64]
    _lib = L
    return L


_KINDS = ("w", "norm", "b", "scale", "snake")


def tensor_specs(cfg):
    """(name, shape, kind) of every tensor the config implies — the engine's registry, from the library, no GPU needed."""
    L = lib()
    L.q3tts_config_num_tensors.argtypes = [C.c_void_p]
    L.q3tts_config_tensor_info.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    n = L.q3tts_config_num_tensors(C.byref(cfg))
    if n <= 0:
        raise ValueError("model config out of range")
    out, name, shape, nd, kind = [], C.create_string_buffer(256), (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(0)
    for i in range(n):
        if L.q3tts_config_tensor_info(C.byref(cfg), i, name, 256, shape, C.byref(nd), C.byref(kind)) != 0:
            raise RuntimeError("q3tts_config_tensor_info failed")
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value)), _KINDS[kind.value]))
    return out


def default_config(name="0.6b"):
    c = Config()
    if lib().q3tts_default_config(name.encode(), C.byref(c)) != 0:
        raise ValueError(f"unknown config {name!r}")
    return c


def enable_audio_encoder(cfg):
    """q3tts_config_enable_audio_encoder: the 12 Hz tokenizer's encoder dimensions filled into cfg (returned for chaining)"""
    if lib().q3tts_config_enable_audio_encoder(C.byref(cfg)) != 0:
        raise ValueError("q3tts_config_enable_audio_encoder failed")
    return cfg


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One engine = one GPU, `max_batch` utterance slots, device-resident weights + KV cache."""

    def __init__(self, cfg, device=0, max_batch=1, max_ctx=2304, flags=0, kv_pool_tokens=0):
        """kv_pool_tokens > 0 bounds the talker's KV page pool (q3tts_create_pooled); 0 reserves max_batch x max_ctx."""
        self.L = lib()
        self.cfg = cfg
        self.max_batch = max_batch
        self.max_ctx = max_ctx
        self.flags = flags
        self.h = self.L.q3tts_create_pooled(C.byref(cfg), device, max_batch, max_ctx, kv_pool_tokens, flags)
        if not self.h:
            raise RuntimeError("q3tts_create failed: " + self.L.q3tts_last_error(None).decode())

    def share(self, max_batch=1, max_ctx=None, flags=None, kv_pool_tokens=0):
        """A second engine on this engine's GPU that holds this engine's finalized weights instead of a copy (q3tts_create_sharing).
        Slots, KV pool, workspaces, streams and graphs are its own; it is ready at once.  None: this engine's value.  May be called
        while this engine generates on another thread.  While both live, the weights cannot be changed on either."""
        other = Engine.__new__(Engine)
        other.L = self.L
        other.cfg = self.cfg
        other.max_batch = max_batch
        other.max_ctx = self.max_ctx if max_ctx is None else max_ctx
        other.flags = self.flags if flags is None else flags
        other.h = self.L.q3tts_create_sharing(self.h, max_batch, other.max_ctx, kv_pool_tokens, other.flags)
        if not other.h:
            raise RuntimeError("q3tts_create_sharing failed: " + self.L.q3tts_last_error(None).decode())
        return other

    def weights_info(self):
        """{'shared_bytes': HBM of the weight set (registry + derived copies), 'holders': engines that hold it,
        'private_weight_bytes': weights or derived copies this engine owns outside the set (0: everything is shared)}"""
        a, b, c = C.c_int64(), C.c_int32(), C.c_int64()
        self._ck(self.L.q3tts_weights_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"shared_bytes": a.value, "holders": b.value, "private_weight_bytes": c.value}

    def kv_pool_info(self):
        """(tokens per page, pages in the pool, pages free)"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.L.q3tts_kv_pool_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def sched_stats(self):
        """(admitted, preempted, peak live) of the last synthesize_batch call"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(self.L.q3tts_sched_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "h", None):
            self.L.q3tts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.q3tts_last_error(self.h).decode())
        return rc

    # ---- weights ----
    def tensor_infos(self):
        out = []
        name = C.create_string_buffer(128)
        shape = (C.c_int64 * 4)()
        nd = C.c_int(0)
        for i in range(self.L.q3tts_num_tensors(self.h)):
            self._ck(self.L.q3tts_tensor_info(self.h, i, name, 128, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return out

    def set_tensor(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        self._ck(self.L.q3tts_set_tensor_host(self.h, name.encode(), _p(a), a.size))

    def get_tensor(self, name, shape):
        out = np.empty(shape, np.float32)
        self._ck(self.L.q3tts_get_tensor_host(self.h, name.encode(), _p(out), out.size))
        return out

    def load(self, weights):
        for k, v in weights.items():
            self.set_tensor(k, v)
        self.finalize()

    def fill_synthetic(self, seed=0):
        self._ck(self.L.q3tts_fill_synthetic(self.h, seed))
        self.finalize()

    def finalize(self):
        self._ck(self.L.q3tts_finalize(self.h))

    def save_weights(self, path):
        self._ck(self.L.q3tts_save_weights_file(self.h, os.fsencode(path)))

    def load_weights(self, path):
        self._ck(self.L.q3tts_load_weights_file(self.h, os.fsencode(path)))

    # ---- session-shaped ----
    def text_project(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty((ids.size, self.cfg.hidden), np.float32)
        self._ck(self.L.q3tts_text_project_host(self.h, _p(ids), ids.size, _p(out)))
        return out

    def codec_embed(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty((ids.size, self.cfg.hidden), np.float32)
        self._ck(self.L.q3tts_codec_embed_host(self.h, _p(ids), ids.size, _p(out)))
        return out

    def cp_embed(self, tok, step):
        out = np.empty(self.cfg.hidden, np.float32)
        self._ck(self.L.q3tts_cp_embed_host(self.h, int(tok), int(step), _p(out)))
        return out

    def _frames(self, codes, what):
        """codes as a contiguous int64 [n][n_groups] array"""
        c = np.ascontiguousarray(codes, dtype=np.int64)
        if c.size == 0:
            return c.reshape(0, self.cfg.n_groups)
        if c.ndim != 2 or c.shape[1] != self.cfg.n_groups:
            raise ValueError("%s: expected [frames][%d] codes, got shape %s" % (what, self.cfg.n_groups, c.shape))
        return c

    def frame_rows(self, codes, frame0=0, trailing=None):
        """talker input rows of given frames (q3tts_frame_rows_host): codes [n][n_groups] -> [n][hidden]; row i carries the text row
        trailing[frame0 + i] while that index exists, then tts_pad — what the fused loop feeds the talker after sampling that frame"""
        c = self._frames(codes, "frame_rows")
        if int(frame0) < 0:
            raise ValueError("frame_rows: frame0 must be >= 0")
        out = np.empty((c.shape[0], self.cfg.hidden), np.float32)
        if c.shape[0] == 0:
            return out
        t = None
        if trailing is not None:
            t = np.ascontiguousarray(trailing, dtype=np.float32)
            if t.size and (t.ndim != 2 or t.shape[1] != self.cfg.hidden):
                raise ValueError("frame_rows: trailing must be [rows][%d]" % self.cfg.hidden)
        nt = 0 if t is None or t.size == 0 else t.shape[0]
        self._ck(self.L.q3tts_frame_rows_host(self.h, _p(c), c.shape[0], int(frame0), _p(t) if nt else None, nt, _p(out)))
        return out

    def prefill(self, embeds, slot=0):
        """run_prefill over embeds [S][hidden], 1 <= S <= max_ctx (more than 16 rows: the chunked long-prompt path)"""
        e = np.ascontiguousarray(embeds, dtype=np.float32)
        S = e.shape[0]
        logits = np.empty((S, self.cfg.vocab), np.float32)
        lh = np.empty(self.cfg.hidden, np.float32)
        self._ck(self.L.q3tts_talker_prefill_host(self.h, slot, _p(e), S, _p(logits), _p(lh)))
        return logits, lh

    def decode(self, embed, slot=0):
        e = np.ascontiguousarray(embed, dtype=np.float32)
        logits = np.empty(self.cfg.vocab, np.float32)
        lh = np.empty(self.cfg.hidden, np.float32)
        self._ck(self.L.q3tts_talker_decode_host(self.h, slot, _p(e), _p(logits), _p(lh)))
        return logits, lh

    def code_predictor(self, seq, step):
        s = np.ascontiguousarray(seq, dtype=np.float32)
        logits = np.empty(self.cfg.sub_vocab, np.float32)
        self._ck(self.L.q3tts_code_predictor_host(self.h, _p(s), s.shape[0], int(step), _p(logits)))
        return logits

    def codec_decode_len(self, F):
        return int(self.L.q3tts_codec_decode_len(C.byref(self.cfg), F))

    def codec_decode(self, codes):
        c = np.ascontiguousarray(codes, dtype=np.int64)
        n = max(self.codec_decode_len(c.shape[0]), 1)   # F = 0 is rejected by the library, not by numpy
        pcm = np.empty(n, np.float32)
        out_len = C.c_int64(0)
        self._ck(self.L.q3tts_codec_decode_host(self.h, _p(c), c.shape[0], _p(pcm), n, C.byref(out_len)))
        return pcm[: out_len.value]

    def codec_decode_batch(self, codes_list):
        """the vocoder phase of a job on its own: one [F_u][n_groups] code array per utterance -> one PCM array each (batched blocks of
        similar length + single utterances over the side lanes, exactly as synthesize_batch vocodes its results)"""
        n = len(codes_list)
        if n == 0:
            return []
        cs = [np.ascontiguousarray(c_, np.int64).reshape(-1, self.cfg.n_groups) for c_ in codes_list]
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([c_.shape[0] for c_ in cs])
        flat = np.ascontiguousarray(np.concatenate(cs)) if offs[-1] else np.zeros((1, self.cfg.n_groups), np.int64)
        cap = max(self.codec_decode_len(max(c_.shape[0] for c_ in cs)), 1)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        self._ck(self.L.q3tts_codec_decode_batch_host(self.h, n, _p(flat), _p(offs), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len)))
        return [pcm[i][: pcm_len[i]] for i in range(n)]

    def codec_decode_chunked(self, codes, chunk_frames, left_context):
        """exact chunked decode: equals codec_decode(codes) when left_context covers the history"""
        c = np.ascontiguousarray(codes, dtype=np.int64)
        n = max(self.codec_decode_len(c.shape[0]), 1)
        pcm = np.empty(n, np.float32)
        out_len = C.c_int64(0)
        self._ck(self.L.q3tts_codec_decode_chunked_host(self.h, _p(c), c.shape[0], chunk_frames, left_context, _p(pcm), n, C.byref(out_len)))
        return pcm[: out_len.value]

    def codec_stream_begin(self, max_frames, sample_rate=24000, dtype="float32", speed=None, gain_db=None, ceiling=None,
                           loudness=None, loudness_range=None, loudness_start=None, *, tone=None, pitch=None):
        """streaming vocoder with carried state: -> stream id (q3tts_codec_stream_begin).  sample_rate / dtype other than 24000 /
        float32 give the stream a sink (q3tts_codec_stream_set_sink): codec_stream_push_batch then delivers at that rate, as float32
        or int16.  speed (permille, 500 .. 2000; None or 1000: none) gives it a stretcher ahead of the sink
        (q3tts_codec_stream_set_speed).  gain_db / ceiling (level_params: rounded to centibels / permille; None: 0) give it a level
        stage between the two (q3tts_codec_stream_set_level).  pitch (permille, 500 .. 2000; None or 1000: none) gives it a pitch
        stage in front of them all (q3tts_codec_stream_set_pitch).  loudness (LUFS, -40 .. -5, or 0: meter only; None: none) with
        loudness_range / loudness_start (dB; loudness_params) gives it a loudness stage between the stretcher and the level stage
        (q3tts_codec_stream_set_loudness).  tone (a spec string or a list of sections, tone_sections; None: none) gives it a tone
        stage between the stretcher and the loudness stage (q3tts_codec_stream_set_tone)."""
        fmt = _pcm_format(dtype)
        sid = C.c_int(-1)
        self.L.q3tts_codec_stream_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_codec_stream_begin(self.h, int(max_frames), C.byref(sid)))
        self.__dict__.setdefault("_codec_stream_fmt", {}).pop(sid.value, None)
        if int(sample_rate) != 24000 or fmt != PCM_F32:
            try:
                self.codec_stream_set_sink(sid.value, sample_rate, dtype)
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        if speed is not None:
            try:
                self.codec_stream_set_speed(sid.value, speed)
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        if gain_db is not None or ceiling is not None:
            try:
                self.codec_stream_set_level(sid.value, *level_params(gain_db, ceiling))
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        if pitch is not None:
            try:
                self.codec_stream_set_pitch(sid.value, pitch)
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        if loudness is not None:
            try:
                self.codec_stream_set_loudness(sid.value, *loudness_params(loudness, loudness_range, loudness_start))
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        if tone is not None:
            try:
                self.codec_stream_set_tone(sid.value, tone)
            except Exception:
                self.codec_stream_end(sid.value)
                raise
        return sid.value

    def codec_stream_set_tone(self, sid, tone):
        """q3tts_codec_stream_set_tone: tone a spec string or a list of sections (tone_sections); refused once the stream has delivered
        a sample; None or no sections take the stage away"""
        arr = _tone_array(tone)
        self.L.q3tts_codec_stream_set_tone.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p]
        self._ck(self.L.q3tts_codec_stream_set_tone(self.h, int(sid), arr.shape[0], _p(arr) if arr.shape[0] else None))
        d = self.__dict__.setdefault("_codec_stream_tone", {})
        if arr.shape[0] == 0:
            d.pop(int(sid), None)
        else:
            d[int(sid)] = arr

    # ---- the tone stage on its own (include/q3tts.h "tone") ----
    def tone_begin(self, tone):
        """a stage that takes 24 kHz float32 and delivers it through a cascade of 1 .. 8 biquads; tone a spec string or a list of
        sections (tone_sections) -> stage id"""
        arr = _tone_array(tone)
        sid = C.c_int(-1)
        self.L.q3tts_tone_begin.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_tone_begin(self.h, arr.shape[0], _p(arr) if arr.shape[0] else None, C.byref(sid)))
        return sid.value

    def tone_push_batch(self, ids, pcm_list, finish=None):
        """more 24 kHz samples for many tone stages in one launch (q3tts_tone_push_batch_host); finish: one flag per stage (nothing is
        flushed: the stage only closes) -> one float32 array per stage, as long as its input"""
        n = len(ids)
        if n == 0:
            return []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("tone_push_batch: one sample array (and one finish flag) per stage")
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = int(lens.max())
        outs = [np.empty(max(cap, 1), np.float32) for _ in range(n)]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        out_len = np.zeros(n, np.int64)
        self.L.q3tts_tone_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._ck(self.L.q3tts_tone_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                   C.cast(optr, C.c_void_p), cap, _p(out_len)))
        return [outs[i][: out_len[i]] for i in range(n)]

    def tone_end(self, stage_id):
        self.L.q3tts_tone_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_tone_end(self.h, int(stage_id)))

    def set_tone(self, tone=None):
        """q3tts_engine_set_tone: the streaming entries deliver through a tone stage; None takes it away"""
        arr = _tone_array(tone)
        self.L.q3tts_engine_set_tone.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        self._ck(self.L.q3tts_engine_set_tone(self.h, arr.shape[0], _p(arr) if arr.shape[0] else None))

    def codec_stream_set_loudness(self, sid, target_dlufs, range_cb=200, start_cb=0):
        """q3tts_codec_stream_set_loudness: target in tenths of a LUFS (0: meter only), range and start gain in centibels; refused once
        the stream has delivered a sample"""
        self.L.q3tts_codec_stream_set_loudness.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int32]
        self._ck(self.L.q3tts_codec_stream_set_loudness(self.h, int(sid), int(target_dlufs), int(range_cb), int(start_cb)))
        self.__dict__.setdefault("_codec_stream_loud", {})[int(sid)] = (int(target_dlufs), int(range_cb), int(start_cb))

    # ---- the loudness stage on its own (include/q3tts.h "loudness") ----
    def loudness_begin(self, target_dlufs, range_cb=200, start_cb=0):
        """a stage that takes 24 kHz float32, measures it (BS.1770) and delivers it with a gain that moves towards target_dlufs
        (tenths of a LUFS, -400 .. -50; 0: meter only) by at most range_cb centibels, starting from start_cb -> stage id"""
        sid = C.c_int(-1)
        self.L.q3tts_loudness_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_loudness_begin(self.h, int(target_dlufs), int(range_cb), int(start_cb), C.byref(sid)))
        return sid.value

    def loudness_push_batch(self, ids, pcm_list, finish=None, report=False):
        """more 24 kHz samples for many loudness stages in one launch (q3tts_loudness_push_batch_host); finish: one flag per stage
        (its tail is flushed with this push) -> one float32 array per stage; report: -> (samples, energies int64, gains float32) per
        stage, E_b and G_b of the sub-blocks the push completed"""
        n = len(ids)
        if n == 0:
            return []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("loudness_push_batch: one sample array (and one finish flag) per stage")
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = int(lens.max()) + 2400                 # the push plus what the stage held back
        outs = [np.empty(cap, np.float32) for _ in range(n)]
        es = [np.zeros(x.size // 2400 + 1, np.int64) for x in xs]
        gs = [np.zeros(x.size // 2400 + 1, np.float32) for x in xs]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        eptr = (C.c_void_p * n)(*[a.ctypes.data for a in es])
        gptr = (C.c_void_p * n)(*[a.ctypes.data for a in gs])
        out_len, nb = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.L.q3tts_loudness_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_loudness_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                       C.cast(optr, C.c_void_p), cap, _p(out_len), C.cast(eptr, C.c_void_p) if report else None,
                                                       C.cast(gptr, C.c_void_p) if report else None, _p(nb)))
        if report:
            return [(outs[i][: out_len[i]], es[i][: nb[i]], gs[i][: nb[i]]) for i in range(n)]
        return [outs[i][: out_len[i]] for i in range(n)]

    def loudness_end(self, stage_id):
        self.L.q3tts_loudness_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_loudness_end(self.h, int(stage_id)))

    def set_loudness(self, target_dlufs=None, range_cb=200, start_cb=0):
        """q3tts_engine_set_loudness: the streaming entries deliver through a loudness stage; None takes it away"""
        self.L.q3tts_engine_set_loudness.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int32]
        if target_dlufs is None:
            self._ck(self.L.q3tts_engine_set_loudness(self.h, 0, 0, 0, 0))
        else:
            self._ck(self.L.q3tts_engine_set_loudness(self.h, 1, int(target_dlufs), int(range_cb), int(start_cb)))

    def codec_stream_set_pitch(self, sid, ratio):
        """q3tts_codec_stream_set_pitch: ratio in permille; refused once the stream has delivered a sample; 1000 takes the stage away"""
        self.L.q3tts_codec_stream_set_pitch.argtypes = [C.c_void_p, C.c_int, C.c_int32]
        self._ck(self.L.q3tts_codec_stream_set_pitch(self.h, int(sid), int(ratio)))
        d = self.__dict__.setdefault("_codec_stream_pitch", {})
        if int(ratio) == 1000:
            d.pop(int(sid), None)
        else:
            d[int(sid)] = int(ratio)

    # ---- the pitch stage on its own (include/q3tts.h "pitch") ----
    def pitch_begin(self, ratio):
        """a stage that takes 24 kHz float32 and delivers it at the same length with the fundamental multiplied by ratio / 1000
        (permille, 500 .. 2000, not 1000) -> stage id"""
        sid = C.c_int(-1)
        self.L.q3tts_pitch_begin.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_pitch_begin(self.h, int(ratio), C.byref(sid)))
        return sid.value

    def pitch_push_batch(self, ids, pcm_list, finish=None):
        """more 24 kHz samples for many pitch stages in one launch (q3tts_pitch_push_batch_host); finish: one flag per stage (its
        tail is flushed with this push) -> one float32 array per stage"""
        n = len(ids)
        if n == 0:
            return []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("pitch_push_batch: one sample array (and one finish flag) per stage")
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = int(lens.max()) + 1248                 # the push plus what the stage held back
        outs = [np.empty(cap, np.float32) for _ in range(n)]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        out_len = np.zeros(n, np.int64)
        self.L.q3tts_pitch_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._ck(self.L.q3tts_pitch_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                    C.cast(optr, C.c_void_p), cap, _p(out_len)))
        return [outs[i][: out_len[i]] for i in range(n)]

    def pitch_end(self, stage_id):
        self.L.q3tts_pitch_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_pitch_end(self.h, int(stage_id)))

    def set_pitch(self, ratio=1000):
        """q3tts_engine_set_pitch: the streaming entries deliver through a pitch stage; 1000 takes it away"""
        self.L.q3tts_engine_set_pitch.argtypes = [C.c_void_p, C.c_int32]
        self._ck(self.L.q3tts_engine_set_pitch(self.h, int(ratio)))

    def codec_stream_set_level(self, sid, gain_cb, ceiling_permille):
        """q3tts_codec_stream_set_level: gain in centibels, ceiling in permille (0: gain only); refused once the stream has delivered a
        sample; (0, 0) takes the stage away"""
        self.L.q3tts_codec_stream_set_level.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32]
        self._ck(self.L.q3tts_codec_stream_set_level(self.h, int(sid), int(gain_cb), int(ceiling_permille)))
        d = self.__dict__.setdefault("_codec_stream_level", {})
        if int(gain_cb) == 0 and int(ceiling_permille) == 0:
            d.pop(int(sid), None)
        else:
            d[int(sid)] = (int(gain_cb), int(ceiling_permille))

    # ---- the output-level stage on its own (include/q3tts.h "output level") ----
    def level_begin(self, gain_cb, ceiling_permille):
        """a stage that takes 24 kHz float32 and delivers it 10^(gain_cb / 200) times as loud, behind a look-ahead limiter at
        ceiling_permille / 1000 when that is not 0 (gain_cb: -600 .. 400; ceiling_permille: 0 .. 1000; not both 0) -> stage id"""
        sid = C.c_int(-1)
        self.L.q3tts_level_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_level_begin(self.h, int(gain_cb), int(ceiling_permille), C.byref(sid)))
        return sid.value

    def level_push_batch(self, ids, pcm_list, finish=None):
        """more 24 kHz samples for many level stages in one launch (q3tts_level_push_batch_host); finish: one flag per stage (its
        tail is flushed with this push) -> one float32 array per stage"""
        n = len(ids)
        if n == 0:
            return []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("level_push_batch: one sample array (and one finish flag) per stage")
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = int(lens.max()) + 128                  # the push plus what a limiter held back
        outs = [np.empty(cap, np.float32) for _ in range(n)]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        out_len = np.zeros(n, np.int64)
        self.L.q3tts_level_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._ck(self.L.q3tts_level_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                    C.cast(optr, C.c_void_p), cap, _p(out_len)))
        return [outs[i][: out_len[i]] for i in range(n)]

    def level_end(self, stage_id):
        self.L.q3tts_level_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_level_end(self.h, int(stage_id)))

    def set_level(self, gain_cb=0, ceiling_permille=0):
        """q3tts_engine_set_level: the streaming entries deliver through a level stage; (0, 0) takes it away"""
        self.L.q3tts_engine_set_level.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        self._ck(self.L.q3tts_engine_set_level(self.h, int(gain_cb), int(ceiling_permille)))

    def codec_stream_set_speed(self, sid, speed):
        """q3tts_codec_stream_set_speed: speed in permille; refused once the stream has delivered a sample; 1000 takes the stage away"""
        self.L.q3tts_codec_stream_set_speed.argtypes = [C.c_void_p, C.c_int, C.c_int32]
        self._ck(self.L.q3tts_codec_stream_set_speed(self.h, int(sid), int(speed)))
        d = self.__dict__.setdefault("_codec_stream_speed", {})
        if int(speed) == 1000:
            d.pop(int(sid), None)
        else:
            d[int(sid)] = int(speed)

    # ---- the speaking-rate stage on its own (include/q3tts.h "speaking rate") ----
    def speed_begin(self, speed):
        """a stretcher that takes 24 kHz float32 and delivers it speed / 1000 times as fast (speed: permille, 500 .. 2000, not 1000)
        -> stretcher id"""
        sid = C.c_int(-1)
        self.L.q3tts_speed_begin.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_speed_begin(self.h, int(speed), C.byref(sid)))
        self.__dict__.setdefault("_speed_of", {})[sid.value] = int(speed)
        return sid.value

    def speed_push_batch(self, ids, pcm_list, finish=None, want_offsets=False):
        """more 24 kHz samples for many stretchers in one launch (q3tts_speed_push_batch_host); finish: one flag per stretcher (its
        tail is flushed with this push) -> one float32 array per stretcher; want_offsets: (arrays, per stretcher the int32 offsets
        of the frames the push completed)"""
        n = len(ids)
        if n == 0:
            return ([], []) if want_offsets else []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("speed_push_batch: one sample array (and one finish flag) per stretcher")
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = (int(lens.max()) + 1320) * 2 + 720     # the slowest speed doubles the push plus what the stretcher held back
        outs = [np.empty(cap, np.float32) for _ in range(n)]
        offs = [np.empty(cap // 360 + 1, np.int32) for _ in range(n)]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        fptr = (C.c_void_p * n)(*[o.ctypes.data for o in offs])
        out_len, n_offs = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.L.q3tts_speed_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_speed_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                    C.cast(optr, C.c_void_p), cap, _p(out_len), C.cast(fptr, C.c_void_p) if want_offsets else None, _p(n_offs)))
        res = [outs[i][: out_len[i]] for i in range(n)]
        return (res, [offs[i][: n_offs[i]] for i in range(n)]) if want_offsets else res

    def speed_end(self, stretcher_id):
        self.L.q3tts_speed_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_speed_end(self.h, int(stretcher_id)))
        self.__dict__.setdefault("_speed_of", {}).pop(int(stretcher_id), None)

    def set_speed(self, speed=None):
        """q3tts_engine_set_speed: the streaming entries deliver time-stretched (speed: permille); None or 1000 takes the stage away"""
        self.L.q3tts_engine_set_speed.argtypes = [C.c_void_p, C.c_int32]
        self._ck(self.L.q3tts_engine_set_speed(self.h, 1000 if speed is None else int(speed)))

    def codec_stream_set_sink(self, sid, sample_rate, dtype="float32"):
        """q3tts_codec_stream_set_sink: refused once the stream has delivered a sample; 24000 / float32 takes the sink away"""
        fmt = _pcm_format(dtype)
        self.L.q3tts_codec_stream_set_sink.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int]
        self._ck(self.L.q3tts_codec_stream_set_sink(self.h, int(sid), int(sample_rate), fmt))
        d = self.__dict__.setdefault("_codec_stream_fmt", {})
        if int(sample_rate) == 24000 and fmt == PCM_F32:
            d.pop(int(sid), None)
        else:
            d[int(sid)] = (int(sample_rate), fmt)

    # ---- PCM sinks on their own (include/q3tts.h "audio out at the sink's rate") ----
    def pcm_sink_begin(self, sample_rate, dtype="float32"):
        """a sink that takes 24 kHz float32 and delivers sample_rate (4000 .. 192000) as float32, int16 or G.711 bytes ("mulaw" / "alaw", np.uint8) -> sink id"""
        fmt = _pcm_format(dtype)
        sid = C.c_int(-1)
        self.L.q3tts_pcm_sink_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_int)]
        self._ck(self.L.q3tts_pcm_sink_begin(self.h, int(sample_rate), fmt, C.byref(sid)))
        self.__dict__.setdefault("_pcm_sink_fmt", {})[sid.value] = (int(sample_rate), fmt)
        return sid.value

    def pcm_sink_push_batch(self, ids, pcm_list, finish=None):
        """more 24 kHz samples for many sinks in one launch (q3tts_pcm_sink_push_batch_host); finish: one flag per sink (its tail is
        flushed with this push) -> one array per sink in its own dtype"""
        n = len(ids)
        if n == 0:
            return []
        if len(pcm_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("pcm_sink_push_batch: one sample array (and one finish flag) per sink")
        fmts = self.__dict__.setdefault("_pcm_sink_fmt", {})
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in pcm_list]
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        lens = np.array([x.size for x in xs], np.int64)
        cap = 1
        for i in range(n):
            rate, _ = fmts.get(int(ids[i]), (192000, PCM_F32))
            cap = max(cap, (int(lens[i]) + 200) * max(rate, 24000) // 24000 + 8)
        outs = [np.empty(cap, _PCM_NP[fmts.get(int(ids[i]), (0, PCM_F32))[1]]) for i in range(n)]
        xptr = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        out_len = np.zeros(n, np.int64)
        self.L.q3tts_pcm_sink_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._ck(self.L.q3tts_pcm_sink_push_batch_host(self.h, n, _p(np.ascontiguousarray(ids, np.int32)), C.cast(xptr, C.c_void_p), _p(lens), _p(fin),
                                                       C.cast(optr, C.c_void_p), cap, _p(out_len)))
        return [outs[i][: out_len[i]] for i in range(n)]

    def pcm_sink_end(self, sink_id):
        self.L.q3tts_pcm_sink_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_pcm_sink_end(self.h, int(sink_id)))
        self.__dict__.setdefault("_pcm_sink_fmt", {}).pop(int(sink_id), None)

    def set_sink(self, sample_rate=None, dtype="float32", on_audio=None):
        """q3tts_engine_set_sink: the streaming entries deliver through on_audio(utt, frame_begin, frame_end, pcm, finished) at
        sample_rate as float32, int16 or G.711 bytes ("mulaw" / "alaw", np.uint8); sample_rate None takes the sink away.  An exception in on_audio cancels the job; it is kept
        in self._sink_raised for the caller to re-raise."""
        self.L.q3tts_engine_set_sink.argtypes = [C.c_void_p, C.c_void_p]
        if sample_rate is None:
            self._ck(self.L.q3tts_engine_set_sink(self.h, None))
            self._sink_keep = None
            return
        fmt = _pcm_format(dtype)
        npdt = _PCM_NP[fmt]
        self._sink_raised = []

        def tramp(_user, utt, fb, fe, p, ns, fin):
            try:
                a = np.frombuffer((C.c_char * (int(ns) * npdt().itemsize)).from_address(p), npdt).copy() if ns > 0 else np.zeros(0, npdt)
                return 1 if on_audio(utt, fb, fe, a, bool(fin)) else 0
            except BaseException as ex:   # an exception must not cross the C frames
                self._sink_raised.append(ex)
                return 1
        sk = Sink(int(sample_rate), fmt, AUDIO_ANY_CB(tramp), None)
        self._ck(self.L.q3tts_engine_set_sink(self.h, C.cast(C.pointer(sk), C.c_void_p)))
        self._sink_keep = sk   # the callback object must outlive the jobs

    def codec_stream_push(self, sid, codes):
        """the next frames' codes [n][n_groups] -> the samples they own"""
        c = np.ascontiguousarray(codes, dtype=np.int64)
        cap = self.codec_decode_len(c.shape[0]) + 4096
        pcm = np.empty(cap, np.float32)
        n = C.c_int64(0)
        self.L.q3tts_codec_stream_push_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        self._ck(self.L.q3tts_codec_stream_push_host(self.h, sid, _p(c), c.shape[0], _p(pcm), cap, C.byref(n)))
        return pcm[: n.value]

    def codec_stream_push_batch(self, sids, codes_list, finish=None):
        """the next frames of many streams in one batched pass (q3tts_codec_stream_push_batch_host): one [n_s][n_groups] code array per
        stream (n_s may be 0: the stream is left untouched) -> one PCM array each.  A stream begun with a sample_rate / dtype returns
        its own format (q3tts_codec_stream_push_batch_any_host); finish: one flag per stream, a sink's tail is flushed with this push."""
        n = len(sids)
        if n == 0:
            return []
        if len(codes_list) != n or (finish is not None and len(finish) != n):
            raise ValueError("codec_stream_push_batch: one code array (and one finish flag) per stream")
        cs = [np.ascontiguousarray(c_, np.int64).reshape(-1, self.cfg.n_groups) for c_ in codes_list]
        ids = np.ascontiguousarray(sids, np.int32)
        offs = np.cumsum([0] + [c_.shape[0] for c_ in cs]).astype(np.int32)
        fmts = self.__dict__.setdefault("_codec_stream_fmt", {})
        spds = self.__dict__.setdefault("_codec_stream_speed", {})
        lvls = self.__dict__.setdefault("_codec_stream_level", {})
        pits = self.__dict__.setdefault("_codec_stream_pitch", {})
        louds = self.__dict__.setdefault("_codec_stream_loud", {})
        tones = self.__dict__.setdefault("_codec_stream_tone", {})   # a tone stage adds nothing to a push's length
        if finish is None and not any(int(i) in fmts or int(i) in spds or int(i) in lvls or int(i) in pits or int(i) in louds or int(i) in tones for i in ids):
            return self._push_batch(ids, cs, offs)
        flat = np.ascontiguousarray(np.concatenate(cs)) if sum(c_.shape[0] for c_ in cs) else np.zeros((1, self.cfg.n_groups), np.int64)
        n24 = self.codec_decode_len(max(max(c_.shape[0] for c_ in cs), 1)) + 4096
        if any(int(i) in pits for i in ids):
            n24 += 1248                    # behind a pitch stage: plus what it held back
        if any(int(i) in spds for i in ids):
            n24 = (n24 + 1320) * 2 + 720   # behind a stretcher: the slowest speed doubles the push plus what it held back
        if any(int(i) in louds for i in ids):
            n24 += 2400                    # behind a loudness stage: plus what it held back
        if any(int(i) in lvls for i in ids):
            n24 += 128                     # behind a limiter: plus what it held back
        cap = max((n24 + 200) * max(fmts.get(int(i), (24000, PCM_F32))[0], 24000) // 24000 + 8 for i in ids)
        pcm = [np.empty(cap, _PCM_NP[fmts.get(int(i), (24000, PCM_F32))[1]]) for i in ids]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        fin = np.zeros(n, np.uint8) if finish is None else np.ascontiguousarray([1 if f else 0 for f in finish], np.uint8)
        self.L.q3tts_codec_stream_push_batch_any_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_codec_stream_push_batch_any_host(self.h, n, _p(ids), _p(flat), _p(offs), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(fin)))
        return [pcm[i][: pcm_len[i]] for i in range(n)]

    def _push_batch(self, ids, cs, offs):
        n = len(ids)
        flat = np.ascontiguousarray(np.concatenate(cs)) if sum(c_.shape[0] for c_ in cs) else np.zeros((1, self.cfg.n_groups), np.int64)
        cap = self.codec_decode_len(max(max(c_.shape[0] for c_ in cs), 1)) + 4096
        pcm = [np.empty(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        self.L.q3tts_codec_stream_push_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._ck(self.L.q3tts_codec_stream_push_batch_host(self.h, n, _p(ids), _p(flat), _p(offs), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len)))
        return [pcm[i][: pcm_len[i]] for i in range(n)]

    def codec_stream_prime_batch(self, sids, codes_list):
        """open streams that hold no frames yet take the state a push of these frames would leave, without their audio
        (q3tts_codec_stream_prime_batch_host): one [n_s][n_groups] code array per stream (n_s may be 0: the stream is left untouched).
        Only the pre-transformer runs; the streams' buffers keep their size."""
        n = len(sids)
        if len(codes_list) != n:
            raise ValueError("codec_stream_prime_batch: one code array per stream")
        if n == 0:
            return
        cs = [np.ascontiguousarray(c_, np.int64).reshape(-1, self.cfg.n_groups) for c_ in codes_list]
        offs = np.cumsum([0] + [c_.shape[0] for c_ in cs]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(cs)) if offs[-1] else np.zeros((1, self.cfg.n_groups), np.int64)
        self._ck(self.L.q3tts_codec_stream_prime_batch_host(self.h, n, _p(np.ascontiguousarray(sids, np.int32)), _p(flat), _p(offs)))

    def slots_codec_prime(self, slots, n_frames):
        """the listed slots' implicit vocoder streams are restarted and primed with the slots' first n_frames[i] frames
        (q3tts_slots_codec_prime): the next slots_codec_decode_new starts at frame n_frames[i]"""
        n = len(slots)
        if len(n_frames) != n:
            raise ValueError("slots_codec_prime: one frame count per slot")
        if n == 0:
            return
        self._ck(self.L.q3tts_slots_codec_prime(self.h, n, _p(np.ascontiguousarray(slots, np.int32)), _p(np.ascontiguousarray(n_frames, np.int32))))

    def codec_stream_info(self, sid):
        """-> (n_done, kv_capacity_rows, bytes) of a carried-state stream (q3tts_codec_stream_info)"""
        nd, kc, by = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._ck(self.L.q3tts_codec_stream_info(self.h, int(sid), C.byref(nd), C.byref(kc), C.byref(by)))
        return nd.value, kc.value, by.value

    def slots_codec_decode_new(self, slots, max_new_frames=None):
        """samples of the frames each listed slot has generated since its previous streaming call, all slots in batched passes
        (q3tts_slots_codec_decode_new_host) -> [(frame_begin, frame_end, pcm)] per slot.  max_new_frames bounds the new frames of
        a slot (default: the slots' frame counts, asked for first)"""
        n = len(slots)
        if n == 0:
            return []
        ids = np.ascontiguousarray(slots, np.int32)
        if not max_new_frames:
            max_new_frames = max(self.slot_status(int(b))[0] for b in slots)
        cap = self.codec_decode_len(max(int(max_new_frames), 1)) + 4096
        pcm = [np.empty(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len, fb, fe = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.L.q3tts_slots_codec_decode_new_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_slots_codec_decode_new_host(self.h, n, _p(ids), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(fb), _p(fe)))
        return [(int(fb[i]), int(fe[i]), pcm[i][: pcm_len[i]]) for i in range(n)]

    def codec_stream_end(self, sid):
        self.L.q3tts_codec_stream_end.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_codec_stream_end(self.h, sid))
        self.__dict__.setdefault("_codec_stream_fmt", {}).pop(int(sid), None)
        self.__dict__.setdefault("_codec_stream_speed", {}).pop(int(sid), None)
        self.__dict__.setdefault("_codec_stream_level", {}).pop(int(sid), None)
        self.__dict__.setdefault("_codec_stream_pitch", {}).pop(int(sid), None)
        self.__dict__.setdefault("_codec_stream_loud", {}).pop(int(sid), None)
        self.__dict__.setdefault("_codec_stream_tone", {}).pop(int(sid), None)

    def slot_codec_decode_range(self, slot, frame_begin, frame_end, left_context):
        """samples owned by frames [frame_begin, frame_end) of a slot (streaming while it generates)"""
        n = self.codec_decode_len(frame_end) - (self.codec_decode_len(frame_begin) if frame_begin > 0 else 0)
        pcm = np.empty(max(n, 1), np.float32)
        out_len = C.c_int64(0)
        self._ck(self.L.q3tts_slot_codec_decode_range_host(self.h, slot, frame_begin, frame_end, left_context, _p(pcm), n, C.byref(out_len)))
        return pcm[: out_len.value]

    def sample(self, logits, sp, u, suppress=False):
        a = np.ascontiguousarray(logits, dtype=np.float32)
        tok = C.c_int64(0)
        self._ck(self.L.q3tts_sample_host(self.h, _p(a), a.size, C.byref(sp), C.c_float(u), int(suppress), C.byref(tok)))
        return int(tok.value)

    def sample_hist(self, logits, sp, u, history, suppress=False):
        """sample() with sp.repetition_penalty applied to the ids in `history` first (q3tts_sample_hist_host)"""
        a = np.ascontiguousarray(logits, dtype=np.float32)
        hist = np.ascontiguousarray(history, dtype=np.int64).reshape(-1)
        tok = C.c_int64(0)
        self.L.q3tts_sample_hist_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        self._ck(self.L.q3tts_sample_hist_host(self.h, _p(a), a.size, C.byref(sp), C.c_float(u), int(suppress), _p(hist) if hist.size else None,
                                               hist.size, C.byref(tok)))
        return int(tok.value)

    def build_prompt(self, ids, lang=0, speaker=None, cap_rows=1024, instruct_ids=None):
        """build_prompt_embeddings; instruct_ids (already framed: frame_instruct_ids) puts the instruction's projected rows in front"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        ins = None if instruct_ids is None else np.ascontiguousarray(instruct_ids, dtype=np.int64).reshape(-1)
        prompt = np.zeros((16 + (0 if ins is None else ins.size), self.cfg.hidden), np.float32)
        trailing = np.zeros((cap_rows, self.cfg.hidden), np.float32)
        S, nt = C.c_int(0), C.c_int(0)
        sp = np.ascontiguousarray(speaker, dtype=np.float32) if speaker is not None else None
        if sp is not None and sp.size != self.cfg.hidden:
            raise ValueError("speaker embedding has %d values, the model needs %d" % (sp.size, self.cfg.hidden))
        if ins is not None:
            self._ck(self.L.q3tts_build_prompt_instruct_host(self.h, _p(ids), ids.size, lang, _p(sp) if sp is not None else None,
                                                             _p(ins) if ins.size else None, ins.size, _p(prompt), prompt.shape[0], C.byref(S),
                                                             _p(trailing), cap_rows, C.byref(nt)))
            return prompt[: S.value].copy(), trailing[: nt.value].copy()
        self._ck(self.L.q3tts_build_prompt_host(self.h, _p(ids), ids.size, lang, _p(sp) if sp is not None else None,
                                                _p(prompt), C.byref(S), _p(trailing), cap_rows, C.byref(nt)))
        return prompt[: S.value].copy(), trailing[: nt.value].copy()

    def build_prompt_open(self, ids, lang=0, speaker=None, cap_rows=1024):
        """build_prompt for a text whose end is not known (q3tts_build_prompt_open_host): every id behind the first text id becomes a
        trailing row, no tts_eos row; begin a slot with the result, then slot_text_open"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        prompt = np.zeros((16, self.cfg.hidden), np.float32)
        trailing = np.zeros((max(cap_rows, 1), self.cfg.hidden), np.float32)
        S, nt = C.c_int(0), C.c_int(0)
        sp = np.ascontiguousarray(speaker, dtype=np.float32) if speaker is not None else None
        if sp is not None and sp.size != self.cfg.hidden:
            raise ValueError("speaker embedding has %d values, the model needs %d" % (sp.size, self.cfg.hidden))
        self._ck(self.L.q3tts_build_prompt_open_host(self.h, _p(ids), ids.size, lang, _p(sp) if sp is not None else None,
                                                     _p(prompt), C.byref(S), _p(trailing), cap_rows, C.byref(nt)))
        return prompt[: S.value].copy(), trailing[: nt.value].copy()

    # ---- live text: append text to generating slots (include/q3tts.h "live text") ----
    def slot_text_open(self, slot):
        """the slot's text may grow (after slot_begin*, before its first step): it stalls instead of reading the pad row"""
        self._ck(self.L.q3tts_slot_text_open(self.h, int(slot)))

    def slot_text_append(self, slot, rows=None, ids=None, close=False):
        """projected rows [n][hidden] (rows=) or token ids (ids=) go behind the slot's text; close=True ends the text (tts_eos row)"""
        if rows is not None and ids is not None:
            raise ValueError("slot_text_append: rows or ids, not both")
        if ids is not None:
            return self.slots_text_append_ids([slot], [ids], [close])
        r = np.zeros((0, self.cfg.hidden), np.float32) if rows is None else np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.cfg.hidden)
        self._ck(self.L.q3tts_slot_text_append_host(self.h, int(slot), _p(r) if r.size else None, r.shape[0], int(bool(close))))

    def slots_text_append_ids(self, slots, id_lists, close=None):
        """q3tts_slots_text_append_ids: slot slots[i] takes id_lists[i]; one projection pass and one scatter launch for all of them"""
        n = len(slots)
        if len(id_lists) != n or (close is not None and len(close) != n):
            raise ValueError("slots_text_append_ids: one entry per slot")
        sl = np.ascontiguousarray(slots, np.int32)
        parts = [np.asarray(t, np.int64).reshape(-1) for t in id_lists]
        flat = np.ascontiguousarray(np.concatenate(parts)) if n else np.zeros(0, np.int64)
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([t.size for t in parts])
        cl = np.zeros(n, np.uint8) if close is None else np.array([1 if c else 0 for c in close], np.uint8)
        self._ck(self.L.q3tts_slots_text_append_ids(self.h, n, _p(sl), _p(flat) if flat.size else None, _p(offs), _p(cl)))

    def slot_text_status(self, slot):
        """(text rows held, open, starved): starved = open and the next frame's text row has not arrived"""
        n, o, st = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.q3tts_slot_text_status(self.h, int(slot), C.byref(n), C.byref(o), C.byref(st)))
        return n.value, bool(o.value), bool(st.value)

    # ---- fused generation ----
    # ---- shared prompt prefix ----
    def prefix_create(self, rows):
        """rows [P][hidden] prefilled once and kept as compact KV rows on the engine (q3tts_prefix_create); returns the prefix id"""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != self.cfg.hidden:
            raise ValueError("prefix rows must be [P][hidden]")
        pid = C.c_int(-1)
        self._ck(self.L.q3tts_prefix_create(self.h, _p(r) if r.size else None, r.shape[0], C.byref(pid)))
        return pid.value

    def prefix_create_instruct(self, framed_ids):
        """text_project of framed instruction ids (frame_instruct_ids) + prefix_create"""
        ids = np.ascontiguousarray(framed_ids, dtype=np.int64).reshape(-1)
        pid = C.c_int(-1)
        self._ck(self.L.q3tts_prefix_create_instruct(self.h, _p(ids) if ids.size else None, ids.size, C.byref(pid)))
        return pid.value

    def prefix_info(self, prefix_id):
        """(rows, bytes of the store)"""
        n, b = C.c_int(0), C.c_int64(0)
        self._ck(self.L.q3tts_prefix_info(self.h, int(prefix_id), C.byref(n), C.byref(b)))
        return n.value, b.value

    def prefix_release(self, prefix_id):
        self._ck(self.L.q3tts_prefix_release(self.h, int(prefix_id)))

    def slots_begin_prefixed(self, slots, prefix_ids, prompts, trailings, sp, seed=0, stream_ids=None, ignore_eos=False):
        """q3tts_slots_begin_prefixed: slot slots[i] begun behind prefix prefix_ids[i] (None / -1: none) with prompts[i] / trailings[i];
        members with equal prompt lengths <= 16 share one pass through the talker"""
        n = len(slots)
        if not (len(prompts) == n and len(trailings) == n and (prefix_ids is None or len(prefix_ids) == n) and (stream_ids is None or len(stream_ids) == n)):
            raise ValueError("slots_begin_prefixed: one entry per slot")
        ps = [np.ascontiguousarray(a, dtype=np.float32) for a in prompts]
        ts = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, self.cfg.hidden) for a in trailings]
        pp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in ps])
        tp = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in ts])
        sl = np.ascontiguousarray(slots, np.int32)
        ids = np.array([-1 if (prefix_ids is None or v is None) else int(v) for v in (prefix_ids if prefix_ids is not None else [None] * n)], np.int32)
        S = np.array([a.shape[0] for a in ps], np.int32)
        nt = np.array([a.shape[0] for a in ts], np.int32)
        st = np.arange(n, dtype=np.uint32) if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32)
        self._ck(self.L.q3tts_slots_begin_prefixed(self.h, n, _p(sl), _p(ids), C.cast(pp, C.c_void_p), _p(S), C.cast(tp, C.c_void_p), _p(nt),
                                                   C.byref(sp), seed, _p(st), int(ignore_eos)))

    def slots_begin_ragged(self, slots, prompts, trailings, sp, prefix_ids=None, prefix_codes=None, seed=0, stream_ids=None, ignore_eos=False):
        """q3tts_slots_begin_ragged: slot slots[i] begun behind prefix prefix_ids[i] (None / -1: none) with prompts[i] of any length,
        trailings[i] and the teacher-forced frames prefix_codes[i] ([F0][n_groups]; None: none).  The members' rows share 128-row
        chunks: one pass through the talker per chunk, whatever the lengths"""
        n = len(slots)
        if not (len(prompts) == n and len(trailings) == n and (prefix_ids is None or len(prefix_ids) == n)
                and (prefix_codes is None or len(prefix_codes) == n) and (stream_ids is None or len(stream_ids) == n)):
            raise ValueError("slots_begin_ragged: one entry per slot")
        ps = [np.ascontiguousarray(a, dtype=np.float32) for a in prompts]
        ts = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, self.cfg.hidden) for a in trailings]
        cs = [None if (prefix_codes is None or a is None) else self._frames(a, "slots_begin_ragged(prefix_codes)") for a in (prefix_codes if prefix_codes is not None else [None] * n)]
        pp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in ps])
        tp = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in ts])
        cp = (C.c_void_p * max(n, 1))(*[a.ctypes.data if (a is not None and a.shape[0]) else None for a in cs])
        sl = np.ascontiguousarray(slots, np.int32)
        ids = np.array([-1 if (prefix_ids is None or v is None) else int(v) for v in (prefix_ids if prefix_ids is not None else [None] * n)], np.int32)
        S = np.array([a.shape[0] for a in ps], np.int32)
        nt = np.array([a.shape[0] for a in ts], np.int32)
        nc = np.array([0 if a is None else a.shape[0] for a in cs], np.int32)
        st = np.arange(n, dtype=np.uint32) if stream_ids is None else np.ascontiguousarray(stream_ids, np.uint32)
        self._ck(self.L.q3tts_slots_begin_ragged(self.h, n, _p(sl), _p(ids), C.cast(pp, C.c_void_p), _p(S), C.cast(tp, C.c_void_p), _p(nt),
                                                 C.cast(cp, C.c_void_p), _p(nc), C.byref(sp), seed, _p(st), int(ignore_eos)))

    def slot_begin(self, slot, prompt, trailing, sp, seed=0, stream_id=0, ignore_eos=False, prefix_codes=None, prefix_id=None):
        """prefix_codes [F0][n_groups]: continue from codes (q3tts_slot_begin_codes) — the slot is armed as if it had generated exactly
        these as its first F0 frames; sp.max_new_tokens counts the frames behind them.  prefix_id: begun behind that shared prompt
        prefix (q3tts_slot_begin_prefixed)"""
        p = np.ascontiguousarray(prompt, dtype=np.float32)
        t = np.ascontiguousarray(trailing, dtype=np.float32)
        if prefix_id is not None:
            c = None if prefix_codes is None else self._frames(prefix_codes, "slot_begin(prefix_codes)")
            nc = 0 if c is None else c.shape[0]
            self._ck(self.L.q3tts_slot_begin_prefixed(self.h, slot, int(prefix_id), _p(p), p.shape[0], _p(t), t.shape[0], _p(c) if nc else None, nc,
                                                      C.byref(sp), seed, stream_id, int(ignore_eos)))
            return
        if prefix_codes is None:
            self._ck(self.L.q3tts_slot_begin(self.h, slot, _p(p), p.shape[0], _p(t), t.shape[0], C.byref(sp), seed,
                                             stream_id, int(ignore_eos)))
            return
        c = self._frames(prefix_codes, "slot_begin(prefix_codes)")
        self._ck(self.L.q3tts_slot_begin_codes(self.h, slot, _p(p), p.shape[0], _p(t), t.shape[0], _p(c) if c.shape[0] else None, c.shape[0],
                                               C.byref(sp), seed, stream_id, int(ignore_eos)))

    def decode_steps(self, n):
        return self._ck(self.L.q3tts_decode_steps(self.h, n))

    def slot_status(self, slot):
        nf, fin = C.c_int(0), C.c_int(0)
        self._ck(self.L.q3tts_slot_status(self.h, slot, C.byref(nf), C.byref(fin)))
        return nf.value, bool(fin.value)

    def slot_codes(self, slot):
        nf, _ = self.slot_status(slot)
        codes = np.zeros((max(nf, 1), self.cfg.n_groups), np.int64)
        self._ck(self.L.q3tts_slot_codes_host(self.h, slot, _p(codes), nf))
        return codes[:nf]

    def slot_logits(self, slot):
        """(logits[vocab], last_hidden[hidden]) the fused path holds for the slot's next frame (run_decode's outputs)"""
        lg = np.empty(self.cfg.vocab, np.float32)
        lh = np.empty(self.cfg.hidden, np.float32)
        self._ck(self.L.q3tts_slot_logits_host(self.h, slot, _p(lg), _p(lh)))
        return lg, lh

    def step_logits(self, slot):
        """one eager decode step; returns [n_groups][max(vocab, sub_vocab)]: the logits row behind each of the frame's decisions of `slot`"""
        cols = max(self.cfg.vocab, self.cfg.sub_vocab)
        out = np.zeros((self.cfg.n_groups, cols), np.float32)
        self._ck(self.L.q3tts_step_logits_host(self.h, slot, _p(out), cols))
        return out

    def slot_codec_decode(self, slot):
        nf, _ = self.slot_status(slot)
        n = self.codec_decode_len(nf) if nf > 0 else 0
        pcm = np.empty(max(n, 1), np.float32)
        out_len = C.c_int64(0)
        self._ck(self.L.q3tts_slot_codec_decode_host(self.h, slot, _p(pcm), n, C.byref(out_len)))
        return pcm[: out_len.value]

    def slot_release(self, slot):
        self._ck(self.L.q3tts_slot_release(self.h, slot))

    def generate(self, prompt, trailing, sp, seed=0, stream_id=0, ignore_eos=False, slot=0, chunk=32, prefix_id=None):
        """generate_codes (reference src/tts_onnx.cpp:782-849) for one utterance on the fused path."""
        self.slot_begin(slot, prompt, trailing, sp, seed, stream_id, ignore_eos, prefix_id=prefix_id)
        left = sp.max_new_tokens
        while left > 0:
            n = min(chunk, left)
            active = self.decode_steps(n)
            left -= n
            if active == 0:
                break
        codes = self.slot_codes(slot)
        return codes

    # ---- voice-clone front end ----
    @property
    def has_speaker_encoder(self):
        return bool(self.L.q3tts_has_speaker_encoder(self.h))

    def speaker_encoder(self, mel):
        """run_speaker_encoder (tts_onnx.cpp:367-403): mel [128][frames] -> [spk_enc_dim]"""
        mel = np.ascontiguousarray(mel, np.float32)
        out = np.zeros(self.cfg.spk_enc_dim, np.float32)
        self._ck(self.L.q3tts_speaker_encoder_host(self.h, _p(mel), mel.shape[1], _p(out)))
        return out

    def extract_speaker_embedding(self, wav_path):
        out = np.zeros(self.cfg.spk_enc_dim, np.float32)
        self._ck(self.L.q3tts_extract_speaker_embedding_host(self.h, os.fsencode(wav_path), _p(out)))
        return out

    def resample_gpu(self, audio, src_rate, dst_rate):
        """io::resample on the GPU (q3tts_resample_gpu_host): the samples of q3tts.resample, bit for bit"""
        a = np.ascontiguousarray(audio, np.float32)
        n = self._ck(self.L.q3tts_resample_gpu_host(self.h, _p(a), a.size, src_rate, dst_rate, None, 0))
        out = np.zeros(max(n, 1), np.float32)
        self._ck(self.L.q3tts_resample_gpu_host(self.h, _p(a), a.size, src_rate, dst_rate, _p(out), n))
        return out[:n]

    def log_mel_gpu(self, audio, sample_rate=24000):
        """resample to 24 kHz + MelExtractor::extract on the GPU (q3tts_mel_gpu_host): [128][frames]; (128, 0) for an empty clip"""
        a = np.ascontiguousarray(audio, np.float32)
        fr = C.c_int32(0)
        if self.L.q3tts_mel_gpu_host(self.h, _p(a), a.size, sample_rate, None, 0, C.byref(fr)) != 0:
            if fr.value == 0 and b"Failed to extract mel" in self.L.q3tts_last_error(self.h):
                return np.zeros((128, 0), np.float32)
            raise RuntimeError(self.L.q3tts_last_error(self.h).decode())
        out = np.zeros((128, fr.value), np.float32)
        self._ck(self.L.q3tts_mel_gpu_host(self.h, _p(a), a.size, sample_rate, _p(out), out.size, C.byref(fr)))
        return out

    def speaker_embeddings(self, clips, sample_rates):
        """extract_speaker_embedding for clips already in memory (mono float arrays, any rate; a scalar rate applies to all):
        [len(clips)][spk_enc_dim] from one batched call (q3tts_speaker_embed_pcm_batch_host)"""
        n = len(clips)
        keep = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1) for a in clips]
        rates = [int(sample_rates)] * n if np.isscalar(sample_rates) else [int(r) for r in sample_rates]
        if len(rates) != n:
            raise ValueError("sample_rates: one rate per clip, or one for all")
        ptrs = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in keep])
        ns = np.array([0 if a is None else a.size for a in keep], np.int64)
        rt = np.array(rates, np.int32)
        out = np.zeros((n, self.cfg.spk_enc_dim), np.float32)
        self._ck(self.L.q3tts_speaker_embed_pcm_batch_host(self.h, n, ptrs, _p(ns) if n else None, _p(rt) if n else None, _p(out) if out.size else None))
        return out

    # ---- audio -> codes: the 12 Hz tokenizer's encoder ----
    @property
    def has_audio_encoder(self):
        return bool(self.L.q3tts_has_audio_encoder(self.h))

    def audio_encode_len(self, n_samples):
        """frames of a clip of n_samples samples at 24 kHz (host-only)"""
        return int(self._ck(self.L.q3tts_audio_encode_len(self.h, int(n_samples))))

    def audio_encode(self, pcm24k, want_latents=False):
        """pcm24k (mono float, 24 kHz) -> codes [F][n_groups] int64, the layout slot_codes returns and slot_begin(prefix_codes=) takes;
        want_latents: (codes, latents [F][enc_hidden]), the rows the quantiser sees (parity aid)"""
        a = np.ascontiguousarray(pcm24k, np.float32).reshape(-1)
        F = max(int(self.L.q3tts_audio_encode_len(self.h, a.size)), 1)
        codes = np.zeros((F, self.cfg.n_groups), np.int64)
        nf = C.c_int32(0)
        if not want_latents:
            self._ck(self.L.q3tts_audio_encode_host(self.h, _p(a), a.size, _p(codes), F, C.byref(nf)))
            return codes[: nf.value]
        lat = np.zeros((F, max(self.cfg.enc_hidden, 1)), np.float32)
        self._ck(self.L.q3tts_audio_encode_latents_host(self.h, _p(a), a.size, _p(lat), _p(codes), F, C.byref(nf)))
        return codes[: nf.value], lat[: nf.value]

    def audio_encode_batch(self, clips, sample_rates=24000, want_latents=False):
        """audio_encode for many clips at once (mono float arrays, any rate; a scalar rate applies to all): one set of launches,
        each clip's codes identical to encoding it alone (q3tts_audio_encode_batch_host).  Returns a list of [F_i][n_groups] arrays;
        want_latents: (that list, the list of latents [F_i][enc_hidden]) — the parity aid."""
        n = len(clips)
        keep = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in clips]
        rates = [int(sample_rates)] * n if np.isscalar(sample_rates) else [int(r) for r in sample_rates]
        if len(rates) != n:
            raise ValueError("sample_rates: one rate per clip, or one for all")
        caps = [max(int(self.L.q3tts_audio_encode_len(self.h, int(a.size * 24000.0 / max(r, 1)) + 1)), 1) for a, r in zip(keep, rates)]
        outs = [np.zeros((cp, self.cfg.n_groups), np.int64) for cp in caps]
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
        optrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        ns = np.array([a.size for a in keep], np.int64)
        rt = np.array(rates, np.int32)
        cp = np.array(caps, np.int32)
        nf = np.zeros(max(n, 1), np.int32)
        args = (self.h, n, ptrs, _p(ns) if n else None, _p(rt) if n else None, optrs)
        if not want_latents:
            self._ck(self.L.q3tts_audio_encode_batch_host(*args, _p(cp) if n else None, _p(nf)))
            return [o[: nf[i]] for i, o in enumerate(outs)]
        lats = [np.zeros((c_, max(self.cfg.enc_hidden, 1)), np.float32) for c_ in caps]
        lptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in lats])
        self._ck(self.L.q3tts_audio_encode_batch_latents_host(*args, lptrs, _p(cp) if n else None, _p(nf)))
        return [o[: nf[i]] for i, o in enumerate(outs)], [a[: nf[i]] for i, a in enumerate(lats)]

    # ---- audio -> codes while the audio arrives (q3tts_audio_stream_*) ----
    def audio_stream_begin(self, max_samples=0):
        """a new encoder stream for at most max_samples samples at 24 kHz (0: 60 s; at most one hour) -> stream id;
        audio_stream_begin_rate at 24 000 Hz / float32"""
        if int(max_samples) < 0:
            raise ValueError("max_samples must be 0 (60 s) or positive")
        return Engine.audio_stream_begin_rate(self, 24000, "float32", max_samples)

    def audio_stream_begin_rate(self, sample_rate, dtype="float32", max_samples=0):
        """a new encoder stream at sample_rate (1 .. 384000) whose samples are pushed as dtype "float32", "int16", or G.711 bytes ("mulaw" / "alaw", np.uint8), for at most
        max_samples of its OWN samples (0: 60 s; at most one hour) -> stream id (q3tts_audio_stream_begin_rate).  Other than 24 kHz
        float32 the stream resamples on the GPU on the way in, bit-identical to audio_encode_batch of the whole audio at that rate
        (int16 v is the float v / 32768; a G.711 byte is decoded to that int16 on the GPU)."""
        if int(max_samples) < 0:
            raise ValueError("max_samples must be 0 (60 s) or positive")
        fmt = _pcm_format(dtype)
        sid = C.c_int(-1)
        self._ck(self.L.q3tts_audio_stream_begin_rate(self.h, int(sample_rate), fmt, int(max_samples), C.byref(sid)))
        self.__dict__.setdefault("_audio_stream_fmt", {})[int(sid.value)] = (int(sample_rate), fmt)
        return int(sid.value)

    def audio_stream_format(self, sid):
        """(sample_rate, dtype name) the stream was begun with"""
        sr, fmt = C.c_int32(0), C.c_int(0)
        self._ck(self.L.q3tts_audio_stream_format(self.h, int(sid), C.byref(sr), C.byref(fmt)))
        return int(sr.value), _PCM_NAMES[fmt.value]

    def audio_stream_push_len(self, sid, n_samples, finish=False):
        """frames the next push of n_samples to this stream would return (host-only)"""
        if int(n_samples) < 0:
            raise ValueError("n_samples must not be negative")
        return int(self._ck(self.L.q3tts_audio_stream_push_len(self.h, int(sid), int(n_samples), 1 if finish else 0)))

    @staticmethod
    def _stream_pcm(pcm, what="pcm", fmt=0):
        a = np.asarray(pcm)
        if fmt != PCM_F32:
            want = np.int16 if fmt == PCM_S16 else np.uint8
            if a.size and a.dtype != want:
                raise ValueError("%s: expected %s samples (the stream was begun with dtype %s), got dtype %s" % (what, np.dtype(want).name, _PCM_NAMES[fmt], a.dtype))
            if a.ndim > 1 and a.size != max(a.shape):
                raise ValueError("%s: expected mono samples [n], got shape %s" % (what, (a.shape,)))
            return np.ascontiguousarray(a, want).reshape(-1)
        if a.size and a.dtype.kind != "f":
            raise ValueError("%s: expected float samples (mono, 24 kHz), got dtype %s" % (what, a.dtype))
        if a.ndim > 1 and a.size != max(a.shape):
            raise ValueError("%s: expected mono samples [n], got shape %s" % (what, (a.shape,)))
        return np.ascontiguousarray(a, np.float32).reshape(-1)

    def audio_stream_push_batch(self, sids, pcms, finish=None, want_latents=False):
        """one push to each of many streams in ONE call (q3tts_audio_stream_push_batch_host): pcms[i] are stream sids[i]'s next samples
        (mono, at the stream's own rate, float or, for a stream begun with dtype int16 / mulaw / alaw, and only for it, int16 / uint8; may be empty), finish[i] ends stream i's audio (None: none; a bool applies to all).  Returns the list of
        the NEW codes [F_i][n_groups] per stream, bit-identical to audio_encode of each stream's concatenated audio; want_latents:
        (that list, the list of latents [F_i][enc_hidden])."""
        n = len(sids)
        if len(pcms) != n:
            raise ValueError("one sample array per stream")
        fin = [False] * n if finish is None else ([bool(finish)] * n if np.isscalar(finish) else [bool(f) for f in finish])
        if len(fin) != n:
            raise ValueError("finish: one flag per stream, one for all, or None")
        if len(set(int(s) for s in sids)) != n:
            raise ValueError("a stream may appear once per push")
        if n == 0:
            return ([], []) if want_latents else []
        # int16 / uint8 arrays for the streams begun with dtype int16 / mulaw / alaw, and only for them (begin recorded it; an id it never
        # saw counts as float32 and is the engine's to refuse)
        begun = vars(self).get("_audio_stream_fmt", {})
        keep = [Engine._stream_pcm(a, "pcms[%d]" % i, fmt=begun.get(int(sids[i]), (24000, PCM_F32))[1]) for i, a in enumerate(pcms)]
        per = 1
        for r in list(self.cfg.enc_ratios)[: self.cfg.enc_n_ratios]:
            per *= int(r)
        # frames of room per stream, from the host rule: the 24 kHz samples this push adds, E(after) - E(before)
        caps = []
        for i, a in enumerate(keep):
            stt = self._stream_state(sids[i])
            if stt is None:                                                # not an open stream: the call below says so
                caps.append(2)
                continue
            rate, _, got, fed = stt
            new24 = resample_stream_emitted(rate, 24000, got + a.size, fin[i]) - fed
            caps.append(max(new24, 0) // (2 * per) + 2)
        outs = [np.zeros((cp, self.cfg.n_groups), np.int64) for cp in caps]
        lats = [np.zeros((cp, max(self.cfg.enc_hidden, 1)), np.float32) for cp in caps] if want_latents else None
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in keep])
        optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        lptrs = (C.c_void_p * n)(*[a.ctypes.data for a in lats]) if want_latents else None
        ids = np.array([int(s) for s in sids], np.int32)
        ns = np.array([a.size for a in keep], np.int64)
        fl = np.array(fin, np.int32)
        cp = np.array(caps, np.int32)
        nf = np.zeros(n, np.int32)
        push = self.L.q3tts_audio_stream_push_batch_any_host if any(a.dtype != np.float32 for a in keep) else self.L.q3tts_audio_stream_push_batch_host
        self._ck(push(self.h, n, _p(ids), ptrs, _p(ns), _p(fl), optrs, lptrs, _p(cp), _p(nf)))
        codes = [o[: nf[i]] for i, o in enumerate(outs)]
        return (codes, [a[: nf[i]] for i, a in enumerate(lats)]) if want_latents else codes

    def _stream_state(self, sid):
        """(rate, format, samples received, 24 kHz samples fed to the encoder) of an open stream, None for an id the engine refuses"""
        sr, fmt, ns = C.c_int32(0), C.c_int(0), C.c_int64(0)
        if self.L.q3tts_audio_stream_format(self.h, int(sid), C.byref(sr), C.byref(fmt)) != 0:
            return None
        if self.L.q3tts_audio_stream_info(self.h, int(sid), C.byref(ns), None, None, None) != 0:
            return None
        return int(sr.value), int(fmt.value), int(ns.value), resample_stream_emitted(int(sr.value), 24000, int(ns.value), False)

    def audio_stream_push(self, sid, pcm, finish=False, want_latents=False):
        """pcm (mono, the stream's own rate and sample format, any length up to 60 s) appended to stream sid -> the NEW frames' codes [F][n_groups];
        finish: the stream's audio ends here.  want_latents: (codes, latents [F][enc_hidden])"""
        r = self.audio_stream_push_batch([sid], [pcm], [finish], want_latents)
        return (r[0][0], r[1][0]) if want_latents else r[0]

    def audio_stream_info(self, sid):
        """(samples received, frames returned, finished, bytes of device state)"""
        ns, nf, fin, by = C.c_int64(0), C.c_int32(0), C.c_int(0), C.c_int64(0)
        self._ck(self.L.q3tts_audio_stream_info(self.h, int(sid), C.byref(ns), C.byref(nf), C.byref(fin), C.byref(by)))
        return int(ns.value), int(nf.value), bool(fin.value), int(by.value)

    def audio_stream_end(self, sid):
        self._ck(self.L.q3tts_audio_stream_end(self.h, int(sid)))
        vars(self).get("_audio_stream_fmt", {}).pop(int(sid), None)

    def audio_encode_long(self, pcm24k, chunk_samples=96000):
        """audio_encode for any length up to one hour: the clip pushed chunk_samples at a time through one stream -> codes
        [F][n_groups], bit-identical to what audio_encode gives where it accepts the clip"""
        a = Engine._stream_pcm(pcm24k, "pcm24k")
        return Engine._encode_long(self, a, chunk_samples, 24000, "pcm24k")

    def audio_encode_long_rate(self, pcm, sample_rate, chunk_samples=None):
        """audio_encode_long for a clip at sample_rate (mono float32, or int16), pushed chunk_samples of its own samples at a time
        (None: 4 s) through one stream begun at that rate -> codes [F][n_groups], bit-identical to what audio_encode_batch gives at
        that rate where it accepts the clip.  Nothing is resampled on the host."""
        a = Engine._stream_pcm(pcm, "pcm", fmt=PCM_S16 if np.asarray(pcm).dtype == np.int16 else PCM_F32)
        return Engine._encode_long(self, a, 4 * int(sample_rate) if chunk_samples is None else chunk_samples, sample_rate, "pcm")

    def _encode_long(self, a, chunk_samples, sample_rate, what):
        if int(chunk_samples) < 1:
            raise ValueError("chunk_samples must be at least 1")
        if a.size < 1:
            raise ValueError("%s: no samples" % what)
        with AudioEncodeStream(self, a.size, sample_rate=sample_rate, dtype="int16" if a.dtype == np.int16 else "float32") as st:
            for i in range(0, a.size, int(chunk_samples)):
                st.push(a[i : i + int(chunk_samples)])
            st.finish()
            return st.codes

    def last_audio_encode_ms(self):
        ms = C.c_float(0)
        self._ck(self.L.q3tts_last_audio_encode_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def audio_encoder_transformer(self, rows):
        """parity aid (FLAG_TEST_HOOKS engines): the encoder's transformer alone on rows [n][enc_hidden]"""
        r = np.ascontiguousarray(rows, np.float32)
        out = np.zeros_like(r)
        self._ck(self.L.q3tts_test_audio_encoder_transformer_host(self.h, _p(r), r.shape[0], _p(out)))
        return out

    def synthesize_icl(self, ref_pcm, ref_ids, ids, sp, lang=0, seed=0, stream_id=0, ignore_eos=False, speaker=None, slot=0, ref_rate=24000):
        """In-context voice clone ([HINT]): the reference audio is encoded to codes, the prompt is built from
        the reference text followed by the target text (ids: the framed target utterance as the other entries take it, ref_ids: the
        reference's text ids alone, spliced in front of the target text), the slot is begun behind the reference codes, and the returned
        samples are the target's only.  Returns (pcm, codes, n_ref_frames): codes cover reference + new frames."""
        ref_codes = self.audio_encode_batch([ref_pcm], ref_rate)[0]
        toks = self.frame_icl_ids(ref_ids, ids)
        prompt, trailing = self.build_prompt(toks, lang, speaker)
        self.slot_begin(slot, prompt, trailing, sp, seed, stream_id, ignore_eos, prefix_codes=ref_codes)
        try:
            left = sp.max_new_tokens
            while left > 0:
                n = min(32, left)
                active = self.decode_steps(n)
                left -= n
                if active == 0:
                    break
            codes = self.slot_codes(slot)
            F0 = ref_codes.shape[0]
            pcm = self.slot_codec_decode_range(slot, F0, codes.shape[0], F0) if codes.shape[0] > F0 else np.zeros(0, np.float32)
        finally:
            self.slot_release(slot)
        return pcm, codes, F0

    def synthesize_icl_batch(self, ref_pcms, ref_ids_list, token_lists, sp, lang=0, seed=0, ignore_eos=False, speakers=None, ref_rates=24000,
                             max_new_per_utt=None, chunk_frames=0, on_audio=None):
        """synthesize_icl for many utterances at once ([HINT] framing): ONE audio_encode_batch call turns the
        reference clips into codes, frame_icl_ids frames each utterance's ids, and the continue entry generates behind the reference
        codes — streaming (on_audio, chunk_frames: synthesize_continue's) or not.  Returns, per utterance, the target's PCM, all codes
        (reference + new frames) and n_ref_frames."""
        n = len(token_lists)
        if len(ref_pcms) != n or len(ref_ids_list) != n:
            raise ValueError("synthesize_icl_batch: one reference clip and one reference id list per utterance")
        if on_audio is not None and int(chunk_frames) < 1:
            raise ValueError("synthesize_icl_batch: on_audio needs chunk_frames >= 1")
        if on_audio is None and chunk_frames:
            raise ValueError("synthesize_icl_batch: chunk_frames without on_audio")
        ref_codes = self.audio_encode_batch(ref_pcms, ref_rates)
        toks = [self.frame_icl_ids(r, t) for r, t in zip(ref_ids_list, token_lists)]
        pcm, codes, _ = self.synthesize_continue(toks, ref_codes, sp, lang, seed, ignore_eos, speakers, max_new_per_utt, chunk_frames, on_audio)
        return pcm, codes, [int(c_.shape[0]) for c_ in ref_codes]

    @staticmethod
    def frame_icl_ids(ref_ids, ids):
        """ids = a framed utterance as every other entry takes it (3 role ids, the text, the template's 2-id tail); the reference's
        text ids go between the role ids and the target text: text = reference text + target text"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        return np.concatenate([ids[:3], np.asarray(ref_ids, np.int64).reshape(-1), ids[3:]])

    @staticmethod
    def _instruct_args(instructs, n):
        """flat framed ids + offsets [n + 1] of a job's per-utterance instructions (None / empty: none for that utterance)"""
        if instructs is None:
            return None, None
        if len(instructs) != n:
            raise ValueError("instructs: one entry (framed ids or None) per utterance")
        rows = [np.zeros(0, np.int64) if t is None else np.asarray(t, np.int64).reshape(-1) for t in instructs]
        flat = np.ascontiguousarray(np.concatenate(rows + [np.zeros(1, np.int64)]))   # never empty: a valid pointer
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([r.size for r in rows])
        return flat, offs

    def synthesize_prefixed(self, token_lists, prefix_ids, sp, lang=0, seed=0, ignore_eos=False, want_codes=True, speakers=None, max_new_per_utt=None,
                            chunk_frames=0, on_audio=None):
        """synthesize_batch with utterance u begun behind shared prompt prefix prefix_ids[u] (None / -1: none): q3tts_synthesize_prefixed_host.
        on_audio: synthesize_stream's delivery, every chunk_frames steps."""
        n = len(token_lists)
        if prefix_ids is None or len(prefix_ids) != n:
            raise ValueError("prefix_ids: one entry (id or None) per utterance")
        ids = np.array([-1 if v is None else int(v) for v in prefix_ids], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in token_lists]))
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(t) for t in token_lists])
        cap = self.codec_decode_len(sp.max_new_tokens)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        nfr = np.zeros(n, np.int32)
        codes = np.zeros((n, sp.max_new_tokens, self.cfg.n_groups), np.int64) if want_codes else None
        spk_keep, spk_ptrs = [], None
        if speakers is not None:
            if len(speakers) != n:
                raise ValueError("speakers: one entry (embedding or None) per utterance")
            spk_keep = [None if s_ is None else np.ascontiguousarray(s_, np.float32) for s_ in speakers]
            for a in spk_keep:
                if a is not None and a.size != self.cfg.hidden:
                    raise ValueError("speaker embedding has %d values, the model needs %d" % (a.size, self.cfg.hidden))
            spk_ptrs = C.cast((C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in spk_keep]), C.c_void_p)
        caps = None if max_new_per_utt is None else np.ascontiguousarray(max_new_per_utt, np.int32)
        if caps is not None and caps.shape != (n,):
            raise ValueError("max_new_per_utt: one entry per utterance")
        raised = []

        def tramp(_user, utt, fb, fe, p, ns, fin):
            try:
                a = np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns > 0 else np.zeros(0, np.float32)
                return 1 if on_audio(utt, fb, fe, a, bool(fin)) else 0
            except BaseException as ex:   # an exception must not cross the C frames: cancel the job, re-raise behind it
                raised.append(ex)
                return 1
        cb = AUDIO_CB(tramp) if on_audio is not None else AUDIO_CB()
        rc = self.L.q3tts_synthesize_prefixed_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                   seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                                   _p(codes) if want_codes else None, int(chunk_frames), cb, None, _p(ids))
        if raised:
            raise raised[0]
        self._ck(rc)
        outs = [pcm[i][: pcm_len[i]] for i in range(n)]
        cl = [codes[i, : nfr[i]] for i in range(n)] if want_codes else None
        return outs, cl, nfr

    def synthesize_batch(self, token_lists, sp, lang=0, seed=0, ignore_eos=False, want_codes=True, speakers=None, max_new_per_utt=None, instructs=None,
                         share_instructs=False):
        """synthesize_tokens (reference src/tts_onnx.cpp:405-436) for a batch of utterances; `speakers` (one
        [hidden] embedding or None per utterance) makes it synthesize_clone (:264-318).  More utterances than slots queue
        (continuous batching); max_new_per_utt caps each utterance separately.  share_instructs: byte-equal instruction arrays become
        one shared prompt prefix each (prefilled once), the job runs through synthesize_prefixed and the prefixes are released after it."""
        n = len(token_lists)
        if share_instructs and instructs is not None:
            if len(instructs) != n:
                raise ValueError("instructs: one entry (framed ids or None) per utterance")
            made, ids = {}, []
            try:
                for t in instructs:
                    a = None if t is None else np.ascontiguousarray(t, np.int64).reshape(-1)
                    if a is None or a.size == 0:
                        ids.append(-1)
                        continue
                    key = a.tobytes()
                    if key not in made:
                        made[key] = self.prefix_create_instruct(a)
                    ids.append(made[key])
                return self.synthesize_prefixed(token_lists, ids, sp, lang=lang, seed=seed, ignore_eos=ignore_eos, want_codes=want_codes,
                                                speakers=speakers, max_new_per_utt=max_new_per_utt)
            finally:
                for pid in made.values():
                    self.prefix_release(pid)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in token_lists]))
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(t) for t in token_lists])
        cap = self.codec_decode_len(sp.max_new_tokens)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        nfr = np.zeros(n, np.int32)
        codes = np.zeros((n, sp.max_new_tokens, self.cfg.n_groups), np.int64) if want_codes else None
        spk_keep, spk_ptrs = [], None
        if speakers is not None:
            if len(speakers) != n:
                raise ValueError("speakers: one entry (embedding or None) per utterance")
            spk_keep = [None if s_ is None else np.ascontiguousarray(s_, np.float32) for s_ in speakers]
            for a in spk_keep:   # the library copies `hidden` floats from each row (the speaker row of the prompt is one talker-width embedding)
                if a is not None and a.size != self.cfg.hidden:
                    raise ValueError("speaker embedding has %d values, the model needs %d" % (a.size, self.cfg.hidden))
            spk_ptrs = C.cast((C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in spk_keep]), C.c_void_p)
        caps = None if max_new_per_utt is None else np.ascontiguousarray(max_new_per_utt, np.int32)
        if caps is not None and caps.shape != (n,):
            raise ValueError("max_new_per_utt: one entry per utterance")
        ins_flat, ins_offs = self._instruct_args(instructs, n)
        if ins_flat is not None:   # voice instructions (framed ids per utterance): q3tts_synthesize_instruct_host without a callback
            self._ck(self.L.q3tts_synthesize_instruct_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                           seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                                           _p(codes) if want_codes else None, 0, AUDIO_CB(), None, _p(ins_flat), _p(ins_offs)))
        else:
            self._ck(self.L.q3tts_synthesize_schedule_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                           seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                                           _p(codes) if want_codes else None))
        outs = [pcm[i][: pcm_len[i]] for i in range(n)]
        cl = [codes[i, : nfr[i]] for i in range(n)] if want_codes else None
        return outs, cl, nfr

    def synthesize_continue(self, token_lists, prefix_codes, sp, lang=0, seed=0, ignore_eos=False, speakers=None, max_new_per_utt=None,
                            chunk_frames=0, on_audio=None):
        """synthesize_batch with teacher-forced frames per utterance (q3tts_synthesize_continue_host): prefix_codes holds one
        [F0_u][n_groups] array (or None / empty: no prefix) per utterance.  Returns (pcm, codes, n_frames): codes[u] and n_frames[u]
        cover prefix + new frames, pcm[u] holds the NEW frames' samples only (they join the prefix's audio without a seam).
        on_audio (with chunk_frames >= 1): the audio is delivered while it is generated, as synthesize_stream delivers it
        (q3tts_synthesize_continue_stream_host); frame_begin / frame_end count the prefix, so an utterance's first call starts at its
        prefix length."""
        n = len(token_lists)
        if prefix_codes is None or len(prefix_codes) != n:
            raise ValueError("prefix_codes: one entry (codes or None) per utterance")
        if on_audio is not None and int(chunk_frames) < 1:
            raise ValueError("synthesize_continue: on_audio needs chunk_frames >= 1")
        if on_audio is None and chunk_frames:
            raise ValueError("synthesize_continue: chunk_frames without on_audio")
        pres = [self._frames(np.zeros((0, self.cfg.n_groups), np.int64) if c_ is None else c_, "synthesize_continue(prefix_codes)") for c_ in prefix_codes]
        poffs = np.zeros(n + 1, np.int32)
        poffs[1:] = np.cumsum([c_.shape[0] for c_ in pres])
        pflat = np.ascontiguousarray(np.concatenate(pres + [np.zeros((1, self.cfg.n_groups), np.int64)]))   # never empty: a valid pointer
        P = max(c_.shape[0] for c_ in pres) if n else 0
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in token_lists]))
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(t) for t in token_lists])
        cap = self.codec_decode_len(P + sp.max_new_tokens)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        nfr = np.zeros(n, np.int32)
        codes = np.zeros((n, P + sp.max_new_tokens, self.cfg.n_groups), np.int64)
        spk_keep, spk_ptrs = [], None
        if speakers is not None:
            if len(speakers) != n:
                raise ValueError("speakers: one entry (embedding or None) per utterance")
            spk_keep = [None if s_ is None else np.ascontiguousarray(s_, np.float32) for s_ in speakers]
            for a in spk_keep:
                if a is not None and a.size != self.cfg.hidden:
                    raise ValueError("speaker embedding has %d values, the model needs %d" % (a.size, self.cfg.hidden))
            spk_ptrs = C.cast((C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in spk_keep]), C.c_void_p)
        caps = None if max_new_per_utt is None else np.ascontiguousarray(max_new_per_utt, np.int32)
        if caps is not None and caps.shape != (n,):
            raise ValueError("max_new_per_utt: one entry per utterance")
        if on_audio is None:
            self._ck(self.L.q3tts_synthesize_continue_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                           seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr), _p(codes),
                                                           _p(pflat), _p(poffs)))
            return [pcm[i][: pcm_len[i]] for i in range(n)], [codes[i, : nfr[i]] for i in range(n)], nfr
        raised = []

        def tramp(_user, utt, fb, fe, p, ns, fin):
            try:
                a = np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns > 0 else np.zeros(0, np.float32)
                return 1 if on_audio(utt, fb, fe, a, bool(fin)) else 0
            except BaseException as ex:   # an exception must not cross the C frames: cancel the job, re-raise behind it
                raised.append(ex)
                return 1
        cb = AUDIO_CB(tramp)
        rc = self.L.q3tts_synthesize_continue_stream_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                          seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr), _p(codes),
                                                          _p(pflat), _p(poffs), int(chunk_frames), cb, None)
        if raised:
            raise raised[0]
        self._ck(rc)
        return [pcm[i][: pcm_len[i]] for i in range(n)], [codes[i, : nfr[i]] for i in range(n)], nfr

    def _sink_job(self, sample_rate, dtype, on_audio, n, run, speed=None, level=(0, 0), pitch=None, loud=None, tone=None):
        """a streaming job through a sink of its own: run(None-pcm_out) with the sink set, the sink taken away afterwards; the chunks
        on_audio saw are also returned joined per utterance"""
        fmt = _pcm_format("float32" if dtype is None else dtype)
        got = [[] for _ in range(n)]

        def tee(utt, fb, fe, a, fin):
            got[utt].append(a)
            return on_audio(utt, fb, fe, a, fin) if on_audio is not None else 0
        self.set_speed(speed)   # refuses a bad speed before the sink is set
        try:
            self.set_level(*level)
            self.set_pitch(1000 if pitch is None else pitch)
            self.set_loudness(*(loud if loud is not None else (None,)))
            self.set_tone(tone)
            self.set_sink(24000 if sample_rate is None else sample_rate, _PCM_NAMES[fmt], tee)
        except BaseException:
            self.set_speed(None)
            self.set_level(0, 0)
            self.set_pitch(1000)
            self.set_loudness(None)
            self.set_tone(None)
            raise
        try:
            rc = run()
        finally:
            raised = self._sink_raised
            self.set_sink(None)
            self.set_speed(None)
            self.set_level(0, 0)
            self.set_pitch(1000)
            self.set_loudness(None)
            self.set_tone(None)
        if raised:
            raise raised[0]
        self._ck(rc)
        npdt = _PCM_NP[fmt]
        return [np.concatenate(g) if g else np.zeros(0, npdt) for g in got]

    def synthesize_stream(self, token_lists, sp, chunk_frames, on_audio, lang=0, seed=0, ignore_eos=False, want_codes=True, speakers=None,
                          max_new_per_utt=None, instructs=None, sample_rate=None, dtype=None, speed=None, gain_db=None, ceiling=None, loudness=None, *, tone=None, pitch=None):
        """synthesize_batch that delivers audio while it generates (q3tts_synthesize_stream_host): every chunk_frames steps
        on_audio(utt, frame_begin, frame_end, pcm, finished) is called once per utterance with new audio (pcm: a copy); a truthy return
        cancels the job (RuntimeError "cancelled by callback").  Returns what synthesize_batch returns."""
        n = len(token_lists)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in token_lists]))
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(t) for t in token_lists])
        cap = self.codec_decode_len(sp.max_new_tokens)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        nfr = np.zeros(n, np.int32)
        codes = np.zeros((n, sp.max_new_tokens, self.cfg.n_groups), np.int64) if want_codes else None
        spk_keep, spk_ptrs = [], None
        if speakers is not None:
            if len(speakers) != n:
                raise ValueError("speakers: one entry (embedding or None) per utterance")
            spk_keep = [None if s_ is None else np.ascontiguousarray(s_, np.float32) for s_ in speakers]
            for a in spk_keep:
                if a is not None and a.size != self.cfg.hidden:
                    raise ValueError("speaker embedding has %d values, the model needs %d" % (a.size, self.cfg.hidden))
            spk_ptrs = C.cast((C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in spk_keep]), C.c_void_p)
        caps = None if max_new_per_utt is None else np.ascontiguousarray(max_new_per_utt, np.int32)
        if caps is not None and caps.shape != (n,):
            raise ValueError("max_new_per_utt: one entry per utterance")
        raised = []

        def tramp(_user, utt, fb, fe, p, ns, fin):
            try:
                a = np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns > 0 else np.zeros(0, np.float32)
                return 1 if on_audio(utt, fb, fe, a, bool(fin)) else 0
            except BaseException as ex:   # an exception must not cross the C frames: cancel the job, re-raise behind it
                raised.append(ex)
                return 1
        cb = AUDIO_CB(tramp)
        vp = C.c_void_p
        self.L.q3tts_synthesize_stream_host.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.POINTER(Sampling), vp, C.c_uint64, C.c_int, vp, C.c_int64, vp, vp, vp,
                                                        C.c_int, AUDIO_CB, vp]
        ins_flat, ins_offs = self._instruct_args(instructs, n)
        if speed is not None and int(speed) == 1000:
            speed = None   # no stage
        level = level_params(gain_db, ceiling)   # gain_db / ceiling: the chunks pass a level stage behind the stretcher (q3tts_engine_set_level)
        if pitch is not None and int(pitch) == 1000:
            pitch = None   # no stage; otherwise (permille) the chunks pass a pitch stage first (q3tts_engine_set_pitch)
        loud = None if loudness is None else loudness_params(loudness)   # LUFS, or (LUFS, range dB, start dB): a loudness stage behind the stretcher (q3tts_engine_set_loudness)
        if tone is not None and _tone_array(tone).shape[0] == 0:
            tone = None   # no stage; otherwise (a spec or sections) the chunks pass a tone stage behind the stretcher (q3tts_engine_set_tone)
        if sample_rate is not None or dtype is not None or speed is not None or level != (0, 0) or pitch is not None or loud is not None or tone is not None:   # through a sink (q3tts_engine_set_sink): sample_rate / dtype are the chunks' and the result's; speed (permille): time-stretched first (q3tts_engine_set_speed)
            def run():
                if ins_flat is not None:
                    return self.L.q3tts_synthesize_instruct_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                                 seed, int(ignore_eos), None, 0, _p(pcm_len), _p(nfr),
                                                                 _p(codes) if want_codes else None, int(chunk_frames), cb, None, _p(ins_flat), _p(ins_offs))
                return self.L.q3tts_synthesize_stream_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                           seed, int(ignore_eos), None, 0, _p(pcm_len), _p(nfr),
                                                           _p(codes) if want_codes else None, int(chunk_frames), cb, None)
            outs = self._sink_job(sample_rate, dtype, on_audio, n, run, speed, level, pitch, loud, tone)
            return outs, ([codes[i, : nfr[i]] for i in range(n)] if want_codes else None), nfr
        if ins_flat is not None:
            rc = self.L.q3tts_synthesize_instruct_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                       seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                                       _p(codes) if want_codes else None, int(chunk_frames), cb, None, _p(ins_flat), _p(ins_offs))
        else:
            rc = self.L.q3tts_synthesize_stream_host(self.h, n, _p(flat), _p(offs), lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                     seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                                     _p(codes) if want_codes else None, int(chunk_frames), cb, None)
        if raised:
            raise raised[0]
        self._ck(rc)
        outs = [pcm[i][: pcm_len[i]] for i in range(n)]
        cl = [codes[i, : nfr[i]] for i in range(n)] if want_codes else None
        return outs, cl, nfr

    def synthesize_live(self, n_utt, text_source, sp, chunk_frames, on_audio, lang=0, seed=0, ignore_eos=False, want_codes=True, speakers=None,
                        max_new_per_utt=None, sample_rate=None, dtype=None, speed=None, gain_db=None, ceiling=None, loudness=None, *, tone=None, pitch=None):
        """synthesize_stream for texts that arrive while their audio is generated (q3tts_synthesize_live_host): text_source(utt) ->
        (ids, closed) is polled between decode chunks for every utterance whose text is open — new ids (possibly none) and whether the
        text has ended; None cancels the job (RuntimeError "cancelled by callback").  An utterance's ids are those synthesize_stream
        takes (role ids first).  An exception in either callback cancels the job and is re-raised.  Returns what synthesize_stream returns."""
        n = int(n_utt)
        cap = self.codec_decode_len(sp.max_new_tokens)
        pcm = [np.zeros(cap, np.float32) for _ in range(n)]
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in pcm])
        pcm_len = np.zeros(n, np.int64)
        nfr = np.zeros(n, np.int32)
        codes = np.zeros((n, sp.max_new_tokens, self.cfg.n_groups), np.int64) if want_codes else None
        spk_keep, spk_ptrs = [], None
        if speakers is not None:
            if len(speakers) != n:
                raise ValueError("speakers: one entry (embedding or None) per utterance")
            spk_keep = [None if s_ is None else np.ascontiguousarray(s_, np.float32) for s_ in speakers]
            for a in spk_keep:
                if a is not None and a.size != self.cfg.hidden:
                    raise ValueError("speaker embedding has %d values, the model needs %d" % (a.size, self.cfg.hidden))
            spk_ptrs = C.cast((C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in spk_keep]), C.c_void_p)
        caps = None if max_new_per_utt is None else np.ascontiguousarray(max_new_per_utt, np.int32)
        if caps is not None and caps.shape != (n,):
            raise ValueError("max_new_per_utt: one entry per utterance")
        raised = []
        backlog = {}   # ids a poll returned beyond the callback's capacity

        def ttramp(_user, utt, ids, cap_ids, n_out, closed_out):
            try:
                if utt in backlog:
                    new, closed = backlog.pop(utt)
                else:
                    r = text_source(utt)
                    if r is None:   # the source gives the job up
                        return 1
                    new, closed = r
                    new = [int(v) for v in new]
                if len(new) > cap_ids:
                    backlog[utt] = (new[cap_ids:], closed)
                    new, closed = new[:cap_ids], False
                for i, v in enumerate(new):
                    ids[i] = v
                n_out[0] = len(new)
                closed_out[0] = 1 if closed else 0
                return 0
            except BaseException as ex:
                raised.append(ex)
                return 1

        def tramp(_user, utt, fb, fe, p, ns, fin):
            try:
                a = np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns > 0 else np.zeros(0, np.float32)
                return 1 if on_audio(utt, fb, fe, a, bool(fin)) else 0
            except BaseException as ex:
                raised.append(ex)
                return 1
        cb, tcb = AUDIO_CB(tramp), TEXT_CB(ttramp)
        if speed is not None and int(speed) == 1000:
            speed = None
        level = level_params(gain_db, ceiling)
        if pitch is not None and int(pitch) == 1000:
            pitch = None
        loud = None if loudness is None else loudness_params(loudness)
        if tone is not None and _tone_array(tone).shape[0] == 0:
            tone = None
        if sample_rate is not None or dtype is not None or speed is not None or level != (0, 0) or pitch is not None or loud is not None or tone is not None:   # through a sink and / or a stretcher, as synthesize_stream
            def run():
                return self.L.q3tts_synthesize_live_host(self.h, n, tcb, None, lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                                         seed, int(ignore_eos), None, 0, _p(pcm_len), _p(nfr),
                                                         _p(codes) if want_codes else None, int(chunk_frames), cb, None)
            try:
                outs = self._sink_job(sample_rate, dtype, on_audio, n, run, speed, level, pitch, loud, tone)
            except BaseException:
                if raised:
                    raise raised[0]
                raise
            return outs, ([codes[i, : nfr[i]] for i in range(n)] if want_codes else None), nfr
        rc = self.L.q3tts_synthesize_live_host(self.h, n, tcb, None, lang, spk_ptrs, C.byref(sp), None if caps is None else _p(caps),
                                               seed, int(ignore_eos), C.cast(ptrs, C.c_void_p), cap, _p(pcm_len), _p(nfr),
                                               _p(codes) if want_codes else None, int(chunk_frames), cb, None)
        if raised:
            raise raised[0]
        self._ck(rc)
        outs = [pcm[i][: pcm_len[i]] for i in range(n)]
        cl = [codes[i, : nfr[i]] for i in range(n)] if want_codes else None
        return outs, cl, nfr

    # ---- measurement ----
    def last_decode_ms(self):
        ms, st = C.c_float(0), C.c_int(0)
        self._ck(self.L.q3tts_last_decode_ms(self.h, C.byref(ms), C.byref(st)))
        return ms.value, st.value

    def last_codec_ms(self):
        ms = C.c_float(0)
        self._ck(self.L.q3tts_last_codec_ms(self.h, C.byref(ms)))
        return ms.value

    def counters(self, reset=False):
        dms, cms = C.c_double(0), C.c_double(0)
        ds, cf = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.q3tts_counters(self.h, C.byref(dms), C.byref(ds), C.byref(cms), C.byref(cf), int(reset)))
        return dict(decode_ms=dms.value, decode_steps=ds.value, codec_ms=cms.value, codec_frames=cf.value)

    def codec_decode_dev(self, codes_ptr, F, pcm_ptr, cap):
        """codes_ptr: device address of int32 [F][n_groups]; pcm_ptr: device address of float [cap] (e.g. torch tensors' data_ptr())."""
        n = C.c_int64(0)
        self.L.q3tts_codec_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        self._ck(self.L.q3tts_codec_decode_dev(self.h, C.c_void_p(codes_ptr), int(F), C.c_void_p(pcm_ptr), int(cap), C.byref(n)))
        return n.value

    @property
    def stream(self):
        self.L.q3tts_stream.restype = C.c_void_p
        self.L.q3tts_stream.argtypes = [C.c_void_p]
        return self.L.q3tts_stream(self.h)

    # ---- batch-first device-pointer entry points: integer arguments are device addresses (0 = NULL) ----
    def talker_prefill_dev(self, embeds_ptr, batch, S, lens=None, logits_ptr=0, hidden_ptr=0, stream=0):
        ln = None if lens is None else np.ascontiguousarray(lens, np.int32)
        self.L.q3tts_talker_prefill_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_talker_prefill_dev(self.h, embeds_ptr, batch, S, _p(ln) if ln is not None else None, logits_ptr or None, hidden_ptr or None, stream or None))

    def talker_decode_dev(self, embeds_ptr, batch, active=None, logits_ptr=0, hidden_ptr=0, stream=0):
        m = None if active is None else np.ascontiguousarray(active, np.uint8)
        self.L.q3tts_talker_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_talker_decode_dev(self.h, embeds_ptr, batch, _p(m) if m is not None else None, logits_ptr or None, hidden_ptr or None, stream or None))

    def code_predictor_dev(self, hidden_ptr, code0_ptr, batch, sp, seed, stream_id0, frame, sub_ptr, stream=0):
        self.L.q3tts_code_predictor_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_code_predictor_dev(self.h, hidden_ptr, code0_ptr, batch, C.byref(sp), seed, stream_id0, frame, sub_ptr, stream or None))

    def sample_dev(self, logits_ptr, batch, n, sp, u_ptr, suppress, ids_ptr, stream=0):
        self.L.q3tts_sample_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_sample_dev(self.h, logits_ptr, batch, n, C.byref(sp), u_ptr, int(suppress), ids_ptr, stream or None))

    def sample_hist_dev(self, logits_ptr, batch, n, sp, u_ptr, suppress, hist_ptr, hist_ld, hist_len_ptr, ids_ptr, stream=0):
        self.L.q3tts_sample_hist_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_sample_hist_dev(self.h, logits_ptr, batch, n, C.byref(sp), u_ptr, int(suppress), hist_ptr, hist_ld, hist_len_ptr, ids_ptr,
                                              stream or None))

    def poison_workspace(self):
        """test hook (FLAG_TEST_HOOKS engines): NaN bytes over the vocoder's reusable workspace (q3tts_test_poison_workspace)"""
        self.L.q3tts_test_poison_workspace.argtypes = [C.c_void_p]
        self._ck(self.L.q3tts_test_poison_workspace(self.h))

    def group_final_conv(self):
        """test hook: (sx [nb][T][C], pcm [nb][T]) of the last batched vocoder group's final conv, read back from its lane's workspace"""
        T, Cc, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.L.q3tts_test_group_final_conv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        self._ck(self.L.q3tts_test_group_final_conv(self.h, None, None, 0, C.byref(T), C.byref(Cc), C.byref(nb)))
        sx = np.empty((nb.value, T.value, Cc.value), np.float32)
        pcm = np.empty((nb.value, T.value), np.float32)
        self._ck(self.L.q3tts_test_group_final_conv(self.h, _p(sx), _p(pcm), sx.size, C.byref(T), C.byref(Cc), C.byref(nb)))
        return sx, pcm

    def final_conv_partials(self):
        """test hook: [tiles][256][8] partial sums of the last batched group's final conv (Q3TTS_COUT1_PACKED=2 only), or None"""
        f = self.L.q3tts_test_final_conv_partials
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        f.restype = C.c_int64
        n = f(self.h, None, 0)
        if n <= 0:
            return None
        out = np.empty(n, np.float32)
        f(self.h, _p(out), n)
        return out.reshape(-1, 256, 8)

    def measure_skip_frames(self, n):
        """measurement aid (FLAG_TEST_HOOKS engines): armed slots jump n frames ahead over a synthetic KV cache (q3tts_measure_skip_frames)"""
        self.L.q3tts_measure_skip_frames.argtypes = [C.c_void_p, C.c_int]
        self._ck(self.L.q3tts_measure_skip_frames(self.h, int(n)))

    def codec_plane_stats(self):
        """(two_product, three_product): codec weight tensors whose fp16 lo plane is empty / needed (q3tts_codec_plane_stats)"""
        a, b = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.q3tts_codec_plane_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def prefill_profile(self, n_slots, n_rows=8, reps=4):
        """mean device ms of a batched prefill pass of n_slots free slots x n_rows synthetic prompt rows (q3tts_prefill_profile)"""
        out = C.c_double(0.0)
        self.L.q3tts_prefill_profile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        self._ck(self.L.q3tts_prefill_profile(self.h, int(n_slots), int(n_rows), int(reps), C.byref(out)))
        return out.value

    def stage_profile(self, n_steps=32):
        """ms per step of {sampler, code predictor, talker decode, sum}: eager steps with events at the stage boundaries."""
        out = (C.c_double * 4)()
        self._ck(self.L.q3tts_stage_profile(self.h, int(n_steps), out))
        return dict(sampler_ms=out[0], code_predictor_ms=out[1], talker_decode_ms=out[2], step_ms=out[3])

    def decode_step_bytes(self):
        w, kv = C.c_double(0), C.c_double(0)
        self._ck(self.L.q3tts_decode_step_bytes(self.h, C.byref(w), C.byref(kv)))
        return w.value, kv.value


def read_wav(path):
    """io::read_wav (reference src/io/wav_reader.cpp:28-143): (mono float32 samples, sample_rate) or None.  Host-only."""
    n, sr = C.c_int64(0), C.c_int32(0)
    if lib().q3tts_read_wav_host(os.fsencode(path), None, 0, C.byref(n), C.byref(sr)) != 0:
        return None
    out = np.zeros(n.value, np.float32)
    lib().q3tts_read_wav_host(os.fsencode(path), _p(out), n.value, C.byref(n), C.byref(sr))
    return out, sr.value


def resample(audio, src_rate, dst_rate):
    """io::resample (wav_reader.cpp:145-164).  Host-only."""
    a = np.ascontiguousarray(audio, np.float32)
    n = lib().q3tts_resample_host(_p(a), a.size, src_rate, dst_rate, None, 0)
    if n < 0:
        raise ValueError("q3tts_resample_host failed")
    out = np.zeros(max(n, 1), np.float32)
    lib().q3tts_resample_host(_p(a), a.size, src_rate, dst_rate, _p(out), n)
    return out[:n]


def resample_stream_emitted(src_rate, dst_rate, n_received, finish=False):
    """q3tts_resample_stream_emitted: the output samples a stream at src_rate has emitted in all once it holds n_received samples
    (finish: resample's own length).  A push's length is the difference of two calls.  Host-only."""
    n = int(lib().q3tts_resample_stream_emitted(int(src_rate), int(dst_rate), int(n_received), 1 if finish else 0))
    if n < 0:
        raise ValueError("resample_stream_emitted: rates must be positive and n_received not negative")
    return n


PCM_F32, PCM_S16, PCM_MULAW, PCM_ALAW = 0, 1, 2, 3
_PCM_NAMES = {PCM_F32: "float32", PCM_S16: "int16", PCM_MULAW: "mulaw", PCM_ALAW: "alaw"}
_PCM_NP = {PCM_F32: np.float32, PCM_S16: np.int16, PCM_MULAW: np.uint8, PCM_ALAW: np.uint8}


def sink_plan(sample_rate, want_table=True):
    """q3tts_sink_plan: -> (L, M, half, taps, table [L][taps] float32, or None) of the output resampler for sample_rate.  Host-only;
    ValueError naming the rate when it is refused."""
    Lb = lib()
    Lb.q3tts_sink_plan.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int64]
    Lb.q3tts_sink_last_error.restype = C.c_char_p
    L_, M_, h_, t_ = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if Lb.q3tts_sink_plan(int(sample_rate), C.byref(L_), C.byref(M_), C.byref(h_), C.byref(t_), None, 0) != 0:
        raise ValueError(Lb.q3tts_sink_last_error().decode())
    tab = None
    if want_table:
        tab = np.zeros((L_.value, t_.value), np.float32)
        if tab.size and Lb.q3tts_sink_plan(int(sample_rate), None, None, None, None, _p(tab), tab.size) != 0:
            raise ValueError(Lb.q3tts_sink_last_error().decode())
    return L_.value, M_.value, h_.value, t_.value, tab


def sink_emitted(sample_rate, n_received, finished=False):
    """q3tts_sink_emitted: the samples a sink at sample_rate has delivered in all after n_received samples at 24 kHz.  Host-only."""
    Lb = lib()
    Lb.q3tts_sink_emitted.argtypes = [C.c_int32, C.c_int64, C.c_int]
    Lb.q3tts_sink_emitted.restype = C.c_int64
    Lb.q3tts_sink_last_error.restype = C.c_char_p
    n = int(Lb.q3tts_sink_emitted(int(sample_rate), int(n_received), 1 if finished else 0))
    if n < 0:
        raise ValueError(Lb.q3tts_sink_last_error().decode())
    return n


def speed_emitted(speed, n_received, finished=False):
    """q3tts_speed_emitted: the samples a stretcher at speed (permille) has delivered in all after n_received samples.  Host-only;
    ValueError naming the value when it is refused."""
    Lb = lib()
    Lb.q3tts_speed_emitted.argtypes = [C.c_int32, C.c_int64, C.c_int]
    Lb.q3tts_speed_emitted.restype = C.c_int64
    Lb.q3tts_speed_last_error.restype = C.c_char_p
    if not -2 ** 31 <= int(speed) < 2 ** 31 or not -2 ** 63 <= int(n_received) < 2 ** 63:
        raise ValueError("speed_emitted: %d / %d does not fit the C types" % (int(speed), int(n_received)))
    n = int(Lb.q3tts_speed_emitted(int(speed), int(n_received), 1 if finished else 0))
    if n < 0:
        raise ValueError(Lb.q3tts_speed_last_error().decode())
    return n


def level_params(gain_db=None, ceiling=None):
    """(gain_db, ceiling) as the C-ABI takes them: gain_db (decibels, float) rounded to the nearest centibel, ceiling (linear, 0 .. 1,
    float) rounded to the nearest permille; None: 0.  A positive ceiling below half a permille is refused (it would round to "no limiter")."""
    g = 0 if gain_db is None else int(round(10.0 * float(gain_db)))
    c = 0 if ceiling is None else int(round(1000.0 * float(ceiling)))
    if ceiling is not None and float(ceiling) > 0 and c == 0:
        raise ValueError("level: ceiling %r rounds to 0 permille, which means no limiter" % (ceiling,))
    return g, c


def loudness_params(loudness, loudness_range=None, loudness_start=None):
    """(LUFS, range dB, start dB) -> (target_dlufs, range_cb, start_cb), rounded to the units of the C-ABI.  loudness may itself be the
    triple.  Range None: 20 dB; start None: 0 dB.  loudness 0 is meter only."""
    if isinstance(loudness, (tuple, list)):
        loudness, loudness_range, loudness_start = (list(loudness) + [None, None])[:3]
    return (int(round(10.0 * float(loudness))), 200 if loudness_range is None else int(round(10.0 * float(loudness_range))),
            0 if loudness_start is None else int(round(10.0 * float(loudness_start))))


TONE_KINDS = {"highpass": 1, "lowpass": 2, "lowshelf": 3, "highshelf": 4, "peak": 5}


def tone_sections(spec):
    """q3tts_tone_parse: the sections of a spec string as an int32 array [n][4] of (kind, freq_hz, gain_cb, q_permille).  A spec is a
    preset's name (telephone, rumble, presence, warm: unheard and untuned) or sections separated by commas, kind:Hz:Q for hp and lp,
    kind:Hz:dB:Q for ls, hs and peak, e.g. "hp:300:0.707,peak:2500:+3:1.0,lp:3400:0.707".  Host-only; ValueError names what could not be
    read or is out of range."""
    Lb = lib()
    Lb.q3tts_tone_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    Lb.q3tts_tone_parse.restype = C.c_int
    Lb.q3tts_tone_last_error.restype = C.c_char_p
    out = np.zeros((8, 4), np.int32)
    n = C.c_int32(0)
    if Lb.q3tts_tone_parse(str(spec).encode(), out.ctypes.data, C.byref(n)) != 0:
        raise ValueError(Lb.q3tts_tone_last_error().decode())
    return out[: n.value].copy()


def _tone_array(tone):
    """None / a spec string / rows of (kind, freq_hz, gain_cb, q_permille) -> int32 [n][4]; the library checks the values"""
    if tone is None:
        return np.zeros((0, 4), np.int32)
    if isinstance(tone, str):
        return tone_sections(tone)
    a = np.asarray(tone)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("tone: sections are integers (kind, freq_hz, gain_cb, q_permille)")
    return np.ascontiguousarray(a, np.int32).reshape(-1, 4)


def tone_coeffs(tone):
    """q3tts_tone_coeffs: float64 [n][5], { b0, b1, b2, a1, a2 } of every section, the very doubles the device uses.  tone a spec
    string or a list of sections.  Host-only; ValueError names the field, the section and the value that is out of range."""
    arr = _tone_array(tone)
    Lb = lib()
    Lb.q3tts_tone_coeffs.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    Lb.q3tts_tone_coeffs.restype = C.c_int
    Lb.q3tts_tone_last_error.restype = C.c_char_p
    out = np.zeros((max(arr.shape[0], 1), 5), np.float64)
    if Lb.q3tts_tone_coeffs(arr.shape[0], arr.ctypes.data if arr.shape[0] else None, out.ctypes.data) != 0:
        raise ValueError(Lb.q3tts_tone_last_error().decode())
    return out[: arr.shape[0]]


def loudness_coeffs(rate=24000):
    """q3tts_loudness_coeffs: the ten doubles { b0, b1, b2, a1, a2 } of the K-weighting's shelf, then of its high-pass, at rate.
    Host-only; ValueError outside 8000 .. 384000."""
    Lb = lib()
    Lb.q3tts_loudness_coeffs.argtypes = [C.c_int32, C.c_void_p]
    Lb.q3tts_loudness_coeffs.restype = C.c_int
    Lb.q3tts_loudness_last_error.restype = C.c_char_p
    out = np.zeros(10, np.float64)
    if Lb.q3tts_loudness_coeffs(int(rate), out.ctypes.data) != 0:
        raise ValueError(Lb.q3tts_loudness_last_error().decode())
    return out


def loudness_emitted(target_dlufs, n_received, finished=False):
    """q3tts_loudness_emitted: the samples a loudness stage has delivered in all after n_received samples.  Host-only; ValueError for
    a negative count."""
    Lb = lib()
    Lb.q3tts_loudness_emitted.argtypes = [C.c_int32, C.c_int64, C.c_int]
    Lb.q3tts_loudness_emitted.restype = C.c_int64
    Lb.q3tts_loudness_last_error.restype = C.c_char_p
    if not -2**63 <= int(n_received) < 2**63:
        raise ValueError("loudness_emitted: %d does not fit the C type" % int(n_received))
    n = int(Lb.q3tts_loudness_emitted(int(target_dlufs), int(n_received), 1 if finished else 0))
    if n < 0:
        raise ValueError(Lb.q3tts_loudness_last_error().decode())
    return n


LOUDNESS_MODES = {"momentary": 0, "short-term": 1, "integrated": 2}


def loudness_lufs(energies, mode="integrated"):
    """q3tts_loudness_lufs: LUFS of the sub-block energies a loudness stage reported; mode momentary (the last 400 ms), short-term
    (the last 3 s) or integrated (BS.1770's two gates).  -inf when nothing passes.  Host-only."""
    Lb = lib()
    Lb.q3tts_loudness_lufs.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    Lb.q3tts_loudness_lufs.restype = C.c_double
    Lb.q3tts_loudness_last_error.restype = C.c_char_p
    E = np.ascontiguousarray(energies, np.int64).reshape(-1)
    v = float(Lb.q3tts_loudness_lufs(E.ctypes.data if E.size else None, E.size, LOUDNESS_MODES[mode] if isinstance(mode, str) else int(mode)))
    if v != v:
        raise ValueError(Lb.q3tts_loudness_last_error().decode())
    return v


def pitch_ratio(cents):
    """q3tts_pitch_ratio: round(1000 * 2^(cents / 1200)), the permille ratio of a shift by cents.  Host-only; ValueError outside
    -1200 .. 1200."""
    Lb = lib()
    Lb.q3tts_pitch_ratio.argtypes = [C.c_double]
    Lb.q3tts_pitch_ratio.restype = C.c_int32
    Lb.q3tts_pitch_last_error.restype = C.c_char_p
    r = int(Lb.q3tts_pitch_ratio(float(cents)))
    if r < 0:
        raise ValueError(Lb.q3tts_pitch_last_error().decode())
    return r


def pitch_emitted(n_received, finished=False):
    """q3tts_pitch_emitted: the samples a pitch stage has delivered in all after n_received samples.  Host-only; ValueError for a
    negative count."""
    Lb = lib()
    Lb.q3tts_pitch_emitted.argtypes = [C.c_int64, C.c_int]
    Lb.q3tts_pitch_emitted.restype = C.c_int64
    Lb.q3tts_pitch_last_error.restype = C.c_char_p
    if not -2**63 <= int(n_received) < 2**63:
        raise ValueError("pitch_emitted: %d does not fit the C type" % int(n_received))
    n = int(Lb.q3tts_pitch_emitted(int(n_received), 1 if finished else 0))
    if n < 0:
        raise ValueError(Lb.q3tts_pitch_last_error().decode())
    return n


def level_gain(gain_cb):
    """q3tts_level_gain: the float32 g = 10^(gain_cb / 200) the device uses.  Host-only; ValueError (naming the value) outside -600 .. 400."""
    Lb = lib()
    Lb.q3tts_level_gain.argtypes = [C.c_int32]
    Lb.q3tts_level_gain.restype = C.c_float
    Lb.q3tts_level_last_error.restype = C.c_char_p
    if not -2 ** 31 <= int(gain_cb) < 2 ** 31:
        raise ValueError("level_gain: %d does not fit the C type" % int(gain_cb))
    g = np.float32(Lb.q3tts_level_gain(int(gain_cb)))
    if g < 0:
        raise ValueError(Lb.q3tts_level_last_error().decode())
    return g


def level_emitted(gain_cb, ceiling_permille, n_received, finished=False):
    """q3tts_level_emitted: the samples a level stage has delivered in all after n_received samples.  Host-only; ValueError (naming the
    value) for parameters out of range or a negative count."""
    Lb = lib()
    Lb.q3tts_level_emitted.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int]
    Lb.q3tts_level_emitted.restype = C.c_int64
    Lb.q3tts_level_last_error.restype = C.c_char_p
    if not (-2 ** 31 <= int(gain_cb) < 2 ** 31 and -2 ** 31 <= int(ceiling_permille) < 2 ** 31 and -2 ** 63 <= int(n_received) < 2 ** 63):
        raise ValueError("level_emitted: %d / %d / %d does not fit the C types" % (int(gain_cb), int(ceiling_permille), int(n_received)))
    n = int(Lb.q3tts_level_emitted(int(gain_cb), int(ceiling_permille), int(n_received), 1 if finished else 0))
    if n < 0:
        raise ValueError(Lb.q3tts_level_last_error().decode())
    return n


def speed_window():
    """q3tts_speed_window: the 720-entry float32 window the device uses.  Host-only."""
    Lb = lib()
    Lb.q3tts_speed_window.argtypes = [C.c_void_p, C.c_int64]
    w = np.zeros(720, np.float32)
    if Lb.q3tts_speed_window(_p(w), w.size) != 0:
        raise ValueError("speed_window failed")
    return w


def _pcm_format(dtype):
    name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
    if name in ("float32", "f32"):
        return PCM_F32
    if name in ("int16", "s16"):
        return PCM_S16
    if name in ("mulaw", "ulaw"):
        return PCM_MULAW
    if name == "alaw":
        return PCM_ALAW
    raise ValueError("dtype must be float32 or int16, or the G.711 names mulaw / ulaw / alaw, got %r" % (dtype,))


def _g711_format(law):
    fmt = law if isinstance(law, (int, np.integer)) else _pcm_format(law)
    return int(fmt)


def g711_encode(law, pcm16):
    """int16 samples -> G.711 bytes (np.uint8) under law "mulaw" / "ulaw" / "alaw" (or PCM_MULAW / PCM_ALAW): the arithmetic of
    include/q3tts.h "G.711", the functions the sink kernel uses.  Host-only.  Any other law raises ValueError."""
    a = np.asarray(pcm16)
    if a.size and a.dtype != np.int16:
        raise ValueError("g711_encode: expected int16 samples, got dtype %s" % a.dtype)
    a = np.ascontiguousarray(a, np.int16)
    out = np.empty(a.shape, np.uint8)
    Lb = lib()
    Lb.q3tts_g711_encode_host.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    if Lb.q3tts_g711_encode_host(_g711_format(law), _p(a), a.size, _p(out)) != 0:
        raise ValueError("g711_encode: law must be mulaw (2) or alaw (3), got %r" % (law,))
    return out


def g711_decode(law, data):
    """G.711 bytes (np.uint8) -> int16 samples; the functions the encoder streams' kernel uses.  Host-only."""
    a = np.asarray(data)
    if a.size and a.dtype != np.uint8:
        raise ValueError("g711_decode: expected uint8 bytes, got dtype %s" % a.dtype)
    a = np.ascontiguousarray(a, np.uint8)
    out = np.empty(a.shape, np.int16)
    Lb = lib()
    Lb.q3tts_g711_decode_host.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    if Lb.q3tts_g711_decode_host(_g711_format(law), _p(a), a.size, _p(out)) != 0:
        raise ValueError("g711_decode: law must be mulaw (2) or alaw (3), got %r" % (law,))
    return out


def log_mel(audio):
    """MelExtractor::extract with the clone path's settings (tts_onnx.cpp:347-354): [128][frames].  Host-only."""
    a = np.ascontiguousarray(audio, np.float32)
    fr = C.c_int32(0)
    if lib().q3tts_mel_host(_p(a), a.size, None, 0, C.byref(fr)) != 0:
        return np.zeros((128, 0), np.float32)
    out = np.zeros((128, fr.value), np.float32)
    if lib().q3tts_mel_host(_p(a), a.size, _p(out), out.size, C.byref(fr)) != 0:
        raise RuntimeError("q3tts_mel_host failed")
    return out


class Tokenizer:
    """Byte-level BPE tokenizer of the text prompt (q3tts_tokenizer_*; reference src/io/tokenizer.h:13-22).
    Host-only: usable without a GPU."""

    def __init__(self, vocab_json=None, merges_txt=None):
        self._h = lib().q3tts_tokenizer_create()
        if not self._h:
            raise MemoryError("q3tts_tokenizer_create failed")
        if vocab_json is not None and not self.load_vocab(vocab_json):
            raise ValueError(f"cannot load vocab {vocab_json}")
        if merges_txt is not None and not self.load_merges(merges_txt):
            raise ValueError(f"cannot load merges {merges_txt}")

    def load_vocab(self, path):
        return lib().q3tts_tokenizer_load_vocab(self._h, os.fsencode(path)) == 0

    def load_merges(self, path):
        return lib().q3tts_tokenizer_load_merges(self._h, os.fsencode(path)) == 0

    @property
    def ready(self):
        return bool(lib().q3tts_tokenizer_ready(self._h))

    def encode(self, text):
        b = text if isinstance(text, (bytes, bytearray)) else text.encode("utf-8")
        b = bytes(b)
        n = lib().q3tts_tokenize(self._h, b, len(b), None, 0)
        if n < 0:
            raise RuntimeError("q3tts_tokenize failed")
        out = np.zeros(max(n, 1), np.int32)
        lib().q3tts_tokenize(self._h, b, len(b), out.ctypes.data_as(C.POINTER(C.c_int32)), n)
        return out[:n]

    def close(self):
        if self._h:
            lib().q3tts_tokenizer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_instruct_ids(text_ids):
    """[HINT], unpinned (include/q3tts.h: q3tts_frame_instruct_ids): a tokenised instruction framed as the chat turn
    <|im_start|>user\\n ... <|im_end|>\\n — what build_prompt(instruct_ids=...) and synthesize_batch(instructs=...) take.  Host-only."""
    t = np.ascontiguousarray(text_ids, np.int32).reshape(-1)
    L = lib()
    n = L.q3tts_frame_instruct_ids(_p(t) if t.size else None, t.size, None, 0)
    if n < 0:
        raise ValueError("frame_instruct_ids: bad argument")
    out = np.zeros(n, np.int64)
    L.q3tts_frame_instruct_ids(_p(t) if t.size else None, t.size, _p(out), n)
    return out


def save_codes(path, codes):
    """the text format of leaxer-tts --save-codes / --continue-codes: one frame per line, n_groups integers.  Host-only."""
    c = np.asarray(codes, np.int64)
    if c.ndim != 2:
        raise ValueError("save_codes: expected [frames][n_groups]")
    with open(path, "w") as f:
        for row in c:
            f.write(" ".join(str(int(v)) for v in row) + "\n")


def load_codes(path):
    """reads what save_codes / leaxer-tts --save-codes wrote: int64 [frames][n_groups].  Host-only."""
    rows = [[int(v) for v in line.replace(",", " ").split()] for line in open(path) if line.strip()]
    if not rows:
        return np.zeros((0, 0), np.int64)
    if any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("load_codes: lines of different lengths in %s" % path)
    return np.array(rows, np.int64)


def rng_uniform(seed, stream, frame, group):
    return float(lib().q3tts_rng_uniform(seed, stream, frame, group))


class AudioEncodeStream:
    """One encoder stream as a context manager: push(pcm) -> the new codes, finish() -> the last ones, .codes: everything so far
    [F][n_groups].  The concatenation is bit-identical to Engine.audio_encode_batch of the concatenated audio at sample_rate (mono;
    dtype float32 or int16, or "mulaw" / "alaw" for G.711 bytes as np.uint8)."""

    def __init__(self, engine, max_samples=0, sample_rate=24000, dtype="float32"):
        self.engine = engine
        self.sid = engine.audio_stream_begin_rate(sample_rate, dtype, max_samples)
        self._parts = []
        self.finished = False

    def push(self, pcm, finish=False):
        if self.sid is None:
            raise RuntimeError("the stream is closed")
        if self.finished:
            raise RuntimeError("the stream is finished")
        codes = self.engine.audio_stream_push(self.sid, pcm, finish)
        self.finished = bool(finish)
        if codes.shape[0]:
            self._parts.append(codes)
        return codes

    def finish(self):
        return self.push(np.zeros(0, np.float32), finish=True)

    @property
    def codes(self):
        if not self._parts:
            return np.zeros((0, self.engine.cfg.n_groups), np.int64)
        return np.concatenate(self._parts, axis=0)

    def close(self):
        if self.sid is not None:
            self.engine.audio_stream_end(self.sid)
            self.sid = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
