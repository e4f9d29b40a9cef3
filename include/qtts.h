/*
 * qtts.h -- C ABI of the MI355X-native Qwen3-TTS hot path (libqtts.so, gfx950 only).
 *
 * The reference (QwenLM/Qwen3-TTS) is 100 % Python and has no FFI of its own; its drop-in
 * boundary is the Python API of `qwen_tts.inference`.  This header is the native
 * seam *below* that API.  Each entry point replaces one reference call (cited per function);
 * the Python host code in `qwen3-tts_amd/` keeps the reference's names/arguments and calls these
 * through ctypes (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Rules of the boundary
 *   - plain C types only: pointers, sizes, POD structs.  No torch / HIP types in signatures
 *     (`stream` is a `hipStream_t` passed as `void*`; NULL = the default stream).
 *   - return 0 (QTTS_OK) or a negative QTTS_ERR_*; qtts_last_error() gives the message of the
 *     last failure on the calling thread.  No exceptions cross the ABI.
 *   - weights are bound from HOST memory in the reference's own state_dict layout and naming
 *     (SURVEY.md Appendix B); the library repacks them once into its streaming layouts in HBM.
 *   - activations / codes / waveforms are DEVICE pointers owned by the caller (PyTorch-ROCm
 *     allocations in the shipped host code); the library borrows them for the call only.
 *   - one handle per (process, device); a handle is not re-entrant (the reference keeps
 *     per-call state on the module too: modeling_qwen3_tts.py:1704 `self.rope_deltas`).
 */
#ifndef QTTS_H
#define QTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QTTS_OK 0
#define QTTS_ERR_ARG (-1)     /* bad argument / shape                                      */
#define QTTS_ERR_HIP (-2)     /* a HIP runtime call failed                                 */
#define QTTS_ERR_STATE (-3)   /* call order violated (e.g. decode before finalize/prefill) */
#define QTTS_ERR_UNBOUND (-4) /* finalize(): a required weight was never bound             */
#define QTTS_ERR_NAME (-5)    /* bind(): unknown parameter name                            */
#define QTTS_ERR_LIMIT (-6)   /* exceeds max_batch / max_seq given at create               */

/* storage / arithmetic type of weights and KV cache inside the engine */
#define QTTS_F32 0  /* parity mode: fp32 weights, exact-f32 MFMA (v_mfma_f32_16x16x4_f32)   */
#define QTTS_BF16 1 /* perf mode:   bf16 weights + KV, v_mfma_f32_16x16x32_bf16, f32 accum  */

const char* qtts_last_error(void);
/* ABI version of this header; bumped on any signature change (2: + qtts_talker_text_embed, qtts_talker_assemble_rows;
 * 3: + qtts_codec_stream_begin, qtts_codec_stream_push; 4: + qtts_encoder_*; 5: + qtts_speaker_*;
 * 6: + qtts_talker_stream_*; 7: + qtts_talker_set_teacher; 8: + qtts_talker_set_profile / get_gemm_profile;
 * 9: + qtts_codec_get_stats; 10: + qtts_set_option / qtts_get_option, qtts_talker_stats grew the fused-launch fields;
 * 11: + qtts_talker_debug_cp_logits, qtts_talker_stats.cp_layer_per_step in the reserved word;
 * 12: + qtts_talker_stats.ks_split_per_step (appended); 13: qtts_talker_stats.attn_gq_per_step in the reserved word, the talker
 * engine takes head_dim 64 | 128 and GQA groups of 1..8; 14: + qtts_row_sampling, qtts_talker_generate_rows,
 * qtts_talker_stream_begin_rows, qtts_talker_stats.graph_captures / row_table_last (appended); 15: + qtts_talker_stream_begin_admitting,
 * qtts_talker_stream_admit, qtts_talker_stream_rows, qtts_talker_stats.admit_calls / admitted_rows (two words IN FRONT of row_table_last:
 * the struct's tail moved by 8 bytes); still 15: + qtts_codec_stream_reset_rows, qtts_codec_stream_push_rows -- two entry points
 * added, no signature and no struct layout changed; a binding that needs them finds out by looking the symbols up; still 15:
 * + qtts_talker_stream_begin_admitting_rows, qtts_talker_stream_row_lens, qtts_talker_stream_mode -- three entry points added, no
 * signature and no struct layout changed: qtts_talker_stats is byte for byte what it was, so a v15 binding keeps working and one that
 * needs the new calls finds out by looking the symbols up; still 15: + qtts_row_warpers, qtts_talker_set_row_warpers,
 * qtts_talker_sampler_class -- a new struct and two entry points, no existing signature or struct changed; still 15:
 * + qtts_codec_stream_prime_rows, qtts_codec_stream_prime_tail -- two entry points added, no signature and no struct changed; a binding
 * that needs them finds out by looking the symbols up; still 15: + qtts_row_processors, qtts_talker_set_row_processors -- a new
 * struct and one entry point, no existing signature or struct changed; still 15: + qtts_speaker_embed_ragged -- one entry point
 * added, no signature and no struct changed). */
#define QTTS_ABI_VERSION 15
int qtts_abi_version(void);

/* A/B switches of the library (measuring tools and tests; a deployment sets none).  Every switch has a name of the form
 * "QTTS_..." (the list: DESIGN.md "switches"); its value is, in this order, what qtts_set_option last gave it, else the
 * environment variable of the same name as it was when the library first looked, else the built-in default.  Engine-level
 * switches are copied into a handle when it is CREATED (qtts_*_create): later changes do not touch existing handles.
 * Launcher-level switches (kernel selection inside csrc/) are looked up per launch and follow the table at once.
 * value = NULL removes the override.  No reference counterpart (the reference has no native code to switch). */
int qtts_set_option(const char* name, const char* value);
/* -> the current value ("" + return 1 when the switch is unset), copied into buf (cap bytes incl. the terminator). */
int qtts_get_option(const char* name, char* buf, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * Codec decoder: Qwen3-TTS-Tokenizer-12Hz  codes -> 24 kHz waveform.
 * Replaces Qwen3TTSTokenizerV2Model.decode / Qwen3TTSTokenizerV2Decoder.{forward,chunked_decode}
 * (qwen_tts/core/tokenizer_12hz/modeling_qwen3_tts_tokenizer_v2.py:993-1024, 869-896).
 * ------------------------------------------------------------------------------------------ */
typedef struct qtts_codec qtts_codec;

typedef struct {
    /* fields of Qwen3TTSTokenizerV2DecoderConfig (configuration_qwen3_tts_tokenizer_v2.py:72-93) */
    int32_t codebook_size;
    int32_t codebook_dim;
    int32_t hidden_size;
    int32_t latent_dim;
    int32_t num_attention_heads;
    int32_t num_key_value_heads;
    int32_t head_dim;
    int32_t sliding_window;
    int32_t intermediate_size;
    int32_t num_hidden_layers;
    int32_t num_quantizers;
    int32_t n_upsample_rates;
    int32_t upsample_rates[8];
    int32_t n_upsampling_ratios;
    int32_t upsampling_ratios[8];
    int32_t decoder_dim;
    float rms_norm_eps;
    float rope_theta;
    /* engine options */
    int32_t compute_dtype; /* QTTS_F32 | QTTS_BF16 */
    int32_t max_batch;     /* largest B of one decode call                     */
    int32_t max_frames;    /* largest frames per *chunk* (reference: 300 + 25) */
} qtts_codec_config;

int qtts_codec_create(const qtts_codec_config* cfg, qtts_codec** out);
void qtts_codec_destroy(qtts_codec* c);

/* Bind one parameter.  `name` is the reference state_dict key relative to `decoder.`
 * (e.g. "quantizer.rvq_first.vq.layers.0._codebook.embedding_sum", "decoder.1.block.1.conv.weight").
 * `host` points to HOST memory, row-major, `src_dtype` QTTS_F32 or QTTS_BF16.  The data is
 * copied/repacked before the call returns. */
int qtts_codec_bind(qtts_codec* c, const char* name, const void* host, int32_t src_dtype,
                    int32_t ndim, const int64_t* shape);
/* Verify every parameter is bound, precompute derived tables (normalised codebooks V2:677,
 * exp(alpha), 1/(exp(beta)+1e-9) V2:608-613) and allocate workspaces. */
int qtts_codec_finalize(qtts_codec* c);

/* One un-chunked Qwen3TTSTokenizerV2Decoder.forward (V2:869-884).
 * codes_dev: int64 (B, Q, T) device, values in [0, codebook_size).
 * wav_dev:   float (B, T*total_upsample) device.
 * pre_clamp_dev: optional float (B, T*total_upsample) device, the tensor before clamp(-1,1). */
int qtts_codec_forward(qtts_codec* c, const int64_t* codes_dev, int32_t B, int32_t T, float* wav_dev,
                       float* pre_clamp_dev, void* stream);

/* Qwen3TTSTokenizerV2Model.decode (V2:993-1024): codes_dev int64 (B, T, Q) device padded with -1,
 * clamp(min=0), chunked_decode(chunk_size, left_context) (V2:886-896; reference defaults 300, 25),
 * wav_dev float (B, T*total_upsample) device.  lengths_host (B) receives
 * (#frames with code > -1) * total_upsample -- the caller trims, as V2:1017 does. */
int qtts_codec_decode(qtts_codec* c, const int64_t* codes_dev, int32_t B, int32_t T, int32_t chunk_size,
                      int32_t left_context, float* wav_dev, int64_t* lengths_host, void* stream);

/* Streaming (state-carrying) decode -- SURVEY.md 8(f2).  The decoder is causal end to end
 * (Qwen3TTSTokenizerV2CausalConvNet / CausalTransConvNet, tokenizer v2:159-208; sliding-window transformer :491), so
 * packets of new frames can be decoded one after the other while the handle carries, per stateful layer, the last
 * (k-1)*dilation input rows (one row per k = 2r transposed conv, window-1 rotated q|k|v rows per transformer layer).
 * The concatenated packets equal Qwen3TTSTokenizerV2Decoder.forward (:869-884) on the whole sequence -- without
 * chunked_decode's (:886-896) re-decode of 25 context frames; algorithm in oracle/codec_stream_ref.py.
 * One session per handle: `begin` zeroes the state for `batch` sequences that advance in lockstep; `push` decodes
 * codes_dev int64 (batch, num_quantizers, n_frames) into wav_dev float (batch, n_frames * total_upsample).
 * STATUS: validated on MI355X (round 2): any packetisation == `forward` on the whole sequence
 * (tests/test_gpu_parity.py::test_codec_incremental_stream_equals_forward). */
/* Bookkeeping of the decode-call graph cache (round 4): `qtts_codec_forward` / `qtts_codec_decode` replay a captured hipGraph from
 * the second call with the same shape (B, T, chunking) on, staging codes and waveform in engine-owned buffers -- the reference's decode is a Python loop of
 * eager PyTorch ops (tokenizer v2:869-896); there is nothing to mirror, this only reports what happened. */
typedef struct qtts_codec_stats {
    int32_t graph_captures;  /* decode shapes captured so far                                   */
    int32_t graph_replays;   /* calls served by hipGraphLaunch                                  */
    int32_t graphs_cached;   /* captured graphs alive (LRU of 8)                                */
    int32_t graph_nodes_last; /* nodes of the most recently REPLAYED graph (0: nothing replayed yet)      */
} qtts_codec_stats;
int qtts_codec_get_stats(qtts_codec* c, qtts_codec_stats* out);

int qtts_codec_stream_begin(qtts_codec* c, int32_t batch);
int qtts_codec_stream_push(qtts_codec* c, const int64_t* codes_dev, int32_t n_frames, float* wav_dev, void* stream);
/* Per-slot form of the streaming decode.  After qtts_codec_stream_begin(c, B) the handle owns B SLOTS (rows 0..B-1), each with its own
 * conv / KV carries and its own position; qtts_codec_stream_push is the push of all B slots in order.
 *   reset_rows: a new sequence starts in each listed slot -- its carries are zeroed by a kernel on `stream` (ordered with the pushes
 *     before and after it on that stream; no hipMemset, no null stream, no device-wide synchronisation -- the small
 *     host-to-device copy of the ids may still hold the host until the stream has taken it), its position returns to 0.  The other slots are untouched.
 *   push_rows: the next n_frames frames of the n_rows listed slots, in the order listed: codes_dev int64 (n_rows, num_quantizers,
 *     n_frames) -> wav_dev float (n_rows, n_frames * total_upsample).  Slots not listed do not advance.  Each listed slot continues at
 *     its own position (RoPE, attention-window padding), so slots admitted at different times decode side by side and every slot's
 *     concatenated packets equal `forward` on its whole sequence.
 * Refusals, all raised before anything is launched (a refused call changes no slot): QTTS_ERR_STATE before stream_begin;
 * QTTS_ERR_ARG for n_rows < 1, a row id outside [0, B) or listed twice (the message names the id); QTTS_ERR_LIMIT when the packet plus
 * the carried rows of n_rows sequences exceed the workspace (the rule of stream_push with n_rows in place of B). */
int qtts_codec_stream_reset_rows(qtts_codec* c, int32_t n_rows, const int32_t* row_ids_host, void* stream);
int qtts_codec_stream_push_rows(qtts_codec* c, int32_t n_rows, const int32_t* row_ids_host, const int64_t* codes_dev, int32_t n_frames,
                                float* wav_dev, void* stream);
/* Priming: sequences START in the listed slots with frames in front of them that are decoded but never heard -- a voice-clone reference,
 * which the reference implementation decodes as cat([ref_code, codes]) and cuts off the waveform (qwen3_tts_model.py:612-631).
 *   prime_rows: slot row_ids_host[m] is left exactly where qtts_codec_stream_reset_rows followed by a qtts_codec_stream_push_rows of its
 *     own n_frames_host[m] frames would leave it (every conv carry, the roped q|k|v rows of every transformer layer, the position
 *     = n_frames_host[m]); the reset is implied, no PCM is written and no final conv is launched.  codes_dev int64 (n_rows, num_quantizers,
 *     n_max); row m's frames are the LAST n_frames_host[m] columns of its block (right-aligned), each in [1, n_max]; the leading columns
 *     are never read.  Slots not listed are untouched.  All rows are primed by one set of launches whatever their lengths (the padding is
 *     masked in the attention, skipped by the RoPE positions and written as zeros in front of every stateful layer), and only the last
 *     qtts_codec_stream_prime_tail frames go through the upsampling stack: behind the transformer every layer has a finite reach, so
 *     the carries depend on no earlier frame.  Switch QTTS_CODEC_PRIME_TAIL=0 (qtts_set_option): all n_max frames go through (A/B).
 *   prime_tail: that number of frames, derived from the upsampling rates (10 for the released rates (2, 2) and (8, 5, 4, 3)).
 * Refusals as for the per-slot calls above, before anything is launched (a refused call changes no slot); QTTS_ERR_ARG also for an
 * n_frames_host[m] outside [1, n_max] (the message names the row); QTTS_ERR_LIMIT by the workspace rule, with n_max frames per row in
 * the transformer and the tail behind it. */
int qtts_codec_stream_prime_rows(qtts_codec* c, int32_t n_rows, const int32_t* row_ids_host, const int64_t* codes_dev,
                                 const int32_t* n_frames_host, int32_t n_max, void* stream);
int qtts_codec_stream_prime_tail(qtts_codec* c, int32_t* tail_frames_host);

/* Test/diagnostic hook: run Qwen3TTSTokenizerV2Decoder.forward on codes_dev (B, Q, T) up to and including
 * `stage` and copy that stage's activation, channel-last float (B, L, C), to out_dev (capacity `cap` floats).
 * Stage names: "rvq","pre_conv","pre_transformer","upsample0","upsample1","decoder0","block1".."block4". */
int qtts_codec_forward_stage(qtts_codec* c, const int64_t* codes_dev, int32_t B, int32_t T, const char* stage,
                             float* out_dev, int64_t cap, int64_t* L, int64_t* C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Codec ENCODER: 24 kHz waveform -> Qwen3-TTS-Tokenizer-12Hz codes -- SURVEY.md 8(f3).
 * Replaces Qwen3TTSTokenizerV2Model.encode (tokenizer v2:961-991), i.e. transformers.MimiModel.encode behind
 * Qwen3TTSTokenizerV2Encoder (v2:897-908): SEANet encoder -> causal transformer -> stride-2 downsample -> split
 * residual VQ; only the first `valid_num_quantizers` codebooks are produced (v2:982-983).
 * STATUS: validated on MI355X (round 2): codes bit-identical to the reference's own encoder class on the golden waveforms.
 * ------------------------------------------------------------------------------------------ */
typedef struct qtts_encoder qtts_encoder;

typedef struct {
    /* encoder-side fields of transformers.MimiConfig as the reference instantiates it */
    int32_t hidden_size;
    int32_t num_filters;
    int32_t num_residual_layers;
    int32_t n_ratios;
    int32_t ratios[8];              /* MimiConfig.upsampling_ratios (the encoder applies them reversed) */
    int32_t kernel_size;
    int32_t last_kernel_size;
    int32_t residual_kernel_size;
    int32_t dilation_growth_rate;
    int32_t compress;
    int32_t codebook_size;
    int32_t codebook_dim;
    int32_t num_quantizers;
    int32_t num_semantic_quantizers;
    int32_t valid_num_quantizers;   /* Qwen3TTSTokenizerV2Config.encoder_valid_num_quantizers (16) */
    int32_t num_hidden_layers;
    int32_t intermediate_size;
    int32_t num_attention_heads;
    int32_t num_key_value_heads;
    int32_t head_dim;
    int32_t sliding_window;
    float rope_theta;
    float norm_eps;
    /* engine options */
    int32_t compute_dtype;          /* QTTS_F32 | QTTS_BF16 (the quantiser always runs in fp32) */
    int32_t max_batch;
    int32_t max_samples;            /* longest waveform of one encode call */
} qtts_encoder_config;

int qtts_encoder_create(const qtts_encoder_config* cfg, qtts_encoder** out);
void qtts_encoder_destroy(qtts_encoder* e);
/* `name` = reference state_dict key relative to `encoder.` (e.g. "encoder.layers.0.conv.weight",
 * "quantizer.acoustic_residual_vector_quantizer.layers.3.codebook.embed_sum").  Host pointer, row-major. */
int qtts_encoder_bind(qtts_encoder* e, const char* name, const void* host, int32_t src_dtype, int32_t ndim,
                      const int64_t* shape);
int qtts_encoder_finalize(qtts_encoder* e);
/* frames produced for a waveform of `samples` samples (MimiModel.get_encoded_length) */
int qtts_encoder_frames(qtts_encoder* e, int64_t samples, int64_t* frames);
/* wav_dev float (B, samples) device, zero-padded rows; codes_dev int64 (B, valid_num_quantizers, frames) device.
 * The caller trims each row to ceil(valid_samples / encode_downsample_rate) frames and transposes, as v2:984-985. */
int qtts_encoder_encode(qtts_encoder* e, const float* wav_dev, int32_t B, int32_t samples, int64_t* codes_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Speaker embedding of the Base (voice-clone) model -- SURVEY.md 8(f4).
 * Replaces Qwen3TTSForConditionalGeneration.extract_speaker_embedding (modeling_qwen3_tts.py:1941-1954):
 * mel_spectrogram (:402-464; n_fft 1024, hop 256, 128 mels, 0..12 kHz, center=False) -> Qwen3TTSSpeakerEncoder
 * (ECAPA-TDNN, :95-393).
 * STATUS: validated on MI355X (round 2) against the oracle (log-mel and embedding); the Slaney filterbank restates
 * librosa.filters.mel, which is absent here: filterbank parity unpinned.
 * ------------------------------------------------------------------------------------------ */
typedef struct qtts_speaker qtts_speaker;

typedef struct {
    /* Qwen3TTSSpeakerEncoderConfig (configuration_qwen3_tts.py:22-67) */
    int32_t mel_dim;
    int32_t enc_dim;
    int32_t n_blocks;               /* len(enc_channels) */
    int32_t channels[8];
    int32_t kernel_sizes[8];
    int32_t dilations[8];
    int32_t attention_channels;
    int32_t res2net_scale;
    int32_t se_channels;
    /* mel front end (the constants of modeling_qwen3_tts.py:1944-1952) */
    int32_t n_fft;
    int32_t hop_size;
    int32_t win_size;
    int32_t num_mels;
    /* engine options */
    int32_t compute_dtype;          /* QTTS_F32 | QTTS_BF16 (the STFT and mel projection always run in fp32) */
    int32_t max_batch;
    int32_t max_samples;
} qtts_speaker_config;

int qtts_speaker_create(const qtts_speaker_config* cfg, qtts_speaker** out);
void qtts_speaker_destroy(qtts_speaker* s);
/* `name` = reference state_dict key relative to `speaker_encoder.` (e.g. "blocks.1.res2net_block.blocks.0.conv.weight"),
 * plus "mel_basis" float (num_mels, n_fft/2+1): the Slaney filterbank the reference takes from librosa.filters.mel. */
int qtts_speaker_bind(qtts_speaker* s, const char* name, const void* host, int32_t src_dtype, int32_t ndim,
                      const int64_t* shape);
int qtts_speaker_finalize(qtts_speaker* s);
int qtts_speaker_mel_frames(qtts_speaker* s, int64_t samples, int64_t* frames);
/* wav_dev float (B, samples) device, 24 kHz, in [-1, 1]; emb_dev float (B, enc_dim); mels_dev optional float
 * (B, mel_frames, mel_dim) (the log-mel features, for tests). */
int qtts_speaker_embed(qtts_speaker* s, const float* wav_dev, int32_t B, int32_t samples, float* emb_dev, float* mels_dev,
                       void* stream);
/* qtts_speaker_embed for B clips of DIFFERENT lengths in one launch sequence.  Packed layout, nothing padded to the longest clip:
 * wav_dev float device holds clip b's samples_host[b] samples at offset sum(samples_host[0..b)); samples_host int32 (B) is HOST memory,
 * read before the call returns.  emb_dev float (B, enc_dim): row b is what qtts_speaker_embed gives for clip b alone (same arithmetic,
 * stage for stage; reflect paddings, time means / deviations and the attention softmax run over the clip's own frames).  mels_dev
 * optional float (sum_b mel_frames(samples_host[b]), mel_dim): the clips' log-mel frames one after the other.
 * Refused before anything is launched or written, the message naming the clip: B outside 1..max_batch or a samples_host[b] outside
 * 1..max_samples (QTTS_ERR_LIMIT); a clip shorter than one STFT window, or with no more mel frames than the widest reflect padding of
 * the configured TDNN layers (QTTS_ERR_ARG) -- with the released kernel sizes and dilations the shortest clip is 1280 samples
 * (5 frames), as in the reference. */
int qtts_speaker_embed_ragged(qtts_speaker* s, const float* wav_dev, int32_t B, const int32_t* samples_host, float* emb_dev,
                              float* mels_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Talker + code predictor: the autoregressive speech-token decoder.
 * Replaces `self.talker.generate(inputs_embeds, attention_mask, trailing_text_hidden,
 * tts_pad_embed, **talker_kwargs)` (modeling_qwen3_tts.py:2272-2278) = HF GenerationMixin._sample
 * around Qwen3TTSTalkerForConditionalGeneration.forward (modeling_qwen3_tts.py:1636-1744) and its
 * nested code_predictor.generate (modeling_qwen3_tts.py:1671-1680, 1250-1312).
 * ------------------------------------------------------------------------------------------ */
typedef struct qtts_talker qtts_talker;

/* Supported head shapes, for the talker and the code predictor independently: head_dim 64 or 128, num_attention_heads a multiple of
 * num_key_value_heads with a GQA group (heads / kv heads) of 1..8.  head_dim 128 with a group <= 2 (the released checkpoints) runs the
 * specialised decode attentions and the code predictor's fused launches; every other shape the general decode attention
 * (qtts_talker_stats.attn_gq_per_step).  Anything else is refused by finalize with QTTS_ERR_ARG. */
typedef struct {
    /* Qwen3TTSTalkerConfig (configuration_qwen3_tts.py:370-454) */
    int32_t vocab_size;
    int32_t hidden_size;
    int32_t intermediate_size;
    int32_t num_hidden_layers;
    int32_t num_attention_heads;
    int32_t num_key_value_heads;
    int32_t head_dim;
    float rms_norm_eps;
    float rope_theta;
    int32_t num_code_groups;
    int32_t text_hidden_size;
    int32_t codec_eos_token_id;
    /* Qwen3TTSTalkerCodePredictorConfig (configuration_qwen3_tts.py:189-258) */
    int32_t cp_vocab_size;
    int32_t cp_hidden_size;
    int32_t cp_intermediate_size;
    int32_t cp_num_hidden_layers;
    int32_t cp_num_attention_heads;
    int32_t cp_num_key_value_heads;
    int32_t cp_head_dim;
    float cp_rms_norm_eps;
    float cp_rope_theta;
    /* engine options */
    int32_t weight_dtype; /* QTTS_F32 | QTTS_BF16 (weights and KV cache)            */
    /* max_batch: sequences per generate call, 1..64 (QTTS_ERR_LIMIT outside).  A call may bring any smaller batch; the frame step's
       launches follow the batch of the call.  The KV pools are reserved for max_batch x max_seq at finalize: at max_batch 64, max_seq
       4096, 1.7B dims (28 layers x 8 kv heads x 128) in bf16 that is 64 x 4096 x 28 x 2 x 8 x 128 x 2 B = 30.1 GB for the talker (plus
       42 MB for the code predictor) -- max_seq is one lever: 1024 keeps it at 7.5 GB.  The other is a shared page pool
       (qtts_talker_set_kv_pool below): the talker cache then holds n_pages pages of 16 keys (1.835 MB each at these dims; the 30.1 GB
       are 16 384 pages) that the rows take as they grow, and max_seq only bounds one request.  Decode scratch above 32 rows grows by the code
       predictor's two-token first pass only (2 x max_batch rows).  QTTS_SKINNY_WIDE=0 (qtts_set_option; A/B runs) sends that pass's
       65..128-row GEMMs out as two launches of <= 64 rows instead of one. */
    int32_t max_batch;
    int32_t max_seq;      /* prompt + generated frames per sequence (KV pages reserved) */
    int32_t use_graph;    /* 1: replay the frame step as a hipGraph; 0: eager launches  */
} qtts_talker_config;

/* HF sampling knobs (generation defaults: qwen_tts/inference/qwen3_tts_model.py:319-352). */
typedef struct {
    int32_t do_sample;
    int32_t top_k;   /* 0 = off */
    float top_p;     /* 1.0 = off */
    float temperature;
    float repetition_penalty;
    int32_t subtalker_dosample;
    int32_t subtalker_top_k;
    float subtalker_top_p;
    float subtalker_temperature;
    uint64_t seed;   /* Philox key; torch's global-RNG stream cannot be reproduced across devices */
} qtts_sampling;

/* The same knobs for ONE request of a batch, plus the request's own length limits (qtts_talker_generate_rows, ABI v14).  The reference
 * resolves these per call (user value > generate_config.json > hard default, qwen_tts/inference/qwen3_tts_model.py:287-352) and hands
 * one set to the whole batch; a service that batches requests of different callers needs them per request.
 *   seed            Philox key of THIS request: its draws are a function of (seed, step, codebook) and not of the row it occupies or
 *                   of the requests it is batched with.  Two rows with the SAME seed therefore draw the same numbers: give every
 *                   request its own (the Python layer does when the caller passes one seed or none).
 *   max_new_tokens  the request's own limit (>= 1).  A row that reaches it is treated like a row that hit EOS: it yields
 *                   max_new_tokens - 1 frames -- what a scalar call with that limit yields -- and receives eos from token index
 *                   max_new_tokens - 1 on (the one visible difference from a scalar run, whose last token is the sampled one).
 *   min_new_tokens  EOS is blocked for this request until it has that many tokens. */
typedef struct qtts_row_sampling {
    int32_t do_sample;
    int32_t top_k;   /* 0 = off */
    float top_p;     /* 1.0 = off; (0, 1] on a sampling row */
    float temperature;
    float repetition_penalty;
    int32_t subtalker_dosample;
    int32_t subtalker_top_k;
    float subtalker_top_p;
    float subtalker_temperature;
    int32_t max_new_tokens;
    int32_t min_new_tokens;
    int32_t reserved;
    uint64_t seed;
} qtts_row_sampling;

int qtts_talker_create(const qtts_talker_config* cfg, qtts_talker** out);
void qtts_talker_destroy(qtts_talker* t);
/* `name` = reference state_dict key relative to `talker.` (e.g. "model.layers.0.self_attn.q_proj.weight",
 * "code_predictor.lm_head.3.weight").  Host pointer, row-major. */
int qtts_talker_bind(qtts_talker* t, const char* name, const void* host, int32_t src_dtype, int32_t ndim,
                     const int64_t* shape);
int qtts_talker_finalize(qtts_talker* t);

/* y = text_projection(x): Qwen3TTSTalkerResizeMLP (modeling_qwen3_tts.py:808-816,1575-1577), used by
 * the prompt assembly (modeling_qwen3_tts.py:2076-2232).  x_dev float (rows, text_hidden) device,
 * y_dev float (rows, hidden) device. */
int qtts_talker_text_projection(qtts_talker* t, const float* x_dev, int32_t rows, float* y_dev, void* stream);

/* Prompt assembly on device (Qwen3TTSForConditionalGeneration.generate, modeling_qwen3_tts.py:2076-2269, and
 * generate_icl_prompt, :1968-2019).  The host resolves WHICH rows make up each prompt (integers only); the device
 * does every gather, projection and sum.
 *
 * qtts_talker_text_embed: y[r] = text_projection(text_embedding[ids[r]]) (:2076-2080, 2177, 2207, 2229) --
 *   ids_dev int64 (rows) device, y_dev float (rows, hidden) device.  Needs "model.text_embedding.weight" and the
 *   text_projection weights bound.  An id outside the table is QTTS_ERR_ARG.
 * qtts_talker_assemble_rows: out[r] = T + C with, from desc_dev int32 (rows, 4) = {text_row, codec_id, spk_row,
 *   ref_frame} (-1 = absent; all four absent = a zero row, i.e. left padding :2251-2254):
 *     T = proj[text_row]                               (proj_dev float (proj_rows, hidden): text_embed output)
 *     C = codec_embedding[codec_id]                    (:2142-2172 codec prefix / pad / bos, speaker ids :2092)
 *       | spk[spk_row]                                 (spk_dev float (n_spk, hidden): voice-clone x-vectors :1957-1966)
 *       | codec_embedding[ref[f][0]] + sum_g cp_embedding[g-1][ref[f][g]]   (ref_codes_dev int64 (n_ref_frames, G):
 *                                                        in-context reference codes :1983-1990)
 *   out_dev float (rows, hidden).  Indices out of range are QTTS_ERR_ARG. */
int qtts_talker_text_embed(qtts_talker* t, const int64_t* ids_dev, int32_t rows, float* y_dev, void* stream);
int qtts_talker_assemble_rows(qtts_talker* t, const int32_t* desc_dev, int32_t rows, const float* proj_dev, int32_t proj_rows,
                              const float* spk_dev, int32_t n_spk, const int64_t* ref_codes_dev, int32_t n_ref_frames,
                              float* out_dev, void* stream);

/* Prefill (modeling_qwen3_tts.py:1665-1667, 1693-1727): embeds_dev float (B, T, H) LEFT-padded,
 * n_pad_host (B) = number of left pads per row (attention_mask = [0]*n_pad + [1]*(T-n_pad),
 * modeling_qwen3_tts.py:2251-2254), trailing_dev float (B, Tt, H) right-padded with tts_pad
 * (modeling_qwen3_tts.py:2255-2269), tts_pad_dev float (H).  Fills the KV cache and leaves the
 * first-step logits / past_hidden on device. */
int qtts_talker_prefill(qtts_talker* t, const float* embeds_dev, int32_t B, int32_t T, const int32_t* n_pad_host,
                        const float* trailing_dev, int32_t Tt, const float* tts_pad_dev, void* stream);

/* The sampling loop after prefill, with HF `_sample` semantics:
 *   processors RepetitionPenalty -> MinNewTokensLength(min_new_tokens, eos) -> SuppressTokens ->
 *   [Temperature -> TopK -> TopP], finished rows keep receiving eos, stop when every row hit eos or
 *   max_new_tokens tokens were drawn.
 * suppress_host: list of suppressed token ids (modeling_qwen3_tts.py:2059-2063), n_suppress entries.
 * codes_dev:  int64 (B, max_new_tokens-1, num_code_groups) device, row-major; frame f of row b holds
 *             [cb0, 15 sub-codes] (modeling_qwen3_tts.py:1681); frames >= *n_frames_host are undefined.
 * hidden_dev: optional float (B, max_new_tokens-1, H): `past_hidden` per frame (modeling_qwen3_tts.py:2281).
 * tokens_dev: optional int64 (B, max_new_tokens): every sampled cb0 token incl. the final one.
 * n_frames_host: number of complete frames (= HF steps - 1, modeling_qwen3_tts.py:2280).
 * Synchronises the stream before returning. */
int qtts_talker_generate(qtts_talker* t, const qtts_sampling* sp, int32_t max_new_tokens, int32_t min_new_tokens,
                         int32_t eos_token_id, const int32_t* suppress_host, int32_t n_suppress,
                         int64_t* codes_dev, float* hidden_dev, int64_t* tokens_dev, int32_t* n_frames_host,
                         void* stream);

/* qtts_talker_generate with per-request settings (ABI v14; knobs as qwen_tts/inference/qwen3_tts_model.py:287-352 resolves them, here
 * one set per row): rows_host[b] holds row b's knobs, seed and limits; n_rows must equal the prefilled batch.  The settings live in a
 * device table the samplers read, so they are NOT part of the captured frame graph: calls that differ only in the table's values
 * replay the same graph (qtts_talker_stats.graph_captures does not advance).  Buffers are sized by the LARGEST max_new_tokens of the
 * table (codes_dev (B, max-1, G), hidden_dev (B, max-1, H), tokens_dev (B, max)); *n_frames_host is the call's frame count: the
 * generation stops when every row hit EOS or its own limit.  Row b's frames end before its first eos in codebook 0 (as
 * modeling_qwen3_tts.py:2283-2289 trims them).  Refused: n_rows != B, top_p outside (0, 1] on a sampling row, temperature <= 0,
 * max_new_tokens < 1 (QTTS_ERR_ARG, the message names the row); prompt + the largest limit beyond max_seq (QTTS_ERR_LIMIT); teacher
 * forcing or profile mode 2 together with a table (QTTS_ERR_ARG). */
int qtts_talker_generate_rows(qtts_talker* t, const qtts_row_sampling* rows_host, int32_t n_rows, int32_t eos_token_id,
                              const int32_t* suppress_host, int32_t n_suppress, int64_t* codes_dev, float* hidden_dev,
                              int64_t* tokens_dev, int32_t* n_frames_host, void* stream);

/* Resumable generation -- qtts_talker_generate in three calls, for streaming OUTPUT (BASELINE config 4; the reference
 * only "simulates streaming text input", qwen3_tts_model.py:513-515, and returns whole utterances):
 *   stream_begin  after qtts_talker_prefill: same arguments as qtts_talker_generate minus the outputs that only exist at
 *                 the end; samples the first token.  codes_dev int64 (B, max_new_tokens-1, G) / hidden_dev (optional)
 *                 are filled progressively.
 *   stream_step   runs up to max_frames_now more frame steps (the same captured frame graph and device-resident loop
 *                 state as qtts_talker_generate) and returns, on the host, how many frames are final so far
 *                 (codes_dev[:, :frames_total]) and whether the stop condition has latched.
 *   stream_end    the closing bookkeeping: tokens_dev int64 (B, max_new_tokens) padded with -1 (optional) and the frame
 *                 count, as qtts_talker_generate reports them.  May be called early to abandon a request.
 * STATUS: validated on MI355X (round 2), eager and hipGraph: packets == one-shot generate. */
int qtts_talker_stream_begin(qtts_talker* t, const qtts_sampling* sp, int32_t max_new_tokens, int32_t min_new_tokens,
                             int32_t eos_token_id, const int32_t* suppress_host, int32_t n_suppress, int64_t* codes_dev,
                             float* hidden_dev, void* stream);
/* stream_begin with per-request settings (see qtts_talker_generate_rows); stream_step / stream_end are the same calls. */
int qtts_talker_stream_begin_rows(qtts_talker* t, const qtts_row_sampling* rows_host, int32_t n_rows, int32_t eos_token_id,
                                  const int32_t* suppress_host, int32_t n_suppress, int64_t* codes_dev, float* hidden_dev, void* stream);
int qtts_talker_stream_step(qtts_talker* t, int32_t max_frames_now, int32_t* frames_total_host, int32_t* finished_host,
                            void* stream);
int qtts_talker_stream_end(qtts_talker* t, int64_t* tokens_dev, int32_t* n_frames_host, void* stream);

/* Admission of queued requests into finished rows of a running stream (ABI v15; no reference counterpart: the reference hands one static
 * batch to HF generate, modeling_qwen3_tts.py:2272-2278 -- each request's result is still what the reference produces for that request).
 * A stream has ONE position, kv_len: the slot the next frame step writes in every row.  A request with a prompt of T_new rows is admitted
 * into a finished row by writing its prompt's K/V into slots [kv_len - T_new, kv_len) of that row; from then on the row looks like a
 * request that was left-padded that far, and everything that counts per request -- token history, min_new_tokens, the row's limit, the
 * trailing-text index, the frame index of its outputs, the Philox step -- counts from the row's own origin.  A request's draws are a
 * function of (its seed, its own step, codebook) whenever it was admitted.
 *   stream_begin_admitting  qtts_talker_stream_begin_rows plus max_row_tokens: codes_dev (B, max_row_tokens - 1, G), hidden_dev
 *                 (B, max_row_tokens - 1, H; optional) and the token history hold ONE occupant per row at a time; frame f of a row's
 *                 occupant is codes_dev[row][f].  The stream's stop condition is "no row unfinished"; how far it can run is bounded by
 *                 max_seq, which is checked per admission.  Refused like stream_begin_rows, and (QTTS_ERR_LIMIT, naming the row) when a
 *                 row's max_new_tokens exceeds max_row_tokens.
 *   stream_admit  between two stream_step calls, on the same stream: rows_host[i] is the finished row request i takes; embeds_dev
 *                 (n_new, T, H) LEFT-padded inside T with n_pad_host[i] pads (T: the longest prompt of the group); trailing_dev
 *                 (n_new, Tt, H), padded by the engine with tts_pad to the stream's trailing capacity; settings_host[i] the request's
 *                 knobs.  Samples token 0 of the admitted rows only; the stream's counters do not move, the other rows' state is not
 *                 touched, and the captured frame graphs are replayed unchanged (graph_captures does not advance; the one exception is an
 *                 occupant outside the fast samplers' class entering a stream that ran inside it).  Refused, the message naming the row:
 *                 no admitting stream open (QTTS_ERR_STATE); a row index >= B, listed twice, or still unfinished (QTTS_ERR_ARG); a prompt
 *                 longer than kv_len, kv_len + max_new_tokens beyond max_seq, max_new_tokens > max_row_tokens, Tt beyond the stream's
 *                 trailing capacity (QTTS_ERR_LIMIT); the settings checks of qtts_talker_generate_rows (QTTS_ERR_ARG).  A refused call
 *                 changes nothing.  The caller copies a finished row's frames out BEFORE admitting into it.
 *   stream_rows   per row: whether its occupant is still running and how many of its frames are final (they end before its first eos in
 *                 codebook 0); and the shared position.  Synchronises the stream the stream was begun on.
 * stream_step / stream_end are the same calls; for an admitting stream frames_total / n_frames count the STREAM's frame steps and
 * tokens_dev is (B, max_row_tokens), each row's current occupant. */
int qtts_talker_stream_begin_admitting(qtts_talker* t, const qtts_row_sampling* rows_host, int32_t n_rows, int32_t max_row_tokens,
                                       int32_t eos_token_id, const int32_t* suppress_host, int32_t n_suppress, int64_t* codes_dev,
                                       float* hidden_dev, void* stream);
int qtts_talker_stream_admit(qtts_talker* t, int32_t n_new, const int32_t* rows_host, const float* embeds_dev, int32_t T,
                             const int32_t* n_pad_host, const float* trailing_dev, int32_t Tt, const qtts_row_sampling* settings_host,
                             void* stream);
int qtts_talker_stream_rows(qtts_talker* t, int32_t* unfinished_host, int32_t* frames_host, int32_t* kv_len_host);

/* Per-row KV positions: an admitting stream that never has to drain.  qtts_talker_stream_begin_admitting_rows takes the arguments of
 * qtts_talker_stream_begin_admitting and opens a stream whose rows each carry their OWN KV length: an admitted request's prompt goes to
 * slots [0, T) of the row it takes (left-padded inside the group's T as before), the row's length restarts at T and grows by one per
 * frame step while its occupant is unfinished; a finished row's length is frozen until the row is re-occupied.  Nothing of a previous
 * occupant is read: its keys lie at or above the new length, or are overwritten.  The decode attention of row b walks row b's keys only,
 * and the split-KV span of a frame step is the bucket of the longest RUNNING row: it goes up when a long prompt is admitted and down
 * when a long row retires (one captured graph per bucket visited, cached).  The stream's stop condition is "no row unfinished" alone:
 * no step count and no position bounds it.
 *   stream_admit  on such a stream: the refusals tied to the stream's position are gone.  The one QTTS_ERR_LIMIT of its own is
 *                 T + max_new_tokens > max_seq for a row of the group (naming the row, before anything is launched; a refused call
 *                 changes no row).  Row not finished / listed twice / out of range, max_row_tokens, the trailing capacity and the
 *                 settings checks are refused as on a shared-position stream.
 *   stream_rows   kv_len_host reports the length of the longest row whose occupant is still running (0: none).
 *   stream_row_lens  lens_host[b] = row b's KV length (a finished row: the frozen one).  QTTS_ERR_STATE without such a stream open.
 *                 Synchronises the stream the stream was begun on.
 * Every other mode -- the shared-position stream, the scalar paths -- is bit for bit what it was. */
int qtts_talker_stream_begin_admitting_rows(qtts_talker* t, const qtts_row_sampling* rows_host, int32_t n_rows, int32_t max_row_tokens,
                                            int32_t eos_token_id, const int32_t* suppress_host, int32_t n_suppress, int64_t* codes_dev,
                                            float* hidden_dev, void* stream);
int qtts_talker_stream_row_lens(qtts_talker* t, int32_t* lens_host /* (B) */);
/* Whether the open or last stream carries per-row positions (0 | 1; any later generation call clears it), and the largest KV length a
 * row of it was seen at (0 without such a stream).  These are statistics, but qtts_talker_stats keeps its layout under ABI 15: they
 * have a call of their own. */
int qtts_talker_stream_mode(qtts_talker* t, int32_t* row_positions_host, int32_t* max_row_len_host);

/* Shared KV page pool for the talker cache (entry points added under ABI 15; no struct changed).
 *   set_kv_pool   between create and finalize (QTTS_ERR_STATE afterwards).  finalize then allocates n_pages + 1 pages of 16 keys for the
 *                 talker's K and V pools instead of max_batch x ceil(max_seq / 16); the extra page is a SINK.  n_pages = 0: the static
 *                 layout (the default).  0 < n_pages < ceil(max_seq / 16) is refused with QTTS_ERR_LIMIT: one request of max_seq keys
 *                 must always fit.  The code predictor's cache stays static.  The choice lives in the handle.
 *   Table invariant: every entry of the page table names a valid page at all times; an entry without a grant names the sink, which is
 *                 zero-filled at finalize.  Speculative loads beyond a row's length and the appends of a finished row at its frozen
 *                 length therefore land in memory nobody reads unmasked.  The allocator is a host-side free list in the engine (last
 *                 released, first granted: deterministic); the table lives in device memory and only the entries that changed are
 *                 patched, on the stream, between frame-graph launches (a grant captures no graph).
 *   Streams with per-row positions take pages as they grow: prefill and stream_admit grant a row ceil(T / 16) pages for the group's
 *                 padded T (stream_admit: QTTS_ERR_LIMIT when the group's prompt pages do not fit, nothing changed);
 *                 stream_step(max_frames_now) first makes sure every running row holds the pages of
 *                 len + min(max_frames_now, frames left under its limit) keys, and is refused with QTTS_ERR_LIMIT -- the message gives the
 *                 pages needed and the pages free -- when the pool cannot cover that: no row advanced, no page moved.  A row's pages
 *                 go back to the pool at the first stream_step / stream_rows return that observes it finished (copy frames out of
 *                 codes_dev, never out of the cache).
 *   Every other path reserves its worst case when it begins -- generate, generate_rows, stream_begin, stream_begin_rows:
 *                 B x ceil((T + max_new_tokens) / 16) pages; the shared-position admitting stream: whole rows -- and is refused with
 *                 QTTS_ERR_LIMIT (the prefill stays valid) when that does not fit.  Results on a pooled engine are the static engine's.
 *   stream_kv     pages_host[b] = pages row b holds (b < the batch of the last prefill), the free pages, the pool size.
 *                 QTTS_ERR_STATE on an engine without a pool.
 *   stream_evict  on a stream with per-row positions: the listed rows' occupants are abandoned -- the rows are marked finished on the
 *                 device, their lengths freeze where stream_row_lens reports them, their pages go back to the pool.  This is preemption
 *                 by restart (a request's codes depend on its seed and its own step only: admitted again it produces the same codes)
 *                 and the way to cancel a request; on an engine without a pool it frees nothing.  Rows listed twice or out of range:
 *                 QTTS_ERR_ARG, nothing changed. */
int qtts_talker_set_kv_pool(qtts_talker* t, int32_t n_pages);
int qtts_talker_stream_kv(qtts_talker* t, int32_t* pages_host /* (B) */, int32_t* free_host, int32_t* pool_host);
int qtts_talker_stream_evict(qtts_talker* t, int32_t n, const int32_t* rows_host);

/* The remaining HF sampling controls of the talker's codebook-0 sampler, per request (entry points added under ABI 15; no struct
 * changed): the four probability warpers HF generate applies after top-p -- min_p, typical_p, epsilon_cutoff, eta_cutoff -- and
 * no_repeat_ngram_size (transformers 4.57.3 generation/logits_process.py; the reference forwards them to generate(),
 * qwen_tts/inference/qwen3_tts_model.py:287-352).  The chain of a row's token is
 *   RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens ->
 *   [Temperature -> TopK -> TopP -> MinP -> Typical -> EpsilonCutoff -> EtaCutoff] -> argmax | softmax + draw;
 * a greedy row skips the bracket (as HF does) and keeps the n-gram ban.  The n-gram history is the row's own generated codebook-0
 * tokens (the prompt is embeds-only), counted from the row's origin like the repetition penalty's.  The code predictor's samplers take
 * none of these (modeling_qwen3_tts.py:1652-1677 hands them the four subtalker_* knobs only).
 *   set_row_warpers  one entry per row, 0 = off for every field.  ONE-SHOT: the table is consumed by the NEXT of generate_rows,
 *                 stream_begin_rows, stream_begin_admitting, stream_begin_admitting_rows or stream_admit, whose n_rows / n_new must equal
 *                 n_rows here -- otherwise that call fails with QTTS_ERR_ARG, nothing is changed and the table is dropped; so does a
 *                 scalar qtts_talker_generate / qtts_talker_stream_begin with a table pending.  NULL / 0 clears a pending table.  Values
 *                 are checked here, the message naming the row: min_p in [0, 1], typical_p in [0, 1] (1 is stored as off),
 *                 epsilon_cutoff / eta_cutoff in [0, 1), no_repeat_ngram_size >= 0; anything else is QTTS_ERR_ARG.  A consuming call
 *                 whose table has every field off is exactly the call without a table.  The entries live in a second device table
 *                 beside the rows' settings: their VALUES are not part of the captured frame graph.  Whether any row of the table has
 *                 any of them on IS (the talker's sampler is then another kernel): like the fast class it is monotone within a stream, so
 *                 the first such occupant admitted into a stream that ran without any re-captures the visited graphs once, later ones
 *                 do not.  A row admitted without a table gets an all-off entry.  Teacher forcing refuses the table call as before.
 *   sampler_class the sampler kernels of the open stream or the last call, talker / code predictor: 0 launch constants (a scalar
 *                 call), 1 sample_kernel_v2, 2 sample_kernel, 3 sample_warp_kernel (talker only).  A call of its own because
 *                 qtts_talker_stats keeps its layout under ABI 15. */
typedef struct qtts_row_warpers {      /* 32 bytes; 0 = off for every field */
    float min_p;
    float typical_p;
    float epsilon_cutoff;
    float eta_cutoff;
    int32_t no_repeat_ngram_size;
    int32_t reserved[3];
} qtts_row_warpers;
int qtts_talker_set_row_warpers(qtts_talker* t, const qtts_row_warpers* rows_host, int32_t n_rows);
int qtts_talker_sampler_class(qtts_talker* t, int32_t* talker_host, int32_t* subtalker_host);

/* The remaining HF logits processors of the talker's codebook-0 sampler, per request (a struct and an entry point added under ABI 15;
 * nothing existing changed): sequence_bias, bad_words_ids, forced_eos_token_id, exponential_decay_length_penalty and
 * begin_suppress_tokens (transformers generation/logits_process.py; min_length is folded into the row's min_new_tokens by the caller).
 * With them the chain of a row's token is, in `_get_logits_processor` order,
 *   SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinLength / MinNewTokensLength -> ForcedEOS ->
 *   ExponentialDecayLengthPenalty -> SuppressTokens -> SuppressTokensAtBegin ->
 *   [Temperature -> TopK -> TopP -> MinP -> Typical -> EpsilonCutoff -> EtaCutoff] -> argmax | softmax + draw.
 * cur_len is the row's own generated count, counted from the row's origin; EOS is the call's eos_token_id.
 *   records       n_words words holding n_records ragged records {kind, len, bias (float bits), tokens[len]}:
 *                 QTTS_PROC_KIND_BIAS   a single token is biased at every step; a longer sequence biases its LAST token when the row
 *                                       has generated at least len tokens and its last len - 1 equal the sequence's first len - 1.
 *                                       Biases that land on one token are summed in fp32 -- single-token records first, then the
 *                                       others in listed order, as HF does -- and the sum is added to the score;
 *                 QTTS_PROC_KIND_BAN    the same match, the token becomes -inf (behind the n-gram ban; `bias` is ignored);
 *                 QTTS_PROC_KIND_BEGIN  every listed token is -inf at the row's own step 0 only.
 *   flags         QTTS_PROC_DECAY: once cur_len > decay_start, x[eos] += |x[eos]| * (decay_factor ** (cur_len - decay_start) - 1) -- the
 *                 power in double ON THE DEVICE (one thread), the product and the sum in fp32, as HF evaluates them; an EOS score
 *                 that is already -inf stays -inf (HF: NaN).  QTTS_PROC_FORCED_EOS: at cur_len == limit - 1 every score becomes -inf and
 *                 EOS 0, where limit is the row's max_new_tokens as qtts_row_sampling holds it; it comes after the EOS floor, so it
 *                 wins over min_new_tokens.
 *   capacity      at most QTTS_PROC_MAX_RECORDS records and QTTS_PROC_MAX_TOKENS tokens per row; more is QTTS_ERR_LIMIT, the
 *                 message naming the row and the cap.  A kind, a length < 1, a token id outside [0, vocab), a non-finite
 *                 decay_factor or one <= 0, records that overrun n_words: QTTS_ERR_ARG, naming the row.
 *   set_row_processors  ONE-SHOT and consumed exactly like qtts_talker_set_row_warpers (above), by the same calls, with the same count
 *                 rule; a scalar qtts_talker_generate / qtts_talker_stream_begin with a table pending is refused and the table
 *                 dropped; NULL / 0 clears.  Both tables may be pending together.  The entries live in a third device table of fixed
 *                 capacity per row: their VALUES are not part of the captured frame graph.  A table with any control on makes the
 *                 talker's sampler sample_warp_kernel (class 3) -- the same monotone graph-key flag as the warpers', so the first such
 *                 occupant admitted into a stream that ran in another class re-captures once and values never do.  A row admitted
 *                 without a table gets an all-off entry; a table with everything off is exactly the call without it.  Teacher
 *                 forcing refuses the table call as before. */
#define QTTS_PROC_MAX_RECORDS 96
#define QTTS_PROC_MAX_TOKENS 512
#define QTTS_PROC_MAX_WORDS (3 * QTTS_PROC_MAX_RECORDS + QTTS_PROC_MAX_TOKENS)
#define QTTS_PROC_KIND_BIAS 1
#define QTTS_PROC_KIND_BAN 2
#define QTTS_PROC_KIND_BEGIN 3
#define QTTS_PROC_DECAY 1
#define QTTS_PROC_FORCED_EOS 2
typedef struct qtts_row_processors {   /* 32 + 4 x QTTS_PROC_MAX_WORDS bytes; all zero = everything off */
    double decay_factor;
    int32_t decay_start;
    int32_t flags;
    int32_t n_records;
    int32_t n_words;
    int32_t reserved[2];
    int32_t records[QTTS_PROC_MAX_WORDS];
} qtts_row_processors;
int qtts_talker_set_row_processors(qtts_talker* t, const qtts_row_processors* rows_host, int32_t n_rows);

/* Opt-in FP8 weights for the talker's decode GEMMs (entry points added under ABI 15; no struct changed).  The four Linear operators of
 * every TALKER layer (q|k|v, o, gate|up, down) are then stored as OCP e4m3fn codes with one power-of-two scale per output row --
 * half the bytes a frame step streams for them; the code predictor, codec_head, the embeddings and the text projection stay bf16.
 * The engine is defined without a tolerance: it is, bit for bit, the bf16 engine of another checkpoint W_eff, which
 * qtts_fp8_effective_rows returns operator by operator (load it into any implementation of the model to judge quality).
 *   quantizer     w'[n][k] = W[n][k] * g[k] in fp32 (g: the RMSNorm weight folded into the operator, NULL = 1); e[n] = the smallest integer
 *                 with 448 * 2^e >= max_k |w'[n][k]|, 0 for an all-zero row, clamped to [-100, 100]; code = RNE_e4m3fn(w' * 2^-e).  NaN
 *                 codes are never produced.  Under the clamp the construction's guarantees end: a row whose maximum exceeds 448 * 2^100
 *                 (5.7e32) has its larger values SATURATED to +-448 * 2^100, a row below 2^-9 * 2^-100 becomes zero, and a non-finite
 *                 weight is not supported.  The bitwise identity with the bf16 kernel on d further assumes that no product x * code
 *                 and no partial sum leaves fp32's normal range in either form (the two differ by the factor 2^e until the
 *                 epilogue); |e| <= 100 leaves 26 binades on either side, and trained weights sit near e = -12.  d[n][k] = code * 2^e is exactly a bf16 number, and the decode kernels convert the codes to
 *                 bf16 in registers and run the bf16 kernels' MFMA chains in the bf16 kernels' order: their output is the bf16 kernel's
 *                 on d.  The talker's row-major prefill operators are built from W_eff[n][k] = fl32(d[n][k] / g[k]) (W[n][k] where
 *                 g[k] == 0), so prompt and decode steps see one model.
 *   set_weight_format  between create and finalize, like qtts_talker_set_kv_pool.  QTTS_WEIGHTS_DEFAULT (0): the engine as it is;
 *                 QTTS_WEIGHTS_FP8 on a bf16 engine only (QTTS_ERR_ARG on an fp32 engine or an unknown value, QTTS_ERR_STATE after finalize).
 *   weight_format the format, and (after finalize) the bytes of all packed decode operators the engine holds on the device: an fp8
 *                 operator counts N * K + 4 N where its bf16 form counts 2 N K.  Either pointer may be NULL.
 *   The two fp8 calls are host-only (no device is touched).  codes: N x K bytes, exps: N. */
#define QTTS_WEIGHTS_DEFAULT 0
#define QTTS_WEIGHTS_FP8 1
int qtts_talker_set_weight_format(qtts_talker* t, int32_t fmt);
int qtts_talker_weight_format(qtts_talker* t, int32_t* fmt_host, int64_t* packed_bytes_host);
int qtts_fp8_quantize_rows(const float* W /* (N, K) */, const float* g_or_null /* (K) */, int32_t N, int32_t K, uint8_t* codes, int32_t* exps);
int qtts_fp8_effective_rows(const float* W /* (N, K) */, const float* g_or_null /* (K) */, int32_t N, int32_t K, float* W_eff);
/* Test hook: ONE launch of the decode GEMM on HOST operands (device memory is allocated, filled, and read back inside the call).
 *   out[M][No] = epilogue(rstd[m] * sum_k bf16(x[m][k]) * P[n][k]), P = the operator packed from W (x g when given) with `fs` features per
 *   strip, as bf16 (fmt 0) or as fp8 codes + scales (fmt QTTS_WEIGHTS_FP8).  W is given in PACKED row order (the caller interleaves
 *   gate / up rows for act 2 = SwiGLU strip pairs, 5 = SwiGLU of one strip).  No = N / 2 with a SwiGLU act, else N; out / res / out16
 *   have leading dimension ldo >= No (columns beyond No are never written); out16 (bf16 bits, NULL = none) is the kernel's bf16 shadow.
 *   last_decode_gemm_kernel: the kernel family that call ran on the calling thread: 2 skinny2_kernel, 4 skinny2_ks_kernel (split-K, batch
 *   17..32), 8 skinny8_kernel (the batch <= 8 form), + 16 for their fp8 forms, 0 any other.
 *   decode_gemm_ks: the same call with what the split-K form needs (plain GEMM: no norm, no act; 17 <= M <= 32 splits where the launcher
 *   has an instantiation and QTTS_SKINNY_KS / QTTS_SKINNY_KS_MINK allow, any other shape runs as in decode_gemm): an 8 MB granule
 *   workspace filled with 0xFF, the device word `serial` the tags derive from, and `launches` >= 1 back-to-back launches with slots
 *   3 + 7 l on that one workspace (each rewrites out).  out / out16 have M + 1 rows: row M is a guard the kernel must not write.
 *   QTTS_ERR_STATE if a reducer gave up (error or latch word raised). */
int qtts_debug_last_decode_gemm_kernel(int32_t* kind_host);
int qtts_debug_decode_gemm(const float* x /* (M, K) */, const float* W /* (N, K) */, const float* g_or_null, const float* bias_or_null /* (N) */,
                           const float* res_or_null /* (M, ldo) */, int32_t M, int32_t N, int32_t K, int32_t fs, int32_t norm, int32_t act,
                           int32_t fmt, int32_t ldo, float* out /* (M, ldo) in/out */, uint16_t* out16_or_null /* (M, ldo) in/out */);
int qtts_debug_decode_gemm_ks(const float* x /* (M, K) */, const float* W /* (N, K) */, const float* g_or_null, const float* bias_or_null /* (N) */,
                              const float* res_or_null /* (M, ldo) */, int32_t M, int32_t N, int32_t K, int32_t fs, int32_t fmt, int32_t ldo,
                              float* out /* (M + 1, ldo) in/out */, uint16_t* out16_or_null /* (M + 1, ldo) in/out */, int32_t launches, int32_t serial);

/* Test/diagnostic hooks (device -> caller device buffers, after prefill / a generate call). */
int qtts_talker_debug_logits(qtts_talker* t, float* logits_dev /* (B, vocab) */, void* stream);
/* The talker cache's page table of one row (0 <= row < max_batch) as it stands on the DEVICE -- what the next launch on `stream` reads:
   ceil(max_seq / 16) entries in slot order.  On a pooled engine an entry without a grant holds n_pages (the sink); on a static engine
   entry i of row b is b x ceil(max_seq / 16) + i.  Synchronises `stream`. */
int qtts_talker_debug_kv_table(qtts_talker* t, int32_t row, int32_t* entries_host /* (ceil(max_seq / 16)) */, void* stream);
/* The code predictor's RAW logits of the last frame step that ran, every pass: what `code_predictor.generate`'s lm_head[j] returned
 * before HF's processors (modeling_qwen3_tts.py:1250-1312; the sampled path is checked against the processed softmax of exactly
 * these numbers, tests/test_gpu_parity.py).  The frame step keeps one row block per pass, so nothing is added to it.  ABI v11. */
int qtts_talker_debug_cp_logits(qtts_talker* t, float* logits_dev /* (num_code_groups - 1, B, cp_vocab) */, void* stream);

/* Per-call statistics of the last generate (for bench.py): kernel-side byte model inputs. */
typedef struct {
    int32_t frames_run;       /* frame steps executed on device (>= n_frames, poll granularity)   */
    int32_t graph_nodes;      /* kernel nodes in the captured frame step (0 if eager)              */
    double weight_bytes_per_frame; /* bytes of packed weights one frame step streams              */
    double gemm_ms_last;      /* HIP-event time of the dominant kernel class over the call, if enabled */
    int64_t gemm_launches_last;
    int32_t long_graphs;      /* long-sequence frame graphs currently cached (one per KV-length bucket the generation reached, ABI v8) */
    int32_t attn_nsplit_last; /* split-KV workgroups per (sequence, kv head) of the last launched frame step (1 = short mode) */
    int32_t attn_span_last;   /* the key span those workgroups partition (the live length's bucket; 0 = short mode) */
    /* the code predictor's fused launch (q|k|v + attention + o-projection of a layer in one launch; ABI v10) */
    int32_t cp_fused_per_step;      /* fused attention + o-projection launches in the frame step last launched / captured (0: separate launches; bf16 only) */
    int64_t cp_fused_launches_last; /* = cp_fused_per_step x frames_run of the last generation                                              */
    int32_t cp_fused_giveups;       /* generations that ended with QTTS_ERR_STATE because a consumer gave up (the engine then left the fused launch) */
    int32_t cp_fused_capacity;      /* engines with the code predictor's fused launches the DEVICE holds at once (register-share account, talker_engine.hip) */
    int32_t cp_fused_active;        /* 1: this engine holds one of those places                                                             */
    int32_t cp_mlp_per_step;        /* fused MLP launches (cp_mlp.hip: gate|up + SwiGLU + down of a code-predictor layer; bf16 and fp32) in that frame step */
    int32_t cp_layer_per_step;      /* of those, the launches that ran BOTH stages of a layer as one (cp_layer.hip, round 6): they count in cp_fused_per_step
                                     * and cp_mlp_per_step too.  (ABI v11: the former reserved word.)                                        */
    int32_t ks_split_per_step;      /* decode GEMMs of that frame step that split K over workgroups and combine inside the launch (skinny.hip: skinny2_ks_kernel;
                                     * bf16 engines at batch 17..32: the o- / down-projections; ABI v12)                                       */
    int32_t attn_gq_per_step;       /* decode-attention launches of that frame step that ran the general kernel family (attn_gq.h: any head shape beyond
                                     * head_dim 128 with a group <= 2, or every launch under QTTS_ATTN_GQ=1; ABI v13: the former reserved word) */
    int32_t admit_calls;            /* qtts_talker_stream_admit calls that succeeded on the last stream (ABI v15) ...        */
    int32_t admitted_rows;          /* ... and the rows they admitted                                                        */
    int32_t row_table_last;         /* 1: the last generation ran with a per-row settings table (qtts_talker_generate_rows; ABI v14) */
    int64_t graph_captures;         /* frame-graph captures over the engine's life: a call that replays a cached graph adds none (ABI v14) */
} qtts_talker_stats;
int qtts_talker_get_stats(qtts_talker* t, qtts_talker_stats* out);
/* Per-class result of the profile mode (qtts_talker_set_profile(t, 1), ABI v8): every launch of the decode GEMM in frames 1..6
 * of the last generate call, timed on its own with the kernel's begin / end timestamps, grouped by (stack, N, K). */
typedef struct {
    int32_t stack;            /* 0 talker layers, 1 code predictor (layers, projection, lm_head), 2 talker codec_head */
    int32_t N, K;             /* GEMM shape: out[M <= 64][N] = x[M][K] . W[N][K]^T */
    int64_t launches;
    double total_ms;          /* sum of the launches' kernel durations */
    double min_us, max_us;
    double bytes_per_launch;  /* algorithmic bytes: the packed weight matrix, N * K * element size */
} qtts_gemm_class;
int qtts_talker_get_gemm_profile(qtts_talker* t, qtts_gemm_class* out, int32_t cap, int32_t* n);
/* Teacher forcing (diagnostic mode for parity measurements; no reference counterpart -- it is how a whole utterance of the
 * bf16 mode is compared decision by decision with the reference's greedy run, SURVEY.md 7 "teacher-forced per-step logits"):
 * until disabled (forced_codes_dev = NULL) every following qtts_talker_generate call -- greedy, min_new_tokens ==
 * max_new_tokens == n_frames + 1, run eagerly -- records the engine's OWN greedy choice of every codebook of every frame into
 * own_dev (B, n_frames + 1, G) int32 ([b][i][0] = own cb-0 token i, [b][f][1 + j] = own sub-code j of frame f) and then
 * continues with forced_codes_dev (B, n_frames, G) int64 instead (frame-level forcing: the 15-pass code predictor runs free
 * inside a frame; its result is replaced before the embedding sum, M:1681-1692; the fed cb-0 token and the repetition-penalty
 * history follow the forced sequence).  logit_slots_dev (n_frames + 1) int32 maps a token step to a slot of
 * logits_trace_dev (n_slots, B, vocab) fp32 that receives the raw cb-0 logits of that step (-1 = not traced); both may be
 * NULL.  All pointers are device pointers owned by the caller and must stay valid while the mode is on. */
int qtts_talker_set_teacher(qtts_talker* t, const int64_t* forced_codes_dev, int32_t n_frames, int32_t* own_dev,
                            const int32_t* logit_slots_dev, float* logits_trace_dev);
/* bench.py's roofline leg.  enable = 1: the next qtts_talker_generate runs its frame steps eagerly and times EVERY launch of the
 * dominant kernel (skinny weight-streaming decode GEMM) of frames 1..6 of the REAL frame step on its own (kernel begin / end
 * timestamps through hipExtLaunchKernelGGL events); results per GEMM class from qtts_talker_get_gemm_profile.  enable = 2:
 * round 2's measurement (the GEMM launches of one frame step replayed in isolation as a hipGraph; the call produces no
 * usable codes).  0 = off. */
int qtts_talker_set_profile(qtts_talker* t, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif /* QTTS_H */
