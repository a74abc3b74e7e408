/* q3asr.h -- C ABI of libq3asr_hip.so: the MI355X (gfx950) backend for the Qwen3-ASR hot path of
 * second-state/qwen3_asr_rs.  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * Each entry point names the reference interface it replaces (file:line in the reference tree).
 * A Rust `feature = "hip"` arm binds these with `extern "C"` exactly as src/backend/mlx/ffi.rs binds
 * mlx-c (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; q3a_last_error() returns the message
 *     (the reference's forward paths are infallible/panic, src/tensor.rs:228,232; its load paths
 *     return anyhow::Result, src/inference.rs:34-65 -- the shim maps non-zero to panic!/bail!).
 *   - an engine handle is thread-compatible (one host thread per handle / per GPU).
 *   - host buffers are caller-owned and never retained after return.
 *   - "utterance" = one independent clip; a batch of B utterances is the data-parallel unit
 *     (new functionality whose semantics equal running the reference B times).
 */
#ifndef Q3ASR_H
#define Q3ASR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct q3a_engine q3a_engine;

/* Engine options. Zero-initialise, then override. */
typedef struct q3a_opts {
  int32_t precise;        /* 0: activations enter the MFMA as bf16, bf16 KV cache (default)
                             1: activations split into bf16 hi+lo pairs (2 MFMAs per tile), fp32 KV cache:
                                near-fp32 logits, used to separate kernel bugs from bf16 rounding        */
  int32_t max_new_tokens; /* generation cap per utterance (reference: 4096, src/inference.rs:153); 0 -> 4096 */
  int32_t use_graph;      /* 1: replay the decode step from a captured hipGraph (default 1 when 0/unset -> see q3a_opts_default) */
  int32_t debug_taps;     /* 1: keep per-stage intermediate tensors readable through q3a_debug_read      */
  int32_t valu_attention; /* 1: use the fp32 VALU attention kernels in default mode too (A/B against the
                             MFMA flash-attention kernels; precise mode always uses them)                 */
  int32_t token_logprobs; /* 1: every generated id also gets its log-probability logit[id] - logsumexp(logits), computed on
                             the device inside the step (graph-replayed or eager) and read with q3a_fetch_logprobs.
                             The one-sequence step then runs the full lm_head GEMV instead of the pruned argmax
                             (same ids).  0 (default): today's kernels, launches and ids                  */
  int32_t reserved[10];
} q3a_opts;

/* Fill `o` with the defaults (precise=0, max_new_tokens=4096, use_graph=1, debug_taps=0, token_logprobs=0). */
void q3a_opts_default(q3a_opts* o);

/* Model dimensions as parsed from config.json (replaces AsrConfig::from_file, src/config.rs:115-121). */
typedef struct q3a_dims {
  int32_t enc_d_model, enc_layers, enc_heads, enc_ffn, num_mel_bins, n_window, n_window_infer,
      conv_channels, enc_output_dim, max_source_positions;
  int32_t vocab_size, hidden_size, intermediate_size, dec_layers, num_q_heads, num_kv_heads, head_dim,
      tie_word_embeddings, mrope_interleaved;
  int32_t mrope_section[4];
  float rms_norm_eps;
  double rope_theta;
} q3a_dims;

/* ---- load -------------------------------------------------------------------------------------- */

/* Device selection of the CLI (src/main.rs:51-65: tch::Cuda::is_available / init_mlx): number of HIP devices this process
 * can use, 0 when there is none (the library has no CPU path).  Never fails. */
int32_t q3a_device_count(void);

/* AsrInference::load (src/inference.rs:30-86): parse config.json, read model.safetensors or the
 * sharded index (src/weights.rs:10-58), build the bf16 device weight arena on GPU `device`. */
int32_t q3a_engine_create(const char* model_dir, int32_t device, const q3a_opts* opts, q3a_engine** out);

/* Weight arena for multi-GPU replicas: pack on one rank, broadcast the bytes over RCCL/xGMI, and
 * create every replica from its device copy (no file reads on the replicas besides config.json). */
int32_t q3a_arena_bytes(const char* model_dir, uint64_t* bytes);
int32_t q3a_arena_pack(const char* model_dir, void* host_dst, uint64_t bytes);
/* `device_arena` stays owned by the caller and must outlive the engine. */
int32_t q3a_engine_create_from_arena(const char* model_dir, int32_t device, void* device_arena, uint64_t bytes,
                                     const q3a_opts* opts, q3a_engine** out);

void q3a_engine_destroy(q3a_engine* e);
/* Last error of `e` (or of the calling thread when e == NULL, e.g. after a failed create). */
const char* q3a_last_error(const q3a_engine* e);
int32_t q3a_get_dims(const q3a_engine* e, q3a_dims* out);
/* 1 when the checkpoint held F16 / F32 matrices: the arena stores every matrix as bf16, so those were rounded to nearest-even
 * (the reference widens them to f32 instead, src/weights.rs:74-89,134-181).  0 for the published BF16 checkpoints, whose
 * bf16 -> f32 widening is exact: arena storage is lossless there.  Vectors (norm weights, biases, conv1) are kept in f32. */
int32_t q3a_weights_rounded(const q3a_engine* e);

/* ---- shape helpers (host integer arithmetic) --------------------------------------------------------- */
/* mel frames for n samples: ceil(n/160) (src/mel.rs:51,83-84). */
int64_t q3a_num_frames(int64_t n_samples);
/* AudioEncoder::get_output_length (src/audio_encoder.rs:269-279). */
int32_t q3a_num_audio_tokens(const q3a_engine* e, int64_t n_frames);
/* AsrInference::build_prompt (src/inference.rs:215-257). Writes 15 + num_audio_tokens + n_prefix ids;
 * `ids` may be NULL to query the length (returned through *len). */
int32_t q3a_build_prompt(int32_t num_audio_tokens, const int32_t* lang_prefix_ids, int32_t n_prefix,
                         int32_t* ids, int32_t* len);

/* ---- stage API (device state chains from one stage to the next) -------------------------------------- */

/* WhisperFeatureExtractor::extract (src/mel.rs:49-96) for B utterances.
 * pcm16k: host f32, utterances concatenated; n_samples[B].  mel_out (nullable): host f32, per
 * utterance a (num_mel_bins, F_b) row-major block, concatenated.  n_frames_out (nullable): [B]. */
int32_t q3a_mel(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B, float* mel_out,
                int32_t* n_frames_out);

/* AudioEncoder::forward (src/audio_encoder.rs:79-169) on the mel of the last q3a_mel call.
 * audio_embeds_out (nullable): host f32 [sum T_b][enc_output_dim].  T_out (nullable): [B]. */
int32_t q3a_encode(q3a_engine* e, float* audio_embeds_out, int32_t* T_out);

/* Steps 5-7 of AsrInference::transcribe (src/inference.rs:110-149): embed `ids`, overwrite the
 * <|audio_pad|> rows with the encoder output of the last q3a_encode, RoPE tables, causal prefill.
 * ids: concatenated prompts, lens[B].  last_logits_out (nullable): host f32 [B][vocab] (last row
 * only; the reference computes all rows and keeps the last, src/inference.rs:156).
 * next_ids (nullable): [B] greedy argmax (first-index tie-break). */
int32_t q3a_prefill(q3a_engine* e, const int32_t* ids, const int32_t* lens, int32_t B, float* last_logits_out,
                    int32_t* next_ids);

/* One iteration of the greedy loop (src/inference.rs:160-200) for all B sequences: feeds the
 * previous argmax (or the ids set by q3a_set_next_tokens), returns the new argmax.
 * done[b]=1 once sequence b has produced an EOS {151643,151645} (the reference breaks out of its
 * loop there, src/inference.rs:163-165).  logits_out nullable host f32 [B][vocab]. */
int32_t q3a_decode_step(q3a_engine* e, int32_t* next_ids, uint8_t* done, float* logits_out);

/* Teacher forcing for parity tests: override the token fed by the next q3a_decode_step. */
int32_t q3a_set_next_tokens(q3a_engine* e, const int32_t* ids, int32_t B);

/* ---- whole path ---------------------------------------------------------------------------------- */

/* Copy B utterances (host f32 16 kHz, concatenated) into the engine's HBM input buffer. */
int32_t q3a_upload_pcm(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B);

/* Steps 2-8 of AsrInference::transcribe (src/inference.rs:95-200) on the resident batch: mel ->
 * encoder -> prompt/injection -> prefill -> greedy decode.  lang_prefix_ids (nullable) =
 * tokenizer.encode("language {Lang}") when the language is forced (src/inference.rs:246-251).
 * fixed_new_tokens > 0: run exactly that many decode iterations ignoring EOS (throughput mode);
 * 0: stop every sequence at its first EOS, capped by max_new (<= opts.max_new_tokens). */
int32_t q3a_run_resident(q3a_engine* e, const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new,
                         int32_t fixed_new_tokens);

/* Generated ids of the last q3a_run_resident: out_ids host [B][stride], out_lens [B] (EOS excluded,
 * as generated_ids in src/inference.rs:167). */
int32_t q3a_fetch_ids(q3a_engine* e, int32_t* out_ids, int32_t stride, int32_t* out_lens);

/* Log-probability (natural log, fp32) of every id q3a_fetch_ids returns for the last run, same order, same lengths
 * (EOS excluded in the natural-EOS mode): out_lp host [B][stride], out_lens [B].  Needs opts.token_logprobs = 1; works after
 * q3a_run_resident, q3a_transcribe_batch[_ptrs] and the stage API (q3a_prefill + q3a_decode_step: the lp of each step's argmax,
 * also when the next token is forced).  Whisper's avg_logprob is the mean of a row.  Fails (q3a_last_error) on an engine created
 * without the option and before anything has been generated.  q3a_group_transcribe returns no log-probabilities: a caller that
 * needs them runs each rank's slice (q3a_group_partition) on q3a_group_engine's handle and fetches them there. */
int32_t q3a_fetch_logprobs(q3a_engine* e, float* out_lp, int32_t stride, int32_t* out_lens);

/* upload + run + fetch: AsrInference::transcribe steps 2-8 (src/inference.rs:95-200) for B utterances, host PCM in,
 * generated ids on the host out -- the window SURVEY.md section 8d times.  The input copy is overlapped with the front
 * end: the (pageable) caller buffers are copied by a few host threads into a pinned mirror of the device layout and shipped
 * in pieces on a copy stream; the log-mel kernel of a piece's utterances runs as soon as that piece has landed. */
int32_t q3a_transcribe_batch(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B,
                             const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new,
                             int32_t fixed_new_tokens, int32_t* out_ids, int32_t stride, int32_t* out_lens);
/* The same with one pointer per utterance (pcm16k[b] -> n_samples[b] floats): what a caller that decoded B files into B
 * buffers has (src/audio.rs:7 returns one Vec<f32> per file) -- no concatenation on the host. */
int32_t q3a_transcribe_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                                  const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new,
                                  int32_t fixed_new_tokens, int32_t* out_ids, int32_t stride, int32_t* out_lens);
/* Where the input side of the last q3a_transcribe_batch[_ptrs] call spent its time. */
typedef struct q3a_io_timings {
  float stage_ms; /* host clock: entry -> last piece copied to pinned memory and its H2D copy + log-mel enqueued */
  float h2d_ms;   /* hipEvents on the copy stream: first piece issued -> last piece landed */
  float wall_ms;  /* host clock of the whole call (upload + hot path + ids on the host) */
  int32_t pieces, threads; /* H2D pieces (runs of utterances) and host copy threads used */
  int32_t mode;   /* 1: staged + overlapped (default); 0: Q3A_UPLOAD_MODE=0, one pageable copy per utterance on the compute stream */
} q3a_io_timings;
int32_t q3a_io_timings_last(const q3a_engine* e, q3a_io_timings* out);

/* ---- multi-GPU: one process, one host thread per GPU ------------------------------------ */
/* The reference is single-device (src/main.rs:51-65 picks ONE device); a batch of independent utterances is new
 * functionality whose result equals running AsrInference::transcribe (src/inference.rs:89) once per utterance. */
typedef struct q3a_group q3a_group;
/* Load once, replicate to n_gpus GPUs: the checkpoint is read and packed on the host ONCE, uploaded to devices[0] and
 * shipped to the other GPUs with ONE ncclBroadcast of the whole weight arena over xGMI (RCCL, ncclCommInitAll; librccl is
 * dlopen'ed here).  devices == NULL means 0..n_gpus-1.  Every GPU then owns a q3a_engine created from its copy. */
int32_t q3a_group_create(const char* model_dir, int32_t n_gpus, const int32_t* devices, const q3a_opts* opts, q3a_group** out);
void q3a_group_destroy(q3a_group* g);
int32_t q3a_group_size(const q3a_group* g);
int32_t q3a_group_used_rccl(const q3a_group* g);  /* 1 when the arena went through ncclBroadcast */
/* Start-up stage times of q3a_group_create in seconds: out4 = {pack (read + lay out the checkpoint into pinned host memory),
 * upload (one asynchronous H2D copy to the first GPU), broadcast (RCCL init + ONE ncclBroadcast of the arena), engines}. */
int32_t q3a_group_startup_seconds(const q3a_group* g, double* out4);
const char* q3a_group_last_error(const q3a_group* g);
q3a_engine* q3a_group_engine(q3a_group* g, int32_t rank);  /* borrowed handle of rank's engine (stage API, timings) */
/* Static contiguous split of n_items utterances: rank gets [*begin, *end) (the first n_items % world_size ranks one more). */
void q3a_group_partition(int32_t n_items, int32_t world_size, int32_t rank, int32_t* begin, int32_t* end);
/* q3a_transcribe_batch over the group: utterances are partitioned with q3a_group_partition, every GPU runs its slice from
 * its own host thread, results land in the caller's arrays in utterance order.  No collective on the data path. */
int32_t q3a_group_transcribe(q3a_group* g, const float* pcm16k, const int64_t* n_samples, int32_t B,
                             const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new, int32_t fixed_new_tokens,
                             int32_t* out_ids, int32_t stride, int32_t* out_lens);
/* The same with one pointer per utterance (see q3a_transcribe_batch_ptrs). */
int32_t q3a_group_transcribe_ptrs(q3a_group* g, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                                  const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new, int32_t fixed_new_tokens,
                                  int32_t* out_ids, int32_t stride, int32_t* out_lens);

/* ---- measurement ---------------------------------------------------------------------------------- */

typedef struct q3a_timings {
  float mel_ms, encoder_ms, prefill_ms, decode_ms, total_ms; /* hipEvent times of the last q3a_run_resident */
  int32_t decode_steps, batch, total_audio_tokens, total_prompt_tokens;
} q3a_timings;
int32_t q3a_stage_timings(const q3a_engine* e, q3a_timings* out);

/* Per-kernel-class timing of ONE decode step, each launch bracketed by hipEvents on the engine's
 * stream (eager, not graph).  Requires a batch in decode state (after q3a_run_resident/q3a_prefill).
 * class ids: see Q3A_KC_* ; arrays have Q3A_KC_COUNT entries. */
enum { Q3A_KC_GEMV = 0 /* qkv and gate/up GEMVs (2 weight rows per wave) */, Q3A_KC_DECODE_ATTN = 1, Q3A_KC_ARGMAX = 2,
       Q3A_KC_GEMM = 3, Q3A_KC_NORM = 4, Q3A_KC_OTHER = 5, Q3A_KC_GEMV_O = 6, Q3A_KC_GEMV_DOWN = 7,
       Q3A_KC_GEMV_LM_HEAD = 8, Q3A_KC_COUNT = 9 };
typedef struct q3a_kernel_profile {
  float total_us[Q3A_KC_COUNT];
  int32_t launches[Q3A_KC_COUNT];
  double weight_bytes[Q3A_KC_COUNT]; /* algorithmic weight bytes streamed by the class in the step */
} q3a_kernel_profile;
int32_t q3a_profile_decode_step(q3a_engine* e, q3a_kernel_profile* out);

/* Back-to-back timing of the dominant decode kernel (the qkv and gate/up GEMVs, gemv1_kernel<2,..>): `reps`
 * sweeps over ALL decoder layers' qkv and gate/up matrices (0.59 GB at 0.6B, larger than the 256 MB
 * Infinity Cache, so every launch streams from HBM as in a real step), captured in a hipGraph and replayed between
 * HIP events on the engine's stream (average of 3 replays; an eager host loop would time the host).
 * avg_us = elapsed / launches; bytes_per_launch = algorithmic weight bytes per launch.
 * Needs decode state with <= 2 sequences (the GEMV path); does not change it. */
int32_t q3a_profile_weight_stream(q3a_engine* e, int32_t reps, float* avg_us, double* bytes_per_launch, int32_t* launches);

/* Measured denominators for the roofline fractions (SURVEY.md section 8d "Peaks to divide by: measure on the box"; csrc/k_peaks.hip):
 * a read-only HBM stream over 2 GiB (the access pattern of the decode-step weight streams), a 1 GiB device copy and a triad
 * (bytes counted on every stream they touch), and the library's own 256x256x64 bf16 GEMM on 8192^3, once on constant and once on random operands -- each the best of `reps`
 * launches between two HIP events.  Needs 2 GiB of free device memory; not on the product path. */
typedef struct q3a_peaks {
  double hbm_read_gbps, hbm_copy_gbps, hbm_triad_gbps; /* GB/s (1e9 bytes per second) */
  double hbm_read_bytes;                                /* bytes one read sweep covers */
  double mfma_bf16_tflops;                              /* 2 M N K / time, operands = one constant (the chip's clock stays high: the ceiling) */
  int32_t gemm_m, gemm_n, gemm_k, n_cu, reps, reserved;
  double mfma_bf16_tflops_random;                       /* the same GEMM on random operands (sign + mantissa bits toggling: what real data draws; the chip clocks down) */
} q3a_peaks;
int32_t q3a_measure_peaks(int32_t device, int32_t reps, q3a_peaks* out);

/* Debug taps (opts.debug_taps=1): copy a named intermediate to host. `bytes` = capacity of dst;
 * *actual receives the tap size. Names: mel conv1 conv2 conv3 enc_in enc_layer0 enc_last
 * audio_embeds dec_embed dec_layer0 dec_last_hidden logits lm_head_bound ([vocab][2] fp32: approximate logit and its error bound
 * of the pruned one-sequence argmax, written next to the stored logits).  "lm_head_prune_stats" (int32[2]: 16-row blocks rescored
 * by the pruned argmax, its launches; cumulative over the engine's life) and "device_bytes" (uint64: bytes of device memory the
 * workspace buffers of ALL engines of the process hold right now -- tables, activations, KV caches, the int8 lm_head copy, taps; not
 * the weight arenas) and "graph_captures" (int32: decode-step graphs captured over the engine's life; a replay adds none) are readable
 * without debug taps; so are the settings "logit_bias", "logit_bias_stats", "sampling" and "repetition" and the counters "draft_stats"
 * (their own sections below), and the setting "sequence_bias" (its own section below). */
int32_t q3a_debug_read(q3a_engine* e, const char* name, void* dst, uint64_t bytes, uint64_t* actual);

/* ---- pipeline shell: host-only helpers around the hot path -------------- */

/* load_audio (src/audio.rs:7): RIFF/WAVE PCM s8/s16/s24/s32/f32 -> mono (channel mean, audio.rs:192-200) -> f32
 * scaled by 1/2^(bits-1) (audio.rs:177) -> `target_sr` with this backend's deterministic windowed-sinc polyphase
 * resampler (the reference's FFmpeg / rubato resamplers are not reproducible outside their code bases).
 * *samples_out is malloc'ed; release it with q3a_free. */
int32_t q3a_load_audio(const char* path, int32_t target_sr, float** samples_out, int64_t* n_out);
int32_t q3a_resample(const float* in, int64_t n, int32_t sr_in, int32_t sr_out, float** samples_out, int64_t* n_out);
/* The reference's WAV-fallback resampler (src/audio.rs:220-245: rubato SincFixedIn, sinc_len 256, f_cutoff 0.95, Linear,
 * oversampling 256, BlackmanHarris2, one `process` call over the whole clip), restated from the crate's published
 * algorithm (rubato 0.16.2 is not vendored in the reference and cannot be built here): same filter family and
 * parameters, output n at input time (n+1)/ratio, the last ~129 input samples produce no output.  q3a_load_audio uses it
 * when the environment has Q3A_RESAMPLER=rubato. */
int32_t q3a_resample_rubato(const float* in, int64_t n, int32_t sr_in, int32_t sr_out, float** samples_out, int64_t* n_out);
void q3a_free(void* p);

/* AsrTokenizer (src/tokenizer.rs:4-50) over HuggingFace's tokenizer.json (byte-level BPE). */
typedef struct q3a_tokenizer q3a_tokenizer;
int32_t q3a_tokenizer_create(const char* tokenizer_json_path, q3a_tokenizer** out);
void q3a_tokenizer_destroy(q3a_tokenizer* t);
/* decode(ids, skip_special_tokens) -> UTF-8 (tokenizer.rs:42-49). *len = bytes needed (excluding NUL). */
int32_t q3a_tokenizer_decode(const q3a_tokenizer* t, const int32_t* ids, int32_t n, int32_t skip_special, char* out,
                             int32_t cap, int32_t* len);
/* encode(text, add_special_tokens = false) (tokenizer.rs:33-39): added tokens cut out first, then the normaliser
 * tokenizer.json names (NFC for Qwen), the Qwen2 pre-tokenisation pattern over Unicode code points and byte-level BPE.  UTF-8 in. */
int32_t q3a_tokenizer_encode(const q3a_tokenizer* t, const char* text, int32_t* ids, int32_t cap, int32_t* n);
/* The normaliser step on its own: Unicode NFC (UAX #15; decomposition / composition data of Unicode 13.0 -- later additions
 * pass through unchanged).  *len = bytes needed (excluding NUL). */
int32_t q3a_normalize_nfc(const char* utf8, char* out, int32_t cap, int32_t* len);

/* parse_asr_output (src/inference.rs:276-305); capitalize_first (inference.rs:307-313). */
int32_t q3a_parse_asr_output(const char* raw, int32_t language_forced, char* language, int32_t language_cap, char* text,
                             int32_t text_cap);
int32_t q3a_capitalize_first(const char* s, char* out, int32_t cap);

/* ---- forced aligner (Qwen3-ForcedAligner: word timestamps) ------------------------------------------------------------------
 * An aligner checkpoint is the ASR network with a classifier head over classify_num time classes (timestamp_segment_time ms
 * each) in place of the vocabulary lm_head; config.json: thinker_config.classify_num, timestamp_token_id and
 * timestamp_segment_time at the top level or in thinker_config (defaults 151705 / 80 ms).  Its input is the audio followed by
 * the transcript's words, each followed by two <timestamp> markers; one prefill, no decode: the argmax class at a marker row
 * times timestamp_segment_time is the start (first marker) or end (second) of the word.  An aligner engine refuses
 * q3a_prefill, q3a_decode_step, q3a_run_resident, q3a_transcribe_batch* and q3a_group_create; an ASR engine refuses q3a_align*. */

/* classify_num (0 for an ASR engine), timestamp_token_id and ms per class (0 for an ASR engine). */
int32_t q3a_aligner_info(const q3a_engine* e, int32_t* classify_num, int32_t* timestamp_token_id, float* segment_ms);
/* The aligner prompt: <|audio_start|> <|audio_pad|> x num_audio_tokens <|audio_end|> text_ids, where text_ids is the word and
 * marker part (q3a_align_text_ids).  `ids` may be NULL to query the length (*len = num_audio_tokens + 2 + n_text). */
int32_t q3a_build_align_prompt(int32_t num_audio_tokens, const int32_t* text_ids, int32_t n_text, int32_t* ids, int32_t* len);
/* Stage form, after q3a_mel + q3a_encode of the same B utterances: one prefill of the B prompts ids / lens (concatenated),
 * then the head at every id equal to timestamp_token_id.  out_classes host [B][stride] (utterance b's markers in prompt order),
 * out_counts [B] markers per utterance (0 for an empty transcript); fails when a count exceeds stride.  logits_out (nullable):
 * host fp32 [sum of out_counts][classify_num], the markers of all utterances in order. */
int32_t q3a_align(q3a_engine* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t* out_classes, int32_t stride,
                  int32_t* out_counts, float* logits_out);
/* Whole path, host PCM in (as q3a_transcribe_batch_ptrs): text_ids = the word and marker parts of the B utterances
 * concatenated, text_lens [B]; the prompts are built with q3a_build_align_prompt.  Outputs as q3a_align.  q3a_stage_timings
 * reports mel, encoder and prefill (the head included) with decode_steps = 0. */
int32_t q3a_align_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B, const int32_t* text_ids,
                             const int32_t* text_lens, int32_t* out_classes, int32_t stride, int32_t* out_counts);
/* Host helpers (no engine).  Words of a transcript as the original aligner splits them for languages other than Japanese and
 * Korean: every CJK ideograph is a word of its own, whitespace separates words, and only letters, numbers, apostrophes and CJK
 * ideographs are kept.  language (nullable): "japanese" / "ja" and "korean" / "ko" need morphological analysers and are
 * refused.  out: the words joined by '\n' and NUL-terminated; *n_words; *len = bytes needed (excluding NUL). */
int32_t q3a_split_words_for_alignment(const char* utf8, const char* language, char* out, int32_t cap, int32_t* n_words,
                                      int32_t* len);
/* The word and marker part of the prompt: for each of the n_words words (UTF-8) encode(word) then two timestamp_token_id.
 * *n = ids needed; at most cap are written. */
int32_t q3a_align_text_ids(const q3a_tokenizer* t, const char* const* words, int32_t n_words, int32_t timestamp_token_id,
                           int32_t* ids, int32_t cap, int32_t* n);
/* Monotone word times from raw marker times (ms): the longest non-decreasing subsequence is kept, runs of at most 2 other
 * values snap to the nearer kept neighbour (the left one on a tie), longer runs are interpolated linearly between their kept
 * neighbours; results are truncated to whole ms.  out may alias ms. */
int32_t q3a_fix_timestamps(const float* ms, int32_t n, float* out);

/* ---- scoring a given transcript: per-token log-probabilities in one prefill ---------------------------------------------------
 * Given audio and a transcript somebody else wrote (a label, another system's hypothesis), how likely does this model find it,
 * token by token, and what would it have written instead?  For utterance b with prompt P_b (length p; what q3a_build_prompt
 * returns) and targets y_0 .. y_{n-1} (n = target_lens[b], may be 0) the engine prefills P_b ++ y_0 .. y_{n-2} ONCE (the last target
 * is never fed); row p - 1 + i of the final residual stream predicts y_i.  With l = lm_head(final_norm(row)) in fp32:
 *   out_lp[b][i]      = l[y_i] - logsumexp(l)                (natural log)
 *   out_top_ids[b][i] = argmax l                             (larger value, then smaller index)
 *   out_top_lp[b][i]  = l[top id] - logsumexp(l)
 * -- what a greedy loop fed y_0 .. y_{i-1} instead of its own argmax would see at step i.  l[y_i] is the accumulator the maximum
 * is taken over: out_lp <= 0 always, and out_lp == out_top_lp bit for bit where y_i is the argmax.  The ids are scored exactly as
 * given: append 151645 (<|im_end|>) as the last target to score "stop here".  The rows x vocabulary logits are never stored (the
 * lm_head reduces in its epilogue) unless logits_out asks for them.
 * Refused: a target < 0 or >= vocabulary, a target equal to <|audio_pad|> (151676: the engine finds audio rows by this id),
 * target_lens[b] > stride, an aligner engine, the stage form without q3a_encode.  n = 0 for every utterance is valid and returns
 * nothing.  No engine option is needed (opts.token_logprobs is about generated ids) and both modes work.  Afterwards the engine
 * holds no decode state, as after q3a_align: until the next prefill q3a_decode_step, q3a_set_next_tokens and q3a_fetch_ids
 * fail.  q3a_stage_timings reports mel, encoder and prefill (the head included; total_ms = mel through head) with decode_steps =
 * 0 and total_prompt_tokens = the rows prefilled; q3a_debug_read(e, "score_head_ms", ..) is the head's own time (a float).
 * Results are bit-identical from run to run on the same engine and inputs.
 * Out of scope: q3a_group_* (score each rank's slice on q3a_group_engine's handle, as for log-probabilities), several hypotheses
 * sharing one encoder pass.  (Continuing generation after a given prefix: "draft-verified decoding" below.) */

/* Stage form, after q3a_mel + q3a_encode of the same B utterances.  prompt_ids / target_ids are concatenated over the batch;
 * outputs are host [B][stride], entries past target_lens[b] untouched; out_top_ids / out_top_lp nullable.  logits_out (nullable;
 * tests and debugging): host fp32 [sum of target_lens][vocab], the scored rows of all utterances in order. */
int32_t q3a_score(q3a_engine* e, const int32_t* prompt_ids, const int32_t* prompt_lens, const int32_t* target_ids,
                  const int32_t* target_lens, int32_t B, float* out_lp, int32_t* out_top_ids, float* out_top_lp, int32_t stride,
                  float* logits_out);
/* Whole path, host PCM in (as q3a_transcribe_batch_ptrs: overlapped upload, prompts set up before the encoder); the prompts are
 * q3a_build_prompt(T_b, lang_prefix_ids, n_prefix): one language prefix for the batch. */
int32_t q3a_score_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                             const int32_t* lang_prefix_ids, int32_t n_prefix, const int32_t* target_ids, const int32_t* target_lens,
                             float* out_lp, int32_t* out_top_ids, float* out_top_lp, int32_t stride);

/* ---- draft-verified decoding: verify a transcript in one prefill, decode on ---------------------------------------------------------
 * The caller hands in a DRAFT transcript per utterance (the previous partial transcript of a stream, a smaller model's output, a cached
 * or human transcript that is "mostly right").  One prefill decides, on the device, the longest prefix of the draft the greedy loop would
 * have written itself, and the captured decode step continues from exactly there: the result IS the greedy transcript; a good draft
 * makes it cheap, a bad one costs one longer prefill.  (Exact as far as a greedy id is: the verified rows come from the prefill kernels,
 * the loop's from the decode kernels, and the two agree to the mode's rounding noise on a logit -- 1e-5 precise, bf16 noise by default.
 * A step whose top-1 / top-2 margin lies inside that noise may resolve differently on the two paths, exactly as between graph replay and
 * the oracle; DESIGN.md section 3.13 has the measured figures.)
 * For utterance s with prompt P_s (length p) and draft d_0 .. d_{n-1} (n >= 0) the engine prefills P_s ++ d_0 .. d_{n-1} ONCE (every
 * draft id is fed, unlike scoring) and runs the lm_head at the n + 1 rows p - 1 .. p - 1 + n.  With t_i the argmax of row p - 1 + i
 * (larger value, then smaller id):
 *   k_s   = min{ i < n : t_i != d_i }, n if there is none -- the FIRST mismatch, not the number of matches;
 *   tok_s = t_{k_s}.
 * Afterwards the engine is in exactly the state the greedy loop has after producing the k_s + 1 tokens d_0 .. d_{k_s - 1}, tok_s: the
 * out_ids rows hold them, step_count = k_s + 1, pos = p + k_s, next_tok = tok_s, the RoPE row of pos, the embedding of tok_s and its
 * pre-normalised copy for the batched path are set; done, n_done and both pinned progress words are what argmax_finalize would have
 * left (the prefill counts as one finalize; an EOS as tok_s finishes the sequence with k_s ids); the out_stride guard applies when
 * k_s >= max_new; cache rows >= p + k_s are stale and are overwritten by the steps that follow.  With opts.token_logprobs the
 * log-probabilities 0 .. k_s are the head's top_lp at those rows (the target's lp bit for bit where the target is the argmax, as in
 * scoring).  Decoding continues with the unchanged captured step (natural EOS, run-ahead loop).
 * A logit bias composes: the verify head is a head of the GENERATION paths and works on l' = l + b (b added to the fp32 accumulator in
 * front of the max, log-sum and target channels; -inf stays -inf and never yields NaN), under the tolerance rule of that section.
 * q3a_score* stays unbiased and bit-identical.
 * Refused (q3a_last_error; the engine stays usable): a draft id < 0 or >= vocabulary; a draft id equal to <|audio_pad|> (151676) or to
 * either EOS id (151643, 151645: a draft ends where its ids end); n > max_new (the engine's max_new_tokens in the stage form); an aligner
 * engine; sampling or repetition control set (their choices are not an argmax of the row alone); a live beam search.  (Likewise a
 * sequence bias: its own section below.)
 * q3a_debug_read(e, "draft_stats", ..) (int32 [1 + rounds]: rounds run by the last draft call, then the rows prefilled in each).
 * q3a_stage_timings reports the prefill (every round, head and accept included) and the decode steps actually run.
 * Out of scope: appending rows to an existing KV cache (the prefill attention keeps q_len = kv_len: every round is a full prefill);
 * drafts under sampling or repetition control; per-slot drafts in beam search; q3a_group_*; a sliding window for endless streams. */

/* Stage form, after q3a_mel + q3a_encode of the same B utterances.  prompt_ids / draft_ids are concatenated over the batch.
 * accepted_out [B] = k_s, next_ids_out [B] = tok_s (both nullable).  logits_out (nullable; a test aid): host fp32
 * [sum of (n + 1)][vocab], the verified rows of all utterances in order (l' under a bias).  Afterwards q3a_decode_step,
 * q3a_set_next_tokens, q3a_fetch_ids and q3a_fetch_logprobs work as after q3a_prefill. */
int32_t q3a_prefill_draft(q3a_engine* e, const int32_t* prompt_ids, const int32_t* prompt_lens, const int32_t* draft_ids,
                          const int32_t* draft_lens, int32_t B, int32_t* accepted_out, int32_t* next_ids_out, float* logits_out);
/* Whole path, host PCM in (the overlapped upload of q3a_transcribe_batch_ptrs; natural EOS only; max_new as there).  Outputs as
 * q3a_transcribe_batch_ptrs, plus accepted_out [B] (nullable) = k_s of the last round.
 * Rounds: after a round with first mismatch k_s the rest of the draft is often still right (a substitution).  A further round runs
 * while round + 1 < max_rounds and the longest rejected tail max_s (n_s - k_s - 1) is at least max(min_tail, 1); it prefills the
 * drafts q3a_draft_next_round gives (cut to max_new ids).  Mel and encoder run once.  Exactness never depends on the rule, only cost. */
int32_t q3a_transcribe_draft_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                                        const int32_t* lang_prefix_ids, int32_t n_prefix, const int32_t* draft_ids, const int32_t* draft_lens,
                                        int32_t max_new, int32_t max_rounds, int32_t min_tail, int32_t* out_ids, int32_t stride,
                                        int32_t* out_lens, int32_t* accepted_out);
/* Host helper, no engine: the draft of the next round, d[:k] ++ [tok] ++ d[k+1:], or d[:k] when tok is an EOS id (0 <= k <= n).
 * *n_out = ids needed, at most cap written. */
int32_t q3a_draft_next_round(const int32_t* draft, int32_t n, int32_t k, int32_t tok, int32_t* out, int32_t cap, int32_t* n_out);
/* The accept kernel on its own (no model; host arrays in and out).  Sequence s owns draft_ids[draft_off[s] .. draft_off[s + 1]) and
 * the head rows top_ids / top_lp [draft_off[s] + s ..] (n + 1 of them); top_lp / out_lp nullable.  embed: bf16 [V][H], H % 64 == 0;
 * norm_w (nullable [H]): also the pre-normalised copy, nn_x [groups][32 * H] bf16 in fragment order and nn_ss [groups][H / 16][32]
 * with groups of group_size sequences; cos_t / sin_t [max_pos][64].  Output buffers arrive pre-filled with the caller's sentinel and
 * come back whole (a write outside one fails the call): accepted [2 S] (k, then tok), out_ids / out_lp [S][out_stride],
 * state = next_tok [S] | step_count [S] | pos [S] | done [S] | n_done | progress word 0 | progress word 1, x_next [S][H],
 * rope_cur [S][128]. */
int32_t q3a_selftest_draft_accept(int32_t device, int32_t S, const int32_t* draft_ids, const int32_t* draft_off, const int32_t* prompt_lens,
                                  const int32_t* top_ids, const float* top_lp, int32_t out_stride, const uint16_t* embed, int32_t V, int32_t H,
                                  const float* norm_w, int32_t group_size, const float* cos_t, const float* sin_t, int32_t max_pos,
                                  int32_t* accepted, int32_t* out_ids, float* out_lp, int32_t* state, float* x_next, float* rope_cur,
                                  uint16_t* nn_x, float* nn_ss);

/* ---- beam search: n-best hypotheses with scores, selected on the device ------------------------------------------------------------
 * U utterances of W slots each (1 <= W <= 8, U * W <= 32): sequence u * W + j of the engine's batch is slot j of utterance u, and the
 * whole-path call uploads each clip once per slot (mel, encoder and prefill run W times per utterance; sharing them is out of scope).
 * A hypothesis has ids (EOS excluded, as q3a_fetch_ids), an fp32 score = the sum of the natural-log probabilities of its tokens (the
 * EOS's included when it finished; one fp32 add per round, score_parent + lp) and a finished flag.  The log-probability of token v on a
 * sequence's row of fp32 logits l is lp = (l[v] - m) - log sum exp(l - m), m the row maximum, the sum in fp32 in a fixed order (the
 * formula of q3a_score); results are bit-identical from run to run.
 *   Round 0 works on the prefill's logits: only slot 0 of every utterance is live (score 0), the other slots are empty (score -inf) and
 *   produce no candidates.  In a round every live unfinished slot s contributes its W best tokens (larger logit, then smaller id; -inf
 *   is a legal logit and ranks last; NaN is outside the contract) as (score_s + lp, s, token) and every finished slot itself as
 *   (score, s, none).  Candidates are ordered by larger score, then smaller parent slot, then smaller token id ("none" first); the first W
 *   survive.  In rank order a survivor takes its parent's slot if that is still free; the remaining survivors, in rank order, take the
 *   free slots in ascending order -- only these have their history (generated KV rows) copied.  A survivor whose token is 151643 or
 *   151645 becomes finished; the token is not appended to its ids.  The search ends when all W slots of every utterance are finished, or
 *   after max_new rounds (rounds 0 .. max_new - 1; max_new <= 0 means, and larger values are capped by, opts.max_new_tokens); unfinished
 *   hypotheses are returned with finished = 0 and max_new ids.  Output per utterance: the W hypotheses by larger score, then smaller slot;
 *   empty slots (length 0, score -inf) last.  With W = 1 the ids and lengths are those of the greedy natural-EOS run, bit for bit.
 * The step's state never leaves the device inside the loop: top-W selection, the round's bookkeeping and the KV reorder are launches of
 * the (captured and replayed) step, and the stop word is read from pinned host memory as in the greedy loop.
 * Refused (q3a_last_error): width < 1 or > 8; U * width > 32 sequences; a batch not divisible by width, or prompts of one utterance
 * that differ in length (q3a_beam_begin); stride < max_new; an aligner engine; q3a_beam_step / q3a_beam_fetch without q3a_beam_begin.
 * Afterwards the engine holds no decode state (as after q3a_score): q3a_decode_step, q3a_set_next_tokens and q3a_fetch_ids fail until the
 * next prefill.  q3a_stage_timings reports mel, encoder, prefill and decode with decode_steps = rounds - 1.  q3a_debug_read (no debug
 * taps needed) reflects the last round: "beam_topk_ids" (int32 [S][W]) / "beam_topk_lp" (fp32 [S][W]); "beam_parent" (int32 [S]: the
 * SEQUENCE u * W + slot the hypothesis now in this slot continued), "beam_token" (int32 [S]: the survivor's token, an EOS id when it
 * finished in this round, -1 for a hypothesis that was finished before), "beam_score" (fp32 [S]), "beam_finished" (uint8 [S]);
 * "beam_stats" (int32 [4]: rounds run, survivors that needed a copy, KV rows copied, hypotheses finished; cumulative over the call).
 * Out of scope: q3a_group_* (search each rank's slice on q3a_group_engine's handle), sharing the encoder or the prompt's KV rows
 * across slots, length penalties inside the search (re-rank the returned list on the host), sampling, log-probabilities of
 * alternatives that did not survive, U * W > 32. */

/* Whole path, host PCM in (as q3a_transcribe_batch_ptrs).  out_ids [U][width][stride], out_lens / out_scores / out_finished [U][width],
 * out_lp nullable [U][width][stride + 1]: per token, then the EOS's when finished. */
int32_t q3a_beam_search_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t U,
                                   const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t width, int32_t max_new, int32_t* out_ids,
                                   int32_t stride, int32_t* out_lens, float* out_scores, uint8_t* out_finished, float* out_lp);
/* Stage form, directly after q3a_mel / q3a_encode / q3a_prefill of U * width sequences in which each utterance appears `width` times in a
 * row.  q3a_beam_begin: round 0 on the prefill's logits.  q3a_beam_step: one decode step and its round; logits_out (nullable): host
 * fp32 [S][vocab], the rows this round selected from; fails once max_new_tokens rounds have run.  q3a_beam_fetch: as the whole path's
 * outputs, for the rounds run so far. */
int32_t q3a_beam_begin(q3a_engine* e, int32_t width);
int32_t q3a_beam_step(q3a_engine* e, uint8_t* all_finished, float* logits_out);
int32_t q3a_beam_fetch(q3a_engine* e, int32_t* out_ids, int32_t stride, int32_t* out_lens, float* out_scores, uint8_t* out_finished,
                       float* out_lp);
/* The three kernels on their own (no model; host arrays in, host arrays out).  top-W: logits [S][V] -> out_ids / out_lp [S][W].
 * advance: one round of U x W slots on the given tables and state (score -inf and not finished = an empty slot); parent_out holds
 * sequence indices, token_out -1 for "none".  kv reorder: cache = the K cache followed by the V cache, each
 * [layers][S][n_kv][max_ctx][128] elements of elem_bytes (2 or 4); for every sequence j with parent[j] != j rows lo[j] .. hi[j] of both
 * become a copy of sequence parent[j]'s (which must share lo and hi). */
int32_t q3a_selftest_beam_topk(int32_t device, const float* logits, int32_t S, int32_t V, int32_t W, int32_t* out_ids, float* out_lp);
int32_t q3a_selftest_beam_advance(int32_t device, int32_t U, int32_t W, const int32_t* topk_ids, const float* topk_lp, const float* score_in,
                                  const uint8_t* finished_in, int32_t* parent_out, int32_t* token_out, float* score_out, uint8_t* finished_out);
int32_t q3a_selftest_kv_reorder(int32_t device, void* cache, int32_t elem_bytes, int32_t layers, int32_t S, int32_t n_kv, int32_t max_ctx,
                                const int32_t* lo, const int32_t* hi, const int32_t* parent);

/* ---- constrained decoding: a per-token logit bias inside every lm_head form ------------------------------------------------------
 * An engine holds one dense fp32 vector b[vocab]; every entry is finite or -inf.  While a bias is set, every head of the GENERATION
 * paths works on l' = l + b instead of the fp32 logits l.  The sum is one fp32 operation that a kernel may fuse with the multiply
 * that forms l (acc * rstd + b), so it is specified to a tolerance, not bitwise: |l' - (l + b)| <= 2^-22 (|l| + |b|) (one rounding of
 * l, one of the sum); exact for b = 0, and l' = -inf exactly where b = -inf.  Everything downstream is defined on l' with the rules
 * it has without a bias:
 *   the greedy id is argmax l' (larger value, then smaller id);
 *   token log-probabilities (q3a_fetch_logprobs) are l'[id] - logsumexp(l'): the renormalised distribution, suppressed tokens
 *     contribute 0 to the sum, never NaN;
 *   beam search selects its top-W and computes lp on l';
 *   logits_out of q3a_prefill / q3a_decode_step / q3a_beam_step and the "logits" tap hold l'; the "lm_head_bound" tap holds the
 *     approximate BIASED logit and its bound ((-inf, 0) for a suppressed row).
 * The one-sequence pruned argmax ("lm_head_prune") keeps running under a bias: its int8 pre-pass adds b and widens the bound by the
 * two sums' roundings, rows with b = -inf are never candidates, and a 16-row block with every row suppressed is never rescored (an
 * allow-list makes the second pass cheaper).
 * Applies to: q3a_prefill (next_ids, last_logits_out), q3a_decode_step, q3a_run_resident, q3a_transcribe_batch[_ptrs],
 * q3a_fetch_logprobs, q3a_beam_*.  Group runs: set it on each q3a_group_engine handle; there is no group-level call.
 * Does NOT apply to q3a_score* and q3a_align*: they score and classify the unconstrained model, and their results are bit-identical
 * with and without a bias.
 * State: the bias persists across calls until cleared.  q3a_set_logit_bias drops the decode state as q3a_score does --
 * q3a_decode_step, q3a_set_next_tokens and q3a_fetch_ids fail until the next prefill -- so a bias never changes under a live sequence
 * or a captured step.  The vector is uploaded inside the call; no decode loop returns to the host for it.
 * Refused (q3a_last_error): an id < 0 or >= vocab; a duplicate id; a NaN or +inf entry; a default_bias other than 0 / -inf; a vector
 * with no finite entry; an aligner engine; q3a_beam_begin / q3a_beam_search_batch_ptrs with width larger than the number of finite
 * entries.
 * Readable without debug taps: q3a_debug_read(e, "logit_bias", ..) (fp32 [vocab] as the device holds it, zeros when off) and
 * "logit_bias_stats" (int32 [2]: active 0 / 1, finite entries).
 * Out of scope: per-utterance biases inside one batch (a [S][vocab] operand: 19 MB per step at 32 sequences); multi-token phrase
 * constraints (multi-token sequences: their own section below); a bias inside q3a_score*.  (Sampling, and the history-dependent processors -- repetition penalty, no-repeat n-gram:
 * their own sections below.) */

/* b = default_bias everywhere (0 or -INFINITY only), then b[ids[i]] = bias[i].  n = 0 with default_bias = 0 clears the bias: the
 * engine is back on the launches, ids and log-probabilities of an engine that never had one, bit for bit.  An allow-list is
 * default_bias = -INFINITY with the allowed ids at 0 (the caller lists 151643 / 151645 if generation should be able to stop). */
int32_t q3a_set_logit_bias(q3a_engine* e, const int32_t* ids, const float* bias, int32_t n, float default_bias);
/* Host helper, no engine: parse "id bias" lines ('#' comments, blank lines, "-inf" accepted, "lo-hi bias" ranges with both ends
 * included) and a comma list "id,lo-hi,..." of ids to suppress (bias -inf) into (ids, bias); either may be null or empty.
 * *n = entries needed, at most cap written.  Refused (q3a_last_error(NULL)): a malformed line or item, a NaN / +inf bias, an id
 * named twice. */
int32_t q3a_parse_logit_bias(const char* text, const char* suppress_list, int32_t* ids, float* bias, int32_t cap, int32_t* n);

/* ---- sampling: the next id drawn from softmax(l' / T) inside the decode step ---------------------------------------------------------
 * With temperature T > 0 every step of the GENERATION paths draws its id instead of taking the argmax, on the device, with no logits
 * going to the host.  l' are the (biased) fp32 logits of sequence s at step t; s is the sequence's index in the call and t the number
 * of ids the sequence has generated so far (the device's own step counter: 0 for the id the prefill produces).
 *   Kept set.  K = { j : l'_j >= m + T ln(min_p) }, m = max_j l'_j, the threshold evaluated in fp32.  min_p = 0 keeps every finite
 *     logit; -inf logits are never kept; the maximum always is.  (The "min-p" rule stated on logits: p_j >= min_p p_max at temperature T.)
 *   Noise.  x_j = word 0 of Philox4x32-10 with counter (j, t, s, 0) and key (seed low word, seed high word) = q3a_sample_word(seed, s,
 *     t, j); u_j = ((x_j >> 8) + 0.5) 2^-24, a real number strictly between 0 and 1 (an fp32 number while x_j < 2^31; above, 1 - u_j is
 *     one, and the kernel takes -log u_j from it); g_j = -log(-log u_j).
 *   Choice.  id = argmax over K of z_j = l'_j + T g_j (larger value, then smaller id): Gumbel-max, so id is distributed as softmax(l' / T)
 *     restricted to K.  No division by T; T -> 0 runs continuously into the greedy id.  z_j is evaluated in fp32 (logf, log1pf, one
 *     fma), so an id is specified up to the fp32 error of z: it is the exact arithmetic's best, or, when the exact best two lie closer
 *     than that error, one of those two (DESIGN.md section 3.11 has the measured figure).
 *   Everything downstream is the greedy step's: EOS, done flags, lengths, q3a_fetch_ids, natural EOS, q3a_decode_step, the logit bias.
 *   Log-probabilities (opts.token_logprobs): log_softmax(l')[id], the biased and UNTEMPERED distribution.
 * The noise of a token depends on (seed, s, t, j) alone: a run is reproducible from its seed, graph replay and the stage API draw the
 * same ids, and a reference can reproduce any single entry.  Because s is the index in the call, a clip sampled alone and the same
 * clip inside a batch draw different noise.
 * temperature == 0 turns sampling off: the engine is back on the launches, graphs and ids of one that never sampled.
 * State: the setting persists until changed.  q3a_set_sampling drops the decode state as q3a_set_logit_bias does, so it never changes
 * under a live sequence.  On / off is part of the captured step's signature; temperature, min_p and seed live in a device buffer
 * the kernels read, so changing them replays the same graph.
 * Applies to: q3a_prefill (next_ids), q3a_decode_step, q3a_run_resident, q3a_transcribe_batch[_ptrs], q3a_fetch_logprobs.  While it
 * is on, every lm_head form stores its logits and the one-sequence pruned argmax is not taken.
 * Refused (q3a_last_error): a negative, NaN or infinite temperature; min_p outside [0, 1]; an aligner engine; q3a_beam_begin /
 * q3a_beam_search_batch_ptrs while sampling is on.  q3a_score* and q3a_align* never see it.
 * Readable: q3a_debug_read(e, "sampling", ..) (uint32 [5]: on 0 / 1, temperature and min_p as fp32 bits, seed low, seed high).
 * Out of scope: sampling inside beam search; a group-level call (set it on each q3a_group_engine handle).  (Top-k / top-p: their own
 * section below.) */
int32_t q3a_set_sampling(q3a_engine* e, float temperature, float min_p, uint64_t seed);
/* Host function, no engine and no device: the random word of token j of sequence s at step t, by the code the kernel runs. */
uint32_t q3a_sample_word(uint64_t seed, uint32_t s, uint32_t t, uint32_t j);
/* The sampler's kernels on their own (no model): logits [S][V] host fp32, every sequence at step `step` -> out_ids [S], out_lp [S]
 * (log_softmax(l)[id]) and out_z [S] (the winning noisy score z_id); any may be null.  temperature > 0. */
int32_t q3a_selftest_sample(int32_t device, const float* logits, int32_t S, int32_t V, float temperature, float min_p,
                            uint64_t seed, int32_t step, int32_t* out_ids, float* out_lp, float* out_z);

/* ---- sampling filter: top-k and top-p (nucleus) inside the sampled step ----------------------------------------------------------------
 * The two warpers a generate() user reaches for first, applied on the device between the sampler's row statistics and its draw.  All
 * else is the sampling section's: l' are the stored (biased, sequence-biased, repetition-processed) fp32 logits of sequence s at a
 * step, m their maximum, T > 0 the temperature.  NaN is outside the contract, as everywhere.
 *   Kept set.  K = { j : l'_j >= tau, l'_j != -inf }, tau = max(tau_k, tau_p, tau_minp).  The threshold is a VALUE, never a rank: equal
 *     values share their fate, and -0.0 and +0.0 are equal values.
 *   Top-k.  top_k = 0 or top_k >= V is off (tau_k = -inf).  Otherwise tau_k is the top_k-th largest entry of the row, counted with
 *     multiplicity, so every entry that ties the k-th value is kept (HuggingFace's scores < topk(scores, k)[0][..., -1]); with fewer
 *     than top_k finite entries every finite entry is kept.  Integer counts only: exact, bit for bit.
 *   Top-p.  top_p = 1 is off.  Otherwise, with K_k = { l' >= tau_k }, w_j = exp((l'_j - m) / T) on K_k, Z = sum w and G(v) = sum over
 *     { j in K_k : l'_j > v } of w_j / Z -- the probability mass strictly above the value v, renormalised over the top-k set at
 *     temperature T -- tau_p is the smallest row value v with G(v) < top_p.  The row maximum always qualifies (G = 0).
 *   Min-p.  tau_minp = m + T ln(min_p), as in the sampling section; a ratio to the maximum, so it commutes with the other two.
 *   Pinned meaning.  On tie-free rows K is exactly what HuggingFace's chain TemperatureLogitsWarper(T) -> TopKLogitsWarper(k) ->
 *     TopPLogitsWarper(p) -> MinPLogitsWarper(min_p) leaves finite.  On ties HuggingFace's top-p cuts inside a run of equal values in
 *     sort order; here the whole run is kept.
 *   Tolerance.  Top-k is exact.  Top-p compares a sum of weights with top_p Z, so membership is specified up to a bound delta on
 *     |G_device - G_exact|: tau_ref(top_p + delta) <= tau <= tau_ref(top_p - delta), the reference in float64, with delta = 1e-5.
 *     Derivation, from the arithmetic: a weight is (uint64)(expf((l' - m) / T) 2^40), summed in integers.  A weight that does not
 *     truncate to zero has |(l' - m) / T| < 28; the subtraction and the division each round once (2^-24 relative), so the argument
 *     is off by at most 28 2^-23 = 3.4e-6, expf adds 2 ulp = 2.4e-7: a relative error of at most 3.6e-6 per weight.  Truncation
 *     loses under 2^-40 per entry, under 2^17.2 2^-40 = 1.4e-7 of Z >= 1 over a row.  G is a ratio of two such sums: at most twice
 *     the sum of the two, 7.5e-6; top_p Z itself is formed in fp64 (2^-53).  Rounded up: 1e-5.
 *   The draw is unchanged: Gumbel-max over K with the same Philox words, so the id is distributed as the renormalised HuggingFace
 *     distribution.  Log-probabilities stay those of the untempered l'.
 *   Determinism.  tau, the kept count and the ids are bit-identical from run to run, graph replay and eager: counts and weights are
 *     accumulated in integers, whose sums do not depend on the order of arrival.
 * State: the setting persists until changed.  q3a_set_sampling_filter drops the decode state as q3a_set_sampling does.  It has an
 * effect only while sampling is on: with temperature == 0 the engine runs the greedy launches whatever the filter says, and with
 * (0, 1.0f) the sampled step enqueues exactly what it enqueues without this section.  On / off is part of the captured step's
 * signature; top_k and top_p live in a device buffer the kernels read, so another value replays the same graph.  Buffers are
 * allocated at the first setting that is not off and freed with the engine.  Cost: two launches in the sampled step while on.
 * Refused (q3a_last_error; the engine stays usable): top_k < 0; top_p NaN or outside (0, 1]; an aligner engine.  Beam search, drafts
 * and scoring keep the refusals and the indifference they have towards sampling.
 * Readable without debug taps: q3a_debug_read(e, "sampling_filter", ..) (uint32 [3]: on 0 / 1, top_k, top_p as fp32 bits);
 * "sample_threshold" (fp32 [S]: max(tau_k, tau_p) of the last step, a row value -- a zero as +0.0 -- or -inf) and "sample_kept"
 * (int32 [S]: the entries >= that threshold), both after a step sampled with the filter on.
 * Out of scope: typical / eta / epsilon sampling; min_tokens_to_keep > 1; a filter inside beam search.
 * (per-utterance settings inside one batch: the "row options" section below.) */
int32_t q3a_set_sampling_filter(q3a_engine* e, int32_t top_k, float top_p);   /* (0, 1.0f) = off */
/* q3a_selftest_sample with the filter's threshold stage in it (run twice on one table, the second run handed out); also out_thr [S]
 * (max(tau_k, tau_p)) and out_kept [S] (entries >= it); any output may be null.  (0, 1.0f) gives q3a_selftest_sample's ids and z. */
int32_t q3a_selftest_sample_filter(int32_t device, const float* logits, int32_t S, int32_t V, float temperature, float min_p,
                                   int32_t top_k, float top_p, uint64_t seed, int32_t step, int32_t* out_ids, float* out_lp,
                                   float* out_z, float* out_thr, int32_t* out_kept);

/* ---- repetition: a repetition penalty and a no-repeat n-gram ban inside the decode step ------------------------------------------------
 * The two history-dependent logits processors every generate() user reaches for, applied on the device to the stored logits of every
 * step of the GENERATION paths, between the lm_head and the choice of the id.  l' are the (biased) fp32 logits of sequence s at a step.
 *   History.  t = min(step_count[s], max_new), h = out_ids[s][0 .. t): exactly the ids q3a_fetch_ids would return so far, a stored EOS
 *     included when fixed_new_tokens runs past it.  The prompt (audio pads and a chat template) is not history.  A token forced with
 *     q3a_set_next_tokens is not history either: it replaces the next step's input, not out_ids.
 *   Penalty p.  For every distinct id j in h: l''_j = l'_j / p if l'_j > 0, else l'_j * p -- one correctly rounded fp32 operation.  An id
 *     that occurred k times is penalised once; -inf stays -inf and 0 stays 0.
 *   No-repeat n-gram n >= 1.  Only when t >= n - 1: for every i in [0, t - n + 1) with h[i + k] == h[t - n + 1 + k] for all k in
 *     [0, n - 1), l''_{h[i + n - 1]} = -inf.  n = 1 bans every id already emitted.  The ban is applied after the penalty and wins.
 *   Pinned meaning: bit for bit what HuggingFace's RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor compute on
 *     input_ids = h.
 *   Everything downstream is defined on l'' by the rules it already has: the greedy id is argmax l'' (larger value, then smaller id);
 *     sampling draws from l'' (kept set, noise and Gumbel-max unchanged); token log-probabilities are log_softmax(l'')[id]; logits_out
 *     of q3a_prefill / q3a_decode_step and the "logits" tap hold l''.  At t = 0 (the id the prefill produces) both are the identity.
 * repetition_penalty == 1 and no_repeat_ngram_size == 0 is off: the engine is back on the launches, graphs, ids, log-probabilities
 * and pruned-pass counts of one that never had the setting.
 * State: the setting persists until changed.  q3a_set_repetition drops the decode state as q3a_set_sampling does.  On / off is part of
 * the captured step's signature; p and n live in a 16-byte device buffer the kernel reads, so another setting replays the same graph.
 * Applies to: q3a_prefill (next_ids, last_logits_out), q3a_decode_step, q3a_run_resident, q3a_transcribe_batch[_ptrs],
 * q3a_fetch_logprobs.  While it is on, every lm_head form stores its logits and the one-sequence pruned argmax is not taken.
 * Group runs: set it on each q3a_group_engine handle.  q3a_score* and q3a_align* never see it: bit-identical with it on and off.
 * Refused (q3a_last_error): a repetition_penalty that is not finite or <= 0; no_repeat_ngram_size < 0 or > 32; an aligner engine;
 * q3a_beam_begin / q3a_beam_search_batch_ptrs while it is on (beam slots reorder their histories); a vocabulary above the 262144 ids
 * the kernel's bitmap holds (151936 fits); no_repeat_ngram_size > 0 together with a logit bias that leaves both EOS ids at -inf and no
 * more finite entries than max_new_tokens -- the only way a row could run out of finite logits -- refused by whichever of
 * q3a_set_repetition / q3a_set_logit_bias comes second.  (Not refused: with fixed_new_tokens running past a stored EOS the EOS id is
 * history like any other, so an n-gram ban over a small allow-list with an EOS id open can still empty a row AFTER the sequence's EOS;
 * the ids and log-probabilities (NaN) of a sequence behind its EOS are unspecified in that combination, those up to it are not touched.)
 * Readable: q3a_debug_read(e, "repetition", ..) (uint32 [3]: on 0 / 1, repetition_penalty as fp32 bits, no_repeat_ngram_size).
 * Out of scope: penalties over the prompt; frequency / presence penalties; a history window; repetition control inside beam search;
 * keeping the one-sequence pruned argmax under it (exact only for p >= 1, and it would need a device-side branch when the pruned
 * winner is a seen id). */
int32_t q3a_set_repetition(q3a_engine* e, float repetition_penalty, int32_t no_repeat_ngram_size);
/* The kernel on its own (no model), followed by the argmax partials and their merge as the engine enqueues them: logits [S][V] host
 * fp32, hist [S][stride] with lens [S] ids of history each (0 <= lens[s] <= stride, every id inside the vocabulary) -> out_logits
 * [S][V] (l''), out_ids [S] (argmax l'') and out_lp [S] (log_softmax(l'')[id]); any of the three may be null. */
int32_t q3a_selftest_repeat(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride,
                            const int32_t* lens, float p, int32_t n, float* out_logits, int32_t* out_ids, float* out_lp);

/* ---- sequence bias: hotword boosts and banned phrases inside the decode step -------------------------------------------------------------
 * The multi-token constraint of generate(): a list of (token sequence, bias) pairs, the bias added to the sequence's last token
 * whenever the ids generated so far end in the rest of the sequence -- applied on the device to the stored logits of every step of the
 * GENERATION paths, between the lm_head and the choice of the id.  A banned phrase is an entry with a bias of -inf; a hotword boost is
 * an entry for every prefix of the phrase (q3a_hotword_sequences).  An engine holds a list of E entries; an entry is a token sequence
 * q_0 .. q_{L-1} with 1 <= L <= 32 and a bias that is finite or -inf.  l' are the (biased) fp32 logits of sequence s at a step.
 *   History.  t = min(step_count[s], max_new), h = out_ids[s][0 .. t): the same words and the same exclusions as in the repetition
 *     section.  The prompt is not history.  A token forced with q3a_set_next_tokens is not history.
 *   Firing.  An entry of length L fires on a row iff t >= L - 1 and h[t - L + 1 .. t) equals q_0 .. q_{L-2}.  A one-token entry
 *     always fires, also at t = 0, which is the id the prefill produces.
 *   Sum.  For a target id v, the entries are those whose last token is v.  acc = 0.0f; the bias of the one-token entry on v is added
 *     first, if there is one (it fires); then the bias of each longer firing entry, in the order the caller gave them; each addition is
 *     one fp32 add.  If at least one entry fired, l''_v = l'_v + acc, one more fp32 add.  Ids that no entry fired on are not touched.
 *     -inf stays -inf and never yields NaN: +inf and NaN biases are refused.
 *   Pinned meaning: for every entry that fires or could fire, bit for bit what HuggingFace's
 *     SequenceBiasLogitsProcessor(sequence_bias = the entries as a dict in the caller's order) computes on input_ids = [x] ++ h for an
 *     arbitrary id x.  The one extra column in front removes HuggingFace's len(sequence) > context quirk, which ignores an L-token
 *     sequence at t = L - 1; here the sequence fires.  NoBadWordsLogitsProcessor is the same processor with every bias -inf.  One
 *     exception: a logit of -0.0 that nothing fired on stays -0.0, where HuggingFace's scores + 0 turns it into +0.0.
 *   Order with the other processors: logit bias (inside the head), sequence bias, repetition penalty, n-gram ban, then argmax or
 *     sampler -- HuggingFace's generate() order for finite biases; a -inf is invariant under the penalty and the ban, so the bad-words
 *     use gives the same row wherever it stands.
 *   Everything downstream is defined on l'' by the rules it already has: the greedy id is the larger value, then the smaller id; the
 *     sampler's kept set and noise; q3a_fetch_logprobs = log_softmax(l'')[id]; logits_out of q3a_prefill / q3a_decode_step and the
 *     "logits" tap hold l''.
 * An empty list (n = 0) is off: the engine is back on the launches, graphs, ids, log-probabilities and pruned-pass counts of one that
 * never had the setting.  While it is on, every lm_head form stores its logits and the one-sequence pruned argmax is not taken, as
 * under repetition control.
 * State: the list persists until changed.  q3a_set_sequence_bias drops the decode state as q3a_set_repetition does.  On / off is part
 * of the captured step's signature; the tables and their counts live in a device buffer of fixed capacity that the kernel reads, so
 * another list replays the same graph.  The buffer is allocated at the first non-empty set and freed with the engine: "device_bytes"
 * is level across set / clear cycles after the first.
 * Applies to: q3a_prefill (next_ids, last_logits_out), q3a_decode_step, q3a_run_resident, q3a_transcribe_batch[_ptrs],
 * q3a_fetch_logprobs.  Group runs: set it on each q3a_group_engine handle.  q3a_score* and q3a_align* never see it: bit-identical
 * with it on and off.
 * Limits: E <= 4096; L <= 32; at most 65536 ids over all entries.
 * Refused (q3a_last_error; the engine stays usable): an id < 0 or >= vocab; an empty sequence, or L > 32; more entries or ids than
 * the limits; the same sequence twice; a NaN or +inf bias; an aligner engine; q3a_beam_begin / q3a_beam_search_batch_ptrs while it is
 * on (beam slots reorder their histories); q3a_prefill_draft / q3a_transcribe_draft_batch_ptrs while it is on (the choice is not an
 * argmax of the row alone); a -inf entry together with an allow-list logit bias (default_bias -inf) whose finite entries are no more
 * than the distinct targets of -inf entries plus, with an n-gram ban on, max_new_tokens -- the only way a row could run out of finite
 * logits -- refused by whichever of q3a_set_sequence_bias / q3a_set_logit_bias / q3a_set_repetition comes second.
 * Readable: q3a_debug_read(e, "sequence_bias", ..) (int32 [4]: on 0 / 1, entries, ids over all entries, distinct targets).
 * (per-utterance lists inside one batch: q3a_set_sequence_bias_lists in the "row options" section below.)
 * Out of scope: subtracting a partial boost when a phrase is abandoned; sequence bias inside
 * beam search or under a draft (so not in StreamingTranscriber); matching over the prompt; boost values tuned on real weights (none
 * has been: q3a_hotword_sequences takes the boost from the caller). */

/* ids: the entries' ids one after the other (sum of lens), lens [n], bias [n].  n = 0 clears the list. */
int32_t q3a_set_sequence_bias(q3a_engine* e, const int32_t* ids, const int32_t* lens, const float* bias, int32_t n);
/* The kernel on its own (no model), followed by the argmax partials and their merge as the engine enqueues them: logits [S][V] host
 * fp32, hist [S][stride] with lens [S] ids of history each (0 <= lens[s] <= stride, every id inside the vocabulary), the list as
 * q3a_set_sequence_bias takes it -> out_logits [S][V] (l''), out_ids [S] (argmax l'') and out_lp [S] (log_softmax(l'')[id]); any of
 * the three may be null.  The arguments are validated before a device is looked for. */
int32_t q3a_selftest_seqbias(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride, const int32_t* lens,
                             const int32_t* seq_ids, const int32_t* seq_lens, const float* seq_bias, int32_t n, float* out_logits,
                             int32_t* out_ids, float* out_lp);
/* Host helpers, no engine.  All three return a list as q3a_set_sequence_bias takes it: *n_ids / *n = ids and entries needed; ids
 * [ids_cap], lens [cap] and bias [cap] are written only when both capacities hold the whole list (call once with 0 / 0 to size).
 * q3a_parse_sequence_bias: lines "bias id id ..." ('#' comments, blank lines, "-inf" accepted).  Refused (q3a_last_error(NULL)): a
 *   malformed line, a NaN / +inf bias, more than 32 ids on a line, a sequence given twice.
 * q3a_hotword_sequences: for each phrase both tokenisations, encode(phrase) and encode(" " + phrase); for each tokenisation
 *   p_0 .. p_{L-1} the entries (p_0 .. p_j), j = 1 .. L-1, with bias `boost`, and, when start_boost != 0, also (p_0) with start_boost
 *   (so a phrase that is ONE token is boosted by start_boost alone).  Equal sequences are merged, keeping the larger bias.  A phrase
 *   whose tokenisation exceeds 32 ids is refused by name; so are an empty phrase and a boost that is not finite.
 * q3a_banned_sequences: both tokenisations of each phrase, whole, at -inf. */
int32_t q3a_parse_sequence_bias(const char* text, int32_t* ids, int32_t ids_cap, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n);
int32_t q3a_hotword_sequences(const q3a_tokenizer* t, const char* const* phrases, int32_t n_phrases, float boost, float start_boost, int32_t* ids,
                              int32_t ids_cap, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n);
int32_t q3a_banned_sequences(const q3a_tokenizer* t, const char* const* phrases, int32_t n_phrases, int32_t* ids, int32_t ids_cap, int32_t* lens,
                             float* bias, int32_t cap, int32_t* n_ids, int32_t* n);

/* ---- row options: per-request decoding options inside one batch, read per row on the device -----------------------------------------
 * A ROW TABLE gives sequence s of the next calls its own record of the settings the sections above hold once per engine: sampling,
 * the sampling filter, repetition control and the sequence-bias list.  s is the index of the sequence in the batch, the same one that
 * seeds the Philox counter.  A server can so put one caller's hotword list, another's temperature 0.8 / top_p 0.9 and a third's plain
 * greedy request into one batch.
 *   Row meaning.  Row s behaves exactly as the sections above define for an engine whose uniform setting is that row's record: the kept
 *     set, the noise q3a_sample_word(seed_s, s, t, j), Gumbel-max, the tau rules, the penalty and the n-gram ban over the row's own
 *     out_ids, the firing and summing rule of the row's own list, the processor order (sequence bias, repetition, then the choice), and
 *     log-probabilities taken from the untempered l''.  Nothing there is redefined: params becomes params[s].
 *   A greedy row (temperature 0) inside a step that samples another row: its id is the argmax of its l'' (larger value, then smaller
 *     id) -- no noise, no filter, no division by T; "sample_threshold" reads -inf and "sample_kept" the count of finite entries; its
 *     log-probability is log_softmax(l'')[id] from the sampler's row statistics; the id equals the id a never-sampling engine writes.
 *   Rows that have nothing on.  (top_k, top_p) = (0, 1.0f) in a step where another row filters: tau = -inf, id and noisy score are the
 *     bits of the unfiltered sampler.  (repetition_penalty, no_repeat_ngram_size) = (1.0f, 0): the repetition launch leaves the row
 *     untouched.  sequence_list = -1: the sequence-bias launch leaves the row untouched.
 *   Lists.  q3a_set_sequence_bias_lists uploads up to 256 lists, entries as q3a_set_sequence_bias takes them, list after list;
 *     q3a_set_sequence_bias is the case of one list, and without a row table every row uses list 0 (so nothing changes for it).  The
 *     limits are totals over all lists: E <= 4096 entries, 65536 ids, L <= 32.  The same sequence twice is refused within a list and
 *     allowed across lists.  A target's group belongs to one list; the groups of a list are contiguous, and a directory of 257 words
 *     behind the tables names each list's range.
 *   State.  The table persists until cleared (n_rows = 0) or replaced; setting it drops the decode state, as every setter here does.
 *     The uniform setters keep working while a table is set: their values are remembered, not read, and are in force again when the
 *     table is cleared.  q3a_debug_read "sampling" / "sampling_filter" / "repetition" / "sequence_bias" keep their meaning (the uniform
 *     values; "sequence_bias" counts over all lists); "row_options" returns the table as uploaded (n_rows records, nothing while clear).
 *   Graph signature.  The switches sampling / filter / repetition / sequence bias are evaluated over ANY row, and one more says
 *     whether a table is present.  The records live in a device buffer of [4][n_rows][4] words that the kernels read with a row stride
 *     of 4 words instead of 0, so another table of the same switches replays the same graph.  With the table cleared the engine is back
 *     on the launches, graphs, ids, log-probability bits and pruned-pass counts it had without one; "device_bytes" is level across
 *     set / clear cycles after the first.
 *   Cost.  A greedy row in a batch where any row samples pays the sampled step (its row is read by the sampler's launches).
 * Refused (q3a_last_error; the engine stays usable): every value the uniform setters refuse, reported with the row index; a
 * sequence_list outside [-1, n_lists), by whichever of the two setters comes second; n_rows < 0; an aligner engine; a prefill whose
 * batch differs from n_rows (q3a_prefill, q3a_run_resident, q3a_transcribe_batch[_ptrs], the draft and beam entry points); beam search
 * and draft verification while any row has something on (the refusals they have towards the uniform settings); the two
 * run-out-of-finite-logits rules of the repetition and sequence-bias sections, applied per row with that row's n-gram size and the
 * -inf targets of that row's list.  q3a_score* and q3a_align* never see the table: bit-identical with it set and cleared.
 * Out of scope: logit-bias vectors per row (a [S][vocab] operand, see the logit-bias section); a forced language per row
 * (lang_prefix_ids stays one per call); per-row max_new_tokens; temperature fallback inside a batched call; q3a_group_* (set the
 * table on each q3a_group_engine handle); a Philox row index other than s. */
typedef struct q3a_row_options {
  float    temperature;          /* 0: this row takes the argmax (larger value, then smaller id) */
  float    min_p;                /* [0, 1] */
  uint64_t seed;
  int32_t  top_k;  float top_p;  /* (0, 1.0f): no filter on this row */
  float    repetition_penalty;   /* (1.0f, 0): identity on this row */
  int32_t  no_repeat_ngram_size;
  int32_t  sequence_list;        /* -1: none; else an index into the engine's sequence-bias lists */
} q3a_row_options;
int32_t q3a_set_row_options(q3a_engine* e, const q3a_row_options* rows, int32_t n_rows);   /* n_rows = 0 clears the table */
/* entries as q3a_set_sequence_bias takes them, list after list: list_lens[n_lists] entries each.  n_lists = 0 clears. */
int32_t q3a_set_sequence_bias_lists(q3a_engine* e, const int32_t* ids, const int32_t* lens, const float* bias,
                                    const int32_t* list_lens, int32_t n_lists);
/* The chain on its own (no model), in the order the engine enqueues it: sequence bias, repetition, then the sampler (with the filter
 * stage if any row filters; run twice on one table as in q3a_selftest_sample_filter) or -- no row samples -- fresh argmax partials,
 * then argmax_finalize and the log-probability.  logits [S][V], hist [S][stride] with lens [S] ids of history each: row s is at step
 * lens[s].  rows [S] and the lists as the two setters take them.  -> out_logits [S][V] (l''), out_ids, out_lp, out_z (the winning
 * noisy score; l''_id on a greedy row; written only when a row samples), out_thr, out_kept [S] (written only when a row filters); any
 * output may be null.  The arguments are validated before a device is looked for. */
int32_t q3a_selftest_row_options(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride,
                                 const int32_t* lens, const q3a_row_options* rows, const int32_t* seq_ids, const int32_t* seq_lens,
                                 const float* seq_bias, const int32_t* list_lens, int32_t n_lists, float* out_logits, int32_t* out_ids,
                                 float* out_lp, float* out_z, float* out_thr, int32_t* out_kept);

/* ---- top log-probabilities: the n best alternatives of every generated token, selected on the device -------------------------------
 * What the engine nearly wrote: OpenAI's top_logprobs, per-word alternatives.  While n > 0, every step of the GENERATION paths that
 * commits a token -- the prefill's head, which produces the first one, included -- also records the n best entries of that step's
 * final row l'': the row after the logit bias, the sequence bias and repetition control, exactly the row the argmax or the sampler
 * reads.  0 <= n <= 20; 0 is off and the default.  Each entry is (id, lp).
 *   Order.  Larger logit first, then smaller id.  -0.0 and +0.0 are one value.  -inf is a legal logit: it ranks last, ordered by id
 *     among itself, and has lp = -inf.  NaN is outside the contract.  This is the argmax's tie rule, so in a greedy run entry 0 is the
 *     id that was written.
 *   lp.  lp = (l''[v] - m) - log sum exp(l'' - m), m the row maximum, in fp32 with a fixed summation order: the untempered, unfiltered
 *     distribution q3a_fetch_logprobs reports.  Under sampling the drawn id need not be among the entries.  Results are bit-identical
 *     from run to run and between graph replay and the eager step.
 *   Slot.  The entries of the step that wrote out_ids[s][t] stand at [s][t][0 .. n).  A row that is already done, or whose slot is >=
 *     the run's stride (max_new), writes nothing: a finished row's entries do not change afterwards.  With teacher forcing
 *     (q3a_set_next_tokens) they are still each step's own row's best entries.
 *   Fetch.  q3a_fetch_top_logprobs: out_ids / out_lp are host [B][stride][n_stride]; for row b the steps 0 .. min(out_lens[b], stride)
 *     and of each the entries 0 .. min(n, n_stride) are written, everything else is untouched.  out_lens as q3a_fetch_ids gives them.
 *     Works after q3a_run_resident, q3a_transcribe_batch[_ptrs] and the stage API (q3a_prefill / q3a_decode_step).  Refused on an
 *     engine whose last run had n == 0, before anything was generated, and after a setter has dropped the decode state.
 * Independent of opts.token_logprobs.  While it is on, every lm_head form stores its logits and the one-sequence pruned argmax is not
 * taken, as under q3a_set_repetition.  With n == 0 the engine is on the launches, graphs, ids, log-probability bits and pruned-pass
 * counts of one that never had the setting.
 * State: the setting persists until changed; q3a_set_top_logprobs drops the decode state as the other setters do.  On / off is part of
 * the captured step's signature; n lives in a device word and the history has a fixed inner stride of 20, so another n > 0 replays the
 * same graph.  Memory: [B][max_new][20] x (int32 + fp32), allocated by the first prefill under n > 0 and freed with the engine;
 * "device_bytes" is level across set / clear / transcribe cycles after the first.
 * The setting is uniform for the batch; it composes with a row table because it only reads the final row.  Group runs: set it on each
 * q3a_group_engine handle.  q3a_score* and q3a_align* never see it: bit-identical with it on and off.
 * Refused (q3a_last_error; the setting and the engine stay as they were): n outside [0, 20]; n above the vocabulary; an aligner
 * engine; q3a_beam_begin / q3a_beam_search_batch_ptrs, q3a_prefill_draft and q3a_transcribe_draft_batch_ptrs while n > 0 (beam search
 * re-orders rows, and accepted draft tokens never pass the step's head).
 * Readable: q3a_debug_read(e, "top_logprobs", ..) (int32 [1]: n as last set).
 * Out of scope: a per-row n; alternatives inside beam search; more than 20 entries. */
int32_t q3a_set_top_logprobs(q3a_engine* e, int32_t n);
int32_t q3a_fetch_top_logprobs(q3a_engine* e, int32_t* out_ids, float* out_lp, int32_t stride, int32_t n_stride, int32_t* out_lens);
/* The two launches on their own (no model), as the engine enqueues them, TWICE on the same scratch: logits [S][V] host fp32, row s at
 * step step_count[s] with done[s] -> the whole history out_ids / out_lp [S][stride][20] of the second run (ids -1 and lp 0 wherever
 * nothing was written).  1 <= n <= min(20, V).  Fails if the second run differs from the first in any bit. */
int32_t q3a_selftest_top_logprobs(int32_t device, const float* logits, int32_t S, int32_t V, int32_t n, const int32_t* step_count,
                                  const uint8_t* done, int32_t stride, int32_t* out_ids, float* out_lp);

/* A/B knobs for kernel experiments (process-wide atomics, read from the environment once; not part of the reference
 * interface).  The knobs that shape the decode step are latched per batch at the next prefill and are part of the captured
 * graph's signature, so changing one on a live engine re-captures instead of replaying a stale graph.  Keys:
 *   "gemm256_min_tiles"  minimum number of 256x256 output tiles for which the bf16 GEMM dispatches to the 8-wave
 *                        counted-vmcnt kernel (k_gemm256.hip): 0 = whenever the shape allows, a huge value = never.
 *   "gemm256_persist"    1 (default): a gemm256 launch is min(tiles, CUs) workgroups that walk the tiles of their XCD's chunk, the next
 *                        tile's first K tile arriving under the epilogue; 0: one workgroup per tile; n > 1: a walk of exactly n workgroups (tests).
 *                        Same arithmetic: bit-identical.
 *   "gemm256_group_m"    gemm256's tile order: groups of this many tile rows, M fastest inside a group (1 = N fastest over the whole
 *                        matrix; 0, the default = 8 where the matrix is at least 8 tiles wide, else 1).  The same tiles assigned to other workgroups: bit-identical.
 *   "dattn_batched_min_wgs"  sequences x kv heads of a decode group from which the batched decode step uses the
 *                        one-workgroup-per-(sequence, kv head) attention kernel (k_dattn.hip) instead of key splits + merge.
 *   "decode_group_size"  sequences per group of the batched decode step (1..32; 0 = 32), taken at the next prefill.
 *   "decode_parallel_groups"  1: groups run as parallel stream / hipGraph branches (default), 0: one after the other.
 *   "fuse_qkrope"        1 (default): batch-sized prefills run QK-norm + RoPE + the KV-cache append as the epilogue of the qkv
 *                        GEMM; 0: as the separate kernel (taken at the next prefill).
 *   "skinny_q"           1 (default): o / down projections of the batched decode step as 8-row x 16-sequence workgroups;
 *                        0: 16 rows x 32 sequences (taken at the next engine / batch set-up: it sizes a buffer).
 *   "eos_run_ahead"      decode steps the natural-EOS greedy loop keeps enqueued ahead of the device (default 1): the stop
 *                        condition is evaluated on the device and read from pinned host memory without synchronising.
 *   "skinny_glu_hp3"     1 (default): when the gate/up projection of the batched decode step has more 32-row pair tiles than the GPU has
 *                        CUs and its output columns divide into 3 half-pair tiles (8 gate + 8 up rows in one MFMA fragment) per
 *                        workgroup with at most one workgroup per CU (hidden 2048 / inter 6144: 256 workgroups), it runs in that
 *                        form: every CU streams the same number of weight bytes and the activations once; 0: never; 2: whenever
 *                        the shape allows (tests).  Same arithmetic.  Taken at the next prefill.
 *   "lm_head_prune"      1 (default): the argmax of a one-sequence decode step whose logits nobody reads comes from an int8 pre-pass
 *                        over the lm_head (approximate logits with a rigorous error bound) and a bf16 rescore of the 16-row blocks
 *                        that can still hold the maximum: the ids are bit-identical to 0, the full bf16 GEMV.  Taken at the next
 *                        batch set-up.
 *   "oproj_by_head"      1 (default): the one-sequence decode step of the default mode (hidden size <= 1024, kv heads of two q heads)
 *                        runs o_proj per pair of kv heads -- partial vectors that the gate / up projection adds to the residual -- and
 *                        decode attention in 32-key splits up to 512 keys of context, 64-key splits up to 1024, 128-key splits up
 *                        to 2048; 0: the o_proj that merges the whole context and 128-key splits, which longer contexts, the
 *                        precise mode and every other shape run anyway.  Same sums in another fp32 order.  Taken at the next
 *                        batch set-up.
 *   "layer_taps"         (debug aid) 1: an engine created with debug taps also keeps raw copies of every encoder / decoder
 *                        prefill layer's intermediate buffers (taps "E%02d_x", "L%02d_ln1" / "_q" (default mode) / "_k" / "_v" /
 *                        "_attn" / "_o" / "_ln2" / "_act" / "_x"; the environment's Q3A_DEBUG_LAYER_TAPS=1 sets it).  Taken at the
 *                        next prefill.
 *   "poison_attn_partials"  (debug aid) 1: every batch set-up fills the decode attention's split statistics and partial outputs
 *                        with 0xFF bytes (NaN), so that a merge reading an entry no attention launch wrote shows up.
 * Round 6 removed the keys whose A/B is settled, together with the code only they selected (docs/HISTORY.md "Pruned in round 6"):
 * fuse_qkv_attn, dattn_pair_split, fattn_pipe, rope_variant, rope_twice, gemm16_ring, gemm256_resid_prefetch, live_key_splits,
 * skinny_glu_2pass.  An unknown key returns non-zero. */
int32_t q3a_debug_set(const char* key, int32_t value);

/* Kernel self-tests against naive device references (no model needed): returns max abs error. */
int32_t q3a_selftest_gemm(int32_t device, int32_t M, int32_t N, int32_t K, int32_t split, float* max_abs_err,
                          float* ref_abs_max);
/* Same for the bf16-activation GEMM (global_load_lds path); with reps > 0 also the average launch time of it and
 * of the fp32-activation kernel on the same shape (HIP events around `reps` back-to-back launches). */
int32_t q3a_selftest_gemm16(int32_t device, int32_t M, int32_t N, int32_t K, int32_t reps, float* max_abs_err,
                            float* ref_abs_max, float* avg_us_bf16, float* avg_us_f32);

/* ONE launch of the GEMM family on the caller's data (no model, no reference arithmetic in the library: tests/gemm_ref.py compares in
 * float64).  Every output buffer is the caller's: pre-filled with a sentinel, uploaded, written by the launch, returned whole -- so rows a
 * row map drops, columns N..ldo, rows past M and cache rows no token names are visible.  On the device each output sits between guard
 * zones; a changed guard byte fails the call.  Arguments the launch could index out of bounds with are refused before anything runs.
 *   launcher  0 launch_gemm, 1 launch_gemm16 (with its dispatch to gemm256), 2 launch_gemm16_small, 3 launch_conv3x3s2_gemm,
 *             4 launch_conv3x3s2_gemm16 (with its dispatch); 0 / 3 take fp32 x, the others bf16 bit patterns
 *   flags     1 split (hi + lo activations; launchers 0 / 3), 2 GLU ([16 gate | 16 up] row blocks of w, N / 2 output columns),
 *             4 out is bf16 [out_rows][ldo] instead of fp32, 8 the residual IS the output buffer (resid null; fp32 output)
 *   x         dense [M][lda]; convolution NHWC [imgs][H][Wd][C], M = imgs * OH * OW, K = 9 * C ordered (kh, kw, c), N = Cout
 *   w         bf16 [N][K];  bias [N], addend [addend_period][ldo], resid [out_rows][ldo], rowmap [M] (negative: dropped) -- each nullable
 *   act       0 none, 1 GELU */
int32_t q3a_selftest_gemm_launch(int32_t device, int32_t launcher, int32_t flags, const void* x, const uint16_t* w, int32_t M, int32_t N, int32_t K,
                                 int32_t lda, int32_t ldo, int32_t imgs, int32_t H, int32_t Wd, int32_t C, const float* bias, const float* addend,
                                 int32_t addend_period, const float* resid, const int32_t* rowmap, int32_t act, void* out, int32_t out_rows);
/* The same for per-head QK-norm + RoPE + KV-cache append.  fused = 1: launch_gemm256_qkrope on bf16 x [M][lda], w [(n_q + 2 n_kv) * 128][K]
 * and a nullable bias; q16 and a bf16 cache required; qkv nullable fp32 [M][N] scratch (with it the launch may split off its trailing
 * rows, see q3a_gemm256_split_rows).  fused = 0: launch_qknorm_rope_kv on fp32 qkv [M][N] (x, w, bias null); q is written to q16 when
 * given, else in place; kv_f32 selects an fp32 cache.  row_seq / row_pos [M], q_norm / k_norm [128], cos_t / sin_t [max_pos][64],
 * kcache / vcache [n_seq][n_kv][max_ctx][128].  Outputs (qkv, q16, kcache, vcache) as above: sentinel in, whole buffer out. */
int32_t q3a_selftest_qkrope_launch(int32_t device, int32_t fused, int32_t kv_f32, const uint16_t* x, int32_t lda, const uint16_t* w, int32_t M, int32_t K,
                                   const float* bias, float* qkv, const int32_t* row_seq, const int32_t* row_pos, const float* q_norm,
                                   const float* k_norm, float eps, const float* cos_t, const float* sin_t, int32_t max_pos, int32_t n_q, int32_t n_kv,
                                   int32_t n_seq, int32_t max_ctx, uint16_t* q16, void* kcache, void* vcache);
/* ONE launch of the one-sequence GEMV family on the caller's data, in the precise arithmetic (fast_math = 0, attn_fast_exp = 0), as
 * q3a_selftest_gemm_launch: tests/decode_kernels_ref.py compares in float64.  w bf16 [N][K]; x [K] fp32, or -- x and rms_w null -- the
 * flash-decoding partials attn_pm / attn_pl [heads][nsplit] and attn_po [heads][nsplit][128] with K = heads * 128, merged on the fly.
 * rms_w [K] (nullable) fuses the RMSNorm with eps; bias [N] nullable; mode 0 store, 1 out = resid + y (resid [N]), 2 GLU (N / 2 outputs),
 * 3 the lm_head: launch_gemv (pruned = 0) or the int8 pre-pass + rescore pair (pruned = 1, out null), then argmax_finalize at step 2 of a
 * 4-step sequence at position 5: out_state = {next token, out_ids[2], step count, position} after it.  out (sentinel in, whole buffer
 * out, guard zones on the device) is [N] ([N / 2] in mode 2), nullable in mode 3. */
int32_t q3a_selftest_gemv_launch(int32_t device, int32_t pruned, const uint16_t* w, int32_t N, int32_t K, const float* x, const float* rms_w, float eps,
                                 const float* bias, int32_t mode, const float* resid, const float* attn_pm, const float* attn_pl, const float* attn_po,
                                 int32_t attn_nsplit, int32_t attn_heads, float* out, int32_t* out_state);
/* The same for launch_decode_attn at one sequence: qkv [(n_q + 2 n_kv) * 128] raw projections of the token at position pos, q_norm / k_norm
 * [128], rope_cur [128] = cos (64) | sin (64) of pos, kcache / vcache [n_kv][max_ctx][128] (bf16 bits, or fp32 with kv_f32: the precise
 * exponential) holding rows 0 .. pos - 1.  Outputs, each sentinel in / whole buffer out: the caches (row pos appended), pm / pl
 * [n_q][nsplit], po [n_q][nsplit][128]. */
int32_t q3a_selftest_decode_attn_launch(int32_t device, int32_t kv_f32, const float* qkv, int32_t pos, const float* q_norm, const float* k_norm, float eps,
                                        const float* rope_cur, void* kcache, void* vcache, int32_t n_q, int32_t n_kv, int32_t max_ctx, int32_t nsplit,
                                        float scale_div, float* pm, float* pl, float* po);
/* The same launch with the split size given: keys_per_split 32 or 64 (bf16 cache, kv heads of at most two q heads: 4 waves per
 * workgroup), 128, or 0 for the default; nsplit splits of that size, every one of them written. */
int32_t q3a_selftest_decode_attn_split_launch(int32_t device, int32_t kv_f32, int32_t keys_per_split, const float* qkv, int32_t pos, const float* q_norm,
                                              const float* k_norm, float eps, const float* rope_cur, void* kcache, void* vcache, int32_t n_q, int32_t n_kv,
                                              int32_t max_ctx, int32_t nsplit, float scale_div, float* pm, float* pl, float* po);
/* ONE launch of the o_proj per pair of kv heads (launch_oproj_head; the default arithmetic: hardware exponential in the merge): w bf16 [N][K],
 * K = attn_heads * 128 = n_parts * 512, the flash-decoding partials as in q3a_selftest_gemv_launch with attn_nsplit <= 16 (more is
 * refused with a message, nothing is launched), bias [N] nullable (added to slice 0).  y_part [n_parts][N] (sentinel in, whole buffer
 * out): the dot products of each 512-column slice with the merged context, no residual. */
int32_t q3a_selftest_oproj_head_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, const float* bias, const float* attn_pm, const float* attn_pl,
                                       const float* attn_po, int32_t attn_nsplit, int32_t attn_heads, int32_t n_parts, float* y_part);
/* ONE launch of the gate / up GEMV that adds partial vectors to its input (launch_gemv with GemvArgs::x_parts; precise arithmetic):
 * GLU of w bf16 [N][K], K <= 1024, on the RMSNorm (rms_w [K], eps) of x + x_parts[0] + ... + x_parts[n_parts - 1] (x [K], x_parts
 * [n_parts][K], n_parts <= 4), bias [N] nullable.  out [N / 2] and x_out [K], the summed vector as the launch stores it (sentinel in,
 * whole buffer out). */
int32_t q3a_selftest_gemv_parts_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, const float* x, const float* rms_w, float eps,
                                       const float* bias, const float* x_parts, int32_t n_parts, float* out, float* x_out);
/* ONE launch_skinny call (the batched decode step's GEMM, 1 .. 32 sequences; skinny_init() first) on the caller's data, as
 * q3a_selftest_gemm_launch: tests/batched_decode_ref.py compares in float64.  w bf16 [N][K], K % 32 == 0, K <= 6144.  The x source is exactly
 * one of: x fp32 [S][ldx] with rms_w [K] (fused RMSNorm with eps) or without; x16 bf16 row-major [S][ldx] or, with x16_frag, in fragment
 * order; xw16f (pre-normalised, fragment order) with ss_parts [ss_nparts][32].  A buffer in fragment order holds 32 sequences: the caller
 * gives all 32 * K elements (32 * cols rounded up to whole 32-column steps for an output), so the slots of sequences >= S are its own, as
 * are the ss_parts columns >= S.  On the device fp32 x and rms_w go on past their end with NaN.  bias [N] nullable; mode 0 store, 1 out =
 * resid + y (resid [S][ldo]), 2 GLU (N / 2 output columns).  Outputs, each sentinel in / whole buffer out between guard zones: out fp32
 * [32][ldo] (rows >= S stay the caller's), or in mode 2 out16 bf16 [32][ldo] / fragment order (out16_frag); with next_w [N] (mode 1) also next_xw16f (fragment order) and
 * next_ss [N / 16 rounded up, or N / 8 with quarter workgroups][32].  flags: 1 split (hi + lo activations), 2 fast_math, 4 qsplit (quarter
 * workgroups), 8 in place (resid null: the residual is what out holds, one device buffer for both, as the engine calls it).  glu_hp3 and
 * n_cu as SkinnyArgs.  form [11] receives the instantiation that ran: split, TILES, SH, XMODE, UNR, WLDS, QS, PALIAS, HP, grid size, dynamic
 * LDS bytes. */
int32_t q3a_selftest_skinny_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, int32_t S, const float* x, int32_t ldx, const float* rms_w,
                                   const uint16_t* x16, int32_t x16_frag, const uint16_t* xw16f, const float* ss_parts, int32_t ss_nparts, float eps,
                                   const float* bias, int32_t mode, const float* resid, float* out, uint16_t* out16, int32_t out16_frag, int32_t ldo,
                                   const float* next_w, uint16_t* next_xw16f, float* next_ss, int32_t flags, int32_t glu_hp3, int32_t n_cu,
                                   int32_t* form);
/* The decode attention of S sequences with ragged pos [S]: launch_decode_attn_batched (split_path = 0, trim_prologue given), or
 * launch_decode_attn with nsplit splits of keys_per_split keys (0: the default) followed by launch_attn_combine (split_path = 1).  qkv
 * [S][(n_q + 2 n_kv) * 128], rope_cur [S][128], kcache / vcache [S][n_kv][max_ctx][128] (bf16 bits, or fp32 with kv_f32).  out_form 0: out
 * fp32 [S][n_q * 128]; 1: bf16 row-major; 2: bf16 in fragment order (32 sequences' room; more than 32 sequences are refused).  Outputs,
 * each sentinel in / whole buffer out: the caches, out, and on the split path pm / pl [S][n_q][nsplit] and po [S][n_q][nsplit][128]
 * (null on the batched path). */
int32_t q3a_selftest_batched_attn_launch(int32_t device, int32_t kv_f32, int32_t split_path, int32_t S, const float* qkv, const int32_t* pos,
                                         const float* q_norm, const float* k_norm, float eps, const float* rope_cur, void* kcache, void* vcache,
                                         int32_t n_q, int32_t n_kv, int32_t max_ctx, float scale_div, int32_t trim_prologue, int32_t nsplit,
                                         int32_t keys_per_split, int32_t out_form, void* out, float* pm, float* pl, float* po);
/* One launch of the segment attention (encoder windows, causal prefill) on the caller's data.  launcher 0: launch_attn_enc, 1:
 * launch_attn_prefill(group, kv_f32), 2: launch_fattn_enc, 3: launch_fattn_prefill(group).  Segment i has seg_len[i] queries / keys, its q
 * and output rows start at seg_q_row0[i], its keys at element seg_kv_off[i] of K / V.  q fp32 and / or q16 bf16, [q_rows][q_rs]; k and v are
 * buffers of kv_elems elements (fp32 with kv_f32, else bf16 bits) whose element k_base / v_base is what the launch is given as K / V (the
 * encoder's interleaved [rows][3 D] buffer: the same array three times, bases D and 2 D); head stride kv_hs, row stride kv_rs.  The output
 * (o fp32 or o16 bf16, [o_rows][o_rs]) goes up with the caller's content between guard zones and comes back whole.  The call fails when
 * the launcher refuses (its message is the error), when an index would leave a buffer, or when a byte of k or v changed.  form[12]: MFMA
 * (1) or VALU (0) family, DMA kernel, HD, GROUP, CAUSAL, fp32 K/V, KSPLIT, NS, QPW, grid x, y, z of the instantiation launched. */
int32_t q3a_selftest_seg_attn_launch(int32_t device, int32_t launcher, int32_t kv_f32, int32_t group, const int32_t* seg_q_row0, const int32_t* seg_len,
                                     const int64_t* seg_kv_off, int32_t n_segs, int32_t max_len, const float* q, const uint16_t* q16, int32_t q_rows,
                                     int32_t q_rs, const void* k, const void* v, int64_t kv_elems, int64_t k_base, int64_t v_base, int64_t kv_hs,
                                     int32_t kv_rs, int32_t n_kv_heads, float scale_div, float* o, uint16_t* o16, int32_t o_rows, int32_t o_rs,
                                     int32_t* form);
/* Rows [0, M1) of an M x N bf16 GEMM that launch_gemm256 gives to the 256 x 256 kernel when it hands the trailing rows to the small
 * tiles (wave quantisation; 0: no split).  Host arithmetic, no device needed. */
int32_t q3a_gemm256_split_rows(int32_t M, int32_t N);

#ifdef __cplusplus
}
#endif
#endif /* Q3ASR_H */
