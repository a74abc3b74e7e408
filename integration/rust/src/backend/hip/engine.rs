//! Engine-level binding (include/q3asr.h): the fused hot path.  `AsrInference::transcribe` under `feature = "hip"` calls
//! `HipEngine::transcribe_batch` (steps 2-8 of src/inference.rs:95-200 in one FFI call) instead of walking the model
//! through `Tensor` ops; `HipGroup` is the same for several GPUs (one broadcast of the weights, utterances partitioned).
//! Uncompiled here (no Rust toolchain on the build boxes).
#![allow(non_camel_case_types, dead_code)]

use anyhow::{bail, Result};
use std::ffi::{CStr, CString};
use std::os::raw::c_char;
use std::path::Path;

#[repr(C)]
pub struct q3a_engine { _private: [u8; 0] }
#[repr(C)]
pub struct q3a_group { _private: [u8; 0] }
#[repr(C)]
pub struct q3a_tokenizer { _private: [u8; 0] }

#[repr(C)]
#[derive(Clone, Copy)]
pub struct q3a_opts {
    pub precise: i32,
    pub max_new_tokens: i32,
    pub use_graph: i32,
    pub debug_taps: i32,
    pub valu_attention: i32,
    pub token_logprobs: i32,
    pub reserved: [i32; 10],
}

#[link(name = "q3asr_hip")]
extern "C" {
    pub fn q3a_opts_default(o: *mut q3a_opts);
    pub fn q3a_device_count() -> i32;
    pub fn q3a_engine_create(model_dir: *const c_char, device: i32, opts: *const q3a_opts, out: *mut *mut q3a_engine) -> i32;
    pub fn q3a_engine_destroy(e: *mut q3a_engine);
    pub fn q3a_last_error(e: *const q3a_engine) -> *const c_char;
    pub fn q3a_transcribe_batch(e: *mut q3a_engine, pcm16k: *const f32, n_samples: *const i64, b: i32, lang_prefix_ids: *const i32,
                                n_prefix: i32, max_new: i32, fixed_new_tokens: i32, out_ids: *mut i32, stride: i32, out_lens: *mut i32) -> i32;
    pub fn q3a_fetch_logprobs(e: *mut q3a_engine, out_lp: *mut f32, stride: i32, out_lens: *mut i32) -> i32;
    pub fn q3a_transcribe_batch_ptrs(e: *mut q3a_engine, pcm16k: *const *const f32, n_samples: *const i64, b: i32, lang_prefix_ids: *const i32,
                                     n_prefix: i32, max_new: i32, fixed_new_tokens: i32, out_ids: *mut i32, stride: i32, out_lens: *mut i32) -> i32;
    pub fn q3a_group_create(model_dir: *const c_char, n_gpus: i32, devices: *const i32, opts: *const q3a_opts, out: *mut *mut q3a_group) -> i32;
    pub fn q3a_group_destroy(g: *mut q3a_group);
    pub fn q3a_group_size(g: *const q3a_group) -> i32;
    pub fn q3a_group_last_error(g: *const q3a_group) -> *const c_char;
    pub fn q3a_group_startup_seconds(g: *const q3a_group, out4: *mut f64) -> i32;
    pub fn q3a_group_transcribe(g: *mut q3a_group, pcm16k: *const f32, n_samples: *const i64, b: i32, lang_prefix_ids: *const i32,
                                n_prefix: i32, max_new: i32, fixed_new_tokens: i32, out_ids: *mut i32, stride: i32, out_lens: *mut i32) -> i32;
    pub fn q3a_group_transcribe_ptrs(g: *mut q3a_group, pcm16k: *const *const f32, n_samples: *const i64, b: i32, lang_prefix_ids: *const i32,
                                     n_prefix: i32, max_new: i32, fixed_new_tokens: i32, out_ids: *mut i32, stride: i32, out_lens: *mut i32) -> i32;
    // forced aligner (word timestamps; include/q3asr.h "forced aligner")
    pub fn q3a_aligner_info(e: *const q3a_engine, classify_num: *mut i32, timestamp_token_id: *mut i32, segment_ms: *mut f32) -> i32;
    pub fn q3a_build_align_prompt(num_audio_tokens: i32, text_ids: *const i32, n_text: i32, ids: *mut i32, len: *mut i32) -> i32;
    pub fn q3a_align(e: *mut q3a_engine, ids: *const i32, lens: *const i32, b: i32, out_classes: *mut i32, stride: i32,
                     out_counts: *mut i32, logits_out: *mut f32) -> i32;
    pub fn q3a_align_batch_ptrs(e: *mut q3a_engine, pcm16k: *const *const f32, n_samples: *const i64, b: i32, text_ids: *const i32,
                                text_lens: *const i32, out_classes: *mut i32, stride: i32, out_counts: *mut i32) -> i32;
    pub fn q3a_split_words_for_alignment(utf8: *const c_char, language: *const c_char, out: *mut c_char, cap: i32, n_words: *mut i32,
                                         len: *mut i32) -> i32;
    pub fn q3a_align_text_ids(t: *const q3a_tokenizer, words: *const *const c_char, n_words: i32, timestamp_token_id: i32, ids: *mut i32,
                              cap: i32, n: *mut i32) -> i32;
    pub fn q3a_fix_timestamps(ms: *const f32, n: i32, out: *mut f32) -> i32;
    // scoring a given transcript (per-token log-probabilities in one prefill; include/q3asr.h "scoring a given transcript")
    pub fn q3a_score(e: *mut q3a_engine, prompt_ids: *const i32, prompt_lens: *const i32, target_ids: *const i32, target_lens: *const i32,
                     b: i32, out_lp: *mut f32, out_top_ids: *mut i32, out_top_lp: *mut f32, stride: i32, logits_out: *mut f32) -> i32;
    pub fn q3a_score_batch_ptrs(e: *mut q3a_engine, pcm16k: *const *const f32, n_samples: *const i64, b: i32, lang_prefix_ids: *const i32,
                                n_prefix: i32, target_ids: *const i32, target_lens: *const i32, out_lp: *mut f32, out_top_ids: *mut i32,
                                out_top_lp: *mut f32, stride: i32) -> i32;
    // constrained decoding: a per-token logit bias inside every lm_head form of the generation paths (include/q3asr.h "constrained
    // decoding"); q3a_score* / q3a_align* never see it
    pub fn q3a_set_logit_bias(e: *mut q3a_engine, ids: *const i32, bias: *const f32, n: i32, default_bias: f32) -> i32;
    pub fn q3a_parse_logit_bias(text: *const c_char, suppress_list: *const c_char, ids: *mut i32, bias: *mut f32, cap: i32, n: *mut i32) -> i32;
    pub fn q3a_set_sampling(e: *mut q3a_engine, temperature: f32, min_p: f32, seed: u64) -> i32;
    pub fn q3a_sample_word(seed: u64, s: u32, t: u32, j: u32) -> u32;
    // top-k / top-p inside the sampled step (include/q3asr.h "sampling filter")
    pub fn q3a_set_sampling_filter(e: *mut q3a_engine, top_k: i32, top_p: f32) -> i32;
    pub fn q3a_selftest_sample_filter(device: i32, logits: *const f32, s: i32, v: i32, temperature: f32, min_p: f32, top_k: i32, top_p: f32,
                                      seed: u64, step: i32, out_ids: *mut i32, out_lp: *mut f32, out_z: *mut f32, out_thr: *mut f32,
                                      out_kept: *mut i32) -> i32;
    // repetition penalty and no-repeat n-grams on the sequence's own generated ids (include/q3asr.h "repetition")
    pub fn q3a_set_repetition(e: *mut q3a_engine, repetition_penalty: f32, no_repeat_ngram_size: i32) -> i32;
    pub fn q3a_selftest_repeat(device: i32, logits: *const f32, s: i32, v: i32, hist: *const i32, stride: i32, lens: *const i32, p: f32, n: i32,
                               out_logits: *mut f32, out_ids: *mut i32, out_lp: *mut f32) -> i32;
    // sequence bias: hotword boosts and banned phrases on the sequence's own generated ids (include/q3asr.h "sequence bias")
    pub fn q3a_set_sequence_bias(e: *mut q3a_engine, ids: *const i32, lens: *const i32, bias: *const f32, n: i32) -> i32;
    pub fn q3a_selftest_seqbias(device: i32, logits: *const f32, s: i32, v: i32, hist: *const i32, stride: i32, lens: *const i32,
                                seq_ids: *const i32, seq_lens: *const i32, seq_bias: *const f32, n: i32, out_logits: *mut f32,
                                out_ids: *mut i32, out_lp: *mut f32) -> i32;
    pub fn q3a_parse_sequence_bias(text: *const c_char, ids: *mut i32, ids_cap: i32, lens: *mut i32, bias: *mut f32, cap: i32,
                                   n_ids: *mut i32, n: *mut i32) -> i32;
    // row options: per-request decoding options inside one batch (include/q3asr.h "row options")
    pub fn q3a_set_row_options(e: *mut q3a_engine, rows: *const RowOptions, n_rows: i32) -> i32;
    pub fn q3a_set_sequence_bias_lists(e: *mut q3a_engine, ids: *const i32, lens: *const i32, bias: *const f32, list_lens: *const i32,
                                       n_lists: i32) -> i32;
    // top log-probabilities: the n best alternatives of every generated token (include/q3asr.h "top log-probabilities")
    pub fn q3a_set_top_logprobs(e: *mut q3a_engine, n: i32) -> i32;
    pub fn q3a_fetch_top_logprobs(e: *mut q3a_engine, out_ids: *mut i32, out_lp: *mut f32, stride: i32, n_stride: i32, out_lens: *mut i32) -> i32;
    pub fn q3a_selftest_top_logprobs(device: i32, logits: *const f32, s: i32, v: i32, n: i32, step_count: *const i32, done: *const u8,
                                     stride: i32, out_ids: *mut i32, out_lp: *mut f32) -> i32;
    // beam search: n-best hypotheses with scores, selected on the device (include/q3asr.h "beam search")
    pub fn q3a_beam_search_batch_ptrs(e: *mut q3a_engine, pcm16k: *const *const f32, n_samples: *const i64, u: i32,
                                      lang_prefix_ids: *const i32, n_prefix: i32, width: i32, max_new: i32, out_ids: *mut i32, stride: i32,
                                      out_lens: *mut i32, out_scores: *mut f32, out_finished: *mut u8, out_lp: *mut f32) -> i32;
    pub fn q3a_beam_begin(e: *mut q3a_engine, width: i32) -> i32;
    pub fn q3a_beam_step(e: *mut q3a_engine, all_finished: *mut u8, logits_out: *mut f32) -> i32;
    pub fn q3a_beam_fetch(e: *mut q3a_engine, out_ids: *mut i32, stride: i32, out_lens: *mut i32, out_scores: *mut f32,
                          out_finished: *mut u8, out_lp: *mut f32) -> i32;
    pub fn q3a_selftest_beam_topk(device: i32, logits: *const f32, s: i32, v: i32, w: i32, out_ids: *mut i32, out_lp: *mut f32) -> i32;
    pub fn q3a_selftest_beam_advance(device: i32, u: i32, w: i32, topk_ids: *const i32, topk_lp: *const f32, score_in: *const f32,
                                     finished_in: *const u8, parent_out: *mut i32, token_out: *mut i32, score_out: *mut f32,
                                     finished_out: *mut u8) -> i32;
    pub fn q3a_selftest_kv_reorder(device: i32, cache: *mut std::ffi::c_void, elem_bytes: i32, layers: i32, s: i32, n_kv: i32, max_ctx: i32,
                                   lo: *const i32, hi: *const i32, parent: *const i32) -> i32;
    // one launch of the GEMM family / of QK-norm + RoPE + cache append on the caller's data (include/q3asr.h; tests/gemm_ref.py)
    pub fn q3a_selftest_gemm_launch(device: i32, launcher: i32, flags: i32, x: *const std::ffi::c_void, w: *const u16, m: i32, n: i32, k: i32,
                                    lda: i32, ldo: i32, imgs: i32, h: i32, wd: i32, c: i32, bias: *const f32, addend: *const f32,
                                    addend_period: i32, resid: *const f32, rowmap: *const i32, act: i32, out: *mut std::ffi::c_void,
                                    out_rows: i32) -> i32;
    pub fn q3a_selftest_qkrope_launch(device: i32, fused: i32, kv_f32: i32, x: *const u16, lda: i32, w: *const u16, m: i32, k: i32,
                                      bias: *const f32, qkv: *mut f32, row_seq: *const i32, row_pos: *const i32, q_norm: *const f32,
                                      k_norm: *const f32, eps: f32, cos_t: *const f32, sin_t: *const f32, max_pos: i32, n_q: i32, n_kv: i32,
                                      n_seq: i32, max_ctx: i32, q16: *mut u16, kcache: *mut std::ffi::c_void, vcache: *mut std::ffi::c_void) -> i32;
    pub fn q3a_gemm256_split_rows(m: i32, n: i32) -> i32;
}

/// src/main.rs:51-65 for the `hip` feature: HIP devices visible to this process (0: none -- there is no CPU path).
pub fn device_count() -> i32 { unsafe { q3a_device_count() } }

fn msg(p: *const c_char) -> String {
    if p.is_null() { "unknown error".into() } else { unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned() }
}

/// One GPU: owns a `q3a_engine` (weights arena, workspace, stream).  One host thread per handle.
pub struct HipEngine { raw: *mut q3a_engine }
unsafe impl Send for HipEngine {}

impl Drop for HipEngine {
    fn drop(&mut self) { if !self.raw.is_null() { unsafe { q3a_engine_destroy(self.raw) } } }
}

impl HipEngine {
    /// AsrInference::load's model part (src/inference.rs:30-66): config.json + safetensors -> device arena.
    pub fn load(model_dir: &Path, device: usize) -> Result<Self> {
        let dir = CString::new(model_dir.to_string_lossy().as_bytes())?;
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { q3a_engine_create(dir.as_ptr(), device as i32, std::ptr::null(), &mut raw) };
        if rc != 0 { bail!("Failed to load model: {}", msg(unsafe { q3a_last_error(std::ptr::null()) })); }
        Ok(HipEngine { raw })
    }

    /// Steps 2-8 of `transcribe` for a batch of independent utterances (16 kHz f32).  Returns generated ids (EOS excluded).
    pub fn transcribe_batch(&self, clips: &[&[f32]], lang_prefix_ids: &[i32], max_new: usize) -> Result<Vec<Vec<i64>>> {
        let b = clips.len();
        let n: Vec<i64> = clips.iter().map(|c| c.len() as i64).collect();
        // one pointer per utterance: the Vec<f32> that load_audio (src/audio.rs:7) returned for each file is handed over as it is --
        // no concatenation on the host; the library stages the pageable buffers into pinned memory and overlaps the copy with the mel
        let ptrs: Vec<*const f32> = clips.iter().map(|c| c.as_ptr()).collect();
        let mut ids = vec![0i32; b * max_new];
        let mut lens = vec![0i32; b];
        let pre = if lang_prefix_ids.is_empty() { std::ptr::null() } else { lang_prefix_ids.as_ptr() };
        let rc = unsafe {
            q3a_transcribe_batch_ptrs(self.raw, ptrs.as_ptr(), n.as_ptr(), b as i32, pre, lang_prefix_ids.len() as i32, max_new as i32, 0,
                                      ids.as_mut_ptr(), max_new as i32, lens.as_mut_ptr())
        };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok((0..b).map(|i| ids[i * max_new..i * max_new + lens[i] as usize].iter().map(|&x| x as i64).collect()).collect())
    }

    /// Top-k / top-p for every later sampled generation call (q3a_set_sampling with a temperature > 0): keep the entries that reach the
    /// `top_k`-th largest logit (0: off; ties kept), and of those the head whose probability reaches `top_p` (1.0: off).
    pub fn set_sampling_filter(&self, top_k: usize, top_p: f32) -> Result<()> {
        if top_k > i32::MAX as usize { bail!("set_sampling_filter: top_k does not fit an int32"); }
        let rc = unsafe { q3a_set_sampling_filter(self.raw, top_k as i32, top_p) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// Repetition control for every later generation call: `repetition_penalty` (1.0: none) over the ids a sequence has generated,
    /// then a ban on every id that would repeat an n-gram of `no_repeat_ngram_size` ids (0: none).  (1.0, 0) turns it off.
    pub fn set_repetition(&self, repetition_penalty: f32, no_repeat_ngram_size: usize) -> Result<()> {
        let rc = unsafe { q3a_set_repetition(self.raw, repetition_penalty, no_repeat_ngram_size as i32) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// Sequence bias for every later generation call: `entries` are (token sequence, bias) pairs; at every step the bias is added to
    /// the logit of the sequence's last id whenever the ids generated so far end in the rest of it (HuggingFace's
    /// SequenceBiasLogitsProcessor; a bias of f32::NEG_INFINITY bans the phrase).  An empty slice turns it off.
    pub fn set_sequence_bias(&self, entries: &[(&[i32], f32)]) -> Result<()> {
        let ids: Vec<i32> = entries.iter().flat_map(|(q, _)| q.iter().copied()).collect();
        let lens: Vec<i32> = entries.iter().map(|(q, _)| q.len() as i32).collect();
        let bias: Vec<f32> = entries.iter().map(|(_, b)| *b).collect();
        let rc = unsafe { q3a_set_sequence_bias(self.raw, ids.as_ptr(), lens.as_ptr(), bias.as_ptr(), entries.len() as i32) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// Several sequence-bias lists at once, for the rows of a row table to choose from (`RowOptions::sequence_list`); without a row
    /// table every sequence uses list 0.  An empty slice clears them.
    pub fn set_sequence_bias_lists(&self, lists: &[&[(&[i32], f32)]]) -> Result<()> {
        let ids: Vec<i32> = lists.iter().flat_map(|l| l.iter()).flat_map(|(q, _)| q.iter().copied()).collect();
        let lens: Vec<i32> = lists.iter().flat_map(|l| l.iter()).map(|(q, _)| q.len() as i32).collect();
        let bias: Vec<f32> = lists.iter().flat_map(|l| l.iter()).map(|(_, b)| *b).collect();
        let list_lens: Vec<i32> = lists.iter().map(|l| l.len() as i32).collect();
        let rc = unsafe { q3a_set_sequence_bias_lists(self.raw, ids.as_ptr(), lens.as_ptr(), bias.as_ptr(), list_lens.as_ptr(), lists.len() as i32) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// One record of decoding options per sequence of the next batches (sequence s of a call reads `rows[s]`); an empty slice clears
    /// the table and the engine's uniform settings are in force again.  The next prefill must hold `rows.len()` sequences.
    pub fn set_row_options(&self, rows: &[RowOptions]) -> Result<()> {
        let rc = unsafe { q3a_set_row_options(self.raw, rows.as_ptr(), rows.len() as i32) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// Top log-probabilities for every later generation call: while `n` > 0 (at most 20) every step also records the `n` best entries
    /// of its final row -- larger logit first, then smaller id -- with their log-probabilities.  0 turns it off.
    pub fn set_top_logprobs(&self, n: usize) -> Result<()> {
        if n > 20 { bail!("set_top_logprobs: n must lie in [0, 20]"); }
        let rc = unsafe { q3a_set_top_logprobs(self.raw, n as i32) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok(())
    }

    /// What the last run of `batch` utterances recorded under `set_top_logprobs(n)`: per utterance and per generated id (at most
    /// `max_new` of them, as `transcribe_batch` returned them) the `n` candidates of its step as (id, log-probability), best first.
    pub fn fetch_top_logprobs(&self, batch: usize, max_new: usize, n: usize) -> Result<Vec<Vec<Vec<(i32, f32)>>>> {
        let mut ids = vec![0i32; batch * max_new * n];
        let mut lp = vec![0f32; batch * max_new * n];
        let mut lens = vec![0i32; batch];
        let rc = unsafe { q3a_fetch_top_logprobs(self.raw, ids.as_mut_ptr(), lp.as_mut_ptr(), max_new as i32, n as i32, lens.as_mut_ptr()) };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_last_error(self.raw) })); }
        Ok((0..batch).map(|b| (0..(lens[b] as usize).min(max_new)).map(|t| {
            let o = (b * max_new + t) * n;
            (0..n).map(|k| (ids[o + k], lp[o + k])).collect()
        }).collect()).collect())
    }
}

/// `q3a_row_options`: what the uniform setters hold once per engine, for one sequence of a batch.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct RowOptions {
    pub temperature: f32,
    pub min_p: f32,
    pub seed: u64,
    pub top_k: i32,
    pub top_p: f32,
    pub repetition_penalty: f32,
    pub no_repeat_ngram_size: i32,
    pub sequence_list: i32,
}

impl Default for RowOptions {
    /// A plain greedy row: nothing on, no list.
    fn default() -> Self {
        RowOptions { temperature: 0.0, min_p: 0.0, seed: 0, top_k: 0, top_p: 1.0, repetition_penalty: 1.0, no_repeat_ngram_size: 0, sequence_list: -1 }
    }
}

/// Several GPUs of one node: weights read once, one RCCL broadcast, utterances partitioned contiguously.
pub struct HipGroup { raw: *mut q3a_group }
unsafe impl Send for HipGroup {}

impl Drop for HipGroup {
    fn drop(&mut self) { if !self.raw.is_null() { unsafe { q3a_group_destroy(self.raw) } } }
}

impl HipGroup {
    pub fn load(model_dir: &Path, n_gpus: usize) -> Result<Self> {
        let dir = CString::new(model_dir.to_string_lossy().as_bytes())?;
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { q3a_group_create(dir.as_ptr(), n_gpus as i32, std::ptr::null(), std::ptr::null(), &mut raw) };
        if rc != 0 { bail!("Failed to load model: {}", msg(unsafe { q3a_last_error(std::ptr::null()) })); }
        Ok(HipGroup { raw })
    }

    /// Start-up stage times in seconds: [checkpoint read + pack into pinned memory, H2D upload, RCCL broadcast, engine creation].
    pub fn startup_seconds(&self) -> [f64; 4] {
        let mut v = [0f64; 4];
        unsafe { q3a_group_startup_seconds(self.raw, v.as_mut_ptr()) };
        v
    }

    pub fn transcribe_batch(&self, clips: &[&[f32]], lang_prefix_ids: &[i32], max_new: usize) -> Result<Vec<Vec<i64>>> {
        let b = clips.len();
        let n: Vec<i64> = clips.iter().map(|c| c.len() as i64).collect();
        let ptrs: Vec<*const f32> = clips.iter().map(|c| c.as_ptr()).collect();
        let mut ids = vec![0i32; b * max_new];
        let mut lens = vec![0i32; b];
        let pre = if lang_prefix_ids.is_empty() { std::ptr::null() } else { lang_prefix_ids.as_ptr() };
        let rc = unsafe {
            q3a_group_transcribe_ptrs(self.raw, ptrs.as_ptr(), n.as_ptr(), b as i32, pre, lang_prefix_ids.len() as i32, max_new as i32, 0,
                                      ids.as_mut_ptr(), max_new as i32, lens.as_mut_ptr())
        };
        if rc != 0 { bail!("{}", msg(unsafe { q3a_group_last_error(self.raw) })); }
        Ok((0..b).map(|i| ids[i * max_new..i * max_new + lens[i] as usize].iter().map(|&x| x as i64).collect()).collect())
    }
}
