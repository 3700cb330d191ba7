/* libkzv -- C ABI of the MI355X-native TrOCR line-OCR training engine.
 *
 * The reference (Kotomiya07/kuzushiji-vision) has no FFI for this path: every FLOP runs inside
 * PyTorch / HF transformers behind the Python class `TrOCRModel`
 * (src/models/trocr_model.py:205-460).  This header is the boundary a maintainer would bind from
 * that class (ctypes stub: INTEGRATION.md).  Each entry point names the reference call it replaces.
 *
 * Conventions: every function returns 0 on success, a negative KZV_E_* code on error and records
 * a message readable through kzv_last_error().  All pointers named d_* are DEVICE pointers owned
 * by the caller (torch tensors in the Python host): parameters, gradients, optimizer state and one workspace
 * sized by kzv_workspace_bytes.  The library itself allocates only small or grow-only scratch on the current device,
 * kept for the life of the process (one device per process): a 4 KiB page of zeros (LDS-DMA loads of out-of-range
 * tile rows are pointed at it), the LayerNorm gamma/beta partial rows (64 regions of 512 KiB: the folds of a backward pass are one
 * launch), the gemm_tn256 partial-tile workspace (6 regions of <= 66 MB: the folds of an encoder layer's four weight gradients are
 * one launch), the embedding backward's partial sums (~5 MB at batch 256) and, per model handle, the generation path's KV cache,
 * beam row tables, decode-layout copy of the cross-attention K/V and the fragment-ordered copy of the decoder weights (9.6 MB;
 * allocated at the first kzv_decode_step / kzv_decode_begin or training forward that needs them, freed by kzv_model_destroy).
 * Other global state: the last-error string, the profiling slots and the CU reserve.  `stream` is a hipStream_t passed as void*.
 * One model handle per process/GPU; a handle is not re-entrant.
 */
#ifndef KZV_H
#define KZV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZV_OK 0
#define KZV_E_ARG (-1)     /* bad argument / shape (reference: ValueError, trocr_model.py:83-86) */
#define KZV_E_HIP (-2)     /* HIP runtime error */
#define KZV_E_STATE (-3)   /* call order violated (e.g. backward before forward) */

const char* kzv_last_error(void);
int kzv_version(void);

/* ------------------------------------------------------------------ geometry */
/* Mirrors encoder_config (trocr_model.py:234-244) + the decoder's RobertaConfig
 * (train_language_model_scratch.py:406-428). */
typedef struct kzv_config {
    int32_t image_h, image_w, patch_h, patch_w, channels;
    int32_t enc_hidden, enc_layers, enc_heads, enc_ffn;
    int32_t dec_hidden, dec_layers, dec_heads, dec_ffn;
    int32_t vocab, max_pos, type_vocab, pad_id;
    float enc_hidden_dropout, enc_attn_dropout, dec_hidden_dropout, dec_attn_dropout;
    float ln_eps;
} kzv_config;

typedef struct kzv_model kzv_model;

/* TrOCRModel.__init__ (trocr_model.py:208-256): validates geometry, builds the parameter table. */
int kzv_model_create(const kzv_config* cfg, kzv_model** out);
/* kzv_model_create with flags (kzv_model_create(cfg, out) == kzv_model_create_ex(cfg, 0, out)).
 * KZV_MODEL_LONG_SEQ: encoders with head_dim 64 or 96 take up to 4,097 tokens (4,096 patches + CLS); attention launches whose
 * key or query count exceeds 288 run the K/V-streaming kernels (kzv_attn_impl_ex), shorter ones the whole-head kernels as before.
 * Other encoder head dims keep the 288-token cap.  kzv_model_bind then also refuses batches whose attention-dropout block index
 * B * heads * ceil(Sq / 4) * ceil(Sk / 4) would pass 2^32 (the generator's block word is 32-bit). */
#define KZV_MODEL_LONG_SEQ 1u
int kzv_model_create_ex(const kzv_config* cfg, unsigned flags, kzv_model** out);
int kzv_model_destroy(kzv_model* m);

/* Parameter table = the reference's state_dict, fused/flattened (kzv/params.py documents the
 * mapping to HF names).  Offsets are in fp32 ELEMENTS into the flat master buffer. */
int kzv_param_count(const kzv_model* m);
int kzv_param_info(const kzv_model* m, int i, const char** name, int64_t* offset, int64_t* rows, int64_t* cols);
int64_t kzv_param_total(const kzv_model* m);                 /* padded element count of the flat buffer */

/* Bytes of caller-provided device memory needed for a per-GPU batch of B crops with labels [B, L]. */
int64_t kzv_workspace_bytes(const kzv_model* m, int batch, int label_len);

/* Bind caller-owned device buffers: fp32 master params, fp32 grads (same layout), workspace.
 * (the reference's nn.Parameter storage + autograd .grad + activation memory) */
int kzv_model_bind(kzv_model* m, float* d_params, float* d_grads, void* d_workspace, int64_t workspace_bytes,
                   int batch, int label_len);

/* Refresh the bf16 compute copies (W and W^T) from the fp32 masters; call after the masters change
 * (load_state_dict / optimizer step).  Stands in for autocast's per-op weight cast. */
int kzv_model_sync_weights(kzv_model* m, void* stream);

/* TrOCRModel.forward(pixel_values, labels) training branch (trocr_model.py:258-297).
 *   d_pixel_values fp32 [B,C,H,W]; d_labels int64 [B,L]; d_loss fp32[1] (mean CE over non-pad targets);
 *   d_logits fp32 [B,L-1,V] or NULL.  train!=0 applies dropout (keyed by `seed`) and keeps what
 *   backward needs.  Image-size mismatch is the caller's ValueError (host checks shapes). */
int kzv_forward_loss(kzv_model* m, const float* d_pixel_values, const int64_t* d_labels,
                     float* d_loss, float* d_logits, int train, uint64_t seed, void* stream);

/* Width buckets (BASELINE.json configs[4]; beyond the reference, whose model instance has ONE image size,
 * src/models/trocr_model.py:83-86,113-115).  The handle is created for the WIDEST crop (cfg.image_w, which sizes the
 * position table and the workspace); a batch of narrower crops [B, C, H, width] runs with (H/ph) * (width/pw) patches:
 * patch (h, w) takes the position row of (h, w) in the widest grid -- for the sin/cos table (trocr_model.py:154-167) that
 * IS the closed-form table of the narrow grid, because an entry depends on (w, h) only.  width must be a multiple of
 * the patch width, <= cfg.image_w.  Applies to the following kzv_forward_loss (default after create: cfg.image_w). */
int kzv_set_image_width(kzv_model* m, int width);

/* Position-id overflow check of the LAST kzv_forward_loss / kzv_decode_logits on this handle: RoBERTa's position ids
 * (count of non-pad decoder inputs + pad_id, HF modeling_roberta.py:142-155) must index the [max_pos, H] table; the reference
 * raises "index out of range" for longer labels, the kernels clamp and raise a device flag.  Synchronises `stream`, reads the
 * flag (cleared by every forward) and returns KZV_E_ARG when it was set.  Optional: the Python host validates labels it can
 * see on the CPU before the call. */
int kzv_check_positions(kzv_model* m, void* stream);

/* Active decoder length.  Labels are [B, L] rows padded to L; when every sample's characters end before column
 * t_active + 1, decoder positions >= t_active hold only padding: they are masked as attention keys, their targets are
 * ignored by the loss and nothing reads their outputs, so the engine may run the decoder on the packed [B, t_active]
 * prefix -- loss and gradients are unchanged (the reference computes and discards those positions).  Default after
 * kzv_model_bind: L - 1 (everything).  kzv_forward_loss with d_logits != NULL requires the full length. */
int kzv_set_active_length(kzv_model* m, int t_active);

/* Decoder-only teacher-forced pass over `d_labels` [B,L] reusing the encoder states (and cross-attention K/V) of the
 * last kzv_forward_loss on this handle; writes the logits of position `pos` of every sample, fp32 [B,V].  Building
 * block of generation (TrOCRModel.forward inference branch, trocr_model.py:298-321): under the causal mask position
 * pos only depends on ids[:, :pos+1].  Invalidates the saved activations (no backward afterwards). */
int kzv_decode_logits(kzv_model* m, const int64_t* d_labels, int pos, float* d_logits, void* stream);

/* What the last kzv_forward_loss knows about each label position beyond the loss, read back from its saved decoder activations.
 * Both need the decoder activations of a FULL kzv_forward_loss (train 0 or 1) in the workspace: a rebind, a change of the image
 * width or the active length, kzv_encode_images, kzv_decode_logits and the kzv_decode_step calls invalidate them (KZV_E_STATE).
 * Both only read saved activations (kzv_score_tokens also rewrites the workspace's logits region, which nothing else reads later):
 * kzv_backward after them still works.
 *
 * Cross-attention weights of decoder layer `layer` (0..Ld-1; -1 = last) of the last kzv_forward_loss,
 * averaged over heads: rows are the PACKED decoder rows [B, t_active]; keys are the active patches,
 * grid_w = active image width / patch_w.  HF: output_attentions=True -> cross_attentions[layer].mean(1).
 * d_map fp32 [B, t_active, ld_map] or NULL, d_pos fp32 [B, t_active, 4], d_peak int32 [B, t_active]: kzv_attn_probs' outputs.  In
 * training mode they are the probabilities before attention dropout. */
int kzv_cross_attention(kzv_model* m, int layer, float* d_map, int64_t ld_map, float* d_pos, int32_t* d_peak, void* stream);
/* Per-position log-probabilities of the labels of the last kzv_forward_loss, [B, t_active] each: kzv_token_scores' outputs on the
 * vocabulary GEMM re-run from the saved LM-head input (valid after the one-launch head + CE path too, which never wrote logits). */
int kzv_score_tokens(kzv_model* m, float* d_logprob, int64_t* d_top1, float* d_top1_logprob, void* stream);
/* The k (1..8) best tokens of every label position of the last kzv_forward_loss and their log-probabilities, best first: d_ids int32
 * and d_logprob fp32, [B, t_active, k] each -- kzv_token_topk's outputs on the same re-run vocabulary GEMM.  Replaces HF's
 * output_scores=True, scores[t].log_softmax(-1).topk(k), for which fp32 logits [B, t_active, vocab] would have to cross the ABI.  State
 * rules, validity (after the one-launch head + CE path too) and workspace use are kzv_score_tokens': entry 0 is its top1 / top1_logprob,
 * and kzv_backward afterwards still works.  KZV_E_ARG: k outside 1..8, a null result array. */
int kzv_score_tokens_topk(kzv_model* m, int k, int32_t* d_ids, float* d_logprob, void* stream);

/* Encoder only (ViTEncoder.forward + encoder_decoder_proj + the cross-attention K/V of every decoder layer) for n_images
 * crops [n_images, C, H, W], n_images dividing the bound batch: the bound batch counts DECODER rows, and beam search runs
 * batch / n_images beams per image that all attend to that image's K/V (HF expands encoder_hidden_states per beam,
 * trocr_model.py:306-316 -> generate; the values are identical, so they are computed and stored once).  Only
 * kzv_decode_step* may follow (kzv_decode_logits / kzv_forward_loss need one image per row). */
int kzv_encode_images(kzv_model* m, const float* d_pixel_values, int n_images, void* stream);

/* KV-cached generation step (what `decoder.generate(use_cache=True)` does per token, trocr_model.py:306-316): feeds ONE
 * token per sequence -- d_tokens [B] at decoder index t, with RoBERTa position ids d_posids [B] (t + 1 + pad_id for a live
 * sequence, pad_id for padding) -- through the decoder against the self-attention keys / values cached by steps 0..t-1
 * (this step's are appended) and the cross-attention K/V of the last kzv_forward_loss; d_valid [B, ld_valid] marks the
 * usable self-attention keys (key j usable iff token j is not padding; column t must already be set).  Writes logits
 * [B, V] for the next token.  Steps must be issued in order t = 0, 1, ...; the cache is sized [B, L-1] at the first call.
 * kzv_decode_reorder re-parents the sequences after a beam step: row b continues from former row d_rows[b] (first `len` key
 * positions).  No cache row moves: a row table tells the next steps' attention which ancestor's row holds each cached key. */
int kzv_decode_step(kzv_model* m, const int64_t* d_tokens, const int32_t* d_posids, int t, const uint8_t* d_valid, int64_t ld_valid,
                    float* d_logits, void* stream);
int kzv_decode_reorder(kzv_model* m, const int64_t* d_rows, int len, void* stream);
/* One beam-search step's ranking on the device (what transformers' GenerationMixin._get_top_k_continuations computes with
 * log_softmax + topk): for each of `batch` images, log_softmax of each of its `num_beams` (<= 8) rows of d_logits [batch *
 * num_beams, ld] + that beam's d_beam_scores entry, then the k (<= 16) best of the num_beams * vocab continuations, best first;
 * equal scores rank by the smaller flat index.  d_top_scores [batch, k] fp32, d_top_index [batch, k] int64 = beam * vocab + token. */
int kzv_beam_topk(const float* d_logits, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                  float* d_top_scores, int64_t* d_top_index, void* stream);
/* The same ranking over rows that already hold log-probabilities (what kzv_logits_process leaves with normalise != 0): no second
 * normalisation, a continuation is d_logprobs[row][token] + the beam's score, -inf entries (banned tokens) never rank.  Arguments and
 * errors as kzv_beam_topk's; the same kernel with its log-sum-exp phase compiled out.  Where fewer than k continuations lie above -inf
 * the surplus entries are -inf at index 0 (inside every table).  kzv_stream_set_controls and the Python layer refuse the masks that
 * lead there by themselves (fewer than 2 tokens left); an n-gram ban on top of a two- or three-token mask can still get there, and
 * the search then carries -inf entries as HF's own top-k does. */
int kzv_beam_rank_logprobs(const float* d_logprobs, int64_t ld, const float* d_beam_scores, int batch, int num_beams, int vocab, int k,
                           float* d_top_scores, int64_t* d_top_index, void* stream);
/* Generation controls on one step's scores, in place -- transformers' repetition_penalty, no_repeat_ngram_size, min_length and
 * suppress_tokens with HF's semantics (kzv/controls.py: process_reference is the readable statement).  For row r of logits [rows, ld]
 * with token history h[0 .. n), BOS included (exactly the input_ids HF hands its logits processors):
 *   repetition_penalty p (> 0; 1 = off): every distinct token v of h once, x[v] = x[v] < 0 ? x[v] * p : x[v] / p (a true fp32 division);
 *   no_repeat_ngram_size g (0 = off, 1..8): nothing while n + 1 < g; else for every i in 0 .. n - g with h[i .. i + g - 1) ==
 *     h[n - g + 1 .. n): x[h[i + g - 1]] = -inf (g = 1 bans every token of h);
 *   min_length L (0 = off): x[eos_id] = -inf while n < L;
 *   suppress_mask (optional, device, (vocab + 31) / 32 words, bit v % 32 of word v / 32): x[v] = -inf for every set bit.
 * The last three only write -inf and the penalty maps -inf to -inf, so their order does not matter.
 * normalise != 0: the row is first replaced by its log-softmax, (x - max) - log(sum exp(x - max)), reduced in the order of kzv_beam_topk's
 * first phase (per wave: maximum, then the sum against it; then the four waves merged), and the controls act on that -- what HF's beam search hands its processors; kzv_beam_rank_logprobs then ranks the rows.
 * Where the history lies (never copied):
 *   slot_image == NULL (lockstep)          h = ids[r][0 .. t + 1), t the host scalar;
 *   slot_image, by_image != 0 (greedy slots, group = 1)   h = ids[slot_image[r]][0 .. slot_t[r] + 1): ids = the wave's out_ids;
 *   slot_image, by_image == 0 (beam slots, group = beams) h = ids[r][0 .. slot_t[r / group] + 1): ids = the wave's run_seq;
 * in the slot cases the step index is read from device memory (one captured graph serves every step), and the rows of a slot with
 * slot_image < 0 (idle) or >= n_images are left as they are.  A history is read up to ld_ids tokens at most; tokens outside the vocabulary
 * are skipped.  One workgroup per row; the two token bitmasks live in LDS, hence vocab <= 16,384.
 * KZV_E_ARG before any launch: null args / logits / ids, rows < 1, vocab outside 1..16,384, ld < vocab, ld_ids < 1, g outside 0..8,
 * p <= 0 (or NaN), min_length < 0, EOS outside the vocabulary while min_length > 0, one of slot_image / slot_t without the other, rows no
 * multiple of group, t < 0 in the lockstep case. */
typedef struct kzv_logits_process_args {
    float* logits; int64_t ld;                           /* [rows, ld >= vocab], edited in place */
    int32_t rows, vocab;
    const int64_t* ids; int64_t ld_ids;                  /* token histories */
    int32_t t;                                           /* lockstep: the step index, history length t + 1 */
    int32_t group;                                       /* slot cases: rows per slot */
    const int32_t* slot_image; const int32_t* slot_t;    /* slot cases: [rows / group] */
    int32_t by_image, n_images;
    int32_t no_repeat_ngram_size, min_length, eos_id, normalise;
    float repetition_penalty; int32_t reserved;
    const uint32_t* suppress_mask;
} kzv_logits_process_args;
int kzv_logits_process(const kzv_logits_process_args* args, void* stream);
/* A character n-gram language model on the device (kzv/lm.py: NGramLM fits, loads and lays it out; NGramLM.row is the readable
 * statement of the evaluation).  order in 1..4, vocab <= 16,384.  All tables are device memory:
 *   uni [vocab] fp32                      log P_1(v), natural logarithm;
 *   per context length k = 1 .. order - 1 (index k - 1), n_ctx[k - 1] contexts:
 *     keys[k - 1] int64, ascending        the context's k tokens as one number in base 16,384, the OLDEST token most significant;
 *     bo[k - 1]   fp32                    log of the context's back-off weight;
 *     off[k - 1]  int32 [n_ctx + 1]       CSR offsets into succ_tok / succ_lp (shared by all lengths);
 *   succ_tok int32, succ_lp fp32          a context's seen successors, ascending by token, with log P_{k+1}(v | context).
 * The tables of a length with n_ctx == 0 may be null.
 * Evaluation for a history h[0 .. n), BOS included, all in fp32 and in this order:
 *   acc = 0;  for k = min(order - 1, n) down to 1:  if h[n - k .. n) is a key of length k:
 *       lm[v] = acc + lp for each of its successors (v, lp) that no longer context has set;  acc = acc + bo(context)
 *   lm[v] = acc + uni[v] for every v not set.
 * A context that holds a token outside [0, vocab) counts as not found. */
typedef struct kzv_ngram_lm {
    int32_t order, vocab;
    int32_t n_ctx[3]; int32_t reserved;
    const float* uni;
    const int64_t* keys[3]; const float* bo[3]; const int32_t* off[3];
    const int32_t* succ_tok; const float* succ_lp;
} kzv_ngram_lm;
/* Shallow fusion of the language model into one step's scores, in place: for row r of logits [rows, ld] with history h,
 *   x[v] = x[v] + weight * lm[v]   for every v < vocab (two fp32 roundings: the multiply, then the add; -inf stays -inf),
 * columns [vocab, ld) untouched.  Where the history lies, the slot cases, idle slots and the meaning of ids / ld_ids / t / group /
 * slot_image / slot_t / by_image / n_images: exactly kzv_logits_process's.  `lm` is a HOST pointer to the struct above (read during
 * the call, passed to the kernel by value); its tables must stay alive until the launch has run.
 * Where the fusion acts (one rule everywhere; kzv/lm.py): greedy decoding -- raw logits, the controls if any, then + weight * lm, then
 * arg-max and log-sum-exp of the result; beam search -- log_softmax(logits) (the normalising kzv_logits_process, with neutral controls
 * when none are set), the controls, + weight * lm, + beam score, ranked by kzv_beam_rank_logprobs without a second normalisation.  The
 * fusion comes after the controls: the repetition penalty acts on the model's score alone, and a ban's -inf survives the addition.
 * One workgroup of 256 threads per row; a claim bitmask of one bit per token lives in LDS, hence vocab <= 16,384.
 * KZV_E_ARG before any launch: null args / logits / ids / lm / tables, rows < 1, vocab outside 1..16,384 or different from the LM's,
 * ld < vocab, ld_ids < 1, order outside 1..4, a negative context count, a non-finite weight, one of slot_image / slot_t without the
 * other, rows no multiple of group, t < 0 in the lockstep case. */
typedef struct kzv_lm_fuse_args {
    float* logits; int64_t ld;                           /* [rows, ld >= vocab], edited in place */
    int32_t rows, vocab;
    const int64_t* ids; int64_t ld_ids;                  /* token histories */
    int32_t t;                                           /* lockstep: the step index, history length t + 1 */
    int32_t group;                                       /* slot cases: rows per slot */
    const int32_t* slot_image; const int32_t* slot_t;    /* slot cases: [rows / group] */
    int32_t by_image, n_images;
    float weight; int32_t reserved;
    const kzv_ngram_lm* lm;                              /* host pointer */
} kzv_lm_fuse_args;
int kzv_lm_fuse(const kzv_lm_fuse_args* args, void* stream);
/* Forced prefixes (kzv/prefix.py: force_reference is the torch statement): decoding continues a line from given tokens.  A prefix is 0 or
 * more token ids per image, without BOS, in prefix [n, ld_prefix] int64 with its length in prefix_len [n] int32 (clamped to ld_prefix);
 * both are device memory indexed by IMAGE: r / group in the lockstep case, slot_image[r / group] in the slot cases.  At a step whose
 * chosen index cur = t + 1 satisfies 1 <= cur <= prefix_len[image], row r of logits [rows, ld] becomes -inf in every column below vocab
 * and 0 at the forced token prefix[image][cur - 1] (HF's ForceTokensLogitsProcessor); rows past their prefix, rows of an idle slot and
 * columns [vocab, ld) are not written.  A forced token outside [0, vocab) leaves the row alone (the callers refuse such a prefix).  It
 * is the LAST node of the logits chain, after kzv_logits_process and kzv_lm_fuse: the prompt is subject to neither.  Selection does not
 * change: arg-max picks the forced token with log-probability exactly 0; a beam step (normalise -> fuse -> force ->
 * kzv_beam_rank_logprobs) carries the prefix in all beams at scores 0, -1e9, -1e9, .. -- HF's state after a prompt.  One decoder step per
 * forced token: there is no prefill pass.
 * t / group / slot_image / slot_t / n_images and the idle-slot rule: kzv_logits_process's (group >= 1 also in the lockstep case, where it
 * is the rows per image; by_image is accepted and ignored, since no history is read).
 * forced_logprob (optional, fp32 [n, ld_forced_logprob > ld_prefix]): the model's own opinion of the forced token, written to
 * forced_logprob[image][cur] BEFORE the overwrite by the first row of the group only: x[f] when `normalised` != 0 (the row holds
 * log-probabilities already), x[f] - logsumexp(x) otherwise.
 * One workgroup of 256 threads per row.  KZV_E_ARG before any launch: null args / logits / prefix / prefix_len, rows < 1, vocab outside
 * 1..16,384, ld < vocab, ld_prefix < 1, group < 1 or rows no multiple of it, forced_logprob rows not longer than ld_prefix, one of
 * slot_image / slot_t without the other, n_images < 1 in the slot cases, t < 0 in the lockstep case. */
typedef struct kzv_force_prefix_args {
    float* logits; int64_t ld;                           /* [rows, ld >= vocab], edited in place */
    int32_t rows, vocab;
    int32_t t;                                           /* lockstep: the step index */
    int32_t group;                                       /* rows per image / slot */
    const int32_t* slot_image; const int32_t* slot_t;    /* slot cases: [rows / group] */
    int32_t by_image, n_images;
    const int64_t* prefix; int64_t ld_prefix;            /* [n, ld_prefix] */
    const int32_t* prefix_len;                           /* [n] */
    int32_t normalised, reserved;
    float* forced_logprob; int64_t ld_forced_logprob;    /* optional [n, ld_forced_logprob] */
} kzv_force_prefix_args;
int kzv_force_prefix(const kzv_force_prefix_args* args, void* stream);
/* The inputs of decoder step t from the token table d_ids [batch, ld_ids]: d_tokens [batch] = column t, d_posids [batch] = its
 * RoBERTa position id (t + 1 + pad_id, or pad_id for padding), d_valid[:, t] = token != pad. */
int kzv_decode_prep(const int64_t* d_ids, int64_t ld_ids, int t, int pad_id, int batch, int64_t* d_tokens, uint8_t* d_valid, int64_t ld_valid,
                    int32_t* d_posids, void* stream);
/* Greedy token selection (num_beams = 1): d_ids[:, t + 1] = argmax of the row (first maximum), or pad_id once the sequence has
 * emitted eos_id (d_done [batch] is read and updated); d_running[t] += sequences still running after this step (the caller
 * zeroes d_running [>= t + 1 ints] once per generation and may read it every few steps: steps past the end only write padding). */
int kzv_greedy_update(const float* d_logits, int64_t ld, int vocab, int64_t* d_ids, int64_t ld_ids, int t, uint8_t* d_done, int batch,
                      int pad_id, int eos_id, int32_t* d_running, void* stream);
/* One beam-search step's bookkeeping on the device -- what transformers' GenerationMixin._beam_search does between two decoder
 * steps (running beams of the next step, finished list, early-stop heuristic; kzv/beam.py states it in torch ops and is pinned
 * against HF on the CPU).  State arrays live in caller memory for the whole generation; token rows are double-buffered (the
 * caller swaps run_seq_in/out and fin_seq_in/out after every call).  `cur` = index of the token being chosen (1 = first after
 * BOS).  Outputs: d_rows [batch * num_beams] = the former flat row every running beam continues from (for kzv_decode_reorder),
 * d_flags [5]: [0..2] = {images whose open beams may still improve, images whose finished list is not full, images with a
 * continuation that did not stop}: the loop goes on iff flags[0] > 0 && !(early_stopping && flags[1] == 0) && flags[2] > 0.  That
 * test is also taken on the device: d_flags[3] becomes 1 when the search has ended and d_flags[4] holds the number of updates
 * applied; calls issued after the end change nothing (the caller may read d_flags only every few steps; the valid token rows are
 * then the buffers written by update number d_flags[4]).  The call with cur == 1 resets d_flags[3..4]. */
typedef struct kzv_beam_state {
    int32_t batch, num_beams, max_len, vocab, eos_id;
    const int64_t* run_seq_in; int64_t* run_seq_out;     /* [batch, num_beams, max_len] */
    const int64_t* fin_seq_in; int64_t* fin_seq_out;     /* [batch, num_beams, max_len] */
    float* run_scores; float* fin_scores;                /* [batch, num_beams] */
    uint8_t* fin_done; int64_t* fin_len;                 /* [batch, num_beams] */
    uint8_t* unsatisfied;                                /* [batch] */
    /* optional, all four or none (null = off: the launch is the one without them): the per-token log-probabilities of the token rows,
     * fp32 [batch, num_beams, max_len], double-buffered and swapped like them.  The lanes that copy a token row copy its log-probability
     * row the same way: the parent's row, plus top_scores[k] - run_scores[parent of k] (the scores BEFORE this call) at `cur` -- one fp32
     * subtraction, HF compute_transition_scores.  The caller zeroes both buffers before the first call. */
    const float* run_lp_in; float* run_lp_out;
    const float* fin_lp_in; float* fin_lp_out;
} kzv_beam_state;
int kzv_beam_update(const kzv_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, int cur, int early_stopping,
                    float length_penalty, int64_t* d_rows, int32_t* d_flags, void* stream);
/* kzv_beam_update for images that carry forced prefixes (kzv_force_prefix): d_prefix_len int32 [batch] holds every image's prefix length
 * and d_divisors fp32 [max_len + 1] the table n -> (float)pow(n, length_penalty) (entry 0 unused), since the generated length now differs
 * per image: g = max(cur - prefix_len[i], 1) is the divisor's index both for a hypothesis that ends at this step (cur + 1 - (1 + prefix_len))
 * and for the early-stop heuristic after it (the same number, as in kzv_beam_update).  The clamp to 1 is the rule for forced steps: there
 * g would be <= 0, nothing can finish (a prefix holds no EOS and ends before max_len - 1), so only the running-beam part of the update
 * has an effect and the image stays unsatisfied (0 / 1 > -1e9).  A null d_prefix_len is kzv_beam_update itself (today's kernel instance; d_divisors is
 * then not read).  The length table is an argument of its own, not a field of kzv_beam_state, whose layout stays what it was. */
int kzv_beam_update_prefix(const kzv_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, int cur, int early_stopping,
                           float length_penalty, const float* d_divisors, const int32_t* d_prefix_len, int64_t* d_rows, int32_t* d_flags, void* stream);
/* The same step replayed from a hipGraph (the eager step is ~100 small launches and host-bound at ~0.85 ms per token):
 * the step index lives in device memory -- kzv_decode_begin resets it to 0, every kzv_decode_step_graph runs step t and
 * leaves t + 1 -- so one instantiated graph serves every step of a generation.  The graph is captured on the first call
 * and re-captured whenever a buffer pointer (or the cache copy in use after kzv_decode_reorder) differs from the captured
 * one: keep d_tokens / d_posids / d_valid / d_logits in fixed buffers.  `stream` must not be the default stream.  The
 * active image width / weights must not change between kzv_decode_begin and the last step. */
int kzv_decode_begin(kzv_model* m, void* stream);
/* How a step runs (both entry points).  1 (default; KZV_DECODE_ONE_LAUNCH): for the reference decoder's geometry -- hidden 256, 4
 * heads, FFN 768, <= 128 cached and <= 320 patch keys, 1 / 2 / 4 rows per image -- embeddings, all layers and the LM head's dense
 * layer are ONE launch (csrc/decode_fused.hip: a workgroup per image owns its beams through every layer), followed by the
 * vocabulary GEMM; up to 160 patch keys go through the attention waves' registers in one pass, 161 .. 320 in chunks with an online
 * softmax.  0, or any other geometry: one launch per operation (~50 per token).  Same results up to fp32 summation order.
 * -1 returns to the environment's default.  The fragment-ordered weight copies the one-launch step reads (9.6 MB) are refreshed by
 * the first step after kzv_model_sync_weights. */
int kzv_set_decode_one_launch(int on);
/* Which of the two the next kzv_decode_step / kzv_decode_step_graph on this handle runs: 1 = the one-launch kernel, 0 = one launch
 * per operation.  Answers for the bound rows, the images of the last kzv_encode_images / forward, the active image width and the
 * current kzv_set_decode_one_launch mode; launches nothing.  A negative error before kzv_model_bind. */
int kzv_decode_step_impl(const kzv_model* m);
/* Generation from e4m3 decoder weights (opt-in; the default is bf16).  With KZV_DECODE_WEIGHTS_E4M3 the one-launch step reads the
 * eight linears it streams per decoder layer (self query | key | value, self output, cross query, cross output, fc1, fc2) and the LM
 * head's dense layer as OCP e4m3 with one POWER-OF-TWO scale per output row -- s = the smallest 2^e with amax(row) / s <= 448,
 * q = e4m3(w / s) rounded to nearest even from the bf16 weight -- widens them to bf16 in registers and runs the same bf16 MFMAs in
 * the same order; activations, attention, LayerNorm, the KV cache, the cross key / value projection, the vocabulary GEMM, every
 * bias and all of training are untouched.  q * s is a bf16 number and the scale commutes with every fp32 rounding, so the step's
 * logits EQUAL, bit for bit, those of the bf16 one-launch step on a model whose nine weights were replaced by q * s
 * (kzv/quant.py: dequantised_decoder_weights); how far that is from the original model is a property of the checkpoint.  Only the
 * one-launch step has this path: wherever kzv_decode_step_impl answers 0 the step keeps reading bf16, silently.  The e4m3 copies
 * (4.7 MB at 12 layers) are made by the first step after the format is chosen and after every kzv_model_sync_weights, in one
 * launch.  Any time after kzv_model_create; a format other than the two is KZV_E_ARG. */
#define KZV_DECODE_WEIGHTS_BF16 0
#define KZV_DECODE_WEIGHTS_E4M3 1
int kzv_set_decode_weights(kzv_model* m, int format);
int kzv_get_decode_weights(const kzv_model* m);      /* the format asked for; a negative error for a null handle */
/* What the next kzv_decode_step / kzv_decode_step_graph on this handle will actually read: KZV_DECODE_WEIGHTS_E4M3 only where the
 * format was asked for AND kzv_decode_step_impl answers 1.  Launches nothing; a negative error before kzv_model_bind. */
int kzv_decode_weights_impl(const kzv_model* m);
/* The quantiser by itself (per-op tests): w_bf16 [N, K] row-major bf16 on the device (N % 16 == 0, K % 64 == 0) -> q_out [N, K]
 * row-major e4m3 bytes and scale_out [N] fp32, by the recipe above; an all-zero row keeps scale 1, a row whose amax lies below
 * 2^-118 scale 2^-126.  (The generation step keeps its own copy in the order its waves consume it; that layout is internal.) */
int kzv_quant_pack_e4m3(const void* w_bf16, int N, int K, void* q_out, float* scale_out, void* stream);
/* Training / evaluation forward: the linear chains of a decoder layer -- [output projection + dropout + residual -> LayerNorm ->
 * cross query] and [output projection -> LayerNorm -> fc1 + GELU -> fc2 -> LayerNorm -> the next layer's QKV] -- as TWO launches
 * per layer (csrc/decoder_chain.hip; hidden 256, 4 heads, FFN 768) instead of nine.  0: one launch per operation; 1: the forward
 * chains (+ the decoder's 256 x 256 input-gradient GEMMs on the row-panel kernel); 2 (default; KZV_DEC_CHAIN): also the BACKWARD's three
 * row-local segments per layer (input-gradient GEMM + residual gradient -> LayerNorm backward -> dropout mask -> input-gradient GEMM) as
 * one launch each, 13 -> 6 launches per layer; -1: the environment's default.  Same tensors, same rounding points, same dropout bits:
 * logits bit-identical across the three modes, gradients equal up to float-atomic order. */
int kzv_set_dec_chain(int on);
/* Training / validation forward without returned logits: lm_head.decoder (HF modeling_roberta.py:888-893, tied weight) + log-softmax +
 * NLL (src/models/trocr_model.py:256,292) + the bf16 gradient of the logits as ONE launch; the [B*T, vocab] fp32 logits are never written
 * (csrc/cross_entropy.hip head_ce_kernel: 64 rows per workgroup against the whole vocabulary twice, online softmax statistics; decoder
 * hidden 256).  1 (default; KZV_HEAD_CE), 0: head GEMM + ce_kernel, -1: the environment's default.  kzv_forward_loss with d_logits != NULL
 * always takes the GEMM (it returns them).  Same arithmetic up to fp32 summation order. */
int kzv_set_head_ce(int on);
/* Label smoothing of the training loss (an extension: the reference's criterion is plain CrossEntropyLoss; the published TrOCR recipe
 * smooths with 0.1): kzv_forward_loss(train != 0) computes torch.nn.functional.cross_entropy(logits, target, ignore_index = pad,
 * label_smoothing = eps), mean over the scored rows, V = the real vocabulary:
 *   loss_row = lse(z) - (1 - eps) z[y] - (eps / V) sum_{v < V} z[v];   dlogits[v] = (softmax(z)[v] - (1 - eps) [v == y] - eps / V) / count
 * on whichever path runs (the one-launch head or head GEMM + ce_kernel).  kzv_forward_loss(train == 0) keeps the plain NLL whatever eps
 * is: validation losses rank checkpoints and stay comparable between runs.  Per handle, 0 after kzv_model_create (the kernels as they
 * were: smoothing is a compile-time variant), in force from the next kzv_forward_loss.  KZV_E_ARG unless 0 <= eps < 1. */
int kzv_set_label_smoothing(kzv_model* m, float eps);
float kzv_get_label_smoothing(const kzv_model* m);      /* 0 for a null handle */
/* Class weights and the focal term of the training loss (extensions, for a vocabulary with a long tail; off after kzv_model_create, and off
 * launches the kernels that run without them).  Over the scored rows i (target y_i = labels[b][t + 1] != pad), with p_ic = softmax(z_i)[c],
 * p_i = p_i,y_i, nll_i = lse_i - z_i[y_i], w fp32 [vocab] finite and > 0 (none: w = 1), W = sum_i w[y_i], S_w = sum_c w[c], eps the label
 * smoothing, V the real vocabulary:
 *   gamma = 0: F.cross_entropy(z, y, weight = w, ignore_index = pad, label_smoothing = eps)
 *     loss          = sum_i [ (1 - eps) w[y_i] nll_i + (eps / V) (S_w lse_i - sum_c w[c] z_ic) ] / W
 *     dlogits[i][c] = [ ((1 - eps) w[y_i] + (eps / V) S_w) p_ic - (1 - eps) w[y_i] [c == y_i] - (eps / V) w[c] ] / W
 *   gamma > 0 (focal; eps must be 0):
 *     loss          = sum_i w[y_i] (1 - p_i)^gamma nll_i / W
 *     dlogits[i][c] = w[y_i] g_i (p_ic - [c == y_i]) / W,   g_i = (1 - p_i)^gamma + gamma (1 - p_i)^(gamma - 1) p_i nll_i
 *     with nll_i clamped at 0, 1 - p_i = -expm1(-nll_i), and g_i = 0 where 1 - p_i = 0.
 * dlogits is exactly zero in pad-target rows and in the padded columns.  W and S_w are summed on the device in a fixed order
 * (kzv_target_weight_sum): 1 / W scales every gradient of the step.  kzv_forward_loss(train == 0) keeps the plain NLL whatever is set, as
 * with label smoothing.  Under data parallelism every rank normalises by its own W.
 * kzv_set_class_weights: n == vocabulary, the values are copied into device memory the handle owns (it waits for the device first);
 *   (NULL, 0) clears them.  A wrong n or a value that is not finite and > 0: KZV_E_ARG, nothing changes.
 * kzv_get_class_weights: the number of weights written to host_out (room for n), 0 when none are set.
 * kzv_set_focal_gamma: 0 <= gamma <= 5, else KZV_E_ARG; KZV_E_ARG too when gamma > 0 meets a label smoothing > 0, and
 *   kzv_set_label_smoothing refuses the reverse order. */
int kzv_set_class_weights(kzv_model* m, const float* host_weights, int n);
int kzv_get_class_weights(const kzv_model* m, float* host_out, int n);
int kzv_set_focal_gamma(kzv_model* m, float gamma);
float kzv_get_focal_gamma(const kzv_model* m);          /* 0 for a null handle */
int kzv_decode_step_graph(kzv_model* m, const int64_t* d_tokens, const int32_t* d_posids, const uint8_t* d_valid, int64_t ld_valid,
                          float* d_logits, void* stream);

/* ---- Slot-refill greedy decoding of many images (opt-in; kzv/stream.py states the bookkeeping in torch ops) ------------------------
 * A fixed set of decoder SLOTS (the bound batch: one workgroup of the one-launch step each) works through a WAVE of n_images images
 * whose cross-attention K/V sit in a pool in decode layout: a slot whose line has ended takes the next unseated image and restarts at
 * BOS in the very next step, so no step is spent on an ended line while images wait.  Selection and seating run on the device; the
 * host only polls a counter.  Greedy only; per image the tokens are those of the lockstep greedy generation.
 *
 * The bookkeeping by itself (per-op tests): the state arrays live in caller memory.  kzv_stream_seat_first gives the first
 * min(slots, n_images) images the slots in order (step 0, token bos_id, position id pad_id + 1), marks the rest idle (slot_image = -1)
 * and sets counters = {next unseated image, lines ended = 0, steps = 0}.  kzv_stream_update takes one step's logits [slots, ld]:
 *   per live slot (image i at step t): token = the first arg-max column; out_ids[i][t + 1] = token; out_logprob[i][t + 1] = max - lse
 *   (if given); the line has ended when token == eos_id, t + 2 >= limit[i] (if given) or t + 2 >= max_len;
 *   then, over all slots: the ended ones take images counters[0], counters[0] + 1, ... in ASCENDING SLOT ORDER (a prefix sum, no
 *   atomic ticket: the same assignment in every run) and restart at step 0, or go idle when no image is left; the others advance
 *   (slot_t + 1, their token, position id t + 2 + pad_id); counters += {images seated, lines ended, 1 while a line was open}.
 * limit [n_images] int32: the most tokens, BOS included, an image may get (values beyond max_len count as max_len, values below 2 as 2).
 * KZV_E_ARG: a null array other than out_logprob / limit, max_len < 2, rows shorter than max_len, ld < vocab. */
typedef struct kzv_stream_state {
    int32_t slots, n_images, max_len, vocab, bos_id, eos_id, pad_id, reserved;
    int32_t* slot_image; int32_t* slot_t;                /* [slots] */
    int64_t* tokens; int32_t* posids;                    /* [slots]: the next step's inputs */
    int32_t* counters;                                   /* [3]: next unseated image, lines ended, steps taken */
    int32_t* scratch;                                    /* [2 * slots]: selection -> seating */
    int64_t* out_ids; int64_t ld_ids;                    /* [n_images, ld_ids >= max_len]; the caller fills BOS / padding */
    float* out_logprob; int64_t ld_logprob;              /* optional [n_images, ld_logprob >= max_len] */
    const int32_t* limit;                                /* optional [n_images] */
} kzv_stream_state;
int kzv_stream_seat_first(const kzv_stream_state* st, void* stream);
int kzv_stream_update(const kzv_stream_state* st, const float* d_logits, int64_t ld, void* stream);
/* The alternatives of one step, from the same logits and BEFORE kzv_stream_update (which replaces slot_image / slot_t): per live slot
 * (image i at step t, t + 1 < max_len) d_alt_ids[i][t + 1][0..k) / d_alt_logprob[i][t + 1][0..k) = kzv_token_topk of the slot's row, so
 * entry 0 is the token kzv_stream_update emits and its out_logprob.  Idle slots write nothing; the caller fills the arrays (int32 / fp32
 * [n_images, ld_alt >= max_len * k]) beforehand.  Reads slots, n_images, max_len, vocab, slot_image and slot_t of the state only.  HF:
 * generate(output_scores=True) -> scores[t].log_softmax(-1).topk(k).  KZV_E_ARG as kzv_token_topk's, and for ld_alt < max_len * k. */
int kzv_stream_topk(const kzv_stream_state* st, const float* d_logits, int64_t ld, int k, int32_t* d_alt_ids, float* d_alt_logprob,
                    int64_t ld_alt, void* stream);
/* On the model handle (the bound batch = the slot count; the bound label length >= max_len).
 * kzv_stream_decode_impl: 1 where the bound geometry gets slot-refill decoding -- exactly where the one-launch step serves one row per
 * image (hidden 256, 4 heads, FFN 768, <= 12 layers, <= 128 cached and <= 320 patch keys) and kzv_set_decode_one_launch is on -- else 0;
 * launches nothing; KZV_E_STATE before kzv_model_bind.
 * kzv_stream_begin: a wave of n_images images over a pool of pool_images >= n_images entries (>= the slot count): checks, (re)allocates
 * the pool (the library's own, grow-only: Ld * 2 * pool_images * patches * hidden bf16), refreshes the weight packs after a weight
 * change, zeroes the head's input so that a never-used slot's vocabulary row stays finite.  d_out_ids [n_images, ld_ids] int64 must hold
 * BOS in column 0 and padding elsewhere.  KZV_E_ARG for a pool smaller than the slot count or the wave, null d_out_ids, max_len < 2 or
 * beyond the bound length, rows shorter than max_len -- nothing is launched then; KZV_E_STATE where kzv_stream_decode_impl says 0.
 * kzv_stream_encode: the encoder + cross K/V projection of n images (n divides the bound batch, as kzv_encode_images) into pool entries
 * first .. first + n - 1.
 * kzv_stream_start: seats the first images.  kzv_stream_step: one token for every live slot -- the one-launch step (slot instances:
 * csrc/decode_fused.hip), the vocabulary GEMM, selection and seating; with graph != 0 replayed from a hipGraph captured at the wave's
 * first step (a single chain of kernel nodes; `stream` must then not be the default stream).
 * kzv_stream_poll: lines ended and steps taken so far (one stream synchronise); the wave is done when *finished == n_images. */
int kzv_stream_decode_impl(const kzv_model* m);
int kzv_stream_begin(kzv_model* m, int pool_images, int n_images, int max_len, int bos_id, int eos_id, int64_t* d_out_ids, int64_t ld_ids,
                     float* d_out_logprob, int64_t ld_logprob, const int32_t* d_limit, void* stream);
int kzv_stream_encode(kzv_model* m, const float* d_pixel_values, int n, int first, void* stream);
int kzv_stream_start(kzv_model* m, void* stream);
int kzv_stream_step(kzv_model* m, int graph, void* stream);
int kzv_stream_poll(kzv_model* m, int32_t* finished, int32_t* steps, void* stream);
/* Alternatives for the greedy wave just begun: after kzv_stream_begin and before kzv_stream_start.  Every kzv_stream_step then runs
 * kzv_stream_topk between the vocabulary GEMM and selection -- one more kernel node of the same single chain -- into d_alt_ids /
 * d_alt_logprob [n_images, ld_alt >= max_len * k], which the caller has filled (-1 / 0) and keeps alive for the wave.  k = 0 switches it
 * off again; the next kzv_stream_begin clears it; when not set a step launches exactly what it launches without this call.  Launches
 * nothing itself.  KZV_E_STATE outside a begun greedy wave and for beam waves (a beam search's per-token candidates are not produced on the
 * slots; its per-token log-probabilities leave through kzv_stream_set_nbest); KZV_E_ARG for k outside 0..8, null arrays, ld_alt < max_len * k. */
int kzv_stream_set_topk(kzv_model* m, int k, int32_t* d_alt_ids, float* d_alt_logprob, int64_t ld_alt, void* stream);

/* ---- Beam search on the same slots (opt-in; kzv/stream.py: beam_select_seat / beam_stream state the bookkeeping in torch ops) ------------
 * Serves decoder.generate(num_beams = 4, early_stopping = True, max_length = 128) as the reference asks for it on every validation and
 * test image (src/models/trocr_model.py:306-316), over a whole dataset: a slot holds an image's whole beam GROUP (decoder rows slot *
 * num_beams .. + num_beams - 1) at its own step index and takes the next unseated image the step after its search has ended.  Beam
 * search is independent per image, so per image the result is that of the lockstep search (kzv_beam_update), in fewer steps.
 *
 * The bookkeeping by itself (per-op tests): the state lives in caller memory.  kzv_stream_beam_seat_first seats the first
 * min(slots, n_images) images, puts every slot's beam state at the start (running scores 0, -1e9, ...; finished scores -1e9, lengths 1,
 * unsatisfied; tokens bos_id at position id pad_id + 1; token rows BOS + padding) and sets counters = {next unseated image, 0, 0, 0}.
 * kzv_stream_beam_update takes one step's ranking (kzv_beam_topk over the slots: d_top_scores / d_top_index [slots, 2 * num_beams]):
 *   per live slot (image i at cur = slot_t + 1): kzv_beam_update's step for that image alone with max_len = min(limit[i], max_len) and
 *   the divisor divisors[cur]; token rows, scores and the beam row table (rows, optional: new[b][j] = old[parent of b][j] for j <= slot_t)
 *   are updated in place.  The search has ended when the image is no longer unsatisfied, or its finished list is full and
 *   early_stopping, or every continuation stopped: then out_ids[i][:fin_len[0]] = fin_seq[0] and out_score[i] = fin_scores[0];
 *   then, over all slots: seating as kzv_stream_update does it, a reseated slot's beam state back at the start;
 *   counters += {images seated, searches ended, 1 while a search was open, running continuations that took pad_id}.
 * A running continuation that takes pad_id breaks what the slots assume (position id = step + 1 + pad_id, every cached key usable): it is
 * counted, and the caller decodes such a wave again with the lockstep search.
 * divisors: device fp32 [max_len + 1], entry n = (float)pow((double)n, (double)length_penalty) -- the value kzv_beam_update divides by.
 * KZV_E_ARG: a null array other than out_score / limit / rows, num_beams other than 2 or 4, max_len outside 2..128, output rows shorter
 * than max_len, row table rows shorter than max_len - 1. */
typedef struct kzv_stream_beam_state {
    int32_t slots, n_images, num_beams, max_len, vocab, bos_id, eos_id, pad_id, early_stopping;
    int32_t n_best;                                      /* 0 = off, else 1..num_beams: see the n-best fields below */
    int32_t* slot_image; int32_t* slot_t;                /* [slots] */
    int64_t* tokens; int32_t* posids;                    /* [slots * num_beams]: the next step's inputs */
    int64_t* run_seq; int64_t* fin_seq;                  /* [slots, num_beams, max_len] */
    float* run_scores; float* fin_scores;                /* [slots, num_beams] */
    uint8_t* fin_done; int64_t* fin_len;                 /* [slots, num_beams] */
    uint8_t* unsatisfied;                                /* [slots] */
    int32_t* counters;                                   /* [4] */
    int32_t* scratch;                                    /* [2 * slots]: update -> seating */
    int64_t* out_ids; int64_t ld_ids;                    /* [n_images, ld_ids >= max_len]; the caller fills BOS / padding */
    float* out_score;                                    /* optional [n_images]: HF sequences_scores */
    const int32_t* limit;                                /* optional [n_images] */
    const float* divisors;                               /* [max_len + 1] */
    int32_t* rows; int64_t ld_rows;                      /* optional beam row table [slots * num_beams, ld_rows >= max_len - 1] */
    /* N-best (n_best in 1..num_beams; HF generate(num_return_sequences = n_best)): when image i's search ends, finished rows r = 0 ..
     * n_best - 1 go to row i * n_best + r of nbest_ids (only fin_len[r] tokens: the caller fills BOS / padding), nbest_scores and
     * nbest_len (tokens, BOS included).  A finished entry that never received a hypothesis writes no tokens, score -1e9 and length 0.
     * Row 0 is what out_ids / out_score get, which are written as before.
     * run_lp / fin_lp (optional, both or none, need n_best): fp32 [slots, num_beams, max_len], the per-token log-probabilities of the
     * token rows, carried as kzv_beam_state's (seat_first zeroes them); with them nbest_logprob (optional) gets the rows' values, column
     * t = the log-probability of the token in column t, 0 in column 0 (the caller fills zeros).
     * KZV_E_ARG: n_best outside 0..num_beams, null ids / scores / lengths, rows shorter than max_len, any of these fields with n_best 0. */
    float* run_lp; float* fin_lp;
    int64_t* nbest_ids; int64_t ld_nbest;                /* [n_images * n_best, ld_nbest >= max_len] */
    float* nbest_scores; int32_t* nbest_len;             /* [n_images * n_best] */
    float* nbest_logprob; int64_t ld_nbest_logprob;      /* optional [n_images * n_best, ld_nbest_logprob >= max_len] */
} kzv_stream_beam_state;
int kzv_stream_beam_seat_first(const kzv_stream_beam_state* st, void* stream);
int kzv_stream_beam_update(const kzv_stream_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, void* stream);
/* kzv_stream_beam_update for a wave with forced prefixes: d_prefix_len int32 [n_images], indexed by IMAGE.  A slot holding image i at
 * cur = slot_t + 1 divides by divisors[max(cur - prefix_len[i], 1)] -- kzv_beam_update_prefix's rule, clamp included (forced steps do
 * the running-beam part only and stay unsatisfied).  Null: kzv_stream_beam_update itself, today's kernel instances. */
int kzv_stream_beam_update_prefix(const kzv_stream_beam_state* st, const float* d_top_scores, const int64_t* d_top_index, const int32_t* d_prefix_len,
                                  void* stream);
/* On the model handle: the bound batch = slots * num_beams decoder rows.
 * kzv_stream_beam_impl: 1 where the bound geometry gets beam search on slots -- where kzv_stream_decode_impl's conditions hold for
 * num_beams (2 or 4) rows per image, the bound batch is a multiple of num_beams and the vocabulary is within kzv_beam_topk's 16,384 --
 * else 0; launches nothing; KZV_E_STATE before kzv_model_bind.
 * kzv_stream_begin_beams: kzv_stream_begin for a wave of beam searches (generate's num_beams, early_stopping, length_penalty): lays the
 * beam state out in the handle's slot state, builds the divisor table, uses the handle's first beam row table.  d_out_scores: optional
 * fp32 [n_images].  d_out_logprob must be null (per-token log-probabilities of a beam search leave through kzv_stream_set_nbest).  Argument errors as
 * kzv_stream_begin's, before any launch; the pool must hold at least bound batch / num_beams images.
 * kzv_stream_encode / kzv_stream_start / kzv_stream_step / kzv_stream_poll then serve the wave as they serve a greedy one; a step is the
 * one-launch step (slot instances with 2 / 4 rows and the row table), the vocabulary GEMM, kzv_beam_topk and kzv_stream_beam_update, in
 * one captured graph.  kzv_stream_poll_beams: kzv_stream_poll plus the padding count (counters[3]). */
int kzv_stream_beam_impl(const kzv_model* m, int num_beams);
int kzv_stream_begin_beams(kzv_model* m, int num_beams, int early_stopping, float length_penalty, float* d_out_scores, int pool_images, int n_images,
                           int max_len, int bos_id, int eos_id, int64_t* d_out_ids, int64_t ld_ids, float* d_out_logprob, int64_t ld_logprob,
                           const int32_t* d_limit, void* stream);
int kzv_stream_poll_beams(kzv_model* m, int32_t* finished, int32_t* steps, int32_t* pad_tokens, void* stream);
/* N-best lists and per-token log-probabilities for the beam wave just begun: after kzv_stream_begin_beams and before kzv_stream_start
 * (as kzv_stream_set_topk for a greedy wave).  Every search that ends then also writes rows 0 .. n_best - 1 of its finished list to
 * d_ids [n_images * n_best, ld_ids] int64 (the caller has filled BOS / padding), d_scores fp32 and d_lengths int32 [n_images * n_best],
 * image-major, best first (kzv_stream_beam_state's n-best fields); row 0 is the wave's d_out_ids / d_out_scores row.  d_logprob:
 * optional fp32 [n_images * n_best, ld_logprob] (the caller has filled zeros): the handle then allocates the log-probability rows
 * beside its token rows and every step carries them (the LP instance of the update kernel); without it the step moves what it moves
 * without this call and only the end of a search writes more.  One captured graph still serves every step.  The setting belongs to
 * one wave: the next begin clears it.  Launches no kernel itself.  KZV_E_STATE outside a begun wave; KZV_E_ARG for a greedy wave, n_best
 * outside 1..num_beams, null ids / scores / lengths, a leading dimension shorter than max_len -- before any launch. */
int kzv_stream_set_nbest(kzv_model* m, int n_best, int64_t* d_ids, int64_t ld_ids, float* d_scores, int32_t* d_lengths, float* d_logprob,
                         int64_t ld_logprob, void* stream);
/* Generation controls for the wave just begun (greedy or beams): after kzv_stream_begin / kzv_stream_begin_beams and before
 * kzv_stream_start.  Every kzv_stream_step then runs kzv_logits_process as one more kernel node of the same single chain, between the
 * vocabulary GEMM and kzv_stream_topk / selection in a greedy wave (histories: the wave's out_ids); in a beam wave the normalising
 * kzv_logits_process plus kzv_beam_rank_logprobs take kzv_beam_topk's place (histories: the slots' running token rows).  The selection's
 * log-probabilities and the alternatives of kzv_stream_set_topk are then those of the processed row.  suppress_mask: optional HOST array
 * of (vocab + 31) / 32 words; the library keeps a device copy of its own, the caller's array need not outlive the call.  The setting
 * belongs to one wave: the next begin clears it.  With every control neutral (0, 1.0, 0, no mask bit set), or when not called, a step
 * launches exactly what it launches without this call.  Launches no kernel itself.  KZV_E_STATE outside a begun wave; KZV_E_ARG for null
 * controls, no_repeat_ngram_size outside 0..8, repetition_penalty <= 0, min_length < 0, a mask that suppresses EOS, a vocabulary beyond
 * 16,384, and in a beam wave a mask that leaves fewer than 2 tokens (the 2 * num_beams continuations a step ranks would not exist). */
typedef struct kzv_logits_controls {
    int32_t no_repeat_ngram_size;                        /* 0 = off, 1..8 */
    float repetition_penalty;                            /* > 0; 1 = off */
    int32_t min_length;                                  /* 0 = off; tokens, BOS included, before EOS may be chosen */
    int32_t reserved;
    const uint32_t* suppress_mask;                       /* optional, host */
} kzv_logits_controls;
int kzv_stream_set_controls(kzv_model* m, const kzv_logits_controls* controls, void* stream);
/* Language-model fusion for the wave just begun (greedy or beams): after kzv_stream_begin / kzv_stream_begin_beams and before
 * kzv_stream_start.  Every kzv_stream_step then runs kzv_lm_fuse as one more kernel node of the same single chain, after the controls'
 * node (if any) and before kzv_stream_topk / selection; a beam wave takes the normalise (kzv_logits_process, neutral controls when none
 * are set) -> fuse -> kzv_beam_rank_logprobs route in place of kzv_beam_topk.  The struct is copied; its tables stay the caller's device
 * memory and must outlive the wave.  The setting belongs to one wave: the next begin clears it.  weight == 0 switches it off: a step then
 * launches exactly what it launches without this call.  Launches no kernel itself.  KZV_E_STATE outside a begun wave; KZV_E_ARG for a
 * null struct or tables, a vocabulary different from the model's, an order outside 1..4 and a non-finite weight. */
int kzv_stream_set_lm(kzv_model* m, const kzv_ngram_lm* lm, float weight, void* stream);
/* Forced prefixes for the wave just begun (greedy or beams): after kzv_stream_begin / kzv_stream_begin_beams and before kzv_stream_start.
 * d_prefix int64 [n_images, ld_prefix] and d_prefix_len int32 [n_images] are kzv_force_prefix's tables, indexed by the wave's image
 * numbers; d_forced_logprob (optional) fp32 [n_images, ld_forced_logprob > ld_prefix] receives the model's own log-probability of every
 * forced token at column cur (the caller has filled zeros).  All three are caller-owned device memory that must outlive the wave.  Every
 * kzv_stream_step then runs kzv_force_prefix as one more kernel node of the same single chain, after the language model's node (if any)
 * and before kzv_stream_topk / selection, on each slot's own image and step: a slot that is reseated reads the new image's prefix from
 * step 0.  A beam wave takes the normalise -> (fuse) -> force -> kzv_beam_rank_logprobs route, as kzv_stream_set_lm's, and updates through
 * kzv_stream_beam_update_prefix.  The lengths live on the device, so the library cannot see them: ld_prefix (the longest prefix) is what
 * it checks against max_len, and ld_prefix == 0 -- every prefix empty -- switches the setting off: a step then launches exactly what it
 * launches without this call.  The setting belongs to one wave: the next begin clears it.  Launches no kernel itself.  KZV_E_STATE outside
 * a begun wave; KZV_E_ARG for a null prefix or length table (with ld_prefix > 0), ld_prefix < 0, 1 + ld_prefix > max_len - 1 (a prefix that
 * reaches max_len - 1 leaves no token to generate), a vocabulary beyond 16,384 and forced_logprob rows not longer than ld_prefix. */
int kzv_stream_set_prefix(kzv_model* m, const int64_t* d_prefix, int64_t ld_prefix, const int32_t* d_prefix_len, float* d_forced_logprob,
                          int64_t ld_forced_logprob, void* stream);

/* loss.backward() for the step above: fills the bound fp32 grad buffer (which must be zero on entry;
 * kzv_zero_grads does that).  Backward is split in `kzv_backward_segments()` segments so the host can
 * launch an RCCL all-reduce for a segment's finished gradients while later segments still run
 * (Lightning DDP bucket overlap, scripts/train_trocr.py:166-169).  After segment s returns (work
 * enqueued on `stream`), grads in [lo, hi) of kzv_backward_segment_range(s) are final. */
int kzv_zero_grads(kzv_model* m, void* stream);
int kzv_backward_segments(const kzv_model* m);
int kzv_backward_segment(kzv_model* m, int seg, void* stream);
int kzv_backward_segment_range(const kzv_model* m, int seg, int64_t* lo, int64_t* hi);
int kzv_backward(kzv_model* m, void* stream);               /* all segments */
/* Frozen bottom of the encoder (fine-tuning), 0 <= n <= encoder layers, 0 (the default) = everything trains.  n > 0 freezes the patch
 * embedding, the CLS token, the position table and encoder layers 0 .. n-1: kzv_backward and kzv_backward_segment launch NOTHING for
 * segments > Le - n and return KZV_OK, so those gradients stay what kzv_zero_grads left; the last segment that runs joins the side
 * stream as the embedding segment does otherwise.  The encoder's final LayerNorm, proj and the decoder (segment 0) always train.  The
 * forward is unchanged (dropout stays on in frozen layers in train mode); kzv_backward_segment_range is unchanged.  The optimizer must
 * be told separately (lr_scale 0 over the same range in kzv_clip_and_step_groups), or weight decay and the z iterate still move the
 * frozen parameters.  KZV_E_ARG: null model, n out of range; get returns 0 for a null handle. */
int kzv_set_frozen_encoder_layers(kzv_model* m, int n);
int kzv_get_frozen_encoder_layers(const kzv_model* m);

/* gradient_clip_val (scripts/train_trocr.py:175) + RAdamScheduleFree.step (trocr_model.py:412-421),
 * fused over the flat buffers.  d_z, d_v: optimizer state (z iterate, second moment), same layout.
 * d_scratch: >= 4 KiB fp32 scratch (partial norms).  Host supplies the step scalars (kzv/optim.py). */
typedef struct kzv_opt_step {
    float lr_t;          /* lr * RAdam rectification for this step (0 in the silent phase) */
    float ckp1;          /* schedule-free averaging weight c_{k+1} */
    float beta1, beta2, eps, weight_decay;
    float bias_correction2;
    int32_t adaptive;    /* 1 once rho_t > 4 (use v), else plain (silent) step */
    float max_grad_norm; /* <= 0 disables clipping */
    float grad_scale;    /* multiplied into grads before everything (1/world for DDP mean) */
    float one_minus_beta2; /* 1 - beta2 evaluated in double on the host, as torch's addcmul_(value=1 - beta2) does: in fp32
                            * 1.f - 0.999f is off by 1.3e-5 relative, a bias on every second-moment entry */
} kzv_opt_step;
int kzv_grad_sqnorm(const float* d_grads, int64_t n, float* d_out1, float* d_scratch, void* stream);
int kzv_clip_and_step(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                      const float* d_sqnorm, const kzv_opt_step* s, void* stream);
/* The same step with the EMA of the parameters (src/callbacks/ema.py:51-58: shadow = decay * shadow + (1 - decay) * param
 * after every batch) updated in the same pass from the freshly stepped parameters; d_ema NULL = no EMA. */
int kzv_clip_and_step_ema(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                          const float* d_sqnorm, const kzv_opt_step* s, float* d_ema, float ema_decay, void* stream);
/* Parameter groups (fine-tuning): the same norm and the same step over a table of ranges of the flat buffer, each with a factor on
 * the learning rate and one on the weight decay.  The table is DEVICE memory: sorted, contiguous, covering [0, n) exactly, every
 * boundary a multiple of 64 floats (the parameter table guarantees it), 1 <= n_groups <= KZV_OPT_MAX_GROUPS.  Its contents cannot be
 * checked here without reading the device: kzv.optim.check_groups does it on the host before the upload; a table that breaks these
 * rules gives wrong scales, never an access outside the buffers.
 *   per element of a group: kzv_clip_and_step's arithmetic with lr_t * lr_scale (both places lr_t enters) and weight_decay * wd_scale;
 *     ckp1 is shared by all groups (a scale constant in time cancels in schedulefree's weight / weight_sum).
 *   lr_scale == 0: FROZEN.  p, z, v and the EMA shadow of the range are neither read nor written (v does not decay), its gradients do not
 *     enter the norm (torch's clip_grad_norm_ sees only parameters that have a gradient), so the clip coefficient is the trainable
 *     groups' own.
 *   one group (1, 1): the bits of kzv_grad_sqnorm / kzv_clip_and_step_ema.  The norm's sum order is fixed: the same bits from run to run.
 * One launch whatever n_groups is, the plain kernels' bytes per trainable parameter.  KZV_E_ARG: a null pointer (d_ema and, without
 * clipping, d_sqnorm may be null), n % 4 != 0, n_groups outside its range, an EMA decay outside [0, 1]. */
#define KZV_OPT_MAX_GROUPS 4096
typedef struct kzv_opt_group { int64_t lo, hi; float lr_scale, wd_scale; } kzv_opt_group;   /* floats [lo, hi) */
int kzv_grad_sqnorm_groups(const float* d_grads, int64_t n, const kzv_opt_group* d_groups, int n_groups,
                           float* d_out1, float* d_scratch, void* stream);
int kzv_clip_and_step_groups(float* d_params, float* d_z, float* d_v, const float* d_grads, int64_t n,
                             const float* d_sqnorm, const kzv_opt_step* s, const kzv_opt_group* d_groups, int n_groups,
                             float* d_ema, float ema_decay, void* stream);
/* optimizer.eval()/train() parameter swap (trocr_model.py:423-451): p <- p + w*(z - p) */
int kzv_lerp_params(float* d_params, const float* d_z, int64_t n, float w, void* stream);

/* -------------------------------------------------------- per-op entry points (unit parity tests) */
enum { KZV_EPI_BF16 = 0, KZV_EPI_F32 = 1,
       KZV_EPI_GELU = 2,       /* C = gelu_erf(acc + bias) bf16, aux = gelu_erf'(acc + bias) bf16 (saved for backward) */
       KZV_EPI_RESID = 3,      /* C = dropout(acc + bias) + resid, fp32 */
       KZV_EPI_DGELU = 4,      /* C = acc * aux, bf16 (aux = the derivative saved by the forward GELU epilogue) */
       KZV_EPI_GELU_F32 = 5    /* like GELU but C is fp32 (feeds a LayerNorm) */ };

/* C[M,N] = A[M,K] . B[N,K]^T (+bias) with a fused epilogue; bf16 operands, fp32 accumulate (MFMA).
 * Replaces every nn.Linear forward / input-gradient on the path. */
typedef struct kzv_gemm_nt_args {
    const void* A; int64_t lda;       /* bf16 [M,K] */
    const void* B; int64_t ldb;       /* bf16 [n_valid,K] */
    void* C; int64_t ldc;             /* bf16 or fp32 [M,N] by epilogue */
    const float* bias;                /* fp32 [n_valid] or NULL */
    const float* resid; int64_t ldr;  /* KZV_EPI_RESID: fp32 [M,N] */
    void* aux; int64_t ldaux;         /* GELU: bf16 gelu'(pre-activation) OUT (what backward needs); DGELU: the same IN */
    int32_t M, N, K, n_valid;         /* N = columns stored (mult of 4), rows of B >= n_valid read as 0 */
    float drop_p; uint32_t drop_key;  /* KZV_EPI_RESID dropout on (acc+bias); p=0 -> off */
} kzv_gemm_nt_args;
int kzv_gemm_nt(const kzv_gemm_nt_args* a, int epilogue, void* stream);
/* kzv_gemm_nt picks a kernel by shape: the LDS-staged 128x128 / 256x256 kernels, except for M <= rows_max_m (default 0 =
 * never; KZV_ROWS_MAX_M), which takes the few-rows kernel the generation step (kzv_decode_step*) uses internally for its
 * M = batch GEMMs (one wave per 16x64 tile).  The per-op tests raise the threshold to check that kernel through this entry. */
int kzv_set_rows_max_m(int n);
/* K-loop schedule of the persistent 256x256 kernel behind kzv_gemm_nt (large shapes, one-store epilogues): 0 = eight-phase
 * ping-pong (gemm_nt256p.hip), 1 = free-running, two barriers per K-tile (gemm_nt256f.hip).  Same results bit for bit (same
 * per-accumulator summation order).  Default: KZV_NT_FREE (environment) or the library's choice; n < 0 restores the default. */
int kzv_set_nt_schedule(int n);
/* Bit 1 of the schedule (n = 2, 3): the epilogues whose bit is set in `mask` (1 << KZV_EPI_*; default all) run on the four-wave
 * 256x128 kernel, two workgroups per CU out of phase so that one's drain overlaps the other's K loop (gemm_nt256h.hip; shapes
 * with K % 384 == 0, others keep the 256x256 kernels).  Same results bit for bit.  `us`: how late the second workgroup of a CU
 * starts (microseconds, ~; KZV_NTH_STAGGER, default 8). */
int kzv_set_nt_half_epilogues(int mask);
int kzv_set_nt_half_stagger(int us);
/* The same choice for the 256x256 weight-gradient kernel behind kzv_gemm_tn (gemm_tn256.hip; KZV_TN_FREE). */
int kzv_set_tn_schedule(int n);
/* The generation step's GEMMs with the decoder's LayerNorms folded in (hidden size 256): RoBERTa is post-LN, so every sub-layer
 * output s is normalised once and LN(s) feeds one GEMM as A and one later residual add; at M = batch rows the consumers normalise
 * themselves instead of a LayerNorm launch per sub-layer.  ln_a != NULL: A = LN(ln_a [M,256]) (K must be 256; A is ignored);
 * ln_r != NULL: the RESID epilogue's residual = LN(ln_r [M,256]) (N must be 256).  Epilogues: BF16, F32, GELU, GELU_F32 with
 * ln_a; RESID with ln_r.  Same arithmetic as kzv_layernorm_fwd + kzv_gemm_nt up to summation order. */
typedef struct kzv_gemm_rows_ln_args {
    const void* A; int64_t lda;       /* bf16 [M,K] or NULL with ln_a */
    const void* B; int64_t ldb;       /* bf16 [n_valid,K] */
    void* C; int64_t ldc;
    const float* bias;
    void* aux; int64_t ldaux;         /* GELU / GELU_F32 */
    int32_t M, N, K, n_valid;
    const float* ln_a; const float* ln_a_gamma; const float* ln_a_beta;
    const float* ln_r; const float* ln_r_gamma; const float* ln_r_beta;
    float eps;
} kzv_gemm_rows_ln_args;
int kzv_gemm_rows_ln(const kzv_gemm_rows_ln_args* a, int epilogue, void* stream);

/* ---- fp8 weight path (BASELINE.json configs[4]: "fp8 MFMA weight path on CDNA4"; beyond the reference, which has no fp8) ----
 * C[M,N] = (A8[M,K] . B8[N,K]^T) * a_scale[m] * b_scale[n] (+bias) with the BF16 / GELU / RESID / DGELU epilogue of kzv_gemm_nt.
 * A8, B8: OCP e4m3 bytes; row m of A8 holds A[m,:] / a_scale[m] (likewise B8 / b_scale).  fp32 accumulate on the block-scaled
 * MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales): twice the bf16 MFMA rate.  K % 256 == 0.
 * GELU only: when c8 is set, a second copy of C as e4m3, quantised with the per-tensor multiplier *c8_qscale (device scalar),
 * feeds the next GEMM; max |C| is folded into *c8_amax (atomic max), from which the caller derives the next multiplier. */
typedef struct kzv_gemm_nt_fp8_args {
    const void* A; int64_t lda;       /* e4m3 [M,K] */
    const void* B; int64_t ldb;       /* e4m3 [n_valid,K] */
    const float* a_scale;             /* fp32 [M] */
    const float* b_scale;             /* fp32 [n_valid] */
    void* C; int64_t ldc;             /* bf16 (BF16, GELU) or fp32 (RESID) [M,N] */
    const float* bias;                /* fp32 [n_valid] or NULL */
    const float* resid; int64_t ldr;  /* RESID: fp32 [M,N] */
    void* aux; int64_t ldaux;         /* GELU: bf16 gelu'(pre-activation) OUT */
    void* c8; int64_t ldc8;           /* GELU: optional e4m3 [M,N] OUT */
    const float* c8_qscale; float* c8_amax;
    int32_t M, N, K, n_valid;
    float drop_p; uint32_t drop_key;  /* RESID dropout on (acc*scales+bias) */
    const float* c8_rowq;             /* DGELU: fp32 [M], c8[m,:] = e4m3(C[m,:] * c8_rowq[m]) (required with DGELU) */
} kzv_gemm_nt_fp8_args;
int kzv_gemm_nt_fp8(const kzv_gemm_nt_fp8_args* a, int epilogue, void* stream);
/* q[r,:] = e4m3(x[r,:] * 448 / amax_r), scale[r] = amax_r / 448 (1 for an all-zero row); cols % 4 == 0.  The quantiser of the
 * weight copies (per output row) and, fused into LayerNorm, of its output rows. */
int kzv_quant_rows_fp8(const float* x, int64_t rows, int64_t cols, void* q, float* scale, void* stream);
/* kzv_layernorm_fwd that also writes the e4m3 copy of each output row and its scale. */
int kzv_layernorm_fwd_fp8(const float* x, const float* gamma, const float* beta, void* y_bf16, void* y_fp8, float* y_scale,
                          float* stats, int rows, int H, float eps, void* stream);
/* Model switch (call before kzv_model_bind; encoder hidden and ffn must be multiples of 256): 1 = the encoder's QKV, fc1 and fc2
 * forward GEMMs run on e4m3 operands (weights quantised per output row at kzv_model_sync_weights; LayerNorm outputs per token
 * row; GELU outputs per tensor with the previous forward's amax); 2 = also the MLP's two input-gradient GEMMs (transposed e4m3
 * weights; gradient rows quantised by their amax in the LayerNorm backward, and per row by a norm bound in the DGELU epilogue).
 * Everything else -- weight gradients, attention, the decoder -- stays bf16. */
int kzv_set_fp8(kzv_model* m, int mode);
int kzv_get_fp8(const kzv_model* m);
/* Parity hook: the per-tensor multipliers the last forward quantised each encoder layer's GELU output with -> d_out[enc_layers]. */
int kzv_fp8_act_scales(const kzv_model* m, float* d_out, void* stream);

/* OUT[N,K] (+)= P[Mtok,N]^T . Q[Mtok,K]   (weight gradient).  fp32 MFMA accumulation; small outputs add their token splits with
 * fp32 atomics, outputs of >= 9 tiles of 256 x 256 pass each split's partial tile through a workspace rounded to bf16 and fold them
 * in fp32 in a fixed order (bit-identical from run to run; error <= 2^-9 of a split's partial sum -- the reference's autocast GEMM
 * rounds the whole weight gradient to bf16). */
typedef struct kzv_gemm_tn_args {
    const void* P; int64_t ldp;       /* bf16 [Mtok, N] */
    const void* Q; int64_t ldq;       /* bf16 [Mtok, K] */
    float* OUT; int64_t ldo;          /* fp32 [n_store, K] accumulated into */
    int32_t Mtok, N, K, n_store;
    float* dbias;                     /* optional fp32 [n_store]: += column sums of P (bias gradient) */
} kzv_gemm_tn_args;
int kzv_gemm_tn(const kzv_gemm_tn_args* a, void* stream);

/* A Linear's input gradient (kzv_gemm_nt arguments, epilogue BF16 / F32 / RESID / DGELU) and weight gradient (kzv_gemm_tn arguments) from
 * the same dY as ONE launch when both take the 256x256 kernels (>= 256 output tiles of the first, >= 9 of the second, 256 CUs): every
 * workgroup runs its gemm_nt tiles and then a token range of one weight-gradient tile, sized on the host so that all workgroups finish
 * together -- the two launches each end on a partly filled round otherwise.  Falls back to the two separate launches.  The gemm_nt
 * result is bit-identical to kzv_gemm_nt's; the weight gradient differs by the bf16 rounding of its partial tiles (other token splits).
 * model.cpp's encoder backward calls it per nn.Linear (HF vit:192-254).  OFF by default (kzv_set_pair(1) / KZV_PAIR=1 turn it on):
 * measured +0.4 % img/s on the training step, one kernel boundary per pair and nothing from the balancing. */
int kzv_gemm_dgrad_wgrad(const kzv_gemm_nt_args* nt, int epilogue, const kzv_gemm_tn_args* tn, void* stream);
int kzv_set_pair(int on);

/* What would run a kzv_gemm_nt / kzv_gemm_tn call, without running it (in the spirit of kzv_attn_impl_ex): the kernel and its launch
 * geometry under the switches in force (the kzv_set_* above, the KZV_* environment, kzv_set_cu_reserve).  The same host function
 * decides for the launching entries (csrc/gemm_plan.h).  The arguments are validated exactly as kzv_gemm_nt / kzv_gemm_tn validate
 * them (same codes, same kzv_last_error text); no memory is read and no device is touched when cus > 0.
 * in_rows_scope: answer for a call from inside the generation step (few-rows kernel up to M = 4096).  cus: compute units to plan
 * for; <= 0 = the current device's.  A KZV_GEMM_TN256* plan still needs a workspace at launch: without one the call runs TN128. */
enum { KZV_GEMM_ROWS = 0,        /* gemm_rows.hip: one wave per 16x64 tile (grid x grid_y) */
       KZV_GEMM_NT256H = 1,      /* gemm_nt256h.hip: four waves, 256x128 tiles, persistent */
       KZV_GEMM_NT256F = 2,      /* gemm_nt256f.hip: 256x256 tiles, persistent, free-running K loop */
       KZV_GEMM_NT256P = 3,      /* gemm_nt256p.hip: 256x256 tiles, persistent, eight-phase K loop */
       KZV_GEMM_NT256 = 4,       /* gemm_nt256.hip: one 256x256 tile per workgroup */
       KZV_GEMM_NT128 = 5,       /* gemm.hip: one 128x128 tile per workgroup */
       KZV_GEMM_NT256P_F8 = 6,   /* gemm_nt256p.hip on e4m3 operands (kzv_gemm_nt_fp8; never a kzv_gemm_nt_plan answer) */
       KZV_GEMM_TN256F = 7,      /* gemm_tn256.hip: 256x256 tiles x token splits, free-running stages */
       KZV_GEMM_TN256 = 8,       /* gemm_tn256.hip: the same on the eight-phase schedule */
       KZV_GEMM_TN128 = 9        /* gemm.hip: 128x128 tiles x token splits, atomics epilogue */ };
typedef struct kzv_gemm_plan_info {
    int32_t kernel;               /* KZV_GEMM_* */
    int32_t grid, grid_y, block;  /* workgroups (x, y) and threads per workgroup */
    int32_t tiles;                /* output tiles of the kernel's tile shape */
    int32_t splits, chunk;        /* gemm_tn: token splits and tokens per split; gemm_nt: 0 */
    int32_t pair;                 /* 1: as one half of a kzv_gemm_dgrad_wgrad call this call meets its half of the one-launch form's
                                   * conditions (kzv_set_pair, shapes); when both halves say 1 the two run as ONE launch instead */
} kzv_gemm_plan_info;
int kzv_gemm_nt_plan(const kzv_gemm_nt_args* a, int epilogue, int in_rows_scope, int cus, kzv_gemm_plan_info* out);
int kzv_gemm_tn_plan(const kzv_gemm_tn_args* a, int cus, kzv_gemm_plan_info* out);

/* The same two products on fp32 OPERANDS (A, B, P, Q are float; leading dimensions in elements, multiples of 4; K % 32 == 0 for
 * the NT form), on the f32-input matrix instruction: exact fp32 products, fp32 accumulation (csrc/gemm_f32.hip).  For the model of
 * ocr_lightning/model.py, which the reference trains in fp32 (ocr_lightning/train.py:132-140; its own test wants singles ==
 * batched at 1e-6, ocr_lightning/tests/test_model.py:48-76).  kzv_gemm_nt_f32 takes the epilogues KZV_EPI_F32 and KZV_EPI_RESID
 * (no dropout); aux is ignored.  Launches with few output tiles split the reduction; the partial tiles are summed in a fixed order. */
int kzv_gemm_nt_f32(const kzv_gemm_nt_args* a, int epilogue, void* stream);
int kzv_gemm_tn_f32(const kzv_gemm_tn_args* a, void* stream);

/* LayerNorm over the last dim (fp32 statistics, eps inside rsqrt).  x fp32 [rows, H].
 * Replaces nn.LayerNorm in ViTLayer / RobertaLayer / heads. */
int kzv_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* y_f32,
                      float* stats /* [rows,2] mean,rstd */, int rows, int H, float eps, void* stream);
/* dx(+)= LN backward; dy bf16 or fp32; dgamma/dbeta accumulated (atomics). */
int kzv_layernorm_bwd(const void* dy, int dy_is_f32, const float* x, const float* stats, const float* gamma,
                      float* dx, int accumulate_dx, float* dgamma, float* dbeta, int rows, int H, void* stream);
/* The same two kernels with everything the model's call sites fuse into them (csrc/layernorm.hip; the fp8 copies keep their own
 * entry, kzv_layernorm_fwd_fp8).  seq / drop_first: the encoder's final LayerNorm drops the CLS token (trocr_model.py:200): rows
 * with row % seq == 0 write no output (their statistics are still written) and row r lands in output row r - r / seq - 1; the
 * backward reads dy at that row and treats the CLS rows' dy as zero.  drop_p / drop_key: hidden-state dropout on the forward's
 * OUTPUT (element index = output row * H + col), and in the backward on dy (same index) before anything else.  out16: optional
 * bf16 copy of the dx row the call stored (the total when accumulate_dx), masked with out_drop_p / out_drop_key at row * H + col. */
typedef struct kzv_ln_fwd_args {
    const float* x; const float* gamma; const float* beta;
    void* y_bf16; float* y_f32;       /* either may be NULL */
    float* stats;                     /* [rows, 2] mean, rstd, or NULL */
    int32_t rows, H, seq, drop_first;
    float eps, drop_p; uint32_t drop_key;
} kzv_ln_fwd_args;
int kzv_ln_fwd_ex(const kzv_ln_fwd_args* a, void* stream);
typedef struct kzv_ln_bwd_args {
    const void* dy; const float* x; const float* stats; const float* gamma;
    float* dx; float* dgamma; float* dbeta;
    void* out16;                      /* bf16 [rows, H] or NULL */
    int32_t dy_is_f32, accumulate_dx, rows, H, seq, drop_first;
    float drop_p; uint32_t drop_key;
    float out_drop_p; uint32_t out_drop_key;
} kzv_ln_bwd_args;
int kzv_ln_bwd_ex(const kzv_ln_bwd_args* a, void* stream);

/* The HBM-bound glue kernels of the training step (csrc/elementwise.hip; the cross-entropy entries: csrc/cross_entropy.hip), as the model handle launches them.
 * kzv_im2row: the data movement of nn.Conv2d(kernel = stride = patch) (trocr_model.py:77,89-90): px fp32 [B, C, H, W] -> bf16
 *   [B * (H / ph) * (W / pw), C * ph * pw], column (c * ph + i) * pw + j; pw % 8 == 0. */
int kzv_im2row(const float* px, void* out_bf16, int B, int C, int H, int W, int ph, int pw, void* stream);
/* kzv_embed_assemble: x0 [B, np + 1, He] = dropout(cat(cls, patch_emb [B, np, He]) + pos) (trocr_model.py:183-190), element index
 *   row * He + col.  gw / gw_max: patches per grid row of this batch / of the position table: patch p takes position row
 *   1 + (p / gw) * gw_max + p % gw (width buckets); <= 0 means the table is the batch's own.
 * kzv_embed_assemble_bwd: dpatch bf16 [B, np, He] = the masked dx0 rows of the patches; dcls [He], dpos [table rows, He] and
 *   dpatch_bias [He] are accumulated into (+=) in a fixed summation order (bit-reproducible). */
int kzv_embed_assemble(const float* patch_emb, const float* cls, const float* pos, float* x0, int B, int np, int He,
                       float drop_p, uint32_t drop_key, int gw, int gw_max, void* stream);
int kzv_embed_assemble_bwd(const float* dx0, void* dpatch_bf16, float* dcls, float* dpos, float* dpatch_bias, int B, int np, int He,
                           float drop_p, uint32_t drop_key, int gw, int gw_max, void* stream);
/* Backward of "dropout(linear(x))": out bf16 [M, N] = g fp32 [M, N] * mask (index row * N + col) [* gelu_pre bf16 [M, N], the GELU
 *   derivative a forward epilogue saved; NULL = none]; dbias [N] += column sums of the ROUNDED out (float atomics).  N % 4 == 0.
 * kzv_colsum_bf16: dbias [N] += column sums of g bf16 [M, N] with row stride ld (N, ld % 4 == 0). */
int kzv_cast_drop_colsum(const float* g, void* out_bf16, float* dbias, int M, int N, float drop_p, uint32_t drop_key,
                         const void* gelu_pre_bf16, void* stream);
int kzv_colsum_bf16(const void* g_bf16, int64_t ld, float* dbias, int M, int N, void* stream);
/* RobertaEmbeddings (HF modeling_roberta.py:75-155) over labels int64 [B, L], decoder inputs = columns 0 .. T - 1 (T < L):
 *   kzv_dec_prepare: posids int32 [B, T] = cumsum(id != pad) * (id != pad) + pad; *count += targets labels[:, 1 : T + 1] != pad;
 *     ids >= max_pos are clamped to max_pos - 1 and *err is set to 1 (never cleared here).
 *   kzv_embed_gather: out fp32 [B * T, Hd] = (word[id] + type0) + postab[posid].
 *   kzv_embed_scatter_bwd: dword[id] += dsum row, dpostab[posid] += dsum row (not for the pad row of either table), dtype0 += every
 *     row (float atomics). */
int kzv_dec_prepare(const int64_t* labels, int B, int L, int T, int pad, int max_pos, int32_t* posids, float* count, int32_t* err, void* stream);
int kzv_embed_gather(const int64_t* labels, int L, const int32_t* posids, const float* word, const float* type0, const float* postab,
                     float* out, int B, int T, int Hd, void* stream);
int kzv_embed_scatter_bwd(const float* dsum, const int64_t* labels, int L, const int32_t* posids, float* dword, float* dtype0,
                          float* dpostab, int B, int T, int Hd, int pad, void* stream);
/* nn.CrossEntropyLoss(ignore_index = pad) (trocr_model.py:256,292) on fp32 logits [B * T, ldl] (ldl % 4 == 0, V <= ldl): row b * T + t
 *   scores labels[b][t + 1]; *loss += mean over the *count scored rows; dlogits bf16 [B * T, ldl] or NULL = (softmax - onehot) /
 *   count, zero in pad-target rows and in columns [V, ldl).  Rows up to 5,120 columns stay in registers; wider ones take three passes.
 * kzv_copy_logits: out fp32 [rows, V] = logits[row * ldl + col] (drops the padding columns; ldl may also skip rows). */
int kzv_ce_fwd_bwd(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                   const float* count, float* loss, void* dlogits_bf16, void* stream);
/* The same with label smoothing (F.cross_entropy(..., label_smoothing), 0 <= label_smoothing < 1, else KZV_E_ARG): loss row = lse -
 *   (1 - eps) z[y] - (eps / V) sum_{v < V} z[v], dlogits = (softmax - (1 - eps) onehot - eps / V) / count in columns < V, zero in pad-target
 *   rows and in columns [V, ldl).  0 is kzv_ce_fwd_bwd itself (the same kernels, the same bits). */
int kzv_ce_fwd_bwd_ls(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                      const float* count, float* loss, void* dlogits_bf16, float label_smoothing, void* stream);
/* The same under class weights and / or the focal exponent (kzv_set_class_weights above states both losses): norm2 = {W, S_w} on the
 *   device, from kzv_target_weight_sum; d_class_weights fp32 [V] on the device or NULL (w = 1); 0 <= focal_gamma <= 5, and > 0 only with
 *   label_smoothing 0, else KZV_E_ARG.  With NULL and 0 it is kzv_ce_fwd_bwd_ls (the same kernels, the same bits), norm2[0] acting as count.
 * kzv_target_weight_sum: d_out2[0] = W = sum of w[labels[b][t + 1]] over the scored rows (t < T; not pad, inside [0, V)), d_out2[1] = S_w =
 *   sum_{c < V} w[c]; one workgroup, a fixed order of additions: two calls give the same bits.  NULL weights: {number of scored rows, V}. */
int kzv_ce_fwd_bwd_w(const float* logits, int64_t ldl, const int64_t* labels, int L, int B, int T, int V, int pad,
                     const float* norm2, float* loss, void* dlogits_bf16, float label_smoothing, const float* d_class_weights,
                     float focal_gamma, void* stream);
int kzv_target_weight_sum(const int64_t* labels, int L, int B, int T, int V, int pad, const float* d_class_weights, float* d_out2, void* stream);
int kzv_copy_logits(const float* logits, int64_t ldl, float* out, int rows, int V, void* stream);
/* fp32 masters -> bf16 compute copies, n matrices in one launch (what kzv_model_sync_weights does for the whole table): dst bf16
 *   [rows, cols], dstT bf16 [cols, ldT] = the transpose, or NULL.  `descs` is a HOST array of device pointers; cols % 4 == 0, and
 *   with dstT rows % 4 == 0, ldT % 4 == 0, ldT >= rows.  Uploads the table, launches and waits for `stream`. */
typedef struct kzv_cast_desc {
    const float* src; void* dst; void* dstT;
    int32_t rows, cols; int64_t ldT;
} kzv_cast_desc;
int kzv_cast_weights(const kzv_cast_desc* descs, int n, void* stream);

/* Multi-head attention, one workgroup per (batch, head) on bf16 MFMA kernels for head_dim 64 (the benchmark geometry and the
 * decoder; attention.hip) and for head_dim 96 in mode 0 with Sq, Sk <= 288 (the reference's CLI default ViT, 768 / 8 heads on
 * 1024 x 64 columns: 257 tokens, scripts/train_trocr.py:39-44; attention_d96.hip).  Other head dimensions (multiples of 8 up to
 * 128) and head_dim 96 beyond 288 keys take a plain fp32 kernel -- same results and dropout masks, several times slower
 * (attention_generic.hip).  kzv_attn_impl reports which one serves a call; it, every other attention entry point and the
 * one dispatch behind them live in attention_api.cpp, what the kernel files share in attention_common.h.
 * mode 0: no mask (ViT self-attn / decoder cross-attn); mode 1: causal AND key-not-pad (decoder self; head_dim 64 only). */
typedef struct kzv_attn_args {
    const void* Q; const void* K; const void* V;   /* bf16, row strides ldq/ldk/ldv (multiples of 8), head h at col h*head_dim */
    void* O;                                        /* bf16 [B*Sq, ldo] */
    float* LSE;                                     /* fp32 [B, heads, Sq] */
    const void* dO; void* dQ; void* dK; void* dV;   /* backward only (same strides as O/Q/K/V) */
    int64_t ldq, ldk, ldv, ldo;
    const int64_t* ids; int64_t ld_ids; int32_t pad_id;   /* mode 1: decoder input ids [B, ld_ids] */
    int32_t B, heads, Sq, Sk, mode;
    float drop_p; uint32_t drop_key;
    int32_t head_dim;                                     /* 0 = 64; head h sits at column h * head_dim */
} kzv_attn_args;
int kzv_attn_fwd(const kzv_attn_args* a, void* stream);
int kzv_attn_bwd(const kzv_attn_args* a, void* stream);
/* Which kernels kzv_attn_fwd (bwd = 0) / kzv_attn_bwd (bwd = 1) would run for these arguments, without launching anything or
 * touching a GPU: KZV_ATTN_MFMA64, KZV_ATTN_MFMA96 or KZV_ATTN_VALU; for arguments the launch would refuse, its negative code and
 * kzv_last_error() message.  The launches dispatch through it. */
#define KZV_ATTN_MFMA64 1
#define KZV_ATTN_MFMA96 2
#define KZV_ATTN_VALU 3
int kzv_attn_impl(const kzv_attn_args* a, int bwd);

/* Long sequences: K/V-streaming (flash-style) kernels for head_dim 64 and 96, mode 0, Sq and Sk in 1..4,097
 * (attention_stream.hip).  Same contract as kzv_attn_fwd / kzv_attn_bwd (arguments, natural-log LSE [B, heads, Sq], dropout masks,
 * written outputs), so a streaming forward's LSE feeds a whole-head backward and vice versa; no buffer grows with Sq * Sk and no
 * float atomics (bitwise reproducible).  These two run the streaming kernels at any length, short ones included. */
int kzv_attn_stream_fwd(const kzv_attn_args* a, void* stream);
int kzv_attn_stream_bwd(const kzv_attn_args* a, void* stream);
/* kzv_attn_impl with flags.  KZV_MODEL_LONG_SEQ: head_dim 0 / 64 / 96 calls in mode 0 with Sq or Sk above 288 (up to 4,097) report
 * KZV_ATTN_STREAM64 / KZV_ATTN_STREAM96; every other call, and every call without the flag, gets kzv_attn_impl's answer. */
#define KZV_ATTN_STREAM64 4
#define KZV_ATTN_STREAM96 5
int kzv_attn_impl_ex(const kzv_attn_args* a, int bwd, unsigned flags);

/* Head-averaged attention probabilities, recomputed from what a forward leaves behind (csrc/attention_probs.hip; HF:
 * output_attentions=True -> attentions.mean(1) in eval mode, i.e. BEFORE dropout).  Q [B*Sq, ldq] and K [B*Sk, ldk] bf16 with head h at
 * column h * 64 and LSE fp32 [B, heads, Sq] in natural log are kzv_attn_args' -- exactly what kzv_attn_fwd / kzv_attn_stream_fwd read and
 * write.  Mode 0 and head_dim 64 only, Sq in 1..288, Sk in 1..4,097; anything else is KZV_E_ARG.
 *   map  fp32 [B, Sq, ld_map] or NULL: map[b,q,k] = (1/heads) * sum_h exp(q_h . k_h * 64^-0.5 - LSE[b,h,q]); with NULL nothing of size Sk is written
 *   pos  fp32 [B, Sq, 4] = (sum_k P (k / grid_w), sum_k P (k % grid_w), max_k P, sum_k P): centroid in patch rows / columns of a grid
 *        grid_w patches wide, the peak weight, and the row sum (~ 1 when LSE belongs to Q and K)
 *   peak int32 [B, Sq] = the first arg-max key
 * No atomics, fixed summation order: bit-reproducible. */
typedef struct kzv_attn_probs_args {
    const void* Q; const void* K; int64_t ldq, ldk;
    const float* LSE;
    float* map; int64_t ld_map;      /* NULL: no map */
    float* pos; int32_t* peak;       /* [B,Sq,4], [B,Sq]; either may be NULL */
    int32_t B, heads, Sq, Sk, grid_w, head_dim;   /* head_dim 0 = 64 */
    int32_t mode;                    /* kzv_attn_args' mode: 0 (no mask) is the only one served */
} kzv_attn_probs_args;
int kzv_attn_probs(const kzv_attn_probs_args* a, void* stream);
/* Per-token scores from fp32 logits rows [rows_b * T, ld], one wave per row: the row's log-sum-exp over `vocab` columns (maximum
 * subtracted first); logprob[b,t] = log-softmax at targets[b, t + 1] (kzv_ce_fwd_bwd's indexing: row b * T + t against column t + 1
 * of int64 targets [rows_b, ld_targets]), 0 where that target is pad_id; top1 = the first arg-max column and top1_logprob its
 * log-probability.  Each output [rows_b, T], any of them NULL. */
int kzv_token_scores(const float* logits, int64_t ld, const int64_t* targets, int64_t ld_targets, int rows_b, int T, int vocab, int pad_id,
                     float* logprob, int64_t* top1, float* top1_logprob, void* stream);
/* The k (1..8) best columns of every fp32 logits row [rows, ld] and their log-softmax values (logit - log-sum-exp over `vocab` columns,
 * maximum subtracted first), one wave per row in ONE pass: ids int32 and logprob fp32, [rows, k] each, best first.  Replaces HF's
 * output_scores=True, scores[t].log_softmax(-1).topk(k).  Order: descending logit, ties by ascending column -- kzv_token_scores' first
 * arg-max rule, so entry 0 is its top1 / top1_logprob.  -inf logits are legal: they rank last (ties by column) with log-probability
 * -inf.  Where vocab < k the surplus entries are id -1, logprob -inf.  Rows holding NaN have unspecified order; every id stays in
 * [-1, vocab).  Bit-reproducible (no atomics).  KZV_E_ARG: null pointers, k outside 1..8, vocab < 1, ld < vocab, rows outside
 * 1..2^31-1. */
int kzv_token_topk(const float* logits, int64_t ld, int64_t rows, int vocab, int k, int32_t* ids, float* logprob, void* stream);
/* Levenshtein distance, edit counts, alignment and per-character error counts of n (prediction row, label row) pairs of token ids, one
 * wave per pair (csrc/edit_distance.hip).  Replaces tokenizer.batch_decode(skip_special_tokens=True) of both sides + calculate_cer's
 * editdistance per line (src/models/trocr_model.py:373-379, 400-410) for a tokenizer of one character per token, where the distance over
 * the ids IS the string distance.  From each int64 row every id that equals one of the n_special (0..8) `special` values, wherever it
 * stands, and every id outside [0, vocab) is dropped (nothing is cut at the first EOS); what is left, at most 128 ids, is the line.
 *   dist, ref_len, pred_len  int32 [n]: unit-cost distance and the two compacted lengths (CER = dist / ref_len on the host)
 *   ops          int32 [n, 4], optional: correct, substituted, deleted (label tokens), inserted (predicted tokens); the last three sum to dist
 *   ref_to_pred  int32 [n, ld_align], optional: per COMPACTED label index the compacted prediction index it is aligned to, -1 where the
 *                label token is deleted, -2 from ref_len on; columns [0, width_ref) are written
 *   pred_to_ref  likewise per compacted prediction index: -1 = inserted, -2 from pred_len on; columns [0, width_pred) are written
 *   char_stats   int32 [vocab, 5], optional, ACCUMULATED (the caller zeroes it; several calls sum over a dataset): per id its occurrences
 *                as a label token, of these correct / substituted / deleted, and its insertions as a predicted token.  Integer atomics:
 *                the same table in every run.
 * The alignment is the walk back from the last cell of the Wagner-Fischer matrix under ONE FIXED PREFERENCE: diagonal (match or
 * substitution) if it attains the cell's minimum, else up (deletion of a label token), else left (insertion of a predicted token);
 * kzv/metrics.py: edit_stats_reference states it in numpy.  With ops, both alignment arrays and char_stats null the distance-only
 * instance runs, which keeps no direction bits.  No model handle; n == 0 returns KZV_OK and launches nothing.
 * KZV_E_ARG, before any launch: null arguments, pred / ref / dist / ref_len / pred_len null (n > 0), a width outside 1..128, a leading dimension
 * smaller than its width, n_special outside 0..8, vocab < 1, n < 0, exactly one of the two alignment arrays, ld_align smaller than a width. */
typedef struct kzv_edit_args {
    const int64_t* pred; int64_t ld_pred;    /* [n, ld_pred >= width_pred] */
    const int64_t* ref;  int64_t ld_ref;     /* [n, ld_ref  >= width_ref]  */
    int32_t n, width_pred, width_ref, vocab, n_special, special[8];
    int32_t *dist, *ref_len, *pred_len;      /* [n] */
    int32_t* ops;                            /* optional [n, 4] */
    int32_t* ref_to_pred; int32_t* pred_to_ref; int64_t ld_align;   /* optional, ld_align >= max(width_pred, width_ref) */
    int32_t* char_stats;                     /* optional [vocab, 5], accumulated */
} kzv_edit_args;
int kzv_edit_distance(const kzv_edit_args* a, void* stream);

/* ------------------------------------------------------------- the ResNet / BiLSTM / CTC model of ocr_lightning/model.py
 * (SURVEY.md section 8(f), row N3).  Per-op entry points; the host mirror kzv/ocr_model.py strings them together the way
 * OCRModel.forward / _shared_step do (ocr_lightning/model.py:61-88, 90-195).  Activations are NHWC (rows = pixels, columns =
 * channels) so that a convolution is kzv_ocr_im2col + kzv_gemm_nt, its weight gradient kzv_gemm_tn on the same column matrix and
 * its input gradient kzv_gemm_nt against the transposed packed weight + kzv_ocr_col2im.  bf16 GEMM operands, fp32 everything else --
 * or, after kzv_ocr_set_precision(1), fp32 operands throughout: every buffer documented as "bf16" below is then a float buffer of
 * the same shape and the GEMMs are kzv_gemm_nt_f32 / kzv_gemm_tn_f32 (the reference's own arithmetic; process-wide switch, set by
 * kzv.OCRModel before each of its passes). */
int kzv_ocr_set_precision(int fp32);
/* images fp32 [N, C, H, W] (ocr_collate_fn's stack, dataset.py:100) -> NHWC bf16 */
int kzv_ocr_nchw_to_nhwc(const float* x, void* out_bf16, int N, int C, int H, int W, void* stream);
/* nn.Conv2d forward operand (resnet34's 7x7/2, 3x3/1, 3x3/2 and 1x1/2 convolutions, model.py:31-32): cols bf16 [N*Ho*Wo, Kp],
 * column (kh * KW + kw) * C + c, Kp >= KH*KW*C a multiple of 8 (the GEMM wants a multiple of 64), zero-filled padding. */
int kzv_ocr_im2col(const void* x_bf16, void* cols_bf16, int N, int H, int W, int C, int KH, int KW, int stride, int pad, int Kp, void* stream);
/* nn.Conv2d input gradient from the gradient of the column matrix (fp32 [N*Ho*Wo, Kp]): dx fp32 [N, H, W, C] (+= if accumulate) */
int kzv_ocr_col2im(const float* dcols, float* dx, int N, int H, int W, int C, int KH, int KW, int stride, int pad, int Kp, int accumulate, void* stream);
/* conv weight fp32 [Cout, Cin, KH, KW] (the state_dict layout) -> packed bf16 [Cout, Kp] (+ its transpose [Kp, Cout] if wpT) */
int kzv_ocr_conv_weight(const float* w, void* wp_bf16, void* wpT_bf16, int Cout, int Cin, int KH, int KW, int Kp, void* stream);
/* gradient of the packed weight fp32 [Cout, Kp] accumulated into the state_dict layout [Cout, Cin, KH, KW] */
int kzv_ocr_conv_wgrad_unpack(const float* gp, float* g, int Cout, int Cin, int KH, int KW, int Kp, void* stream);
/* Both for n <= 40 convolutions in ONE launch each (what a ResNet34 step needs after its optimizer step / at the end of its backward):
 * HOST arrays of n device pointers and geom[n][5] = (Cout, Cin, KH, KW, Kp). */
int kzv_ocr_conv_weight_multi(int n, const float* const* w, void* const* wp_bf16, void* const* wpT_bf16, const int32_t* geom, void* stream);
int kzv_ocr_conv_wgrad_unpack_multi(int n, const float* const* gp, float* const* g, const int32_t* geom, void* stream);
/* nn.BatchNorm2d (+ the BasicBlock's residual add and ReLU): out bf16 = [relu](gamma * (y - mean) * rstd + beta [+ resid]); y fp32
 * [M, C].  train: batch statistics (biased variance), running statistics updated with `momentum` and the unbiased variance;
 * eval: the running statistics.  mean / rstd [C] are kept for the backward.  d_scratch: kzv_ocr_bn_scratch_floats(M, C) floats.
 * The statistics (and the backward's dgamma / dbeta) are reduced in a fixed order, without atomics: a one-ulp difference of a mean
 * flips the bf16 rounding of an activation and, through ReLU masks, ~1 % of the gradients downstream. */
int64_t kzv_ocr_bn_scratch_floats(int64_t M, int C);
int kzv_ocr_bn_fwd(const float* y, int64_t M, int C, const float* gamma, const float* beta, float* run_mean, float* run_var, float* mean,
                   float* rstd, const void* resid_bf16, void* out_bf16, int relu, int train, float eps, float momentum, float* d_scratch, void* stream);
/* its backward: da fp32 [M, C] = gradient of the (post-ReLU) output; dz fp32 = da masked by the ReLU (also the gradient of the
 * residual input); dgamma / dbeta are accumulated into (+=); dy bf16 = gradient of y.  d_scratch as for the forward. */
int kzv_ocr_bn_bwd(const float* da, const void* a_bf16, const float* y, int64_t M, int C, const float* mean, const float* rstd, const float* gamma,
                   float* dz, float* dgamma, float* dbeta, void* dy_bf16, int relu, int train, float* d_scratch, void* stream);
/* nn.MaxPool2d(3, stride 2, padding 1) of the ResNet stem, NHWC bf16; idx = winning tap per output (first maximum, like torch) */
int kzv_ocr_maxpool_fwd(const void* x_bf16, void* out_bf16, unsigned char* idx, int N, int H, int W, int C, void* stream);
int kzv_ocr_maxpool_bwd(const float* dout, const unsigned char* idx, float* dx, int N, int H, int W, int C, void* stream);
/* nn.AdaptiveAvgPool2d((1, 1)) + flatten (model.py:34, 66-67): feat fp32 and bf16 [N, C] */
int kzv_ocr_avgpool_fwd(const void* x_bf16, float* feat_f32, void* feat_bf16, int N, int HW, int C, void* stream);
int kzv_ocr_avgpool_bwd(const float* dfeat, float* dx, int N, int HW, int C, void* stream);
/* One nn.LSTM direction on a length-1 sequence with zero initial state (model.py:40-47, 73-75): gates fp32 [B, 4H] = x W_ih^T + b_ih
 * (a kzv_gemm_nt; torch order i, f, g, o), b_hh [4H] added here; h written into columns of the [B, ldh] output (forward | reverse
 * halves).  With h0 = c0 = 0 the recurrent weight W_hh multiplies zeros and the forget gate receives no gradient. */
int kzv_ocr_lstm_cell_fwd(const float* gates, const float* b_hh, float* h_f32, void* h_bf16, int64_t ldh, int B, int H, void* stream);
int kzv_ocr_lstm_cell_bwd(const float* gates, const float* b_hh, const float* dh, int64_t lddh, void* dgates_bf16, int B, int H, void* stream);
/* F.log_softmax(dim = -1) on fp32 rows (model.py:125) */
int kzv_ocr_log_softmax(const float* x, float* lp, int rows, int C, void* stream);
/* nn.CTCLoss(blank, zero_infinity) on lp fp32 [T, B, C] (model.py:51-55, 171-176): d_nll[b] = -log p(target_b) (0 where infinite and
 * zero_infinity); if d_dlogits: the gradient with respect to the logits behind lp, times d_gscale[b] (the caller folds the
 * reduction -- 'mean' = 1 / (max(target_len, 1) * B) -- and the loss weight into it).  d_scratch: 2 * B * T * (2 * min(max_target_len, T) + 1)
 * floats (a label longer than T has no alignment: loss inf -> 0 with zero_infinity, zero gradient, whatever its length; T <= 511).  targets int64 [B, ld_targets]; lengths int64 [B]. */
int kzv_ocr_ctc(const float* lp, const int64_t* targets, int64_t ld_targets, const int64_t* input_lengths, const int64_t* target_lengths, int T,
                int B, int C, int blank, int zero_infinity, int max_target_len, float* d_scratch, float* d_nll, const float* d_gscale,
                float* d_dlogits, void* stream);
/* The localisation loss of _shared_step (model.py:100-122): mean over the samples with n_i = min(count_i, max_boxes) > 0 of the mean
 * SmoothL1 (beta 1) between pred[i, :n_i] and gt[i, :n_i].  *d_loss += loss (zero it first); d_dpred fp32 [B, max_boxes, 4]. */
int kzv_ocr_smooth_l1_boxes(const float* pred, int max_boxes, const float* gt, int gt_boxes, const int32_t* counts, int B, float* d_loss,
                            float* d_dpred, void* stream);
/* torch.optim.Adam (model.py:197; no weight decay, no amsgrad), `step` = 1-based step count */
int kzv_ocr_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int step, void* stream);
/* The same step with the bias corrections in device memory: d_bc[0] = 1 - beta1^t, d_bc[1] = sqrt(1 - beta2^t) (fp32).  For a step
 * replayed from a captured hipGraph (kzv.OCRModel.fit_step): no step-dependent scalar among the kernel arguments. */
int kzv_ocr_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, const float* d_bc,
                     void* stream);
int kzv_ocr_cast_bf16(const float* x, void* out_bf16, int64_t n, void* stream);
int kzv_ocr_cast_transpose(const float* x, void* out_bf16, int rows, int cols, void* stream);   /* [rows, cols] fp32 -> bf16 [cols, rows] */

/* ------------------------------------------------------------- measurement hooks (bench.py roofline leg)
 * When enabled, every launch of the hot kernels is bracketed by HIP events on its own stream.
 * kind: 0 gemm_nt, 1 gemm_tn, 2 attn_fwd, 3 attn_bwd, 4 gemm_nt_fp8.  work = algorithmic FLOPs (2*M*N*K; 4*B*h*Sq*Sk*64 /
 * 10*B*h*Sq*Sk*64 for attention fwd / bwd).  Collect after synchronising the stream.
 * kzv_prof_select restricts recording to the kinds in `kind_mask` (bit k = kind k; default all): every bracketed
 * launch costs ~2 us of stream time, so the timed region records only the kernel it reports. */
int kzv_prof_enable(int on, int capacity);
int kzv_prof_select(unsigned kind_mask);
int kzv_prof_collect(int kind, double* total_ms, double* total_flops, int64_t* launches);
/* Sampling: bracket only every `stride`-th launch of each selected kind (default 1 = all).  A bracket costs ~2 us of stream
 * time; with a stride co-prime to the launches per step every launch site is sampled equally often over `stride` steps.
 * kzv_prof_collect then sums the SAMPLED launches; kzv_prof_seen = launches of that kind seen since kzv_prof_enable(1, n). */
int kzv_prof_sample(int stride);
int64_t kzv_prof_seen(int kind);
uint32_t kzv_drop_key(uint64_t seed, uint32_t site);

/* Dropout call sites of the training step (nn.Dropout / F.dropout in the reference).  kzv_forward_loss(train=1, seed) keys
 * site s with kzv_drop_key(seed, s); backward regenerates the same masks from the same keys (nothing is stored).
 *   KZV_SITE_ENC_EMB           ViTEncoder dropout on cat(cls, patches) + pos            (trocr_model.py:190)      [B*Se, He]
 *   KZV_SITE_ENC_LAYER(i, 0)   attention-probability dropout of ViT layer i            (HF modeling_vit.py:184)  [B*heads*Sq, Sk]
 *   KZV_SITE_ENC_LAYER(i, 1)   ViTLayer.dropout on the attention block's output        (HF modeling_vit.py:276)  [B*Se, He]
 *   KZV_SITE_ENC_LAYER(i, 2)   ViTLayer.dropout on the MLP output                      (HF modeling_vit.py:283)  [B*Se, He]
 *   KZV_SITE_DEC_EMB           RobertaEmbeddings.dropout                               (HF modeling_roberta.py:120) [B*T, Hd]
 *   KZV_SITE_DEC_LAYER(i, 0/2) self / cross attention-probability dropout              (HF modeling_roberta.py:178)
 *   KZV_SITE_DEC_LAYER(i, 1/3) RobertaSelfOutput.dropout of the self / cross block     (HF modeling_roberta.py:338)
 *   KZV_SITE_DEC_LAYER(i, 4)   RobertaOutput.dropout (FFN)                             (HF modeling_roberta.py:396)
 * Element index of a [rows, cols] hidden site: row * cols + col (kzv_debug_dropout_mask); an attention site is indexed by
 * (b * heads + h, q, key) (kzv_debug_attn_dropout_mask).  Rows are token rows of the PACKED decoder ([B, t_active],
 * kzv_set_active_length). */
#define KZV_SITE_ENC_EMB 1u
#define KZV_SITE_ENC_LAYER(i, k) (16u + 4u * (uint32_t)(i) + (uint32_t)(k))
#define KZV_SITE_DEC_EMB 1000u
#define KZV_SITE_DEC_LAYER(i, k) (1016u + 8u * (uint32_t)(i) + (uint32_t)(k))

/* Debug / parity entry (mask replay): writes the multiplier (0 or 1/P(keep)) the kernels apply to element
 * index row * ld_index + col under `key` and drop probability p, for row < rows, col < cols: d_out fp32 [rows, cols].
 * Uses the same device hash as every fused dropout epilogue, so a test can hand the exact masks of a training step to the
 * CPU oracle and compare logits, loss and every gradient with dropout ON. */
int kzv_debug_dropout_mask(uint32_t key, float p, int64_t rows, int64_t cols, int64_t ld_index, float* d_out, void* stream);
/* The same for an ATTENTION-PROBABILITY site (KZV_SITE_*_LAYER(i, 0 / 2); F.dropout on the softmax output, HF modeling_vit.py:184,
 * modeling_roberta.py:178): d_out fp32 [pairs * Sq, Sk], pairs = batch * heads.  These sites draw their bits from one 32-bit hash
 * per 4 x 4 block of a (batch, head)'s [Sq, Sk] matrix and a 16-bit multiply per element (kzv_common.h, "attention-probability
 * dropout"; numpy statement: oracle/attn_dropout.py), because the forward kernel holds 4 keys of one query per lane and the
 * backward kernel 4 queries of one key, and this costs the same few instructions in both orientations. */
int kzv_debug_attn_dropout_mask(uint32_t key, float p, int64_t pairs, int32_t Sq, int32_t Sk, float* d_out, void* stream);

/* Data-parallel runs: the GEMM kernels that put exactly one workgroup on every CU (persistent gemm_nt256p, gemm_tn256)
 * double their time when a concurrently running collective holds a few CUs.  With n > 0 the launchers leave n CUs
 * free: gemm_nt falls back to the one-tile-per-workgroup kernel (its workgroups flow to whatever CUs are free) and
 * gemm_tn256 sizes its token splits to (CUs - n) workgroups.  Default 0 (or KZV_CU_RESERVE); kzv/trainer.py sets it
 * when world_size > 1.  kzv_get_cu_reserve returns the value in force (so that a caller can restore it). */
int kzv_set_cu_reserve(int n);
int kzv_get_cu_reserve(void);

/* Diagnostic: how often one of the library's process-wide scratch workspaces (split-K partial tiles of the GEMMs, the generic
 * attention backward, the patch-embedding backward) has moved to a larger block since the library was loaded.  A workspace that
 * grows keeps its old block allocated for the rest of the process, so a captured graph or a kernel in flight never reads freed
 * memory; each doubles at least, from 1 MiB, so the count stays small. */
int64_t kzv_scratch_growths(void);

/* ------------------------------------------------------------------ N2: input pipeline on the device
 * Replaces ResizeWithPadding + ToTensor + Normalize(0.5, 0.5) (src/data/trocr_dataset.py:24-53, 97-104) for a batch of
 * decoded uint8 RGB crops of different sizes: Pillow's two-pass LANCZOS resample (bit-exact: fixed-point coefficients,
 * uint8 intermediate), centred paste on a white canvas, [-1, 1] fp32 CHW output.
 *
 * kzv_lanczos_coeffs (HOST, no GPU needed; also usable from DataLoader workers): Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc for resampling `in_size` samples to `out_size`: bounds[out][2] = (first input index, count),
 * kk[out][ksize] = 22-bit fixed-point weights; returns ksize through *ksize (call with kk == NULL to query it).
 * kzv_preprocess_lines (device pointers; `rgb` and `tmp` need 4 bytes of slack after their last byte: pixels are fetched
 * as unaligned 32-bit words): rgb = the crops packed back to back (HWC, 3 bytes per pixel), desc[i] locates
 * crop i, its geometry and its coefficient tables inside `coef` (int32 offsets); tmp = scratch for the horizontal pass
 * (desc[i].tmp_off, in_h * new_w * 3 bytes per crop); max_tmp_pixels = max over crops of in_h * new_w (sizes the launch);
 * lut256 = the 256 possible output values; out = [n, 3, target_h, target_w] fp32. */
typedef struct {
    int64_t src_off;            /* byte offset of the crop in `rgb` */
    int64_t tmp_off;            /* byte offset of its scratch in `tmp` */
    int64_t hb_off, hk_off;     /* int32 offsets in `coef`: horizontal bounds [new_w][2], weights TRANSPOSED [hk_size][new_w] */
    int64_t vb_off, vk_off;     /* vertical bounds [new_h][2], weights [new_h][vk_size] */
    int32_t in_h, in_w, new_h, new_w, paste_x, paste_y, hk_size, vk_size;
} kzv_line_desc;
int kzv_lanczos_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk, int* ksize);
int kzv_preprocess_lines(const uint8_t* rgb, const kzv_line_desc* desc, const int32_t* coef, int n, int target_h, int target_w,
                         int64_t max_tmp_pixels, const float* lut256, uint8_t* tmp, float* out, void* stream);

/* ------------------------------------------------------------------ training-time augmentation of line crops (csrc/augment.hip)
 * The reference's augmentation vocabulary (T.RandomAffine of scripts/train_stackganv2_bcr_char.py:54; rotation, brightness /
 * contrast, noise and blur of src/utils/augmentation.py:35-98; the TrOCR recipe's stroke dilation / erosion) as ONE launch over a
 * batch of the crops `forward` takes: in = [n, 3, H, W] fp32 in [-1, 1] (white = +1), params = n device structs (the host draws
 * them: kzv/augment.py), out = same shape.  A pure function of (in, params); per output pixel, in this fixed order:
 *   1. affine warp: sx = m0*x + m1*y + m2, sy = m3*x + m4*y + m5 (output pixel -> source pixel, pixel-index units), sx clamped to
 *      [-1, W] and sy to [-1, H] before floor; four bilinear taps, a tap outside the canvas is +1; a + fx*(b - a), then
 *      top + fy*(bot - top), so an identity map returns its input bit for bit.
 *      torch: grid_sample(x - 1, grid, 'bilinear', 'zeros', align_corners=False) + 1, grid = ((2*sx + 1)/W - 1, (2*sy + 1)/H - 1).
 *   2. stroke morphology on the warped image: morph 1 = 3x3 maximum (ink is dark: strokes thin), 2 = 3x3 minimum, neighbours
 *      outside the canvas skipped.  torch: max_pool2d(x, 3, 1, 1) / -max_pool2d(-x, 3, 1, 1).
 *   3. separable 7-tap blur, horizontal then vertical, indices clamped to the canvas (replicate); {0,0,0,1,0,0,0} is exact identity.
 *   4. out = clamp(contrast*v + brightness + noise_sigma*g, -1, 1), g = (b0 + b1 + b2 + b3 - 510) * (1/147.80) with b0..b3 the four
 *      bytes of hash32(e * 0x9E3779B9 + noise_key), hash32 = the dropout sites' counter hash, e = (c*H + y)*W + x (a sum of four
 *      bytes has variance 4 * 65535/12 = 21845 = 147.80^2: g has unit variance; integer-exact, so numpy reproduces it).
 * KZV_E_ARG before any launch: a null pointer, n < 1, H or W < 1, 3*H*W >= 2^32, 2^24 or more tiles (a tile = 32x64 pixels of one
 * channel of one crop, 256 threads, and a launch carries fewer than 2^32 threads: n * 3 * ceil(H/32) * ceil(W/64) < 2^24; split a
 * larger batch), or `out` overlapping `in` (the kernel gathers: it cannot run in place). */
typedef struct {
    float m[6];                 /* inverse map, output pixel -> source pixel */
    float blur[7];              /* 7-tap blur weights */
    float contrast, brightness, noise_sigma;
    uint32_t noise_key;         /* per-image hash key */
    int32_t morph;              /* 0 none, 1 thinner strokes (3x3 max), 2 thicker strokes (3x3 min) */
} kzv_augment_params;           /* 72 bytes */
int kzv_augment_lines(const float* in, const kzv_augment_params* params, int n, int H, int W, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KZV_H */
