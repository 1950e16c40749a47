/* libsocior -- C ABI of the MI355X-native SocioReasoner inference hot path.
 *
 * The reference (AMAP-ML/SocioReasoner) has no native code and therefore no FFI for this path: its plugin boundary
 * is the Python class InferenceStrategy (roll/distributed/strategy/strategy.py:16-138) and the engine behind it is
 * vLLM (roll/distributed/strategy/vllm_strategy.py:114-141).  This header is the derived contract of SURVEY.md
 * section 8(B): what a ctypes binding inside a replacement InferenceStrategy binds (INTEGRATION.md shows that stub).
 * Each entry point cites the reference behaviour it replaces (paths relative to /root/reference, `hf:` =
 * transformers/models/qwen2_5_vl/modeling_qwen2_5_vl.py).
 *
 * Conventions: extern "C"; plain pointers and sizes; every call returns 0 on success, a negative errno-style value or
 * a positive hipError_t on failure (sr_last_error() gives the text).  Device buffers are caller-owned
 * (torch.Tensor.data_ptr()); "host" marks the few small control arrays read on the CPU.  Every call that enqueues GPU
 * work takes the caller's hipStream_t (as void*) and is asynchronous with respect to the host unless stated.  The
 * engine allocates no device memory after sr_engine_create(): everything lives in the caller-provided workspace.
 * One engine per process/GPU; calls on one engine must not overlap (no internal threads, not re-entrant).
 */
#ifndef SOCIOR_H
#define SOCIOR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libsocior.so is built with -fvisibility=hidden: the declarations between this push and the pop at the end of the file are the library's
 * whole dynamic symbol table (tests/test_host_round6.py checks `nm -D` against this header). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct sr_engine sr_engine;

#define SR_DTYPE_BF16 0
#define SR_DTYPE_F32 1

/* Geometry (HF config fields of Qwen2.5-VL; values for SocioReasoner-3B in SURVEY.md 2.3) + capacities. */
typedef struct sr_config {
    /* vision tower */
    int32_t v_depth, v_hidden, v_heads, v_inter, v_patch, v_temporal, v_merge, v_window, v_out_hidden, v_in_ch;
    int32_t v_n_fullatt;
    int32_t v_fullatt[16];
    /* language model */
    int32_t t_layers, t_hidden, t_heads, t_kv_heads, t_head_dim, t_inter, t_vocab;
    float t_rms_eps, t_rope_theta;
    int32_t mrope_section[3];
    int32_t image_token_id;      /* <|image_pad|>: positions holding it take rows of the image embeddings (hf:1210-1216) */
    /* capacities that size the workspace */
    int32_t max_patches;         /* ViT rows (all images of one sr_vit_forward call) */
    int32_t max_prefill_tokens;  /* packed prompt tokens of one sr_prefill call */
    int32_t max_batch;           /* batch rows = concurrent sequences (<= 128; more than 32 rows: bf16 LM weights, decode GEMVs stream
                                  * each weight tile once for all rows -- csrc/gemv.hip k_gemv32g) */
    int32_t max_ctx;             /* KV rows per slot, multiple of 64 (prompt + generated) */
    int32_t max_new_tokens;      /* rows of the device token log */
    /* storage of the LM decoder linears (q/k/v, o, gate/up, down) -- BASELINE.json configs[4]:
     *   0 = bf16;  1 = fp8 e4m3 with one float32 scale per output channel, W[n,k] = q[n,k] * scale[n], scale[n] = amax_n / 448.
     * Embedding / LM head stay bf16; the ViT has a switch of its own (v_weight_dtype below).  The decode GEMV streams the fp8 image
     * (half the HBM bytes) and widens it to bf16 in registers (exact); prefill multiplies a bf16 image of the same q; both apply
     * scale[n] to the float32 accumulator.
     *   2 = 1, and the PREFILL linears run fp8 x fp8 on the block-scaled K = 128 MFMA (twice the bf16 rate): their inputs are
     * quantised to OCP-MX e4m3 (32-wide blocks along k, e8m0 shared scales; definition: oracle/model_ref.py mx_quantize), the
     * weight operand is the same fp8 image; decode is unchanged (bf16 activations). */
    int32_t lm_weight_dtype;
    /* KV-cache slots, 0 = max_batch.  More slots than batch rows let an admission (sr_admit_stage) prefill the NEXT sequences into
     * spare slots while all max_batch rows are still decoding; sr_admit_commit then maps freed rows onto those slots. */
    int32_t kv_slots;
    /* storage of the vision tower's linears -- visual.blocks.N.{attn.qkv, attn.proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj}.weight and
     * visual.merger.mlp.{0,2}.weight; independent of lm_weight_dtype (all six combinations are valid):
     *   0 = bf16 (the default);
     *   2 = the definition of lm_weight_dtype = 2 applied to the tower: weights fp8 e4m3 with one float32 scale per output channel
     * (scale[n] = amax_n / 448), the INPUT of each of these linears quantised to OCP-MX e4m3 after its bf16 rounding (32-wide blocks along
     * k, e8m0 shared scales; oracle/model_ref.py mx_quantize), fp8 x fp8 on the block-scaled K = 128 MFMA at any row count, the accumulator
     * multiplied by scale[n], then bias / residual / activation with the bf16 rounding points of mode 0.  The patch embedding (K = 1176,
     * padded to 1216: no multiple of 128; 0.4 % of the tower's FLOPs), norm weights, biases, rotary tables and attention stay bf16.  The
     * bf16 masters are kept: sr_finalize_weights quantises from them, and again after any reload.
     *   1 is refused: fp8 weights under bf16 activations pay for a decode weight stream, which the tower does not have. */
    int32_t v_weight_dtype;
} sr_config;

/* Bytes of device workspace sr_engine_create needs for this configuration (0 on invalid config). */
size_t sr_workspace_bytes(const sr_config* cfg);

/* Replaces VllmStrategy.initialize (vllm_strategy.py:46-106): builds the engine inside `workspace` (device memory,
 * >= sr_workspace_bytes, 256-byte aligned).  Weights are loaded afterwards with sr_load_weight. */
int sr_engine_create(const sr_config* cfg, void* workspace, size_t workspace_bytes, sr_engine** out);
int sr_engine_destroy(sr_engine* e);
/* Text of the last error of this engine (or of the last failed create when e == NULL).  Never NULL. */
const char* sr_last_error(const sr_engine* e);

/* Replaces the weight path (from_pretrained / the trainer->engine broadcast, megatron_strategy.py:411-448):
 * hands one HF-named tensor (device pointer, row-major, `shape`) to the engine, which copies it into its own layout
 * (K padded to 64, q/k/v fused, gate/up interleaved).  Accepted names: reference-era checkpoints
 * (`visual.*`, `model.layers.*`, `model.embed_tokens.weight`, `model.norm.weight`, `lm_head.weight`;
 * mcore_adapter/src/mcore_adapter/models/converter/template.py:845-899) and transformers-5 names
 * (`model.visual.*`, `model.language_model.*`).  `lm_head.weight` is accepted and ignored (tied embeddings). */
int sr_load_weight(sr_engine* e, const char* hf_name, const void* dev_ptr, int dtype, const int64_t* shape, int ndim,
                   void* stream);
/* Number of parameters still missing (0 = ready); when `first_missing` is non-NULL it receives one missing name. */
int sr_weights_missing(const sr_engine* e, char* first_missing, size_t cap);

/* Synthetic weights (no checkpoint is available offline): fills `n` bf16 values at dev_out with the counter-based
 * generator defined in oracle/weights.py (independent implementation), element index = start + i. */
int sr_synth_fill(void* dev_out_bf16, int64_t n, const char* hf_name, uint32_t seed, float base, void* stream);

/* K1 -- replaces the HF image processor's rescale/normalise/patchify (hf:models/qwen2_vl/
 * image_processing_pil_qwen2_vl.py:153-248, invoked at roll/datasets/collator.py:456-461): uint8 HWC image (h, w
 * multiples of patch*merge, already smart_resize'd) -> bf16 patch rows [N, sr_pixel_ld()], zero padded. */
/* The attention plan of the last sr_vit_forward's grids: out4 = {window work items, full-attention work items, 1 when every window holds exactly 64
 * tokens (the window blocks then run k_attn_win64), 1 when every image starts on a multiple of 8 patches (full attention through k_attn_prefill2)}.
 * Lets tests assert WHICH kernel a geometry takes. */
int sr_vit_plan(const sr_engine* e, int32_t* out4);
int sr_pixel_ld(const sr_engine* e);
int sr_patchify_u8(sr_engine* e, const uint8_t* dev_img_hwc, int h, int w, void* dev_pixels_bf16, void* stream);

/* K2-K9 -- replaces Qwen2_5_VisionTransformerPretrainedModel.forward (hf:408-474): pixel values of n_img images
 * (rows concatenated) -> merged image embeddings [sum(t*h*w)/merge^2, v_out_hidden] bf16.
 * pixels: SR_DTYPE_BF16 = rows of sr_pixel_ld() (output of sr_patchify_u8); SR_DTYPE_F32 = [N, C*T*p*p] as the HF
 * processor emits them.  grid_thw: host int64 [n_img][3] (t must be 1). */
int sr_vit_forward(sr_engine* e, const void* dev_pixels, int pixels_dtype, const int64_t* host_grid_thw, int n_img,
                   void* dev_out_bf16, void* stream);

/* K10-K17 prefill -- replaces the prompt phase of vllm.LLM.generate (vllm_strategy.py:127) / the HF forward at
 * hf_strategy.py:84-93: B un-padded sequences packed back to back.
 *   host_ids   int64 [n_tok]      token ids; image_token_id positions take consecutive rows of dev_image_embeds
 *   host_pos3  int64 [3][n_tok]   mRoPE position ids (roll/datasets/collator.py / get_rope_index)
 *   host_seq_lens int32 [B], host_slots int32 [B] (KV-cache slot of each sequence, < max_batch)
 * Leaves the KV cache filled, the greedy next token of every sequence in the device state, and (when not NULL)
 * float32 last-position logits [B, vocab] in dev_logits_out. */
int sr_prefill(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
               const int32_t* host_slots, int B, const void* dev_image_embeds, int n_image_rows, float* dev_logits_out,
               void* stream);

/* Teacher-forced forward with logits at EVERY position -- what a logits-consuming caller of
 * InferenceStrategy.forward_step gets from the HF forward (hf_strategy.py:49-94, use_cache=False): arguments as
 * sr_prefill (sequences use KV slots 0..B-1), dev_all_logits float32 [n_tok, vocab] for the packed tokens.  Un-rounded
 * float32 like sr_prefill's last-position logits (HF rounds to bf16). */
int sr_forward_logits(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens, int B,
                      const void* dev_image_embeds, int n_image_rows, float* dev_all_logits, void* stream);

/* Decode -- replaces the autoregressive loop of vllm.LLM.generate with SamplingParams built at
 * vllm_strategy.py:289-309 for temperature 0 (greedy): generates up to max_new tokens for the sequences prefilled
 * into slots host_slots[0..B).  Stops a sequence at the first token in host_eos (the token is kept, later positions
 * hold pad_id -- the layout gather_outputs_to_pad_tensor produces, vllm_strategy.py:279-286).
 *   dev_tokens_out int32 [B][max_new]
 *   dev_logits_trace (optional) float32 [max_new][B][vocab]: logits that produced every token (forces eager launch)
 *   dev_forced (optional) int32 [B][max_new]: teacher forcing -- token fed back at step i is forced[b][i]
 *   use_graph: replay one captured hipGraph per step (ignored when tracing)
 * Synchronises the stream before returning; *steps_done = number of token positions written. */
int sr_decode(sr_engine* e, const int32_t* host_slots, int B, int max_new, const int32_t* host_eos, int n_eos,
              int32_t pad_id, int32_t* dev_tokens_out, float* dev_logits_trace, const int32_t* dev_forced, int use_graph,
              void* stream, int* steps_done);

/* Call once after the last sr_load_weight / sr_synth_fill and before the first forward: checks that every tensor arrived and,
 * with lm_weight_dtype = 1, quantises the LM decoder linears in place (see sr_config).  Idempotent. */
int sr_finalize_weights(sr_engine* e, void* stream);

/* Sampled decode on the device -- replaces vllm.LLM.generate with the SamplingParams of vllm_strategy.py:289-309
 * (temperature > 0, top_k <= 1024 with top_k <= 0 = no top-k bound [round 5: nucleus sampling over the whole vocabulary, k_sample_full], 0 < top_p <= 1,
 * repetition_penalty): as sr_decode, but every token is drawn by
 * k_sample (exact top-k, temperature softmax, top-p, one categorical draw with a counter-based RNG keyed by
 * (seed, sequence, step)); with use_graph one captured graph per step includes the draw.  The stream of random numbers is
 * this library's own (vLLM's cannot be reproduced): top_k = 1 equals greedy decode exactly, everything else is pinned
 * distributionally (tests). */
int sr_decode_sample(sr_engine* e, int B, int max_new, const int32_t* host_eos, int n_eos, int32_t pad_id, float temperature,
                     int top_k, float top_p, float repetition_penalty, uint32_t seed, int32_t* dev_tokens_out, int use_graph,
                     void* stream, int* steps_done);

/* Beam search (the reference's num_beams > 1: HF GenerationMixin._beam_search with do_sample=False, early_stopping=False) over the G
 * prompts of the last sr_prefill, W beams each: every prompt is fanned out to W KV slots on the device, and every step (one captured graph
 * with use_graph) feeds each beam its token, runs the forward, takes the top K = max(2, 1 + n_eos) * W candidates running + log_softmax
 * of each group (ties: lower beam * V + token), picks the next W running beams, merges the candidates among the first W that end (an eos
 * token, or the max_new-th token) into the group's finished list with score cum / gen_len^length_penalty, applies HF's early-stop
 * heuristic, and reorders the KV slots (the first child of a parent inherits its slot, the others take the slots of childless parents and
 * get a copy of the parent's generated suffix).  Outputs (host): tokens_out [G][R][max_new] (eos included, then pad_id), scores_out
 * [G][R], lengths_out [G][R] -- the R best finished hypotheses of every group, best first.  Optional (device): dev_logits_trace
 * [max_new][G*W][V] float32 (eager launches), dev_beam_trace [max_new][G*W][2] int32 (parent beam, token; -1 -1 for steps not run,
 * -1 pad_id for a group that has stopped).  Refused, with the value named: G*W > max_batch, W > 8, K > 64, R > W, context overflow,
 * continuous-batching mode.  A new sr_prefill is required afterwards. */
int sr_decode_beam(sr_engine* e, int G, int W, int R, int max_new, const int32_t* host_eos, int n_eos, int32_t pad_id, float length_penalty,
                   int32_t* tokens_out, float* scores_out, int32_t* lengths_out, float* dev_logits_trace, int32_t* dev_beam_trace, int use_graph,
                   void* stream, int* steps_done);

/* One decode step with the token choice left to the caller -- the `sr_decode_step` of SURVEY section 8(B); this is what a
 * sampling caller (temperature / top-k / top-p of vllm_strategy.py:289-309) or the logits-gathering verification
 * mode of the multi-GPU path drives.  Feeds dev_last_ids[b] (int64, device; NULL = the greedy token of the logits the
 * engine holds) to sequence b of the last sr_prefill, runs one forward pass and returns (each optional) the float32
 * logits [B, vocab] and their greedy ids int64 [B].  Asynchronous on `stream`; eos handling is the caller's. */
int sr_decode_step(sr_engine* e, const int64_t* dev_last_ids, int B, float* dev_logits_out, int64_t* dev_next_ids, void* stream);

/* Continuous batching (BASELINE.json configs[2]; replaces vLLM's request-level scheduling behind
 * vllm_strategy.py:156-205): the max_batch batch rows have independent lifecycles, row index = KV-cache slot.
 *   sr_rows_begin : all rows free.
 *   sr_admit      : prefill n sequences into the free rows host_rows[0..n) WITHOUT disturbing running rows; sequence i may
 *                   generate at most host_max_new[i] tokens (its row then reports finished).  Arguments as sr_prefill.
 *   sr_rows_step  : n_steps decode steps for all rows (one hipGraph replay each); a row stops at its first eos token or
 *                   at its limit, later positions are not written.  Asynchronous.
 *   sr_rows_poll  : host copies of the per-row finished flags and generated-token counts (synchronises the stream).
 *   sr_rows_read  : the first n generated tokens of a row (int32, device to device).
 *   sr_rows_abort : the rows host_rows[0..n) stop NOW (their finished flag is set between two steps: no further token is logged,
 *                   nothing more is appended to their KV slot); the next sr_rows_poll reports them finished and the caller may
 *                   re-use row and slot at once -- what vLLM's abort_request does for the reference's ABORT command
 *                   (/root/reference/roll/distributed/strategy/vllm_strategy.py:188-193).
 *   sr_rows_set_cus : a HINT for the decode steps queued on `stream` after it (sr_rows_step, sr_decode, sr_decode_step): they will run on
 *                   n_cus compute units -- a CU-masked stream next to an overlapped admission; 0 = the whole chip, the state after
 *                   sr_engine_create.  With n_cus > 0 the engine replays a second captured form of the step whose gate/up and
 *                   down-projection GEMVs and LM head at 17..32 rows keep their activations in registers / LDS and walk the weight
 *                   tiles (dealt to n_cus blocks): 4.6 % more tiles/s on the headline, 1 % slower on the whole chip.
 *                   Results do not depend on it, bit for bit.
 *   sr_rows_sampling : (optional, after sr_rows_begin) all rows draw their tokens with k_sample (temperature > 0, top_k <= 1024 -- <= 0: no top-k bound --,
 *                   0 < top_p <= 1) instead of the greedy arg-max; temperature 0 switches back. */
int sr_rows_begin(sr_engine* e, void* stream);
int sr_rows_sampling(sr_engine* e, float temperature, int top_k, float top_p, uint32_t seed);
int sr_admit(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
             const int32_t* host_rows, const int32_t* host_max_new, int n, const void* dev_image_embeds, int n_image_rows,
             float* dev_logits_out, void* stream);
/* The admission in two halves, so that its expensive half can run UNDER the running rows' decode steps on another (CU-masked) stream:
 *   sr_admit_stage  : prefill n sequences into SPARE KV slots (sr_config.kv_slots > max_batch), LM head, first token -- touches no row
 *                     state and only admission-owned scratch; at most one staged admission at a time.
 *   sr_admit_commit : install the NEXT n staged sequences (in staging order; several calls may share one staged admission as rows
 *                     free up) into free batch rows (row -> KV slot), on the DECODE stream between two steps; the caller orders it
 *                     after the staging stream's work (event).  sr_admit = stage into slot == row + commit of all. */
int sr_admit_stage(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
                   const int32_t* host_kv_slots, const int32_t* host_max_new, int n, const void* dev_image_embeds, int n_image_rows,
                   float* dev_logits_out, void* stream);
int sr_admit_commit(sr_engine* e, const int32_t* host_rows, int n, void* stream);
/* Fan-out admission (the reference's num_return_sequences n > 1 -- vLLM serves it from one prefill whose KV blocks the n sequences share):
 * n PROMPTS, prompt i becomes host_fanout[i] >= 1 staged sequences, in prompt-major order; host_kv_slots (sr_admit_fanout: host_rows, slot ==
 * row) holds one entry per sequence (sum of host_fanout), sequence j of prompt i takes the j-th of prompt i's entries.  Prompt i is prefilled
 * ONCE, into the slot of its first sequence; the LM head runs once per prompt (dev_logits_out, optional: n rows); one k_kv_fanout launch on
 * `stream` copies every prompt's KV prefix (positions [0, len) of all layers) into the slots of its other sequences before the call returns.
 * Each sequence gets its own first token: the prompt's arg-max (greedy) or its own k_sample draw from the prompt's logits row (sampling mode,
 * the sequence's staged index picks the random stream).  host_max_new has n entries (per prompt).  sr_admit_commit installs the sequences
 * unchanged, in portions as rows free up: the forks of one prompt may start at different steps.  Refused, with the value named: a fanout
 * below 1, more than MAXB (128) sequences in one admission, a slot or row given twice or out of range.  sr_admit_stage / sr_admit are
 * these calls with every fanout 1 (the same code path, no k_kv_fanout launch). */
int sr_admit_stage_fanout(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
                          const int32_t* host_fanout, const int32_t* host_kv_slots, const int32_t* host_max_new, int n,
                          const void* dev_image_embeds, int n_image_rows, float* dev_logits_out, void* stream);
int sr_admit_fanout(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
                    const int32_t* host_fanout, const int32_t* host_rows, const int32_t* host_max_new, int n,
                    const void* dev_image_embeds, int n_image_rows, float* dev_logits_out, void* stream);
/* Per-request sampling in the continuous batcher: one parameter entry per staged SEQUENCE (prompt-major, as the fan-out's slots). */
typedef struct sr_sampling {
    float temperature;          /* 0: greedy -- the arg-max of the (penalised) logits, ties to the lowest id; < 0 refused */
    int32_t top_k;              /* <= 1024 (<= 0: no top-k bound) */
    float top_p;                /* (0, 1] */
    float repetition_penalty;   /* > 0, 1 = none: l > 0 ? l / rp : l * rp on every token of the prompt and of the generated sequence */
    uint32_t seed;              /* the draws of step s use the counter-based key (seed, stream, s) */
    int32_t stream;             /* >= 0: the stream id (e.g. the fork index: tokens that depend on no row, slot, admission order or neighbour);
                                 * < 0: the row's stream of sr_rows_sampling (seed = its seed gives that path's tokens exactly) */
} sr_sampling;
/*   sr_admit_stage_sampling / sr_admit_sampling : sr_admit_stage_fanout / sr_admit_fanout (host_fanout may be null: one sequence per prompt)
 *                   with host_sampling[sum of fanout]: each sequence draws its first token under its own entry, its KV slot's
 *                   repetition-penalty bitmap is cleared and marked with its prompt (forks: each slot gets the prompt), and sr_admit_commit
 *                   installs the entries with the rows.  The first call allocates the per-row state outside the workspace (parameter table
 *                   + one bitmap of ceil(V / 32) words per KV slot); from then on EVERY admission stages entries (the plain calls: the
 *                   sr_rows_sampling configuration, keyed by the row).  Refused by name: temperature < 0, top_k > 1024, top_p outside
 *                   (0, 1], repetition_penalty <= 0.
 *   sr_rows_per_row : on = 1: sr_rows_step replays the per-row step -- greedy, top-k, unbounded nucleus and penalised rows in one captured
 *                   graph (the consumed tokens are marked in their slot's bitmap, k_sample skips the unbounded rows, k_sample_full the
 *                   others) -- instead of the shared greedy / sampled step; 0 = back to the shared step.  With every entry equal to the
 *                   shared configuration both give the same tokens, so the switch may happen between any two steps. */
int sr_admit_stage_sampling(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
                            const int32_t* host_fanout, const int32_t* host_kv_slots, const int32_t* host_max_new,
                            const sr_sampling* host_sampling, int n, const void* dev_image_embeds, int n_image_rows, float* dev_logits_out,
                            void* stream);
int sr_admit_sampling(sr_engine* e, const int64_t* host_ids, const int64_t* host_pos3, const int32_t* host_seq_lens,
                      const int32_t* host_fanout, const int32_t* host_rows, const int32_t* host_max_new, const sr_sampling* host_sampling,
                      int n, const void* dev_image_embeds, int n_image_rows, float* dev_logits_out, void* stream);
int sr_rows_per_row(sr_engine* e, int on, void* stream);
int sr_rows_step(sr_engine* e, int n_steps, const int32_t* host_eos, int n_eos, int32_t pad_id, void* stream);
int sr_rows_poll(sr_engine* e, int32_t* host_finished, int32_t* host_steps, void* stream);
int sr_rows_read(sr_engine* e, int row, int32_t* dev_tokens_out, int n, void* stream);

/* Token log-probs (vLLM's SamplingParams.logprobs = N with raw log-probs; the reference asks logprobs=0 for every rollout,
 * roll/distributed/strategy/vllm_strategy.py:289-309): the engine records, in the step that picks a token, the log-prob of that token and
 * optionally the row's N most likely tokens.
 *   For every generated token of a sequence, with x the float32 logits row that produced it exactly as the LM head stored it:
 *     lp = x[tok] - logsumexp(x)   -- no temperature, no repetition penalty, no top-k / top-p truncation (with temperature 1 and no penalty
 *                                     that is the log-prob under the distribution the token was drawn from before truncation);
 *     top_n = N > 0: the N largest logits of the row ordered by (logit descending, token id ascending), stored as top_ids[N] int32 and
 *                                     top_lp[N] = x[id] - logsumexp(x).  The top arrays always have 8 entries per record: ids past N are -1,
 *                                     their log-probs 0.
 *   A record exists for every logged token of a live row, eos included.  Position 0 comes from the prefill / admission logits (a fork of a
 *   fan-out admission: its prompt's logits row and its own first token; staged sequences carry it until sr_admit_commit installs them).
 *   Positions a static decode pads after a row finished hold lp = 0, top_ids = -1, top_lp = 0, and a row never shows records of its
 *   previous occupant (an admission clears the rest of its row's log).  Greedy rows: top_ids[0] == tok and top_lp[0] == lp bit for bit.
 *   Under teacher forcing (sr_decode's `forced`) the logged token is the arg-max, and so is its record.
 *   Deterministic: every reduction runs in a fixed order and a token's record depends only on its logits row -- not on the batch size, the
 *   row index, the neighbours, graph replay or eager launches, sr_rows_set_cus, or overlapped / plain admission.  NaN logits are outside
 *   the contract; -inf logits are allowed (lp may be -inf); nothing overflows for logits of magnitude 80.
 *   Recorded by sr_decode, sr_decode_sample and sr_rows_step (shared greedy, shared sampled, per-row) inside their captured step, and by
 *   the admissions.  NOT recorded by sr_decode_beam (its scores already are summed log-probs) and sr_decode_step (the caller holds the
 *   logits).  With the switch off (the default) every captured step holds exactly the launches it held before.
 *   sr_logprobs : top_n -1 = off, 0..8 = record with that N from the next step / admission / decode on; anything else is refused (-22, the
 *                 value named).  May be called between any two steps or calls; records are written under the N in force.  The first
 *                 call that switches on allocates the log outside the workspace (max_batch x max_new_tokens records laid out for N = 8,
 *                 cleared), so sr_workspace_bytes and sr_config are unchanged.
 *   sr_rows_read_logprobs : the first n records of a row, device to device: dev_lp float32 [n], and (each optional) dev_top_ids int32
 *                 [n][8], dev_top_lp float32 [n][8].  After sr_decode / sr_decode_sample, row = batch index. */
int sr_logprobs(sr_engine* e, int top_n, void* stream);
int sr_rows_read_logprobs(sr_engine* e, int row, float* dev_lp, int32_t* dev_top_ids, float* dev_top_lp, int n, void* stream);
int sr_rows_abort(sr_engine* e, const int32_t* host_rows, int n, void* stream);
int sr_rows_set_cus(sr_engine* e, int n_cus, void* stream);

/* K19-K22 raster tail -- replaces seg_strategy.py:58-65 (union, cv2.INTER_NEAREST resize),
 * rlvr_socioseg_vlm_pipeline_infer.py:45-58 (IoU counts) and :383-452 (render).  No engine needed. */
int sr_mask_union(uint8_t* dev_acc, const uint8_t* dev_mask, size_t n, void* stream);
int sr_resize_nearest_u8(const uint8_t* dev_src, int sh, int sw, uint8_t* dev_dst, int dh, int dw, void* stream);
/* PIL's Image.resize of 8-bit images (BICUBIC / BILINEAR / LANCZOS), bit for bit -- replaces the host resize in front of the ViT and of SAM2
 * (rlvr_socioseg_vlm_pipeline_infer.py:126-144, seg_strategy.py:44).  n_img equally sized images, contiguous: dev_src [n_img][sh][sw][channels] ->
 * dev_dst [n_img][dh][dw][channels]; any byte alignment.  The horizontal pass (skipped when sw == dw) runs over every source row, the vertical
 * pass (skipped when sh == dh) on its uint8 result in dev_tmp; with both sizes equal the call is a device-to-device copy.  One launch per pass.
 *   dev_kk_h [dw][ksize_h], dev_bounds_h [dw][2], dev_kk_v [dh][ksize_v], dev_bounds_v [dh][2]: the 22-bit fixed-point taps and (first source
 *     index, tap count) of each output index, as socioreasoner_amd/hostops.py pil_resample_coeffs(sw, dw, filter) / (sh, dh, filter) builds
 *     them.  Preconditions (not checked): first >= 0, first + count <= the source size, count <= ksize, both non-decreasing in the output index.
 *   dev_tmp: n_img * sh * dw * channels bytes; may be NULL when at most one pass runs.  dev_src, dev_dst and dev_tmp do not overlap.
 * Returns -22 and launches nothing for: channels not 1 or 3 (PIL resizes RGBA through a premultiplied copy), a side outside 1 .. 8192,
 * n_img < 1, a missing table of a pass that runs, a missing dev_tmp when both passes run. */
int sr_resize_pil_u8(const uint8_t* dev_src, int sh, int sw, uint8_t* dev_dst, int dh, int dw, int channels, int n_img,
                     const int32_t* dev_kk_h, const int32_t* dev_bounds_h, int ksize_h,
                     const int32_t* dev_kk_v, const int32_t* dev_bounds_v, int ksize_v, uint8_t* dev_tmp, void* stream);
int sr_iou_counts(const uint8_t* dev_pred, const uint8_t* dev_gt, size_t n, int64_t* dev_out2, void* stream);
/* the same counts for n_items (prediction, ground truth) pairs of n bytes each, stored back to back, in ONE launch: dev_out [n_items][2] */
int sr_iou_counts_batched(const uint8_t* dev_pred, const uint8_t* dev_gt, size_t n, int n_items, int64_t* dev_out, void* stream);
int sr_render_overlay(uint8_t* dev_img_rgb, int h, int w, const uint8_t* dev_mask, int mh, int mw,
                      const int32_t* dev_boxes, int n_boxes, void* stream);

/* Single-kernel entry points used by the parity tests and micro-benchmarks (same kernels the engine launches).
 * All pointers are device pointers; layouts are documented in DESIGN.md "Kernels".
 * Flag bits OR-ed into `epilogue` / `mode`: 0x100 W fragment-ordered (tiled16x64); sr_op_gemm: 0x200 / 0x400 force the 256- /
 * 128-tile kernel, 0x800 the GELU epilogue through the erfc-polynomial form (|error| 4e-7, SAM2 image encoder), 0x1000 ReLU in its place (SAM2 mask decoder MLPs); sr_op_gemv*: 0x800 x fragment-ordered (tiled16x64 of a [ceil16(M), K] matrix), 0x1000 SwiGLU output
 * fragment-ordered. */
/* ---- SAM2 (Hiera-L) image path behind seg_infer -- /root/reference/roll/distributed/strategy/seg_strategy.py:47-60 calls
 * SAM2ImagePredictor.set_image / predict; the network (transformers/models/sam2/modeling_sam2.py = the sam2 package's) is driven from
 * socioreasoner_amd/sam2.py through sr_op_gemm, sr_op_attention and the passes below.  Token matrices are bf16 [rows][ld], channel-last.
 *   sr_op_attention : softmax(q k^T * scale) v per work item (struct {int q_row0, seq_len, q_off, k_row0; int64 vt_off; int q_len, pad}
 *                     on the device, one item per q_tile queries of a sequence / window); V is passed TRANSPOSED ([head*hd + d][key]).
 *                     head_dim 16 / 32 / 80 / 128 (72 runs as 80 with zero channels).  v2_ok: vt key runs are 16-byte aligned and finite.
 *                     Preconditions (the kernels check none of them; tests/attention_ref.py check_preconditions is their executable form):
 *                       - q_stride, k_stride, k_head_stride and head_dim are multiples of 8 elements and q / k 16-byte aligned (16-byte
 *                         fragment loads); vt 8-byte aligned, vt_stride, vt_head_stride and every vt_off multiples of 4 elements, and each
 *                         V^T key run readable up to the next multiple of 4 keys past seq_len (8-byte loads; what lies past seq_len is
 *                         masked, it may be other data, NaN or inf); out 8-byte aligned and out_stride a multiple of 4.  K rows past
 *                         seq_len are never read (row indices are clamped to seq_len - 1).
 *                       - an item covers queries q_off .. min(q_off + q_tile, q_len ? q_len : seq_len) of its sequence (q_off a multiple
 *                         of q_tile, seq_len >= 1) and writes exactly those rows, columns [0, n_heads * head_dim); kv head = head / group.
 *                       - q_tile 0 / 64: head_dim 128 (causal or not), 80 / 32 / 16 (not causal).  q_tile 16: head_dim 16, not causal
 *                         (<= 16 queries per item, the block's waves split the keys).  Anything else returns -22 before a launch;
 *                         n_work 0 returns 0.
 *                       - v2_ok = 1 additionally promises: vt 16-byte aligned, vt_off, vt_stride and vt_head_stride multiples of 8; every
 *                         V^T row allocated and FINITE up to the end of the last 64-key tile of its run (those values are multiplied by
 *                         P = 0, not masked); items cut at q_tile queries.  It is used when n_heads % 4 == 0 and (head_dim 128, causal,
 *                         q_tile 64, group % 4 == 0) or (head_dim 80, not causal, q_tile 128, group 1), with bit-identical results;
 *                         q_tile 128 without it is refused.
 *   The passes below work on row-major matrices [rows][ld] with C live columns (bf16 here, float32 in the _f32 forms further down).
 *   Preconditions (the kernels check none of them unless a refusal is named; tests/sam2_ops_ref.py check_preconditions is their
 *   executable form): every matrix holds (rows - 1) * ld + C elements from its pointer, ld >= C; elements are naturally aligned; an op
 *   writes the live columns of its output rows and nothing else unless pad columns are named; what lies in the pad columns [C, ld) and in
 *   the rows past the end of an input is never read (it may be NaN or inf).  Outputs may not overlap inputs except where "in place" is
 *   named.  Rounding: one rounding to the storage type per op, float32 arithmetic inside.
 *   sr_op_sam_preprocess : uint8 HWC [h][w][3] -> CHW [3][S][S]: /255, bilinear resize (align_corners false, no antialiasing), ImageNet
 *                     normalisation.  h, w, S >= 1; img holds h * w * 3 bytes, out 3 * S * S elements.
 *   sr_op_im2col    : k x k / stride / pad windows of a CHW image [3][S][S] -> rows [(ty, tx)][c * k * k + ky * k + kx] of T * T tokens,
 *                     T = (S + 2 pad - k) / stride + 1 >= 1 (floor); zero beyond the image and in the pad columns [3 k k, ld), which this
 *                     op owns.  rowmap (NULL = identity): T * T DISTINCT destination rows in [0, T * T).  ld < 3 k k returns -22.
 *   sr_op_layernorm : LayerNorm with bias over C channels of each of `rows` rows (two-pass float32 statistics); the pad columns [C, ldo)
 *                     are written as zeros, so out holds rows * ldo elements.  1 <= C <= ldo, ldx >= C; w and b hold C elements.  C or ldo
 *                     above 1152 returns -22; rows <= 0 returns 0.  In place (out == x, ldo == ldx) is allowed.  bf16: 16-byte accesses
 *                     when C, ldx and ldo are multiples of 8 and x, w, b, out 16-byte aligned, one channel per lane otherwise -- the same
 *                     formula and rounding point, the statistics summed in another order.
 *   sr_op_maxpool_win : 2 x 2 max pooling of tokens stored window by window: [n_win][ws * ws] rows -> [n_win][(ws / 2)^2] rows, C columns.
 *                     n_win >= 1, ws >= 2; an odd ws returns -22.
 *   sr_op_ew        : mode 0 a + b, 1 a + row vector b[0 .. C), 2 relu(a), 3 gelu(a) (erf form), 4 silu(a) * b; rows x C elements with
 *                     leading dimensions lda / ldb / ldo.  b is not read in modes 2 / 3.  In place on a (out == a, ldo == lda) is allowed.
 *                     rows <= 0 returns 0.
 *   sr_op_transpose : out[c][r] = in[r][c] for rows x cols (bf16 only); writes columns [0, rows) of `cols` output rows, ld_out >= rows.
 *                     16-byte accesses when cols, ld_in, ld_out are multiples of 8 and both pointers 16-byte aligned (any rows), element by
 *                     element otherwise; the same bits either way.
 *   sr_op_upsample2x_add : FPN top-down step out[y][x] = lat[y][x] + top[y / 2][x / 2] on an H2 x H2 grid of rows (top: H2 / 2 x H2 / 2),
 *                     one ld for all three.  An odd H2 returns -22 (the top map has no row for y / 2 of the last row).
 *   sr_op_pixel_shuffle_add : second half of a 2 x 2 / stride 2 transposed convolution: the GEMM wrote g [W * W][co * 4 + dy * 2 + dx]
 *                     (ldg >= 4 Co); out[(2y + dy) * 2W + 2x + dx][co] = g[y * W + x][co * 4 + dy * 2 + dx] + feat[same row][co], 4 W W rows.
 *   sr_op_mask_resize_or : low float32 [m * m][ld], column col0 + i = logit map i of n >= 1 (col0 + n <= ld); best = the FIRST arg-max of
 *                     score[col0 .. col0 + n) (finite); that map, bilinear (align_corners false) to h x w, sets acc[i] = 1 where > 0 and
 *                     leaves acc alone elsewhere (acc: h * w bytes, the running union).  logits_out (NULL or float32 [n][h * w]) receives all
 *                     n resized maps and does not change acc.
 *   sr_op_gather_rows : out[i] = in[rows[i]] for n rows of H bf16 elements (a float32 row of H / 2 floats is gathered with the doubled H);
 *                     16 bytes per lane: in and out 16-byte aligned, rows[i] in range; H % 8 != 0 returns -22, n <= 0 returns 0. */
int sr_op_attention(const void* q, int q_stride, const void* k, int k_stride, long long k_head_stride, const void* vt, int vt_stride,
                    long long vt_head_stride, void* out, int out_stride, const void* dev_work, int n_work, int n_heads, int group, float scale,
                    int causal, int head_dim, int q_tile, int v2_ok, void* stream);
int sr_op_sam_preprocess(const uint8_t* img, int h, int w, void* out_chw, int S, void* stream);
int sr_op_im2col(const void* chw, int S, int k, int stride, int pad, void* out, int ld, const int32_t* rowmap, void* stream);
int sr_op_layernorm(const void* x, int ldx, const void* w, const void* b, void* out, int ldo, int rows, int C, float eps, void* stream);
int sr_op_maxpool_win(const void* in, int ld_in, int C, int n_win, int ws, void* out, int ld_out, void* stream);
int sr_op_ew(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int rows, int C, int mode, void* stream);
int sr_op_transpose(const void* in, int ld_in, int rows, int cols, void* out, int ld_out, void* stream);
int sr_op_upsample2x_add(const void* lat, const void* top, void* out, int H2, int C, int ld, void* stream);
int sr_op_pixel_shuffle_add(const void* g, int ldg, const void* feat, int ldf, void* out, int ldo, int W, int Co, void* stream);
int sr_op_mask_resize_or(const float* low, int ld, int col0, int n, int m, const float* score, uint8_t* acc, float* logits_out, int h, int w, void* stream);
int sr_op_gather_rows(const void* in, const int32_t* rows, void* out, int n, int H, void* stream);
int sr_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, void* out, int ldo, const void* bias,
               const void* resid, const int32_t* rowmap, int epilogue, void* stream);
/* ---- SAM2 at the REFERENCE's precision.  The reference builds SAM2ImagePredictor(build_sam2(...)) in float32 and calls it without
 * autocast (/root/reference/roll/models/model_providers.py:540-548, roll/distributed/strategy/seg_strategy.py:47-60): these are the
 * float32 forms of the entry points above (same argument meaning, preconditions and refusals, float32 row-major matrices [rows][ld]; the
 * GEMM and the attention need ld % 4 == 0 and 16-byte aligned pointers, the passes access element by element and take any ld >= C)
 * that socioreasoner_amd/sam2.py drives when Sam2Engine(dtype=float32) -- the default behind seg_infer.
 *   sr_op_gemm_f32      : out = act(A . W^T + bias) (+ resid), float32 in and out; epilogue 0 store, 1 residual, 3 GELU (erf form; | 0x1000 =
 *                         ReLU), 4 = 0; K % 16 == 0, N % 4 == 0.  Round 5: computed on the bf16 matrix pipe from an exact three-term bf16 split of
 *                         every operand (six partial products, float32 accumulation: float32-grade results at 2-3 x the rate of the f32-input
 *                         MFMA, which SR_SAM_F32_SPLIT=0 selects instead).  The split is exact for finite operands inside bf16's range (|x| < 3.39e38):
 *                         beyond it, and for +-inf, hi rounds to inf and the remainders turn NaN where the f32-input kernel returns inf.
 *   sr_op_attention_f32 : softmax(q k^T * scale) v per work item (the struct of sr_op_attention, <= 64 queries per item; vt_off unused:
 *                         V is ROW-major, element (key j, head h, d) = v[(k_row0 + j) * v_stride + h * head_dim + d]); head_dim 16 / 32 / 80. */
int sr_op_gemm_f32(const float* A, int lda, const float* W, int M, int N, int K, float* out, int ldo, const float* bias, const float* resid,
                   const int32_t* rowmap, int epilogue, void* stream);
int sr_op_attention_f32(const float* q, int q_stride, const float* k, int k_stride, const float* v, int v_stride, float* out, int out_stride,
                        const void* dev_work, int n_work, int n_heads, float scale, int head_dim, void* stream);
/* ---- float32 VERIFICATION path (round 6).  north_star asks for logits "within 1e-3 of the reference's eager path"; with bf16 activations no implementation,
 * HF against itself included, meets that.  These entry points complete the float32 ops above to the whole Qwen2.5-VL forward -- ViT,
 * merger, LM prefill and KV-cache decode with float32 activations on the same bf16-representable weights -- so that tests/f32_path.py can hold the arithmetic
 * this library implements (RMSNorm eps and form, softmax scale, rotary angles, SiLU / GELU forms, GQA mapping, causal mask) to max |dlogit| <= 1e-3 against HF
 * run in float32 (/root/reference/roll/distributed/strategy/hf_strategy.py:49-94 with torch_dtype float32; tests/golden/hf_truth3b.npz).  Not a serving path.
 *   sr_op_attention_f32_causal : sr_op_attention_f32 with the causal mask (query i of an item sees keys 0 .. seq_len - queries + q_off + i); head_dim 128 too.
 *   sr_op_rmsnorm_f32          : out = w * x * rsqrt(mean(x^2) + eps) per row (hf:65-79 without the bf16 roundings), C <= 8192.
 *   sr_op_rope_table_f32       : cos | sin [n_pos][n_freq] of pos[i] * inv_freq[f] -- the device cosf / sinf the engine's bf16 rotary tables are rounded from.
 *   sr_op_rope_f32             : x <- x * cos + rotate_half(x) * sin in place for n_heads heads of head_dim columns; cos / sin rows [rows][ldc >= head_dim].
 *   sr_op_ew_f32 mode 4        : silu(a) * b with the engine's own silu_f. */
int sr_op_attention_f32_causal(const float* q, int q_stride, const float* k, int k_stride, const float* v, int v_stride, float* out, int out_stride,
                               const void* dev_work, int n_work, int n_heads, float scale, int head_dim, void* stream);
int sr_op_rmsnorm_f32(const float* x, int ldx, const float* w, float* out, int ldo, int rows, int C, float eps, void* stream);
int sr_op_rope_f32(float* x, int ld, const float* cos_t, const float* sin_t, int ldc, int rows, int n_heads, int head_dim, void* stream);
int sr_op_rope_table_f32(const float* inv_freq, int n_freq, const int32_t* pos, int n_pos, float* cos_t, float* sin_t, void* stream);
int sr_op_sam_preprocess_f32(const uint8_t* img, int h, int w, float* out_chw, int S, void* stream);
int sr_op_im2col_f32(const float* chw, int S, int k, int stride, int pad, float* out, int ld, const int32_t* rowmap, void* stream);
int sr_op_layernorm_f32(const float* x, int ldx, const float* w, const float* b, float* out, int ldo, int rows, int C, float eps, void* stream);
int sr_op_maxpool_win_f32(const float* in, int ld_in, int C, int n_win, int ws, float* out, int ld_out, void* stream);
int sr_op_ew_f32(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int C, int mode, void* stream);
int sr_op_upsample2x_add_f32(const float* lat, const float* top, float* out, int H2, int C, int ld, void* stream);
int sr_op_pixel_shuffle_add_f32(const float* g, int ldg, const float* feat, int ldf, float* out, int ldo, int W, int Co, void* stream);
/* fp8 x fp8 prefill GEMM on the block-scaled MFMA (BASELINE.json configs[4]): sr_op_quant_mx quantises bf16 activations [M][ldx] to
 * OCP-MX e4m3 (q [M][K] bytes + e8m0 scales [K/128][rows_pad][4]); sr_op_gemm_mx multiplies them with an fp8 weight image (tiled8,
 * per-output-channel float32 scale) -- out = bf16((q_x . q_w^T with block scales) * w_scale + bias), epilogues 0 / 1 / 2 / 4 as sr_op_gemm */
int sr_op_quant_mx(const void* x, int ldx, int M, int K, void* q, void* scales, int rows_pad, void* stream);
int sr_op_gemm_mx(const void* A8, int lda, const void* a_scale, int a_rows_pad, const void* W8, const float* w_scale, int M, int N, int K, void* out,
                  int ldo, const void* bias, const void* resid, int epilogue, void* stream);
/* The vision tower's fp8 mode (sr_config.v_weight_dtype = 2) at op level:
 *   sr_op_rmsnorm_mx    : per-row RMSNorm over C channels fused with the MX quantiser -- the bytes of sr_op_rmsnorm (its wave-per-row form)
 *                         followed by sr_op_quant_mx on the [rows / group][group * C] view (`group` normalised rows = one GEMM row)
 *   sr_op_gemm_mx_vit   : sr_op_gemm_mx with the operands the tower's epilogues need beyond it: a destination row map (epilogues 0 / 1 / 3),
 *                         and for epilogue 6 (qkv Linear + 2-D rotary on the PAIRED q / k channel order + V^T write; N = 3 * heads * head_dim)
 *                         the float32 tables [row][head_dim / 2] and V^T [N / 3][vt_stride]; epilogue 3 = GELU
 *   sr_op_quant_f8_rows : fp8 image (tiled8) + per-channel scales of a ROW-MAJOR bf16 matrix [N][K], which is left unchanged */
int sr_op_rmsnorm_mx(const void* x, const void* w, void* q, void* scales, int rows, int C, int group, int rows_pad, float eps, void* stream);
int sr_op_gemm_mx_vit(const void* A8, int lda, const void* a_scale, int a_rows_pad, const void* W8, const float* w_scale, int M, int N, int K, void* out,
                      int ldo, const void* bias, const void* resid, const int32_t* rowmap, const float* cos_t, const float* sin_t, void* vt, int vt_stride,
                      int head_dim, int epilogue, void* stream);
int sr_op_quant_f8_rows(const void* w, int N, int K, void* w8, float* scale, void* stream);
int sr_op_gemv(const void* x, int ldx, const void* W, int M, int N, int K, void* out, int ksplit, int mode, void* stream);
/* decode GEMV with its fusions (mode 3 = bias epilogue, 4 = residual epilogue in place; norm_w != NULL = RMSNorm
 * prologue, optionally after adding n_slabs float32 slabs [n_slabs][M][K]; amax_* = per-block argmax partials of the
 * float32 mode, row length sr_op_gemv_f32_blocks(N, M, K, norm_w != NULL)) */
int sr_op_gemv_fused(const void* x, int ldx, const void* W, int M, int N, int K, void* out, int ldo, int mode, const void* bias,
                     const void* norm_w, float eps, const float* slabs, int n_slabs, void* x_out, float* amax_val,
                     int32_t* amax_idx, void* stream);
/* the CU-count hint of sr_rows_set_cus for the op-level GEMVs (sr_op_gemv / sr_op_gemv_fused at 17..32 rows; process-wide, one stream at a time): 0 = the whole
 * chip = the streaming kernels, n > 0 = the x-stationary forms dealt to n blocks (n >= the device's CU count: one block per CU) */
int sr_op_gemv_set_cus(int n_cus, void* stream);
int sr_op_gemv_f32_blocks(int N, int M, int K, int has_norm);
/* fused decode attention: qkv rows (bias applied, pre-rope) -> mRoPE -> KV-cache append -> attention; slots = identity.
 * kcache [B][kvh][ctx_max][128], vtcache [B][kvh][128][ctx_max]; ctx_len counts the new token; rope_cos/sin: bf16 [max_pos+1][64] tables; scores_scratch: bf16 [B][heads][ctx_max] */
int sr_op_attn_decode(const void* qkv, int qkv_stride, const int32_t* pos, const int32_t* ctx_len, const void* rope_cos,
                      const void* rope_sin, void* kcache, void* vtcache, void* out, int out_stride, int B, int n_q_heads, int n_kv_heads, int ctx_max,
                      float scale, void* scores_scratch, void* stream);
int sr_op_rmsnorm(const void* x, const void* w, void* out, int rows, int H, float eps, void* stream);
int sr_op_resid_rmsnorm(void* x, const float* partials, int ksplit, const void* w, void* out, int rows, int H, float eps,
                        void* stream);
int sr_op_argmax(const float* logits, int rows, int V, int32_t* out_idx, void* stream);
/* the log-prob kernels of sr_logprobs alone, on caller-provided buffers: record i (0 <= i < rows <= 128) reads the float32 logits row
 * row_map[i] (int32, device; null: i) of `logits` (leading dimension ld >= V >= 16; columns V .. ld are never read) and the token
 * dev_tokens[i] (int64, device; null: the arg-max, lowest id among the maxima) -> lp [rows], tok_out int32 [rows] (optional), top_ids int32
 * [rows][8] and top_lp [rows][8] (optional, both or neither; entries past top_n hold -1 / 0).  0 <= top_n <= 8.  Nothing else is written.
 * NOT thread-safe: the call keeps one process-wide scratch buffer for the chunk partials, grown (after a device synchronize) when a call needs more;
 * call it from one thread at a time and on one device. */
int sr_op_token_logprobs(const float* logits, int64_t ld, int rows, int V, const int64_t* dev_tokens, const int32_t* row_map, int top_n, float* lp,
                         int32_t* tok_out, int32_t* top_ids, float* top_lp, void* stream);
/* the fan-out kernel of sr_admit_stage_fanout on caller-provided caches kcache [layer][slot][kvh][max_ctx][128], vtcache
 * [layer][slot][kvh][128][max_ctx] (layer_stride_elems elements from one layer to the next in each): positions [0, L) of slot src_slot ->
 * slots dev_dst_slots[0..d) (int32, device), all layers, one launch; nothing else is written.  max_ctx % 64 == 0. */
int sr_op_kv_fanout(void* kcache, void* vtcache, int n_layers, int64_t layer_stride_elems, int n_kv_heads, int max_ctx, int src_slot,
                    const int32_t* dev_dst_slots, int d, int L, void* stream);
/* the KV suffix copy of sr_decode_beam on caller-provided caches (layout as sr_op_kv_fanout): for each of the n entries (src slot, dst slot,
 * L0, L1) of dev_copies (int32 [n][4], device; src < 0: skipped), positions [L0, L1) of src -> dst, all layers, one launch; nothing else
 * is written.  max_len >= every L1 - L0 sizes the grid. */
int sr_op_kv_suffix_copy(void* kcache, void* vtcache, int n_layers, int64_t layer_stride_elems, int n_kv_heads, int max_ctx,
                         const int32_t* dev_copies, int n, int max_len, void* stream);
/* one beam-search step (row statistics + group select of sr_decode_beam, no KV reorder) on caller-provided float32 logits [G*W, V] and
 * device state: dev_scores float32 [G*W] running scores (in / out), dev_fin [G*W] finished entries (float score, int32 step, parent beam,
 * token: 16 bytes each, best first) with counts dev_fin_n int32 [G] (in / out), dev_done int32 [G] stop flags (in / out), dev_trace int32
 * [max_new][G*W][2] (row `step` written: parent beam, token), dev_next_tok int64 [G*W].  Synchronous. */
int sr_op_beam_select(const float* dev_logits, int G, int W, int V, const int32_t* host_eos, int n_eos, int step, int max_new,
                      float length_penalty, int32_t pad_id, float* dev_scores, void* dev_fin, int32_t* dev_fin_n, int32_t* dev_done,
                      int32_t* dev_trace, int64_t* dev_next_tok, void* stream);
/* the sampling kernel on caller-provided float32 logits [B, V]; dev_seen: optional bitmask [B][(V+31)/32]; dev_step: optional
 * int32 [B]; dev_blk_max: optional per-block maxima [B][n_blk] of blk_rows consecutive ids each (the LM head's argmax partials):
 * the exact top-k is then searched only in the blocks that can contain it */
int sr_op_sample(const float* dev_logits, int B, int V, float temperature, int top_k, float top_p, float repetition_penalty,
                 const uint32_t* dev_seen, uint32_t seed, const int32_t* dev_step, int64_t* dev_out, const float* dev_blk_max,
                 int n_blk, int blk_rows, void* stream);
/* fp8 quantisation of a fragment-ordered bf16 matrix (the kernel sr_finalize_weights runs): dev_w8 [N*K] bytes (tiled8),
 * dev_scale float32 [N]; W itself becomes the bf16 image of q */
int sr_op_quant_f8(void* dev_w_tiled, int N, int K, void* dev_w8, float* dev_scale, void* stream);
/* decode GEMV on an fp8 weight image: mode 0 PARTIAL / 1 SWIGLU / 3 BIAS / 4 RESID as sr_op_gemv_fused */
int sr_op_gemv_f8(const void* x, int ldx, const void* w8, const float* w_scale, int M, int N, int K, void* out, int ldo, int mode,
                  const void* bias, const void* norm_w, float eps, int ksplit, void* stream);
int sr_version(void);
/* The library's SR_* tuning / test switches ("Switches") are read from the environment once -- at the first call that
 * needs one and again at every sr_engine_create -- never in per-call dispatch.  A caller that changes one of them inside a running process
 * (the bit-identity tests do) calls this to have the environment read again.  No reference counterpart (vLLM reads its VLLM_* variables at
 * import: roll/distributed/strategy/vllm_strategy.py:13-30). */
int sr_switches_reload(void);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SOCIOR_H */
