/*
 * emmax.h -- C ABI of libemmax_hip.so: the MI355X-native (gfx950) Emma-X VLA forward/generate hot path.
 *
 * The reference (declare-lab/Emma-X) has NO FFI/plugin ABI: its extension point is HuggingFace Auto-class registration
 * of pure-Python nn.Modules (experiments/robot/openvla_utils.py:38-41).  This header is therefore the boundary a
 * maintainer would bind from Python (ctypes) in place of the third-party math the reference calls:
 *
 *   emmax_vision_encode*   replaces PrismaticVisionBackbone.forward + PrismaticProjector.forward
 *                          (prismatic/extern/hf/modeling_prismatic.py:114-123, 146-158; native twin
 *                          prismatic/models/backbones/vision/dinosiglip_vit.py:142-147, prismatic/util/nn_utils.py:37-53)
 *   emmax_prefill          replaces the multimodal branch of PrismaticForConditionalGeneration.forward
 *                          (modeling_prismatic.py:362-415: embed, splice [BOS]+patches+text[1:], LlamaForCausalLM prefill)
 *   emmax_decode_step      replaces the cached branch (modeling_prismatic.py:325-341) + one greedy step of
 *                          transformers GenerationMixin.generate (invoked at modeling_prismatic.py:519,
 *                          prismatic/models/vlms/prismatic.py:659-663)
 *   emmax_generate         replaces the whole greedy loop (<= max_new_tokens, EOS stop) without a host sync per token
 *   emmax_prefill_logits   replaces `forward(...).logits` (all positions), for API parity of `forward()`
 *   emmax_op_*             single-kernel entry points, used by the parity tests
 *
 * Conventions: every function returns 0 on success or a negative emmax_status; emmax_last_error() gives the message of
 * the last failure on the calling thread.  All pointers named *_dev are device pointers owned by the caller; the
 * library never allocates device memory (the caller passes arenas sized by the *_bytes queries).  `stream` is a
 * hipStream_t (NULL = default stream).  Handles are thread-compatible (one thread per handle at a time).  bf16 tensors
 * are raw uint16_t bit patterns.  No torch types cross this boundary.
 */
#ifndef EMMAX_H
#define EMMAX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever emmax_config / emmax_tower_config change layout or an entry point changes signature.
 *   1: rounds 1-2;  2: emmax_config grew `decode_fp8` (round 2, not bumped then);  3: round 4 -- emmax_config_size / emmax_tuning_*
 *   added, the lab-only entry points (persistent layer chain, in-attention split merge) removed;  4: round 5 -- emmax_session_*_ex (staging rows
 *   are asked for, the plain calls give none), decode batches / slot counts up to 64 (emmax_model_max_decode_batch);  5: exact numerics (emmax_session_exact, emmax_op_x_*);
 *   6: emmax_op_sample (seeded sampling over rows of logits);  7: sampling inside the decode step (emmax_session_set_sampling and the calls
 *   around it), the workspace grew the per-row sampling state;  8: logits processors and scores inside the decode step
 *   (emmax_session_set_processing, emmax_session_set_scores and the calls around them), the workspace grew the per-row processing state and
 *   prompt ids;  9: beam search inside the decode step (emmax_session_set_beams and the calls around it), the workspace grew the beam
 *   state and trace; the paged KV region did not grow;  10: emmax_op_decode_stage / emmax_op_decode_kv_read (one decode stage through the step's
 *   own dispatch), the workspace grew that op's per-row scratch;  11: emmax_config.decode_fp8 = 2 selects MXFP4 decode weights (the struct keeps
 *   its layout), emmax_op_quant_mxfp4 / emmax_op_dequant_mxfp4 / emmax_op_gemm_small_mxfp4;  12: the prefill's stage kernels one by one (emmax_op_gemm_stream, emmax_op_rmsnorm_f32,
 *   emmax_op_rope_kv_write, emmax_op_kv_quant_rows, emmax_op_embed_splice, emmax_op_gather_last_rows): new symbols only; still 12: MXFP4 at 17-64 rows
 *   (tuning switch mx4_wide, emmax_model_mxfp4_wide, emmax_op_gemm_wide_mxfp4): new symbols only; still 12: top-N and watched-token
 *   log-probabilities (emmax_op_top_logprobs, emmax_session_set_top_logprobs and the calls around it): new symbols only, the workspace grew
 *   their six device words and the watch list (1.3 KB); still 12: extending a cached context (emmax_extend, emmax_slot_extend,
 *   emmax_session_context, emmax_op_extend_attention(_kv8), emmax_op_rope_kv_write_at, emmax_extend_attn_plan): new symbols only, the workspace
 *   grew one int32 per decode row; still 12: taps -- hidden states and attention maps out of the passes (emmax_session_set_pass_taps,
 *   emmax_session_set_step_taps, emmax_session_clear_taps, emmax_session_taps, emmax_op_attn_probs(_kv8), emmax_op_tap_rows): new symbols only, the
 *   workspace did not grow; still 12: emmax_gemm_launches (the GEMM's kernel launches as text, host only): a new symbol only; still 12: scoring
 *   without logits (emmax_prefill_score, emmax_op_score_rows, emmax_score_plan): new symbols only, the workspace did not grow; still 12: draft-verified
 *   greedy decoding (emmax_verify, emmax_session_set_budget, emmax_session_output, emmax_op_verify_accept): new symbols only, the workspace did not grow;
 *   still 12: emmax_config.decode_fp8 = 4 selects MXFP6 decode weights (the struct keeps its layout; 3 stays refused), emmax_op_quant_mxfp6 /
 *   emmax_op_dequant_mxfp6 / emmax_op_gemm_small_mxfp6: new symbols only. */
#define EMMAX_ABI_VERSION 12

typedef enum emmax_status {
    EMMAX_OK = 0,
    EMMAX_ERR_INVALID = -1,     /* bad argument / shape / config outside the hot path          */
    EMMAX_ERR_MISSING = -2,     /* finalize: a required weight was never bound                  */
    EMMAX_ERR_NOMEM = -3,       /* arena / workspace too small                                  */
    EMMAX_ERR_HIP = -4,         /* a HIP runtime call failed                                    */
    EMMAX_ERR_STATE = -5        /* call order violated (e.g. decode before prefill)             */
} emmax_status;

typedef enum emmax_dtype { EMMAX_BF16 = 0, EMMAX_F32 = 1, EMMAX_U8 = 2, EMMAX_I32 = 3 } emmax_dtype;

typedef void* emmax_stream;            /* hipStream_t */
typedef struct emmax_model emmax_model;
typedef struct emmax_session emmax_session;

/* One timm ViT tower as the reference instantiates it (modeling_prismatic.py:78-101). */
typedef struct emmax_tower_config {
    int32_t embed_dim, depth, num_heads, mlp_hidden;
    int32_t has_cls, n_reg, layerscale;
    int32_t patch, image_size;
    int32_t take_index;                /* block whose output is returned: depth-2 (modeling_prismatic.py:86,100) */
    float ln_eps;
    float mean[3], std[3];             /* per-tower normalisation (processing_prismatic.py:136-139)              */
} emmax_tower_config;

typedef struct emmax_config {
    emmax_tower_config tower[2];       /* [0]=featurizer (DINOv2), [1]=fused_featurizer (SigLIP)                  */
    int32_t hidden, inter, n_layers, n_heads, n_kv_heads, head_dim, vocab;
    float rms_eps, rope_theta;
    int32_t bos_id, eos_id, pad_id;
    int32_t decode_fp8;                /* the decode weight format.  0: bf16 weights (the headline path); 1: the decode projections stream an
                                          fp8-e4m3 (per-row scale) weight copy, de-quantised in registers (BASELINE config 5); 2: MXFP4 (OCP MX
                                          v1.0: e2m1 elements, one e8m0 scale per 32 elements along K; 4.25 bits per weight), widened to bf16 in
                                          registers -- decode batches 1-16 (17-64 too for a model created under the tuning switch mx4_wide), LLM shapes with hidden and n_heads * head_dim in multiples of 1024
                                          up to 4096 and an intermediate size % 128 == 0 in 4097..12288 (emmax_model_create refuses others); the
                                          prefill reads the de-quantised values, so prefill and decode evaluate the same quantised model;
                                          4: MXFP6 (OCP MX v1.0, e2m3 elements: sign, two exponent bits, three mantissa bits -- +-{0, 0.125 .. 0.875,
                                          1 .. 1.875, 2 .. 3.75, 4 .. 7.5} -- and the same e8m0 scale per 32 elements along K; 6.25 bits per
                                          weight; e3m2 is not built), widened to bf16 in registers -- decode batches 1-16, the LLM shapes of MXFP4,
                                          the de-quantised values in the prefill's rows as for MXFP4: one model for every pass (prefill, extend,
                                          verify, scoring, taps, decode).  3 is no format: refused                                               */
} emmax_config;

const char* emmax_version(void);
const char* emmax_last_error(void);
int emmax_abi_version(void);
/* sizeof(emmax_config) as the LIBRARY was compiled: a binding whose mirror struct has another size must refuse to call
 * emmax_model_create (it would be read out of bounds).  emma-x_amd/emmax/_lib.py checks it at load time. */
int emmax_config_size(void);

/* Tuning switches: a fixed table of named integers (emma-x_amd/csrc/kernels.h, struct EmmaxTune).  The library reads the
 * environment variable EMMAX_<NAME> for each of them ONCE, the first time any value is needed; afterwards only emmax_tuning_set
 * changes them (no launcher reads the environment).  Every default is the product path; the other values are the A/B partners
 * DESIGN.md quotes.  Names: graph (1 = hipGraph replay of the decode step, BASELINE configs[4]), ks, ks_oproj, ks_oproj_grid, km,
 * km_down, km_roll, streamk, fp8_gemv, attn_nsplit, attn_direct, attn_nw, attn_deep, attn_group (-1 = the grouped decode attention at the batches it was measured faster at, 1 = wherever it applies, 0 = never), attn_ksplit, attn_lazy, vis_streams, fold_embed, mfma_xbar, gemm_big (2 = the 128 x 256 x 32 lab tile), gemm_splitk, gemm_sk_big,
 * gemm_hybrid, gemm_normfuse, gemm_deep, gemm_lnfuse, attn_resident, resid32 (1 = fp32 residual stream in prefill and decode, 2 = decode only,
 * 0 = bf16 rows), kv_fp8 (1 = sessions created from now on keep an e4m3 KV cache), mx4_wide (1 = MXFP4 models created from now on serve decode
 * batches of 17-64 rows too; 0, the default: 1-16).
 * Four switches are read when an object is BUILT and frozen in it: gemm_lnfuse at emmax_model_finalize (the LayerNorm fold rewrites the ViT
 * qkv / fc1 weights in place: setting it afterwards does not change a finalized model), km at emmax_model_build_aux (which copies exist),
 * kv_fp8 at emmax_session_create (the cache format), mx4_wide at emmax_model_create (emmax_model_mxfp4_wide; emmax_config_max_decode_batch has
 * no model and reads it as it stands at the call).
 * exact (round 6; 0 = off, the default): EXACT NUMERICS -- the reference's fp32 CPU arithmetic (prismatic/models/vlms/prismatic.py:659-663 under
 * BASELINE configs[0]) instead of bf16 operands: fp32 activations end to end, every activation operand of a bf16 MFMA / dot2 as TWO bf16 terms
 * hi + lo (the checkpoint's weights are exact bf16), attention on the fp32 MFMA over an fp32 KV cache.  Read at emmax_model_finalize (the ViT
 * LayerNorms stay unfolded: the fold rounds W .* gamma) and at emmax_session_create (fp32 scratch, fp32 cache = twice the KV bytes).  Exact
 * sessions run on bf16 weights, 8 rows per projection launch (1-2: decode_ks.hip's two-term dot products; 3-8: decode_km.hip with the two terms of a row
 * in the MFMA's sixteen batch columns; larger batches, up to 64 rows / slots, in chunks of 8 that each stream the weights again), slot serving included; emmax_session_exact() tells which kind a session is.  Logits sit
 * ~1e-5 of max|logit| from the fp32 restatement at full depth (default path: 2.4e-2) -- measured cost in DESIGN.md section 6.
 * Not thread-safe against concurrent launches; a session re-captures its decode graph after a change. */
int emmax_tuning_set(const char* name, int value);
int emmax_tuning_get(const char* name, int* value_out);

/* ---- model: weights ------------------------------------------------------------------------------------------------
 * bind every tensor of the HF state dict (key names: vla-scripts/extern/convert_openvla_weights_to_hf.py:74-116) as a
 * bf16 device pointer, then finalize(): all weights are re-laid-out into `arena` (kernel-native: fused QKV rows,
 * 16-row interleaved gate/up, K/N padded to tile multiples, im2col-ordered patch-embed; fp8 models: plus the e4m3 copies).
 * After finalize the bound pointers are no longer referenced and may be freed. */
int emmax_model_create(const emmax_config* cfg, emmax_model** out);
void emmax_model_destroy(emmax_model* m);
int emmax_model_bind_weight(emmax_model* m, const char* hf_key, const void* ptr_dev, int dtype,
                            const int64_t* shape, int ndim);
int64_t emmax_model_arena_bytes(const emmax_model* m);
/* rows of one decode batch / slot set this model can run: the largest B <= 64 such that every projection launch of every step of 1 .. B
 * rows is taken by a launcher family -- asked of the launchers' own shape checks (emmax_op_decode_route answers the same question per stage),
 * under the tuning switches as they are now.  64 (bf16 or fp8 weights) when every LLM projection is a shape the K-split MFMA kernels take
 * (K % 256 (fp8: % 512) == 0 and <= 4096, N <= 32768, intermediate size % 32 (fp8: % 64) == 0 and <= 11264: LLaMA-2-7B is), else usually 8.
 * emmax_model_max_decode_batch_exact: the same for exact-numerics sessions (8 rows per launch, larger batches in chunks of 8): 64 on the
 * shapes decode_km.hip's two-term kernels take, 2 where only decode_ks.hip's do, 0 on fp8 / MXFP4 / MXFP6 weights.
 * MXFP4 models (decode_fp8 = 2): 16 -- decode_km.hip is the only kernel family that reads the 4-bit tiles -- or 8 when a batch of nine rows would
 * split the attention (the o-proj then reads split partials, which its 16-row form does not take); emmax_session_bytes / create refuse a larger
 * max_batch for such a model, naming the format (a model created under the tuning switch mx4_wide: emmax_model_mxfp4_wide below).  The one-split rule reads the tuning switches attn_direct / attn_nsplit: the limit is checked when a
 * session is sized and created and again at every prefill and emmax_slots_open, not inside a step -- changing those switches between a prefill of
 * 9-16 rows and its decode steps makes the step fail with EMMAX_ERR_INVALID (no other kernel reads the 4-bit tiles: there is no fall-back).
 * MXFP6 models (decode_fp8 = 4): the same -- 16, or 8 when nine rows would split the attention; the refusals name MXFP6; the tuning switch mx4_wide
 * does not concern them (no 17-64-row form reads the 6-bit tiles). */
int emmax_model_max_decode_batch(const emmax_model* m);
int emmax_model_max_decode_batch_exact(const emmax_model* m);
/* 1: the model was created under the tuning switch mx4_wide = 1 on MXFP4 weights -- decode_kmp.hip's MXFP4 form serves it at 17-64 rows, and
 * emmax_model_max_decode_batch answers up to 64 (LLaMA-2-7B shapes: 64; 2 kv heads: still 8; an intermediate size above 11264: still 16, its
 * down projection has no 17-row route); 0: any other model (MXFP4: the limits above); -1: null.  Frozen at emmax_model_create: the planner, the
 * session checks, every prefill and emmax_slots_open ask the model, whatever the switch says later. */
int emmax_model_mxfp4_wide(const emmax_model* m);
/* the same planner on a config, before (or without) a model: negative status when the config fails the checks that do not concern the decode
 * weight format.  An MXFP4 config is accepted by emmax_model_create exactly when this answers >= 8. */
int emmax_config_max_decode_batch(const emmax_config* cfg, int exact);
int emmax_model_finalize(emmax_model* m, void* arena_dev, int64_t arena_bytes, emmax_stream stream);
/* bf16 models: decode batches >= 3 stream the LLM projections from MFMA-fragment-major copies that a model serving batches 1-2
 * never reads.  They live in a SECOND caller-owned arena, built on demand from the finalized main arena (no bound tensors
 * needed): 13.2 GB at 7B (main arena 15.1 GB; with the tuning switch km = 0 at build time decode_mfma.hip's qkv / gate-up pair is
 * added, +9 GB).  Until it is built, emmax_prefill / emmax_slots_open with B >= 3 return EMMAX_ERR_STATE.  fp8 models keep every
 * e4m3 copy in the main arena, MXFP4 / MXFP6 models their 4-bit / 6-bit copy (N K 6 / 8 bytes of tiles + N K / 32 of scales per projection):
 * aux_bytes is 0 and build_aux a no-op. */
int64_t emmax_model_aux_bytes(const emmax_model* m);
int emmax_model_build_aux(emmax_model* m, void* aux_arena_dev, int64_t aux_bytes, emmax_stream stream);

/* ---- session: activations workspace + paged KV cache for up to max_batch sequences of <= max_ctx tokens ------------ */
int emmax_session_bytes(const emmax_model* m, int max_batch, int max_prompt, int max_ctx,
                        int64_t* workspace_bytes, int64_t* kv_bytes);
int emmax_session_create(emmax_model* m, int max_batch, int max_prompt, int max_ctx,
                         void* workspace_dev, int64_t workspace_bytes, void* kv_dev, int64_t kv_bytes,
                         emmax_session** out);
/* ... plus `stage_rows` STAGING rows (0 .. min(max_batch, 32)) for overlapped admissions, emmax_slots_prefill_staged below: each costs per-row
 * state and its share of the paged KV region.  The plain calls above are stage_rows = 0. */
int emmax_session_bytes_ex(const emmax_model* m, int max_batch, int max_prompt, int max_ctx, int stage_rows,
                           int64_t* workspace_bytes, int64_t* kv_bytes);
int emmax_session_create_ex(emmax_model* m, int max_batch, int max_prompt, int max_ctx, int stage_rows,
                            void* workspace_dev, int64_t workspace_bytes, void* kv_dev, int64_t kv_bytes,
                            emmax_session** out);
int emmax_session_stage_rows(const emmax_session* s);
/* 1: the session was created under the tuning switch exact = 1 (fp32 activations / fp32 KV cache, see above), 0: bf16-operand path */
int emmax_session_exact(const emmax_session* s);
void emmax_session_destroy(emmax_session* s);

/* frames_u8_dev: uint8 [B,224,224,3] RGB (normalisation fused into the patch gather);  out: bf16 [B,256,hidden].
 * EXACT-NUMERICS sessions exchange patch embeddings as FP32 rows: `patch_embeds_out_dev` here and every `patch_embeds*` argument of the
 * prefill / slot entry points below then hold float [B,256,hidden] (bf16 rows would put 2^-9 back into the input of the fp32 arithmetic). */
int emmax_vision_encode(emmax_session* s, const uint8_t* frames_u8_dev, int B, void* patch_embeds_out_dev,
                        emmax_stream stream);
/* pixel_values_dev: bf16 [B,6,224,224] as PrismaticProcessor emits (already normalised per tower). */
int emmax_vision_encode_pixels(emmax_session* s, const void* pixel_values_bf16_dev, int B, void* patch_embeds_out_dev,
                               emmax_stream stream);
/* raw concatenated tower features bf16 [B,256,D0+D1] of the last emmax_vision_encode* call (parity tests). */
int emmax_vision_features(emmax_session* s, int B, void* feats_out_dev, emmax_stream stream);

/* ids_dev: int32 [B,P_max] (row b uses the first lens_host[b] ids, ids[b][0] = BOS); patch_embeds: bf16 [B,256,hidden].
 * Builds [BOS]+patches+text[1:] per row (no padding: rows are packed), runs the decoder stack, fills the KV cache and
 * leaves the greedy first token of every row as the session's "current token". */
int emmax_prefill(emmax_session* s, const int32_t* ids_dev, const int32_t* lens_host, int B, int P_max,
                  const void* patch_embeds_dev, emmax_stream stream);
/* Language-only prefill (no image): the `pixel_values is None` branch of forward (modeling_prismatic.py:343-359). */
int emmax_prefill_text(emmax_session* s, const int32_t* ids_dev, const int32_t* lens_host, int B, int P_max, emmax_stream stream);
/* f32 logits of every prefill position, packed rows [sum_b S_b, vocab] (S_b = 256 + lens[b]); valid after prefill. */
int emmax_prefill_logits(emmax_session* s, float* logits_out_dev, emmax_stream stream);
/* Teacher-forced scoring of the same rows WITHOUT their logits (still ABI 12: new symbols only): what `forward(labels=...)` needs of
 * `logits` -- replaces log_softmax / gather / argmax over the [rows, vocab] buffer (HF LlamaForCausalLM.forward's loss,
 * prismatic/training/strategies/base_strategy.py:392-416).  targets_dev int32 [total_rows], packed as the pass packed its rows: the id whose logit
 * row r is scored against (the caller applies HF's shift); -100, or anything outside [0, vocab), scores nothing and yields target_logit 0.0f.
 * Outputs, packed [total_rows]: lse = log sum_c exp(logit[r, c]), target_logit = logit[r, target[r]], argmax (the lowest id wins a tie, as torch).
 * A token's log-probability is target_logit - lse.  Valid wherever emmax_prefill_logits is (after emmax_prefill, emmax_prefill_text, emmax_extend,
 * emmax_slot_extend); runs the same final norm, uses the session's split-K scratch and changes nothing a later step or emmax_prefill_logits reads.
 * EMMAX_ERR_STATE before a prefill and in an exact-numerics session (the scoring kernel has no two-term form).  Models with fp8 / MXFP4 decode
 * weights score on the bf16 lm-head their own prefill multiplies by (MXFP4: the de-quantised copy). */
int emmax_prefill_score(emmax_session* s, const int32_t* targets_dev, float* lse_out_dev, float* target_logit_out_dev, int32_t* argmax_out_dev,
                        emmax_stream stream);
/* f32 last-position logits [B,vocab] of the most recent prefill/decode step (parity tests; costs one extra pass). */
int emmax_last_logits(emmax_session* s, float* logits_out_dev, emmax_stream stream);

/* One greedy step for all rows: consumes each row's current token, appends KV, leaves argmax as the new current token
 * and records it in the session's output buffer.  Rows that already emitted EOS (or ran out of context) emit pad_id.
 * Reads all step-varying state from device memory, so it is hipGraph-capturable. */
int emmax_decode_step(emmax_session* s, emmax_stream stream);
/* Overwrite the current token of every row with a CALLER-supplied one: tokens_dev int32 [B] (teacher-forced scoring, external
 * sampling loops, the HF cached step `forward(input_ids[B,1], past_key_values)`).  The rows decode again whatever the engine's
 * own greedy prediction was: done flags, stop-rule state and token budgets are cleared.  EMMAX_ERR_NOMEM when a row's context
 * is full (the next append would leave the KV pages), EMMAX_ERR_STATE while request slots are open. */
int emmax_set_current_tokens(emmax_session* s, const int32_t* tokens_dev, emmax_stream stream);
/* Run up to max_new_tokens steps (including the token produced by prefill) -- eager launch-ahead by default, replays of a
 * captured hipGraph of emmax_decode_step with the tuning switch graph = 1; no host synchronisation per token; stops early once
 * all rows are done if stop_on_eos != 0.
 * out_ids_dev int32 [B,max_new_tokens] (pad_id after a row's EOS), out_lens_dev int32 [B] (tokens incl. EOS). */
int emmax_generate(emmax_session* s, int max_new_tokens, int stop_on_eos, int32_t* out_ids_dev, int32_t* out_lens_dev,
                   emmax_stream stream);

/* 1 when emmax_generate is replaying a captured hipGraph of the step (0: eager launches). */
int emmax_session_graph_active(emmax_session* s);
/* Measurement hook (bench.py `roofline`): launch decode stage `stage` (0 qkv GEMV, 1 paged attention, 2 o-proj GEMV,
 * 3 gate/up GEMV, 4 down GEMV: once per layer; 5 lm-head GEMV+argmax) `reps` sweeps on `stream`, bracketed by HIP
 * events on that stream; returns the mean duration of one launch in microseconds.  Needs a prefilled session; the
 * residual stream it leaves behind is garbage (run a new prefill afterwards). */
int emmax_profile_decode_stage(emmax_session* s, int stage, int reps, float* avg_us_out, emmax_stream stream);

/* ---- early exit + slot serving (continuous batching) -------------------------------------------------
 * The reference always decodes to EOS / max_new_tokens (prismatic.py:655-664, generate(max_new_tokens=512)) although the
 * Solver only reads the line after "POLICIES:" (policy_parser: extract_action_policies).  These entry points let a serving
 * loop stop a row as soon as its action line is complete and refill the freed row while the others keep decoding. */
/* Device-side stop rule of every later decode step: a row is done once it has emitted the id sequence trigger_ids[0..n)
 * followed by n_after more tokens (the emitted prefix is exactly the prefix of the full greedy generation).  n_trigger = 0
 * clears the rule; at most 16 ids; a mismatch restarts the match at the current token (no overlapping-prefix handling). */
int emmax_session_set_stop(emmax_session* s, const int32_t* trigger_ids_host, int n_trigger, int n_after, emmax_stream stream);
/* Turn the first n_slots rows of the session into independent, idle request slots (n_slots <= max_batch, <= emmax_model_max_decode_batch). */
int emmax_slots_open(emmax_session* s, int n_slots, emmax_stream stream);
/* Prefill ONE request into `slot` without disturbing the other slots: prompt ids (device int32[len]), its
 * [n_patches, hidden] bf16 patch embeddings (device; NULL = language-only) and its token budget.  The first generated
 * token is in place afterwards. */
int emmax_slot_prefill(emmax_session* s, int slot, const int32_t* ids_dev, int len, const void* patch_embeds_dev, int max_new,
                       emmax_stream stream);
/* Prefill n requests into the CONSECUTIVE slots slot0 .. slot0 + n - 1 in one packed pass (what a scheduler does when several
 * slots are free at once: eight one-row prefills cost ~1.6x one eight-row prefill): ids_dev int32 [n][P_max] (row i: lens_host[i]
 * ids, the rest ignored), patch_embeds_dev [n][n_patches, hidden] bf16 (NULL = language-only), max_new_host[i] the token budgets.
 * The other slots are not disturbed; every row's first generated token is in place afterwards. */
int emmax_slots_prefill(emmax_session* s, int slot0, int n, const int32_t* ids_dev, int P_max, const int32_t* lens_host,
                        const void* patch_embeds_dev, const int32_t* max_new_host, emmax_stream stream);
/* Overlapped admission.  emmax_slot_prefill and emmax_slots_prefill run on the stream the slots decode on: while a request is prefilled (16 ms for one
 * 7B row, 70 ms for eight) the other slots stand still.  The staged pair removes that stall: a session created with
 * emmax_session_create_ex holds `stage_rows` STAGING rows beside its decode rows (per-row state, output row, KV pages).
 *   emmax_slots_prefill_staged  prefills n requests into the staging rows on `stream`, which must be a stream of its own (not the
 *                               default stream, not the one the decode steps run on): the call touches nothing a decode step reads,
 *                               so decode steps may run beside it.  Arguments as emmax_slots_prefill without slot0.
 *   emmax_slots_commit          moves staged request staged_idx_host[i] (0 .. n_staged-1 of the last staged batch) into slot
 *                               slots_host[i] (idle, released) on the DECODE stream, between two steps: per-row state and the output
 *                               row are copied and the page-table rows swapped -- no K/V moves.  A staged batch may be committed
 *                               piecemeal, as slots free up.  The caller orders it after the staged prefill (event), and orders the
 *                               NEXT staged prefill after the last commit of the batch.
 * One staged batch at a time.  Host scheduler: emmax/serving.py (SlotScheduler, overlap=True). */
int emmax_slots_prefill_staged(emmax_session* s, int n, const int32_t* ids_dev, int P_max, const int32_t* lens_host,
                               const void* patch_embeds_dev, const int32_t* max_new_host, emmax_stream stream);
int emmax_slots_commit(emmax_session* s, const int32_t* staged_idx_host, const int32_t* slots_host, int n, emmax_stream stream);
/* n_steps greedy decode steps over all slots (no host synchronisation); idle / finished slots stay put. */
int emmax_slots_step(emmax_session* s, int n_steps, emmax_stream stream);
/* Copy the per-slot done flags and generated-token counts to device buffers int32[n_slots] (asynchronous on `stream`). */
int emmax_slots_state(emmax_session* s, int32_t* done_dev, int32_t* n_out_dev, emmax_stream stream);
/* Copy the first n generated ids of `slot` to a device buffer. */
int emmax_slot_output(emmax_session* s, int slot, int32_t* ids_dev, int n, emmax_stream stream);
/* Mark `slot` idle again (empty context: its share of a batched step then reads no K/V). */
int emmax_slot_release(emmax_session* s, int slot, emmax_stream stream);

/* ---- extending a cached context (still ABI 12: new symbols only) -------------------------------------------------------
 * A prefill starts a row at position 0 and a decode step appends one token.  These calls append MANY tokens to what a row has cached -- a follow-up
 * turn, a teacher-forced continuation, the second chunk of a long prompt -- at the price of one pass over the new rows alone: the prefill's
 * pipeline on the packed new rows, whose attention reads the cached prefix and the new rows from the paged cache (bf16 or fp8).
 *   emmax_extend           rows row0 .. row0 + B - 1 of the live batch (after a prefill and any number of steps) each get lens_host[b] >= 1 ids
 *                          appended at their cached length: ids_dev int32 [B][P_max] (row b: lens_host[b] ids).  A row's pending token -- picked,
 *                          not yet cached -- is discarded: a caller who wants it passes it as the first id.  Afterwards the rows are as a prefill
 *                          leaves them: first token of the continuation picked (greedy, or the session's sampling / warpers / token rules /
 *                          automaton: a row keeps its automaton state, a row outside the automaton -- state -1 -- enters at its start state), context += lens, done / n_out / stop match / token budget reset,
 *                          output row empty; emmax_prefill_logits returns the logits of the new rows [sum_b lens[b], vocab].  max_new (>= 0): the
 *                          tokens the caller will generate next, for the capacity check only.  The rows' lengths are read back (the call
 *                          synchronises the stream and is not capturable); later steps and graph replays need nothing new.
 *   emmax_slot_extend      the same for ONE request slot whose request has finished (done, not released), between two steps on the serving
 *                          stream, with its token budget: a follow-up turn on the kept context.  The other slots are untouched.  Like
 *                          emmax_slot_prefill it runs in the session's prefill scratch, which emmax_slots_prefill_staged uses on its own stream:
 *                          no staged prefill may be in flight when it is called (wait for it, or commit it, first).
 *   emmax_session_context  the cached lengths of rows row0 .. row0 + n - 1, read back to the host (synchronises the stream).
 * EMMAX_ERR_STATE: exact-numerics sessions; beams on; sample groups on, or a slot inside a fork group; history-reading processors on (the
 * [rows][max_prompt] id history has no room for the extension); no prefill yet; a slot that still decodes or holds nothing.  EMMAX_ERR_NOMEM:
 * context + lens + max(max_new, 1) beyond max_ctx (= the row's pages); more packed rows than the prefill holds.  A refused call changes nothing.
 * The automaton (emmax_session_set_automaton) while it is set: a row inside it keeps its state across the extension; a row OUTSIDE it -- state -1:
 * one that never entered, and equally one that an earlier constrained generation left through a transition to -1 -- enters at its start state
 * again (a start state of -1 leaves it unconstrained).  A caller who wants such a row to stay outside sets its start to -1 first. */
int emmax_extend(emmax_session* s, int row0, int B, const int32_t* ids_dev, const int32_t* lens_host, int P_max, int max_new, emmax_stream stream);
int emmax_slot_extend(emmax_session* s, int slot, const int32_t* ids_dev, int len, int max_new, emmax_stream stream);
int emmax_session_context(emmax_session* s, int row0, int n, int32_t* ctx_out_host, emmax_stream stream);

/* ---- draft-verified greedy decoding (still ABI 12: new symbols only) ----------------------------------------------------
 * A greedy generation in flight checks a GUESSED continuation in one pass instead of one decode step per token.  Row b's window is ids_dev[b][0 ..
 * lens_host[b]): id 0 is the row's pending token (picked, not yet cached: checked against the device, EMMAX_ERR_INVALID on a mismatch), ids 1 .. the guess.
 *   emmax_verify           rows row0 .. row0 + B - 1 of the live batch: the extension pass of emmax_extend over the windows, the argmax of every window
 *                          row (the scoring launch of emmax_prefill_score, no logits stored), then the accept walk on the device: the token behind
 *                          window row i is emitted -- ctx_len + 1, output row, n_out, EOS / token budget / stop rule / cache end, pending token: exactly a
 *                          decode step's bookkeeping -- and row i + 1 is reached only while the row is not done and that token equals the window's
 *                          id i + 1.  The rows emit 1 .. lens[b] tokens (emitted_host[b]; new_ids_host [B][P_max]: those tokens, pad behind them;
 *                          done_host[b]: the row's done flag afterwards) and are then as that many decode steps would have left them; K / V rows the
 *                          pass wrote beyond a row's new cached length are dead (nothing reads past it, later appends overwrite them).  max_new
 *                          (1 .. max_out) becomes the rows' token budget, as emmax_generate sets it.  A row that is already done takes part with any
 *                          window (its pending token alone will do; its first id is not checked) and is left exactly as it is, emitted 0.
 *                          emmax_prefill_logits returns the window rows' logits afterwards.  The call reads the rows' state back before and its
 *                          results after the pass: it synchronises the stream and is not capturable; decode steps and graph replays go on behind it.
 *   emmax_session_set_budget  the token budget of rows row0 .. row0 + B - 1 (what emmax_generate sets before its loop) for a host loop of emmax_decode_step.
 *   emmax_session_output   out_ids[b][first .. first + n) of those rows into ids_host [B][n], their n_out and done flags (either may be NULL), read
 *                          back to the host (synchronises the stream).
 * EMMAX_ERR_STATE, each with its own message: everything emmax_extend refuses; open request slots; sampling, logits processing, warpers, token rules,
 * a token automaton, bound scores, top / watched log-probabilities or step taps (the accepted ids are argmaxes of raw rows); a model with fp8 decode
 * weights (its prefill multiplies by the unquantised matrices: the pass would verify another model).  bf16, MXFP4 and MXFP6 weights, bf16 and fp8 KV caches
 * are served.  EMMAX_ERR_NOMEM: context + lens + 1 (a done row: context + lens) beyond max_ctx or the row's pages; more packed rows than the prefill
 * holds.  A refused call changes nothing: the caller falls back to plain decode steps.
 *   emmax_op_verify_accept the accept walk alone on caller-owned device arrays: argmax_dev [cu[B]] packed as cu_dev [B + 1] says, ids_dev [B][P_max],
 *                          the per-row state arrays [B] and out_ids_dev [B][max_out], stop_ids_dev [16] / stop_cfg_dev {n_trigger, n_after} as
 *                          emmax_session_set_stop uploads them; emitted_dev [B], new_ids_dev [cu[B]] (packed like argmax; may be NULL). */
int emmax_verify(emmax_session* s, int row0, int B, const int32_t* ids_dev, const int32_t* lens_host, int P_max, int max_new, int32_t* emitted_host,
                 int32_t* new_ids_host, int32_t* done_host, emmax_stream stream);
int emmax_session_set_budget(emmax_session* s, int row0, int B, int max_new, emmax_stream stream);
int emmax_session_output(emmax_session* s, int row0, int B, int first, int n, int32_t* ids_host, int32_t* n_out_host, int32_t* done_host, emmax_stream stream);
int emmax_op_verify_accept(const int32_t* argmax_dev, const int32_t* ids_dev, int P_max, const int32_t* cu_dev, int B, int32_t* cur_tok_dev, int32_t* ctx_len_dev,
                           int32_t* done_dev, int32_t* n_out_dev, const int32_t* max_new_dev, int32_t* stop_m_dev, int32_t* stop_after_dev, int32_t* out_ids_dev,
                           int max_out, const int32_t* stop_ids_dev, const int32_t* stop_cfg_dev, int eos_id, int pad_id, int max_ctx, int32_t* emitted_dev,
                           int32_t* new_ids_dev, emmax_stream stream);

/* ---- seeded sampling over rows of logits (ABI 6) --------------------------------------------------------------------
 * emmax_op_sample draws one token per row of logits_dev [B][ld] (fp32, V <= 32768 entries, ld >= V) and returns it with its
 * log-probability.  Per-row parameters and steps are device arrays of B entries.  Since ABI 7 the decode step draws the same way itself
 * (emmax_session_set_sampling below); an external loop samples the rows of emmax_last_logits and feeds the tokens back with
 * emmax_set_current_tokens (emmax/sampling.py: sample_logits).
 *   temperature 0     greedy: the argmax, lowest id on ties (top_k / top_p ignored);
 *   temperature T > 0 z = l / T (fp32); top_k > 0 keeps z_i >= the k-th largest z (ties kept); top_p < 1 then keeps, over those, the i with
 *                     sum_{kept j, z_j > z_i} W_j < top_p * sum_{kept j} W_j, W_j = floor(exp(z_j - max z) 2^32) as 64-bit integers
 *                     (the argmax always stays); token = argmax over the kept i of z_i + g_i (Gumbel-max: an exact draw from softmax(z)
 *                     renormalised over the kept set), lowest id on ties;
 *   noise             g_i = -log(-log u_i), u_i = ((x >> 8) + 0.5) 2^-24, x = word i % 4 of Philox4x32-10 with key (seed low, seed high
 *                     32 bits) and counter (i / 4, step, subseq, 0).  Nothing else enters: not the row's place in the batch or B;
 *   log-probability   l_tok - logsumexp(l) over the raw logits (T = 1, unfiltered): HF compute_transition_scores(normalize_logits=True).
 * Every reduction has a fixed order and only integer atomics are used: the same inputs give the same bits.  An all-NaN row gives
 * token -1.  EMMAX_ERR_INVALID for a null pointer, B < 1, V outside 1..32768 or ld < V.  The values of the parameter arrays are the
 * caller's to check (emmax/sampling.py: SamplingParams): temperature finite and >= 0, 0 <= top_k, 0 < top_p <= 1. */
int emmax_op_sample(const float* logits_dev, int ld, int B, int V, const float* temperature_dev, const int32_t* top_k_dev, const float* top_p_dev,
                    const uint64_t* seed_dev, const uint32_t* subseq_dev, const int32_t* step_dev, int32_t* tok_out_dev, float* logprob_out_dev,
                    emmax_stream stream);

/* ---- sampling inside the decode step (ABI 7) ------------------------------------------------------------------------
 * A session samples once emmax_session_set_sampling (or emmax_slots_set_sampling_staged) has run: from then on every lm-head that emits a
 * token -- prefills (emmax_prefill*, emmax_slot_prefill, emmax_slots_prefill*), decode steps eager and replayed, emmax_generate,
 * emmax_slots_step -- also writes the fp32 logits of its rows to the session's own logit rows, and the step's finish draws each row's token
 * from them exactly as emmax_op_sample does (the same token and log-probability bits) with step = the row's generation index (0 for the
 * token a prefill emits) and the row's (temperature, top_k, top_p, seed, subseq).  A sampled step has the launch count of a greedy one;
 * the captured step graph is keyed on sampling on / off, and changed parameters re-capture nothing (they are device words).  Rows at
 * temperature 0 take the argmax of those fp32 logits: the greedy token.  A row whose logits are all NaN emits pad_id and is done.
 * Parameters are per row and stay until set again; a row's parameters must be set before the prefill whose first token they govern.
 * emmax_session_clear_sampling turns sampling off: the session launches exactly what a session that never sampled launches.
 *   emmax_session_set_sampling       decode rows row0 .. row0 + n - 1 (slots when request slots are open); host arrays of n values, checked
 *                                    here: temperature finite and >= 0, top_k >= 0 (0 = off), 0 < top_p <= 1 -- else EMMAX_ERR_INVALID.
 *                                    Synchronises the stream (the values pass through pinned memory).  Turns sampling on.
 *   emmax_slots_set_sampling_staged  the same for the n requests of the next emmax_slots_prefill_staged (call it on that prefill's stream);
 *                                    emmax_slots_commit moves a request's parameters and log-probabilities with the rest of its state.
 *   emmax_session_sampling           1 = sampling on, 0 = off, -1 = null session.
 *   emmax_session_logprobs           after emmax_generate: out_dev fp32 [B][max_new], the log-probability of every emitted token
 *                                    (l_tok - logsumexp(l) over the raw logits, T = 1, unfiltered: emmax_op_sample's); entries past a
 *                                    row's length are 0.  emmax_slot_logprobs: the first n of one slot (as emmax_slot_output).
 *                                    Both EMMAX_ERR_STATE while sampling is off. */
int emmax_session_set_sampling(emmax_session* s, int row0, int n, const float* temperature_host, const int32_t* top_k_host, const float* top_p_host,
                               const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream);
int emmax_slots_set_sampling_staged(emmax_session* s, int n, const float* temperature_host, const int32_t* top_k_host, const float* top_p_host,
                                    const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream);
int emmax_session_clear_sampling(emmax_session* s, emmax_stream stream);
int emmax_session_sampling(const emmax_session* s);
int emmax_session_logprobs(emmax_session* s, int max_new, float* out_dev, emmax_stream stream);
int emmax_slot_logprobs(emmax_session* s, int slot, float* out_dev, int n, emmax_stream stream);

/* ---- logits processors and scores inside the decode step (ABI 8) ----------------------------------------------------
 * The semantics of transformers 5.15's processors (generation/utils.py: _get_logits_processor), applied in HF's order before the warpers
 * and the draw of ABI 7.  Per row, the history H is the row's prompt ids (the text ids its prefill got, BOS included; the patch rows carry
 * no ids) followed by the ids the row has emitted (out_ids[0 .. n_out)):
 *   repetition penalty p   every distinct id of H: x < 0 ? x * p : x / p (fp32, p as fp32), once per id.  p = 1: off.
 *   no_repeat_ngram_size n every id that would complete an n-gram already in H is -inf.  n = 0: off; n <= EMMAX_MAX_NGRAM (32).
 *   min_new_tokens m       the EOS logit (eos_id) is -inf while n_out < m.  (HF min_length L is m = max(min_new_tokens, L - P_max), P_max
 *                          the longest prompt of the call: the Python layer folds it.)
 * Then temperature / top_k / top_p and the draw as in ABI 7 (sampling on), else the argmax of the processed row.  Log-probabilities keep
 * their ABI 7 meaning: l_tok - logsumexp(l) over the RAW logits.  A row with no finite entry left emits pad_id and is done.  Known
 * differences from HF: H is each row's own, unpadded; the patch rows are not in it (HF's input_ids for this model hold none either).
 * A session processes once emmax_session_set_processing (or emmax_slots_set_processing_staged) has run, and keeps scores once
 * emmax_session_set_scores bound a buffer.  Either way every lm-head that emits a token writes the rows' fp32 logits and the step ends in
 * the processing finish (same launch count); the captured step graph is keyed on greedy / sampled / processing, and changed parameters or
 * score buffers re-capture nothing (they are device words).  With processing and scores off the session launches exactly what it launched
 * before.  Every prefill (emmax_prefill*, emmax_slot_prefill, emmax_slots_prefill*) keeps its rows' prompt ids while processing is on:
 * set processing before the prefill whose tokens it governs.
 *   emmax_session_set_processing       rows row0 .. row0 + n - 1 (slots when request slots are open); host arrays of n values, checked here:
 *                                      penalty finite and > 0, 0 <= ngram <= 32, min_new >= 0 -- else EMMAX_ERR_INVALID.  Synchronises the
 *                                      stream.  Turns processing on.
 *   emmax_slots_set_processing_staged  the same for the n requests of the next emmax_slots_prefill_staged; emmax_slots_commit moves a
 *                                      request's parameters and prompt ids with the rest of its state.
 *   emmax_session_clear_processing     processing off.  emmax_session_processing: 1 on, 0 off, -1 null session.
 *   emmax_session_set_scores           binds fp32 [max_new][B][vocab] buffers for the next generation (B = the rows of the next prefill; bind
 *                                      before it: the prefill emits token 0; a later prefill of another batch size unbinds them).  scores[t][b] = HF's `scores`: the processed row of a greedy
 *                                      row; z / T on the kept set and -inf elsewhere for a sampled one.  logits[t][b] = the raw lm-head row.
 *                                      t = the row's generation index; entries of tokens not emitted are not written.  Either may be NULL;
 *                                      both NULL unbinds.  EMMAX_ERR_STATE while request slots are open; emmax_slots_open unbinds.
 * While processing is on, emmax_set_current_tokens returns EMMAX_ERR_STATE (forced tokens would be missing from H). */
int emmax_session_set_processing(emmax_session* s, int row0, int n, const float* penalty_host, const int32_t* ngram_host, const int32_t* min_new_host,
                                 emmax_stream stream);
int emmax_slots_set_processing_staged(emmax_session* s, int n, const float* penalty_host, const int32_t* ngram_host, const int32_t* min_new_host,
                                      emmax_stream stream);
int emmax_session_clear_processing(emmax_session* s, emmax_stream stream);
int emmax_session_processing(const emmax_session* s);
int emmax_session_set_scores(emmax_session* s, float* scores_dev, float* logits_dev, int max_new, emmax_stream stream);

/* ---- the further warpers and the token rules inside the decode step (new symbols, same ABI) --------------------------------------------
 * The rest of that family of transformers 5.15 (generation/logits_process.py; order of _get_logits_processor), per row.  They run in the
 * EXT form of the processing finish: its own instantiation of the kernel, launched only while warpers or token rules are set -- a
 * session that sets neither launches exactly what it launched before.  Same launch count; the step graph is keyed on the two being on or
 * off; values, the rule table and the enable words are device words behind stable pointers: changing them re-captures nothing.
 *
 * WARPERS, after temperature, top_k and top_p, in this order, on sampled rows (temperature 0 ignores them as it ignores top_k / top_p).
 * K = the set kept so far, W_i = floor(exp(z_i - max z) 2^32) the integer masses of ABI 6 (max z = the processed row's maximum over T:
 * W = 2^32 there), S = sum_{i in K} W_i as a 64-bit integer, recomputed before each warper.  -inf and NaN entries are never in K.
 *   min_p m in (0, 1]      keep i iff W_i >= floor(fp32(m) 2^32) (an integer comparison; the maxima always stay).  0 = off.
 *   typical_p t in (0, 1)  lnZ = logf(fp32(S) 2^-32), lp_i = (z_i - max z) - lnZ, p_i = fp32(W_i) * (1 / fp32(S)), all fp32;
 *                          H = -sum_{i in K} p_i lp_i, one fp32 reduction in the order of the row's log-sum-exp (a lane's entries in register
 *                          order with separately rounded products and sums, xor butterfly 32..1, the 16 waves in order);
 *                          d_i = |(-lp_i) - H| (fp32).  Keep i iff sum_{j in K, d_j < d_i} W_j < fp64(fp32(t)) fp64(S) (one rounding), or that
 *                          sum is 0: the shortest prefix in ascending d whose mass reaches t S, ties kept -- one more radix walk, over the
 *                          order-preserving key of d.  As in HF the row's maximum may go.  0 or 1 = off.
 *   epsilon_cutoff e in (0, 1)  keep i iff fp64(W_i) >= fp64(fp32(e)) fp64(S) (one rounding), or z_i = the largest kept z.  0 = off.
 *   eta_cutoff e in (0, 1)      the same with e' = fminf(e, sqrtf(e) * expf(-H)) (fp32, H as above over the set kept so far).  0 = off.
 * scores[t][b] keeps its meaning (z on the final kept set, -inf elsewhere), log-probabilities theirs (raw logits, T = 1, unfiltered).  No
 * float atomics; the same inputs give the same bits; the kept set does not depend on the row's place in the batch or on B.
 *
 * TOKEN RULES, processors on the row's history H (ABI 8's: prompt ids, then emitted ids; L ids).  One table per session: n rules, rule r =
 * ids[off[r] .. off[r + 1]) = (s_1 .. s_m), flags[r] (bits 0-1 the kind: 0 sequence_bias, 1 bad_words_ids, 2 suppress_tokens, 3
 * begin_suppress_tokens; bit 2: the rule fires for the first generated token only, n_out == 0), bias[r] (kind 0).  Caps: 512 rules
 * (EMMAX_MAX_RULES), 16 ids per rule, 8192 ids in all.  A rule applies to a row iff bit `kind` of the row's enable word is set.  It FIRES
 * iff m == 1, or m <= L (HF skips a sequence longer than the context) and H ends with s_1 .. s_{m-1}; its target is s_m (ignored when >= V).
 *   kind 0   first of all processors: x[s_m] += B, B = the fp32 sum, from 0 in rule order, of the biases of the fired rules with that target
 *            (HF builds the bias row, then adds it once; list 1-id rules first to reproduce HF's bits).
 *   kinds 1-3  x[s_m] = -inf, with the n-gram ban (after the repetition penalty).
 * A row with no finite entry left emits pad_id and is done.  The rules need the history: setting a table turns processing on with neutral
 * values (penalty 1, ngram 0, min_new 0) where it was off, and clearing the table turns that off again.
 *   emmax_session_set_warpers            rows row0 .. row0 + n - 1, host arrays of n values (0 = off), checked here: 0 <= min_p <= 1,
 *                                        0 <= typical_p <= 1, 0 <= epsilon_cutoff < 1, 0 <= eta_cutoff < 1 -- else EMMAX_ERR_INVALID and nothing
 *                                        changes.  Turns the warpers on.  emmax_session_set_sampling leaves them as they were;
 *                                        emmax_session_clear_sampling and emmax_session_clear_warpers zero every row's and turn them off.
 *   emmax_slots_set_warpers_staged       the same for the n requests of the next emmax_slots_prefill_staged.
 *   emmax_session_set_token_rules        the table (host arrays), checked here: counts within the caps, offsets rising from 0, ids >= 0, flags
 *                                        0..7, no NaN bias -- else EMMAX_ERR_INVALID and nothing changes.  Synchronises the stream.  The first
 *                                        table enables every kind on every row.  emmax_session_set_processing leaves table and words alone;
 *                                        emmax_session_clear_processing and emmax_session_clear_token_rules turn the rules off.
 *   emmax_session_set_rule_enables       rows row0 .. row0 + n - 1: enable words 0..15.  EMMAX_ERR_STATE before a table is set.
 *   emmax_slots_set_rule_enables_staged  the same for the n requests of the next emmax_slots_prefill_staged.
 *   emmax_slots_commit / emmax_slots_fork move a request's warper values and enable word with the rest of its state (a fork's followers
 *                                        take the source's).
 *   emmax_session_warpers / emmax_session_token_rules   1 on, 0 off, -1 null session.
 * Beams: the setters return EMMAX_ERR_STATE while beams are on, and emmax_session_set_beams while either is on.
 *
 * emmax_op_sample_ext is that finish on its own: emmax_op_sample's rows and sampling arrays (n_out_dev = the Philox step = the generation
 * index the rules and min_new see), the four warper arrays (all or none; NULL = off), the processor arrays of ABI 8 with the rows' complete
 * histories hist_dev [B][max_hist] + hist_len_dev (all or none), a rule table in device memory (n_rules = 0: none; needs the histories) with
 * the rows' enable words.  Out: the token (pad_id for a row with no finite entry left after processing, -1 for an all-NaN row without
 * processing), the log-probability of ABI 6 and, when scores_out_dev is not NULL, the row's HF scores [B][V].  Array values are the caller's to
 * check. */
int emmax_session_set_warpers(emmax_session* s, int row0, int n, const float* min_p_host, const float* typical_p_host, const float* epsilon_cutoff_host,
                              const float* eta_cutoff_host, emmax_stream stream);
int emmax_slots_set_warpers_staged(emmax_session* s, int n, const float* min_p_host, const float* typical_p_host, const float* epsilon_cutoff_host,
                                   const float* eta_cutoff_host, emmax_stream stream);
int emmax_session_clear_warpers(emmax_session* s, emmax_stream stream);
int emmax_session_warpers(const emmax_session* s);
int emmax_session_set_token_rules(emmax_session* s, int n_rules, const int32_t* offsets_host, const int32_t* ids_host, const int32_t* flags_host,
                                  const float* bias_host, emmax_stream stream);
int emmax_session_set_rule_enables(emmax_session* s, int row0, int n, const uint32_t* enable_host, emmax_stream stream);
int emmax_slots_set_rule_enables_staged(emmax_session* s, int n, const uint32_t* enable_host, emmax_stream stream);
int emmax_session_clear_token_rules(emmax_session* s, emmax_stream stream);
int emmax_session_token_rules(const emmax_session* s);
int emmax_op_sample_ext(const float* logits_dev, int ld, int B, int V, const float* temperature_dev, const int32_t* top_k_dev, const float* top_p_dev,
                        const uint64_t* seed_dev, const uint32_t* subseq_dev, const int32_t* n_out_dev, const float* min_p_dev, const float* typical_p_dev,
                        const float* epsilon_cutoff_dev, const float* eta_cutoff_dev, const float* penalty_dev, const int32_t* ngram_dev,
                        const int32_t* min_new_dev, const int32_t* hist_dev, const int32_t* hist_len_dev, int max_hist, int n_rules,
                        const int32_t* rule_off_dev, const int32_t* rule_ids_dev, const int32_t* rule_flags_dev, const float* rule_bias_dev,
                        const uint32_t* rule_enable_dev, int eos_id, int pad_id, int32_t* tok_out_dev, float* logprob_out_dev, float* scores_out_dev,
                        emmax_stream stream);

/* ---- constrained decoding: a token automaton in the decode step (new symbols, same ABI) ---------------------------------
 * HF's prefix_allowed_tokens_fn (PrefixConstrainedLogitsProcessor) as a compiled automaton over TOKEN CLASSES, so that it runs inside a
 * captured step.  One automaton per session, device words behind stable pointers (another table re-captures nothing):
 *   cls[V]       uint8   the class of every token id; C classes, C <= 256 (EMMAX_MAX_AUT_CLASSES)
 *   allow[S][8]  uint32  bit c of allow[s] (word c / 32, bit c % 32): class c is allowed in state s; S states, S <= 1024 (EMMAX_MAX_AUT_STATES)
 *   next[S][C]   int16   the state after a token of class c in state s; -1: the row is DONE AFTER THIS TOKEN, whatever the token is
 * and per row (decode rows and staging rows) start[b] (int32, -1: the row is unconstrained for its whole life) and state[b], which every
 * prefill that restarts the row sets to start[b] -- where the stop rule's matcher is reset.
 * A row that emits a token in state s >= 0: every id i whose bit cls[i] of allow[s] is clear becomes -inf together with the other bans
 * (after the sequence biases and the repetition penalty; every later processor only bans, so their order does not matter: HF's result).  The
 * warpers and the draw, or the argmax, are unchanged.  Then state[b] = next[s][cls[tok]] for the token emitted; -1 marks the row done as an
 * EOS does (and stays in state[b]).  A row that was done, is idle or is out of budget does not move.  A state that allows nothing leaves no
 * finite entry: the row emits pad_id and is done (its state stays).  EOS is a token like any other: the automaton says where it may appear.
 * Log-probabilities and top-N / watched log-probabilities are of the RAW row; scores[t][b] is the processed row (-inf at the disallowed
 * ids); logits[t][b] is raw.  No float atomics; the same inputs give the same bits; the kept set and the token do not depend on the row's
 * place in the batch or on B.  The mask is a processor on whole fp32 logit rows: setting an automaton turns processing on with neutral
 * values where it was off, and clearing it turns that off again.  A session without an automaton launches what it launched before: the
 * constrained finish is an instantiation of its own (finish mode bit 16).
 *   emmax_session_set_automaton              the tables (host arrays: cls[V], allow[S][8], next[S][C]), checked here: 1 <= S <= 1024,
 *                                            1 <= C <= 256, every cls < C, every next in [-1, S) -- else EMMAX_ERR_INVALID and nothing
 *                                            changes.  Synchronises the stream.  The first table leaves every row at start = -1; a later
 *                                            one keeps the rows' starts (a state the new table does not have allows nothing).
 *   emmax_session_set_automaton_starts       rows row0 .. row0 + n - 1: start states in [-1, S).  EMMAX_ERR_STATE before a table is set.  Set
 *                                            them before the prefill whose first token they govern.
 *   emmax_slots_set_automaton_starts_staged  the same for the n requests of the next emmax_slots_prefill_staged.
 *   emmax_session_clear_automaton            off (emmax_session_clear_processing turns it off too).
 *   emmax_session_automaton                  1 on, 0 off, -1 null session.
 *   emmax_session_automaton_state            rows row0 .. row0 + n - 1 of state[] (staging rows behind the decode rows) to a device array.
 *   emmax_slots_commit / emmax_slots_fork    move start and state with the rest of a request's state; a fork's followers enter at the
 *                                            source's start, as if the prompt had been prefilled for each of them alone.
 *   emmax_set_current_tokens                 stays EMMAX_ERR_STATE (processing is on).
 * Beams: the setter returns EMMAX_ERR_STATE while beams are on, and emmax_session_set_beams while an automaton is set.
 *
 * emmax_op_sample_constrained is that finish on its own: the arguments of emmax_op_sample_ext (the processor arrays and histories are
 * required: the mask is a processor), the three tables in device memory (next at a pitch of n_classes) and state_dev[B] (-1: unconstrained;
 * a state outside 0 .. n_states - 1 allows nothing).  Out: token, raw log-probability, state_out_dev[B] = the state after the token (the
 * row's state where it emitted pad_id) and, when scores_out_dev is not NULL, the scores. */
int emmax_session_set_automaton(emmax_session* s, int n_states, int n_classes, const uint8_t* cls_host, const uint32_t* allow_host, const int16_t* next_host,
                                emmax_stream stream);
int emmax_session_set_automaton_starts(emmax_session* s, int row0, int n, const int32_t* start_host, emmax_stream stream);
int emmax_slots_set_automaton_starts_staged(emmax_session* s, int n, const int32_t* start_host, emmax_stream stream);
int emmax_session_clear_automaton(emmax_session* s, emmax_stream stream);
int emmax_session_automaton(const emmax_session* s);
int emmax_session_automaton_state(emmax_session* s, int row0, int n, int32_t* state_out_dev, emmax_stream stream);
int emmax_op_sample_constrained(const float* logits_dev, int ld, int B, int V, const float* temperature_dev, const int32_t* top_k_dev, const float* top_p_dev,
                                const uint64_t* seed_dev, const uint32_t* subseq_dev, const int32_t* n_out_dev, const float* min_p_dev,
                                const float* typical_p_dev, const float* epsilon_cutoff_dev, const float* eta_cutoff_dev, const float* penalty_dev,
                                const int32_t* ngram_dev, const int32_t* min_new_dev, const int32_t* hist_dev, const int32_t* hist_len_dev, int max_hist,
                                int n_rules, const int32_t* rule_off_dev, const int32_t* rule_ids_dev, const int32_t* rule_flags_dev,
                                const float* rule_bias_dev, const uint32_t* rule_enable_dev, int eos_id, int pad_id, int n_states, int n_classes,
                                const uint8_t* cls_dev, const uint32_t* allow_dev, const int16_t* next_dev, const int32_t* state_dev, int32_t* tok_out_dev,
                                float* logprob_out_dev, int32_t* state_out_dev, float* scores_out_dev, emmax_stream stream);

/* ---- beam search inside the decode step (ABI 9) ----------------------------------------------------------------------
 * The semantics of transformers 5.15's GenerationMixin._beam_search (_get_top_k_continuations, _get_running_beams_for_next_iteration,
 * _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences) for do_sample = False, one EOS id and no
 * logits processor.  A GROUP is one request (one prompt, one frame) with K = num_beams beams; a session decodes G groups as G x K rows
 * (row g K + k = running beam k of group g), G x K <= min(max_batch, emmax_model_max_decode_batch).  2 <= K <= EMMAX_MAX_BEAMS (8); K = 1
 * is not a beam run.  The arithmetic is pinned so that a host can replay it bit for bit (tests/beam_ref.py does):
 *   lse            per running row, one fp32 log-sum-exp of the raw fp32 logit row: m = max l, s = sum expf(l_i - m) in the fixed order of
 *                  the sampling kernel (entry i = 4 (g 1024 + lane) + c summed over (g, c) per lane, the 64 lanes of a wave by xor
 *                  butterfly 32 .. 1, the 16 waves in order), lse = m + logf(s).  The trace returns it: a replay takes it from there.
 *   candidates     acc = fp32(fp32(l - lse) + score), score = the row's running score: two correctly rounded fp32 operations.
 *   masks          HF's -1e9 masks are fp32 additions of -1e9f, applied in HF's order; a mask that is off adds nothing.
 *   length penalty never pow on the device: emmax_session_set_beams uploads pw[n] = fp32(pow((double)n, (double)length_penalty)) for
 *                  n = 0 .. max_ctx, and the device divides (score / pw[n], correctly rounded).
 *   top 2K         per group the best 2K of the K x V candidates (beams_to_keep = 2K), acc descending; EQUAL acc (as fp32 values) are
 *                  ordered by the lower flat index beam V + token.  (torch.topk leaves the order of equal values open.)
 *   running beams  the best K of the 2K by fp32(acc + -1e9f [the candidate stopped]), ties to the lower place in the list.  A candidate
 *                  stops when its token is eos_id (stop_on_eos) or it is the max_new-th generated token.
 *   finished set   HF's merge: the kept K followed by the 2K candidates scored fp32(acc / pw[n]) + masks (all K kept are finished and
 *                  early_stopping is True; the heuristic is no longer unsatisfied; the candidate is not a just-finished one among the TOP K),
 *                  best K, ties to the lower place in the merged list.  n = the candidate's generated length.
 *   early stop     early_stopping 0 = False, 1 = True, 2 = "never", HF's heuristic with pw[] (best running score / pw[n], or / pw[max_new]
 *                  for "never" with a positive penalty, against min kept score where finished, else -1e9f).
 *   first step     taken from the prefill's one logit row per group with running score 0.  HF's initial scores [0, -1e9, ...] select the
 *                  same candidates whenever that row has 2K entries above -inf.
 *   NaN            a NaN never compares greater: a row with a NaN logit has lse = NaN and contributes no candidate; a group with no
 *                  candidate left is done and keeps what it has.
 * Known differences from HF: lengths enter only as generated-token counts (HF left-pads a batch, these rows are packed: a group's result
 * does not depend on the other groups' prompt lengths); the trigger stop rule of emmax_session_set_stop is not applied to beams.
 *
 * THE CACHE FOLLOWS THE BEAMS ON THE PAGE TABLE.  Complete pages (64 tokens) are immutable and shared by reference; only the page a beam
 * is filling is private.  After every step beam j continues parent p(j): page-table row j takes p(j)'s entries, and where p(j) != j the
 * parent's partial page is copied (every layer, K and V, every plane of the cache format) into j's SPARE page, which then swaps with j's
 * old one -- never in place, because that old page may be another beam's source in the same step.  A page that the step completed is shared
 * instead of copied.  The prefill runs ONE row per group and forks it: K page-table rows over the prompt's complete pages, the partial
 * page copied K - 1 times.  Group g lives on the pages of rows g K .. g K + K - 1; pages of a dead lineage are not reclaimed within a run:
 * a group uses  floor(S / 64) shared prompt pages + K x (pages from floor(S / 64) to the last generated position) + K spares,  S = patches +
 * prompt ids.  Where that exceeds K x max_pages emmax_generate returns EMMAX_ERR_NOMEM before it decodes anything (emmax_prefill* checks
 * the same for max_new = 1).  emmax_session_bytes is the same for the same max_batch: the KV region does not grow.
 *
 *   emmax_session_set_beams    K = num_beams, length_penalty finite, early_stopping in {0, 1, 2}; 2 <= K <= min(8, max_batch), vocab >= 2K
 *                              and <= 32768 -- else EMMAX_ERR_INVALID.  EMMAX_ERR_STATE while request slots are open, sampling or
 *                              processing is on, or a `scores` buffer is bound (a raw `logits` buffer may stay: [max_new][G K][vocab],
 *                              row g K + k at step t = the row running beam k read at that step, before the step's reorder; the prefill's
 *                              row is written at [0][g K]).  Synchronises the stream.
 *   emmax_session_clear_beams  beams off; the page table is the identity again.  With beams off a session launches exactly what it
 *                              launched before ABI 9.  emmax_session_beams: K, 0 = off, -1 null session.
 * With beams on: emmax_prefill* takes G rows (G x K must fit); emmax_generate(max_new, ...) runs the first beam step, the fork and the
 * decode steps of G x K rows (the step graph is keyed on beams on / off and K; parents, scores and pages are device words), resolves the
 * kept hypotheses and returns them in out_ids [G K][max_new] / out_lens [G K], best first per group, pad_id behind the end; it runs once per
 * prefill.  emmax_decode_step, emmax_set_current_tokens, emmax_last_logits, the slot calls, emmax_session_set_sampling /
 * _set_processing and emmax_session_set_scores with a `scores` buffer return EMMAX_ERR_STATE.
 *   emmax_session_beam_result  after emmax_generate: seq [G K][max_new] (as out_ids), len [G K], score [G K] fp32 = HF's sequences_scores
 *                              of all K kept hypotheses, beam_indices [G K][max_new] (HF's meaning: the session row g K + parent beam each
 *                              token was continued from, -1 behind the end).  Device pointers; any may be NULL.
 *   emmax_session_beam_trace   per step t < max_new and running beam: tok, parent [max_new][G K] int32, score (the running score after
 *                              the step), lse (of the row the step read for this beam slot; step 0 read one row per group: slot k > 0
 *                              holds 0) [max_new][G K] fp32; and the step's candidate list the finished-set update consumed: cand_idx
 *                              [max_new][G 2K] int32 (flat index beam V + token, -1 = none) and cand_acc fp32.  Steps a group did not run
 *                              hold tok = parent = cand_idx = -1 and zeros.  Device pointers; any may be NULL. */
#define EMMAX_MAX_BEAMS 8
int emmax_session_set_beams(emmax_session* s, int num_beams, double length_penalty, int early_stopping, emmax_stream stream);
int emmax_session_clear_beams(emmax_session* s, emmax_stream stream);
int emmax_session_beams(const emmax_session* s);
int emmax_session_beam_result(emmax_session* s, int max_new, int32_t* seq_dev, int32_t* len_dev, float* score_dev, int32_t* beam_indices_dev,
                              emmax_stream stream);
int emmax_session_beam_trace(emmax_session* s, int max_new, int32_t* tok_dev, int32_t* parent_dev, float* score_dev, float* lse_dev,
                             int32_t* cand_idx_dev, float* cand_acc_dev, emmax_stream stream);

/* ---- sample groups: N sampled rows per prompt on the prompt's KV pages (additions to ABI 11: new symbols only) ------------
 * HF generate(do_sample = True, num_return_sequences = N).  A SAMPLE GROUP is one prompt (one frame) with N rows; a session decodes G
 * groups as G x N rows, row g N + j = sample j of prompt g (the order of HF's expand_inputs_for_generation).  2 <= N and
 * G x N <= min(max_batch, emmax_model_max_decode_batch): there is no cap of 8.  Sampling must be on (emmax_session_set_sampling): N greedy
 * rows of one prompt are identical, and a prefill with groups on and sampling off returns EMMAX_ERR_STATE (HF raises there too).
 *
 * With groups on emmax_prefill* takes G rows (G x N must fit, else EMMAX_ERR_INVALID) and does all of this before it returns:
 *   prefill      one row per group, written to the first pages of the group's pool (the pages of rows g N .. g N + N - 1).
 *   lm-head      one row per group (exact numerics: one row per launch, as with beams -- a group's first row does not depend on G); the row is
 *                then given to all N rows: the session's fp32 logit rows (what emmax_last_logits returns until the first decode step), the
 *                prompt-history rows when processing is on, and logits[0] / scores[0] of every row when buffers are bound
 *                (emmax_session_set_scores: buffers of [max_new][G N][vocab]).
 *   token 0      row g N + j draws with its own (temperature, top_k, top_p, seed, subseq) at step 0: the sampled or processing finish a
 *                G x N batch's prefill ends in, unchanged.
 *   fork         the page-table rows of the group reference the prompt's floor(S / 64) complete pages, S = patches + prompt ids; the
 *                partial page is copied N - 1 times into each row's own page at that index, in every layer and every plane of the cache
 *                format; no copy is made when S % 64 == 0.  Every later page is the row's own.
 * From then on the rows are ordinary decode rows on a non-identity page table: emmax_decode_step, emmax_generate, emmax_last_logits,
 * emmax_set_current_tokens, the log-probabilities, the scores, the stop rule and graph replay behave as for a G x N batch, and a step
 * launches the kernels a G x N sampled batch launches (but for the attention where emmax_session_attn_grouped says so: below).  Nothing is reordered after the fork: there are no spares and no per-step
 * copies, private pages come out of each row's own static share, so no EMMAX_ERR_NOMEM case exists beyond a plain batch's, and
 * emmax_session_bytes grows by one int32 per decode row (the groups' shared page counts).  Every weight format and every cache format is served (the copy goes by planes).
 *
 *   emmax_session_set_sample_groups    N = n for every prefill from now on.  EMMAX_ERR_INVALID outside 2 .. min(max_batch,
 *                                      emmax_model_max_decode_batch); EMMAX_ERR_STATE while beams are on or request slots are open.
 *   emmax_session_clear_sample_groups  groups off; the page table is the identity again and the session launches what it launched before.
 *   emmax_session_sample_groups        N, 0 = off, -1 null session.
 * With groups on emmax_session_set_beams and emmax_slots_open return EMMAX_ERR_STATE. */
int emmax_session_set_sample_groups(emmax_session* s, int n, emmax_stream stream);
int emmax_session_clear_sample_groups(emmax_session* s, emmax_stream stream);
int emmax_session_sample_groups(const emmax_session* s);
/* GROUPED DECODE ATTENTION (new symbols, same ABI).  The rows of a sample group, and the beams of a forked beam group, all reference the
 * prompt's floor(S / 64) complete pages.  Where the route rule holds, a step's attention reads those pages ONCE per group (split partials
 * per (row, head)) and a second launch reads each row's own tail, folds the partials in and writes the row the o-proj reads.  The rule:
 * groups on (sample groups, or beams behind their fork), default numerics, a step whose attention is the one-split direct form (5 rows
 * and more at 32 kv heads), and the tuning switch attn_group: 1 = at every such step, -1 (the default) = only at the batches where the
 * two launches were measured faster than the one (sample groups of 4-16 rows at 32, 48 or 64 rows), 0 = never.  Every other step launches what
 * it launched before.  The page counts
 * live in device memory, written by the fork: a captured step replays for later prompts of other lengths.
 *   emmax_session_attn_grouped   1 if a B-row step of the session, as configured now, takes that route, 0 if not, -1 null session. */
int emmax_session_attn_grouped(const emmax_session* s, int B);

/* ---- sample groups as request slots: one prefill, N sampled slots (new symbols, same ABI) ------------------------------------
 * Slot serving with sampling on (emmax_session_set_sample_groups stays off: the two refusals above are unchanged).  A freshly prefilled
 * slot is FORKED into idle slots between two decode steps, on the decode stream: the followers read the source's floor(S / 64) complete
 * prompt pages through their page-table rows, get a copy of the prompt's partial page (none when S % 64 == 0) and own every later page;
 * each draws its token 0 from the prompt's logit row with the parameters passed here -- the finish of a one-row prefill, so follower j's
 * first token and log-probability are emmax_op_sample of that row with (seed, subseq, step 0).  No logits are copied and no other K/V moves.
 *   source       holds a request whose token 0 is in place, prefilled with sampling on: in place (emmax_slot_prefill / emmax_slots_prefill;
 *                staged_idx = -1) with no decode step since, or committed from request staged_idx of the CURRENT staged batch (the logit
 *                row read is that staging row's, which emmax_slots_commit does not move and the next emmax_slots_prefill_staged
 *                overwrites).
 *   followers    n >= 1 idle slots (released, or never filled), none named twice, none the source.  Each gets ctx_len = S, the source's token
 *                budget, a fresh stop-rule state, the source's processors and prompt ids when processing is on, and the sampling
 *                parameters of the host arrays (n values each, checked as emmax_session_set_sampling checks them).
 *   pages        the slot page table is a permutation (commits swap rows).  A follower's own first floor(S / 64) pages wait in its row of the
 *                session's HIDDEN pages; at every moment the entries a row owns (its table row, but for a follower's shared entries) plus
 *                the hidden entries are a permutation of all page ids, and no slot outside a group references the group's pages.
 *   release      emmax_slot_release as before, one slot at a time.  A follower takes its hidden pages back.  The owner of the shared pages
 *                (the source, later its heirs) takes the hidden pages of the lowest-numbered live follower, which owns the shared pages
 *                from then on and hides nothing; the other followers are untouched.  The last member leaves nothing hidden.
 *                emmax_slots_open, a plain emmax_prefill*, emmax_session_set_beams and emmax_session_set_sample_groups first give
 *                every hidden page back.
 * EMMAX_ERR_STATE (nothing launched): slots not open; sampling off (N greedy rows of one prompt are identical); a decode step ran since
 * an in-place source's prefill; staged_idx is not the request of the current staged batch the source was committed from; the source
 * already belongs to a group; and emmax_slot_prefill / emmax_slots_prefill / emmax_slots_commit into a slot that still belongs to a group.
 * EMMAX_ERR_INVALID: null pointers, n < 1, a slot out of range, a follower named twice / equal to the source / not idle, bad sampling values.
 * Not here: the grouped decode attention (groups in slots are ragged and change at every poll; the one-launch attention reads the shared
 * pages through the table), scores, beams as slots.  emmax_session_bytes grows by one int32 per row and page (the hidden pages).
 *   emmax_slots_page_state   test read-back: the page table and the hidden pages, device int32 [max_batch + stage rows][max pages] each
 *                            (hidden: -1 where a row hides no page). */
int emmax_slots_fork(emmax_session* s, int src_slot, int staged_idx, const int32_t* dst_slots_host, int n, const float* temperature_host,
                     const int32_t* top_k_host, const float* top_p_host, const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream);
int emmax_slots_page_state(emmax_session* s, int32_t* table_out_dev, int32_t* hidden_out_dev, emmax_stream stream);

/* ---- single-kernel entry points (parity tests + micro-benchmarks) -------------------------------------------------- */
/* C[M,N] = epilogue(A[M,K] @ W[N,K]^T): bf16 in, fp32 accumulate on MFMA.  K % 64 == 0, N % 128 == 0.
 * bias/scale: bf16 [N] or NULL; residual: bf16 [M,ldr] or NULL; act: 0 none, 1 exact-erf GELU, 2 SwiGLU over
 * 16-column interleaved (gate,up) groups (then C is [M,N/2]); out_f32: store fp32 instead of bf16. */
int emmax_op_gemm(const void* A_dev, int lda, const void* W_dev, int ldw, void* C_dev, int ldc, int M, int N, int K,
                  const void* bias_dev, int act, const void* scale_dev, const void* residual_dev, int ldr, int out_f32,
                  emmax_stream stream);
/* The same GEMM with `ksplit` K slices per 128x128 tile (fp32 partial tiles in ws_dev, >= ksplit*M*N*4 bytes) and a reduce +
 * epilogue pass: the path the session takes by itself for under-filled problems with a long K (prefill o / down at one
 * frame, batch-1 ViT fc2).  act in {0, 1, 2}.  ksplit = 0: the launch plan a session stage runs with this scratch -- whole
 * tiles, split-K, or whole rounds of 256x256 tiles + the remaining tile columns K-split (one-frame prefill gate/up). */
int emmax_op_gemm_splitk(const void* A_dev, int lda, const void* W_dev, int ldw, void* C_dev, int ldc, int M, int N, int K,
                         const void* bias_dev, int act, const void* scale_dev, const void* residual_dev, int ldr, int out_f32,
                         int ksplit, void* ws_dev, int64_t ws_bytes, emmax_stream stream);
/* The launch plan emmax_op_gemm / a session stage would run for this problem, as text (host only, no device work): which tile
 * geometry, row / column parts, split-K slices, and whether the split-K reduce pass also applies the RMSNorm behind the projection
 * (with_norm; one-frame prefill o-proj / down).  ws_bytes = size of the split-K scratch (0: none).  e.g. M = 768, N = 22016, K = 4096,
 * act = 2, 64 MB scratch: "hybrid cols 0..21760: big | cols 21760..22016: splitk ks=8".  has_residual = 2 (with out_f32): the residual and the
 * result are fp32 rows -- the prefill's fp32 residual stream (round 5). */
int emmax_gemm_plan(int M, int N, int K, int act, int out_f32, int has_ln, int has_residual, int with_norm, int64_t ws_bytes, char* text_out,
                    int text_len);
/* Every kernel launch the same call would make, one line of text each (host only, no device work): the launchers themselves run with
 * their launches diverted into the text, so the list is what runs.  Beyond emmax_gemm_plan's arguments it takes what the choice of epilogue
 * looks at -- which of bias / LayerScale exist, the pitches (elements), n_store, a_hl (K is then the width of the two-term rows, 2 x the real
 * K), the addresses of C and of the residual modulo 16 -- and ksplit (0: the launch plan; >= 2: that many K slices, as emmax_op_gemm_splitk).
 *   gemm geom=small|big|k32 act=A out=bf16|f32 ln=L deep=D epi=staged|direct-vec|direct-elt rows=a..b cols=c..d ks=S ksteps=b0..e0,b1..e1,...
 *        hl=H lnrt=R res=none|bf16|f32 grid=G     one tile kernel: its template arguments, the epilogue it takes, the part of the problem it
 *        covers (weight columns), the K steps of every slice, run-time LayerNorm operands, the residual it reads
 *   reduce0|reduce1|reduce2|reduce_norm_bf16|reduce_norm_f32 out=.. store=vec|elt res=none|bf16-vec|... rows=.. cols=.. ks=S
 * Returns the number of launches (>= 0), or EMMAX_ERR_INVALID when the launchers refuse the problem. */
int emmax_gemm_launches(int M, int N, int K, int act, int out_f32, int has_ln, int has_residual, int with_norm, int64_t ws_bytes, int has_bias,
                        int has_scale, int lda, int ldw, int ldc, int ldr, int n_store, int a_hl, int c_align, int res_align, int ksplit,
                        char* text_out, int text_len);
/* LayerNorm folded into the projection that consumes it, as the ViT qkv / fc1 stages run (timm Block: norm1 -> attn.qkv, norm2 ->
 * mlp.fc1): C[M,N] = act(LN(X; gamma, beta, eps) @ W^T + bias) without materialising LN(X).  W_dev bf16 [N, ldw] is REWRITTEN in
 * place to bf16(W .* gamma) (what emmax_model_finalize does once per model); stats_ws f32 [M][2], ln_s_ws / ln_c_ws f32 [N] are
 * caller scratch.  act in {0, 1}; K % 64 == 0, N % 128 == 0, K = the LayerNorm width. */
int emmax_op_gemm_ln(const void* X_dev, int ldx, void* W_dev, int ldw, void* C_dev, int ldc, int M, int N, int K, const void* gamma_dev,
                     const void* beta_dev, const void* bias_dev, float eps, int act, float* stats_ws_dev, float* ln_s_ws_dev,
                     float* ln_c_ws_dev, emmax_stream stream);
int emmax_op_layernorm(const void* x_dev, void* y_dev, const void* w_dev, const void* b_dev, int rows, int D, float eps,
                       emmax_stream stream);
int emmax_op_rmsnorm(const void* x_dev, void* y_dev, const void* w_dev, int rows, int D, float eps, emmax_stream stream);
/* softmax(QK^T * scale [+causal]) V over a packed qkv buffer: token t of sequence b lives at row cu_seqlens[b]+t of
 * qkv_dev (bf16, row stride ld_qkv elements); q head h at column q_off + h*head_dim, k/v head h/(Hq/Hkv) at k_off/v_off.
 * out: bf16 rows of Hq*head_dim (row stride ld_out).  head_dim in {64,72,128}. */
int emmax_op_attention(const void* qkv_dev, int ld_qkv, int q_off, int k_off, int v_off, void* out_dev, int ld_out,
                       const int32_t* cu_seqlens_dev, int B, int max_seqlen, int Hq, int Hkv, int head_dim, float scale,
                       int causal, emmax_stream stream);
/* Which instantiation emmax_op_attention (and every ViT block / prefill layer of a session) launches for B sequences of at most max_seqlen
 * tokens -- HOST ONLY, launches nothing and needs no device; the launcher dispatches on the very struct this call fills (attention.hip:
 * attention_form), so the answer cannot differ from the launch.  Outputs (any may be NULL): resident 0 / 1 (the ring kernel: 64-key tiles through
 * a double-buffered LDS ring, one block per query chunk; the resident kernel: an item's whole K / V in LDS, persistent blocks -- short non-causal
 * head_dim 64 / 72 sequences, from 512 / 2048 (sequence, head) items and up to 256 / 288 / 256 tokens; tuning switch attn_resident: 0 never, 2
 * from 8 items), the query waves of a block (3 / 4: whichever wastes fewer padded query rows of max_seqlen; resident 8 / 9), the producer waves
 * (resident: 2), the key groups over the same query waves (2: causal head_dim 128 when the grid leaves at most one block per CU; attn_ksplit 0
 * never / 1 always), the lazy reference maximum 0 / 1 (head_dim 128 unless attn_lazy = 0, and every resident form), and the query rows of a block
 * (resident: the rows an item may hold).  EMMAX_ERR_INVALID: what the launcher refuses for these arguments (B < 1 or max_seqlen < 1 launch nothing). */
int emmax_attention_plan(int B, int max_seqlen, int Hq, int Hkv, int head_dim, int causal, int* resident_out, int* query_waves_out,
                         int* producer_waves_out, int* key_groups_out, int* lazy_out, int* rows_out);
/* Split-KV decode attention over a paged cache (the kernel of emmax_decode_step; HF cached attention at q_len = 1,
 * modeling_prismatic.py:325-341): row b attends to keys 0..ctx_len_dev[b] (inclusive: the key appended by this step's qkv
 * kernel sits at position ctx_len[b]).  q: bf16 [B, Hq*128] rotated queries; k/vcache: bf16 [n_pages][Hkv][page][128];
 * page_table: int32 [B][max_pages] (token t of row b lives in page page_table[b][t / page]); done_dev: int32 [B] or NULL
 * (rows flagged done read no K/V).  Writes the un-merged partials f32 [B][Hq][nsplit][132] = {o[128] un-normalised, m, l,
 * pad}; the decode step merges them in the o-proj prologue (with ONE split the session's launch normalises and writes the
 * bf16 row itself).  nsplit: power of two <= 16, or 0 = what the session picks
 * for this (B, Hkv) (returned through nsplit_out when non-NULL).  head_dim 128, page = 2^k, max_pages <= 512. */
int emmax_op_decode_attention(const void* q_dev, const void* kcache_dev, const void* vcache_dev, const int32_t* page_table_dev,
                              const int32_t* ctx_len_dev, const int32_t* done_dev, float* part_out_dev, int B, int Hq, int Hkv,
                              int page, int max_pages, int nsplit, float scale, int* nsplit_out, emmax_stream stream);
/* The ONE-split form of the same kernel, as the decode step launches it when a (row, kv head) has a single KV split (batch >= 5 at
 * 32 heads): the block holds the head's whole result, normalises it and writes o_out_dev bf16 [B, Hq*128] -- the row the o-proj
 * reads -- instead of partials (rows flagged done: zeros). */
int emmax_op_decode_attention_direct(const void* q_dev, const void* kcache_dev, const void* vcache_dev, const int32_t* page_table_dev,
                                     const int32_t* ctx_len_dev, const int32_t* done_dev, void* o_out_dev, int B, int Hq, int Hkv,
                                     int page, int max_pages, float scale, emmax_stream stream);
/* The same kernel over the opt-in fp8 KV cache (round 5, tuning switch kv_fp8 at emmax_session_create): K / V pages hold e4m3 rows
 * [pages][Hkv][page][128] with one power-of-two fp32 scale per row (the smallest with amax / scale <= 448), kscale / vscale fp32 [pages][Hkv][page].  The key of THIS step
 * (position ctx_len[b]) is NOT in the cache yet: it waits as bf16 in kv_stage [B][Hkv][2][128] (K row, V row), every block quantises
 * it itself and split 0 appends bytes + scale.  o_out != NULL: the one-split direct form (bf16 [B, Hq*128]); else partials as
 * emmax_op_decode_attention. */
int emmax_op_decode_attention_kv8(const void* q_dev, void* kcache8_dev, void* vcache8_dev, float* kscale_dev, float* vscale_dev,
                                  const void* kv_stage_dev, const int32_t* page_table_dev, const int32_t* ctx_len_dev, const int32_t* done_dev,
                                  float* partials_out_dev, void* o_out_dev, int B, int Hq, int Hkv, int page, int max_pages, int nsplit,
                                  float scale, emmax_stream stream);
/* The grouped form of the one-split attention (emmax_session_attn_grouped), as a pure op: the B rows are B / N groups of N, and the CALLER
 * GUARANTEES that rows g N .. g N + N - 1 hold identical page-table entries for their first shared_pages_dev[g] pages, all of them complete
 * (shared_pages[g] * page <= ctx_len of every row of the group).  Launch 1 reads keys [0, shared_pages[g] * page) once per group, launch 2
 * the keys from there to ctx_len[b] per row; the result is o_out_dev bf16 [B, Hq*128] (rows flagged done: zeros), to the tolerance of
 * emmax_op_decode_attention_direct.  part_ws_dev: f32 scratch of B * Hq * 8 * 132 elements.  shared_pages_dev: int32 [B / N], read back and
 * checked, with ctx_len_dev, before anything is launched (the call synchronises the stream).  EMMAX_ERR_INVALID: N < 2, B % N != 0, a
 * count outside 0 .. max_pages or beyond the context of a row of its group, or a shape the kernels do not take (as the direct form).  _kv8: the same over the fp8 cache, the step's key waiting in
 * kv_stage as for emmax_op_decode_attention_kv8. */
int emmax_op_decode_attention_group(const void* q_dev, const void* kcache_dev, const void* vcache_dev, const int32_t* page_table_dev,
                                    const int32_t* ctx_len_dev, const int32_t* done_dev, void* o_out_dev, int B, int Hq, int Hkv, int page,
                                    int max_pages, float scale, int N, const int32_t* shared_pages_dev, float* part_ws_dev, emmax_stream stream);
int emmax_op_decode_attention_group_kv8(const void* q_dev, void* kcache8_dev, void* vcache8_dev, float* kscale_dev, float* vscale_dev,
                                        const void* kv_stage_dev, const int32_t* page_table_dev, const int32_t* ctx_len_dev,
                                        const int32_t* done_dev, float* part_ws_dev, void* o_out_dev, int B, int Hq, int Hkv, int page,
                                        int max_pages, int N, const int32_t* shared_pages_dev, float scale, emmax_stream stream);
/* Which form of the decode attention a launch takes -- HOST ONLY, launches nothing and needs no device; the launchers dispatch on the very
 * structs these calls fill (decode_attn.hip: decode_attn_form, group_attn_form), so the answer cannot differ from the launch.
 * emmax_decode_attn_plan: B rows, Hq / Hkv heads, kv8 = the fp8 cache.  nsplit > 0 and direct in {0, 1}: what emmax_op_decode_attention (direct
 * 0) / _direct (1; one split only) / _kv8 launch for these arguments under the tuning switches attn_nw / attn_deep.  nsplit = 0, direct = -1:
 * what a B-row step of a default-numerics session with these heads launches (splits by shape or attn_nsplit; direct with one split unless
 * attn_direct = 0).  Outputs (any may be NULL): the GQA group G of the instantiation, waves per block (4 / 8), direct 0 / 1, deep = four chunks of
 * keys in flight instead of two (0 / 1), the split count.  emmax_group_attn_plan: the two launches of emmax_op_decode_attention_group(_kv8) for B
 * rows in groups of N: queries per span block (2 / 4 / 8), splits of the span, query chunks per (group, kv head), the tail's G.
 * EMMAX_ERR_INVALID: a shape the launchers refuse. */
int emmax_decode_attn_plan(int B, int Hq, int Hkv, int nsplit, int direct, int kv8, int* G_out, int* nw_out, int* direct_out, int* deep_out,
                           int* nsplit_out);
int emmax_group_attn_plan(int B, int N, int Hq, int Hkv, int kv8, int* span_width_out, int* span_nsplit_out, int* span_chunks_out, int* tail_G_out);
/* Extension attention (extend_attn.hip): causal attention of n new query rows per sequence over the paged cache.  q_dev bf16 packed rows
 * [total_rows, ldq] (head h at q_off + 128 h, already rotated); sequence b owns rows cu[b] .. cu[b + 1] and its row i sits at position base[b] + i
 * and sees keys 0 .. base[b] + i, ALL read from the cache (kcache / vcache bf16 [pages][Hkv][64][128], or e4m3 bytes + kscale / vscale fp32
 * [pages][Hkv][64]) through page_table int32 [B][max_pages]: the new rows' K / V must have been appended (emmax_op_rope_kv_write_at).  out bf16
 * [total_rows, ld_out].  cu_dev [B + 1] / base_dev [B] are device arrays; the op reads them back and checks them first (it synchronises).  nsplit:
 * 1..16 key splits (kps = ceil((base + n) / nsplit) rounded up to 16; empty splits allowed), 0 = the planner's choice, returned in nsplit_out
 * (may be NULL); more than one split needs ws_dev, f32 [total_rows][Hq][nsplit][132].  head_dim 128, page 64, GQA group in {1, 2, 4, 8}, B <= 64.
 * emmax_op_rope_kv_write_at: emmax_op_rope_kv_write with row i of sequence b at position base[b] + i (cos / sin of max_pos rows); the 16-byte kernel
 * only (head_dim % 16 == 0, 16-byte aligned tables), bit-identical to emmax_op_rope_kv_write at the same positions.
 * emmax_extend_attn_plan: HOST ONLY -- what the launch dispatches on for B sequences of at most max_n new rows and at most max_L keys: the GQA
 * group, tokens per block (128 / G), query tiles per sequence, the split count (asked, or for nsplit = 0 the planner's: one split once
 * B x Hkv x query tiles fill the chip's 256 CUs, else up to one per page and 16) and whether the split form (partials + merge pass) runs. */
int emmax_op_extend_attention(const void* q_dev, int ldq, int q_off, const void* kcache_dev, const void* vcache_dev, const int32_t* page_table_dev,
                              const int32_t* cu_dev, const int32_t* base_dev, int B, int total_rows, int Hq, int Hkv, int page, int max_pages, int nsplit,
                              float scale, void* out_dev, int ld_out, float* ws_dev, long long ws_floats, int* nsplit_out, emmax_stream stream);
int emmax_op_extend_attention_kv8(const void* q_dev, int ldq, int q_off, const void* kcache8_dev, const void* vcache8_dev, const float* kscale_dev,
                                  const float* vscale_dev, const int32_t* page_table_dev, const int32_t* cu_dev, const int32_t* base_dev, int B,
                                  int total_rows, int Hq, int Hkv, int page, int max_pages, int nsplit, float scale, void* out_dev, int ld_out,
                                  float* ws_dev, long long ws_floats, int* nsplit_out, emmax_stream stream);
int emmax_op_rope_kv_write_at(void* qkv_dev, int ld, int q_off, int k_off, int v_off, const int32_t* cu_dev, const int32_t* base_dev, int B, int total_rows,
                              const float* cos_dev, const float* sin_dev, int max_pos, void* kcache_dev, void* vcache_dev, const int32_t* page_table_dev,
                              int max_pages, int Hq, int Hkv, int head_dim, int page, emmax_stream stream);
int emmax_extend_attn_plan(int B, int max_n, int max_L, int Hq, int Hkv, int nsplit, int kv8, int* G_out, int* tokens_per_block_out, int* query_tiles_out,
                           int* nsplit_out, int* split_form_out);
/* SCORING as a pure op (score.hip; still ABI 12: new symbols only).  logits[r, c] = sum_k x[r, k] W[c, k] in fp32 are formed tile by tile and never
 * stored: x bf16 [rows, ldx], W bf16 [Np, ldw] with Np = V padded to a multiple of 128 (rows V .. Np - 1 may hold anything: they never influence an
 * output), K a multiple of 64, ldx / ldw >= K in multiples of 8, both 16-byte aligned.  Launch 1: row tiles (128 rows) x vocabulary slices (runs of
 * 128-column tiles); each block leaves (max, sum exp(x - max), index of the max) per row in ws_dev -- three planes [slices][rows], 12 bytes per row
 * and slice -- and the block whose slice holds targets_dev[r] writes target_logit[r].  Launch 2 merges the slices per row: lse, argmax (the lowest id
 * wins a tie).  No block waits for another inside a launch.  slices: 0 = the planner's choice (about two blocks per CU, at most one slice per column
 * tile and ws_bytes / (12 rows)), else 1 .. column tiles (a count that does not divide the tiles yields ceil(tiles / ceil(tiles / slices)) slices).
 * Outputs as emmax_prefill_score.  EMMAX_ERR_INVALID: K % 64, Np < V or Np % 128, rows < 1 or V < 1, slices above the column tiles, a scratch too
 * small for the slice count asked for (the planner's: for one slice).
 * emmax_score_plan: HOST ONLY -- the planner's row tiles, column tiles, slices and tiles per slice for a scratch of ws_bytes. */
int emmax_op_score_rows(const void* x_dev, int ldx, const void* W_dev, int ldw, int rows, int V, int Np, int K, const int32_t* targets_dev, int slices,
                        float* ws_dev, int64_t ws_bytes, float* lse_out_dev, float* target_logit_out_dev, int32_t* argmax_out_dev, emmax_stream stream);
int emmax_score_plan(int rows, int V, int K, int64_t ws_bytes, int* row_tiles_out, int* col_tiles_out, int* slices_out, int* tiles_per_slice_out);
/* TAPS: HF's output_hidden_states / output_attentions out of the fused path.  A tap is a caller-owned fp32 device buffer that the session fills while
 * it runs a pass it would run anyway; a session that binds nothing launches exactly what it launched before.
 * hidden_layers: bit i (0 <= i <= n_layers) selects HF's hidden_states[i] -- bit 0 the rows behind the embed / patch splice, bit i the residual stream
 * behind layer i's down projection, bit n_layers that of the last layer NORMED (final norm, fp32: HF's last entry is norm(h_L)).  attn_layers: bit i
 * selects layer i's map softmax(q k^T / sqrt(d)) over the row's keys, exact zeros behind them up to ld_keys.  n_sel = the set bits, lowest first.
 * emmax_session_set_pass_taps: filled by the NEXT prefill (emmax_prefill / emmax_prefill_text) or emmax_extend over its packed rows -- hidden_dev
 * [n_sel][total_rows][H], attn_dev [n_sel][total_rows][Hq][ld_keys] -- consumed by that pass and unbound after it.
 * emmax_session_set_step_taps (after a prefill: the buffers' batch B is that of the live rows): filled by every decode step that follows, eager or
 * replayed -- hidden_dev [max_new][n_sel][B][H], attn_dev [max_new][n_sel][B][Hq][ld_keys], a row's entry in the slot of its generation index (the
 * n_out of emmax_session_set_scores: the step that emits token t fills slot t, t >= 1; slot 0 is the prefill's and stays untouched); rows that are done
 * write nothing.  max_new = 1 is the single-step form: every live row lands in slot 0.  During a step ctx_len[b] is the row's cached length before the
 * step = the position of its token: the map covers ctx_len + 1 keys.  Unbound by the next prefill or emmax_extend.
 * A buffer and its mask go together; all NULL / 0 unbinds; emmax_session_clear_taps unbinds both; emmax_session_taps: bit 0 pass taps, bit 1 step
 * taps, -1 for NULL.  Binding or unbinding step taps re-captures the step's graph.  EMMAX_ERR_INVALID: a bit above n_layers (hidden) / n_layers - 1
 * (attentions), ld_keys not a multiple of 4 or smaller than the keys a row sees (checked where the lengths are known: by the pass for pass taps,
 * which then fails before it launches anything; at the binding for step taps), max_new outside 1..max_ctx, head_dim != 128 or a GQA group outside
 * {1, 2, 4, 8} with a map.  EMMAX_ERR_STATE: exact-numerics sessions, beams on, sample groups on, request slots open, step taps before a prefill.  A
 * refused call changes nothing.  emmax_slots_open, emmax_session_set_beams and emmax_session_set_sample_groups UNBIND whatever is bound.
 * What the session cannot check is the caller's: the buffers' SIZES.  A pass fills total_rows = the sum of the pass's row counts (patch rows included)
 * and trusts the pass-tap buffers to hold that many; the step-tap buffers are trusted to hold max_new slots of the B live rows of the binding.  A
 * decode step of another batch than that B (there is none between a binding and the prefill or emmax_extend that unbinds it, short of slot
 * serving, which unbinds) writes NOTHING into the step taps rather than index rows the buffers do not have. */
int emmax_session_set_pass_taps(emmax_session* s, float* hidden_dev, uint64_t hidden_layers, float* attn_dev, uint64_t attn_layers, int ld_keys, emmax_stream stream);
int emmax_session_set_step_taps(emmax_session* s, float* hidden_dev, uint64_t hidden_layers, float* attn_dev, uint64_t attn_layers, int ld_keys, int max_new,
                                emmax_stream stream);
int emmax_session_clear_taps(emmax_session* s, emmax_stream stream);
int emmax_session_taps(const emmax_session* s);
/* Taps (taps.hip): the kernels that hand the residual stream and the attention maps out as fp32, as pure ops.
 * emmax_op_attn_probs(_kv8): for the sequences of emmax_op_extend_attention (q_dev, cu_dev, base_dev, the page table and the K cache as there; no V)
 * the fp32 rows softmax(scale q . K^T): probs_dev f32 [total_rows][Hq][ld_keys], row i of sequence b holds its probabilities at keys 0 .. base[b] + i
 * and EXACT ZEROS from there to ld_keys - 1 -- every entry of every row is written, the caller does not clear the buffer; nothing past total_rows is
 * touched.  Two passes over the keys (maximum and fp32 sum; then fl(2^(fl(s c - m c)) x fl(1 / l)), c = fl(scale log2 e)).  ld_keys: a multiple of 4,
 * at least the keys any row sees (checked against the lengths read back: EMMAX_ERR_INVALID); probs_dev 16-byte aligned; head_dim 128, page 64, GQA
 * group in {1, 2, 4, 8}, B <= 64.  The launch dispatches on the GQA group and the cache format alone: there is no plan to ask for.
 * emmax_op_tap_rows: rows x H of src_dev (fp32 rows when src_f32, else bf16; row pitch ld_src elements) into dst_dev f32 [rows][H]; norm_w_dev (bf16
 * [H], may be NULL): the RMSNorm of each row in fp32, y = fl(fl(x rstd) w) with rstd = rsqrt(sum x^2 / H + eps).  H % 8 == 0, 16-byte aligned. */
int emmax_op_attn_probs(const void* q_dev, int ldq, int q_off, const void* kcache_dev, const int32_t* page_table_dev, const int32_t* cu_dev,
                        const int32_t* base_dev, int B, int total_rows, int Hq, int Hkv, int page, int max_pages, float scale, float* probs_dev, int ld_keys,
                        emmax_stream stream);
int emmax_op_attn_probs_kv8(const void* q_dev, int ldq, int q_off, const void* kcache8_dev, const float* kscale_dev, const int32_t* page_table_dev,
                            const int32_t* cu_dev, const int32_t* base_dev, int B, int total_rows, int Hq, int Hkv, int page, int max_pages, float scale,
                            float* probs_dev, int ld_keys, emmax_stream stream);
int emmax_op_tap_rows(const void* src_dev, int src_f32, int ld_src, float* dst_dev, int rows, int H, const void* norm_w_dev, float eps, emmax_stream stream);
/* Decode-path weight-streaming GEMV: y[b,n] = sum_k x[b,k] W[n,k]  (bf16 in, fp32 accumulate, bf16 out), B <= 8. */
int emmax_op_gemv(const void* x_dev, const void* W_dev, void* y_dev, int B, int N, int K, emmax_stream stream);

/* Pillow-exact antialiased bicubic resize of uint8 RGB frames [B,H,W,3] -> [B,OH,OW,3] on the device (the `resize-naive`
 * transform of processing_prismatic.py:136 for non-224 cameras).  bounds_* int32 [out,2] = (first input index, taps),
 * kk_* int32 [out,ksize] = 22-bit fixed-point taps as Pillow's precompute_coeffs/normalize_coeffs_8bpc produce them
 * (emmax/resize.py builds them); tmp: uint8 [B,H,OW,3] scratch, needed when both axes change. */
int emmax_op_resize_bicubic_u8(const uint8_t* src_dev, int B, int H, int W, uint8_t* dst_dev, int OH, int OW, uint8_t* tmp_dev,
                               const int32_t* bounds_h_dev, const int32_t* kk_h_dev, int ksize_h, const int32_t* bounds_v_dev,
                               const int32_t* kk_v_dev, int ksize_v, emmax_stream stream);

/* fp8 variant: quantise a row-major bf16 [N,ld] matrix to e4m3 fragment-major tiles + fp32 per-row scales (N % 16, K % 64),
 * and the matching small-batch projection (activations bf16, weights de-quantised in registers).  B <= 8: decode_mfma.hip; 9-32 rows:
 * the K-split kernels over the same tiles (decode_km.hip 9-16: K % 512 == 0 up to 4096 or the phased form above; decode_kmp.hip 17-32:
 * K % 64 == 0, K >= 512, the widest wave share <= 1408 elements), EMMAX_ERR_INVALID outside those shapes. */
int emmax_op_quant_fm8(const void* W_dev, int ld, void* W8_fm_out_dev, float* scales_out_dev, int N, int K, emmax_stream stream);
/* MXFP4 copy of a bf16 weight [N, ld] as emmax_model_finalize builds it for decode_fp8 = 2, and its way back.  Blocks of 32 consecutive k of
 * one row share the exponent e = floor(log2(amax)) - 2 clamped to [-127, 127], stored as the e8m0 code e + 127 (an all-zero block: code 127);
 * elements are w / 2^e rounded to nearest, ties to even, onto +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at 6.  tiles_out: N K / 2 bytes --
 * 1 KiB tiles of 16 rows x 128 k in decode_km.hip's row order (perm / perm_hd as emmax_op_repack_km), lane l = row l & 15, dword j of its 16
 * bytes = elements 8 (l >> 4) .. + 8 of the tile's j-th 32 k, element i in nibble i; scales_out: N K / 32 bytes, one dword of four codes per
 * (tile, row) in the tiles' order.  N % 16 == 0, K % 128 == 0, ld % 8 == 0.  emmax_op_dequant_mxfp4 writes the values the copy holds as bf16
 * (exact: one mantissa bit times a power of two; zeros are +0) to the rows of W_out [N, ld] the permutation took them from. */
int emmax_op_quant_mxfp4(const void* W_dev, int ld, void* tiles_out_dev, void* scales_out_dev, int N, int K, int perm, int perm_hd, emmax_stream stream);
int emmax_op_dequant_mxfp4(const void* tiles_dev, const void* scales_dev, void* W_out_dev, int ld, int N, int K, int perm, int perm_hd, emmax_stream stream);
/* the plain projection over such a copy (perm 0) on the kernels the decode step runs, 1 <= B <= 16: y bf16 [B, N] = x bf16 [B, K] W^T with the tiles
 * widened in registers.  K % 1024 == 0 and K <= 4096 (the K-split kernel; the phased kernel of the down projection is reached through
 * emmax_op_decode_stage); N % 16 == 0, N <= 32768.  Test hook: pins what the hardware widening does on every scale code. */
int emmax_op_gemm_small_mxfp4(const void* x_dev, const void* tiles_dev, const void* scales_dev, void* y_dev, int B, int N, int K, emmax_stream stream);
/* The same three for MXFP6 e2m3 (decode_fp8 = 4).  Blocks, the scale rule (e = floor(log2(amax)) - 2 clamped to [-127, 127], code e + 127, an
 * all-zero block: code 127) and the scale stream (one dword of four codes per (tile, row): scales_out N K / 32 bytes) are MXFP4's; elements are
 * w / 2^e rounded to nearest, ties to even, onto +-{0, 0.125 .. 0.875 (subnormals), 1 .. 1.875, 2 .. 3.75, 4 .. 7.5}, saturating at 7.5; the 6-bit
 * code is sign . exponent (2 bits, bias 1) . mantissa (3 bits).  tiles_out: N K 6 / 8 bytes -- tiles of 16 rows x 128 k = 1536 B in decode_km.hip's row
 * order, lane l = 16 g + r owns the 32 elements of scale block g of row r (consecutive k, as OCP defines a block) as 192 bits, element i in bits
 * [6 i, 6 i + 6) little endian -- what v_cvt_scalef32_pk32_bf16_fp6 reads from six registers; bytes 0-15 of the 24 at 16 l of the tile's first KiB,
 * bytes 16-23 at 8 l of the 512 B behind it.  N % 16 == 0, K % 128 == 0, ld % 8 == 0.  emmax_op_dequant_mxfp6 writes the values back as bf16
 * (exact: four significant bits times a power of two; zeros are +0; a value past the largest bf16 -- scale codes 253 / 254 with large elements,
 * out of a bf16 weight's reach -- is infinity).  emmax_op_gemm_small_mxfp6: the plain projection, 1 <= B <= 16, K % 1024 == 0 and K <= 4096,
 * N % 16 == 0, N <= 32768.  Test hook: pins the hardware widening on every element code at every position of a block and on every scale code. */
int emmax_op_quant_mxfp6(const void* W_dev, int ld, void* tiles_out_dev, void* scales_out_dev, int N, int K, int perm, int perm_hd, emmax_stream stream);
int emmax_op_dequant_mxfp6(const void* tiles_dev, const void* scales_dev, void* W_out_dev, int ld, int N, int K, int perm, int perm_hd, emmax_stream stream);
int emmax_op_gemm_small_mxfp6(const void* x_dev, const void* tiles_dev, const void* scales_dev, void* y_dev, int B, int N, int K, emmax_stream stream);
/* MXFP4's sibling for 17 <= B <= 32: decode_kmp.hip's MXFP4 form (what a model created under the tuning switch mx4_wide runs at 17-64 rows), plain
 * epilogue.  N % 16 == 0, N <= 32768; K % 128 == 0 and at least 1024 (one load step of 128 k for each of eight waves); K <= 4096 (four phases of
 * 128 k per wave), or K <= 11264 with N <= 4096 (the eleven-phase form of the down projection: one tile per block).  Needs no model and no switch. */
int emmax_op_gemm_wide_mxfp4(const void* x_dev, const void* tiles_dev, const void* scales_dev, void* y_dev, int B, int N, int K, emmax_stream stream);
int emmax_op_gemm_small_fp8(const void* x_dev, const void* W8_fm_dev, const float* scales_dev, void* y_dev, int B, int N, int K,
                            emmax_stream stream);
/* Batch 3-32 decode projection on the K-split MFMA kernels (decode_km.hip up to 16 rows, decode_kmp.hip above; K > 4096: the phased kernel of the
 * down projection, y = W x through a zeroed residual; what emmax_decode_step runs for qkv / o-proj / gate-up /
 * lm-head at batch >= 3): W_km = emmax_op_repack_km(W row-major [N, ld]) -- fragment-major 16-row tiles, perm 0 natural row order,
 * 1 = qkv (rows d and d + head_dim/2 of a head in one tile), 2 = gate/up (gate_g and up_g in one tile; source in the 16-row
 * interleaved order of the model arena).  y bf16 [B, N] = x bf16 [B, K] W^T (perm 0).  K % 256 == 0, K <= 4096. */
int emmax_op_repack_km(const void* W_dev, int ld, void* W_km_dev, int N, int K, int perm, int head_dim, emmax_stream stream);
int emmax_op_gemm_small_km(const void* x_dev, const void* W_km_dev, void* y_dev, int B, int N, int K, emmax_stream stream);
/* fp8 rows for batch 1-2: the same e4m3 values and scales as emmax_op_quant_fm8, laid out as N rows of K bytes in the span
 * order the dot-product GEMV streams (decode.hip, emmax_quant_rm8_kernel; K % 16 == 0), and that GEMV (1 <= B <= 2). */
int emmax_op_quant_rm8(const void* W_dev, int ld, void* W8_rows_out_dev, float* scales_out_dev, int N, int K, emmax_stream stream);
int emmax_op_gemv_fp8(const void* x_dev, const void* W8_rows_dev, const float* scales_dev, void* y_dev, int B, int N, int K,
                      emmax_stream stream);
/* Small-batch decode projection on MFMA: y[b,n] = sum_k x[b,k] W[n,k], weights in the MFMA-fragment-major layout that
 * emmax_op_repack_fm produces from a row-major [N,ld] matrix (N % 16 == 0, K % 32 == 0); 1 <= B <= 8. */
int emmax_op_repack_fm(const void* W_dev, int ld, void* W_fm_out_dev, int N, int K, emmax_stream stream);
int emmax_op_gemm_small(const void* x_dev, const void* W_fm_dev, void* y_dev, int B, int N, int K, emmax_stream stream);

/* ---- one stage of a decode step through the step's own dispatch (ABI 10; tests/test_decode_stages_gpu.py) ------------------------------
 * emmax_op_decode_stage runs ONE projection stage -- 0 qkv, 2 o-proj, 3 gate/up, 4 down of decoder layer `layer`, or 5 the lm-head with the
 * greedy finish -- for rows 0 .. B - 1 of a created session (no prefill needed) exactly as emmax_decode_step would: the step's routing, the
 * weight copies emmax_model_finalize / emmax_model_build_aux built, its two-launch splits (down / lm-head above 32 rows, chunks of 8 rows in
 * exact numerics).  The caller's rows are copied into the session's buffers, the stage runs, the results are copied back; the stream is
 * synchronised.  R = min(max_batch, 64) below.  Greedy sessions only (EMMAX_ERR_STATE with sampling, processing, scores, beams or open slots).
 *   h_in_dev, h32_in_dev    the hidden rows: bf16 [R][hidden] and the fp32 stream [R][hidden] -- ALL R rows go in, the stage runs on B
 *   h_out_dev, h32_out_dev  the same R rows afterwards (any may be NULL): rows B .. R - 1 must come back bit-unchanged
 *   ctx_len_host            qkv: int32 [B], the position each row's K / V go to; a value outside 0 .. max_ctx - 2 is EMMAX_ERR_INVALID
 *                           before anything is launched
 *   page_table_host         qkv, optional: int32 [B][max_pages], rows 0 .. B - 1 of the page table for this launch; together they must be a
 *                           permutation of pages 0 .. B * max_pages - 1 (what those rows own), else EMMAX_ERR_INVALID.  The identity table
 *                           is back afterwards.  NULL: the session's table as it is
 *   x_in_dev                o-proj: what *oproj_form_out says -- 0: the bf16 attention rows [B][Hq * 128]; 1: split partials f32
 *                           [B][Hq][*nsplit_out][132] = {o[128] un-normalised, m, l, pad}; 2 (exact numerics, one split): fp32 rows
 *                           [B][Hq * 128].  down: the activation rows [B][inter_p], inter_p = inter padded to 64 (bf16; fp32 in exact numerics).
 *                           A call with stage 2 and h_in_dev = h32_in_dev = x_in_dev = NULL only reports form and nsplit for B rows
 *   y_out_dev               qkv: the q rows [B][Hq * 128] (bf16; fp32 in exact numerics); gate/up: the activation rows [B][inter_p] (bf16;
 *                           fp32 in exact numerics); lm-head: f32 [B][vocab] logits (required there)
 *   tok_out_dev             lm-head: int32 [B], the token the greedy finish picks per row -- run against per-row state of the op's own, not
 *                           the session's generation state
 *   via_out                 the launcher family that served the LAST launch of the stage (EMMAX_VIA_*)
 * emmax_op_decode_route answers on the HOST, launching nothing and needing no device, which family emmax_op_decode_stage would report for
 * (stage, B rows) of a model -- created is enough -- under the current tuning switches (exact != 0: for an exact-numerics session), from the
 * copies the model has or emmax_model_build_aux would build now; EMMAX_ERR_INVALID with the refusal when a launch of the stage has no taker.
 * emmax_op_decode_kv_read decodes the K and V rows of (layer, row, positions p0 .. p0 + n - 1) of the paged cache to fp32 on the HOST:
 * k_out_host / v_out_host float [n][Hkv][head_dim], whatever the cache format (bf16, e4m3 + scale, 24-bit, fp32).  page_row_host: int32
 * [max_pages], the row's page-table row to look positions up in (NULL: the session's).  from_stage = 1 (fp8 KV cache only): the row's entry
 * of the staging rows the qkv launch writes instead of the cache, [1][Hkv][head_dim] each (p0 / n ignored). */
enum { EMMAX_VIA_NONE = 0, EMMAX_VIA_KS = 1, EMMAX_VIA_GEMV = 2, EMMAX_VIA_GEMV_FP8 = 3, EMMAX_VIA_KM = 4, EMMAX_VIA_KMP = 5, EMMAX_VIA_MFMA = 6 };
int emmax_op_decode_stage(emmax_session* s, int layer, int stage, int B, const void* h_in_dev, const float* h32_in_dev, const int32_t* ctx_len_host,
                          const int32_t* page_table_host, const void* x_in_dev, void* h_out_dev, float* h32_out_dev, void* y_out_dev,
                          int32_t* tok_out_dev, int* via_out, int* oproj_form_out, int* nsplit_out, emmax_stream stream);
int emmax_op_decode_route(const emmax_model* m, int stage, int B, int exact, int* via_out);
int emmax_op_decode_kv_read(emmax_session* s, int layer, int row, int p0, int n, const int32_t* page_row_host, int from_stage, float* k_out_host,
                            float* v_out_host, emmax_stream stream);

/* ---- the prefill's stage kernels one by one (ABI 12; tests/test_prefill_stages_gpu.py) -----------------------------------------------------------
 * Thin wrappers over the launchers the LLM prefill runs between its GEMMs and its attention: pure ops -- no session, no device allocation.
 * Every argument check returns EMMAX_ERR_INVALID (a split-K workspace that is too small: EMMAX_ERR_NOMEM) with a message.
 *   emmax_op_gemm_stream       the projection onto the fp32 residual stream (tuning switch resid32): C32[M, ldc] = residual32 + scale .* act(A W^T +
 *                              bias) (act 0 none, 1 exact-erf GELU), A bf16 [M, lda], W bf16 [N, ldw], fp32 accumulate, fp32 residual in, fp32 rows out -- nothing of the stream passes
 *                              through bf16.  residual32 = NULL: the stream is its own residual, C32 += ..., the aliased form the prefill runs (ldr
 *                              ignored); else a separate fp32 [M, ldr].  Columns >= n_store are not written (1 <= n_store <= N,
 *                              ldc >= n_store).  ksplit = 0: the launch plan a session stage runs with this workspace (emmax_gemm_plan with
 *                              has_residual = 2 prints it); ksplit >= 2: that many K slices + the reduce pass, on the tile geometry the tuning switch
 *                              gemm_sk_big names, as emmax_op_gemm_splitk.  norm_w / norm_out (both or neither): norm_out bf16 [M, ld_norm] =
 *                              RMSNorm of the result rows (norm_w bf16 [N], eps), applied by the split-K reduce pass.  A path that cannot apply it
 *                              there (act 1, N != 4096, n_store < N, a launch plan that does not split K) REFUSES the call: the norm is never skipped.
 *                              K % 64 == 0, N % 128 == 0, lda / ldw % 8 == 0, 16-byte aligned pointers.
 *   emmax_op_rmsnorm_f32       HF LlamaRMSNorm on fp32 rows x [rows, ldx]: statistics and normalise in fp32, round to bf16, multiply by w bf16 [D], round;
 *                              y bf16 [rows, ldy].  D % 8 == 0, D <= 8192, ldx % 4 == 0, ldy % 8 == 0.
 *   emmax_op_rope_kv_write     RoPE (rotate-half pairs d, d + head_dim / 2) in place on the q and k heads of every packed row of qkv bf16 [total_rows, ld]
 *                              (token t of sequence b = row cu[b] + t, position t) from fp32 tables cos_t / sin_t [position][head_dim / 2], and the
 *                              append of the rotated K and the V rows to kcache / vcache bf16 [pages][Hkv][page][head_dim] at page
 *                              page_table[b][t / page], slot t % page.  kcache = vcache = NULL: rotate only (the fp8 KV cache: emmax_op_kv_quant_rows
 *                              appends).  head_dim, ld and the offsets in multiples of 8; the 16-byte kernel runs when head_dim % 16 == 0 and the
 *                              tables are 16-byte aligned, else the element-wise one -- bit-identical.  1 <= B <= 64.
 *   emmax_op_kv_quant_rows     the fp8 KV append of the prefill: the K (already rotated) and V rows of every packed token as e4m3 bytes k8 / v8
 *                              [pages][Hkv][page][128] with one power-of-two fp32 scale per row (the smallest with amax / scale <= 448; an all-zero
 *                              row: 1), kscale / vscale fp32 [pages][Hkv][page]; the rows are written back into qkv as bf16 of e4m3 x scale.
 *                              head_dim 128 only.
 *   emmax_op_embed_splice      h bf16 [sum_b S_b, hidden], row cu[b] + s = s == 0 ? E[ids[b][0]] : s <= n_patches ? patches[b][s - 1] :
 *                              E[ids[b][s - n_patches]], ids int32 [B, P_max] clamped to 0 .. vocab - 1, S_b = cu[b + 1] - cu[b] <= max_seqlen;
 *                              n_patches = 0 (patches may be NULL): text only.  h32 != NULL: the same rows widened to fp32.  hidden % 8 == 0.
 *   emmax_op_gather_last_rows  out bf16 [B, D] = the last row of every packed sequence, row cu[b + 1] - 1 of in bf16 [.., D] or, when in32 is given
 *                              instead, of in32 fp32 [.., D] rounded to nearest even; out32 != NULL: the rows also as fp32 (widened, or copied from
 *                              in32).  D % 8 == 0. */
int emmax_op_gemm_stream(const void* A_dev, int lda, const void* W_dev, int ldw, float* C32_dev, int ldc, const float* residual32_dev, int ldr, int M, int N,
                         int K, const void* bias_dev, int act, const void* scale_dev, int n_store, int ksplit, void* ws_dev, int64_t ws_bytes,
                         const void* norm_w_dev, void* norm_out_dev, int ld_norm, float eps, emmax_stream stream);
int emmax_op_rmsnorm_f32(const float* x_dev, int ldx, void* y_dev, int ldy, const void* w_dev, int rows, int D, float eps, emmax_stream stream);
int emmax_op_rope_kv_write(void* qkv_dev, int ld, int q_off, int k_off, int v_off, const int32_t* cu_seqlens_dev, int B, int total_rows, const float* cos_dev,
                           const float* sin_dev, void* kcache_dev, void* vcache_dev, const int32_t* page_table_dev, int max_pages, int Hq, int Hkv, int head_dim,
                           int page, emmax_stream stream);
int emmax_op_kv_quant_rows(void* qkv_dev, int ld, int k_off, int v_off, const int32_t* cu_seqlens_dev, int B, int total_rows, void* k8_dev, void* v8_dev,
                           float* kscale_dev, float* vscale_dev, const int32_t* page_table_dev, int max_pages, int Hkv, int head_dim, int page, emmax_stream stream);
int emmax_op_embed_splice(const int32_t* ids_dev, int P_max, const int32_t* cu_seqlens_dev, const void* embed_dev, const void* patches_dev, void* h_dev,
                          float* h32_dev, int B, int max_seqlen, int n_patches, int hidden, int vocab, emmax_stream stream);
int emmax_op_gather_last_rows(const void* in_dev, const float* in32_dev, void* out_dev, float* out32_dev, const int32_t* cu_seqlens_dev, int B, int D,
                              emmax_stream stream);

/* ---- the vision encode's glue kernels and stages one by one (still ABI 12: new symbols only; tests/test_vision_stages_gpu.py) ----------------------
 * The glue kernels as pure ops -- no session, no device allocation.  Each refuses with EMMAX_ERR_INVALID what its kernel cannot do, and launches
 * nothing then.
 *   emmax_op_patch_gather     the processor's normalisation fused with timm PatchEmbed's im2col: out row (b, py, px) = the patch's 3 patch^2 values in
 *                             conv-weight order k = c patch^2 + dy patch + dx, zeros from 3 patch^2 to kpad.  from_u8 = 1: src uint8 [B, img, img, 3],
 *                             value = ((float)u / 255 - mean[c]) / std[c] in fp32 (mean_host / std_host: float[3] on the HOST; chan0 ignored);
 *                             from_u8 = 0: src bf16 pixel_values [B, 6, img, img], channels chan0 .. chan0 + 2 (chan0 0 or 3; mean / std unused but
 *                             required).  hl = 0: out bf16 [B (img / patch)^2, kpad], one rounding.  hl = 1 (exact numerics): out bf16
 *                             [.., 2 kpad], per 64 elements 64 hi = bf16(v) then 64 lo = bf16(v - hi); kpad % 64 == 0.  img % patch == 0,
 *                             kpad >= 3 patch^2.
 *   emmax_op_assemble_tokens  timm _pos_embed: tokens row (b, 0) = cls (has_cls = 1), rows (b, has_cls .. has_cls + n_reg - 1) = reg rows in order,
 *                             row (b, has_cls + n_reg + p) = pe[b, p] + pos[p]; pos / cls / reg bf16 with rows of D, pe and tokens rows of pitch ld.
 *                             f32 = 0: pe and tokens bf16, one fp32 add and one rounding; columns D .. ld of tokens are NOT written.  f32 = 1 (exact
 *                             numerics): pe and tokens fp32, and columns D .. ld are written as ZEROS.  ld >= D.
 *   emmax_op_copy_rows        out[(b rows_out + r) ld_out + col_off + d] = in[(b rows_in + r_off + r) ld_in + d], d < D, bf16, 16 bytes at a time:
 *                             D, ld_in, ld_out, col_off in multiples of 8; r_off + rows_out <= rows_in; col_off + D <= ld_out.
 *   emmax_op_row_stats        stats f32 [rows][2] = (mean, rsqrt(var + eps)) of x bf16 [rows, ldx] over D columns, variance about the mean, fp32.
 *                             D % 8 == 0, D <= 8192, ldx % 8 == 0, ldx >= D.
 *   emmax_op_ln_fold          LayerNorm folded into the weight behind it, IN PLACE: W[n, k] = bf16(W[n, k] gamma[k]) for k < K (columns K .. ldw
 *                             untouched), ln_s[n] = sum_k W'[n, k], ln_c[n] = sum_k W[n, k] beta[k] + bias[n] (beta / bias may be NULL: 0).
 *   emmax_op_x_to_bf16        y bf16 [rows, ldy] = x fp32 [rows, ldx] rounded to nearest even, D columns.  D, ldx, ldy in multiples of 8.
 * emmax_op_vision_stage runs ONE stage of the bf16 vision encode of a created session through the encode's own stage functions, as
 * emmax_op_decode_stage does for the decode step.  The caller hands packed bf16 rows at the REAL width; they are copied into the session's
 * padded scratch (whose padding columns keep what they hold), the stage runs, the result is copied out.  Stages (in -> out; N tokens and D columns
 * of the tower, M its MLP width, np patches, V = D0 + D1 the feature width, P1 and H the projector's):
 *   EMBED         frames uint8 [B, img, img, 3] -> token rows [B N, D]: gather, patch GEMM + bias, assemble (EMBED_PIXELS: pixel_values bf16 [B, 6, img, img])
 *   QKV           tokens [B N, D] -> [B N, 3 D]: LayerNorm then GEMM + bias, or row statistics + the folded GEMM (as the model was finalized)
 *   ATTN          qkv [B N, 3 D] -> [B N, D]
 *   PROJ          attention rows [B N, D], tok_in tokens [B N, D] -> tokens + ls1 .* (x W^T + proj_b)
 *   FC1           tokens -> [B N, M]: LayerNorm (or its folded form), GEMM + bias, GELU
 *   FC2           MLP rows [B N, M], tok_in tokens -> tokens + ls2 .* (x W^T + fc2_b)
 *   FEATURES      tokens [B N, D] -> the feature rows [B np, V] with the tower's patch rows at its columns; tok_in (optional): the feature rows before
 *   PJ1 PJ2 PJ3   [B np, V] -> [B np, P1] -> [B np, H] -> [B np, H] (tower / block ignored)
 * It refuses an exact-numerics session, a bad tower, block or stage, and B outside 1 .. max_batch.  The session's last vision result is dropped. */
enum { EMMAX_VSTAGE_EMBED = 0, EMMAX_VSTAGE_QKV = 1, EMMAX_VSTAGE_ATTN = 2, EMMAX_VSTAGE_PROJ = 3, EMMAX_VSTAGE_FC1 = 4, EMMAX_VSTAGE_FC2 = 5,
       EMMAX_VSTAGE_FEATURES = 6, EMMAX_VSTAGE_PJ1 = 7, EMMAX_VSTAGE_PJ2 = 8, EMMAX_VSTAGE_PJ3 = 9, EMMAX_VSTAGE_EMBED_PIXELS = 10 };
int emmax_op_patch_gather(const void* src_dev, void* out_dev, int B, int img, int patch, int kpad, int chan0, const float* mean_host, const float* std_host,
                          int from_u8, int hl, emmax_stream stream);
int emmax_op_assemble_tokens(const void* pe_dev, const void* pos_dev, const void* cls_dev, const void* reg_dev, void* tokens_dev, int B, int n_patches,
                             int has_cls, int n_reg, int D, int ld, int f32, emmax_stream stream);
int emmax_op_copy_rows(const void* in_dev, int ld_in, void* out_dev, int B, int rows_in, int r_off, int rows_out, int D, int ld_out, int col_off,
                       emmax_stream stream);
int emmax_op_row_stats(const void* x_dev, int ldx, float* stats_dev, int rows, int D, float eps, emmax_stream stream);
int emmax_op_ln_fold(void* W_dev, int ldw, int N, int K, const void* gamma_dev, const void* beta_dev, const void* bias_dev, float* ln_s_dev, float* ln_c_dev,
                     emmax_stream stream);
int emmax_op_x_to_bf16(const float* x_dev, int ldx, void* y_dev, int ldy, int rows, int D, emmax_stream stream);
int emmax_op_vision_stage(emmax_session* s, int tower, int block, int stage, int B, const void* in_dev, const void* tok_in_dev, void* out_dev,
                          emmax_stream stream);

/* ---- exact numerics (tuning switch exact), kernel by kernel: fp32 operands in, fp32 results out (tests/test_exact_gpu.py).
 * hl_ws: device scratch for the two-term bf16 image of the activation operand, 4 bytes per (padded) element.
 *   emmax_op_x_gemm       C32[M, N] = act(A32[M, K] W[N, K]^T + bias) (+ residual32): A split into hi + lo, both through the bf16 MFMAs
 *                         (replaces F.linear on fp32 activations; act 0 / 1 GELU / 2 SwiGLU over 16-column (gate, up) groups, C32 [M, N / 2])
 *   emmax_op_x_rownorm    mode 0: y = hi + lo of x (the split alone); 1: HF LlamaRMSNorm in fp32; 2: F.layer_norm in fp32 -- y32 = the two
 *                         terms the consumer GEMM would read, joined
 *   emmax_op_x_attention  softmax(q k^T scale [causal]) v on the fp32 MFMA over packed fp32 qkv rows -> HL rows in hl_ws (pitch 2 * pad64(Hq *
 *                         head_dim)); emmax_op_x_join widens HL rows to fp32 (timm Attention / HF SDPA: modeling_prismatic.py:114-123,404-415)
 *   emmax_op_x_decode_attention  emmax_op_decode_attention over fp32 q rows and the exact-numerics paged cache (same partial layout): kv24_elems = 0:
 *                         fp32 rows [pages][Hkv][page][128] (tuning switch exact = 2); > 0: the 24-bit cache of exact = 1 -- per operand a bf16 plane of
 *                         kv24_elems elements (the top 16 bits of the fp32 value rounded to 24 bits) followed by an 8-bit extension plane
 *   emmax_op_x_decode_attention_direct  its ONE-split form, as exact sessions launch it at 3 - 8 rows: the block normalises the head's result and
 *                         writes the fp32 row IN PLACE over the head's 128 q values in q32_dev [B, Hq * 128] (rows flagged done: zeros); no partials */
int emmax_op_x_gemm(const float* A32_dev, int lda, const void* W_dev, int ldw, float* C32_dev, int ldc, int M, int N, int K, const void* bias_dev, int act,
                    const float* residual32_dev, int ldr, void* hl_ws_dev, void* ws_dev, int64_t ws_bytes, emmax_stream stream);
int emmax_op_x_rownorm(int mode, const float* x_dev, float* y32_dev, const void* w_dev, const void* b_dev, int rows, int D, float eps, void* hl_ws_dev,
                       emmax_stream stream);
int emmax_op_x_attention(const float* qkv32_dev, int ld_qkv, int q_off, int k_off, int v_off, const int32_t* cu_seqlens_dev, int B, int max_seqlen, int Hq,
                         int Hkv, int head_dim, float scale, int causal, void* hl_ws_dev, emmax_stream stream);
int emmax_op_x_join(const void* hl_dev, float* out32_dev, int rows, int D, emmax_stream stream);
int emmax_op_x_decode_attention(const float* q32_dev, const void* kcache_dev, const void* vcache_dev, int64_t kv24_elems, const int32_t* page_table_dev,
                                const int32_t* ctx_len_dev, const int32_t* done_dev, float* part_out_dev, int B, int Hq, int Hkv, int page, int max_pages,
                                int nsplit, float scale, emmax_stream stream);
int emmax_op_x_decode_attention_direct(float* q32_dev, const void* kcache_dev, const void* vcache_dev, int64_t kv24_elems, const int32_t* page_table_dev,
                                       const int32_t* ctx_len_dev, const int32_t* done_dev, int B, int Hq, int Hkv, int page, int max_pages, float scale,
                                       emmax_stream stream);

/* ---- top-N and watched-token log-probabilities (new symbols, same ABI) ---------------------------------------------------------
 * A short, fixed-size slice of the distribution a row's token was drawn from, over the RAW fp32 lm-head row l of V entries (T = 1,
 * unprocessed, unfiltered: the meaning of the chosen token's log-probability, ABI 6 / 7):
 *   lse        m + logf(sum expf(l_i - m)), m = max l, in the sampling kernel's fixed order: the bits of emmax_op_sample's.
 *   top N      1 <= N <= EMMAX_MAX_TOP_LOGPROBS, N <= V.  The entries that are not NaN, ordered by l_i descending, equal fp32 values (+0 = -0)
 *              by the lower id; the first N as (id, fp32(l_i - lse)).  -inf entries are ordinary candidates with log-probability -inf.  Fewer
 *              than N entries that are not NaN: the remaining places are (-1, -inf).  A row that holds a NaN has lse = NaN, and so every
 *              entry's log-probability; the ids are still the order above.
 *   watched    one list of 0 <= W <= EMMAX_MAX_WATCH_IDS ids in [0, V) (256 = the model's n_action_bins: the whole action-bin range fits),
 *              duplicates allowed: watch_lp[w] = fp32(l[id_w] - lse).
 * The emitted token's entry, where it is among them, has exactly the bits of emmax_session_logprobs.  No float atomics: the same inputs give
 * the same bits, whatever the row's place in the batch or B.
 *   emmax_op_top_logprobs           the kernel on its own over rows logits_dev [B][ld] (as emmax_op_sample): top_ids_out / top_lp_out [B][n_top],
 *                                   watch_lp_out [B][n_watch], watch_ids_dev [n_watch] (device; its values are the caller's to check).  Either
 *                                   part may be off (n_top = 0 / n_watch = 0: its pointers are not read).  EMMAX_ERR_INVALID for a null pointer
 *                                   of a part that is on, n_top or n_watch outside the caps, n_top > V, V outside 1..32768 or ld < V.
 *   emmax_session_set_top_logprobs  binds caller-owned device buffers top_ids_dev int32 / top_lp_dev fp32 [R][max_new][n_top] and watch_lp_dev
 *                                   fp32 [R][max_new][n_watch], R = max_batch + emmax_session_stage_rows (row index = the decode row or slot;
 *                                   staging row k is row max_batch + k); the library allocates nothing.  From then on every lm-head that emits
 *                                   a token -- prefills, decode steps eager and replayed, emmax_generate, emmax_slots_step -- is followed by
 *                                   one launch that writes entry [row][t] of each row that emits a token at generation index t (0: the token
 *                                   a prefill emits).  A row that is done, idle or out of budget writes nothing, nor does t >= max_new: such
 *                                   entries keep what the caller put there.  The step graph is keyed on bound / not bound; the buffers, N, W,
 *                                   max_new and the watch list are device words (a change re-captures nothing; the call synchronises the
 *                                   stream).  watch_ids_host is checked against the model's vocabulary.  EMMAX_ERR_INVALID: a cap, a null
 *                                   pointer of a part that is on, both parts off, a watch id outside [0, V), max_new outside 1..max_ctx.
 *                                   EMMAX_ERR_STATE: beams on, or the session does not write its logit rows (neither sampling nor logits
 *                                   processing on; greedy rows sample at temperature 0).  The binding survives emmax_slots_open and prefills
 *                                   of any batch size; emmax_session_clear_sampling / emmax_session_clear_processing / emmax_session_clear_
 *                                   token_rules unbind when they turn the logit rows off, and emmax_session_set_beams is EMMAX_ERR_STATE
 *                                   while bound.  emmax_slots_commit copies a staged request's entry 0 to its slot; emmax_slots_fork and
 *                                   sample groups give every follower the entry 0 of the prompt's one logit row.
 *   emmax_session_clear_top_logprobs  unbinds: the session launches what it launched before.  emmax_session_top_logprobs: 1 / 0 / -1 (null). */
#define EMMAX_MAX_TOP_LOGPROBS 20
#define EMMAX_MAX_WATCH_IDS 256
int emmax_op_top_logprobs(const float* logits_dev, int ld, int B, int V, int n_top, int32_t* top_ids_out_dev, float* top_lp_out_dev, int n_watch,
                          const int32_t* watch_ids_dev, float* watch_lp_out_dev, emmax_stream stream);
int emmax_session_set_top_logprobs(emmax_session* s, int n_top, int32_t* top_ids_dev, float* top_lp_dev, int n_watch, const int32_t* watch_ids_host,
                                   float* watch_lp_dev, int max_new, emmax_stream stream);
int emmax_session_clear_top_logprobs(emmax_session* s, emmax_stream stream);
int emmax_session_top_logprobs(const emmax_session* s);

#ifdef __cplusplus
}
#endif
#endif /* EMMAX_H */
