/* plbert.h — C ABI of the MI355X-native PL-BERT pre-training hot path (libplbert_hip.so).
 *
 * The reference (Fadi987/PL-BERT) has no FFI: its boundary for this path is a Python nn.Module
 * contract.  Each entry point below names the reference interface it stands in
 * for; the Python host in plbert_amd/ (model.py, engine.py) binds them with ctypes and mirrors the
 * reference classes on top.  Plain pointers and sizes only: device pointers are raw HBM addresses
 * (any allocator — the Python host passes torch tensors' data_ptr()), `stream` is a hipStream_t
 * passed as void* (NULL = the legacy default stream).  Every call is asynchronous on `stream`
 * unless stated otherwise.  Return value: 0 = ok, non-zero = error, text via plb_last_error().
 * One engine serves one GPU and one host thread at a time (the reference runs one process per
 * GPU with a single-threaded step loop, train.py:350-357).
 */
#ifndef PLBERT_H
#define PLBERT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PlbEngine PlbEngine;

/* The AlbertConfig subset of the path (train.py:263-265; configs/config.yml:32-39; HF defaults
 * configuration_albert.py:56-75) plus the head sizes (model.py:6,20) and workspace capacity. */
typedef struct {
  int32_t vocab_size;              /* len(symbols) = 188 (train.py:263) */
  int32_t embedding_size;          /* 128 */
  int32_t hidden_size;             /* 768 */
  int32_t num_attention_heads;     /* 12; hidden_size / heads must be 64 */
  int32_t intermediate_size;       /* 2048 */
  int32_t num_hidden_layers;       /* 12 applications of the one shared layer */
  int32_t max_position_embeddings; /* 512 */
  int32_t type_vocab_size;         /* 2 */
  float layer_norm_eps;            /* 1e-12 */
  int32_t num_phonemes;            /* phoneme_predictor out features (model.py:10,24) */
  int32_t num_tokens;              /* token_predictor out features, 0 = PhonemeOnlyModel (model.py:11) */
  int32_t max_batch;               /* capacity: largest B accepted by the calls below */
  int32_t max_seq;                 /* capacity: largest S (<= max_position_embeddings) */
  int32_t inference_only;          /* 1: forward / loss-only use (README.md:91, train.py:288-304 validate): the workspace
                                      keeps ONE layer's activations instead of all of them, no gradient stash; the
                                      backward and AdamW entry points then fail. 0: training engine. */
} PlbConfig;

/* Parameter tensors in flat-buffer order; names follow the reference state_dict.
 * query/key/value weights (and biases) are adjacent so they form the fused [3H,H] QKV operand. */
enum PlbParam {
  PLB_WORD_EMB = 0,   /* encoder.embeddings.word_embeddings.weight        [V,E]  */
  PLB_POS_EMB,        /* encoder.embeddings.position_embeddings.weight    [P,E]  */
  PLB_TYPE_EMB,       /* encoder.embeddings.token_type_embeddings.weight  [2,E]  */
  PLB_EMB_LN_W,       /* encoder.embeddings.LayerNorm.weight              [E]    */
  PLB_EMB_LN_B,       /* encoder.embeddings.LayerNorm.bias                [E]    */
  PLB_MAP_W,          /* encoder.encoder.embedding_hidden_mapping_in.weight [H,E] */
  PLB_MAP_B,          /* ...embedding_hidden_mapping_in.bias              [H]    */
  PLB_LN2_W,          /* <layer>.full_layer_layer_norm.weight             [H]    */
  PLB_LN2_B,          /* <layer>.full_layer_layer_norm.bias               [H]    */
  PLB_Q_W, PLB_K_W, PLB_V_W,   /* <layer>.attention.{query,key,value}.weight [H,H] each */
  PLB_Q_B, PLB_K_B, PLB_V_B,   /* <layer>.attention.{query,key,value}.bias   [H] each   */
  PLB_DENSE_W,        /* <layer>.attention.dense.weight                   [H,H]  */
  PLB_DENSE_B,        /* <layer>.attention.dense.bias                     [H]    */
  PLB_LN1_W,          /* <layer>.attention.LayerNorm.weight               [H]    */
  PLB_LN1_B,          /* <layer>.attention.LayerNorm.bias                 [H]    */
  PLB_FFN_W,          /* <layer>.ffn.weight                               [I,H]  */
  PLB_FFN_B,          /* <layer>.ffn.bias                                 [I]    */
  PLB_FFNO_W,         /* <layer>.ffn_output.weight                        [H,I]  */
  PLB_FFNO_B,         /* <layer>.ffn_output.bias                          [H]    */
  PLB_HEAD_W,         /* phoneme_predictor.weight                         [NP,H] */
  PLB_HEAD_B,         /* phoneme_predictor.bias                           [NP]   */
  /* --- everything below receives no gradient in the reference (train.py:383-390 never reads it) */
  PLB_POOL_W,         /* encoder.pooler.weight                            [H,H]  */
  PLB_POOL_B,         /* encoder.pooler.bias                              [H]    */
  PLB_TOK_W,          /* token_predictor.weight                           [NT,H] (size 0 when num_tokens = 0) */
  PLB_TOK_B,          /* token_predictor.bias                             [NT]   */
  PLB_NPARAM
};

/* Thread-local text of the last error returned by any call on this thread. */
const char* plb_last_error(void);

/* Stands in for: AlbertModel(AlbertConfig(...)) + PhonemeOnlyModel/MultiTaskModel construction
 * (train.py:263-270; model.py:6-11,20-24). Host-only; allocates no device memory. */
int plb_create(const PlbConfig* cfg, PlbEngine** out);
void plb_destroy(PlbEngine* e);

/* Flat parameter layout: offsets/sizes in floats for each PlbParam, the total float count and the
 * count of leading floats that receive gradients (AdamW range). Stands in for
 * nn.Module.parameters()/state_dict() (train.py:272,417). Arrays hold PLB_NPARAM entries. */
int plb_param_layout(const PlbEngine* e, int64_t* offsets, int64_t* sizes, int64_t* total, int64_t* trainable);

/* Bytes of device workspace the engine needs for its capacity (activations stashed for all
 * layers, bf16 weight copies, split-K slabs). The caller allocates it ZERO-FILLED. */
int64_t plb_workspace_bytes(const PlbEngine* e);

/* Borrow the caller's device buffers: fp32 params / grads / AdamW moments (each `total` floats,
 * laid out per plb_param_layout; grads and moments may be NULL for inference-only use) and the
 * workspace. Stands in for module.to(device) / accelerator.prepare (train.py:160-162). */
int plb_bind(PlbEngine* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* workspace,
             int64_t workspace_bytes);

/* Refresh the bf16 (and transposed) compute copies from the fp32 parameters. Call after the
 * parameters were written from outside (load_state_dict, train.py:100; broadcast at start-up).
 * plb_adamw_step does this itself. */
int plb_sync_weights(PlbEngine* e, void* stream);

/* Stands in for PhonemeOnlyModel.forward / MultiTaskModel.forward / AlbertModel.forward
 * (model.py:13-18,26-30; train.py:386; README.md:91): ids int64 [B,S]; lengths int32 [B] = number
 * of valid (attention_mask == 1) leading tokens per sample, or NULL for no padding. Any of the
 * outputs may be NULL: hidden fp32 [B,S,H] (.last_hidden_state), phoneme_logits fp32 [B,S,NP],
 * token_logits fp32 [B,S,NT]. */
int plb_forward(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, float* hidden,
                float* phoneme_logits, float* token_logits, void* stream);

/* AlbertModel's pooler_output (modeling_albert.py:403; computed by the reference, never used by its loss):
 * pooled[b,:] = tanh(pooler.weight · hidden[b,0,:] + pooler.bias); hidden fp32 [B,S,H] (plb_forward's output),
 * pooled fp32 [B,H]. */
int plb_pooler(PlbEngine* e, const float* hidden, int32_t B, int32_t S, float* pooled, void* stream);

/* Stands in for process_batch + calculate_phoneme_loss + accelerator.backward (train.py:381-390,
 * 107-131, 356): masked_ids/labels int64 [B,S]; lengths int32 [B]; the per-sample masked index
 * lists as CSR (idx_offsets int32 [B+1], idx_flat int32 [n_masked], positions < lengths[b], unique
 * within a sample). Writes the scalar loss (fp32, device) and the gradient of every trainable
 * parameter into the bound grads buffer (overwritten, not accumulated). n_masked == 0 reproduces
 * the reference's zero-loss fallback: loss 0 and all gradients 0. */
int plb_loss_fwd_bwd(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int32_t* lengths,
                     const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked, int32_t B, int32_t S,
                     float* loss, void* stream);

/* Stands in for process_batch under torch.no_grad() — validate() (train.py:288-304): forward + the same loss as
 * plb_loss_fwd_bwd (or plb_loss_fwd_bwd_dual when token_ids != NULL; loss_parts optional), NO backward: the bound
 * gradient buffer is not touched, nothing is stashed. Works on training and inference-only engines. */
int plb_loss_fwd(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                 const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked, int32_t B,
                 int32_t S, float* loss, float* loss_parts, void* stream);

/* Dual-head training step for MultiTaskModel (model.py:5-18: phoneme_predictor + token_predictor) fed by the
 * 4-tuple Collater batch (dataloader.py:200-223: token_ids, labels, masked, lengths, indices). The reference
 * defines the head and the batch but trains PhonemeOnlyModel only (train.py:266-270); the token loss here is
 * upstream PL-BERT's: per-sample CrossEntropyLoss (mean) of token_pred[b, :len_b] against token_ids[b, :len_b],
 * averaged over the B samples. loss = phoneme loss (as plb_loss_fwd_bwd) + token loss; loss_parts (optional)
 * receives the two terms. token_ids int64 [B,S] in [0, num_tokens). Gradients of token_predictor.{weight,bias}
 * are written as well and the next plb_adamw_step updates them; after a plb_loss_fwd_bwd call the token head
 * has no gradient and is left alone, like the pooler. n_masked == 0 is allowed (phoneme term 0). */
int plb_loss_fwd_bwd_dual(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                          const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked,
                          int32_t B, int32_t S, float* loss, float* loss_parts, void* stream);

/* Stands in for torch.optim.AdamW.step (train.py:272,357): decoupled weight decay on every
 * trainable parameter, bias-corrected moments; `step` counts from 1; gradients are multiplied by
 * grad_scale first (1/world_size after a sum all-reduce). Also refreshes the bf16 copies. Hyper-parameters are
 * doubles, as torch holds them: the update's scalars (1 - beta2, lr / bias_correction1, ...) are formed in double and
 * rounded to fp32 once, which is what makes the result agree with torch.optim.AdamW to the last bits. */
int plb_adamw_step(PlbEngine* e, double lr, double beta1, double beta2, double eps, double weight_decay, int32_t step,
                   double grad_scale, void* stream);

/* ---- gradient accumulation and global-norm clipping (opt-in: a step that calls none of these launches what it launched
 * before) ----
 * Stands in for what the reference's trio `optimizer.zero_grad(); accelerator.backward(loss); optimizer.step()`
 * (train.py:355-357) gives a caller for free: .grad accumulates over several backward() calls until zero_grad, and
 * torch.nn.utils.clip_grad_norm_ / accelerator.clip_grad_norm_ sits between backward and step. Every backward entry point
 * here OVERWRITES the bound gradient buffer; these calls add the accumulation beside it, in a second flat buffer of the
 * caller's, and a norm / clipping coefficient that never leaves the device. Plain vector loads and stores, no atomics on
 * gradient data, fixed summation order: results are bitwise reproducible from run to run.
 * plb_grad_accum_bind: accum = `total` floats laid out like grads (16-byte aligned, contents arbitrary); NULL unbinds.
 *   Host state only. The workspace is not involved.
 * plb_grad_accum_add: folds the gradients the LAST backward entry point (plb_loss_fwd_bwd*, plb_encode_bwd) left in the
 *   gradient buffer into a WINDOW of micro-steps: phase 0 FIRST (accum = grads; opens the window), 1 ADD (accum += grads),
 *   2 LAST (grads = accum + grads; closes the window: the gradient buffer then holds the sum of the window's micro-steps in
 *   the order ((g1 + g2) + g3) + ..., fp32). A window of one micro-step needs no add at all.
 *   Ranges: the ones plb_adamw_step steps — [0, trainable), or [0, offset of PLB_HEAD_W) after plb_encode_bwd, plus the
 *   token head after a dual-head call. The engine keeps the UNION of what the window's micro-steps produced; a range in the
 *   union that a micro-step did not produce contributes zeros (an ADD skips it; a LAST copies the accumulator out — that
 *   part of the gradient buffer is never read, a phoneme-only call leaves the token range alone). After LAST the "has a
 *   gradient" state of the phoneme head and the token head IS the union: plb_allreduce_grads, plb_grad_norm and either AdamW
 *   entry cover exactly the accumulated ranges, and the token head's step count advances once per update.
 *   norm_buf (LAST only; NULL: not wanted): every workgroup of the LAST pass also leaves the sum of squares of the values it
 *   stored behind the four result floats of norm_buf, so that an accumulated and clipped step reads its gradients once
 *   (plb_grad_norm with have_partials = 1).
 *   Fails BEFORE anything is launched, with a text: no buffer bound; ADD or LAST without a FIRST; the same gradients added
 *   twice (no backward entry point has run since the last add); micro-steps of one window on different parameters
 *   (plb_adamw_step[_clipped], plb_sync_weights, plb_broadcast_params and plb_grad_accum_bind end a window); micro-steps of
 *   which some were all-reduced and some not.
 *   Ordering: like plb_adamw_step, an add first joins the all-reduce pieces its micro-step issued. No add drops a live
 *   plb_encode stash.
 * plb_grad_norm_floats: floats of norm_buf (16-byte aligned, ZERO-FILLED once by the caller): [0] total_norm, [1] coef,
 *   [2] 1.0 when the norm was not finite else 0.0, [3] the number of updates plb_adamw_step_clipped left out for that reason
 *   (it only ever grows; the caller may zero it), then the partial sums of every range.
 * plb_grad_norm: total_norm = grad_scale * sqrt(sum of squares of the gradients plb_adamw_step is about to step), the sum
 *   in fp32 per workgroup on a fixed grid and in double over the workgroups; coef = min(1, max_norm / (total_norm + 1e-6)),
 *   the constants of torch.nn.utils.clip_grad_norm_; max_norm <= 0: no clipping, coef = 1. A norm that is not finite gives
 *   [2] = 1 and coef = 0. have_partials = 1: use the partial sums the preceding plb_grad_accum_add(LAST, norm_buf) left
 *   (fails if there are none in this buffer, or if the gradients were exchanged since); 0: one pass over the gradients.
 *   Nothing is read back: the host may look at norm_buf whenever it reads the loss.
 * plb_adamw_step_clipped: plb_adamw_step with the gradient (g * grad_scale) * coef, coef = norm_buf[1] loaded on the device
 *   (the two products in that order: torch forms the mean gradient, then clips it). With coef == 1 every output is
 *   bit-identical to plb_adamw_step's. norm_buf[2] != 0: parameters, moments and compute copies are left untouched — like
 *   the hand-off skip, which is tested first and keeps its meaning — and norm_buf[3] grows by one (the launch writes that
 *   one float although the argument is const). The host's step count, and plb_token_head_steps after a dual-head window,
 *   have then advanced for an update that did not happen: a host that cares rewinds them when it sees [3] grow.
 * HEALTH WORD (plb_status): unchanged. A micro-step whose hand-off timed out leaves the word set; either AdamW entry skips;
 *   after plb_status has reported it the host starts the window again with FIRST.
 * DATA-PARALLEL RUNS: with overlap off (plb_set_grad_overlap(e, 0)), or with a host-side exchange, the micro-steps do NOT
 *   call plb_allreduce_grads and ONE exchange follows LAST (plb_allreduce_grads covers the accumulated ranges). With overlap
 *   on every micro-step's pieces travel as usual and are joined by its add: the same sum, with k times the traffic.
 *   grad_scale = 1 / (world * k) turns the sum over k micro-steps and `world` ranks into the mean. The norm is taken AFTER
 *   the exchange (have_partials = 0 unless the window came in all-reduced), so every rank computes the same coef. */
int64_t plb_grad_norm_floats(const PlbEngine* e);
int plb_grad_accum_bind(PlbEngine* e, float* accum);
int plb_grad_accum_add(PlbEngine* e, int32_t phase, float* norm_buf, void* stream);
int plb_grad_norm(PlbEngine* e, double grad_scale, double max_norm, float* norm_buf, int32_t have_partials, void* stream);
int plb_adamw_step_clipped(PlbEngine* e, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int32_t step, double grad_scale, const float* norm_buf, void* stream);

/* ---- AdamW parameter groups and frozen tensors (opt-in: a step that calls none of these launches what it launched
 * before) ----
 * Stands in for torch.optim.AdamW([{"params": ..., "lr": ..., "betas": ..., "eps": ..., "weight_decay": ...}, ...]) and for
 * requires_grad = False: every tensor of the flat layout belongs to one of n_groups hyper-parameter sets or is FROZEN.
 * group_of: int32 [PLB_NPARAM] on the host, group_of[i] = the group of tensor i (enum PlbParam), -1 = frozen. The update
 * stays ONE launch per range (the trainable range, the token head), with no further pass over the parameters: the range is
 * cut into SEGMENTS, each with its own pre-rounded scalars, and the segment table travels as a kernel argument (no device
 * table, no copy: the calls stay asynchronous and capturable). A frozen tensor is a hole between segments: neither its
 * parameters nor its moments nor its bf16 copy are loaded or stored, as torch skips such a tensor and leaves its state alone.
 * plb_adamw_plan (host only, no device access; works on an engine that was created and never bound): the live segments
 *   the next plb_adamw_step_groups would launch, in flat-buffer order. begin / end: floats from the start of the flat
 *   buffer, multiples of 4. The scalars are formed in DOUBLE and rounded to fp32 once, exactly as plb_adamw_step forms
 *   them: decay = 1 - lr * weight_decay, omb1 = 1 - beta1, b2 = beta2, omb2 = 1 - beta2, eps, step_size =
 *   lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step). Adjacent tensors of the same group whose rounded scalars and
 *   step agree are merged into one segment. A frozen tensor does not appear; nor does a tensor the engine would not step
 *   anyway, whatever group it was given (torch skips a parameter whose .grad is None): the pooler unless the last backward
 *   call was a plb_encode_bwd_pooled with a d_pooled, the phoneme head after
 *   plb_encode_bwd, the token head unless the last loss call was a dual-head one. Segments of the token head carry the token
 *   head's own next step count (plb_token_head_steps + 1), all others `step`. segs has room for PLB_NPARAM entries.
 * plb_adamw_step_groups: plb_adamw_step (norm_buf == NULL) or plb_adamw_step_clipped (norm_buf = what plb_grad_norm* wrote)
 *   over that plan, with all of their bookkeeping: joins pending all-reduce pieces, ends a live plb_encode stash, the final
 *   state and an accumulation window, refreshes the compute copies, counts a left-out update in word 1 (trainable range) /
 *   word 2 (token head) of the health word and in norm_buf[3]. One group that holds every tensor gives plb_adamw_step's
 *   (plb_adamw_step_clipped's) results bit for bit. A range without a live segment launches nothing; the token head's step
 *   count advances only when the token head is stepped.
 *   `step` is ONE count for all tensors outside the token head, as in plb_adamw_step. DEVIATION from torch, which keeps a
 *   count per parameter: a tensor that was frozen for some steps and is thawed later continues with the shared count, not
 *   with the number of steps it took itself (the deviation plb_encode_bwd documents for the phoneme head).
 * plb_grad_norm_groups: plb_grad_norm with have_partials = 0, over the tensors with group_of[i] >= 0 only (a select, not a
 *   product: a NaN in a frozen tensor's gradient does not reach the norm). Same norm_buf layout, same finish.
 * Refused BEFORE anything is launched, with a text: n_groups < 1; a group_of entry outside [-1, n_groups); lr or eps
 *   negative or not finite; a beta outside [0, 1); step < 1; optimizer buffers not bound; an inference-only engine. */
typedef struct { double lr, beta1, beta2, eps, weight_decay; } PlbAdamWGroup;
typedef struct {
  int64_t begin, end;
  int32_t group, step;
  float decay, omb1, b2, omb2, eps, step_size, bc2_sqrt;
} PlbAdamWSegment;
int plb_adamw_plan(const PlbEngine* e, const PlbAdamWGroup* groups, int32_t n_groups, const int32_t* group_of, int32_t step,
                   PlbAdamWSegment* segs, int32_t* n_segs);
int plb_adamw_step_groups(PlbEngine* e, const PlbAdamWGroup* groups, int32_t n_groups, const int32_t* group_of, int32_t step,
                          double grad_scale, const float* norm_buf, void* stream);
int plb_grad_norm_groups(PlbEngine* e, const int32_t* group_of, double grad_scale, double max_norm, float* norm_buf,
                         void* stream);

/* ---- LAMB: Adam with a layer-wise trust ratio (opt-in: a step that calls none of these launches what it launched before) ----
 * The optimizer of ALBERT and of large-batch BERT pre-training (You et al., "Large Batch Optimization for Deep Learning").
 * torch ships no LAMB, so THIS TEXT IS THE DEFINITION. Per tensor t of the flat layout (one entry of plb_param_layout; tensors
 * are never merged, even when they are adjacent and share their scalars), in a group with lr, beta1, beta2, eps, weight_decay,
 * adapt, at step count k:
 *   g   = (grad * grad_scale) * coef          coef = norm_buf[1] when a norm_buf is given, else 1: plb_adamw_step_clipped's
 *   m   = m + (1-beta1) * (g - m)             the AdamW kernels' expressions, operation for operation
 *   v   = beta2 * v + (1-beta2) * (g*g)
 *   r   = m / (sqrt(v) / sqrt(bc2) + eps)     bc = 1 - beta^k; scalars formed in double on the host and rounded to fp32 once
 *   u   = r * (1/bc1) + weight_decay * p      the decay is INSIDE the update (LAMB), not decoupled
 *   wn  = ||p||_2 over t (p BEFORE the update),  un = ||u||_2 over t
 *   trust = wn / un  if adapt and wn > 0 and un > 0  else 1
 *   p   = p - (lr * trust) * u                then the bf16 compute copy, as AdamW writes it
 * Bias correction is on; neither wn nor trust is clamped. adapt = 0 turns the trust ratio off for a group's tensors (the
 * "exclude from layer adaptation" convention for biases and LayerNorm, which usually have weight_decay = 0 as well). k is
 * `step` for everything outside the token head and plb_token_head_steps + 1 for the token head, as in plb_adamw_step_groups
 * (with its DEVIATION from torch: one count for all tensors outside the token head). A tensor in no group (group_of[i] = -1)
 * or not stepped by this call (the pooler without a gradient, the phoneme head after plb_encode_bwd, the token head unless the last loss call was
 * a dual-head one) is a hole: nothing of it is loaded or stored.
 * exp_avg and exp_avg_sq after a LAMB step are BIT-IDENTICAL to those after plb_adamw_step[_clipped] from the same state with
 * the same betas, grad_scale and coef: a run may change between the two optimizers without touching its moments.
 * The norms: fp32 sums of at most 1024 squares per workgroup, added per tensor in double in a fixed order (no atomics on
 * float data: bitwise reproducible from run to run). Nothing is read back and nothing waits for the host: per range (the
 * trainable range, the token head) two streaming passes and a one-workgroup-per-tensor finish between them, their tensor table
 * a kernel argument. The gradient buffer is only read (`.grad` views of it stay what backward left).
 * plb_lamb_floats: floats of the caller-owned, 16-byte aligned lamb_buf (contents arbitrary). Its first 4 * PLB_NPARAM floats
 *   are [wn, un, trust, live] per tensor (enum PlbParam order) as the LAST step left them — live = 1: stepped, 0: a hole (wn, un
 *   and trust are then 0) —, the per-workgroup partial sums follow. The engine's workspace plan does not change.
 * plb_lamb_plan (host only, like plb_adamw_plan): the per-tensor segments the next plb_lamb_step would launch, in flat-buffer
 *   order: begin / end in floats, tensor = its enum PlbParam, and the scalars omb1 = 1 - beta1, b2 = beta2, omb2 = 1 - beta2,
 *   eps, bc2_sqrt = sqrt(1 - beta2^step), inv_bc1 = 1 / (1 - beta1^step), weight_decay, lr. segs has room for PLB_NPARAM entries.
 * plb_lamb_step: the update over that plan with all the bookkeeping of plb_adamw_step_groups: joins pending all-reduce pieces,
 *   ends a live plb_encode stash, the final state and an accumulation window, advances the token head's step count when the
 *   token head is stepped, refreshes the compute copies (bf16, transposed, fp8). HEALTH WORD: tested first by every launch;
 *   while it is set nothing is stored — m and v are NOT advanced, lamb_buf keeps the last step's results — and the left-out
 *   update is counted once per range in word 1 / word 2 (plb_status_ex). norm_buf[2] != 0 (a norm that is not finite) leaves
 *   everything untouched in the same way and norm_buf[3] grows by one.
 *   Refused BEFORE anything is launched, with a text: what plb_adamw_step_groups refuses, an adapt that is neither 0 nor 1,
 *   a lamb_buf that is null or not 16-byte aligned.
 * DATA-PARALLEL RUNS: the sums are taken over all-reduced gradients and replicated parameters, so wn, un and trust are
 *   identical on every rank: LAMB adds no collective. */
typedef struct { double lr, beta1, beta2, eps, weight_decay; int32_t adapt; } PlbLambGroup;
typedef struct {
  int64_t begin, end;
  int32_t tensor, group, step, adapt;
  float omb1, b2, omb2, eps, bc2_sqrt, inv_bc1, weight_decay, lr;
} PlbLambSegment;
int64_t plb_lamb_floats(const PlbEngine* e);
int plb_lamb_plan(const PlbEngine* e, const PlbLambGroup* groups, int32_t n_groups, const int32_t* group_of, int32_t step,
                  PlbLambSegment* segs, int32_t* n_segs);
int plb_lamb_step(PlbEngine* e, const PlbLambGroup* groups, int32_t n_groups, const int32_t* group_of, int32_t step,
                  double grad_scale, const float* norm_buf, float* lamb_buf, void* stream);

/* fp8 mode (BASELINE.json configs[4]): EVERY projection GEMM of the shared layer runs on OCP fp8 operands with fp32
 * accumulation through the block-scaled MFMA with unit block scales (twice the bf16 MFMA rate) — forward: QKV, dense
 * (+ LayerNorm 1), FFN up (+ gelu_new), FFN output (+ LayerNorm 2); backward: the four dX GEMMs (two of them carrying a
 * LayerNorm backward, one the gelu backward) and the four weight-gradient GEMMs over all applications. e4m3 weights and
 * activations, e5m2 gradients. The 1-byte images are written by the launches that produce the tensors (fused epilogues,
 * attention kernels), one per application of the layer; attention itself, the head, LayerNorm / softmax statistics, the
 * loss and the optimizer stay bf16 / fp32. Delayed scaling, one scale per operand SITE shared by the L applications: a
 * tensor is quantised with 448 / the maximum its site showed in the previous call (gradients: 28672 / the maximum, one
 * binade of headroom); the first call after switching the mode on — and a training call whose gradient sites have not
 * been seen yet — runs in bf16 and only records the maxima. hidden_size 768 or 1024; calls whose GEMM shapes have no
 * pipeline-tile form run in bf16. The reference has no fp8 path (configs/config.yml:15: fp16 autocast): parity is against
 * this library's own bf16 path (tests/test_gpu_fp8.py: loss within 2e-2, whole-gradient relative L2 0.11) and against a
 * CPU restatement of exactly these semantics on top of the pinned oracle (oracle/fp8_np.py). */
int plb_set_fp8(PlbEngine* e, int32_t on, void* stream);
int plb_fp8_state(const PlbEngine* e, int32_t* enabled, int32_t* calibrated);
/* Delayed scaling and its limits. Every operand site quantises a call's values with the scale the PREVIOUS calls' maxima
 * gave — the LARGEST maximum of the last four calls: activations (e4m3) map it to 448, gradients (e5m2) to 28672 = half the
 * format's range. A call whose values exceed everything seen in the last four calls (gradients: 2x that) has the excess
 * CLAMPED in every GEMM operand of that site — silently as far as the loss goes. plb_fp8_stats makes it visible: per site
 * (order: x, a, gelu(u), context; dpre2, dU, dpre1, dQKV), the number of calls since plb_set_fp8 in which values were
 * clamped by more than the top value's rounding step (true maximum x scale > 1.0625 x format maximum) and the worst such
 * overshoot. Synchronises `stream`. No reference counterpart (the reference has no fp8 path). */
int plb_fp8_stats(PlbEngine* e, float clamped_calls[8], float worst_overshoot[8], void* stream);

/* The token head (trained by dual-head steps only) keeps its own AdamW step count, as torch keeps one per parameter
 * (train.py:417-421 saves it in 'optimizer'). Read / restore it around checkpoints. */
int32_t plb_token_head_steps(const PlbEngine* e);
int plb_set_token_head_steps(PlbEngine* e, int32_t steps);

/* ---- data-parallel exchange step (train.py:218-221,160-162,356: accelerate -> DDP -> NCCL; here RCCL over xGMI) ----
 * One process per GPU, one engine per process. Rank 0 calls plb_comm_unique_id and hands the 128 bytes to every rank
 * over any host channel (the Python host: torch.distributed's store); then every rank calls plb_comm_init (collective,
 * blocks until all ranks arrived). The library resolves RCCL at run time (the librccl.so.1 already mapped in the
 * process, else the system one; PLBERT_RCCL_LIB overrides) - it is not linked against it. */
#define PLB_COMM_ID_BYTES 128
int plb_comm_unique_id(uint8_t id[PLB_COMM_ID_BYTES]);
int plb_comm_init(PlbEngine* e, const uint8_t id[PLB_COMM_ID_BYTES], int32_t rank, int32_t world);
int plb_comm_destroy(PlbEngine* e);
int plb_comm_info(const PlbEngine* e, int32_t* rank, int32_t* world, int32_t* rccl_version);
/* Health of the in-launch hand-offs between the column tiles of the LayerNorm-in-GEMM launches (csrc/gemm_ln.hip). Their
 * wait is bounded so that a launch whose tiles were not co-resident long enough ENDS instead of hanging the device; the
 * launch then raises the engine's error word, and by construction (no host round trip anywhere):
 *   - the loss that call returns is NaN, and the word is mirrored into pinned host memory by the call's last launch;
 *   - plb_adamw_step leaves parameters, moments and compute copies untouched while the word is set;
 *   - the word stays set — every later step is skipped the same way — until plb_status has reported it.
 * plb_poll_status: NO synchronisation; the count as of the last loss call that has COMPLETED on the device (read it
 *   wherever the host has just read a loss back, or one step late at the top of the next step).
 * plb_status / plb_status_ex: SYNCHRONISES the device and returns the count since its previous report; a non-zero report also re-zeroes
 *   the exchange buffer and the word (a producer's store that landed after its consumer gave up would otherwise look
 *   fresh to the next launch), so the step after a reported failure starts clean. 0 in every run so far.
 * DATA-PARALLEL RUNS: the word is agreed between the ranks inside every plb_loss_fwd_bwd[_dual] call of an engine with a
 *   communicator — one float per rank, summed by a one-element all-reduce issued after the last launch that can raise
 *   it (overlap on: on the communication stream, between the head piece and the first weight's; overlap off: in
 *   `stream`) and merged by the call's last launch. A time-out on ONE rank therefore gives EVERY rank a NaN loss, a
 *   skipped update and a non-zero count (the sum over the ranks): the replicas stay bit-identical, nobody applies the
 *   poisoned sum. The status all-reduce is not counted by plb_comm_pieces. A host that exchanges gradients by other
 *   means uses plb_status_export / plb_status_import (below) at the same point. plb_loss_fwd (validation) issues no
 *   collective: a word raised there is sticky and travels with the next training call.
 * No reference counterpart (the reference's LayerNorm is torch's kernel); the Python host raises HandoffTimeout. */
int plb_status(PlbEngine* e, int32_t* ln_exchange_timeouts);
/* plb_status + the number of plb_adamw_step calls the device left out since the word was raised (a host that counts
 * optimizer steps for the bias correction rewinds its count by it); either pointer may be NULL. */
int plb_status_ex(PlbEngine* e, int32_t* ln_exchange_timeouts, int32_t* skipped_updates);
int plb_poll_status(const PlbEngine* e, int32_t* ln_exchange_timeouts);
/* For a host that runs the gradient exchange itself (torch.distributed, a foreign communicator): plb_status_export writes
 * this rank's count as one float to `out` (device) behind the loss call in `stream`; the host sums it over the ranks;
 * plb_status_import merges the sum into the word, mirrors it to the host and turns the last loss call's loss into NaN —
 * before plb_adamw_step (the loss buffer handed to that loss call must still be valid: the import writes the NaN there).
 * (With the engine's own communicator both happen inside plb_loss_fwd_bwd.) */
int plb_status_export(PlbEngine* e, float* out, void* stream);
int plb_status_import(PlbEngine* e, const float* summed, void* stream);
/* A phoneme-only loss call evaluates the part of its LAST shared-layer application that lies behind the attention
 * (dense + LayerNorm, FFN, LayerNorm) on the masked rows alone, forward and backward: the reference computes every row
 * and then reads the masked ones (train.py:107-131: pred[b, :len_b][idx_b]), rows only meet inside attention, so the other
 * rows of that part reach neither the loss nor — their output gradient being exactly zero — any gradient. Same results,
 * ~5 % less arithmetic at 13 % masked positions. Reports what the last loss call did: rows = token rows that part ran on
 * (padded to 128), of = the call's padded token count (rows == of: every row — a dual-head call, more than half of the
 * positions masked, or PLBERT_PRUNE_LAST=0; calls in fp8 mode prune like bf16 calls). */
int plb_last_application_rows(const PlbEngine* e, int64_t* rows, int64_t* of);
/* ---- token-packed execution of ragged batches (opt-in) ----
 * The reference collater zero-pads every sample to the batch maximum (dataloader.py:276-297) and the loss slices the pads
 * away again (train.py:107-131); a padded call of B x S runs every projection, FFN, LayerNorm and weight-gradient row for the
 * pads too. A packed call runs on a dense token axis instead: sample b owns rows [row_start[b], row_start[b] + lengths[b])
 * of every activation buffer, in a slot of ceil(lengths[b] / 128) * 128 rows (the attention kernels' row tile: a sample's
 * tiles are those of the padded call). ids / labels / index lists / outputs keep the padded [B,S] layout of the caller.
 * plb_packing_plan (host only, no device access): lengths int32 [B] on the HOST -> row_start int32 [B+1] (host; the caller
 *   copies it to the device with the batch), *used = row_start[B] = rows covered by the slots, *rows = the rows the call
 *   executes = used rounded up to the coarsest of 1024 (LayerNorm in the GEMM epilogues) / 256 (gelu' stash) / 128 that
 *   still leaves fewer rows than the padded call's ceil128(B*S). When nothing is saved (every length == S, or the slots
 *   alone reach ceil128(B*S)) the plan is the padded layout itself: row_start[b] = b*S, rows = ceil128(B*S).
 * The *_packed entry points are their namesakes with a plan (packing == NULL or packing->row_start == NULL: exactly the
 * namesake). row_start is a DEVICE pointer; a plan must come from plb_packing_plan for the same lengths, B and S (the
 * engine checks what it can see on the host: rows, used). Nothing in a packed call synchronises with the host: for a fixed
 * plan it is graph-capturable like the padded call. Same results as the padded call up to bf16 summation order in the
 * weight gradients (each valid row's arithmetic is unchanged). A call runs PADDED, with the padded call's results bit for
 * bit, when the plan is the padded layout (S < 128 included: such a batch has no plan that packs), when lengths == NULL,
 * while fp8 mode is on unless plb_set_packed_fp8 is on, for plb_forward_packed with token_logits (a full [B,S,NT] fp32
 * output is a debugging output, not a hot path) and for dual-head loss calls (token_ids given) unless plb_set_packed_dual
 * is on. plb_forward_packed: hidden / phoneme_logits at pad positions (s >= lengths[b]) are ZEROS (the padded path leaves
 * values there that nothing reads). plb_pooler takes the [B,S,H] output as before.
 * Rows of the packed axis that hold no token are given defined values in every call (zeros from the embeddings, computed
 * like padded rows inside a slot, a zeroed attention output and zero gradients in the tail), so a packed call does not
 * depend on what an earlier call left in the workspace.
 * plb_last_call_rows: rows = token rows the last plb_forward / plb_loss_* call executed, of = the B*S it stood for
 * (rows == of: the call ran padded). */
typedef struct {
  const int32_t* row_start;   /* device, int32 [B+1], from plb_packing_plan */
  int32_t rows;               /* rows the call executes (plb_packing_plan's *rows) */
  int32_t used;               /* rows covered by the samples' slots (plb_packing_plan's *used) */
} PlbPacking;
int plb_packing_plan(const int32_t* lengths, int32_t B, int32_t S, int32_t* row_start, int32_t* rows, int32_t* used);
int plb_forward_packed(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                       const PlbPacking* packing, float* hidden, float* phoneme_logits, float* token_logits, void* stream);
int plb_loss_fwd_bwd_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int32_t* lengths,
                            const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked, int32_t B, int32_t S,
                            const PlbPacking* packing, float* loss, void* stream);
int plb_loss_fwd_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                        const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked,
                        int32_t B, int32_t S, const PlbPacking* packing, float* loss, float* loss_parts, void* stream);
int plb_last_call_rows(const PlbEngine* e, int64_t* rows, int64_t* of);
/* Token-packed DUAL-HEAD loss calls (opt-in on top of the plan; off by default, engine state, no device state touched, a
 * live plb_encode stash stays live). Off: every call with token_ids runs padded, plan or not, as above. On: a dual-head
 * loss call that is given a plan that packs — plb_loss_fwd_bwd_dual_packed, plb_loss_fwd_packed with token_ids — runs the
 * encoder AND the token head on the plan's row axis: the head's three rows x num_tokens GEMMs, its weight-gradient GEMM and
 * the bf16 [rows][num_tokens] logit-gradient image shrink with the executed rows. Same results as the padded call up to
 * summation order: each valid row's forward arithmetic, token logit statistics and logit-gradient row are unchanged; the
 * token-loss sum and the weight / bias gradient sums run over another row set (rows that hold no token contribute exact
 * zeros in both layouts). plb_last_call_rows reports rows < of for such a call; plb_last_application_rows stays rows == of
 * (a dual-head call prunes nothing). Still padded with the switch on: fp8 mode unless plb_set_packed_fp8 is on as well,
 * S < 128 and plans that are the padded layout, lengths == NULL, and plb_forward_packed with token_logits.
 * plb_loss_fwd_bwd_dual_packed: plb_loss_fwd_bwd_dual with a plan; packing == NULL, or the switch off: exactly
 * plb_loss_fwd_bwd_dual. */
int plb_set_packed_dual(PlbEngine* e, int32_t on);
int plb_loss_fwd_bwd_dual_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                                 const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked,
                                 int32_t B, int32_t S, const PlbPacking* packing, float* loss, float* loss_parts, void* stream);
/* Token-packed calls IN FP8 MODE (opt-in on top of the plan; off by default, engine state, no device state touched, a live
 * plb_encode stash stays live). Off: every call made while fp8 mode is on runs padded, plan or not, as above. On: while
 * fp8 mode is on, a call that is given a plan that packs and lengths runs on the plan's rows — plb_forward_packed without
 * token_logits, plb_loss_fwd_bwd_packed, plb_loss_fwd_packed, and the dual-head forms (plb_loss_fwd_bwd_dual_packed,
 * plb_loss_fwd_packed with token_ids) when plb_set_packed_dual is on too — the calibration call(s), which compute in bf16,
 * and the fp8 calls alike. plb_last_call_rows reports rows < of, plb_last_application_rows what it reports for a bf16
 * packed call. plb_encode keeps refusing fp8 mode.
 * Site maxima: the per-site maxima a packed call in fp8 mode records are taken over the rows it executes — rows [0, used)
 *   in a calibration call, every row an image-writing launch covers in an fp8 call (the tail [used, rows) included) — the
 *   rest of a sample's slot included, just as pad rows count in a padded call: in fp8 mode those rows are embedded from
 *   ids like pad positions (a bf16 packed call writes zero embeddings there), so a packed call whose slots all have one
 *   size S' < S records the maxima, and gives the results, of the padded call on the batch trimmed to [B,S'] bit for bit.
 *   Delayed scaling, the four-call history and plb_fp8_stats are otherwise unchanged; a run may mix padded and packed
 *   calls, the history simply holds both.
 * Tile forms: which fp8 forms a call gets follows the rows it executes (fp8 pipeline tiles: rows % 128; LayerNorm in the
 *   GEMM epilogues: rows % 1024; gelu' stash; the fp8 weight-gradient GEMMs: layers x rows >= 8192). A packed call can
 *   therefore take the weight gradients from the bf16 tensors where the padded call of the same batch took them from the
 *   1-byte images.
 * Rows that hold no token have zeros in every gradient image and finite values in every activation image that depend on
 *   this call's inputs only, so a packed call in fp8 mode does not depend on what an earlier call left in the workspace.
 * Not graph-captured by anything in this library; fp8 fine-tuning (plb_encode) stays out of scope. */
int plb_set_packed_fp8(PlbEngine* e, int32_t on);
/* ---- differentiable encoder: fine-tuning a checkpoint inside a downstream model ----
 * Stands in for the reference README's "Finetuning" use (README.md:36-119):
 *   bert_dur = model.bert(texts, attention_mask=(~text_mask).int()).last_hidden_state   -> plb_encode
 *   ... the caller's own model and loss, its backward down to d(loss)/d(last_hidden_state) ...
 *   loss.backward()                                                                     -> plb_encode_bwd
 *   optimizer.step('bert')                                                              -> plb_adamw_step
 * plb_encode: the forward of a TRAINING engine that keeps every application's activations (nothing is pruned). hidden fp32
 *   [B,S,H] = .last_hidden_state: at valid positions bit-equal to what plb_forward[_packed] returns on the same engine; at
 *   pad positions (s >= lengths[b]) ZEROS, in the padded and the packed layout alike. This deviates from HuggingFace (and
 *   from the padded plb_forward), whose pad query rows hold values: a differentiable output must not hand a downstream
 *   model numbers that carry no gradient. packing may be NULL. Fails on an inference-only engine, and while fp8 mode is
 *   on: the gradient sites' delayed-scale history belongs to the pre-training loss and must not be mixed with the
 *   magnitudes of a foreign gradient (fp8 fine-tuning is out of scope; plb_set_fp8(e, 0, ...) first).
 * plb_encode_bwd: d_hidden fp32 [B,S,H] = d(loss)/d(hidden) from the caller; values at pad positions are ignored (never
 *   read: treated as zero). ids / lengths / B / S / packing as given to the plb_encode call whose stash is LIVE: the stash
 *   stops being live after any call that writes the workspace or moves the weights — plb_forward*, plb_loss_*, plb_encode,
 *   plb_encode_bwd itself (one backward per forward), plb_adamw_step, plb_sync_weights, plb_set_fp8,
 *   plb_broadcast_params. Without a live stash, or with another B, S or plan, the call fails with a text that says which,
 *   launches nothing and leaves the gradient buffer alone.
 *   Gradient buffer: the encoder range [0, offset of PLB_HEAD_W) is overwritten (not accumulated) as by a loss call; the
 *   phoneme head's range is written as ZEROS and the head — like the token head after a phoneme-only call, and like the pooler
 *   after every call but a plb_encode_bwd_pooled that was given a d_pooled (below) —
 *   is marked as having no gradient: the plb_adamw_step that follows updates [0, PLB_HEAD_W) only and leaves the head's
 *   parameters, both moments and bf16 copies bit-unchanged, as torch skips a parameter whose .grad is None. The head does
 *   NOT get a step count of its own: it keeps sharing the engine's (`step` of plb_adamw_step), so after k fine-tuning steps
 *   its next pre-training update is bias-corrected for step + k. The next plb_loss_fwd_bwd makes the head live again.
 *   Data-parallel runs: with a communicator and overlap on, the call issues the ten pieces of a regular step in the same
 *   order (the head piece carries its zeros, the status all-reduce sits behind it); overlap off: plb_allreduce_grads as
 *   before. plb_comm_pieces and plb_last_call_rows report for these calls too.
 *   A host that steps the parameters with an optimizer of its own (torch.optim.AdamW over the views) must check
 *   plb_poll_status itself: the device-side skip of a poisoned step lives in the fused optimizer entries (plb_adamw_step*,
 *   plb_lamb_step) only. */
int plb_encode(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing,
               float* hidden, void* stream);
int plb_encode_bwd(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing,
                   const float* d_hidden, void* stream);
/* ---- per-application outputs: output_hidden_states / output_attentions, with gradients (opt-in: a call that asks for
 * nothing launches what it launched before) ----
 * The shared layer is applied num_hidden_layers (L) times, so hidden_states[l] is the model after l applications: what depth
 * probing, weighted sums over depths and early exit read. Semantics follow HuggingFace modeling_albert.py with the deviations
 * this library already makes for plb_encode.
 * PlbLayerOutputs: two HOST arrays of DEVICE pointers, read on the host during the call (they need not outlive it).
 *   hidden_states: L + 1 entries, each NULL (not wanted) or fp32 [B,S,H]. hidden_states[0] is the output of
 *     embedding_hidden_mapping_in (H wide, not the embedding), hidden_states[l] the output of application l, hidden_states[L]
 *     is last_hidden_state. Values are the fp32 image of the bf16 rows the call itself computed: nothing is recomputed. At
 *     valid positions every slot is bit-equal between the padded and the packed layout, between plb_forward_layers and
 *     plb_encode_layers, and slot L to the `hidden` of the same call.
 *   attentions: L entries, each NULL or fp32 [B,NH,S,S]. attentions[l][b,h,i,j] = softmax over the keys j < lengths[b] of
 *     scale * q_i·k_j of application l, from the bf16 qkv that application wrote and the log-sum-exp its attention kernel
 *     stored: the probabilities the call's attention used, up to fp32 rounding. Key columns j >= lengths[b] are exactly 0.
 *   Pad positions (s >= lengths[b]): every hidden-state slot is ZERO there and every attention QUERY row i >= lengths[b] is
 *     ZERO, in both layouts. This deviates from HuggingFace, which leaves values in pad query rows: the same deviation, for
 *     the same reason, as plb_encode. lengths == NULL: no padding. Every element of every requested output is written
 *     exactly once by the call: the caller need not zero anything. Either array may be NULL (none of that kind).
 * plb_forward_layers: plb_forward_packed(hidden, no logits) plus the outputs; hidden may be NULL. Training and inference-only
 *   engines, padded or packed, bf16 or fp8 mode (the outputs are those of the arithmetic that call ran). Engine state
 *   afterwards is exactly that of the plb_forward_packed call: the final hidden state for plb_token_report,
 *   plb_last_call_rows, the fp8 scale update, the dropped plb_encode stash.
 * plb_encode_layers: plb_encode plus the outputs; with layers == NULL it is exactly plb_encode. Same refusals, same live
 *   stash, hidden required.
 * plb_encode_bwd_layers: plb_encode_bwd with gradients entering at the application boundaries too. d_below: HOST array of L
 *   DEVICE pointers; d_below[l] (l in [0, L)) is NULL (no gradient there) or fp32 [B,S,H] = d(loss)/d(hidden_states[l]); slot
 *   L's gradient is d_hidden, and a NULL d_hidden means a zero output gradient of the last application. Values at pad
 *   positions are never read. With d_below == NULL or all-NULL and d_hidden given it is exactly plb_encode_bwd: the same
 *   launches, the gradient buffer bit for bit. All of plb_encode_bwd's bookkeeping is unchanged (the stash is consumed, the
 *   head range is zeroed and marked without gradient, the exchange's pieces and the status exchange keep their order).
 *   Attentions are outputs only: no gradient enters through them.
 * Refusals, each before anything is launched and with a text: a NULL engine or one that is not bound, every refusal of the
 *   namesake call, and for plb_encode_bwd_layers nothing to differentiate (d_hidden == NULL and no entry of d_below). A
 *   `layers` whose arrays are both NULL, or hold NULL entries only, is no refusal: it is the namesake call. */
typedef struct {
  float* const* hidden_states;  /* HOST array of num_hidden_layers + 1 DEVICE pointers (each NULL = not wanted, else fp32 [B,S,H]); NULL = none */
  float* const* attentions;     /* HOST array of num_hidden_layers DEVICE pointers (each NULL = not wanted, else fp32 [B,NH,S,S]); NULL = none */
} PlbLayerOutputs;
int plb_forward_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing,
                       float* hidden, const PlbLayerOutputs* layers, void* stream);
int plb_encode_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing,
                      float* hidden, const PlbLayerOutputs* layers, void* stream);
int plb_encode_bwd_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                          const PlbPacking* packing, const float* d_hidden, const float* const* d_below, void* stream);
/* ---- embedding inputs: token_type_ids / position_ids / inputs_embeds, with gradients (opt-in: a call that passes none
 * launches what it launched before) ----
 * Semantics are HuggingFace AlbertEmbeddings.forward (modeling_albert.py:67-106) with dropout 0:
 *   LN_E( (inputs_embeds[b,s] | word[ids[b,s]]) + type[token_type_ids[b,s]] + pos[position_ids[b,s]] )
 * with the deviations this library already makes for plb_encode: zeros at pad positions, prefix masks (lengths), word row 0 is
 * the padding row and gets no gradient.
 * PlbEmbedInputs: three DEVICE pointers, each optional, each indexed by the padded [B,S] position in the padded and the packed
 *   layout alike (as ids are); values at pad positions are read by a padded call (as ids are there) and must be in range.
 *   token_type_ids NULL means row 0 for every token, position_ids NULL means s. Exactly one of ids and inputs_embeds is given;
 *   inputs_embeds is E = embedding_size wide (the input of the embedding LayerNorm), not hidden_size. The host validates the
 *   index ranges; an index outside its table reads row 0 on the device, never memory outside the table.
 * plb_forward_inputs / plb_encode_inputs / plb_encode_bwd_inputs: supersets of plb_forward_layers / plb_encode_layers /
 *   plb_encode_bwd_layers. With inputs == NULL, or its three pointers NULL, and d_inputs_embeds == NULL each is exactly its
 *   namesake: the same launches, bit-identical results, and the same engine state afterwards (plb_last_call_rows, the final
 *   hidden state for plb_token_report, the live stash, the exchange's pieces, the status exchange). With token_type_ids = 0 and
 *   position_ids = s passed explicitly the forward is bit-equal to the plain call's too (the same arithmetic per row).
 * plb_encode_bwd_inputs: `inputs` as given to the live plb_encode_inputs call (as ids are passed again). The encoder range of
 *   the gradient buffer is overwritten as by plb_encode_bwd. EVERY row of the token-type table receives its gradient (the sum
 *   over the tokens of that type; a plain call trains row 0 only), a position row the sum over the tokens whose position_id it
 *   is. No atomics: every sum has a fixed order and results are bitwise reproducible from run to run; a row that owns many
 *   tokens is summed in 512-token chunks by separate workgroups, the partial rows added in chunk order. With inputs_embeds the
 *   word table's range is written as ZEROS, and the fused optimizer entries (plb_adamw_step*, plb_lamb_step) see a zero
 *   gradient there: with weight decay the table still decays. A host that wants torch's "no gradient" for that tensor
 *   freezes it through the `frozen` plan of plb_adamw_step_groups / plb_lamb_step.
 *   d_inputs_embeds (or NULL): fp32 [B,S,E], the gradient of the pre-LayerNorm sum per token, in the padded layout, every
 *   element written exactly once, exact zeros at pad positions. Available whether the forward took ids (the per-phoneme
 *   saliency) or inputs_embeds (its gradient).
 * Refusals, each before anything is launched and with a text naming the cause: both or neither of ids / inputs_embeds; any of
 *   the three inputs or d_inputs_embeds while fp8 mode is on; every refusal of the namesake.
 * Out of scope: the inputs in the pre-training loss calls (plb_loss_*), fp8 mode, dropout. (Non-prefix attention masks: the
 *   plb_*_masked calls below.) */
typedef struct {
  const int64_t* token_type_ids;  /* device int64 [B,S] or NULL (all 0); values in [0, type_vocab_size) */
  const int64_t* position_ids;    /* device int64 [B,S] or NULL (s);     values in [0, max_position_embeddings) */
  const float*   inputs_embeds;   /* device fp32 [B,S,embedding_size] or NULL; given <=> ids == NULL */
} PlbEmbedInputs;
int plb_forward_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths, int32_t B, int32_t S,
                       const PlbPacking* packing, float* hidden, const PlbLayerOutputs* layers, void* stream);
int plb_encode_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths, int32_t B, int32_t S,
                      const PlbPacking* packing, float* hidden, const PlbLayerOutputs* layers, void* stream);
int plb_encode_bwd_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths, int32_t B,
                          int32_t S, const PlbPacking* packing, const float* d_hidden, const float* const* d_below,
                          float* d_inputs_embeds, void* stream);
/* ---- key masks: attention masks that are no prefix, with gradients (opt-in: a call that passes none launches what it
 * launched before) ----
 * key_mask: DEVICE int32 [B,S], nonzero = attend, indexed by the padded position in the padded and the packed layout alike.
 *   HuggingFace's 2-D key-padding rule: key j of sample b takes part in the softmax of EVERY query of b iff key_mask[b,j] != 0.
 *   `lengths` is the EXTENT of each sample, 1 + the last position whose key_mask is nonzero (NULL: S); bits at and past
 *   lengths[b] are ignored. Positions at and past the extent are pad positions exactly as in every other call: zeros in
 *   `hidden` / hidden_states / attentions, never read by the backward, skipped by token packing (the plan is made from the
 *   extents; holes stay inside their slot). A position below the extent whose key_mask is 0 is a HOLE: it is removed as a KEY
 *   only. It stays a query like any other — it attends to the valid keys, has a hidden state, receives and carries gradient
 *   (as in HuggingFace) — and attentions[l][b,h,i,j] is exactly 0 in its column j; rows i below the extent sum to 1.
 * plb_forward_masked / plb_encode_masked / plb_encode_bwd_masked: supersets of plb_forward_inputs / plb_encode_inputs /
 *   plb_encode_bwd_inputs. With key_mask == NULL each is exactly its namesake: the same launches, bit-identical results, the
 *   same engine state afterwards (plb_last_call_rows, the final hidden state for plb_token_report, the live stash, the
 *   exchange's pieces, the status exchange). With a key mask the call packs it into one bit per key in the workspace (one small
 *   launch) and every attention launch runs the masked instantiation of its kernel (plbert_kernels.h: PlbAttn.key_words); the
 *   backward then runs in the two-kernel form, whatever plb_set_attn_bwd_fused / PLBERT_ATTN_BWD say. A key mask that is a
 *   prefix of ones gives the results of the call without it bit for bit (the same arithmetic per row).
 * plb_encode_bwd_masked: key_mask as given to the live plb_encode_masked call (as ids and inputs are passed again).
 * A sample without a single nonzero key_mask entry below its length is the host's to reject: on the device its own rows are
 *   not finite; nothing outside the sample is affected and nothing outside its rows is read.
 * Refusals, each before anything is launched and with a text naming the cause: key_mask while fp8 mode is on; key_mask with
 *   S > 2048; plb_encode_bwd_masked with a key mask when the live forward had none, or without one when it had; every
 *   refusal of the namesake.
 * Out of scope: the pre-training loss calls (plb_loss_*), the logits of plb_forward, fp8 mode, 3-D / 4-D masks, dropout. */
int plb_forward_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                       const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing, float* hidden,
                       const PlbLayerOutputs* layers, void* stream);
int plb_encode_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                      const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing, float* hidden,
                      const PlbLayerOutputs* layers, void* stream);
int plb_encode_bwd_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                          const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing, const float* d_hidden,
                          const float* const* d_below, float* d_inputs_embeds, void* stream);
/* ---- differentiable pooler_output (opt-in: a call without d_pooled launches what it launched before) ----
 * pooled[b,:] = tanh(pooler.weight · h[b,0,:] + pooler.bias) (plb_pooler; modeling_albert.py:403), h the last hidden state;
 * position 0 is used whether or not a key mask makes it a hole. A sentence-level head on pooler_output trains the pooler and
 * the encoder through this call.
 * plb_encode_bwd_pooled: superset of plb_encode_bwd_masked. d_pooled (or NULL): fp32 [B,H] = d(loss)/d(pooled), 16-byte
 *   aligned. With d_pooled == NULL the call is exactly its namesake: the same launches, the gradient buffer bit for bit, the
 *   same engine state afterwards. With d_pooled the pooler backward runs first in the call, from the bf16 rows of the final
 *   hidden state the live stash holds and the fp32 parameters:
 *     y = pooled, recomputed with plb_pooler's arithmetic (its bits);  dpre = d_pooled * (1 - y*y)
 *     d(pooler.weight) = sum_b dpre[b,:]^T h[b,0,:]    d(pooler.bias) = sum_b dpre[b,:]    dh0[b,:] = dpre[b,:] · pooler.weight
 *   all in fp32, every sum in a fixed order without atomics (bitwise reproducible from run to run). The pooler's range of the
 *   gradient buffer is overwritten, and the output gradient of the last application at position 0 of sample b becomes
 *   bf16(d_hidden[b,0,:] + dh0[b,:]) (one fp32 add, one round to nearest even; d_hidden == NULL: a zero addend, every other
 *   row zero). Nothing else in the backward changes. "Nothing to differentiate" means that d_hidden, d_below and d_pooled are
 *   all absent.
 *   The pooler is then marked as having a gradient, by the scheme of the phoneme head: every optimizer and norm entry
 *   (plb_adamw_step, _clipped, _groups, plb_adamw_plan, plb_lamb_plan, plb_lamb_step, plb_grad_norm, plb_grad_norm_groups)
 *   covers [PLB_POOL_W, end of PLB_POOL_B) with one more launch, with the engine's step count (the pooler has none of its own);
 *   groups and `frozen` apply to the two tensors as to any other. The mark is cleared by every later backward call: a loss
 *   call, or a plb_encode_bwd* call without d_pooled, leaves the pooler without gradient and its parameters, moments and bf16
 *   copy bit-unchanged by the step that follows.
 *   plb_grad_accum_add carries the pooler through a window like the phoneme head (live after the LAST add iff a micro-step of
 *   the window produced it). A window that would hold both the token head's and the pooler's gradients is refused before
 *   anything is launched: in a norm buffer the two share one set of partial sums.
 *   Data-parallel runs: the pooler range lies right behind the phoneme head's; when it is live the head piece of the overlapped
 *   exchange, and the first collective of plb_allreduce_grads, reach to its end. The number and order of collectives stay as
 *   they are; plb_comm_pieces reports the grown float count.
 * Refusals, each before anything is launched and with a text: nothing to differentiate; a d_pooled that is not 16-byte
 *   aligned; every refusal of the namesake (no live stash, another B, S, plan or key mask, fp8 mode through plb_encode).
 * Out of scope: the pre-training loss calls, fp8 mode, dropout, a pooler step count of its own. */
int plb_encode_bwd_pooled(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                          const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing, const float* d_hidden,
                          const float* const* d_below, float* d_inputs_embeds, const float* d_pooled, void* stream);
/* ---- masked-phoneme evaluation: accuracy, top-k and fill-mask from a loss call (opt-in: a step that does not ask launches
 * what it launched before) ----
 * The reference reports the scalar loss only (train.py:288-336, 395-410). A masked LM's users also expect the accuracy at the
 * masked positions, the per-sample losses behind the scalar and the model's predictions at chosen positions ("fill-mask").
 * Every loss call leaves the fp32 logits of exactly its masked rows on the device; plb_masked_report reads them there.
 * plb_masked_report reports on the LAST plb_loss_* call of this engine — plb_loss_fwd_bwd, plb_loss_fwd_bwd_packed,
 *   plb_loss_fwd_bwd_dual, plb_loss_fwd_bwd_dual_packed, plb_loss_fwd, plb_loss_fwd_packed: training or loss-only, padded or
 *   packed, pruned or not, bf16 or fp8, phoneme-only or dual-head, on a training or an inference-only engine. The report is
 *   available from that call's return until the next plb_loss_* call replaces it (one that fails after its first launch
 *   leaves none) or plb_bind rebinds the buffers. Every other entry point leaves it available and unchanged — plb_adamw_step[_clipped],
 *   plb_grad_accum_add, plb_grad_norm, plb_allreduce_grads, plb_status*, plb_sync_weights, plb_set_fp8, plb_forward*,
 *   plb_encode, plb_encode_bwd — so a training loop may ask after its optimizer step.
 *   idx_offsets (device, int32 [B+1]) and B as given to that loss call; rows are in the CSR order of its index lists.
 *   Every pointer of PlbMaskedReport is optional (NULL = not wanted) and names DEVICE memory of the caller:
 *     with the classes of a row ordered by (logit descending, class index ascending — among equal logits the LOWEST index
 *     wins): pred = the first class; rank = the 0-based position of the label in that order (pred == label iff rank == 0, the
 *     label is in the top-k list iff rank < topk); topk_ids / topk_logprob = the first topk classes and their log-softmax
 *     (fp32), 0 <= topk <= 8, entries past num_phonemes: id -1, -inf; nll = -log_softmax at the label, the very value the
 *     loss call summed; logits = the rows' logits [n_masked][num_phonemes]. A row with a NaN logit: pred -1, rank
 *     num_phonemes, nll NaN, ids -1, logprobs NaN — never counted correct.
 *     sample_loss [B] = mean nll of the sample's rows (0 without rows): the mean of these over the samples that have rows IS
 *     the phoneme loss the call returned, up to fp32 summation order. sample_top1 / sample_topk [B] = the sample's rows with
 *     rank == 0 / rank < topk. totals [4] = {rows, top-1 correct, top-k correct, samples that have rows}.
 *     token_totals [2] (after a dual-head call only) = {valid positions, positions whose target logit EQUALS the row maximum
 *     of the token head}: top-1 only, and TIE-INCLUSIVE (a target that ties for the maximum counts), because the fused token
 *     head keeps per-tile maxima but no arg-max index. Predicted token ids, exact (lowest-index) accuracy and top-k of the
 *     token head: plb_token_report below.
 *   Fails before anything is launched, with a text: no loss call has run; B differs from that call's; token_totals after a
 *   phoneme-only call; topk outside [0, 8]; a sample output or totals wanted with idx_offsets == NULL.
 *   A call with n_masked == 0 reports zeros (sample outputs, totals) and writes no row output.
 *   The call writes the caller's buffers and scratch regions of its own inside the workspace that no other entry point
 *   touches: it changes no engine state, does not drop a live plb_encode stash, leaves the health word alone, and the next
 *   call computes what it would have computed without it. Nothing is read back; bitwise reproducible (no atomics).
 *   HEALTH WORD: after a hand-off time-out (plb_status) the logits are whatever the poisoned call left; the report does not
 *   look at the word, which stays the authority — read the report wherever the loss is read, behind the same check.
 *   DATA-PARALLEL RUNS: counts are per rank; a host that wants global accuracy sums totals over the ranks itself. */
typedef struct {
  int32_t* pred; int32_t* rank; float* nll;                         /* [n_masked], CSR order of the call's index lists */
  int32_t* topk_ids; float* topk_logprob;                           /* [n_masked][topk] */
  float* logits;                                                    /* [n_masked][num_phonemes] */
  float* sample_loss; int32_t* sample_top1; int32_t* sample_topk;   /* [B] */
  int32_t* totals;                                                  /* [4] */
  int32_t* token_totals;                                            /* [2]; dual-head calls only */
} PlbMaskedReport;
int plb_masked_report(PlbEngine* e, const int32_t* idx_offsets, int32_t B, int32_t topk, const PlbMaskedReport* out,
                      void* stream);
/* ---- token-head predictions without logits (the reference has no counterpart: its loop reports the scalar loss only) ------
 * What the token (grapheme) head predicts at chosen positions: the best topk classes with their log-probabilities, the
 * log-sum-exp, the target's log-probability and its position in the list, exact counts — from one fused GEMM + top-k pass
 * over the vocabulary that never stores a logit (plb_forward's token_logits is a full fp32 [B,S,num_tokens] array: 4.2 GB at
 * 32 x 512 x 64000).
 * WHAT IT REPORTS ON: the final hidden state of the LAST call of this engine that ran the encoder on every row and left it
 *   in the workspace — plb_forward / plb_forward_packed, plb_encode, and plb_loss_fwd* / plb_loss_fwd_bwd* unless the call
 *   pruned its last application (a phoneme-only loss call whose masked rows are less than half of the batch; a dual-head
 *   call never prunes) — padded or packed, bf16 or fp8, training or inference-only engine; multiplied by the bf16 compute
 *   copy of token_predictor.weight as that call saw it, plus the fp32 bias.
 * UNTIL WHEN: the next call that runs the encoder replaces the state. A call that moves the weights ends it —
 *   plb_adamw_step[_clipped], plb_sync_weights, plb_broadcast_params: a report behind the update would multiply old hidden
 *   rows by new weights, so a training loop asks BETWEEN the loss call and the optimizer step — and so does plb_bind.
 *   plb_encode_bwd, plb_masked_report, plb_grad_*, plb_allreduce_grads, plb_status*, plb_set_fp8 leave it alone.
 * ROWS: the CSR position lists of the loss calls — idx_offsets (device, int32 [B+1]) and idx_flat (int32 [n], positions
 *   < lengths[b]) — or idx_offsets == NULL: every position in [B,S] order, n == B*S; a position s >= lengths[b] then has NO
 *   ROW (ids -1, log-probs -inf, lse / target_logprob NaN, target_pos -1, logits 0; never counted). lengths (NULL: no
 *   padding), B, S and packing as given to the call reported on, as plb_encode_bwd asks for them.
 * OUTPUTS: every pointer of PlbTokenReport is optional and names DEVICE memory of the caller. Classes are ordered by (logit
 *   descending, class index ascending): topk_ids / topk_logprob = the first topk classes and their log-softmax (fp32),
 *   0 <= topk <= 8, entries past num_tokens: id -1, -inf; lse = the row's log-sum-exp; with token_ids (device, int64 [B,S],
 *   read at the reported positions only): target_logprob = log-softmax at the target (minus the mean over samples of the mean
 *   over valid positions of it IS the token loss of a dual-head call, up to fp32 summation order), target_pos = the 0-based
 *   position of the target in the list, -1 when it is not among the first topk; totals [3] = {rows counted, rows with
 *   target_pos == 0 (exact top-1: the lowest index wins a tie, unlike token_totals), rows with target_pos >= 0 (top-k)};
 *   logits [n][num_tokens] = the kernel's own fp32 values, for small n and debugging. A row with a NaN (or +inf) logit: ids
 *   -1, log-probs, lse and target_logprob NaN, target_pos -1; counted as a row, never as a hit.
 * REFUSALS, each before anything is launched, with a text: engine not bound; num_tokens == 0; no qualifying call since
 *   plb_bind (or the last one failed, or had nothing to run); the call pruned; the weights moved since; another B / S / plan;
 *   topk outside [0, 8]; target_logprob, target_pos or totals wanted without token_ids; n < 0, n larger than B*S, or
 *   idx_offsets == NULL with n != B*S. n == 0 is no refusal: totals are zeros and no row output is written.
 * SIDE EFFECTS: none. The call writes the caller's buffers and scratch regions of its own inside the workspace (at most
 *   2 KiB per row of the engine's capacity, independent of num_tokens; none when num_tokens == 0): it changes no engine
 *   state, keeps a live plb_encode stash live, leaves the health word and plb_masked_report's regions alone, runs on the
 *   caller's stream only and reads nothing back. No atomics: bitwise reproducible.
 * HEALTH WORD and DATA-PARALLEL RUNS: as for plb_masked_report. */
typedef struct {
  int32_t* topk_ids; float* topk_logprob;        /* [n][topk] */
  float* lse;                                    /* [n] */
  float* target_logprob; int32_t* target_pos;    /* [n]; need token_ids */
  float* logits;                                 /* [n][num_tokens]; small n / debugging */
  int32_t* totals;                               /* [3] = {rows counted, target_pos == 0, target_pos >= 0}; need token_ids */
} PlbTokenReport;
int plb_token_report(PlbEngine* e, const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n,
                     int32_t B, int32_t S, const PlbPacking* packing, const int64_t* token_ids, int32_t topk,
                     const PlbTokenReport* out, void* stream);
/* What the last training step exchanged: the number of collectives it issued (10 pieces for the reference's phoneme-only
 * step with overlap on, 1 with overlap off; one more after a dual-head step) and the floats they covered. The reference
 * has no counterpart (DDP's bucket count is internal to torch, train.py:218-221); a caller logs it to see which form of
 * the exchange actually ran. */
int plb_comm_pieces(const PlbEngine* e, int32_t* collectives, int64_t* floats);
/* DDP's start-up broadcast of rank `root`'s parameters; refreshes the bf16 copies. */
int plb_broadcast_params(PlbEngine* e, int32_t root, void* stream);
/* overlap = 1 (default): plb_loss_fwd_bwd[_dual] itself issues the gradient all-reduce, in contiguous pieces of the
 * flat buffer on the engine's communication stream as each piece becomes final (head gradients at the start of the
 * backward; the shared layer's weight gradients one by one, each while the next weight-gradient GEMM runs), and
 * plb_allreduce_grads only joins it. overlap = 0: plb_allreduce_grads performs ONE all-reduce in `stream`. */
int plb_set_grad_overlap(PlbEngine* e, int32_t overlap);
/* Sum all-reduce of every gradient the last loss call produced (the trainable range; plus the token head after a
 * dual-head step) over the ranks of the communicator; plb_adamw_step's grad_scale = 1/world turns it into DDP's mean.
 * After the call returns the reduced gradients are ordered before later work on `stream`. No communicator: no-op. */
int plb_allreduce_grads(PlbEngine* e, void* stream);

/* Bit-exact application of the reference's word-level masking (dataloader.py:59-137) on the device. The HOST draws the
 * reference's random streams in the reference's order (plbert_amd/data.py: MaskedPhonemeDataset.decisions) and hands
 * over, per sample, the UNCROPPED phoneme ids with a separator after each word, the word boundaries and one decision
 * per word; the device writes labels / masked ids (cropped to max_seq_length at crop_start, zero padded to S — the
 * collater's pad, dataloader.py:276-297) and the masked index list re-based to the crop (CSR), exactly as
 * __getitem__ + the collater produce them. Integer work only: results are bit-identical to the reference's.
 *   ids int64 [n_total]: all samples' uncropped ids back to back; sample_off int32 [B+1]: offsets into ids;
 *   word_off int32 [B+1]: offsets into word_begin / word_len / action / word_token (one entry per word: first position
 *   inside the sample, phoneme count, action 0 keep | 1 mask | 2 replace, grapheme-token id);
 *   repl int64 [n_total]: replacement ids (read at the positions of action-2 words); crop_start int32 [B];
 *   word_token + tokens (both NULL, or both given): the 4-tuple Collater's token_ids row, every phoneme of a word
 *   carrying the word's token id and separators sep_token (dataloader.py:66-71).
 * Outputs: labels / masked / tokens int64 [B,S]; lengths_out int32 [B] = min(len, S); idx_offsets int32 [B+1];
 * idx_flat int32 [capacity B*S]; scratch int32 [B + B*S]. S <= 1024, B <= 1024. */
int plb_apply_mask(const int64_t* ids, const int32_t* sample_off, const int32_t* word_off, const int32_t* word_begin,
                   const int32_t* word_len, const int8_t* action, const int64_t* repl, const int64_t* word_token,
                   int64_t sep_token, const int32_t* crop_start, int32_t B, int32_t S, int32_t mask_id, int64_t* labels,
                   int64_t* masked, int64_t* tokens, int32_t* lengths_out, int32_t* idx_offsets, int32_t* idx_flat,
                   int32_t* scratch, void* stream);

/* Device-side fast mode of the word-level masking that MaskedPhonemeDataset does on the host
 * (dataloader.py:83-108): same decision tree and probabilities (select a word with word_pred_prob;
 * then mask with phoneme_mask_prob / replace from the sample's own phonemes with replace_prob / keep),
 * separators never masked or indexed, but counter-based Philox randomness keyed by (seed, step, sample,
 * word) instead of the reference's global NumPy/Python streams — distribution-matched, NOT bit-exact
 * (the bit-exact path is the host one in plbert_amd/data.py). Needs no engine.
 * labels int64 [B,S] (separator id sep_id between words, positions >= lengths[b] ignored); outputs:
 * masked int64 [B,S], idx_offsets int32 [B+1], idx_flat int32 [up to B*S], scratch int32 [B + B*S].
 * S <= 512, B <= 1024. The total count is idx_offsets[B] (read it back before plb_loss_fwd_bwd). */
int plb_mask_batch(const int64_t* labels, const int32_t* lengths, int32_t B, int32_t S, uint64_t seed, uint32_t step,
                   float word_pred_prob, float phoneme_mask_prob, float replace_prob, int32_t mask_id, int32_t sep_id,
                   int64_t* masked, int32_t* idx_offsets, int32_t* idx_flat, int32_t* scratch, void* stream);

/* Measurement aid (no reference counterpart; the reference has no profiling): when
 * enabled, every kernel launch is bracketed by two HIP events on its stream. plb_profile_read waits
 * for them and returns, per kernel class, total milliseconds, launch count and the algorithmic
 * flops / bytes of those launches (arrays of plb_profile_num_classes() entries), then clears. */
void plb_profile_enable(int on);
int plb_profile_num_classes(void);
const char* plb_profile_class_name(int cls);
int plb_profile_read(double* ms, int64_t* launches, double* flops, double* bytes);

/* ---- test and tuning hooks (exported by the same library; NOT part of the drop-in surface, no reference counterpart).
 * They change process-wide state of the launchers and exist for tests/ and tools/ only:
 *   plb_debug_skip_piece(i)       the next loss call leaves out its i-th all-reduce piece, as a forgotten tensor would;
 *                                 the call must fail ("gradient exchange covered ..."), tests/test_gpu_comm_fake_rccl.py
 *   plb_debug_ln_fault(mode, n)   the next n fused LayerNorm launches run with a broken hand-off (1: one column tile
 *                                 never publishes; 2: consumed granules stay tagged), tests/test_gpu_handoff_fault.py
 *   plb_debug_hb_audit(e, on, k)  happens-before audit of the backward's three streams: a host-side
 *                                 vector-clock model of every event record / stream wait the engine issues, checked
 *                                 against the cross-stream buffer accesses of each launch; a violation fails the loss
 *                                 call. k >= 0: the MODEL forgets the k-th wait of the next call (the audit must then
 *                                 report it; the HIP call is still made). Also PLBERT_HB_AUDIT=1. plb_debug_hb_report
 *                                 returns the checks made, the violations and the first one's text.
 *   plb_comm_trace / plb_comm_trace_read
 *                                 timing events around every all-reduce piece of the last loss call: when the piece was
 *                                 released, when its collective had finished, begin / end of the weight-gradient tail
 *                                 (bench.py --gpus N prints them: RCCL-vs-GEMM contention readable from one line)
 *   plb_set_gemm_nt_tile / plb_set_gemm_nt_prefetch / plb_set_attn_bwd_fused
 *                                 force a tile, a K-loop form or the attention-backward form for the launches that
 *                                 follow (0 / -1 / -1 restore the per-shape policy; attention backward: 1 single-kernel
 *                                 form, 0 two kernels, 2 policy + split by sample), tests/test_gpu_kernels.py, tools/
 *                                 plb_set_gemm_nt_tile(64 / -64): the kernel is still picked per shape, and every / no
 *                                 launch that goes to the small NT kernel takes its 64x64 form (0: the shape rule of
 *                                 csrc/gemm.hip decides; 128 forces the small kernel in its 128x128 form). The environment
 *                                 variable PLBERT_NT_SMALL_TILE=128|64, read once per process, does the same for a whole
 *                                 run (tools/step_ab.py); the setter's 64 / -64 / 128 go before it. Results are equal bit
 *                                 for bit in both forms, tests/test_gpu_gemm_small_tile.py */
void plb_debug_skip_piece(int index);
void plb_debug_ln_fault(int mode, int launches);
int plb_debug_hb_audit(PlbEngine* e, int32_t on, int32_t break_wait);
int plb_debug_hb_report(const PlbEngine* e, int64_t* checks, int32_t* violations, char* first, int32_t first_bytes);
int plb_comm_trace(PlbEngine* e, int32_t on);
int plb_comm_trace_read(PlbEngine* e, int32_t max_pieces, int32_t* n, int64_t* begin, int64_t* end, float* released_ms,
                        float* done_ms, float* tail_ms);
void plb_set_gemm_nt_tile(int tile);
void plb_set_gemm_nt_prefetch(int on);
void plb_set_attn_bwd_fused(int on);
/* 0: every loss call evaluates every row of the last application (plb_last_application_rows), 1: masked rows only where
 * the call qualifies, -1: PLBERT_PRUNE_LAST's choice (default on). tests/test_gpu_engine.py compares the two. */
void plb_set_prune_last(int on);

#ifdef __cplusplus
}
#endif
#endif /* PLBERT_H */
