// Call-level stages of the engine: row selection of a padded or token-packed call, the heads, the stages of a loss call and
// the two-stream tail of its backward, and the entry points plb_forward*, plb_loss_*, plb_encode, plb_encode_bwd and their
// *_layers forms (per-application outputs; a gradient at every application boundary), *_inputs forms (token_type_ids /
// position_ids / inputs_embeds) and *_masked forms (key masks). Every entry point is one statement that names itself and fills
// the arguments of its family's implementation (EncArgs; loss_impl's in place); the implementation builds ONE Call
// (engine_internal.h) behind its refusals, and every stage below — run_encoder, token_head, encoder_bwd, the backward tail —
// takes that and nothing else about the call. Only
// writer of the encode stash (stash_*: every unit ends its life through drop_stash), pruned_rows, last_app_rows,
// last_exec_rows, tok_grads_live, head_grads_live and pool_grads_live (which a LAST add of engine_optim.cpp replaces by its
// window's union),
// and of what plb_masked_report reads (rep_*: engine_eval.cpp; plb_bind clears rep_valid) and of the record of the final
// hidden state plb_token_report reads (fin_*: note_final here; ended through drop_final by the calls that move the weights).
// (packed_dual, packed_fp8: plb_set_packed_dual / _fp8, engine.cpp.)
#include "engine_internal.h"

// Every call that writes the workspace or moves the weights ends the life of a plb_encode stash.
void drop_stash(PlbEngine* e, const char* by) {
  if (e && e->stash_live) { e->stash_live = false; e->stash_dead_by = by; }
}

// plb_token_report (engine_eval.cpp) reads the final hidden state of the last call that ran the encoder on every row.
void drop_final(PlbEngine* e, const char* by) {
  if (e) { e->fin_live = false; e->fin_dead_by = by; }
}
static void note_final(PlbEngine* e, const bf16_t* x, const Call& c) {
  e->fin_live = true; e->fin_x = x; e->fin_B = c.B; e->fin_S = c.S;
  e->fin_rows = c.rw.Tp; e->fin_used = c.rw.T; e->fin_row_start = c.rw.row_start;
}

static int check_shape(const PlbEngine* e, int B, int S, const char* who) {
  if (!e || !e->ws) return fail("%s: engine not bound", who);
  if (B < 1 || S < 1 || B > e->c.max_batch || S > e->c.max_seq || (int64_t)B * S > (int64_t)e->c.max_batch * e->c.max_seq)
    return fail("%s: batch %d x seq %d exceeds the engine capacity %d x %d", who, B, S, e->c.max_batch, e->c.max_seq);
  return 0;
}

static Rows padded_rows(int B, int S) { return Rows{nullptr, B * S, rup(B * S, 128)}; }
// Does this call run packed? It runs padded — same results as without a plan — when the plan saves nothing (every
// sample full, or slots that add up to the padded rows), while fp8 mode is on and plb_set_packed_fp8 is off, and when the
// caller says so (`padded`: a forward call that returns token logits, a dual-head loss call while plb_set_packed_dual is
// off, plb_encode_bwd never gets here in fp8 mode).
static int pick_rows(PlbEngine* e, const PlbPacking* pk, const int32_t* lengths, bool padded, int B, int S, const char* who,
                     Rows* out) {
  *out = padded_rows(B, S);
  e->last_exec_rows[0] = e->last_exec_rows[1] = (int64_t)B * S;
  if (!pk || !pk->row_start) return 0;
  if (pk->rows < 128 || pk->rows % 128 || pk->used < 1 || pk->used > pk->rows)
    return fail("%s: packing plan of %d rows (%d used) is not one plb_packing_plan made", who, pk->rows, pk->used);
  if (pk->rows > out->Tp) return fail("%s: packing plan of %d rows exceeds the call's %lld", who, pk->rows, (long long)out->Tp);
  if (!lengths || padded || (e->fp8_on && !e->packed_fp8) || pk->rows == out->Tp) return 0;   // (rows == Tp: the plan is the padded layout)
  if (pk->used % 128) return fail("%s: packing plan with %d used rows: slots are multiples of 128", who, pk->used);
  *out = Rows{pk->row_start, pk->used, pk->rows};
  e->last_exec_rows[0] = pk->rows;
  return 0;
}

// The embedding inputs of a plb_*_inputs call (in: the caller's struct or null; d_ie: where a backward puts the gradient of the
// pre-LayerNorm sum, or null), checked before anything is launched. Nothing given: *ec is a plain call's and only the namesake's
// own refusal (ids is null) applies.
static int embed_call(const PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* in, float* d_ie, const char* who, EmbedCall* ec) {
  memset(ec, 0, sizeof(*ec));
  if (in) ec->in = *in;
  ec->d_inputs_embeds = d_ie;
  if (ids && ec->in.inputs_embeds) return fail("%s: both ids and inputs_embeds are given (exactly one of them feeds the embeddings)", who);
  if (!ids && !ec->in.inputs_embeds)
    return ec->any() ? fail("%s: neither ids nor inputs_embeds is given (exactly one of them feeds the embeddings)", who)
                     : fail("%s: ids is null", who);
  if (ec->any() && e->fp8_on)
    return fail("%s: fp8 mode is on: token_type_ids / position_ids / inputs_embeds / d_inputs_embeds are bf16-mode inputs (plb_set_fp8(e, 0, stream) first)", who);
  return 0;
}

// The key mask of a plb_*_masked call (int32 [B,S] on the device, or null: nothing to check), refused before anything is launched.
static int key_mask_check(const PlbEngine* e, const int32_t* key_mask, int S, const char* who) {
  if (!key_mask) return 0;
  if (e->fp8_on)
    return fail("%s: fp8 mode is on: key_mask is a bf16-mode input (plb_set_fp8(e, 0, stream) first)", who);
  if (S > 2048) return fail("%s: key_mask with seq %d: the masked attention kernels take S <= 2048", who, S);
  return 0;
}
// ... and packed into the words the attention launches of the call read (key_mask.hip), first launch of the call
static int key_mask_words(PlbEngine* e, const int32_t* key_mask, Call* c) {
  if (!key_mask) return 0;
  uint32_t* const words = e->at<uint32_t>(e->o_keywords);
  const int ldkw = 2 * ((c->S + 63) / 64);
  HB_W(c->s, words, (int64_t)c->B * ldkw * 4, "key-mask words of the call");
  TRY(plb_launch_key_mask_words(key_mask, c->lengths, c->B, c->S, words, ldkw, c->s));
  c->rw.key_words = words; c->rw.ldkw = ldkw;
  return 0;
}

// What a plb_forward* / plb_encode* / plb_encode_bwd* entry point was given beside its outputs (null: not given, or a rung
// below the one that takes it). inputs: the embedding inputs of plb_*_inputs; key_mask: the key mask of plb_*_masked; layers:
// the per-application outputs of plb_*_layers, written by run_encoder as the call goes.
struct EncArgs {
  const int64_t* ids; const PlbEmbedInputs* inputs; const int32_t* key_mask; const int32_t* lengths;
  int32_t B, S;
  const PlbPacking* packing; const PlbLayerOutputs* layers; void* stream;
};

static int forward_impl(PlbEngine* e, const char* who, const EncArgs& a, float* hidden, float* phoneme_logits,
                        float* token_logits) {
  if (check_shape(e, a.B, a.S, who)) return 1;
  drop_stash(e, "plb_forward rewrote the workspace since");
  drop_final(e, "the last call that ran the encoder (plb_forward) failed");
  EmbedCall ec;
  if (embed_call(e, a.ids, a.inputs, nullptr, who, &ec)) return 1;
  if (key_mask_check(e, a.key_mask, a.S, who)) return 1;
  if (token_logits && !e->NT) return fail("%s: token_logits requested but num_tokens = 0", who);
  const int H = e->H;
  Rows rw;
  // (token logits: a full [B,S,NT] fp32 output is a debugging output and runs padded, whatever plb_set_packed_dual says.
  // Phoneme logits of a packed call pass, as [Tp][NP] fp32, through a slot
  // of the forward-only call that is free once the encoder is done: QKV (6H bytes per row) or the FFN's u (2I))
  const int64_t lg_off = 4 * e->NP <= 6 * H ? e->o_qkv : 4 * e->NP <= 2 * e->I ? e->o_u : -1;
  if (pick_rows(e, a.packing, a.lengths, token_logits != nullptr || lg_off < 0, a.B, a.S, who, &rw)) return 1;
  Call c = {who, a.ids, a.lengths, a.B, a.S, rw, ec, a.layers, (hipStream_t)a.stream};
  hipStream_t s = c.s;
  const int T = rw.T;
  const int64_t Tp = rw.Tp;
  bf16_t* x = nullptr;
  if (key_mask_words(e, a.key_mask, &c)) return 1;
  if (run_encoder(e, c, false, &x, nullptr)) return 1;
  // packed: back to the caller's [B,S,*] layout, zeros at the pad positions (by row_start, not by lengths: a padded call
  // leaves values at the pad positions of hidden)
  if (hidden) {
    if (rw.row_start) TRY(plb_launch_unpack_rows(x, 1, H, rw.row_start, a.lengths, a.B, a.S, H, hidden, s));
    else TRY(plb_launch_bf16_to_f32(x, H, hidden, H, T, H, s));
  }
  if (phoneme_logits) {
    float* const lg = rw.row_start ? e->at<float>(lg_off) : phoneme_logits;
    PlbGemmNT g = nt_desc(x, e->wbf(PLB_HEAD_W), Tp, e->NP, H);
    g.Mstore = T; g.bias = e->par(PLB_HEAD_B); g.Cf = lg; g.ldcf = e->NP;
    TRY(plb_launch_gemm_nt(&g, 0, 1, s));
    if (rw.row_start) TRY(plb_launch_unpack_rows(lg, 0, e->NP, rw.row_start, a.lengths, a.B, a.S, e->NP, phoneme_logits, s));
  }
  if (token_logits) {
    PlbGemmNT g = nt_desc(x, e->wbf(PLB_TOK_W), Tp, e->NT, H);
    g.Mstore = T; g.bias = e->par(PLB_TOK_B); g.Cf = token_logits; g.ldcf = e->NT;
    TRY(plb_launch_gemm_nt(&g, 0, 1, s));
  }
  if (e->fp8_on) {
    TRY(fp8_update_scales(e, s));
    e->fp8_ready = true;
  }
  TRY(plb_launch_step_status(e->at<unsigned int>(e->o_lnerr), nullptr, e->host_err_dev, nullptr, s));
  note_final(e, x, c);
  return 0;
}
extern "C" int plb_forward(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S, float* hidden,
                           float* phoneme_logits, float* token_logits, void* stream) {
  return forward_impl(e, "plb_forward", {ids, nullptr, nullptr, lengths, B, S, nullptr, nullptr, stream}, hidden, phoneme_logits,
                      token_logits);
}
extern "C" int plb_forward_packed(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                                  const PlbPacking* packing, float* hidden, float* phoneme_logits, float* token_logits,
                                  void* stream) {
  return forward_impl(e, "plb_forward", {ids, nullptr, nullptr, lengths, B, S, packing, nullptr, stream}, hidden, phoneme_logits,
                      token_logits);
}
// plb_forward_packed(hidden, no logits) plus the per-application outputs (include/plbert.h: PlbLayerOutputs)
extern "C" int plb_forward_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                                  const PlbPacking* packing, float* hidden, const PlbLayerOutputs* layers, void* stream) {
  return forward_impl(e, "plb_forward_layers", {ids, nullptr, nullptr, lengths, B, S, packing, layers, stream}, hidden, nullptr,
                      nullptr);
}
// plb_forward_layers with the embedding inputs (include/plbert.h: PlbEmbedInputs); none given: that call
extern "C" int plb_forward_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths, int32_t B,
                                  int32_t S, const PlbPacking* packing, float* hidden, const PlbLayerOutputs* layers, void* stream) {
  return forward_impl(e, "plb_forward_inputs", {ids, inputs, nullptr, lengths, B, S, packing, layers, stream}, hidden, nullptr,
                      nullptr);
}
// plb_forward_inputs with a key mask (include/plbert.h); key_mask == NULL: that call
extern "C" int plb_forward_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                                  const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* packing, float* hidden,
                                  const PlbLayerOutputs* layers, void* stream) {
  return forward_impl(e, key_mask ? "plb_forward_masked" : "plb_forward_inputs",
                      {ids, inputs, key_mask, lengths, B, S, packing, layers, stream}, hidden, nullptr, nullptr);
}

// ---- stages of a loss call ----------------------------------------------------------------------------------------------
// Bookkeeping at the start of a training call.
static int begin_training_call(PlbEngine* e, bool dual, hipStream_t s) {
  // All-reduce pieces of a PREVIOUS backward that nobody joined (two plb_loss_fwd_bwd calls with no plb_allreduce_grads /
  // plb_adamw_step between them: gradient probing, a caller that skips a step on a bad loss) still read and write the
  // gradient buffer on the communication stream: this call's kernels must not touch it before they have finished.
  if (join_comm(e, s)) return 1;
  e->tok_grads_live = dual;
  e->head_grads_live = true;
  e->pool_grads_live = false;   // (only plb_encode_bwd_pooled with a d_pooled sets it, behind this)
  e->grads_reduced = false;
  e->grads_fresh = true;   // (plb_grad_accum_add: these gradients have not been added yet; partials of older ones are void)
  e->norm_nparts = 0;
  e->piece_floats = 0;
  e->piece_count = 0;
  e->status_collectives = 0;
  if (e->hb.on) {
    // this call's first launches on the caller's stream may touch any byte of the workspace and the gradient buffer:
    // whatever the previous call left running on the side / communication stream must be ordered before them
    HB_W(s, e->ws, e->ws_bytes, "start of a loss call (whole workspace)");
    HB_W(s, e->grads, e->ptotal * 4, "start of a loss call (gradient buffer)");
    if (e->hb.violations) return fail("happens-before audit: %s", e->hb.first.c_str());
    e->hb.new_call();
  }
  for (auto& t : e->trace) { e->trace_pool.push_back(t.released); e->trace_pool.push_back(t.done); }
  e->trace.clear();
  if (e->trace_on) {
    if (!e->tr_call0) { (void)hipEventCreate(&e->tr_call0); (void)hipEventCreate(&e->tr_tail0); (void)hipEventCreate(&e->tr_tail1); }
    (void)hipEventRecord(e->tr_call0, s);
    e->tr_tail_valid = false;
  }
  return 0;
}

// A phoneme-only call without masked positions (train.py:129): zero loss, nothing to back-propagate.
static int zero_loss_call(PlbEngine* e, bool backward, float* loss, hipStream_t s) {
  HIPTRY(hipMemsetAsync(loss, 0, sizeof(float), s));
  if (!backward) return 0;
  HIPTRY(hipMemsetAsync(e->grads, 0, (size_t)e->ptrain * 4, s));
  if (overlapping(e)) {
    // The other ranks still contribute theirs — and they issue the pieces of a regular step: a collective
    // sequence must be the same on every rank, so this rank issues the very same ranges in the very same order
    // (its zeros), not one all-reduce of the whole buffer.
    for (int i = 0; i < kNPieces; ++i) {
      HB_W(s, e->grads + piece_begin(e, i), (piece_end(e, i) - piece_begin(e, i)) * 4, "zero gradients of a rank without masked phonemes");
      if (reduce_pieces(e, i, i + 1, s)) return 1;
      if (i == kPieceHead && status_exchange(e, s)) return 1;   // where a regular step issues it: behind the head piece
    }
    if (pieces_done(e)) return 1;
  } else if (status_exchange(e, s)) {
    return 1;
  }
  return status_finish(e, loss, s);
}

// The masked rows: head GEMM, cross-entropy, and in a training call the head's gradients and its rows of dy (the output
// gradient of the last application; pruned: the compact rows o_dhm are that gradient).
static int phoneme_head(PlbEngine* e, bool backward, bool prune, const bf16_t* xL, int n_masked, int64_t Tp, bf16_t* dy,
                        float* loss, hipStream_t s) {
  const int H = e->H, NP = e->NP;
  const int NM = (int)rup(n_masked, 128);
  int32_t* rows = e->at<int32_t>(e->o_rows);
  bf16_t* hm = e->at<bf16_t>(e->o_hm);
  float* logm = e->at<float>(e->o_logm);
  float* lrows = e->at<float>(e->o_lrows);
  bf16_t* dlog = e->at<bf16_t>(e->o_dlog);
  bf16_t* dhm = e->at<bf16_t>(e->o_dhm);
  if (backward && !prune) HIPTRY(hipMemsetAsync(dy, 0, (size_t)Tp * H * 2, s));
  if (n_masked > 0) {
    if (!prune) TRY(plb_launch_gather_rows(xL, H, rows, n_masked, NM, H, hm, H, s));   // (pruned: xL IS hm, the compact rows)
    PlbGemmNT g = nt_desc(hm, e->wbf(PLB_HEAD_W), NM, NP, H);
    g.bias = e->par(PLB_HEAD_B); g.Cf = logm; g.ldcf = 256;
    TRY(plb_launch_gemm_nt(&g, 0, 1, s));
    TRY(plb_launch_ce_fwd_bwd(logm, 256, NP, e->at<int32_t>(e->o_tgt), e->at<float>(e->o_w), n_masked, NM, lrows, dlog, 256, s));
    TRY(plb_launch_sum_rows(lrows, n_masked, loss, s));
    if (backward) {
      if (weight_grad(e, dlog, 256, 256, hm, H, NM, NP, H, e->grd(PLB_HEAD_W), s)) return 1;
      TRY(plb_launch_colsum(dlog, 1, (size_t)NM, 256, 256, e->grd(PLB_HEAD_B), NP, 0, e->at<float>(e->o_scratch), 8, s));
      g = nt_desc(dlog, e->at<bf16_t>(e->o_wpT), NM, H, 256);
      g.C = dhm; g.ldc = H;
      TRY(plb_launch_gemm_nt(&g, 0, 0, s));
      // (pruned: the compact gradient rows dhm ARE the output gradient of the last application's compact part)
      if (!prune) TRY(plb_launch_scatter_rows(dhm, H, rows, n_masked, H, dy, H, s));
    }
  } else {  // dual-head step on a batch without masked phonemes: phoneme loss 0, its head gets zero gradients
    HIPTRY(hipMemsetAsync(loss, 0, sizeof(float), s));
    if (backward)
      HIPTRY(hipMemsetAsync(e->grd(PLB_HEAD_W), 0, (size_t)(e->psize[PLB_HEAD_W] + e->psize[PLB_HEAD_B]) * 4, s));
  }
  if (!backward) return 0;
  // the phoneme head's gradients are final: their all-reduce runs beside the whole backward
  HB_W(s, e->grd(PLB_HEAD_W), (e->ptrain - e->poff[PLB_HEAD_W]) * 4, "phoneme head gradients (weight-gradient GEMM, bias column sums)");
  if (overlapping(e) && reduce_pieces(e, kPieceHead, kPieceHead + 1, s)) return 1;
  return 0;
}

// ---- token (grapheme) head over every valid position: fused GEMM + cross-entropy, head gradients, dH ------------
// The fp32 logits are never stored. Pass 1 computes them tile by tile and keeps, per row and 256-column tile, the
// maximum and the sum of exponentials (+ the target logit); a small kernel merges those into the row's
// log-sum-exp, weight and loss; pass 2 recomputes the logits and writes the gradient (softmax - onehot) * w in
// bf16 [Tp][NTp] (2.1 GB at 16384 x 64000), the operand of dWt = dlogits^T · H and dH = dlogits · Wt, and the
// column-sum partials that give the bias gradient.
// Token-packed call (c.rw.row_start): the row axis is the plan's — Tp = rw.Tp rows, the targets and the row weights placed by
// the plan, zeros on the rows that hold no token: pass 2 selects an exact 0 for a row of weight 0, so those rows add nothing
// to the head's gradients or to dH.
static int token_head(PlbEngine* e, const Call& c, bool backward, const bf16_t* xL, const int64_t* token_targets, bf16_t* dy,
                      float* loss, float* loss_parts) {
  const int H = e->H, NT = e->NT, NTp = e->NTp, B = c.B, S = c.S, T = B * S;
  const Rows& rw = c.rw;
  const int64_t Tp = rw.Tp;
  hipStream_t s = c.s;
  // the two passes run on one tile, 256 columns wide (one per-tile maximum / sum per 256 columns); pass 2 leaves cprows rows
  // of column sums
  const PlbGemmNTPlan pass1 = nt_plan(Tp, NTp, H, PLB_NT_CE1), pass2 = nt_plan(Tp, NTp, H, PLB_NT_CE2, PLB_NT_BF16, PLB_NT_COLPART);
  if (pass1.rc || pass2.rc || pass1.tile != pass2.tile) return fail("token_head: no fused GEMM + cross-entropy form for %lld x %d x %d", (long long)Tp, NTp, H);
  const int tile = pass1.tile, ntile = NTp / pass1.tile_n, cprows = pass2.colpart_rows;
  if (backward && cprows > e->tcolp_rows) return fail("token_head: pass 2 writes %d column-sum rows, %d are reserved", cprows, e->tcolp_rows);
  float* tlrows = e->at<float>(e->o_tlrows);
  float* tloss = e->at<float>(e->o_tloss);
  int64_t* ttgt = e->at<int64_t>(e->o_ttgt);
  if (rw.row_start) {
    TRY(plb_launch_pack_token_targets(token_targets, c.lengths, rw.row_start, B, S, (int)Tp, ttgt, s));
  } else {
    HIPTRY(hipMemcpyAsync(ttgt, token_targets, (size_t)T * 8, hipMemcpyDeviceToDevice, s));
    if (Tp > T) HIPTRY(hipMemsetAsync(ttgt + T, 0, (size_t)(Tp - T) * 8, s));
  }
  PlbGemmNT g = nt_desc(xL, e->wbf(PLB_TOK_W), Tp, NTp, H);
  g.bias = e->at<float>(e->o_bt);
  g.ce_cols = NT; g.ce_tgt = ttgt;
  g.ce_pmax = e->at<float>(e->o_tpmax); g.ce_psum = e->at<float>(e->o_tpsum); g.ce_tlogit = e->at<float>(e->o_ttl);
  int tok = plb_prof_begin(pass1.cls, s, pass1.flops, pass1.bytes);
  TRY(plb_launch_gemm_nt_big(&g, tile, 3, 0, s));
  plb_prof_end(tok, s);
  if (rw.row_start) {
    TRY(plb_launch_token_ce_combine_packed(g.ce_pmax, g.ce_psum, ntile, g.ce_tlogit, c.lengths, rw.row_start, B, S, (int)Tp,
                                           e->at<float>(e->o_tlse), e->at<float>(e->o_tw), tlrows, s));
    TRY(plb_launch_sum_rows(tlrows, (int)Tp, tloss, s));
  } else {
    TRY(plb_launch_token_ce_combine(g.ce_pmax, g.ce_psum, ntile, g.ce_tlogit, c.lengths, B, S, (int)Tp,
                                    e->at<float>(e->o_tlse), e->at<float>(e->o_tw), tlrows, s));
    TRY(plb_launch_sum_rows(tlrows, T, tloss, s));
  }
  TRY(plb_launch_add_scalar(loss, loss, tloss, s));
  if (loss_parts) HIPTRY(hipMemcpyAsync(loss_parts + 1, tloss, sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!backward) return 0;
  bf16_t* tdl = e->at<bf16_t>(e->o_tdl);
  g.ce_lse = e->at<float>(e->o_tlse); g.ce_w = e->at<float>(e->o_tw);
  g.C = tdl; g.ldc = NTp; g.colpart = e->at<float>(e->o_tcolp);
  tok = plb_prof_begin(pass2.cls, s, pass2.flops, pass2.bytes);
  TRY(plb_launch_gemm_nt_big(&g, tile, 4, 0, s));
  plb_prof_end(tok, s);
  TRY(plb_launch_colsum(g.colpart, 0, (size_t)cprows, NTp, NTp, e->grd(PLB_TOK_B), NT, 0, e->at<float>(e->o_tscr), 1, s));
  float* gw = NTp == NT ? e->grd(PLB_TOK_W) : e->at<float>(e->o_tgrad);
  if (weight_grad(e, tdl, NTp, NTp, xL, H, Tp, NTp, H, gw, s)) return 1;
  if (NTp != NT) HIPTRY(hipMemcpyAsync(e->grd(PLB_TOK_W), gw, (size_t)NT * H * 4, hipMemcpyDeviceToDevice, s));
  HB_W(s, e->grd(PLB_TOK_W), (e->ptotal - e->poff[PLB_TOK_W]) * 4, "token head gradients");
  if (overlapping(e) && reduce_piece(e, e->poff[PLB_TOK_W], e->ptotal, s)) return 1;
  // dH += dlogits · Wt, on top of the scattered phoneme-head rows (in place: a tile reads its residual
  // before its own stores)
  g = nt_desc(tdl, e->at<bf16_t>(e->o_wtT), Tp, H, NTp);
  g.res = dy; g.ldr = H; g.C = dy; g.ldc = H;
  TRY(plb_launch_gemm_nt(&g, 0, 0, s));
  return 0;
}

// Tail of the backward on two streams.
//  main: the four large token-major weight-gradient GEMMs (MFMA-bound, ~2 ms at config A), each followed — when a
//        communicator is attached — by the all-reduce of the weight it completed, on the communication stream: weight i
//        travels over xGMI while GEMM i+1 runs. The smallest GEMM goes last, so only dense.weight and the small
//        tensors (3.2 MB of 23.4) have nothing left to hide behind.
//  side: everything else that only needs finished gradients — embedding chain, bias and LayerNorm-affine column sums
//        (HBM-bound) — with its own slab / scratch so nothing is shared; joined before the first piece that holds
//        any of its outputs.
static int backward_tail_streams(PlbEngine* e, const Call& c, bf16_t* dy, int du_rows, hipStream_t s2, float* scratch2) {
  const int E = e->E, H = e->H, I = e->I, L = e->L, B = c.B, S = c.S;
  const int64_t Tp = c.rw.Tp;
  hipStream_t s = c.s;
  const int64_t Mtot = (int64_t)L * Tp;
  // stacked rows of the operands whose last application ran on its masked rows only (ffn.weight, ffn_output.weight,
  // dense.weight: their slots of application L-1 hold Mc compact rows); the Q/K/V weights' operands are always full
  const int64_t Mtot_c = e->pruned_rows ? (int64_t)(L - 1) * Tp + e->pruned_rows : Mtot;
  // the stacks the layer loop wrote: application 0's slots, L blocks of partial rows behind them
  const Slots st = slots(e, Tp, B, S, 0, true, e->part_rows_used, du_rows);
  const int64_t qkvcol_all = (int64_t)L * qkvcol_rows(e, B, S);
  // side stream -------------------------------------------------------------------------------------------------------
  // (HB_R / HB_W: the happens-before audit's view of each launch — what it reads that another stream wrote, what it
  // writes that another stream reads. The stash operands of the GEMMs are only ever written in the layer loop, which the
  // fork orders before both streams: they are covered by the whole-workspace entry at the fork.)
  bf16_t* evec = e->at<bf16_t>(e->o_e);
  bf16_t* de = e->at<bf16_t>(e->o_de);
  PlbGemmNT g = nt_desc(dy, e->at<bf16_t>(e->o_winT), Tp, E, H);
  g.C = de; g.ldc = E;
  HB_R(s2, dy, Tp * H * 2, "dX of application 0"); HB_W(s2, de, Tp * E * 2, "dE (map-in backward)");
  TRY(plb_launch_gemm_nt(&g, 0, 0, s2));
  HB_W(s2, e->at<float>(s2 != s ? e->o_slab2 : e->o_slab), (s2 != s ? e->slab2_floats : e->slab_floats) * 4, "map-in weight-gradient slab");
  HB_W(s2, e->grd(PLB_MAP_W), e->psize[PLB_MAP_W] * 4, "map-in weight gradient");
  if (weight_grad(e, dy, H, H, evec, E, Tp, H, E, e->grd(PLB_MAP_W), s2, s2 != s)) return 1;
  HB_W(s2, scratch2, 512 * (3 * H > I ? 3 * H : I) * 4, "column-sum scratch of the side stream");
  HB_W(s2, e->grd(PLB_MAP_B), H * 4, "map-in bias gradient");
  TRY(plb_launch_colsum(dy, 1, (size_t)Tp, H, H, e->grd(PLB_MAP_B), H, 0, scratch2, 128, s2));
  const bool sources = c.ec.any();   // per-token embedding sources / d_inputs_embeds: the launches of embed_inputs.hip
  HB_W(s2, e->grd(PLB_TYPE_EMB), e->psize[PLB_TYPE_EMB] * 4, "token-type embedding gradient");
  if (!sources) HIPTRY(hipMemsetAsync(e->grd(PLB_TYPE_EMB), 0, (size_t)e->psize[PLB_TYPE_EMB] * 4, s2));
  PlbEmbed em = embed_desc(e, c);
  em.dout = de; em.lddo = E; em.dword = e->grd(PLB_WORD_EMB); em.dpos = e->grd(PLB_POS_EMB);
  em.dx = e->at<float>(e->o_dxe);
  em.partials = e->at<float>(e->o_parte); em.nblocks = e->emb_blocks;
  HB_W(s2, em.dx, Tp * E * 4, "embedding LayerNorm backward rows"); HB_W(s2, em.partials, (int64_t)e->emb_blocks * 2 * E * 4, "embedding LayerNorm partials");
  HB_W(s2, e->grd(PLB_WORD_EMB), (e->poff[PLB_MAP_W] - e->poff[PLB_WORD_EMB]) * 4, "embedding tables' and embedding LayerNorm's gradients");
  if (sources) {
    // every row of the three tables is written by the scatter: word rows as below (zeros with inputs_embeds), position and
    // token-type rows from the chunk partial rows where position_ids / token_type_ids key them
    em.lengths = c.lengths; em.B = B;   // (padded call too: d_inputs_embeds gets its zeros at the pad positions)
    PlbEmbedIn xi = embed_in_desc(e, c.ec, &em);
    xi.dtype_rows = e->grd(PLB_TYPE_EMB); xi.d_inputs_embeds = c.ec.d_inputs_embeds;
    xi.chunk_part = e->at<float>(e->o_embpart);
    if (xi.d_inputs_embeds) HB_W(s2, xi.d_inputs_embeds, (int64_t)B * S * E * 4, "d_inputs_embeds (the caller's buffer)");
    HB_W(s2, xi.chunk_part, (int64_t)plb_embed_inputs_part_floats(B * S, e->P, xi.NTY, E) * 4, "chunk partial rows of the keyed table sums");
    TRY(plb_launch_embed_inputs_bwd(&xi, s2));
    TRY(plb_launch_embed_inputs_scatter(&xi, s2));
    TRY(plb_launch_colsum(em.partials, 0, (size_t)e->emb_blocks, 2 * E, 2 * E, e->grd(PLB_EMB_LN_W), 2 * E, 0, scratch2, 1, s2));
  } else {
    TRY(plb_launch_embed_bwd(&em, s2));
    TRY(plb_launch_embed_scatter(&em, e->P, s2));
    TRY(plb_launch_colsum(em.partials, 0, (size_t)e->emb_blocks, 2 * E, 2 * E, e->grd(PLB_EMB_LN_W), 2 * E, 0, scratch2, 1, s2));
    // token_type row 0 receives every token's gradient = the column sums of dpos
    TRY(plb_launch_colsum(e->grd(PLB_POS_EMB), 0, (size_t)e->P, E, E, e->grd(PLB_TYPE_EMB), E, 0, scratch2, 1, s2));
  }
  // Q/K/V biases: the attention-backward kernels left the column sums of every 32-row patch they stored, per application
  // ([L][B*QT*4][3H])
  HB_R(s2, st.qkvcol, qkvcol_all * 3 * H * 4, "Q/K/V bias partial rows");
  HB_W(s2, e->grd(PLB_Q_B), 3 * H * 4, "Q/K/V bias gradients");
  TRY(plb_launch_colsum(st.qkvcol, 0, (size_t)qkvcol_all, 3 * H, 3 * H, e->grd(PLB_Q_B), 3 * H, 0, scratch2, 64, s2));
  HB_W(s2, e->grd(PLB_FFN_B), I * 4, "ffn.bias gradient");
  if (du_rows > 0) {
    HB_R(s2, st.ducol, (int64_t)L * du_rows * I * 4, "dU column-sum partial rows");
    TRY(plb_launch_colsum(st.ducol, 0, (size_t)L * du_rows, I, I, e->grd(PLB_FFN_B), I, 0, scratch2, 16, s2));
  } else {
    HB_R(s2, st.du, Mtot_c * I * 2, "dU of every application");
    TRY(plb_launch_colsum(st.du, 1, (size_t)Mtot_c, I, I, e->grd(PLB_FFN_B), I, 0, scratch2, 64, s2));
  }
  // LayerNorm-backward partials [L*blocks][3H]: dgamma | dbeta | column sums of dx. (Summing the L applications into
  // one image inside the kernel — PlbLayerNorm.accumulate — was measured: the read-modify-write costs the main stream
  // 2.5 us per launch to save side-stream traffic that is hidden behind the weight-gradient GEMMs anyway.) The third block is the bias
  // gradient of the Linear that produced the LayerNorm's input (dense.bias = colsum(dpre1), ffn_output.bias =
  // colsum(dpre2)): no pass over the stacked gradients.
  const size_t prow = (size_t)L * e->part_rows_used;
  HB_R(s2, st.part1, (int64_t)L * e->part_rows * 3 * H * 4, "LayerNorm-1 backward partial rows");
  HB_W(s2, e->grd(PLB_DENSE_B), 3 * H * 4, "dense.bias + LayerNorm-1 affine gradients");
  TRY(plb_launch_colsum(st.part1, 0, prow, 3 * H, 3 * H, e->grd(PLB_LN1_W), 2 * H, 0, scratch2, 64, s2));
  TRY(plb_launch_copy_cols(scratch2, 64, 3 * H, 2 * H, H, e->grd(PLB_DENSE_B), s2));
  HB_R(s2, st.part2, (int64_t)L * e->part_rows * 3 * H * 4, "LayerNorm-2 backward partial rows");
  HB_W(s2, e->grd(PLB_LN2_W), 2 * H * 4, "LayerNorm-2 affine gradients"); HB_W(s2, e->grd(PLB_FFNO_B), H * 4, "ffn_output.bias gradient");
  TRY(plb_launch_colsum(st.part2, 0, prow, 3 * H, 3 * H, e->grd(PLB_LN2_W), 2 * H, 0, scratch2, 64, s2));
  TRY(plb_launch_copy_cols(scratch2, 64, 3 * H, 2 * H, H, e->grd(PLB_FFNO_B), s2));
  if (s2 != s) HIPTRY(ev_record(e, e->ev_join, s2));
  // main stream: shared-layer weight gradients, one token-major GEMM per weight over all L applications ------------
  // Overlapped exchange: a weight's range travels as soon as its GEMM (+ slab reduction) has written it; the small
  // tensors between the weights in the flat order (biases, LayerNorm, embeddings) travel behind the SIDE stream's event
  // (below, after the first weight's piece); the smallest weight goes last.
  const bool ov = overlapping(e);
  const bool t8 = e->tn8_call;   // fp8 call: gradient (e5m2) x activation (e4m3) images of all L applications
  float* const slab = e->at<float>(e->o_slab);
  HB_W(s, slab, e->slab_floats * 4, "weight-gradient slab"); HB_W(s, e->grd(PLB_Q_W), 3 * H * H * 4, "Q/K/V weight gradients");
  if (t8 ? weight_grad(e, st.dq8, 3 * H, 3 * H, st.x8, H, Mtot, 3 * H, H, e->grd(PLB_Q_W), s, false, F8_DQ, F8_X)
         : weight_grad(e, st.dqkv, 3 * H, 3 * H, st.x, H, Mtot, 3 * H, H, e->grd(PLB_Q_W), s)) return 1;
  if (ov && reduce_pieces(e, kPieceQkvW, kPieceFfnW, s)) return 1;
  HB_W(s, slab, e->slab_floats * 4, "weight-gradient slab"); HB_W(s, e->grd(PLB_FFN_W), (int64_t)I * H * 4, "ffn.weight gradient");
  if (t8 ? weight_grad(e, st.du8, I, I, st.a8, H, Mtot_c, I, H, e->grd(PLB_FFN_W), s, false, F8_DU, F8_A)
         : weight_grad(e, st.du, I, I, st.a, H, Mtot_c, I, H, e->grd(PLB_FFN_W), s)) return 1;
  if (ov && reduce_pieces(e, kPieceFfnW, kPieceSmall, s)) return 1;
  if (ov) {
    // The small tensors between the weights in the flat order (embeddings + map-in + LayerNorm 2 | Q/K/V biases | dense.bias +
    // LayerNorm 1 | ffn.bias | ffn_output.bias) all come from the side stream, which is done after about three of the four
    // GEMMs: their pieces are released by the SIDE stream's own event (everything it does in this call has been enqueued
    // above), behind the second weight's piece in the communication stream's queue (the side stream, stretched by the
    // GEMMs it runs beside, ends between GEMM 2 and GEMM 3: piece_trace) — five latency-bound all-reduces that
    // travel beside the remaining GEMMs instead of after the last one (they were the step's exposed tail at world > 1:
    // four collectives in a row behind the join). The main stream joins the side stream at the end of the tail as before.
    if (reduce_pieces(e, kPieceSmall, kPieceFfnoW, s2)) return 1;
  }
  HB_W(s, slab, e->slab_floats * 4, "weight-gradient slab"); HB_W(s, e->grd(PLB_FFNO_W), (int64_t)I * H * 4, "ffn_output.weight gradient");
  if (t8 ? weight_grad(e, st.dp8, H, H, st.g8, I, Mtot_c, H, I, e->grd(PLB_FFNO_W), s, false, F8_DP, F8_G)
         : weight_grad(e, st.dpre2, H, H, st.g, I, Mtot_c, H, I, e->grd(PLB_FFNO_W), s)) return 1;
  if (ov && reduce_pieces(e, kPieceFfnoW, kPieceDenseW, s)) return 1;
  HB_W(s, slab, e->slab_floats * 4, "weight-gradient slab"); HB_W(s, e->grd(PLB_DENSE_W), (int64_t)H * H * 4, "dense.weight gradient");
  if (t8 ? weight_grad(e, st.dp18, H, H, st.c8, H, Mtot_c, H, H, e->grd(PLB_DENSE_W), s, false, F8_DP1, F8_C)
         : weight_grad(e, st.dpre1, H, H, st.ctx, H, Mtot_c, H, H, e->grd(PLB_DENSE_W), s)) return 1;
  if (ov && reduce_pieces(e, kPieceDenseW, kNPieces, s)) return 1;   // the smallest weight goes last
  return 0;
}

static int backward_tail(PlbEngine* e, const Call& c, bf16_t* dy, int du_rows) {
  hipStream_t s = c.s, s2 = s;
  float* scratch2 = e->at<float>(e->o_scratch);
  // the layer loop (all of it on the caller's stream) has written the stash, the partial-row tables, dX: one entry
  HB_W(s, e->ws, e->ws_bytes, "layer loop (whole workspace)");
  if (e->trace_on) (void)hipEventRecord(e->tr_tail0, s);
  if (e->side) {
    s2 = e->side;
    scratch2 = e->at<float>(e->o_scratch2);
    HIPTRY(ev_record(e, e->ev_fork, s));
    HIPTRY(ev_wait(e, s2, e->ev_fork));
  }
  const int rc = backward_tail_streams(e, c, dy, du_rows, s2, scratch2);
  // Whatever happened above, the caller's stream must not run ahead of the side stream's work (also on an error
  // path: the side stream may hold launches that read buffers the caller is about to reuse).
  if (s2 != s) {
    if (rc) (void)ev_record(e, e->ev_join, s2);
    const hipError_t je = ev_wait(e, s, e->ev_join);
    if (!rc && je != hipSuccess) return fail("plb_loss_fwd_bwd: joining the side stream: %s", hipGetErrorString(je));
  }
  if (e->trace_on) { (void)hipEventRecord(e->tr_tail1, s); e->tr_tail_valid = true; }
  if (rc) return rc;
  // from here on the caller's stream may again touch anything in the workspace (the next call's forward will)
  HB_W(s, e->ws, e->ws_bytes, "after the side stream's join (whole workspace)");
  return pieces_done(e);
}

static const char* const kPrunedText =
    "the last loss call was phoneme-only and pruned its last application to the masked rows: it left no final hidden state "
    "of every row (a dual-head call, a forward or plb_set_prune_last(0) leaves one)";

// token_targets == NULL: the reference's phoneme-only step. Otherwise dual-head: loss = phoneme loss + token loss.
// backward == false: validate() — forward and loss only, one layer of activations, the gradient buffer untouched.
static int loss_impl(PlbEngine* e, bool backward, const int64_t* masked_ids, const int64_t* labels,
                     const int64_t* token_targets, const int32_t* lengths, const int32_t* idx_offsets,
                     const int32_t* idx_flat, int32_t n_masked, int32_t B, int32_t S, const PlbPacking* pk, float* loss,
                     float* loss_parts, void* stream) {
  const char* who = backward ? "plb_loss_fwd_bwd" : "plb_loss_fwd";
  if (check_shape(e, B, S, who)) return 1;
  drop_stash(e, "a plb_loss_* call rewrote the workspace since");
  drop_final(e, "the last call that ran the encoder (a plb_loss_* call) failed");
  if (backward && e->infer) return fail("%s: inference-only engine (PlbConfig.inference_only = 1)", who);
  if (backward && !e->grads) return fail("%s: no gradient buffer bound", who);
  if (!masked_ids || !labels || !idx_offsets || !loss) return fail("%s: null argument", who);
  if (n_masked < 0 || n_masked > e->NMcap) return fail("%s: n_masked %d out of range", who, n_masked);
  if (token_targets && !e->NT) return fail("%s: the engine has no token head (num_tokens = 0)", who);
  hipStream_t s = (hipStream_t)stream;
  Rows rw;
  if (pick_rows(e, pk, lengths, token_targets != nullptr && !e->packed_dual, B, S, who, &rw)) return 1;
  const int64_t Tp = rw.Tp;
  // from here on the call launches: what plb_masked_report reads is this call's, once it has gone through
  e->rep_valid = false;
  e->rep_n = n_masked; e->rep_B = B; e->rep_dual = token_targets != nullptr; e->rep_tok_rows = token_targets ? Tp : 0;
  const Call c = {who, masked_ids, lengths, B, S, rw, {}, nullptr, s};
  if (backward && begin_training_call(e, token_targets != nullptr, s)) return 1;
  if (n_masked == 0 && !token_targets) {
    drop_final(e, "the last loss call had no masked position and no token targets: it did not run the encoder");
    if (zero_loss_call(e, backward, loss, s)) return 1;
    e->rep_valid = true;
    return 0;
  }

  // the row list first: a phoneme-only call runs the post-attention part of its LAST application on these rows alone
  // (last_application_fwd_pruned) when that is less than half of the batch; dual-head calls run every row
  const int NM = (int)rup(n_masked, 128);
  Prune pr = {e->at<int32_t>(e->o_rows), n_masked, NM};
  const bool prune = prune_enabled() && n_masked > 0 && !token_targets && e->L >= 2 && 2 * (int64_t)NM <= Tp;
  if (n_masked > 0) {
    if (rw.row_start)
      TRY(plb_launch_ce_prepare_packed(idx_offsets, idx_flat, labels, B, S, rw.row_start, e->at<int32_t>(e->o_rows),
                                       e->at<int32_t>(e->o_tgt), e->at<float>(e->o_w), s));
    else
      TRY(plb_launch_ce_prepare(idx_offsets, idx_flat, labels, B, S, e->at<int32_t>(e->o_rows), e->at<int32_t>(e->o_tgt),
                                e->at<float>(e->o_w), s));
  }
  if (backward) e->pruned_rows = prune ? NM : 0;
  e->last_app_rows[0] = prune ? NM : Tp; e->last_app_rows[1] = Tp;
  bf16_t* xL = nullptr;
  if (run_encoder(e, c, backward, &xL, prune ? &pr : nullptr)) return 1;
  bf16_t* dy = backward ? e->at<bf16_t>(e->o_dy0) : nullptr;
  if (phoneme_head(e, backward, prune, xL, n_masked, Tp, dy, loss, s)) return 1;
  if (loss_parts) HIPTRY(hipMemcpyAsync(loss_parts, loss, sizeof(float), hipMemcpyDeviceToDevice, s));
  if (token_targets && token_head(e, c, backward, xL, token_targets, dy, loss, loss_parts)) return 1;
  if (!backward) {
    if (e->fp8_on) {  // forward-only call in fp8 mode: activation sites only (gradient sites saw nothing and keep theirs)
      TRY(fp8_update_scales(e, s));
      e->fp8_ready = true;
    }
    // (no collective in a loss-only call: ranks may validate different numbers of batches. A word raised here is sticky
    // and travels with the next training call's exchange.)
    e->last_loss = loss;
    TRY(plb_launch_step_status(e->at<unsigned int>(e->o_lnerr), loss, e->host_err_dev, nullptr, s));
    e->rep_valid = true;
    if (prune) drop_final(e, kPrunedText); else note_final(e, xL, c);
    return 0;
  }

  int du_rows = 0;
  if (encoder_bwd(e, c, prune ? &pr : nullptr, &dy, &du_rows, nullptr)) return 1;
  // the last launch that can raise the hand-off error word is behind us: the word travels now (beside the tail)
  if (status_exchange(e, s)) return 1;
  if (backward_tail(e, c, dy, du_rows)) return 1;
  if (e->fp8_on) {
    // This call's maxima become the next call's scales; a calibration call arms the fp8 path. AFTER the tail: the weight-
    // gradient GEMMs dequantise this call's images with the scales they were written with (updated before the tail, a
    // call that follows one with 4x larger gradients came out 2x off: tools/fp8_diag.py).
    TRY(fp8_update_scales(e, s));
    e->fp8_ready = true;
    e->fp8_bwd_ready = true;
  }
  // Last launch of the step: a hand-off of the fused LayerNorm launches that timed out — on ANY rank — turns the loss into
  // NaN and shows in plb_poll_status; plb_adamw_step skips on the same word. No host round trip anywhere.
  if (status_finish(e, loss, s)) return 1;
  e->rep_valid = true;
  if (prune) drop_final(e, kPrunedText); else note_final(e, xL, c);
  return 0;
}

extern "C" int plb_loss_fwd_bwd(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int32_t* lengths,
                                const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked, int32_t B,
                                int32_t S, float* loss, void* stream) {
  return loss_impl(e, true, masked_ids, labels, nullptr, lengths, idx_offsets, idx_flat, n_masked, B, S, nullptr, loss, nullptr,
                   stream);
}
extern "C" int plb_loss_fwd_bwd_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int32_t* lengths,
                                       const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked, int32_t B,
                                       int32_t S, const PlbPacking* packing, float* loss, void* stream) {
  return loss_impl(e, true, masked_ids, labels, nullptr, lengths, idx_offsets, idx_flat, n_masked, B, S, packing, loss, nullptr,
                   stream);
}

extern "C" int plb_loss_fwd_bwd_dual(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels,
                                     const int64_t* token_ids, const int32_t* lengths, const int32_t* idx_offsets,
                                     const int32_t* idx_flat, int32_t n_masked, int32_t B, int32_t S, float* loss,
                                     float* loss_parts, void* stream) {
  if (!token_ids) return fail("plb_loss_fwd_bwd_dual: token_ids is null");
  return loss_impl(e, true, masked_ids, labels, token_ids, lengths, idx_offsets, idx_flat, n_masked, B, S, nullptr, loss,
                   loss_parts, stream);
}

extern "C" int plb_loss_fwd_bwd_dual_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels,
                                            const int64_t* token_ids, const int32_t* lengths, const int32_t* idx_offsets,
                                            const int32_t* idx_flat, int32_t n_masked, int32_t B, int32_t S,
                                            const PlbPacking* packing, float* loss, float* loss_parts, void* stream) {
  if (!token_ids) return fail("plb_loss_fwd_bwd_dual_packed: token_ids is null");
  return loss_impl(e, true, masked_ids, labels, token_ids, lengths, idx_offsets, idx_flat, n_masked, B, S, packing, loss,
                   loss_parts, stream);
}

extern "C" int plb_loss_fwd(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                            const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat, int32_t n_masked,
                            int32_t B, int32_t S, float* loss, float* loss_parts, void* stream) {
  return loss_impl(e, false, masked_ids, labels, token_ids, lengths, idx_offsets, idx_flat, n_masked, B, S, nullptr, loss,
                   loss_parts, stream);
}
extern "C" int plb_loss_fwd_packed(PlbEngine* e, const int64_t* masked_ids, const int64_t* labels, const int64_t* token_ids,
                                   const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat,
                                   int32_t n_masked, int32_t B, int32_t S, const PlbPacking* packing, float* loss,
                                   float* loss_parts, void* stream) {
  return loss_impl(e, false, masked_ids, labels, token_ids, lengths, idx_offsets, idx_flat, n_masked, B, S, packing, loss,
                   loss_parts, stream);
}

// ---- differentiable encoder: forward now, backward from a caller's gradient later (include/plbert.h) --------------------
// plb_encode[_layers] is run_encoder with the stash on and nothing pruned; the stash then waits, marked live, while the caller's
// downstream model runs. plb_encode_bwd turns the caller's d(last_hidden_state) into the output gradient of the last
// application (plb_launch_seed_dy) and runs the stages of a loss call's backward behind it. The phoneme head takes no
// part: its gradient range is written as zeros (and still travels as the first piece of the exchange, as in
// zero_loss_call: the collective sequence of a step is the same whatever the step computes). The pooler takes part only when
// plb_encode_bwd_pooled brings a gradient of pooler_output: its backward (pooler_bwd.hip) then runs first, writes the pooler's
// range — which travels with the head's piece — and adds its share to row (b, 0) of the seeded output gradient.
static int encode_impl(PlbEngine* e, const char* who, const EncArgs& a, float* hidden) {
  if (check_shape(e, a.B, a.S, who)) return 1;
  if (e->infer) return fail("%s: inference-only engine (PlbConfig.inference_only = 1): a differentiable forward keeps every application's activations", who);
  if (!e->grads) return fail("%s: no gradient buffer bound", who);
  if (e->fp8_on) return fail("%s: fp8 mode is on (the gradient sites' delayed scales belong to the pre-training loss); call plb_set_fp8(e, 0, stream) first", who);
  EmbedCall ec;
  if (embed_call(e, a.ids, a.inputs, nullptr, who, &ec)) return 1;
  if (key_mask_check(e, a.key_mask, a.S, who)) return 1;
  if (!hidden) return fail("%s: hidden is null", who);
  Rows rw;
  if (pick_rows(e, a.packing, a.lengths, false, a.B, a.S, who, &rw)) return 1;
  drop_stash(e, "a plb_encode call that failed rewrote the workspace since");
  drop_final(e, "the last call that ran the encoder (plb_encode) failed");
  Call c = {who, a.ids, a.lengths, a.B, a.S, rw, ec, a.layers, (hipStream_t)a.stream};
  hipStream_t s = c.s;
  // (whatever an earlier call left on the side / communication stream was joined by that call's tail; audit on: checked)
  HB_W(s, e->ws, e->ws_bytes, "plb_encode (whole workspace)");
  e->last_app_rows[0] = e->last_app_rows[1] = rw.Tp;
  bf16_t* x = nullptr;
  if (key_mask_words(e, a.key_mask, &c)) return 1;
  if (run_encoder(e, c, true, &x, nullptr)) return 1;
  // .last_hidden_state in the caller's [B,S,H] layout, ZEROS at the pad positions in both layouts (by lengths, as tap_hidden
  // does): a downstream model must not be handed numbers that carry no gradient
  if (a.lengths) TRY(plb_launch_unpack_rows(x, 1, e->H, rw.row_start, a.lengths, a.B, a.S, e->H, hidden, s));
  else TRY(plb_launch_bf16_to_f32(x, e->H, hidden, e->H, rw.T, e->H, s));
  TRY(plb_launch_step_status(e->at<unsigned int>(e->o_lnerr), nullptr, e->host_err_dev, nullptr, s));
  e->stash_live = true;
  e->stash_B = a.B; e->stash_S = a.S; e->stash_rows = rw.Tp; e->stash_used = rw.T; e->stash_row_start = rw.row_start;
  e->stash_masked = a.key_mask != nullptr;
  note_final(e, x, c);
  return 0;
}
extern "C" int plb_encode(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                          const PlbPacking* pk, float* hidden, void* stream) {
  return encode_impl(e, "plb_encode", {ids, nullptr, nullptr, lengths, B, S, pk, nullptr, stream}, hidden);
}
extern "C" int plb_encode_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                                 const PlbPacking* pk, float* hidden, const PlbLayerOutputs* layers, void* stream) {
  return encode_impl(e, "plb_encode_layers", {ids, nullptr, nullptr, lengths, B, S, pk, layers, stream}, hidden);
}
// plb_encode_layers with the embedding inputs (include/plbert.h: PlbEmbedInputs); none given: that call
extern "C" int plb_encode_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths, int32_t B,
                                 int32_t S, const PlbPacking* pk, float* hidden, const PlbLayerOutputs* layers, void* stream) {
  return encode_impl(e, "plb_encode_inputs", {ids, inputs, nullptr, lengths, B, S, pk, layers, stream}, hidden);
}
// plb_encode_inputs with a key mask (include/plbert.h); key_mask == NULL: that call
extern "C" int plb_encode_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                                 const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* pk, float* hidden,
                                 const PlbLayerOutputs* layers, void* stream) {
  return encode_impl(e, key_mask ? "plb_encode_masked" : "plb_encode_inputs", {ids, inputs, key_mask, lengths, B, S, pk, layers, stream},
                     hidden);
}

// plb_encode_bwd_layers, and plb_encode_bwd as a call of it (layers_call false: d_hidden required, with its own text).
// d_below[l] (host array of L device pointers, or null): the caller's gradient of hidden_states[l], the input of application
// l; it joins the residual operand of the dX GEMM that produces that state's gradient (attention_bwd_dx). d_hidden == NULL:
// the output gradient of the last application is zero. d_pooled (fp32 [B,H], or null; pooled_call: the entry that takes one): the
// caller's gradient of pooler_output — the pooler backward (pooler_bwd.hip) runs first, from the final hidden state of the
// stash and the fp32 parameters: it writes the pooler range of the gradient buffer and dh0, which joins row (b, 0) of dy.
static int encode_bwd_impl(PlbEngine* e, const char* who, const EncArgs& a, const float* d_hidden, const float* const* d_below,
                           float* d_inputs_embeds, bool layers_call, const float* d_pooled = nullptr, bool pooled_call = false) {
  if (check_shape(e, a.B, a.S, who)) return 1;
  if (e->infer) return fail("%s: inference-only engine (PlbConfig.inference_only = 1)", who);
  if (!e->grads) return fail("%s: no gradient buffer bound", who);
  // the pointer array is read here, on the host: a copy without its NULL-only form
  std::vector<const float*> below;
  if (d_below) {
    below.assign(d_below, d_below + e->L);
    bool any = false;
    for (const float* p : below) any = any || p != nullptr;
    if (!any) below.clear();
  }
  EmbedCall ec;
  if (embed_call(e, a.ids, a.inputs, d_inputs_embeds, who, &ec)) return 1;
  if (key_mask_check(e, a.key_mask, a.S, who)) return 1;
  if (!d_hidden && below.empty() && !d_pooled)
    return pooled_call ? fail("%s: nothing to differentiate (d_hidden and d_pooled are null and d_below has no entry)", who) :
           layers_call ? fail("%s: nothing to differentiate (d_hidden is null and d_below has no entry)", who)
                       : fail("%s: d_hidden is null", who);
  if ((uintptr_t)d_pooled & 15) return fail("%s: d_pooled must be 16-byte aligned", who);
  if (!e->stash_live) return fail("%s: no live plb_encode stash: %s", who, e->stash_dead_by);
  if (a.B != e->stash_B || a.S != e->stash_S)
    return fail("%s: batch %d x seq %d differs from the plb_encode call's %d x %d", who, a.B, a.S, e->stash_B, e->stash_S);
  if ((a.key_mask != nullptr) != e->stash_masked)
    return fail("%s: %s, the live plb_encode call ran %s one (the backward takes the key mask of its forward again)", who,
                a.key_mask ? "a key mask is given" : "no key mask is given", e->stash_masked ? "with" : "without");
  Rows rw;
  // (a call that fails launches nothing and leaves what plb_last_call_rows reports alone)
  const int64_t exec_rows[2] = {e->last_exec_rows[0], e->last_exec_rows[1]};
  const bool plan_ok = pick_rows(e, a.packing, a.lengths, false, a.B, a.S, who, &rw) == 0;   // (its own text names the plan)
  const bool same = plan_ok && rw.Tp == e->stash_rows && rw.T == e->stash_used && rw.row_start == e->stash_row_start;
  if (!same) {
    e->last_exec_rows[0] = exec_rows[0]; e->last_exec_rows[1] = exec_rows[1];
    if (!plan_ok) return 1;
    return fail("%s: packing plan differs from the plb_encode call's (%lld rows, %lld used, %s; that call: %lld rows, %lld used, %s)",
                who, (long long)rw.Tp, (long long)rw.T, rw.row_start ? "packed" : "padded", (long long)e->stash_rows,
                (long long)e->stash_used, e->stash_row_start ? "packed" : "padded");
  }
  Call c = {who, a.ids, a.lengths, a.B, a.S, rw, ec, nullptr, (hipStream_t)a.stream};
  hipStream_t s = c.s;
  if (begin_training_call(e, false, s)) return 1;
  e->stash_live = false;
  e->stash_dead_by = "plb_encode_bwd has consumed it (one backward per plb_encode)";
  e->head_grads_live = false;
  e->pruned_rows = 0;
  const int64_t Tp = rw.Tp;
  float* const dh0 = e->at<float>(e->o_pool_dh0);
  if (d_pooled) {
    e->pool_grads_live = true;
    const bf16_t* const xL = slots(e, Tp, a.B, a.S, e->L - 1, true).y;   // the output of the last application
    float* const dpre = e->at<float>(e->o_pool_dpre);
    HB_R(s, xL, Tp * e->H * 2, "final hidden state (pooler backward)");
    HB_W(s, dpre, (int64_t)a.B * e->H * 4, "dpre of the pooler backward"); HB_W(s, dh0, (int64_t)a.B * e->H * 4, "dh0 of the pooler backward");
    HB_W(s, e->grd(PLB_POOL_W), (pool_end(e) - e->poff[PLB_POOL_W]) * 4, "pooler gradients");
    TRY(plb_launch_pooler_bwd(xL, e->H, rw.row_start, a.B, a.S, e->H, e->par(PLB_POOL_W), e->par(PLB_POOL_B), d_pooled, dpre,
                              e->grd(PLB_POOL_W), e->grd(PLB_POOL_B), dh0, s));
  }
  bf16_t* dy = e->at<bf16_t>(e->o_dy0);
  HB_W(s, dy, Tp * e->H * 2, "output gradient of the last application, seeded from d_hidden");
  if (key_mask_words(e, a.key_mask, &c)) return 1;
  if (d_hidden) TRY(plb_launch_seed_dy(d_hidden, a.lengths, rw.row_start, a.B, a.S, e->H, (int)Tp, dy, s));
  else HIPTRY(hipMemsetAsync(dy, 0, (size_t)Tp * e->H * 2, s));   // (no gradient at the last slot: every row zero)
  if (d_pooled) TRY(plb_launch_seed_dy_first_rows(d_hidden, dh0, rw.row_start, a.B, a.S, e->H, dy, s));   // row (b, 0) += dh0[b]
  // the phoneme head took no part: zeros, final before the layer loop — its piece travels where a regular step's does
  HB_W(s, e->grd(PLB_HEAD_W), (e->ptrain - e->poff[PLB_HEAD_W]) * 4, "phoneme head gradients (zeros: plb_encode_bwd)");
  HIPTRY(hipMemsetAsync(e->grd(PLB_HEAD_W), 0, (size_t)(e->ptrain - e->poff[PLB_HEAD_W]) * 4, s));
  // (with a d_pooled the pooler range, adjacent and final too, travels in the same collective)
  if (overlapping(e) && (d_pooled ? reduce_piece(e, e->poff[PLB_HEAD_W], pool_end(e), s) : reduce_pieces(e, kPieceHead, kPieceHead + 1, s)))
    return 1;
  int du_rows = 0;
  if (encoder_bwd(e, c, nullptr, &dy, &du_rows, below.empty() ? nullptr : below.data())) return 1;
  if (status_exchange(e, s)) return 1;
  if (backward_tail(e, c, dy, du_rows)) return 1;
  return status_finish(e, nullptr, s);
}
extern "C" int plb_encode_bwd(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                              const PlbPacking* pk, const float* d_hidden, void* stream) {
  return encode_bwd_impl(e, "plb_encode_bwd", {ids, nullptr, nullptr, lengths, B, S, pk, nullptr, stream}, d_hidden, nullptr, nullptr,
                         false);
}
extern "C" int plb_encode_bwd_layers(PlbEngine* e, const int64_t* ids, const int32_t* lengths, int32_t B, int32_t S,
                                     const PlbPacking* pk, const float* d_hidden, const float* const* d_below, void* stream) {
  return encode_bwd_impl(e, "plb_encode_bwd_layers", {ids, nullptr, nullptr, lengths, B, S, pk, nullptr, stream}, d_hidden, d_below,
                         nullptr, true);
}
// plb_encode_bwd_layers with the embedding inputs of the live plb_encode_inputs call and, when asked, the gradient of the
// pre-LayerNorm embedding sum; nothing of the two given: that call
extern "C" int plb_encode_bwd_inputs(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* lengths,
                                     int32_t B, int32_t S, const PlbPacking* pk, const float* d_hidden, const float* const* d_below,
                                     float* d_inputs_embeds, void* stream) {
  return encode_bwd_impl(e, "plb_encode_bwd_inputs", {ids, inputs, nullptr, lengths, B, S, pk, nullptr, stream}, d_hidden, d_below,
                         d_inputs_embeds, true);
}
// plb_encode_bwd_inputs with the key mask of the live plb_encode_masked call; key_mask == NULL: that call
extern "C" int plb_encode_bwd_masked(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                                     const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* pk, const float* d_hidden,
                                     const float* const* d_below, float* d_inputs_embeds, void* stream) {
  return encode_bwd_impl(e, key_mask ? "plb_encode_bwd_masked" : "plb_encode_bwd_inputs",
                         {ids, inputs, key_mask, lengths, B, S, pk, nullptr, stream}, d_hidden, d_below, d_inputs_embeds, true);
}
// plb_encode_bwd_masked with the caller's gradient of pooler_output; d_pooled == NULL: that call
extern "C" int plb_encode_bwd_pooled(PlbEngine* e, const int64_t* ids, const PlbEmbedInputs* inputs, const int32_t* key_mask,
                                     const int32_t* lengths, int32_t B, int32_t S, const PlbPacking* pk, const float* d_hidden,
                                     const float* const* d_below, float* d_inputs_embeds, const float* d_pooled, void* stream) {
  return encode_bwd_impl(e, d_pooled ? "plb_encode_bwd_pooled" : key_mask ? "plb_encode_bwd_masked" : "plb_encode_bwd_inputs",
                         {ids, inputs, key_mask, lengths, B, S, pk, nullptr, stream}, d_hidden, d_below, d_inputs_embeds, true, d_pooled,
                         true);
}
