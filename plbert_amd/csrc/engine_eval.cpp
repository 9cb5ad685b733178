// The reports: entry points that read what a call left in the workspace and take no part in the step — plb_masked_report
// (below) and plb_token_report (further down).
// plb_masked_report (include/plbert.h): accuracy, top-k, per-row and per-sample losses of the LAST loss call, from what that
// call left in the workspace — the fp32 logits of its masked rows and their labels (o_logm, o_tgt: phoneme_head) and, after
// a dual-head call, the token head's per-tile row maxima, target logits and row weights (o_tpmax, o_ttl, o_tw: token_head).
// Reads those regions and PlbEngine's rep_* block; writes the caller's buffers and the report's own regions (o_rep_*), and
// nothing else: no engine state changes, a live plb_encode stash stays live, the health word is left alone.
#include "engine_internal.h"

extern "C" int plb_masked_report(PlbEngine* e, const int32_t* idx_offsets, int32_t B, int32_t topk, const PlbMaskedReport* out,
                                 void* stream) {
  if (!e || !e->ws) return fail("plb_masked_report: engine not bound");
  if (!out) return fail("plb_masked_report: out is null");
  if (!e->rep_valid) return fail("plb_masked_report: no loss call has run on this engine since plb_bind (or the last one failed)");
  if (B != e->rep_B) return fail("plb_masked_report: B %d differs from the loss call's %d", B, e->rep_B);
  if (out->token_totals && !e->rep_dual) return fail("plb_masked_report: token_totals asked after a phoneme-only loss call");
  if (topk < 0 || topk > 8) return fail("plb_masked_report: topk %d outside [0, 8]", topk);
  const bool per_sample = out->sample_loss || out->sample_top1 || out->sample_topk;
  if ((per_sample || out->totals) && !idx_offsets)
    return fail("plb_masked_report: %s wanted but idx_offsets is null", per_sample ? "a sample output" : "totals");
  hipStream_t s = (hipStream_t)stream;
  const int n = e->rep_n;
  if (n == 0) {  // nothing was masked: zeros wherever something [B] or fixed-size was asked for
    if (out->sample_loss) HIPTRY(hipMemsetAsync(out->sample_loss, 0, (size_t)B * 4, s));
    if (out->sample_top1) HIPTRY(hipMemsetAsync(out->sample_top1, 0, (size_t)B * 4, s));
    if (out->sample_topk) HIPTRY(hipMemsetAsync(out->sample_topk, 0, (size_t)B * 4, s));
    if (out->totals) HIPTRY(hipMemsetAsync(out->totals, 0, 4 * 4, s));
  } else {
    const bool need_rank = out->rank || out->sample_top1 || out->sample_topk || out->totals;
    const bool need_nll = out->nll || out->sample_loss;
    int32_t* rank = out->rank ? out->rank : need_rank ? e->at<int32_t>(e->o_rep_rank) : nullptr;
    float* nll = out->nll ? out->nll : need_nll ? e->at<float>(e->o_rep_nll) : nullptr;
    if (out->pred || rank || nll || out->topk_ids || out->topk_logprob || out->logits)
      TRY(plb_launch_masked_report_rows(e->at<float>(e->o_logm), 256, e->NP, e->at<int32_t>(e->o_tgt), n, topk, out->pred, rank,
                                        nll, out->topk_ids, out->topk_logprob, out->logits, s));
    // (threshold min(topk, NP): the rank NP of a NaN row never counts, also where the list is longer than the vocabulary)
    if (per_sample || out->totals)
      TRY(plb_launch_masked_report_samples(idx_offsets, B, rank, nll, topk < e->NP ? topk : e->NP, out->sample_loss,
                                           out->sample_top1, out->sample_topk, out->totals, s));
  }
  if (out->token_totals)
    TRY(plb_launch_token_top1(e->at<float>(e->o_tpmax), e->NTp / 256, e->at<float>(e->o_ttl), e->at<float>(e->o_tw),
                              (int)e->rep_tok_rows, e->at<int32_t>(e->o_rep_tok), out->token_totals, s));
  return 0;
}

// plb_token_report (include/plbert.h): what the token head predicts on the final hidden state of the last call that ran the
// encoder on every row — fin_x, the last slot of o_x (PlbEngine: fin_*; nothing but run_encoder writes o_x) — times the bf16
// copy of the token head, through the fused GEMM + top-k kernels of token_topk.hip: no logit is stored unless out->logits
// asks. Reads fin_*, the slot, the weight copy and the fp32 bias; writes the caller's buffers and the report's own regions
// (o_tr_*), and nothing else: no engine state changes, a live plb_encode stash stays live, the health word and the regions of
// plb_masked_report are left alone. Every refusal comes before the first launch.
extern "C" int plb_token_report(PlbEngine* e, const int32_t* lengths, const int32_t* idx_offsets, const int32_t* idx_flat,
                                int32_t n, int32_t B, int32_t S, const PlbPacking* packing, const int64_t* token_ids,
                                int32_t topk, const PlbTokenReport* out, void* stream) {
  if (!e || !e->ws) return fail("plb_token_report: engine not bound");
  if (!out) return fail("plb_token_report: out is null");
  if (!e->NT) return fail("plb_token_report: the engine has no token head (num_tokens = 0)");
  if (!e->fin_live) return fail("plb_token_report: no final hidden state to report on: %s", e->fin_dead_by);
  if (B != e->fin_B || S != e->fin_S)
    return fail("plb_token_report: batch %d x seq %d differs from the reported call's %d x %d", B, S, e->fin_B, e->fin_S);
  // the plan as the reported call executed it (pick_rows in engine_calls.cpp: a plan that packs nothing, or that the call
  // was told to ignore, ran padded)
  const bool packed = e->fin_row_start != nullptr;
  if (packed) {
    if (!packing || !packing->row_start || !lengths)
      return fail("plb_token_report: the reported call ran token-packed (%lld rows, %lld used): its lengths and packing plan are needed",
                  (long long)e->fin_rows, (long long)e->fin_used);
    if (packing->row_start != e->fin_row_start || packing->rows != e->fin_rows || packing->used != e->fin_used)
      return fail("plb_token_report: packing plan differs from the reported call's (%d rows, %d used; that call: %lld rows, %lld used)",
                  packing->rows, packing->used, (long long)e->fin_rows, (long long)e->fin_used);
  } else if (packing && packing->row_start && packing->rows > e->fin_rows) {
    return fail("plb_token_report: packing plan of %d rows exceeds the reported call's %lld", packing->rows, (long long)e->fin_rows);
  }
  if (topk < 0 || topk > PLB_TOPK_MAX) return fail("plb_token_report: topk %d outside [0, %d]", topk, PLB_TOPK_MAX);
  if ((out->target_logprob || out->target_pos || out->totals) && !token_ids)
    return fail("plb_token_report: %s wanted but token_ids is null", out->totals ? "totals" : "a target output");
  if (n < 0 || (int64_t)n > (int64_t)B * S) return fail("plb_token_report: n %d outside [0, %lld], the call's positions", n, (long long)B * S);
  if (!idx_offsets && (int64_t)n != (int64_t)B * S)
    return fail("plb_token_report: idx_offsets is null (every position), so n must be B*S = %lld, not %d", (long long)B * S, n);
  if (idx_offsets && n > 0 && !idx_flat) return fail("plb_token_report: idx_flat is null");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (out->totals) HIPTRY(hipMemsetAsync(out->totals, 0, 3 * sizeof(int32_t), s));
    return 0;
  }
  int32_t* rows = e->at<int32_t>(e->o_tr_rows);
  int32_t* tgt = e->at<int32_t>(e->o_tr_tgt);
  TRY(plb_launch_token_topk_prepare(idx_offsets, idx_flat, lengths, packed ? e->fin_row_start : nullptr, token_ids, n, B, S, rows,
                                    tgt, s));
  TRY(plb_launch_token_topk(e->fin_x, e->H, rows, n, e->wbf(PLB_TOK_W), e->H, e->par(PLB_TOK_B), e->NT, e->H, topk, 0,
                            e->at<char>(e->o_tr_scratch), token_ids ? tgt : nullptr, out->topk_ids, out->topk_logprob, out->lse,
                            out->target_logprob, out->target_pos, out->logits, out->totals, s));
  return 0;
}
