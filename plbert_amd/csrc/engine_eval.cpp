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
