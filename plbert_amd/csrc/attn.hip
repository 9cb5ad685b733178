// Fused multi-head attention for the shared ALBERT layer, head_dim 64, gfx950.
// Restates AlbertAttention's softmax(q·k^T·d^-0.5 + key_padding_mask)·v (modeling_albert.py:110-135,
// 166-200) as a flash-style single pass: scores never leave registers.
//
// Forward, one workgroup = 4 waves = 128 query rows of one (batch, head); a wave owns 32 queries.
//   S^T[key][q] = K·Q^T  (MFMA 32x32x16, K rows from LDS, Q fragments in registers) puts one query
//   per lane, so the row max / row sum are lane-local (+ one exchange with lane^32).  The S^T
//   accumulator converted to bf16 is directly the B operand of O^T[dv][q] = V^T·P^T (accumulator-as-
//   operand, k order 16s+8(j>>2)+4h+(j&3)); V^T fragments come from ds_read_b64_tr_b16 on a
//   [4 keys][32 dv] sub-tiled LDS image (each half-wave read = one 256-B bank row).
// Backward, two kernels that recompute P from the saved log-sum-exp:
//   dq kernel  (same tiling as forward): dS^T = P^T∘(dP^T - delta), dQ^T = K^T·dS^T ; also writes delta.
//   dkv kernel (a wave owns 32 keys, loops over query tiles): dV^T = dO^T·P, dK^T = Q^T·dS.
// Key padding comes from lengths[b]; whole key tiles past the length are skipped.
// Key masks (PlbAttn.key_words): the kernels live in attn_kernels.h, which is compiled twice. ATTN_KM 0 is the code as it
// always was; ATTN_KM 1 takes the valid keys from one bit per key — the words of the sample's row sit one per lane
// (S <= 2048) and a tile gets its two words by v_readlane — so that a tile of all-ones words pays two scalar compares.
// Which kernels a call gets, on what grid, and the form of its backward: attn_plan.h.
#include "attn_common.h"
#include "row_common.h"

namespace {

#define ATTN_KM 0
#define ATTN_KERNEL(name) name##_kernel
#include "attn_kernels.h"
#undef ATTN_KM
#undef ATTN_KERNEL
#define ATTN_KM 1
#define ATTN_KERNEL(name) name##_km_kernel
#include "attn_kernels.h"
#undef ATTN_KM
#undef ATTN_KERNEL

}  // namespace


// The one argument check of the attention launchers (plbert_kernels.h); host code, runs before any HIP call.
extern "C" int plb_attn_args_check(const PlbAttn* p, int direction) {
  if (!p || direction < PLB_ATTN_FWD || direction > PLB_ATTN_PROBS) return 1;
  PlbAttnPlan pl;   // B, S, NH >= 1, a grid below 2^31, key masks with S <= 2048 and without compact queries
  if (plb_attn_plan(p->B, p->S, p->NH, plb_attn_flags(p), &pl)) return 1;
  if (p->H != (int64_t)p->NH * 64 || !p->qkv || !p->lse || p->ldqkv % 8) return 1;
  if ((int64_t)p->S * p->ldqkv * 2 >= ((int64_t)1 << 32)) return 1;   // (the staging's 32-bit byte offsets count from the sample's first row)
  if (p->row_start && !p->lengths) return 1;   // token-packed rows are defined by the lengths
  if (p->key_words && p->ldkw < 2 * ((p->S + 63) / 64)) return 1;   // the row has two words per 64-key tile
  if (direction == PLB_ATTN_PROBS) return 0;
  if (!p->ctx || p->ldctx % 8) return 1;
  if (p->qoff && (!p->q || p->ldq % 8 || p->nq_total < 0)) return 1;
  if (direction == PLB_ATTN_FWD) return p->ctx8 && (!p->ctx_scale || p->ldctx8 % 8);
  if (!p->dctx || p->lddctx % 8 || p->lddqkv % 8 || (!p->dqkv && !p->dqkv8) || (p->dqkv8 && (!p->dqkv_scale || p->lddqkv8 % 8))) return 1;
  if (p->qoff && ((!p->dq && !p->dq8) || (p->dq && p->lddq % 8) || (p->dq8 && p->lddq8 % 8))) return 1;
  // the single kernel owns every key of a (batch, head) in one workgroup and has no masked or compact form; bf16 rows AND the
  // image would need 4 more registers than the file has
  return direction == PLB_ATTN_BWD_SINGLE && (p->S > 512 || p->key_words || p->qoff || (p->dqkv && p->dqkv8));
}

extern "C" int plb_launch_attn_fwd(const PlbAttn* p, hipStream_t stream) {
  if (plb_attn_args_check(p, PLB_ATTN_FWD)) return 1;
  PlbAttnPlan pl;
  plb_attn_plan(p->B, p->S, p->NH, plb_attn_flags(p), &pl);
  ProfScope ps(pl.cls_fwd, stream, pl.fwd_flops, pl.fwd_bytes);
  if (pl.km) hipLaunchKernelGGL(attn_fwd_km_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
  else hipLaunchKernelGGL(attn_fwd_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
  return LAUNCH_OK();
}

static int launch_attn_bwd_two(const PlbAttn* p, hipStream_t stream) {
  PlbAttnPlan pl;
  plb_attn_plan(p->B, p->S, p->NH, plb_attn_flags(p), &pl);
  {
    ProfScope ps(pl.cls_bwd_dq, stream, pl.bwd_flops / 2, pl.bwd_bytes);
    if (pl.km) hipLaunchKernelGGL(attn_bwd_dq_km_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
    else hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
  }
  ProfScope ps(pl.cls_bwd_dkv, stream, pl.bwd_flops / 2, pl.bwd_bytes);
  if (pl.km) hipLaunchKernelGGL(attn_bwd_dkv_km_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
  else hipLaunchKernelGGL(attn_bwd_dkv_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, *p);
  return LAUNCH_OK();
}
// samples [b0, b0 + nb) of a call as a call of their own; pl: the plan of the whole call
static PlbAttn attn_samples(const PlbAttn* p, const PlbAttnPlan& pl, int b0, int nb) {
  PlbAttn q = *p;
  const size_t t0 = (size_t)b0 * p->S, stat0 = (size_t)b0 * (size_t)(pl.stat_floats / p->B);
  q.B = nb;
  q.lse = p->lse + stat0;
  if (p->delta) q.delta = p->delta + stat0;
  if (p->colpart) q.colpart = p->colpart + (size_t)b0 * pl.colpart_sample_rows * (3 * p->H);
  if (p->lengths) q.lengths = p->lengths + b0;
  if (p->key_words) q.key_words = p->key_words + (size_t)b0 * p->ldkw;
  if (p->row_start) {   // token-packed rows: the table holds absolute rows, so the row pointers stay where they are
    q.row_start = p->row_start + b0;
    return q;
  }
  q.qkv = p->qkv + t0 * p->ldqkv;
  q.ctx = p->ctx + t0 * p->ldctx;
  q.dctx = p->dctx + t0 * p->lddctx;
  if (p->dqkv) q.dqkv = p->dqkv + t0 * p->lddqkv;
  if (p->dqkv8) q.dqkv8 = p->dqkv8 + t0 * p->lddqkv8;
  return q;
}

extern "C" int plb_launch_attn_bwd(const PlbAttn* p, hipStream_t stream) {
  if (plb_attn_args_check(p, PLB_ATTN_BWD)) return 1;
  PlbAttnPlan pl;
  plb_attn_plan(p->B, p->S, p->NH, plb_attn_flags(p), &pl);
  if (pl.bwd_form == PLB_ATTN_BWD_TWO) return launch_attn_bwd_two(p, stream);
  if (pl.bwd_form == PLB_ATTN_BWD_ONE) return plb_launch_attn_bwd_fused(p, stream);
  const PlbAttn a = attn_samples(p, pl, 0, pl.bwd_one_samples), b = attn_samples(p, pl, pl.bwd_one_samples, p->B - pl.bwd_one_samples);
  if (const int rc = plb_launch_attn_bwd_fused(&a, stream)) return rc;
  return launch_attn_bwd_two(&b, stream);
}
