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
#include "attn_common.h"
#include <stdlib.h>
#include <string.h>

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

static int check_attn(const PlbAttn* p) {
  if (p->H != p->NH * 64 || p->S < 1 || p->B < 1) return 1;
  if (p->row_start && !p->lengths) return 1;   // token-packed rows are defined by the lengths
  if (p->ldqkv % 8 || p->ldctx % 8) return 1;
  // key masks: one word per lane holds a sample's row (S <= 2048), the row has two words per 64-key tile; no compact queries
  if (p->key_words && (p->S > 2048 || p->ldkw < 2 * ((p->S + 63) / 64) || p->qoff)) return 1;
  return 0;
}

extern "C" int plb_launch_attn_fwd(const PlbAttn* p, hipStream_t stream) {
  if (check_attn(p) || (p->ctx8 && (!p->ctx_scale || p->ldctx8 % 8))) return 1;
  if (p->qoff && (!p->q || p->ldq % 8 || p->nq_total < 0)) return 1;
  dim3 grid(((p->S + 127) / 128) * p->NH * p->B), block(256);
  const double unit = (double)p->B * p->NH * (double)p->S * p->S * 64.0;
  const double io = 2.0 * p->B * p->S * (double)p->H;
  const int tok = plb_prof_begin(PLB_K_ATTN_FWD, stream, 4.0 * unit, 4.0 * io);
  if (p->key_words) hipLaunchKernelGGL(attn_fwd_km_kernel, grid, block, 0, stream, *p);
  else hipLaunchKernelGGL(attn_fwd_kernel, grid, block, 0, stream, *p);
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Two forms of the backward. The two-kernel form (dQ kernel + dK/dV kernel, any S) runs 4 workgroups per CU and packs
// any grid; the single-kernel form (attn_bwd_fused.hip, S <= 512: five products instead of seven, one exponential pass)
// needs a whole CU per (batch, head), so it pays only where B x heads fills the 256 CUs in (nearly) whole rounds —
// measured (profiles/r03_attn_bwd_fused_vs_split.txt, r05_attn_bwd_policy_ab.txt): 16 x 16 heads = exactly one round: 74-78
// vs 83 us per launch, -0.35 ms per step at config D (bf16; fp8 -0.23); 32 x 12 = 1.5 rounds: 143-149 vs 127 us.
// Policy per call (PLBERT_ATTN_BWD = fused | split | auto | hybrid, default auto; plb_set_attn_bwd_fused(1 / 0 / -1 / 2)):
//   auto:   S in (384, 512] and the last round of B x heads at least 90 % full -> fused; everything else -> two kernels.
//           An fp8 call that needs bf16 rows AND the image -> two kernels.
//   hybrid: as auto, and a batch with at least one (nearly) full round of whole samples plus a short remainder is split
//           BY SAMPLE: floor(256 / heads) samples per round to the fused kernel, the rest to the two kernels. Built and
//           measured in round 5 at config A (21 + 11 samples): +0.26 ms per step in bf16, +0.30 in fp8 — the remainder's
//           528 short workgroups cost 70 us, not the 44 their share of the full grid suggests. Off; kept for the record.
static int g_bwd_fused = -2;   // -2: read the environment; -1 auto, 0 split, 1 fused, 2 auto + hybrid
extern "C" void plb_set_attn_bwd_fused(int on) { g_bwd_fused = on < 0 ? -1 : (on > 2 ? 1 : on); }
static int launch_attn_bwd_split(const PlbAttn* p, hipStream_t stream) {
  dim3 grid(((p->S + 127) / 128) * p->NH * p->B), block(256);
  // algorithmic work of the backward = 4 products (dP, dQ, dV, dK); the S recomputation in each
  // kernel and the second dP are not credited
  const double unit = (double)p->B * p->NH * (double)p->S * p->S * 64.0;
  const double io = 2.0 * p->B * p->S * (double)p->H;
  int tok = plb_prof_begin(PLB_K_ATTN_BWD_DQ, stream, 4.0 * unit, 6.0 * io);
  if (p->key_words) hipLaunchKernelGGL(attn_bwd_dq_km_kernel, grid, block, 0, stream, *p);
  else hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, block, 0, stream, *p);
  plb_prof_end(tok, stream);
  tok = plb_prof_begin(PLB_K_ATTN_BWD_DKV, stream, 4.0 * unit, 6.0 * io);
  if (p->key_words) hipLaunchKernelGGL(attn_bwd_dkv_km_kernel, grid, block, 0, stream, *p);
  else hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, block, 0, stream, *p);
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// samples [b0, b0 + nb) of a call as a call of their own
static PlbAttn attn_samples(const PlbAttn* p, int b0, int nb) {
  PlbAttn q = *p;
  const size_t t0 = (size_t)b0 * p->S;
  q.B = nb;
  q.qkv = p->qkv + t0 * p->ldqkv;
  q.ctx = p->ctx + t0 * p->ldctx;
  q.dctx = p->dctx + t0 * p->lddctx;
  if (p->dqkv) q.dqkv = p->dqkv + t0 * p->lddqkv;
  if (p->dqkv8) q.dqkv8 = p->dqkv8 + t0 * p->lddqkv8;
  if (p->lengths) q.lengths = p->lengths + b0;
  q.lse = p->lse + (size_t)b0 * p->NH * p->S;
  if (p->delta) q.delta = p->delta + (size_t)b0 * p->NH * p->S;
  if (p->colpart) q.colpart = p->colpart + (size_t)b0 * ((p->S + 127) / 128) * 4 * (3 * p->H);
  if (p->key_words) q.key_words = p->key_words + (size_t)b0 * p->ldkw;
  if (p->row_start) {   // token-packed rows: the table holds absolute rows, so the row pointers stay where they are
    q.row_start = p->row_start + b0;
    q.qkv = p->qkv; q.ctx = p->ctx; q.dctx = p->dctx; q.dqkv = p->dqkv; q.dqkv8 = p->dqkv8;
  }
  return q;
}

extern "C" int plb_launch_attn_bwd(const PlbAttn* p, hipStream_t stream) {
  if (check_attn(p) || p->lddctx % 8 || p->lddqkv % 8 || (!p->dqkv && !p->dqkv8) || (p->dqkv8 && (!p->dqkv_scale || p->lddqkv8 % 8))) return 1;
  if (g_bwd_fused == -2) {
    const char* e = getenv("PLBERT_ATTN_BWD");
    g_bwd_fused = (e && !strcmp(e, "fused")) ? 1 : (e && !strcmp(e, "split")) ? 0 : (e && !strcmp(e, "hybrid")) ? 2 : -1;
  }
  const bool hybrid_on = g_bwd_fused == 2;
  if (p->qoff && (!p->q || p->ldq % 8 || p->nq_total < 0 || (!p->dq && !p->dq8) || (p->dq && p->lddq % 8) || (p->dq8 && p->lddq8 % 8))) return 1;
  // (compact queries, key masks: the two-kernel form only, whatever the policy says)
  const bool can_fuse = p->S <= 512 && !(p->dqkv && p->dqkv8) && !p->qoff && !p->key_words;
  if (!can_fuse || g_bwd_fused == 0) return launch_attn_bwd_split(p, stream);
  if (g_bwd_fused == 1) return plb_launch_attn_bwd_fused(p, stream);
  if (p->S <= 384) return launch_attn_bwd_split(p, stream);
  const int items = p->B * p->NH, rounds = (items + 255) / 256;
  if (items * 10 >= rounds * 256 * 9) return plb_launch_attn_bwd_fused(p, stream);
  // hybrid: whole samples worth (nearly) full rounds to the fused kernel, the rest to the two kernels
  const int per_round = 256 / p->NH;                      // samples whose (batch, head) items fit one round
  const int full = per_round > 0 ? (p->B / per_round) : 0; // full rounds available
  const int nb_f = full * per_round, rest = p->B - nb_f;
  if (hybrid_on && full >= 1 && per_round * p->NH * 10 >= 256 * 9 && rest * p->NH <= 160) {
    const PlbAttn a = attn_samples(p, 0, nb_f);
    const int rc = plb_launch_attn_bwd_fused(&a, stream);
    if (rc || rest == 0) return rc;
    const PlbAttn b = attn_samples(p, nb_f, rest);
    return launch_attn_bwd_split(&b, stream);
  }
  return launch_attn_bwd_split(p, stream);
}
