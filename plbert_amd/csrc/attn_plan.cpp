// The launch plan of the attention kernels (attn_plan.h) and the policy state of the backward's form. Plain C++: no HIP, no
// device code.
#include "attn_plan.h"

#include <stdlib.h>
#include <string.h>

// Two forms of the backward. The two-kernel form (dQ kernel + dK/dV kernel, any S) runs 4 workgroups per CU and packs any
// grid; the single-kernel form (attn_bwd_fused.hip, S <= 512: five products instead of seven, one exponential pass) needs a
// whole CU per (batch, head), so it pays only where B x heads fills the 256 CUs in (nearly) whole rounds — measured
// (profiles/r03_attn_bwd_fused_vs_split.txt, r05_attn_bwd_policy_ab.txt): 16 x 16 heads = exactly one round: 74-78 vs 83 us
// per launch, -0.35 ms per step at config D (bf16; fp8 -0.23); 32 x 12 = 1.5 rounds: 143-149 vs 127 us.
// Policy (PLBERT_ATTN_BWD = fused | split | auto | hybrid, default auto; plb_set_attn_bwd_fused(1 / 0 / -1 / 2)):
//   split:  two kernels. fused: the single kernel wherever it exists (S <= 512).
//   auto:   S in (384, 512] and the last round of B x heads at least 90 % full -> single kernel; everything else -> two.
//   hybrid: as auto, and a batch with at least one (nearly) full round of whole samples plus a short remainder is split
//           BY SAMPLE: floor(256 / heads) samples per round to the single kernel, the rest to the two kernels. Built and
//           measured in round 5 at config A (21 + 11 samples): +0.26 ms per step in bf16, +0.30 in fp8 — the remainder's
//           528 short workgroups cost 70 us, not the 44 their share of the full grid suggests. Off; kept for the record.
// Whatever the policy: key masks, compact queries and a call that needs bf16 rows AND the image (4 registers more than the
// single kernel's file has) take the two kernels.
static int g_policy = -2;   // -2: read the environment; -1 auto, 0 split, 1 fused, 2 auto + hybrid
extern "C" void plb_set_attn_bwd_fused(int on) { g_policy = on < 0 ? -1 : (on > 2 ? 1 : on); }
static int policy() {
  if (g_policy == -2) {
    const char* e = getenv("PLBERT_ATTN_BWD");
    g_policy = (e && !strcmp(e, "fused")) ? 1 : (e && !strcmp(e, "split")) ? 0 : (e && !strcmp(e, "hybrid")) ? 2 : -1;
  }
  return g_policy;
}

// leading samples of the call that the single kernel takes
static int bwd_one_samples(int B, int S, int NH, int flags) {
  const bool both = (flags & PLB_ATTN_OUT_ROWS) && (flags & PLB_ATTN_OUT_IMAGE);
  const bool can = S <= 512 && !both && !(flags & (PLB_ATTN_COMPACT | PLB_ATTN_KEYMASK));
  const int pol = policy();
  if (!can || pol == 0) return 0;
  if (pol == 1) return B;
  if (S <= 384) return 0;
  const int64_t items = (int64_t)B * NH, rounds = (items + 255) / 256;
  if (items * 10 >= rounds * 256 * 9) return B;
  // hybrid: whole samples worth (nearly) full rounds to the single kernel, the rest to the two kernels
  const int per_round = 256 / NH;                            // samples whose (batch, head) items fit one round
  const int full = per_round > 0 ? B / per_round : 0;        // full rounds available
  const int rest = B - full * per_round;
  if (pol == 2 && full >= 1 && per_round * NH * 10 >= 256 * 9 && (int64_t)rest * NH <= 160) return full * per_round;
  return 0;
}

extern "C" int plb_attn_plan(int B, int S, int NH, int flags, PlbAttnPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  if (B < 1 || S < 1 || NH < 1) return plan->rc = 1;
  // key masks: one word per lane holds a sample's row (64 lanes x 32 keys); no compact queries
  if ((flags & PLB_ATTN_KEYMASK) && (S > 2048 || (flags & PLB_ATTN_COMPACT))) return plan->rc = 1;
  const int64_t qt = ((int64_t)S + 127) / 128;
  // qt * NH * B and qt * 4 * B as a launch's grid and an int hold them (qt <= 2^24, so no product below overflows)
  if (qt * NH > 0x7fffffffLL / B || qt * 4 > 0x7fffffffLL / B) return plan->rc = 1;
  plan->grid = (int)(qt * NH * B);
  plan->block = 256;
  plan->km = (flags & PLB_ATTN_KEYMASK) != 0;
  const int n1 = bwd_one_samples(B, S, NH, flags);
  plan->bwd_form = n1 == 0 ? PLB_ATTN_BWD_TWO : n1 == B ? PLB_ATTN_BWD_ONE : PLB_ATTN_BWD_HYBRID;
  plan->bwd_one_samples = n1;
  plan->bwd_one_grid = NH * n1;
  plan->colpart_rows = (int)(qt * 4 * B);
  plan->colpart_sample_rows = (int)(qt * 4);
  plan->unwritten_rows = (flags & PLB_ATTN_PACKED) && S % 128 != 0;
  plan->cls_fwd = PLB_K_ATTN_FWD; plan->cls_bwd_dq = PLB_K_ATTN_BWD_DQ; plan->cls_bwd_dkv = PLB_K_ATTN_BWD_DKV;
  plan->cls_bwd_one = PLB_K_ATTN_BWD;
  plan->stat_floats = (int64_t)B * NH * S;
  // algorithmic work: forward 2 products (S, O), backward 4 (dP, dQ, dV, dK); the recomputation of S in the backward
  // kernels and the second dP of the two-kernel form are not credited. Bytes: Q, K, V, O rows once; the backward 6 row sets.
  const double unit = (double)B * NH * (double)S * S * 64.0;
  const double io = 2.0 * B * S * ((double)NH * 64.0);
  plan->fwd_flops = 4.0 * unit; plan->fwd_bytes = 4.0 * io;
  plan->bwd_flops = 8.0 * unit; plan->bwd_bytes = 6.0 * io;
  return 0;
}
