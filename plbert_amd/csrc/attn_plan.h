// Launch plan of the attention kernels (attn.hip, attn_bwd_fused.hip, the probabilities of layer_outputs.hip): THE place where
// a batch, a sequence length, a head count and the modes of a call become a grid, a kernel variant, the form of the backward,
// the partial rows of the Q/K/V bias gradient and the profiler's credit. Host only (no HIP), like gemm_nt_plan.h and
// gemm_tn_plan.h. The launchers run what the plan says, the engine sizes and indexes its buffers and places its clears by the
// same answer, tests and tools ask it too. What depends on a descriptor's POINTERS and row strides is plb_attn_args_check's
// (plbert_kernels.h).
#pragma once
#include <stdint.h>

#include "prof_classes.h"   // PlbKernelClass: the plan names the classes of its launches

#ifdef __cplusplus
extern "C" {
#endif

enum PlbAttnFlags {
  PLB_ATTN_PACKED = 1,      // token-packed rows (PlbAttn.row_start)
  PLB_ATTN_KEYMASK = 2,     // key masks (PlbAttn.key_words): the _km kernels
  PLB_ATTN_COMPACT = 4,     // compact queries (PlbAttn.qoff)
  PLB_ATTN_OUT_ROWS = 8,    // backward: dQKV leaves as bf16 rows (PlbAttn.dqkv)
  PLB_ATTN_OUT_IMAGE = 16   // backward: dQKV leaves as its e5m2 image (PlbAttn.dqkv8)
};
enum PlbAttnBwdForm {
  PLB_ATTN_BWD_TWO = 0,     // dQ kernel + dK/dV kernel (attn.hip): any S, every mode
  PLB_ATTN_BWD_ONE = 1,     // the single kernel (attn_bwd_fused.hip): S <= 512, one workgroup per (sample, head)
  PLB_ATTN_BWD_HYBRID = 2   // the first bwd_one_samples samples to the single kernel, the rest to the two kernels
};

typedef struct {
  int rc;                   // 0: runs; 1: refused (no launch takes the shape with these modes)
  int grid, block;          // forward, two-kernel backward, probabilities: ceil(S/128) * NH * B workgroups of 256 threads
  int km;                   // 1: the _km kernel variants (key masks)
  int bwd_form;             // PlbAttnBwdForm under the policy in force
  int bwd_one_samples;      // leading samples the single kernel takes: B (one), 0 (two), in between (hybrid)
  int bwd_one_grid;         // its workgroups: NH * bwd_one_samples
  int colpart_rows;         // Q/K/V bias partial rows the backward writes: B * ceil(S/128) * 4 ...
  int colpart_sample_rows;  // ... of which one sample owns ceil(S/128) * 4 consecutive ones
  int unwritten_rows;       // 1: rows at or past position S of a sample's packed slot are written by NO attention launch
                            // (packed and S % 128 != 0: the slot of a full-length sample runs on to the next multiple of 128)
  int cls_fwd, cls_bwd_dq, cls_bwd_dkv, cls_bwd_one;   // PlbKernelClass of each launch
  int64_t stat_floats;      // floats of lse, and of delta: B * NH * S (compact queries: [NH][nq_total], the caller's count)
  double fwd_flops, fwd_bytes;          // credit of the forward launch
  double bwd_flops, bwd_bytes;          // credit of the backward: the single kernel takes both; each of the two kernels is
                                        // credited bwd_flops / 2 and bwd_bytes
} PlbAttnPlan;

// flags: PlbAttnFlags. Returns plan->rc; on rc != 0 every other field is 0. Refused: B, S or NH < 1, a key mask with
// S > 2048 or with compact queries, a grid or a partial-row count of 2^31 or more.
// The form of the backward follows the policy state of this unit: plb_set_attn_bwd_fused (plbert_kernels.h) or, until its
// first call, PLBERT_ATTN_BWD = fused | split | auto | hybrid, read once per process (attn_plan.cpp).
int plb_attn_plan(int B, int S, int NH, int flags, PlbAttnPlan* plan);

#ifdef __cplusplus
}
#endif
