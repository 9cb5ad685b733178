// Launch plan of the NT GEMM family: THE place where a shape, a form and an operand kind become a kernel, a tile, a grid, a
// profiler class and a count of column-sum partial rows. Host only (no HIP): the launchers (gemm.hip, gemm_big.hip,
// gemm_fp8.hip, gemm_ln.hip, gemm_fp8_ln.hip) run what the plan says, the engine sizes and indexes its buffers from the same
// answer, tests and tools ask it too. What depends on a descriptor's POINTERS (null outputs, alignment) is the launchers'.
#pragma once
#include "prof_classes.h"   // PlbKernelClass: the plan names the class of a launch

#ifdef __cplusplus
extern "C" {
#endif

// form: the epilogue. 1 - 8 are the ACT numbers of the kernel templates (gemm_epilogue.h, gemm_nt_pipeline.h).
enum PlbGemmNTForm {
  PLB_NT_PLAIN = 0, PLB_NT_GELU = 1, PLB_NT_GELUBWD = 2,   // bf16 out (+bias, +residual); gelu_new stashing u; its backward from u
  PLB_NT_CE1 = 3, PLB_NT_CE2 = 4,                          // fused GEMM + cross-entropy passes (256-column tiles)
  PLB_NT_LNFWD = 5, PLB_NT_LNBWD = 6,                      // LayerNorm in the epilogue, forward / backward
  PLB_NT_GELUD = 7, PLB_NT_GELUDBWD = 8,                   // gelu_new stashing the derivative; its backward from the stash
  PLB_NT_F32 = 9                                           // fp32 out
};
enum PlbGemmNTOperands { PLB_NT_BF16 = 0, PLB_NT_FP8_E4M3 = 1, PLB_NT_FP8_E5M2 = 2 };   // fp8: 1-byte A and B, A's format
// opts: what of the descriptor's optional outputs and inputs the launch has (they change the bytes, colpart the kernel too)
enum PlbGemmNTOpts {
  PLB_NT_COLPART = 1,   // column-sum partials wanted (PlbGemmNT.colpart)
  PLB_NT_RES = 2,       // residual operand
  PLB_NT_C8 = 4,        // 1-byte image of the output
  PLB_NT_OUT16 = 8      // fp8 stash forms: the bf16 image of gelu(u) / dU leaves too
};

typedef struct {
  int rc;             // 0: runs; 3: no form for this shape (the caller takes another path); 1: refused
  int family;         // 0: small kernel (gemm.hip, 4 waves), 1: pipeline kernel (gemm_nt_pipeline.h, 8 waves)
  int tile;           // small: 128 / 64; pipeline: 256 = 256x256, 384 = 128x384, 1256 = 128x256
  int tile_m, tile_n; // rows x columns of a workgroup's output tile
  int kloop;          // pipeline: 1 interleaved K loop, 0 staggered; small: -1
  int grid, block;    // workgroups, threads per workgroup
  int cls;            // PlbKernelClass of the launch
  int colpart_rows;   // rows of column-sum partials the launch writes: 2 per row tile, 0: none
  double flops;       // 2 M N K
  double bytes;       // algorithmic HBM bytes: each operand and each output once (0: the cross-entropy passes are not priced)
} PlbGemmNTPlan;

// tile: 0 = the form's rule (and, for the forms of plb_launch_gemm_nt, the tuning hooks below); 256 / 384 / 1256 = that
// pipeline tile whatever the rule says (plb_launch_gemm_nt_big: bf16 operands, forms 0 - 4 and 9), rc 1 where the shape does
// not divide. Returns plan->rc. On rc != 0 every other field is 0.
// (The wrappers over it and the tuning hooks it reads — plb_gemm_nt_colpart_rows, plb_gemm_nt_fp8_gelud_tile_rows,
// plb_set_gemm_nt_tile, plb_set_gemm_nt_prefetch — are declared with the launchers in plbert_kernels.h.)
int plb_gemm_nt_plan(int M, int N, int K, int form, int operands, int opts, int tile, PlbGemmNTPlan* plan);

#ifdef __cplusplus
}
#endif
