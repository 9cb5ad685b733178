// Classes of the per-launch HIP-event profiler (engine_prof.cpp holds their names, in this order). A header of its own, free
// of HIP, so that host-only units (gemm_nt_plan.cpp) and the kernel interface (plbert_kernels.h) name the same classes.
#pragma once

enum PlbKernelClass {
  PLB_K_GEMM_NT = 0, PLB_K_GEMM_NT_GELU, PLB_K_GEMM_NT_GELUBWD, PLB_K_GEMM_NT_F32, PLB_K_GEMM_TN,
  PLB_K_ATTN_FWD, PLB_K_ATTN_BWD_DQ, PLB_K_ATTN_BWD_DKV, PLB_K_LN_FWD, PLB_K_LN_BWD, PLB_K_EMBED_FWD,
  PLB_K_EMBED_BWD, PLB_K_COLSUM, PLB_K_REDUCE, PLB_K_ROWS, PLB_K_CE, PLB_K_ADAMW, PLB_K_CAST, PLB_K_TOKEN_CE, PLB_K_GEMM_NT_CE, PLB_K_GEMM_NT_SMALL, PLB_K_FP8, PLB_K_ATTN_BWD,
  PLB_K_GEMM_NT_FP8, PLB_K_GEMM_NT_GELU_FP8, PLB_K_GEMM_NT_GELUBWD_FP8,  // the fp8 launches: priced against the fp8 MFMA peak
  PLB_K_GEMM_NT_LNFWD, PLB_K_GEMM_NT_LNBWD,  // GEMM + LayerNorm epilogue (gemm_ln.hip)
  PLB_K_GEMM_NT_LNFWD_FP8, PLB_K_GEMM_NT_LNBWD_FP8, PLB_K_GEMM_TN_FP8,  // fp8 forms of the same, and of the weight-gradient GEMM
  PLB_K_NCLASS
};
