// Launch plan of the token-major ("TN") weight-gradient GEMMs, dW[N,K] = A[Mtot,Ncols]^T · B[Mtot,K]: THE place where a
// shape and an operand kind become a kernel, a count of row splits, a grid and the size of the fp32 slab the splits write.
// Host only (no HIP), like gemm_nt_plan.h. The engine's weight_grad runs what the plan says and plb_create sizes the slabs
// from the same answer; tests and tools ask it too. The launchers (gemm_tn.hip, gemm_tn_fp8.hip) keep their signatures
// and their own argument checks: they run whatever splits a caller hands them.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum PlbGemmTNOperands { PLB_TN_BF16 = 0, PLB_TN_FP8 = 1 };   // fp8: A = e5m2 image, B = e4m3 image, 1 byte per element
enum PlbGemmTNKernel {
  PLB_TN_SMALL = 0,      // gemm_tn_kernel: 128x128 tiles, grid (tiles, splits)
  PLB_TN_PIPELINE = 1,   // gemm_tn_big_kernel: 256x256 tiles on the LDS-DMA pipeline, grid tiles * splits
  PLB_TN_PIPELINE_FP8 = 2   // gemm_tn_fp8_kernel: the same on 1-byte images
};

typedef struct {
  int rc;               // 0: runs; 1: refused (no kernel takes the shape)
  int kernel;           // PlbGemmTNKernel
  int splits;           // row splits: one fp32 slab [N, K] each
  int rows_per_split;   // a multiple of the kernel's K-tile (64 rows, fp8 128); splits * rows_per_split >= Mtot
  int direct;           // splits == 1 && N == Ncols: the kernel writes the output itself, no slab and no reduce
  int grid_x, grid_y, block;
  int64_t slab_floats;  // 0 when direct, else splits * N * K
  double flops;         // 2 Mtot N K
} PlbGemmTNPlan;

// Ncols: readable columns of A (the row width the kernel may stage), N <= Ncols: rows of dW that are stored (the phoneme
// head reads 256 columns and stores NP rows). Returns plan->rc; on rc != 0 every other field is 0.
// Environment, read once per process: PLBERT_TN_SPLITS, PLBERT_TN_CUS (gemm_tn_plan.cpp).
int plb_gemm_tn_plan(int64_t Mtot, int Ncols, int N, int K, int operands, PlbGemmTNPlan* plan);

#ifdef __cplusplus
}
#endif
