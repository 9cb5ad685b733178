// LayerNorm fused into the epilogue of the GEMM that produces its input (gemm_nt_pipeline.h, ACT 5 / 6; shapes and tiles are
// the plan's, gemm_nt_plan.h; the argument checks its launchers share are nt_args_check there): the dense and
// FFN-output projections of the shared layer (forward: AlbertAttention.LayerNorm / full_layer_layer_norm,
// modeling_albert.py:196-200, 225-238) and the two dX GEMMs whose output is the gradient of a LayerNorm's output
// (backward). A translation unit of its own so that the plain instantiations keep their register allocation.
#include "gemm_nt_pipeline.h"

static int g_ln_fault_mode = 0, g_ln_fault_launches = 0;
extern "C" void plb_debug_ln_fault(int mode, int launches) { g_ln_fault_mode = mode; g_ln_fault_launches = launches; }
extern "C" int plb_ln_fault_take(void) {
  if (g_ln_fault_launches <= 0) return 0;
  --g_ln_fault_launches;
  return g_ln_fault_mode;
}

// 3: a shape these forms do not take (the caller runs the GEMM and the LayerNorm kernel), reported before a bad argument (1)
extern "C" int plb_launch_gemm_nt_ln(const PlbGemmNT* p_in, int mode, hipStream_t stream) {
  PlbGemmNT q_ = *p_in;
  q_.ln_fault = plb_ln_fault_take();   // (consumed by a launch that is then refused, too)
  const PlbGemmNT* p = &q_;
  if (mode != PLB_NT_LNFWD && mode != PLB_NT_LNBWD) return 1;
  PlbGemmNTPlan pl;
  if (plb_gemm_nt_plan(p->M, p->N, p->K, mode, PLB_NT_BF16, p->res ? PLB_NT_RES : 0, 0, &pl)) return pl.rc;
  if (nt_args_check(p, mode, false)) return 1;
  const dim3 grid(pl.grid), block(pl.block);
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  if (pl.tile == 384) {
    if (mode == PLB_NT_LNFWD) hipLaunchKernelGGL((gemm_nt_big_kernel<3, 5, false, true>), grid, block, 0, stream, *p);
    else hipLaunchKernelGGL((gemm_nt_big_kernel<3, 6, false, true>), grid, block, 0, stream, *p);
  } else {
    if (mode == PLB_NT_LNFWD) hipLaunchKernelGGL((gemm_nt_big_kernel<1, 5, false, true>), grid, block, 0, stream, *p);
    else hipLaunchKernelGGL((gemm_nt_big_kernel<1, 6, false, true>), grid, block, 0, stream, *p);
  }
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// gelu_new epilogues that stash the DERIVATIVE (forms 7 / 8 of gemm_nt_pipeline.h): FFN up-projection forward
// C = gelu_new'(u), C2 = gelu_new(u) with u = A·B^T + bias (modeling_albert.py:225-232, activations.py:59-66), and the
// matching backward C = (A·B^T) * aux with aux = that stash (+ column-sum partials = the FFN bias gradient). 256x256 tiles;
// returns 3 for other shapes: the caller then uses forms 1 / 2 (which stash u) for BOTH.
extern "C" int plb_launch_gemm_nt_gelud(const PlbGemmNT* p, int backward, hipStream_t stream) {
  const int form = backward ? PLB_NT_GELUDBWD : PLB_NT_GELUD;
  PlbGemmNTPlan pl;
  if (plb_gemm_nt_plan(p->M, p->N, p->K, form, PLB_NT_BF16, p->colpart ? PLB_NT_COLPART : 0, 0, &pl)) return pl.rc;
  if (nt_args_check(p, form, false)) return 1;
  const dim3 grid(pl.grid), block(pl.block);
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  if (backward) hipLaunchKernelGGL((gemm_nt_big_kernel<2, 8, false, true>), grid, block, 0, stream, *p);
  else if (p->colpart) hipLaunchKernelGGL((gemm_nt_big_kernel<2, 7, false, true>), grid, block, 0, stream, *p);
  else hipLaunchKernelGGL((gemm_nt_big_kernel<2, 7, false, true, false, false, true>), grid, block, 0, stream, *p);
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
