// fp8 (OCP e4m3 weights; e4m3 activations or e5m2 gradients) instantiations of the NT pipeline GEMM (BASELINE.json
// configs[4]: "fp8 (e4m3) MFMA path for QKV/FFN GEMMs"). Same kernel template as the bf16 build (gemm_nt_pipeline.h): a
// K-tile of 128-byte rows holds 128 k, one block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales replaces
// two bf16 MFMAs (twice the MFMA rate at the same LDS-DMA instruction count per K-tile row: half per FLOP), fp32
// accumulation, per-tensor dequantisation in the epilogue. A translation unit of its own so that the bf16
// instantiations keep their register allocation (co-compiled template variants perturb each other).
#include "gemm_nt_pipeline.h"

namespace {

// Tiles: 128x384 (N % 384 == 0, plain epilogue) and 128x256. The 256x256 tile is not built in fp8: its 128
// accumulators + 96 registers of 8-register operand tuples do not fit 256 VGPRs without spilling, and at one byte per
// element the 128x256 tile already moves fewer operand bytes per flop (170 FLOP/B) than the bf16 256x256 tile (128).
template <int V, int ACT, bool ABF8>
void launch_fp8(const PlbGemmNT* p, const PlbGemmNTPlan& pl, hipStream_t stream) {
  hipLaunchKernelGGL((gemm_nt_big_kernel<V, ACT, false, true, true, ABF8>), dim3(pl.grid), dim3(pl.block), 0, stream, *p);
}
template <bool ABF8>
void dispatch(const PlbGemmNT* p, const PlbGemmNTPlan& pl, int act, hipStream_t stream) {
  if (act == 0 && pl.tile == 384) launch_fp8<3, 0, ABF8>(p, pl, stream);
  else if (act == 0) launch_fp8<1, 0, ABF8>(p, pl, stream);
  else if (act == 1) launch_fp8<1, 1, ABF8>(p, pl, stream);
  else launch_fp8<1, 2, ABF8>(p, pl, stream);
}

}  // namespace

// 3: a shape without an fp8 form (the caller runs the bf16 GEMM)
extern "C" int plb_launch_gemm_nt_fp8(const PlbGemmNT* p, int act, int a_bf8, hipStream_t stream) {
  const bool known = act >= 0 && act <= 2;   // (another act is refused behind the shape, as a form with an epilogue)
  PlbGemmNTPlan pl;
  const int opts = (p->colpart ? PLB_NT_COLPART : 0) | (p->res ? PLB_NT_RES : 0) | (p->C8 ? PLB_NT_C8 : 0);
  if (plb_gemm_nt_plan(p->M, p->N, p->K, known ? act : PLB_NT_GELU, a_bf8 ? PLB_NT_FP8_E5M2 : PLB_NT_FP8_E4M3, opts, 0, &pl))
    return pl.rc;
  if (!known || nt_args_check(p, act, true)) return 1;
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  if (a_bf8) dispatch<true>(p, pl, act, stream);
  else dispatch<false>(p, pl, act, stream);
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
