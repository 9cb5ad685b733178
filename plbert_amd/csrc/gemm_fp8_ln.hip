// fp8-operand instantiations of the LayerNorm-in-epilogue forms (5 / 6) and of the gelu-derivative-stash forms (7 / 8) of
// the NT pipeline GEMM (gemm_nt_pipeline.h): what lets a call in fp8 mode (BASELINE.json configs[4]) keep the fusions of the
// bf16 path — dense and FFN-output projections with their LayerNorm (modeling_albert.py:196-200, 225-238), the two dX GEMMs
// that carry a LayerNorm backward, FFN up-projection + gelu_new (activations.py:59-66) and its backward — while every operand
// is a 1-byte image. Each launch also WRITES the 1-byte image (+ running maximum) of its output for the fp8 GEMMs that read
// it next: the following projection and, at the end of the backward, the token-major weight-gradient GEMM.
// LayerNorm forms: 128-row tiles (128x384 for N % 384 == 0, else 128x256); gelu forms: 256x256 where M allows — the plan's
// rules (gemm_nt_plan.h). A translation unit of its own: co-compiled template variants perturb each other's register allocation.
#include "gemm_nt_pipeline.h"

namespace {
template <int V, int ACT, bool NOCS = false>
void launch(const PlbGemmNT* p, const PlbGemmNTPlan& pl, int a_bf8, hipStream_t stream) {
  const dim3 grid(pl.grid), block(pl.block);
  if (a_bf8) hipLaunchKernelGGL((gemm_nt_big_kernel<V, ACT, false, true, true, true, NOCS>), grid, block, 0, stream, *p);
  else hipLaunchKernelGGL((gemm_nt_big_kernel<V, ACT, false, true, true, false, NOCS>), grid, block, 0, stream, *p);
}
int operands(int a_bf8) { return a_bf8 ? PLB_NT_FP8_E5M2 : PLB_NT_FP8_E4M3; }
}  // namespace

extern "C" int plb_launch_gemm_nt_fp8_ln(const PlbGemmNT* p_in, int mode, int a_bf8, hipStream_t stream) {
  PlbGemmNT q_ = *p_in;
  q_.ln_fault = plb_ln_fault_take();   // (consumed by a launch that is then refused, too)
  const PlbGemmNT* p = &q_;
  if (mode != PLB_NT_LNFWD && mode != PLB_NT_LNBWD) return 1;
  PlbGemmNTPlan pl;
  if (plb_gemm_nt_plan(p->M, p->N, p->K, mode, operands(a_bf8), (p->res ? PLB_NT_RES : 0) | (p->C8 ? PLB_NT_C8 : 0), 0, &pl))
    return pl.rc;
  if (nt_args_check(p, mode, true)) return 1;
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  if (pl.tile == 384) {
    if (mode == PLB_NT_LNFWD) launch<3, 5>(p, pl, a_bf8, stream); else launch<3, 6>(p, pl, a_bf8, stream);
  } else {
    if (mode == PLB_NT_LNFWD) launch<1, 5>(p, pl, a_bf8, stream); else launch<1, 6>(p, pl, a_bf8, stream);
  }
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// Forward: C = gelu_new'(u) (lane-layout stash, bf16), C2 = gelu_new(u) (bf16, optional), C8 = its e4m3 image. Backward:
// C = (A·B^T) * aux (bf16, optional), C8 = its e5m2 image, colpart = column-sum partials (2 rows per row tile).
// The 256x256 tile fits the register file since the fp8 units are compiled with MachineSink off (build.py). The stash is in
// the lane layout of the tile that wrote it: forward and backward of one call get the same tile from the same M.
extern "C" int plb_launch_gemm_nt_fp8_gelud(const PlbGemmNT* p, int backward, int a_bf8, hipStream_t stream) {
  const int form = backward ? PLB_NT_GELUDBWD : PLB_NT_GELUD;
  PlbGemmNTPlan pl;
  const int opts = (p->colpart ? PLB_NT_COLPART : 0) | (p->C8 ? PLB_NT_C8 : 0) | ((backward ? p->C : p->C2) ? PLB_NT_OUT16 : 0);
  if (plb_gemm_nt_plan(p->M, p->N, p->K, form, operands(a_bf8), opts, 0, &pl)) return pl.rc;
  if (nt_args_check(p, form, true)) return 1;
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  if (pl.tile == 256) {
    if (backward) launch<2, 8>(p, pl, a_bf8, stream);
    else if (p->colpart) launch<2, 7>(p, pl, a_bf8, stream);
    else launch<2, 7, true>(p, pl, a_bf8, stream);
  } else {
    if (backward) launch<1, 8>(p, pl, a_bf8, stream);
    else if (p->colpart) launch<1, 7>(p, pl, a_bf8, stream);
    else launch<1, 7, true>(p, pl, a_bf8, stream);
  }
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
