// Large-tile NT GEMMs with a multi-phase, counted-vmcnt LDS-DMA pipeline (gfx950).
//
// Why: at a 128x128 tile the operand stream into LDS is 64 FLOP/B, and a CU's LDS-DMA path (one 1 KiB
// global_load_lds per 16 clocks through the texture addresser: ~94 GB/s per CU measured) bounds the kernel
// long before the MFMA pipe. Here one workgroup of 8 waves (2 per SIMD) owns a CU, the tile is 256x256
// (128 FLOP/B), 128x384 (96 FLOP/B) or 128x256 (85 FLOP/B), and 4-6 16-KiB half-tiles of LDS-DMA stay in
// flight across barriers (counted s_waitcnt vmcnt(N), never 0 in steady state). Tile choice is by wave
// quantisation on 256 CUs: N = 768 -> 128x384 gives exactly 256 tiles at M = 16384 (256x256 would give 192:
// a quarter of the chip idle), N = 2304 -> 768 tiles = 3 per CU, N = 2048 -> 512 tiles of 256x256.
//
// A K-tile (64 deep) is 3-4 128-row half-tiles, streamed through a 10-slot ring (the whole 160 KiB LDS) in
// consumption order:   256x256: A0 B0 B1 A1      128x384: A B0 B1 B2      128x256: A B0 B1
// 8 waves = 2 (M) x 4 (N). Wave (wm, wn) owns rows {mh*128 + wm*64 + 0..63} and columns
// {nh*128 + wn*32 + 0..31} of every (mh, nh): its output is interleaved over the half-tiles, so one
// phase (16 MFMAs 16x16x32 = a 64x32 patch) reads fragments of ONE A half and ONE B half:
//   256x256:  ph1 A0,B0 -> (0,0) | ph2 B1 -> (0,1) | ph3 A1 -> (1,1) | ph4 (1,0)
//   128x384:  ph1 A,B0 -> nh 0   | ph2 B1 -> nh 1  | ph3 B2 -> nh 2
// A slot is re-filled once the phase that read its previous occupant is behind a barrier. Barriers are raw
// s_barrier (asm: __syncthreads() would drain vmcnt to 0). Two forms of the K loop exist, chosen per launch
// by measurement (the plan: gemm_nt_plan.cpp): "interleaved" (fragment reads of the next phase and the DMA
// issues dealt into the MFMA shadows, one barrier per phase) and "staggered" (two barriers per phase, the
// two waves of a SIMD half a phase apart) — see the comments at the loops.
#include "gemm_nt_pipeline.h"

// Timing builds (tools/build_variant.py <name> --only <the pipeline units> -DNT_DBG=<bit mask>): 16 prints the shader
// clock over the K loop, 32 the phase stamps of one workgroup (tools/nt_stamps.py, tools/nt_stamps_fp8.py). Results stay
// valid. The shipped library has 0.
namespace {

// the instantiations of this unit: tile V (1 128x256, 2 256x256, 3 128x384) x K-loop form PF x the forms 0 - 4 and 9
template <int V, bool PF>
void launch_big(const PlbGemmNT* p, int form, dim3 grid, dim3 block, hipStream_t stream) {
  switch (form) {
    case PLB_NT_F32: hipLaunchKernelGGL((gemm_nt_big_kernel<V, 0, true, PF>), grid, block, 0, stream, *p); break;
    case PLB_NT_PLAIN:   // (the column sums are compiled out where nobody wants them)
      if (p->colpart) hipLaunchKernelGGL((gemm_nt_big_kernel<V, 0, false, PF>), grid, block, 0, stream, *p);
      else hipLaunchKernelGGL((gemm_nt_big_kernel<V, 0, false, PF, false, false, true>), grid, block, 0, stream, *p);
      break;
    case PLB_NT_GELU: hipLaunchKernelGGL((gemm_nt_big_kernel<V, 1, false, PF>), grid, block, 0, stream, *p); break;
    case PLB_NT_GELUBWD: hipLaunchKernelGGL((gemm_nt_big_kernel<V, 2, false, PF>), grid, block, 0, stream, *p); break;
    case PLB_NT_CE1: case PLB_NT_CE2:   // fused GEMM + cross-entropy passes: 256-column tiles only (the plan refuses 128x384)
      if constexpr (V != 3) {
        if (form == PLB_NT_CE1) hipLaunchKernelGGL((gemm_nt_big_kernel<V, 3, false, PF>), grid, block, 0, stream, *p);
        else hipLaunchKernelGGL((gemm_nt_big_kernel<V, 4, false, PF>), grid, block, 0, stream, *p);
      }
      break;
  }
}

}  // namespace

// The pipeline launch of a plan of this unit's forms (bf16 operands, forms 0 - 4 and 9). Not exported: plb_launch_gemm_nt
// (gemm.hip), which has planned already, calls it too.
int gemm_nt_big_run(const PlbGemmNT* p, const PlbGemmNTPlan& pl, int form, hipStream_t stream) {
  if (nt_args_check(p, form, false)) return 1;
  const dim3 grid(pl.grid), block(pl.block);
  if (pl.kloop) {
    if (pl.tile == 384) launch_big<3, true>(p, form, grid, block, stream);
    else if (pl.tile == 1256) launch_big<1, true>(p, form, grid, block, stream);
    else launch_big<2, true>(p, form, grid, block, stream);
  } else {
    if (pl.tile == 384) launch_big<3, false>(p, form, grid, block, stream);
    else if (pl.tile == 1256) launch_big<1, false>(p, form, grid, block, stream);
    else launch_big<2, false>(p, form, grid, block, stream);
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// tile = 256: 256x256 (M % 256, N % 256); 384: 128x384 (M % 128, N % 384); 1256: 128x256 (M % 128, N % 256); any other
// value: 256. The K-loop form is the plan's (gemm_nt_plan.h: plb_set_gemm_nt_prefetch). No profiler scope of its own: its
// callers (plb_launch_gemm_nt, the token head) open one.
extern "C" int plb_launch_gemm_nt_big(const PlbGemmNT* p, int tile, int act, int out_f32, hipStream_t stream) {
  if ((out_f32 && act != 0) || act < 0 || act > 4) return 1;
  const int form = out_f32 ? PLB_NT_F32 : act;
  PlbGemmNTPlan pl;
  if (plb_gemm_nt_plan(p->M, p->N, p->K, form, PLB_NT_BF16, p->colpart ? PLB_NT_COLPART : 0,
                       tile == 384 || tile == 1256 ? tile : 256, &pl))
    return pl.rc;
  return gemm_nt_big_run(p, pl, form, stream);
}
