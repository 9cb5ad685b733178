// bf16 MFMA GEMMs of the ALBERT step, gfx950: the small NT kernel and the NT entry.
//
//  gemm_nt : C[M,N] = A[M,K] · B[N,K]^T (+bias) (+residual) with fused epilogues
//            forward projections (Y = X·W^T with W stored [out,in] as in the reference state-dict,
//            modeling_albert.py:166-170,196,228-230,272; model.py:28) and the dX products of the
//            backward pass (dX = dY·W computed as dY·(W^T)^T against the transposed weight copy).
// (The token-major weight-gradient GEMMs, dW = A^T · B, are gemm_tn.hip's.)
//
// Tile 128x128, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 tiles, fp32
// accumulate (also as 64x64, waves of 32x32, for launches too small to fill the chip). Operands
// are staged by LDS-DMA (global_load_lds); LDS images are XOR-swizzled so ds_read_b128 is bank-conflict free.
#include "common.h"
#include "plbert_kernels.h"
#include "gemm_epilogue.h"

namespace {

constexpr int BK = 64;

// LDS image of a [TILE rows][64 k] bf16 tile: 128-B rows, 16-B chunk index XORed with (row>>1)&7.
DEVI int nt_lds_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3); }

// TILE x TILE outputs per workgroup, 256 threads = 2x2 waves of (TILE/2) x (TILE/2) each.
//   128: the form every launch took before the 64 form existed (64 KiB of LDS, 4x4 MFMA tiles per wave)
//    64: for launches whose 128x128 grid leaves most of the chip idle: four times the workgroups, each staging half the
//        bytes and issuing a quarter of the MFMAs per K-tile (32 KiB of LDS, 2x2 MFMA tiles per wave, two workgroups per
//        CU and more)
// An output element sees the same K-chunks of 32 in the same order through the same fragment layout and the same
// epilogue in both forms: the tile only decides which wave computes which 16x16 patch, results are equal bit for bit
// (tests/test_gpu_gemm_small_tile.py).
template <int ACT, bool OUTF32, int TILE>
__global__ __launch_bounds__(256) void gemm_nt_kernel(PlbGemmNT p) {
  constexpr int WT = TILE / 2;    // rows and columns of a wave's patch
  constexpr int FR = WT / 16;     // MFMA tiles per wave and direction
  constexpr int SR = TILE / 4;    // rows of A and of B a wave stages per K-tile
  constexpr int ND = SR / 8;      // DMA instructions per operand for them (8 rows x 128 B each)
  __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][TILE * BK];  // [stage][A|B] 64 KiB (32 KiB at TILE 64)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int nbn = (p.N + TILE - 1) / TILE;
  const int nwg = gridDim.x;
  const int logical = xcd_remap(blockIdx.x, nwg);
  const int bm = logical / nbn, bn = logical % nbn;

  // Staging: LDS-DMA (global_load_lds, 16 B per lane). One wave-instruction fills 8 rows x 128 B of
  // the image; the destination is wave-uniform base + lane*16, so the XOR swizzle is applied to the
  // per-lane SOURCE chunk (row r, stored chunk c' <- global chunk c' ^ ((r>>1)&7)). Each wave stages
  // rows [SR w, SR w + SR) of A and of B: 2 ND DMA instructions per k-tile (8 / 4), no VGPR round trip.
  // (SR w is a multiple of 16, so (r>>1)&7 of row SR w + 8 i + (lane>>3) is (4 i + (lane>>4)) & 7 in both forms.)
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  const int drow = lane >> 3, dch = lane & 7;
  const bf16_t* gA = p.A + (size_t)(bm * TILE + uw * SR + drow) * p.lda;
  const bf16_t* gB = p.B + (size_t)(bn * TILE + uw * SR + drow) * p.ldb;
  const size_t sa = (size_t)8 * p.lda, sb = (size_t)8 * p.ldb;
  int sch[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) sch[i] = (dch ^ ((4 * i + (lane >> 4)) & 7)) * 8;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
#define NT_STAGE(st, kt)                                                                              \
  do {                                                                                                \
    _Pragma("unroll") for (int i = 0; i < ND; ++i) {                                                  \
      __builtin_amdgcn_global_load_lds((gptr_t)(gA + i * sa + (size_t)(kt) * BK + sch[i]),            \
                                       (lptr_t)&smem[st][0][(uw * SR + i * 8) * BK], 16, 0, 0);       \
      __builtin_amdgcn_global_load_lds((gptr_t)(gB + i * sb + (size_t)(kt) * BK + sch[i]),            \
                                       (lptr_t)&smem[st][1][(uw * SR + i * 8) * BK], 16, 0, 0);       \
    }                                                                                                 \
  } while (0)
#define NT_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

  f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  // (row>>1)&7 of a fragment row depends on the lane only: rows are wr*WT + i*16 + frow, WT a multiple of 16
  const int fsw = (frow >> 1) & 7;
  const int offA = (wr * WT + frow) * BK, offB = (wc * WT + frow) * BK;
#define NT_COMPUTE(st)                                                                                   \
  do {                                                                                                   \
    const bf16_t* sA = smem[st][0];                                                                      \
    const bf16_t* sB = smem[st][1];                                                                      \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                                   \
      const int ch = ((kk * 4 + fq) ^ fsw) << 3;                                                         \
      bf16x8 af[FR], bfr[FR];                                                                            \
      _Pragma("unroll") for (int i = 0; i < FR; ++i) {                                                   \
        af[i] = *(const bf16x8*)&sA[offA + i * 16 * BK + ch];                                            \
        bfr[i] = *(const bf16x8*)&sB[offB + i * 16 * BK + ch];                                           \
      }                                                                                                  \
      _Pragma("unroll") for (int mi = 0; mi < FR; ++mi)                                                  \
        _Pragma("unroll") for (int ni = 0; ni < FR; ++ni)                                                \
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);  \
    }                                                                                                    \
  } while (0)

  // swapped MFMA operands: D[row = n][col = m], so each lane owns 4 consecutive n of one row m
  const int nk = p.K / BK;
  NT_STAGE(0, 0);
  NT_LANDED();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) NT_STAGE(cur ^ 1, kt + 1);  // buffer cur^1 was last read before the previous barrier
    NT_COMPUTE(cur);  // one copy of the MFMA body: a peeled last iteration made the allocator shuffle AGPRs
    NT_LANDED();
    __syncthreads();
  }
#undef NT_STAGE
#undef NT_LANDED
#undef NT_COMPUTE

  // epilogue: lane holds C[m][n0..n0+3]
#pragma unroll
  for (int mi = 0; mi < FR; ++mi) {
    const int m = bm * TILE + wr * WT + mi * 16 + frow;
#pragma unroll
    for (int ni = 0; ni < FR; ++ni)
      nt_epilogue<ACT, OUTF32>(p, acc[mi][ni], m, bn * TILE + wc * WT + ni * 16 + fq * 4);
  }
}

}  // namespace

int gemm_nt_big_run(const PlbGemmNT* p, const PlbGemmNTPlan& pl, int form, hipStream_t stream);   // gemm_big.hip

// Which kernel, tile and grid a shape gets is the plan's (gemm_nt_plan.h); here: the small kernel's instantiations, and the
// hand-over of the plan to the pipeline kernel's (gemm_big.hip). act 3 / 4 (the cross-entropy passes, which the token head
// sends to plb_launch_gemm_nt_big itself) take the tile of the per-shape policy, as a plain launch of the shape would, and
// exist on the pipeline kernel only.
extern "C" int plb_launch_gemm_nt(const PlbGemmNT* p, int act, int out_f32, hipStream_t stream) {
  if ((out_f32 && act != 0) || act < 0 || act > 4) return 1;
  const bool ce = act > 2;
  const int form = out_f32 ? PLB_NT_F32 : ce ? PLB_NT_PLAIN : act;
  PlbGemmNTPlan pl;
  const int opts = (p->colpart ? PLB_NT_COLPART : 0) | (p->res ? PLB_NT_RES : 0);
  if (plb_gemm_nt_plan(p->M, p->N, p->K, form, PLB_NT_BF16, opts, 0, &pl)) return pl.rc;
  if (ce && pl.family == 0) return 1;
  const int tok = plb_prof_begin(pl.cls, stream, pl.flops, pl.bytes);
  int rc = 0;
  if (pl.family == 1) {
    rc = ce ? plb_launch_gemm_nt_big(p, pl.tile, act, 0, stream) : gemm_nt_big_run(p, pl, form, stream);
  } else {
    const dim3 grid(pl.grid), block(pl.block);
    if (pl.tile == 64) {
      if (out_f32) hipLaunchKernelGGL((gemm_nt_kernel<0, true, 64>), grid, block, 0, stream, *p);
      else if (act == 0) hipLaunchKernelGGL((gemm_nt_kernel<0, false, 64>), grid, block, 0, stream, *p);
      else if (act == 1) hipLaunchKernelGGL((gemm_nt_kernel<1, false, 64>), grid, block, 0, stream, *p);
      else hipLaunchKernelGGL((gemm_nt_kernel<2, false, 64>), grid, block, 0, stream, *p);
    } else {
      if (out_f32) hipLaunchKernelGGL((gemm_nt_kernel<0, true, 128>), grid, block, 0, stream, *p);
      else if (act == 0) hipLaunchKernelGGL((gemm_nt_kernel<0, false, 128>), grid, block, 0, stream, *p);
      else if (act == 1) hipLaunchKernelGGL((gemm_nt_kernel<1, false, 128>), grid, block, 0, stream, *p);
      else hipLaunchKernelGGL((gemm_nt_kernel<2, false, 128>), grid, block, 0, stream, *p);
    }
    rc = hipGetLastError() == hipSuccess ? 0 : 2;
  }
  plb_prof_end(tok, stream);
  return rc;
}
