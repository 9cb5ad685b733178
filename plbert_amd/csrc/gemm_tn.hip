// Token-major ("TN") weight-gradient GEMMs on bf16 operands (gfx950): dW[N,K] = A[Mtot,N]^T · B[Mtot,K], the reference's
// dW = dY^T·X of autograd. The reduction runs over token rows and is split over the grid into fp32 slabs that
// plb_launch_reduce_slabs sums; both operands are token-major, so MFMA fragments (reduction index on the k axis) are
// COLUMNS of the staged images and come from transposed LDS reads (ds_read_b64_tr_b16).
//   gemm_tn_kernel      128x128 tile, 4 waves, operands staged through registers: head and map-in gradients, small calls
//   gemm_tn_big_kernel  256x256 tile on the LDS-DMA pipeline (gemm_tn_pipeline.h): the four layer weights, the token head
// Which of them a shape gets, and its row splits, is the plan's (gemm_tn_plan.h). The fp8 form of the pipeline kernel is a
// unit of its own (gemm_tn_fp8.hip: it is built with other flags).
#include "gemm_tn_pipeline.h"

namespace {

// ---- 128x128 -------------------------------------------------------------------------------------------------------
// Tile 128x128, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 tiles, fp32 accumulate; double buffered,
// one barrier per k-tile.
// LDS image of a [64 t][128 cols] bf16 tile for transposed reads: 16-column strips, each strip a
// run of 64 32-byte units (one per t) ordered so that t and t+8 are 4 units apart (bits 2,3 of t
// swapped) and rotated by the strip index: a half-wave's ds_read_b64_tr_b16 (8 rows x 32 B) then
// covers one contiguous 256-B window, and an 8-lane ds_write_b128 group covers 128 B.
DEVI int tn_unit(int t) { return (t & 3) | (((t >> 3) & 1) << 2) | (((t >> 2) & 1) << 3) | (t & 48); }
DEVI int tn_lds_off(int t, int col) {
  int s = col >> 4;
  return s * 1024 + (((tn_unit(t) + s) & 63) << 4) + (col & 15);
}

__global__ __launch_bounds__(256) void gemm_tn_kernel(PlbGemmTN p) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][64 * 128];  // [stage][A|B] 64 KiB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int nbk = (p.K + 127) / 128;
  const int bn = blockIdx.x / nbk, bk = blockIdx.x % nbk;
  const int split = blockIdx.y;
  const int t_begin = split * p.rows_per_split;
  int t_end = t_begin + p.rows_per_split;
  if (t_end > p.Mtot) t_end = p.Mtot;
  const int nt = (t_end - t_begin) / 64;

  const int lc = tid & 15, lr = tid >> 4;  // staging: 16 rows x 16 chunks per pass, 4 passes
  const int colA = bn * 128 + lc * 8, colB = bk * 128 + lc * 8;
  const bool okA = colA < p.Ncols, okB = colB < p.K;
  uint4 ra[4], rb[4];
  auto load_tile = [&](int it) {
    const size_t t0 = (size_t)t_begin + (size_t)it * 64 + lr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = okA ? *(const uint4*)(p.A + (t0 + 16 * i) * p.lda + colA) : make_uint4(0, 0, 0, 0);
      rb[i] = okB ? *(const uint4*)(p.B + (t0 + 16 * i) * p.ldb + colB) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](int st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int off = tn_lds_off(lr + 16 * i, lc * 8);
      *(uint4*)&smem[st][0][off] = ra[i];
      *(uint4*)&smem[st][1][off] = rb[i];
    }
  };

  f32x4 acc[4][4];  // [n tile][k tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  if (nt > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  for (int it = 0; it < nt; ++it) {
    const int cur = it & 1;
    if (it + 1 < nt) load_tile(it + 1);
    const bf16_t* sA = smem[cur][0];
    const bf16_t* sB = smem[cur][1];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int t0 = ks * 32 + 8 * g + q;
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ca = wn * 64 + i * 16 + 4 * pp, cb = wk * 64 + i * 16 + 4 * pp;
        s16x4 a0 = lds_read_tr16(&sA[tn_lds_off(t0, ca)]);
        s16x4 a1 = lds_read_tr16(&sA[tn_lds_off(t0 + 4, ca)]);
        s16x4 b0 = lds_read_tr16(&sB[tn_lds_off(t0, cb)]);
        s16x4 b1 = lds_read_tr16(&sB[tn_lds_off(t0 + 4, cb)]);
        af[i] = bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        bfr[i] = bf16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int ki = 0; ki < 4; ++ki)
          // D[row = k col][col = n]: lane owns 4 consecutive k of one output row n
          acc[ni][ki] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ki], af[ni], acc[ni][ki], 0, 0, 0);
    }
    if (it + 1 < nt) store_tile(cur ^ 1);
    __syncthreads();
  }

  float* out = p.slab + (size_t)split * p.N * p.K;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = bn * 128 + wn * 64 + ni * 16 + li;
    if (n >= p.N) continue;
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const int k0 = bk * 128 + wk * 64 + ki * 16 + 4 * g;
      if (k0 >= p.K) continue;
      f32x4 v = acc[ni][ki];
      *(float4*)(out + (size_t)n * p.K + k0) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ---- 256x256 on the pipeline, bf16 operands --------------------------------------------------------------------------
// The reduction runs over token rows t in steps of 64. A half-tile is [64 t][128 cols] = two [64][64] LDS images with
// 128-B rows filled by LDS-DMA in full 128-B lines. A half-wave's transposed read touches rows
// {r..r+3, r+8..r+11} x 32 B; XOR-ing the 32-B pair index with ((row>>1)&1) | ((row>>3)&1)<<1 spreads
// those eight segments over all 64 banks (the swizzle is applied to the DMA's per-lane source chunk).
DEVI int tn_g(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1); }

__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(224))) void gemm_tn_big_kernel(PlbGemmTN p) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 4 * HT];  // [buf][A0,A1,B0,B1][2 images][64][64]
  TN_PLACE(6);

  // ---- staging: instruction i = 2w + j of a half-tile covers image i>>3, rows (i&7)*8 + (lane>>3)
  const int i0 = 2 * uw, i1 = 2 * uw + 1;
  const int r0 = (i0 & 7) * 8 + (lane >> 3), r1 = (i1 & 7) * 8 + (lane >> 3);
  const int sc0 = (((lane & 7) ^ (2 * tn_g(r0))) * 8) + (i0 >> 3) * 64;  // source column within the half
  const int sc1 = (((lane & 7) ^ (2 * tn_g(r1))) * 8) + (i1 >> 3) * 64;
  const int dst0 = (i0 >> 3) * 4096 + (i0 & 7) * 8 * 64, dst1 = (i1 >> 3) * 4096 + (i1 & 7) * 8 * 64;
  // ---- fragment reads (transposed): lane 4q+p of a 16-lane group supplies row q, columns 4p..4p+3;
  // k-step kk covers t rows kk*32 + 8*(lane>>4) + {0..3} (first read) and +4 (second read)
  const int fg = lane >> 4, li = lane & 15, q4 = li >> 2, p4 = li & 3;
  // A fragment (mi): image wm of the half, columns mi*16 + 4p ; B fragment (ni): image wn>>1, columns
  // (wn&1)*32 + ni*16 + 4p. The swizzle term of row kk*32 + 8*fg + 4*s2 + q depends on the lane only
  // (((row>>1)&1) = (q>>1)&1, ((row>>3)&1) = fg&1), so every read is lane base + compile-time offset.
  const int gsw = 2 * (((q4 >> 1) & 1) | ((fg & 1) << 1));
  const int rowbase = (8 * fg + q4) * 64 + (p4 & 1) * 4;
  int aoff[4], boff[2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) aoff[mi] = wm * 4096 + rowbase + (((2 * mi + (p4 >> 1)) ^ gsw) << 3);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    boff[ni] = (wn >> 1) * 4096 + rowbase + (((4 * (wn & 1) + 2 * ni + (p4 >> 1)) ^ gsw) << 3);
  const unsigned lds0 = (unsigned)(size_t)&smem[0];
#define FRAG(r, kk) (bf16x8{r[2 * (kk)][0], r[2 * (kk)][1], r[2 * (kk)][2], r[2 * (kk)][3],              \
                            r[2 * (kk) + 1][0], r[2 * (kk) + 1][1], r[2 * (kk) + 1][2], r[2 * (kk) + 1][3]})

  TN_ZERO_ACC();
// TN_DBG (timing builds only, tools/tn_wait.py): 1 = print, from one workgroup, the share of the K loop a wave spends in the
// vmcnt wait that precedes phase 4 (is the loop waiting for memory?) and the loop's time per K-tile
#ifndef TN_DBG
#define TN_DBG 0
#endif
#if TN_DBG
  unsigned long long tnw_ = 0, tnq_ = 0;
#define TN_W0() tnq_ = __builtin_readcyclecounter()
#define TN_W1() tnw_ += __builtin_readcyclecounter() - tnq_
#else
#define TN_W0()
#define TN_W1()
#endif
#define LANDED(more)                                                      \
  do {                                                                    \
    TN_W0();                                                              \
    if (more) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");            \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 \
    TN_W1();                                                              \
  } while (0)

  s16x4 ra1[4][4], rb2[2][2][4];  // [A fragment][kk*2 + second], [B buffer][fragment][kk*2 + second]
// LDS addresses: one lane-constant base per (buffer, fragment) — the swizzle makes a fragment's offset non-linear in its
// index — and everything else (half-tile, image piece) in the instruction's 16-bit offset field: a buffer spans 64 KiB.
// The reads are the BUILTIN (beside builtin DMAs hipcc drains vmcnt before every LDS read that might alias one; with the
// DMAs written as asm nothing makes it do that, and
// it tracks lgkmcnt for the reads itself — as asm, their outputs looked ready at once, and the 16-bit shuffles that
// assemble a fragment from its two halves were hoisted above the arrival of the data (wrong results, not a crash).
#define TR1(dst, addr, OFF) dst = lds_read_tr16_addr((addr) + (OFF))
#define RD4(dst, ad_, o_)  /* the four pieces of one fragment */ \
  do { TR1(dst[0], ad_, (o_)); TR1(dst[1], ad_, (o_) + 512); TR1(dst[2], ad_, (o_) + 4096); TR1(dst[3], ad_, (o_) + 4608); PIN(); } while (0)
#define RA4(buf, h, mi) RD4(ra1[mi], abase[buf][mi], (h) * 16384)
#define RB4(bb, buf, h, ni) RD4(rb2[bb][ni], bbase[buf][ni], (2 + (h)) * 16384)
// DMA in the scalar-base form (common.h): lane-constant 32-bit offsets, the K-tile's base address on the scalar unit
#define SA_(h, kt) ((const char*)p.A + ((size_t)(t_begin + (kt) * 64) * p.lda + bn * 256 + (h) * 128) * 2)
#define SB_(h, kt) ((const char*)p.B + ((size_t)(t_begin + (kt) * 64) * p.ldb + bk * 256 + (h) * 128) * 2)
#define STG_A(buf, h, kt)                                                                     \
  do {                                                                                        \
    const char* sb_ = SA_(h, kt);                                                             \
    DMA16(sb_, vA0, ldsb + (((buf) * 4 + (h)) * HT + dst0) * 2);                              \
    DMA16(sb_, vA1, ldsb + (((buf) * 4 + (h)) * HT + dst1) * 2);                              \
    PIN();                                                                                    \
  } while (0)
#define STG_B(buf, h, kt)                                                                     \
  do {                                                                                        \
    const char* sb_ = SB_(h, kt);                                                             \
    DMA16(sb_, vB0, ldsb + (((buf) * 4 + 2 + (h)) * HT + dst0) * 2);                          \
    DMA16(sb_, vB1, ldsb + (((buf) * 4 + 2 + (h)) * HT + dst1) * 2);                          \
    PIN();                                                                                    \
  } while (0)
  const uint32_t vA0 = (uint32_t)(r0 * p.lda + sc0) * 2, vA1 = (uint32_t)(r1 * p.lda + sc1) * 2;
  const uint32_t vB0 = (uint32_t)(r0 * p.ldb + sc0) * 2, vB1 = (uint32_t)(r1 * p.ldb + sc1) * 2;
  const uint32_t ldsb = LDS_ADDR(&smem[0]);
  unsigned abase[2][4], bbase[2][2];
#pragma unroll
  for (int bf = 0; bf < 2; ++bf) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) abase[bf][mi] = lds0 + 65536u * bf + 2u * aoff[mi];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bbase[bf][ni] = lds0 + 65536u * bf + 2u * boff[ni];
  }
// one piece (0..3 -> byte offsets 0, 512, 4096, 4608) of an A / B fragment
#define PO_(pc) ((pc) == 0 ? 0 : (pc) == 1 ? 512 : (pc) == 2 ? 4096 : 4608)
#define RA1(buf, h, mi, pc) do { TR1(ra1[mi][pc], abase[buf][mi], (h) * 16384 + PO_(pc)); PIN(); } while (0)
#define RB1(bb, buf, h, ni, pc) do { TR1(rb2[bb][ni][pc], bbase[buf][ni], (2 + (h)) * 16384 + PO_(pc)); PIN(); } while (0)
// MFMA j of a phase, fragment-major: mi = j >> 2, kk = (j >> 1) & 1, ni = j & 1 (each accumulator still sees kk = 0 first)
#define MF1(mh, nh, bb, j)                                                                                      \
  do {                                                                                                          \
    acc[mh][(j) >> 2][nh][(j) & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                                   \
        FRAG(rb2[bb][(j) & 1], ((j) >> 1) & 1), FRAG(ra1[(j) >> 2], ((j) >> 1) & 1), acc[mh][(j) >> 2][nh][(j) & 1], 0, 0, 0); \
    PIN();                                                                                                      \
  } while (0)
  TN_PROLOGUE();
#if TN_DBG
  tnw_ = 0;
  const unsigned long long tn_c0 = __builtin_readcyclecounter(), tn_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  TN_KLOOP()
#if TN_DBG
  if ((blockIdx.x == 17 || blockIdx.x == 130) && lane == 0 && (uw == 0 || uw == 5)) {
    const unsigned long long dc = __builtin_readcyclecounter() - tn_c0, dr = __builtin_amdgcn_s_memrealtime() - tn_r0;
    printf("TN blk %d wave %d: %d K-tiles, %.3f us per K-tile, %.0f MHz, vmcnt wait %.1f %% of the loop\n", (int)blockIdx.x, uw, nk,
           (double)dr / 100.0 / nk, (double)dc / ((double)dr / 100.0), 100.0 * (double)tnw_ / (double)dc);
  }
#endif
  TN_STORE(TN_PLAIN4)
}

}  // namespace

extern "C" int plb_launch_gemm_tn(const PlbGemmTN* p, hipStream_t stream) {
  if (p->Mtot % 64 || p->rows_per_split % 64 || p->K % 4 || p->N <= 0 || p->splits <= 0) return 1;
  if ((long)p->splits * p->rows_per_split < p->Mtot) return 1;
  dim3 grid(((p->N + 127) / 128) * ((p->K + 127) / 128), p->splits), block(256);
  const int tok = plb_prof_begin(PLB_K_GEMM_TN, stream, 2.0 * p->Mtot * (double)p->N * p->K,
                                 2.0 * p->Mtot * ((double)p->N + p->K) + 4.0 * p->splits * (double)p->N * p->K);
  hipLaunchKernelGGL(gemm_tn_kernel, grid, block, 0, stream, *p);
  plb_prof_end(tok, stream);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The pipeline kernel: Ncols % 256 == 0 (readable columns of A), K % 256 == 0, rows_per_split % 64 == 0. N (rows stored)
// may be smaller than Ncols. No profiler scope of its own: the engine's weight_grad opens one.
extern "C" int plb_launch_gemm_tn_big(const PlbGemmTN* p, hipStream_t stream) {
  if (p->Ncols % 256 || p->K % 256 || p->rows_per_split % 64 || p->Mtot % 64 || p->splits <= 0) return 1;
  if ((long)p->splits * p->rows_per_split < p->Mtot) return 1;
  dim3 grid((p->Ncols / 256) * (p->K / 256) * p->splits), block(512);
  hipLaunchKernelGGL(gemm_tn_big_kernel, grid, block, 0, stream, *p);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
