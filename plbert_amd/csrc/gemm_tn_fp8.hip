// dW[N,K] = A[rows,N]^T · B[rows,K] on 1-byte operand images (gfx950): the token-major ("TN") weight-gradient GEMM of
// gemm_tn.hip in fp8 mode (BASELINE.json configs[4]). A = the e5m2 image of a gradient (dQKV, dpre1, dU, dpre2), B = the
// e4m3 image of the activation it multiplies (x, context, a, gelu(u)), both written by the launches that produced the
// tensors (engine.cpp), fp32 accumulation, fp32 slabs: the reference's dW = dY^T·X of autograd (train.py:356), summed over
// the 12 applications of the shared layer in ONE launch per weight.
//
// Same pipeline as gemm_tn_big_kernel (gemm_tn_pipeline.h: placement, schedule and store are that header's; this unit
// supplies the operand hooks) — 256 (n) x 256 (k) output tile, one 8-wave workgroup per CU, LDS-DMA in full
// 128-byte lines into a double-buffered 128 KiB stage, interleaved K loop with one barrier per phase — on twice the tokens
// per byte: a half-tile is [128 t][128 columns] bytes (16 KiB), a K-tile 128 tokens, and ONE block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales (plain fp8 arithmetic at twice the bf16 MFMA rate) replaces four
// bf16 MFMAs. MFMA fragments need the reduction index (the token) on the k axis, i.e. COLUMNS of the token-major images:
// ds_read_b64_tr_b8. Measured semantics (tools/probe_tr8.hip, profiles/r04_probe_tr8_hw.txt): within a 16-lane group,
// lane 2q + p supplies the address of row q (0..7), 8-byte column piece p (0..1); lane i receives column i's 8 rows.
// A fragment = 32 tokens per lane = 4 such reads; lane group g = lane >> 4 takes tokens [32 g, 32 g + 32) of the K-tile,
// read r the rows 32 g + 8 r + {0..7}. A and B use the same assignment, so the k order inside the MFMA does not matter.
// Banks: a half-wave's read touches 2 groups x 8 rows x 16 B; a 128-byte row is 32 banks, so the 8 rows of one parity
// must fall into 8 different 16-byte units: unit' = unit ^ f(row), f(row) = ((row >> 1) & 3) | (((row >> 5) & 1) << 2)
// (rows of one group differ in bits 1-2, the two groups of a half-wave in bit 5), applied to the DMA's per-lane SOURCE unit.
#include "gemm_tn_pipeline.h"

namespace {

typedef int i32x2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2v lds_i32x2v;
DEVI i32x2v lds_read_tr8_addr(uint32_t lds_byte_addr) {
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2v*)(uintptr_t)lds_byte_addr);
}
DEVI int tn8_f(int row) { return ((row >> 1) & 3) | (((row >> 5) & 1) << 2); }

__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(224))) void gemm_tn_fp8_kernel(PlbGemmTN p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 4 * 16384];  // [buf][A0,A1,B0,B1][128 t][128 B]
  TN_PLACE(7);

  // ---- staging: instruction i = 2w + j of a half-tile covers rows 8 i + (lane >> 3); lane writes physical unit lane & 7
  const int r0 = (2 * uw) * 8 + (lane >> 3), r1 = (2 * uw + 1) * 8 + (lane >> 3);
  const int sc0 = ((lane & 7) ^ tn8_f(r0)) * 16, sc1 = ((lane & 7) ^ tn8_f(r1)) * 16;   // source column (bytes) within the half
  const int dst0 = (2 * uw) * 1024, dst1 = (2 * uw + 1) * 1024;
  // ---- fragment reads: lane (g, q, pp) of read r supplies row 32 g + 8 r + q, unit (logical ^ f(row)), piece pp
  const int fg = lane >> 4, li = lane & 15, q8 = li >> 1, pp = li & 1;
  const int fx = tn8_f(32 * fg + q8);                  // (8 r never touches bits 1, 2, 5)
  const int rowbase = (32 * fg + q8) * 128 + pp * 8;
  const unsigned lds0 = (unsigned)(size_t)&smem[0];

  TN_ZERO_ACC();
#define LANDED(more)                                                      \
  do {                                                                    \
    if (more) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");            \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 \
  } while (0)

  // Fragments as 8-register tuples written piece by piece (sub-registers: no copy to form the MFMA operand). One rolling
  // A buffer, two B buffers; the fp8 MFMA of (mi, ni) sits in slot 4 mi + 2 ni of its phase (8 MFMAs of twice the length),
  // and a fragment is 4 pieces here as in the bf16 kernel, so reads and DMA issues take the slots the shared table names.
  i32x8v ra[4], rb[2][2];
#define TR1(dst, pc, addr, OFF)                                         \
  do {                                                                  \
    const i32x2v t_ = lds_read_tr8_addr((addr) + (OFF));                \
    dst[2 * (pc)] = t_[0]; dst[2 * (pc) + 1] = t_[1];                   \
  } while (0)
#define SA_(h, kt) ((const char*)p.A + ((size_t)(t_begin + (kt) * 128) * p.lda + bn * 256 + (h) * 128))
#define SB_(h, kt) ((const char*)p.B + ((size_t)(t_begin + (kt) * 128) * p.ldb + bk * 256 + (h) * 128))
#define STG_A(buf, h, kt)                                                                     \
  do {                                                                                        \
    const char* sb_ = SA_(h, kt);                                                             \
    DMA16(sb_, vA0, ldsb + ((buf) * 4 + (h)) * 16384 + dst0);                                 \
    DMA16(sb_, vA1, ldsb + ((buf) * 4 + (h)) * 16384 + dst1);                                 \
    PIN();                                                                                    \
  } while (0)
#define STG_B(buf, h, kt)                                                                     \
  do {                                                                                        \
    const char* sb_ = SB_(h, kt);                                                             \
    DMA16(sb_, vB0, ldsb + ((buf) * 4 + 2 + (h)) * 16384 + dst0);                             \
    DMA16(sb_, vB1, ldsb + ((buf) * 4 + 2 + (h)) * 16384 + dst1);                             \
    PIN();                                                                                    \
  } while (0)
  const uint32_t vA0 = (uint32_t)(r0 * p.lda + sc0), vA1 = (uint32_t)(r1 * p.lda + sc1);
  const uint32_t vB0 = (uint32_t)(r0 * p.ldb + sc0), vB1 = (uint32_t)(r1 * p.ldb + sc1);
  const uint32_t ldsb = LDS_ADDR(&smem[0]);
  // one lane-constant base per (buffer, fragment): the swizzle makes a fragment's offset non-linear in its index;
  // half-tile and piece go into the instruction's 16-bit offset field (a buffer spans 64 KiB)
  unsigned abase[2][4], bbase[2][2];
#pragma unroll
  for (int bf = 0; bf < 2; ++bf) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) abase[bf][mi] = lds0 + 65536u * bf + rowbase + (((wm * 4 + mi) ^ fx) << 4);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bbase[bf][ni] = lds0 + 65536u * bf + rowbase + (((wn * 2 + ni) ^ fx) << 4);
  }
// piece pc (0..3) of a fragment = rows + 8 pc: byte offset 1024 pc
#define RA1(buf, h, mi, pc) do { TR1(ra[mi], pc, abase[buf][mi], (h) * 16384 + (pc) * 1024); PIN(); } while (0)
#define RB1(bb, buf, h, ni, pc) do { TR1(rb[bb][ni], pc, bbase[buf][ni], (2 + (h)) * 16384 + (pc) * 1024); PIN(); } while (0)
#define RA4(buf, h, mi) do { RA1(buf, h, mi, 0); RA1(buf, h, mi, 1); RA1(buf, h, mi, 2); RA1(buf, h, mi, 3); } while (0)
#define RB4(bb, buf, h, ni) do { RB1(bb, buf, h, ni, 0); RB1(bb, buf, h, ni, 1); RB1(bb, buf, h, ni, 2); RB1(bb, buf, h, ni, 3); } while (0)
// slot j of a phase: the MFMA of (mi = j >> 2, ni = (j >> 1) & 1) in the even slots. First operand (rows of D) = the
// activation fragment (e4m3), second = the gradient fragment (e5m2): D[row = k][col = n], as in the bf16 kernel.
#define MF1(mh, nh, bb, j)                                                                                      \
  do {                                                                                                          \
    if (((j) & 1) == 0)                                                                                         \
      acc[mh][(j) >> 2][nh][((j) >> 1) & 1] =                                                                   \
          mfma_fp8<true>(rb[bb][((j) >> 1) & 1], ra[(j) >> 2], acc[mh][(j) >> 2][nh][((j) >> 1) & 1]);          \
    PIN();                                                                                                      \
  } while (0)
  TN_PROLOGUE();
  TN_KLOOP()

  // both per-tensor dequantisation factors are applied in the store
  const float deq = p.deq_a[0] * p.deq_b[0];
#define TN_DEQ4(v) make_float4(v[0] * deq, v[1] * deq, v[2] * deq, v[3] * deq)
  TN_STORE(TN_DEQ4)
}

}  // namespace

// Ncols % 256 == 0 (readable byte columns of A), K % 256 == 0, rows_per_split % 128 == 0, Mtot % 128 == 0; lda / ldb in
// bytes, multiples of 16; deq_a / deq_b: device scalars (1 / scale of each image).
extern "C" int plb_launch_gemm_tn_fp8(const PlbGemmTN* p, hipStream_t stream) {
  if (p->Ncols % 256 || p->K % 256 || p->rows_per_split % 128 || p->Mtot % 128 || p->splits <= 0) return 1;
  if ((long)p->splits * p->rows_per_split < p->Mtot) return 1;
  if (p->lda % 16 || p->ldb % 16 || !p->deq_a || !p->deq_b) return 1;
  dim3 grid((p->Ncols / 256) * (p->K / 256) * p->splits), block(512);
  hipLaunchKernelGGL(gemm_tn_fp8_kernel, grid, block, 0, stream, *p);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
