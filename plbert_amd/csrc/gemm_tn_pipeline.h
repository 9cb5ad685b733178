// The 256x256 token-major ("TN") pipeline kernel, dW[N,K] = A[rows,N]^T · B[rows,K], as far as its two operand kinds share
// it: block placement, accumulators, the schedule of the K loop and the store. gemm_tn_big_kernel (gemm_tn.hip: bf16
// operands, ds_read_b64_tr_b16, K-tiles of 64 tokens) and gemm_tn_fp8_kernel (gemm_tn_fp8.hip: 1-byte images,
// ds_read_b64_tr_b8, K-tiles of 128 tokens) each define the hooks below and then expand these macros inside their body.
// The sharing is TEXTUAL on purpose: the compiler sees the token stream it saw when each kernel carried its own copy, so
// the instruction lists do not move (profiles/tn_pipeline_isa.txt); as inline functions the placement, zeroing and store
// changed the register allocation of both kernels.
//
// One 8-wave workgroup per CU = 2 (n) x 4 (k) waves; wave (wm, wn) owns rows {mh*128 + wm*64 + 0..63} (n) and columns
// {nh*128 + wn*32 + 0..31} (k) of every (mh, nh) quarter of the tile. A K-tile is four half-tiles [tokens][128 columns]
// (A0, A1, B0, B1; 16 KiB each) filled by LDS-DMA in full 128-byte lines into a double-buffered 128 KiB stage.
//
// Hooks (macros of the kernel, defined before the expansion; buf = stage buffer, h = half, mi / ni = fragment, pc = piece):
//   RA1(buf, h, mi, pc)       one of the four transposed piece reads of A fragment mi, into the rolling A registers
//   RB1(bb, buf, h, ni, pc)   the same for B fragment ni, into B register buffer bb
//   RA4(buf, h, mi), RB4(bb, buf, h, ni)   all four pieces (prologue)
//   STG_A(buf, h, kt), STG_B(buf, h, kt)   the two DMA issues of one half-tile of K-tile kt
//   MF1(mh, nh, bb, j)        slot j (0..15) of a phase: bf16 = one MFMA per slot, fragment-major (mi = j >> 2); fp8 = one
//                             block-scaled MFMA of twice the length in the even slots (mi = j >> 2, ni = (j >> 1) & 1)
//   LANDED(more)              the vmcnt wait: 6 (three half-tiles stay in flight) while K-tiles remain, else 0
//   tokens per K-tile         as the shift that TN_PLACE takes (6 / 7)
//
// ---- the schedule -------------------------------------------------------------------------------------------------------
// Interleaved K loop (the NT kernel's default form, see gemm_nt_pipeline.h): a phase is {BARRIER, 16 slots}; the transposed
// fragment reads for the NEXT phase and the DMA issues are dealt into the shadows of the MFMAs. One barrier per phase, no
// stagger. The register budget decides the details: with 128 accumulators, ping-pong A buffers put the bf16 kernel at 254
// VGPRs, i.e. two waves fill a SIMD's register file and the side stream's small kernels (16-64 VGPRs), which ran BESIDE the
// old 223-register kernel on the same CUs, were left with the 4-13 CUs it does not use: the whole step measured no faster
// although this kernel was 10 % faster alone. Hence amdgpu_num_vgpr(224) on both kernels (two waves then leave 64
// registers of every SIMD, and 32 KiB of LDS, to those kernels) and ONE A buffer that rolls: a phase issues its MFMAs
// fragment-major, and once the MFMAs of A fragment mi have issued (the last one sits in slot 4 mi + 3, in fp8 4 mi + 2),
// the reads of the NEXT A half's fragment mi go to the same registers, in slot 4 mi + 4 or later; only fragment 3 cannot
// roll inside its phase and is read at the start of the next one, under that phase's first 12 slots, with its own lgkmcnt
// wait. B keeps two buffers whose roles alternate from one K-tile to the next (loop written for two K-tiles).
//  ph1 (A0,B0): reads A0[3] (late), B1(t); issue A1(t+1)        ph2 (A0,B1): reads A1(t)[0..2]; issue A0(t+2)
//  ph3 (A1,B1): reads A1(t)[3] (late); issue B0(t+2), B1(t+2); then the vmcnt wait
//  ph4 (A1,B0): reads A0(t+1)[0..2], B0(t+1)
//  RAW: what ph4's shadows read (K-tile t+1's A0, B0) and what ph1 / ph2 of the next tile read (its B1, A1) was issued
//       before the three newest half-tiles that the wait leaves in flight; a BARRIER follows the wait.
//  WAR: a slot's previous occupant was read at the latest in the phase before the one whose shadows re-fill it, and
//       those reads retired at that phase's BARRIER or at the explicit wait of a late fragment.
// (The staggered two-barrier form of this loop, 6-9 % slower, was removed in round 3; it is in the history.)
#pragma once
#include "gemm_nt_pipeline.h"

// Work placement: every tile of one row split streams the same token rows, so the tiles of a split should share an L2.
// Blocks are dealt round-robin over the 8 XCDs (block id % 8 labels the XCD group — speed only, never correctness), and
// xcd_remap hands XCD x the x-th contiguous run of the logical order (split-major): whole splits when their count is a
// multiple of 8, otherwise a split may straddle two XCDs (its rows are then fetched by both L2s).
// Declares wm, wn, split, bn, bk, t_begin and nk = K-tiles (1 << KSHIFT tokens each) of this split.
#define TN_PLACE(KSHIFT)                                         \
  const int tid = threadIdx.x, lane = tid & 63;                  \
  const int uw = __builtin_amdgcn_readfirstlane(tid >> 6);       \
  const int wm = uw >> 2, wn = uw & 3;                           \
  const int nbk = p.K >> 8;                                      \
  const int tiles = (p.Ncols >> 8) * nbk;                        \
  const int logical = xcd_remap(blockIdx.x, gridDim.x);          \
  const int split = logical / tiles, tile = logical % tiles;     \
  const int bn = tile / nbk, bk = tile % nbk;                    \
  const int t_begin = split * p.rows_per_split;                  \
  int t_end = t_begin + p.rows_per_split;                        \
  if (t_end > p.Mtot) t_end = p.Mtot;                            \
  const int nk = (t_end - t_begin) >> (KSHIFT)

// acc[mh][mi][nh][ni]: n = mh*128 + wm*64 + mi*16 + .., k = nh*128 + wn*32 + ni*16 + ..
#define TN_ZERO_ACC()                                                                      \
  f32x4 acc[2][4][2][2];                                                                   \
  _Pragma("unroll") for (int a = 0; a < 2; ++a)                                            \
    _Pragma("unroll") for (int b = 0; b < 4; ++b)                                          \
      _Pragma("unroll") for (int c = 0; c < 2; ++c)                                        \
        _Pragma("unroll") for (int d = 0; d < 2; ++d) acc[a][b][c][d] = f32x4{0.f, 0.f, 0.f, 0.f}

#define PH1(mh, nh, bb, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                    \
  do {                                                                                                          \
    BARRIER(); PIN();                                                                                           \
    MF1(mh, nh, bb, 0); s0; MF1(mh, nh, bb, 1); s1; MF1(mh, nh, bb, 2); s2; MF1(mh, nh, bb, 3); s3;             \
    MF1(mh, nh, bb, 4); s4; MF1(mh, nh, bb, 5); s5; MF1(mh, nh, bb, 6); s6; MF1(mh, nh, bb, 7); s7;             \
    MF1(mh, nh, bb, 8); s8; MF1(mh, nh, bb, 9); s9; MF1(mh, nh, bb, 10); s10; MF1(mh, nh, bb, 11); s11;         \
    MF1(mh, nh, bb, 12); s12; MF1(mh, nh, bb, 13); s13; MF1(mh, nh, bb, 14); s14; MF1(mh, nh, bb, 15); s15;     \
  } while (0)
#define NOP_ (void)0
#define TWO(x, y) do { x; y; } while (0)
#define TN_STEP(bb)                                                                                             \
  do {                                                                                                          \
    constexpr int b = (bb); /* the loop alternates TN_STEP(0) / TN_STEP(1) from t = 0: buffer t & 1 is a literal */ \
    const bool n1 = t + 1 < nk, n2 = t + 2 < nk;                                                                \
    /* ph1: A0 (fragment 3 arrives under the first 12 slots), B0; B1(t) for ph2 */                              \
    PH1(0, 0, bb, RA1(b, 0, 3, 0), RA1(b, 0, 3, 1), RA1(b, 0, 3, 2), RA1(b, 0, 3, 3),                           \
        RB1(1 - bb, b, 1, 0, 0), RB1(1 - bb, b, 1, 0, 1), RB1(1 - bb, b, 1, 0, 2), RB1(1 - bb, b, 1, 0, 3),     \
        RB1(1 - bb, b, 1, 1, 0), RB1(1 - bb, b, 1, 1, 1), RB1(1 - bb, b, 1, 1, 2), RB1(1 - bb, b, 1, 1, 3),     \
        TWO(if (n1) STG_A(b ^ 1, 1, t + 1), NOP_), NOP_, NOP_, NOP_);                                           \
    /* ph2: A0, B1; A1's fragments roll in behind the MFMAs that are done with A0's */                          \
    PH1(0, 1, 1 - bb, NOP_, NOP_, NOP_, NOP_, RA1(b, 1, 0, 0), RA1(b, 1, 0, 1), RA1(b, 1, 0, 2), RA1(b, 1, 0, 3), \
        RA1(b, 1, 1, 0), RA1(b, 1, 1, 1), RA1(b, 1, 1, 2), RA1(b, 1, 1, 3),                                     \
        RA1(b, 1, 2, 0), RA1(b, 1, 2, 1), RA1(b, 1, 2, 2), TWO(RA1(b, 1, 2, 3), TWO(if (n2) STG_A(b, 0, t + 2), NOP_))); \
    /* ph3: A1 (fragment 3 late), B1 */                                                                         \
    PH1(1, 1, 1 - bb, RA1(b, 1, 3, 0), RA1(b, 1, 3, 1), RA1(b, 1, 3, 2), RA1(b, 1, 3, 3),                       \
        TWO(if (n2) STG_B(b, 0, t + 2), NOP_), NOP_, NOP_, NOP_, TWO(if (n2) STG_B(b, 1, t + 2), NOP_), NOP_, NOP_, NOP_, \
        NOP_, NOP_, NOP_, NOP_);                                                                                \
    LANDED(n2);                                                                                                 \
    /* ph4: A1, B0; the next K-tile's A0[0..2] roll in, its B0 goes to the buffer B1 has left */                \
    PH1(1, 0, bb, RB1(1 - bb, b ^ 1, 0, 0, 0), RB1(1 - bb, b ^ 1, 0, 0, 1), RB1(1 - bb, b ^ 1, 0, 0, 2),        \
        RB1(1 - bb, b ^ 1, 0, 0, 3),                                                                            \
        TWO(RA1(b ^ 1, 0, 0, 0), RB1(1 - bb, b ^ 1, 0, 1, 0)), TWO(RA1(b ^ 1, 0, 0, 1), RB1(1 - bb, b ^ 1, 0, 1, 1)), \
        TWO(RA1(b ^ 1, 0, 0, 2), RB1(1 - bb, b ^ 1, 0, 1, 2)), TWO(RA1(b ^ 1, 0, 0, 3), RB1(1 - bb, b ^ 1, 0, 1, 3)), \
        RA1(b ^ 1, 0, 1, 0), RA1(b ^ 1, 0, 1, 1), RA1(b ^ 1, 0, 1, 2), RA1(b ^ 1, 0, 1, 3),                     \
        RA1(b ^ 1, 0, 2, 0), RA1(b ^ 1, 0, 2, 1), RA1(b ^ 1, 0, 2, 2), RA1(b ^ 1, 0, 2, 3));                    \
  } while (0)

// Prologue: K-tile 0 in consumption order (A0 B0 B1 A1), K-tile 1 without its A1 (ph1 of tile 0 issues it), then the wait
// that leaves those three half-tiles in flight.
#define TN_PROLOGUE()                                                \
  if (nk > 0) {                                                      \
    STG_A(0, 0, 0); STG_B(0, 0, 0); STG_B(0, 1, 0); STG_A(0, 1, 0);  \
    if (nk > 1) { STG_A(1, 0, 1); STG_B(1, 0, 1); STG_B(1, 1, 1); }  \
    LANDED(nk > 1);                                                  \
  }                                                                  \
  BARRIER()
// (an empty split, nk = 0, stores zeros)
#define TN_KLOOP()                                                                   \
  if (nk > 0) {                                                                      \
    RA4(0, 0, 0); RA4(0, 0, 1); RA4(0, 0, 2); RB4(0, 0, 0, 0); RB4(0, 0, 0, 1);      \
    int t = 0;                                                                       \
    while (true) {                                                                   \
      TN_STEP(0);                                                                    \
      if (++t >= nk) break;                                                          \
      TN_STEP(1);                                                                    \
      if (++t >= nk) break;                                                          \
    }                                                                                \
    BARRIER();                                                                       \
  }

// Store. D[row = k][col = n] (B fragment first): lane owns dW[n = .. + li][k0 .. k0+3] of its split's slab; OUT4(v) makes
// the float4 that leaves (TN_PLAIN4, or the fp8 kernel's dequantising form).
// The lane's coordinates are re-derived here (from mbcnt, behind an opaque copy): carried across the K loop they — or the
// thread id they come from — cost the registers that decide whether the kernel fits 224 VGPRs.
#define TN_PLAIN4(v) make_float4(v[0], v[1], v[2], v[3])
#define TN_STORE(OUT4)                                                                                               \
  float* out = p.slab + (size_t)split * p.N * p.K;                                                                   \
  int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));  /* the lane id without v0 */ \
  asm volatile("" : "+v"(lane_e));                                                                                   \
  const int li_e = lane_e & 15, fg_e = lane_e >> 4;                                                                  \
  _Pragma("unroll") for (int mh = 0; mh < 2; ++mh)                                                                   \
    _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) {                                                               \
      const int n = bn * 256 + mh * 128 + wm * 64 + mi * 16 + li_e;                                                  \
      if (n >= p.N) continue;                                                                                        \
      _Pragma("unroll") for (int nh = 0; nh < 2; ++nh)                                                               \
        _Pragma("unroll") for (int ni = 0; ni < 2; ++ni) {                                                           \
          const int k0 = bk * 256 + nh * 128 + wn * 32 + ni * 16 + 4 * fg_e;                                         \
          const f32x4 v = acc[mh][mi][nh][ni];                                                                       \
          *(float4*)(out + (size_t)n * p.K + k0) = OUT4(v);                                                          \
        }                                                                                                            \
    }
