// Per-application outputs of the encoder (include/plbert.h: PlbLayerOutputs, plb_encode_bwd_layers), gfx950.
//  attn_probs:   the attention probabilities flash attention never materialises, from what an application leaves behind: its
//                bf16 qkv rows and the log-sum-exp its forward kernel stored. One pass: p = exp2(scale·log2e·(q·k) - LSE), no
//                second normalisation, so these are the probabilities the call's attention used (up to fp32 rounding).
//  add_row_grad: a caller's fp32 gradient of a per-application hidden state joins the residual operand of the dX GEMM that
//                produces that state's gradient.
#include "attn_common.h"
#include "row_common.h"

namespace {

// One workgroup = 4 waves = 128 query rows of one (batch, head), a wave owns 32 queries: the forward's tiling (attn.hip).
// S^T[key][q] = K·Q^T on the 32x32x16 bf16 MFMA, K rows from the forward's LDS row image (LDS-DMA, two stages), Q fragments
// in registers: a lane holds one query and, per accumulator register group, 4 CONSECUTIVE keys. The fp32 probabilities of a
// 64-key tile go through a per-wave LDS patch (32 rows x 64 floats, 272-byte rows: the eight lanes of a 16-byte write group
// cover the 32 banks exactly once) and leave as whole row segments: 16 lanes store the 256 contiguous bytes of one row, a
// wave instruction four rows. The kernel is bound by its stores (B·NH·S·S floats against B·NH·S·64 bf16 of K per 128 rows).
// The workgroup writes EVERY element of its 128 x S tile exactly once: key columns at or past the length and query rows at
// or past it are zeros (key tiles past the length are not computed, a query tile past it is all zero stores), rows at or
// past S do not exist. VEC: S % 4 == 0 and a 16-byte aligned output, 16-byte stores; otherwise scalar stores.
constexpr int PPS = 68;  // floats per patch row

template <bool VEC, bool ZERO>
DEVI void probs_store_rows(const float* patch, float* out_bh, int S, int q0, int k0, int lane) {
  const int c4 = 4 * (lane & 15), c = k0 + c4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 4 * i + (lane >> 4), q = q0 + row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ZERO) v = *(const float4*)&patch[row * PPS + c4];
    if (q < S && c < S) {
      float* d = out_bh + (size_t)q * S + c;
      if (VEC) {
        *(float4*)d = v;   // (S % 4 == 0: c < S covers c + 3)
      } else {
        d[0] = v.x;
        if (c + 1 < S) d[1] = v.y;
        if (c + 2 < S) d[2] = v.z;
        if (c + 3 < S) d[3] = v.w;
      }
    }
  }
}

// KM: key masks (PlbAttn.key_words; kw = the words, ldkw their row stride): a masked key's column is zeros in every row.
// Both forms of the body are instantiated under kernel symbols of their own; KM = false is the code as it always was.
template <bool VEC, bool KM>
DEVI void attn_probs_body(const bf16_t* qkv, int ld, const float* lse, const int32_t* lengths, const int32_t* row_start, int S,
                          int NH, float scale, float* out, const uint32_t* kw, int ldkw) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[2][64 * 64];   // [stage] K row image, 16 KiB
  __shared__ __attribute__((aligned(16))) float spatch[4][32 * PPS];  // per-wave transpose patches, 34 KiB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ATTN_TILE_OF_BLOCK(S, NH);   // (1-D grid, XCD-aware as the forward: the q-tiles of one (batch, head) read the same K)
  const int H = NH * 64;
  const int len = clamp_len(lengths ? lengths[b] : S, S);
  const int q0 = bx * 128 + wave * 32;
  const int lq = lane & 31, h = lane >> 5;
  float* out_bh = out + (size_t)bh * S * S;
  const int nct = (S + 63) >> 6;   // 64-column tiles of the output rows
  float* patch = spatch[wave];
  if (bx * 128 >= len) {   // (workgroup-uniform, before any barrier) no query of this tile is valid: zeros
    if (q0 < S)
      for (int kt = 0; kt < nct; ++kt) probs_store_rows<VEC, true>(patch, out_bh, S, q0, kt * 64, lane);
    return;
  }
  const size_t tok0 = row_start ? (size_t)row_start[b] : (size_t)b * S;   // (token-packed rows: PlbAttn.row_start)
  // rows at or past the length are never read (packed: they may lie outside the sample's slot): the clamped row stands in
  const int qr = min(q0 + lq, len - 1);
  const bool qok = q0 + lq < len;
  bf16x8 qf[4];
  {
    const bf16_t* qp = qkv + hd * 64 + (tok0 + qr) * ld + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  const float sl2 = scale * LOG2E;
  const float lse2 = lse[((size_t)b * NH + hd) * S + qr] * sl2;   // stored as -LSE in raw-score units (PlbAttn.lse)

  const int nkt = (len + 63) >> 6;
  const StageLane g = stage_lane(wave, lane);
  const uint32_t vA0 = (uint32_t)(g.rA * ld + g.cA0) * 2, vA1 = (uint32_t)((g.rA + 8) * ld + g.cA1) * 2;
  const uint32_t lds0 = LDS_ADDR(&smem[0][0]) + (uint32_t)wave * 2048;
  const bf16_t* gk = qkv + H + hd * 64 + tok0 * ld;
#define K_STAGE(ST, kt_)                                                                                 \
  do {                                                                                                   \
    const int k0_ = (kt_) * 64;                                                                          \
    const uint32_t l_ = lds0 + (ST) * 8192;                                                              \
    if (k0_ + 64 <= len) {                                                                               \
      const char* sk_ = (const char*)(gk + (size_t)k0_ * ld);                                            \
      DMA16(sk_, vA0, l_); DMA16(sk_, vA1, l_ + 1024);                                                   \
    } else { /* the tile that crosses the length: rows are clamped, every lane computes its own offsets */ \
      const int a0_ = min(k0_ + g.rA, len - 1), a1_ = min(k0_ + g.rA + 8, len - 1);                      \
      DMA16((const char*)gk, (uint32_t)(a0_ * ld + g.cA0) * 2, l_);                                      \
      DMA16((const char*)gk, (uint32_t)(a1_ * ld + g.cA1) * 2, l_ + 1024);                               \
    }                                                                                                    \
  } while (0)

  int kqo[4];
  row_frag_offsets(lane, kqo);
  uint32_t kwl = 0;   // KM: word i of the sample's row on lane i (S <= 2048), as in the forward
  if constexpr (KM) kwl = lane < 2 * ((S + 63) >> 6) ? kw[(size_t)b * ldkw + lane] : 0u;
  K_STAGE(0, 0);
  DMA_WAIT();
  __syncthreads();
  if constexpr (KM) asm volatile("" : "+v"(kwl));   // (the word's load is consumed before the loop: attn_kernels.h, the forward)
  // One tile of 64 keys out of LDS stage CUR (a literal, as in the forward: every LDS address is a lane constant + an
  // immediate). Register r of s0 is key kt*64 + 4h + (r & 3) + 8 (r >> 2), s1 the same + 32: register group rg holds the
  // four consecutive keys 8 rg + 4h .. + 3 of this lane's query.
#define PROBS_TILE(CUR, kt_)                                                                             \
  do {                                                                                                   \
    const int kt = (kt_);                                                                                \
    if (kt + 1 < nkt) K_STAGE((CUR) ^ 1, kt + 1);                                                        \
    const bf16_t* sK = smem[CUR];                                                                        \
    f32x16 s0 = zero16(), s1 = zero16();                                                                 \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                                   \
      s0 = MFMA32(ROW_FRAG(sK, 0, ks, kqo), qf[ks], s0);                                                 \
      s1 = MFMA32(ROW_FRAG(sK, 1, ks, kqo), qf[ks], s1);                                                 \
    }                                                                                                    \
    uint32_t b0 = ~0u, b1 = ~0u; /* KM: register r = bit 4h + (r & 3) + 8 (r >> 2) of the tile's two words */ \
    if constexpr (KM) {                                                                                  \
      b0 = (uint32_t)__builtin_amdgcn_readlane((int)kwl, 2 * kt) >> (4 * h);                             \
      b1 = (uint32_t)__builtin_amdgcn_readlane((int)kwl, 2 * kt + 1) >> (4 * h);                         \
    }                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                     \
      const int key = kt * 64 + 4 * h + (r & 3) + 8 * (r >> 2);                                          \
      const float p0 = EXP2(__builtin_fmaf(s0[r], sl2, lse2)), p1 = EXP2(__builtin_fmaf(s1[r], sl2, lse2)); \
      if constexpr (KM) { /* (bits at or past the length are clear) */                                   \
        s0[r] = (qok && ((b0 >> ((r & 3) + 8 * (r >> 2))) & 1u)) ? p0 : 0.f;                             \
        s1[r] = (qok && ((b1 >> ((r & 3) + 8 * (r >> 2))) & 1u)) ? p1 : 0.f;                             \
      } else {                                                                                           \
        s0[r] = (qok && key < len) ? p0 : 0.f;                                                           \
        s1[r] = (qok && key + 32 < len) ? p1 : 0.f;                                                      \
      }                                                                                                  \
    }                                                                                                    \
    if (q0 < S) { /* (wave-uniform) */                                                                   \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0): the previous tile's patch reads have landed */  \
      __builtin_amdgcn_wave_barrier();                                                                   \
      _Pragma("unroll") for (int rg = 0; rg < 4; ++rg) {                                                 \
        *(float4*)&patch[lq * PPS + 8 * rg + 4 * h] = make_float4(s0[4 * rg], s0[4 * rg + 1], s0[4 * rg + 2], s0[4 * rg + 3]); \
        *(float4*)&patch[lq * PPS + 32 + 8 * rg + 4 * h] = make_float4(s1[4 * rg], s1[4 * rg + 1], s1[4 * rg + 2], s1[4 * rg + 3]); \
      }                                                                                                  \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* the patch is private to this wave */                        \
      __builtin_amdgcn_wave_barrier();                                                                   \
      probs_store_rows<VEC, false>(patch, out_bh, S, q0, kt * 64, lane);                                 \
    }                                                                                                    \
    DMA_WAIT();                                                                                          \
    TILE_SYNC();                                                                                         \
  } while (0)
  for (int kt2 = 0; kt2 < nkt; kt2 += 2) {
    PROBS_TILE(0, kt2);
    if (kt2 + 1 < nkt) PROBS_TILE(1, kt2 + 1);
  }
#undef PROBS_TILE
#undef K_STAGE
  // key tiles past the length: zeros, nothing computed
  if (q0 < S)
    for (int kt = nkt; kt < nct; ++kt) probs_store_rows<VEC, true>(patch, out_bh, S, q0, kt * 64, lane);
}
template <bool VEC>
__global__ __launch_bounds__(256) void attn_probs_kernel(const bf16_t* qkv, int ld, const float* lse, const int32_t* lengths,
                                                         const int32_t* row_start, int S, int NH, float scale, float* out) {
  attn_probs_body<VEC, false>(qkv, ld, lse, lengths, row_start, S, NH, scale, out, nullptr, 0);
}
template <bool VEC>
__global__ __launch_bounds__(256) void attn_probs_km_kernel(const bf16_t* qkv, int ld, const float* lse, const int32_t* lengths,
                                                            const int32_t* row_start, int S, int NH, float scale, float* out,
                                                            const uint32_t* kw, int ldkw) {
  attn_probs_body<VEC, true>(qkv, ld, lse, lengths, row_start, S, NH, scale, out, kw, ldkw);
}

}  // namespace

extern "C" int plb_launch_attn_probs(const bf16_t* qkv, int ldqkv, const float* lse, const int32_t* lengths,
                                     const int32_t* row_start, int B, int S, int NH, float scale, float* out,
                                     hipStream_t stream) {
  return plb_launch_attn_probs_masked(qkv, ldqkv, lse, lengths, row_start, nullptr, 0, B, S, NH, scale, out, stream);
}

extern "C" int plb_launch_attn_probs_masked(const bf16_t* qkv, int ldqkv, const float* lse, const int32_t* lengths,
                                            const int32_t* row_start, const uint32_t* key_words, int ldkw, int B, int S, int NH,
                                            float scale, float* out, hipStream_t stream) {
  // the shape part of the attention launchers' check, on the descriptor these arguments would make
  PlbAttn a = {};
  a.qkv = qkv; a.ldqkv = ldqkv; a.lse = const_cast<float*>(lse); a.lengths = lengths; a.row_start = row_start;
  a.key_words = key_words; a.ldkw = ldkw; a.B = B; a.S = S; a.NH = NH; a.H = (int)((int64_t)NH * 64);
  if (plb_attn_args_check(&a, PLB_ATTN_PROBS)) return 1;
  if (!out || ldqkv < (int64_t)3 * NH * 64 || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 3)) return 1;
  PlbAttnPlan pl;
  plb_attn_plan(B, S, NH, plb_attn_flags(&a), &pl);
  const dim3 grid(pl.grid), block(pl.block);
  const double elems = (double)B * NH * (double)S * S;
  ProfScope ps(PLB_K_ROWS, stream, 2.0 * elems * 64.0, 4.0 * elems);
  const bool vec = S % 4 == 0 && !((uintptr_t)out & 15);
  if (pl.km) {
    if (vec) hipLaunchKernelGGL(attn_probs_km_kernel<true>, grid, block, 0, stream, qkv, ldqkv, lse, lengths, row_start, S, NH, scale, out, key_words, ldkw);
    else hipLaunchKernelGGL(attn_probs_km_kernel<false>, grid, block, 0, stream, qkv, ldqkv, lse, lengths, row_start, S, NH, scale, out, key_words, ldkw);
  } else {
    if (vec) hipLaunchKernelGGL(attn_probs_kernel<true>, grid, block, 0, stream, qkv, ldqkv, lse, lengths, row_start, S, NH, scale, out);
    else hipLaunchKernelGGL(attn_probs_kernel<false>, grid, block, 0, stream, qkv, ldqkv, lse, lengths, row_start, S, NH, scale, out);
  }
  return LAUNCH_OK();
}

namespace {
// out[r] = bf16(float(res[r]) + g[b,s,:]) (round to nearest even) on the row that holds token (b, s < lengths[b]), out[r] =
// res[r] on every other of the Tp rows (pad positions, the rest of a packed slot, the tail): ONE pass writes every row
// exactly once and g is never read at a pad position. The row lookup and the lane layout are seed_dy_kernel's
// (loss_rows.hip): one lane per four columns, 16-byte load of g, 8-byte load and store of the bf16 rows.
__global__ __launch_bounds__(256) void add_row_grad_kernel(const bf16_t* res, const float* g, const int32_t* lengths,
                                                           const int32_t* row_start, int B, int S, int H4, unsigned int total,
                                                           bf16_t* out) {
  for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int r = (int)(i / (unsigned int)H4), c = (int)(i - (unsigned int)r * (unsigned int)H4);
    int b = 0, s = 0;
    bool live;
    if (row_start) {
      live = packed_locate(row_start, lengths, B, S, r, &b, &s);
    } else {
      b = r / S; s = r - b * S;
      live = b < B;
      if (live && lengths) live = s < clamp_len(lengths[b], S);
    }
    uint2 o = *(const uint2*)(res + (size_t)i * 4);
    if (live) {
      const float4 v = *(const float4*)(g + ((size_t)b * S + s) * ((size_t)H4 * 4) + (size_t)c * 4);
      o.x = pack_bf2(bf_lo(o.x) + v.x, bf_hi(o.x) + v.y);
      o.y = pack_bf2(bf_lo(o.y) + v.z, bf_hi(o.y) + v.w);
    }
    *(uint2*)(out + (size_t)i * 4) = o;
  }
}
}  // namespace

extern "C" int plb_launch_add_row_grad(const bf16_t* res, const float* g, const int32_t* lengths, const int32_t* row_start, int B,
                                       int S, int H, int Tp, bf16_t* out, hipStream_t stream) {
  if (!res || !g || !out || B < 1 || S < 1 || H < 4 || H % 4 || Tp < 1) return 1;
  if (row_start ? !lengths : (int64_t)Tp < (int64_t)B * S) return 1;   // (packed: the plan's rows; padded: at least B*S of them)
  if (((uintptr_t)g & 15) || ((uintptr_t)res & 7) || ((uintptr_t)out & 7)) return 1;
  const int64_t total = (int64_t)Tp * (H / 4);
  if (total >= ((int64_t)1 << 31)) return 1;
  const int64_t blocks = (total + 255) / 256;
  ProfScope ps(PLB_K_ROWS, stream, 0, (double)Tp * H * 8.0);
  hipLaunchKernelGGL(add_row_grad_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, res, g, lengths,
                     row_start, B, S, H / 4, (unsigned int)total, out);
  return LAUNCH_OK();
}
