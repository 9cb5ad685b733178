// LayerNorm(H) of the PL-BERT step, gfx950 (A7/A8): forward and backward, HBM-bound.
// nn.LayerNorm over the last dim, biased variance, eps inside the sqrt; fp32 statistics (layer_norm_eps = 1e-12 is
// below bf16 resolution). Two forms of each direction: the 8-byte form for any H % 4 == 0, H <= 1024 (NCH = ceil(H/256)),
// and the 16-byte form for the model widths H = 768 / 1024, which also writes the fp8 image of its output.
// Rows are dealt to workgroups through xcd_remap: XCD x then owns the same contiguous eighth of the token rows
// as in the GEMMs and the attention kernels that produce / consume them (worth 0.05 ms per step, measured).
// The backward keeps the padding rows [T, Tzero) of dx zero so they add nothing to the batched dW GEMMs, and leaves
// partials[block][dgamma | dbeta | colsum(dx)] for the column reduction (reduce.hip).
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
// A wave handles LN_R rows per iteration with all their loads issued before the first reduction:
// the kernels are pure HBM streams and one row per wave (3 x 8 B per lane) left them latency-bound.
constexpr int LN_R = 2;
// the backward keeps x, dy and three accumulator sets per lane: one row in flight per wave (more waves per SIMD)
// measured 16.5 vs 18.7 us at 16384 x 768 (tools/ln_bench.py)
constexpr int LN_RB = 1;
constexpr int LNW_FWD_BLOCKS = 2048;   // grid cap of the 16-byte forward

template <int NCH>
__global__ __launch_bounds__(256) void ln_fwd_kernel(PlbLayerNorm p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = p.H;
  const float invH = 1.0f / (float)H;
  float4 g[NCH], b[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 4;
    g[i] = (c < H) ? *(const float4*)(p.gamma + c) : make_float4(0, 0, 0, 0);
    b[i] = (c < H) ? *(const float4*)(p.beta + c) : make_float4(0, 0, 0, 0);
  }
  for (int t0 = (xcd_remap(blockIdx.x, gridDim.x) * 4 + wave) * LN_R; t0 < p.T; t0 += gridDim.x * 4 * LN_R) {
    uint2 u[LN_R][NCH];
#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
      const int t = (t0 + r < p.T) ? t0 + r : p.T - 1;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 4;
        u[r][i] = (c < H) ? *(const uint2*)(p.x + (size_t)t * p.ldx + c) : make_uint2(0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
      const int t = t0 + r;
      float x[NCH][4], s = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        x[i][0] = bf_lo(u[r][i].x); x[i][1] = bf_hi(u[r][i].x); x[i][2] = bf_lo(u[r][i].y); x[i][3] = bf_hi(u[r][i].y);
        s += x[i][0] + x[i][1] + x[i][2] + x[i][3];
      }
      const float mean = wave_sum(s) * invH;
      float vs = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[i][j] = (c < H) ? x[i][j] - mean : 0.f; vs += x[i][j] * x[i][j]; }
      }
      const float rstd = rsqrtf(wave_sum(vs) * invH + p.eps);
      if (t < p.T) {
        if (lane == 0 && p.mean) { p.mean[t] = mean; p.rstd[t] = rstd; }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = (lane + 64 * i) * 4;
          if (c < H) {
            uint2 o;
            o.x = pack_bf2(x[i][0] * rstd * g[i].x + b[i].x, x[i][1] * rstd * g[i].y + b[i].y);
            o.y = pack_bf2(x[i][2] * rstd * g[i].z + b[i].z, x[i][3] * rstd * g[i].w + b[i].w);
            *(uint2*)(p.y + (size_t)t * p.ldy + c) = o;
          }
        }
      }
    }
  }
}

// ---- 16-byte form for the model widths (H = 768: 96 chunks of 8 bf16 per row, H = 1024: 128) -------------------------
// A wave takes RW consecutive rows as ONE run of RW*CPR 16-byte chunks, NL = RW*CPR/64 loads per lane (lane l, load i:
// chunk l + 64 i -> row (l + 64 i) / CPR, columns ((l + 64 i) % CPR) * 8 ...): full 1-KiB wave loads and stores, half
// the memory instructions of the 8-byte form, and LNW_GROUPS row groups in flight per wave before the first
// reduction. H = 768: RW = 2, NL = 3 (load 1 straddles the two rows); H = 1024: RW = 1, NL = 2.
constexpr int LNW_GROUPS = 2;
template <int CPR> struct LnWide {
  static constexpr int RW = (CPR == 96) ? 2 : 1;
  static constexpr int NL = RW * CPR / 64;
  static_assert(RW * CPR % 64 == 0, "row group must fill whole wave loads");
};

template <int CPR>
__global__ __launch_bounds__(256) void ln_fwd_wide_kernel(PlbLayerNorm p) {
  constexpr int RW = LnWide<CPR>::RW, NL = LnWide<CPR>::NL, G = LNW_GROUPS, H = CPR * 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invH = 1.0f / (float)H;
  const float qs = p.out8 ? p.q_scale[0] : 1.0f;
  float amax = 0.f;
  int lrow[NL], lcol[NL];
  float gm[NL][8], bt[NL][8];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int c = lane + 64 * i;
    lrow[i] = c / CPR; lcol[i] = (c % CPR) * 8;
    const float4 g0 = *(const float4*)(p.gamma + lcol[i]), g1 = *(const float4*)(p.gamma + lcol[i] + 4);
    const float4 b0 = *(const float4*)(p.beta + lcol[i]), b1 = *(const float4*)(p.beta + lcol[i] + 4);
    gm[i][0] = g0.x; gm[i][1] = g0.y; gm[i][2] = g0.z; gm[i][3] = g0.w; gm[i][4] = g1.x; gm[i][5] = g1.y; gm[i][6] = g1.z; gm[i][7] = g1.w;
    bt[i][0] = b0.x; bt[i][1] = b0.y; bt[i][2] = b0.z; bt[i][3] = b0.w; bt[i][4] = b1.x; bt[i][5] = b1.y; bt[i][6] = b1.z; bt[i][7] = b1.w;
  }
  const int step = gridDim.x * 4 * RW * G;
  for (int t0 = (xcd_remap(blockIdx.x, gridDim.x) * 4 + wave) * RW * G; t0 < p.T; t0 += step) {
    uint4 u[G][NL];
#pragma unroll
    for (int gI = 0; gI < G; ++gI)
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        int t = t0 + gI * RW + lrow[i];
        t = t < p.T ? t : p.T - 1;
        u[gI][i] = *(const uint4*)(p.x + (size_t)t * p.ldx + lcol[i]);
      }
#pragma unroll
    for (int gI = 0; gI < G; ++gI) {
      float x[NL][8], rs[RW], mean[RW], rstd[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) rs[r] = 0.f;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        unpack8(u[gI][i], x[i]);
        const float s = ((x[i][0] + x[i][1]) + (x[i][2] + x[i][3])) + ((x[i][4] + x[i][5]) + (x[i][6] + x[i][7]));
#pragma unroll
        for (int r = 0; r < RW; ++r) rs[r] += (lrow[i] == r) ? s : 0.f;
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) { mean[r] = wave_sum(rs[r]) * invH; rs[r] = 0.f; }
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        float mu = mean[0];
#pragma unroll
        for (int r = 1; r < RW; ++r) mu = (lrow[i] == r) ? mean[r] : mu;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { x[i][j] -= mu; v += x[i][j] * x[i][j]; }
#pragma unroll
        for (int r = 0; r < RW; ++r) rs[r] += (lrow[i] == r) ? v : 0.f;
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) rstd[r] = rsqrtf(wave_sum(rs[r]) * invH + p.eps);
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int t = t0 + gI * RW + r;
        if (lane == 0 && p.mean && t < p.T) { p.mean[t] = mean[r]; p.rstd[t] = rstd[r]; }
      }
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        float rsd = rstd[0];
#pragma unroll
        for (int r = 1; r < RW; ++r) rsd = (lrow[i] == r) ? rstd[r] : rsd;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = x[i][j] * rsd * gm[i][j] + bt[i][j];
        const int t = t0 + gI * RW + lrow[i];
        if (t < p.T) {
          const uint4 pk = pack8(o);
          *(uint4*)(p.y + (size_t)t * p.ldy + lcol[i]) = pk;
          if (p.out8) {  // e4m3 image of the row as stored in bf16, for the fp8 GEMM that consumes it
            float q[8];
            unpack8(pk, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(q[j]));
            uint2 w;
            w.x = pack_fp8x4(q[0] * qs, q[1] * qs, q[2] * qs, q[3] * qs, false);
            w.y = pack_fp8x4(q[4] * qs, q[5] * qs, q[6] * qs, q[7] * qs, false);
            *(uint2*)(p.out8 + (size_t)t * p.ld8 + lcol[i]) = w;
          }
        }
      }
    }
  }
  if (p.out8 && p.q_amax) {
    amax = wave_max(amax);
    if (lane == 0) atomic_max_abs(p.q_amax, amax, blockIdx.x * 4 + wave);
  }
}
}  // namespace
extern "C" int plb_launch_ln_fwd(const PlbLayerNorm* p, hipStream_t stream) {
  if (p->H % 4 || p->H > 1024 || p->T <= 0) return 1;
  int blocks = (p->T + 4 * LN_R - 1) / (4 * LN_R); if (blocks > 4096) blocks = 4096;
  ProfScope ps(PLB_K_LN_FWD, stream, 0, (double)p->T * (4.0 * p->H + 8));
  const bool fwide_ok = (p->H == 768 || p->H == 1024) && p->ldx % 8 == 0 && p->ldy % 8 == 0;
  if (p->out8 && !fwide_ok) return 1;
  if (fwide_ok) {
    const int rows_per_block = 4 * (p->H == 768 ? 2 : 1) * LNW_GROUPS;
    int wb = (p->T + rows_per_block - 1) / rows_per_block; if (wb > LNW_FWD_BLOCKS) wb = LNW_FWD_BLOCKS;
    if (p->H == 768) hipLaunchKernelGGL((ln_fwd_wide_kernel<96>), dim3(wb), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL((ln_fwd_wide_kernel<128>), dim3(wb), dim3(256), 0, stream, *p);
    return LAUNCH_OK();
  }
  const int nch = (p->H + 255) / 256;
  switch (nch) {
    case 1: hipLaunchKernelGGL((ln_fwd_kernel<1>), dim3(blocks), dim3(256), 0, stream, *p); break;
    case 2: hipLaunchKernelGGL((ln_fwd_kernel<2>), dim3(blocks), dim3(256), 0, stream, *p); break;
    case 3: hipLaunchKernelGGL((ln_fwd_kernel<3>), dim3(blocks), dim3(256), 0, stream, *p); break;
    default: hipLaunchKernelGGL((ln_fwd_kernel<4>), dim3(blocks), dim3(256), 0, stream, *p); break;
  }
  return LAUNCH_OK();
}

namespace {
template <int NCH>
__global__ __launch_bounds__(256) void ln_bwd_kernel(PlbLayerNorm p) {
  __shared__ float red[4][3][NCH * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = p.H;
  const float invH = 1.0f / (float)H;
  float dg[NCH][4], db[NCH][4], gm[NCH][4], dxs[NCH][4];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 4;
    float4 g = (c < H) ? *(const float4*)(p.gamma + c) : make_float4(0, 0, 0, 0);
    gm[i][0] = g.x; gm[i][1] = g.y; gm[i][2] = g.z; gm[i][3] = g.w;
#pragma unroll
    for (int j = 0; j < 4; ++j) dg[i][j] = db[i][j] = dxs[i][j] = 0.f;
  }
  for (int t0 = (xcd_remap(blockIdx.x, gridDim.x) * 4 + wave) * LN_RB; t0 < p.T; t0 += gridDim.x * 4 * LN_RB) {
    uint2 ux[LN_RB][NCH], ud[LN_RB][NCH];
    float mean[LN_RB], rstd[LN_RB];
#pragma unroll
    for (int r = 0; r < LN_RB; ++r) {
      const int t = (t0 + r < p.T) ? t0 + r : p.T - 1;
      mean[r] = p.mean[t]; rstd[r] = p.rstd[t];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 4;
        ux[r][i] = (c < H) ? *(const uint2*)(p.x + (size_t)t * p.ldx + c) : make_uint2(0, 0);
        ud[r][i] = (c < H) ? *(const uint2*)(p.dy + (size_t)t * p.lddy + c) : make_uint2(0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < LN_RB; ++r) {
      const int t = t0 + r;
      if (t >= p.T) continue;  // wave-uniform
      float xh[NCH][4], dxh[NCH][4];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 4;
        const float xv[4] = {bf_lo(ux[r][i].x), bf_hi(ux[r][i].x), bf_lo(ux[r][i].y), bf_hi(ux[r][i].y)};
        const float dyv[4] = {bf_lo(ud[r][i].x), bf_hi(ud[r][i].x), bf_lo(ud[r][i].y), bf_hi(ud[r][i].y)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[i][j] = (c < H) ? (xv[j] - mean[r]) * rstd[r] : 0.f;
          dxh[i][j] = dyv[j] * gm[i][j];
          s1 += dxh[i][j]; s2 += dxh[i][j] * xh[i][j];
          dg[i][j] += dyv[j] * xh[i][j]; db[i][j] += dyv[j];
        }
      }
      s1 = wave_sum(s1) * invH; s2 = wave_sum(s2) * invH;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < H) {
          uint2 o;
          o.x = pack_bf2(rstd[r] * (dxh[i][0] - s1 - xh[i][0] * s2), rstd[r] * (dxh[i][1] - s1 - xh[i][1] * s2));
          o.y = pack_bf2(rstd[r] * (dxh[i][2] - s1 - xh[i][2] * s2), rstd[r] * (dxh[i][3] - s1 - xh[i][3] * s2));
          *(uint2*)(p.dx + (size_t)t * p.lddx + c) = o;
          // column sums of dx as stored: the bias gradient of the Linear whose output this LayerNorm normalised
          dxs[i][0] += bf_lo(o.x); dxs[i][1] += bf_hi(o.x); dxs[i][2] += bf_lo(o.y); dxs[i][3] += bf_hi(o.y);
        }
      }
    }
  }
  // padding rows of the token dimension: keep them zero so they add nothing to the batched dW GEMMs
  for (int t = p.T + blockIdx.x * 4 + wave; t < p.Tzero; t += gridDim.x * 4) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < H) *(uint2*)(p.dx + (size_t)t * p.lddx + c) = make_uint2(0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { red[wave][0][c + j] = dg[i][j]; red[wave][1][c + j] = db[i][j]; red[wave][2][c + j] = dxs[i][j]; }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * H; i += 256) {  // partials[block][dgamma | dbeta | colsum(dx)]
    const int which = i / H, col = i % H;
    float* dst = &p.partials[(size_t)blockIdx.x * 3 * H + i];
    const float v = red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
    *dst = p.accumulate ? *dst + v : v;
  }
}

template <int CPR>
__global__ __launch_bounds__(256) void ln_bwd_wide_kernel(PlbLayerNorm p) {
  constexpr int RW = LnWide<CPR>::RW, NL = LnWide<CPR>::NL, H = CPR * 8;
  __shared__ float red[4][3][H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invH = 1.0f / (float)H;
  const float qs = p.out8 ? p.q_scale[0] : 1.0f;
  float amax = 0.f;
  int lrow[NL], lcol[NL];
  float gm[NL][8], dg[NL][8], db[NL][8], dxs[NL][8];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int c = lane + 64 * i;
    lrow[i] = c / CPR; lcol[i] = (c % CPR) * 8;
    const float4 g0 = *(const float4*)(p.gamma + lcol[i]), g1 = *(const float4*)(p.gamma + lcol[i] + 4);
    gm[i][0] = g0.x; gm[i][1] = g0.y; gm[i][2] = g0.z; gm[i][3] = g0.w; gm[i][4] = g1.x; gm[i][5] = g1.y; gm[i][6] = g1.z; gm[i][7] = g1.w;
#pragma unroll
    for (int j = 0; j < 8; ++j) dg[i][j] = db[i][j] = dxs[i][j] = 0.f;
  }
  const int step = gridDim.x * 4 * RW;
  int t0 = (xcd_remap(blockIdx.x, gridDim.x) * 4 + wave) * RW;
  // one row group ahead: the loads of group k+1 are in flight while group k is reduced and stored
  uint4 nx[NL], nd[NL];
  float nmean[NL], nrstd[NL];
#define LNW_LOAD(tb)                                                                          \
  _Pragma("unroll") for (int i = 0; i < NL; ++i) {                                            \
    int t_ = (tb) + lrow[i];                                                                  \
    t_ = t_ < p.T ? t_ : p.T - 1;                                                             \
    nx[i] = *(const uint4*)(p.x + (size_t)t_ * p.ldx + lcol[i]);                              \
    nd[i] = *(const uint4*)(p.dy + (size_t)t_ * p.lddy + lcol[i]);                            \
    nmean[i] = p.mean[t_]; nrstd[i] = p.rstd[t_];                                             \
  }
  if (t0 < p.T) { LNW_LOAD(t0); }
  for (; t0 < p.T; t0 += step) {
    uint4 ux[NL], ud[NL];
    float mean[NL], rstd[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) { ux[i] = nx[i]; ud[i] = nd[i]; mean[i] = nmean[i]; rstd[i] = nrstd[i]; }
    if (t0 + step < p.T) { LNW_LOAD(t0 + step); }
    float xh[NL][8], dxh[NL][8], s1[RW], s2[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) s1[r] = s2[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      float xv[8], dyv[8];
      unpack8(ux[i], xv);
      unpack8(ud[i], dyv);
      const bool live = t0 + lrow[i] < p.T;
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = live ? dyv[j] : 0.f;
        xh[i][j] = (xv[j] - mean[i]) * rstd[i];
        dxh[i][j] = d * gm[i][j];
        a1 += dxh[i][j]; a2 += dxh[i][j] * xh[i][j];
        dg[i][j] += d * xh[i][j]; db[i][j] += d;
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) { s1[r] += (lrow[i] == r) ? a1 : 0.f; s2[r] += (lrow[i] == r) ? a2 : 0.f; }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) { s1[r] = wave_sum(s1[r]) * invH; s2[r] = wave_sum(s2[r]) * invH; }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      float m1 = s1[0], m2 = s2[0];
#pragma unroll
      for (int r = 1; r < RW; ++r) { m1 = (lrow[i] == r) ? s1[r] : m1; m2 = (lrow[i] == r) ? s2[r] : m2; }
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rstd[i] * (dxh[i][j] - m1 - xh[i][j] * m2);
      const uint4 pk = pack8(o);
      if (t0 + lrow[i] < p.T) {
        *(uint4*)(p.dx + (size_t)(t0 + lrow[i]) * p.lddx + lcol[i]) = pk;
        float q[8];
        unpack8(pk, q);  // column sums of dx as stored
#pragma unroll
        for (int j = 0; j < 8; ++j) dxs[i][j] += q[j];
        if (p.out8) {  // e5m2 image of the gradient row for the fp8 dX GEMM
#pragma unroll
          for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(q[j]));
          uint2 w;
          w.x = pack_fp8x4(q[0] * qs, q[1] * qs, q[2] * qs, q[3] * qs, true);
          w.y = pack_fp8x4(q[4] * qs, q[5] * qs, q[6] * qs, q[7] * qs, true);
          *(uint2*)(p.out8 + (size_t)(t0 + lrow[i]) * p.ld8 + lcol[i]) = w;
        }
      }
    }
  }
#undef LNW_LOAD
  if (p.out8 && p.q_amax) {
    amax = wave_max(amax);
    if (lane == 0) atomic_max_abs(p.q_amax, amax, blockIdx.x * 4 + wave);
  }
  // padding rows of the token dimension: keep them zero so they add nothing to the batched dW GEMMs
  for (int t = p.T + blockIdx.x * 4 + wave; t < p.Tzero; t += gridDim.x * 4)
    for (int c = lane; c < CPR; c += 64) {
      *(uint4*)(p.dx + (size_t)t * p.lddx + c * 8) = make_uint4(0, 0, 0, 0);
      if (p.out8) *(uint2*)(p.out8 + (size_t)t * p.ld8 + c * 8) = make_uint2(0, 0);
    }
  // per-block partials: loads i and i' of one lane set can hold the same columns (H = 768: load 1 wraps), so the NL
  // slots are folded into the wave's LDS row one after the other
#pragma unroll
  for (int i = 0; i < NL; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float* r0 = &red[wave][0][lcol[i] + j];
      if (i == 0 || (CPR == 128)) {  // first touch of these columns by this wave (H = 1024: the two loads are disjoint)
        r0[0] = dg[i][j]; r0[H] = db[i][j]; r0[2 * H] = dxs[i][j];
      }
    }
    if (CPR != 128 && i + 1 < NL) __builtin_amdgcn_wave_barrier();
  }
  if (CPR != 128) {
    // H = 768: load 0 covered columns [0,512); load 1 lanes 0-31 cover [512,768) (first touch), lanes 32-63 [0,256)
    // (second touch); load 2 covers [256,768) (second touch)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float* r1 = &red[wave][0][lcol[1] + j];
      if (lane < 32) { r1[0] = dg[1][j]; r1[H] = db[1][j]; r1[2 * H] = dxs[1][j]; }
      else { r1[0] += dg[1][j]; r1[H] += db[1][j]; r1[2 * H] += dxs[1][j]; }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float* r2 = &red[wave][0][lcol[2] + j];
      r2[0] += dg[2][j]; r2[H] += db[2][j]; r2[2 * H] += dxs[2][j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * H; i += 256) {
    const int which = i / H, col = i % H;
    float* dst = &p.partials[(size_t)blockIdx.x * 3 * H + i];
    const float v = red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
    *dst = p.accumulate ? *dst + v : v;
  }
}
}  // namespace
extern "C" int plb_launch_ln_bwd(const PlbLayerNorm* p, hipStream_t stream) {
  if (p->H % 4 || p->H > 1024 || p->T <= 0 || p->nblocks <= 0) return 1;
  ProfScope ps(PLB_K_LN_BWD, stream, 0, (double)p->T * (6.0 * p->H + 8));
  const bool wide_ok = (p->H == 768 || p->H == 1024) && p->ldx % 8 == 0 && p->lddy % 8 == 0 && p->lddx % 8 == 0;
  if (p->out8 && !wide_ok) return 1;  // the fp8 copy exists in the 16-byte kernels only
  // measured (tools/ln_bench.py): at H = 1024 the 16-byte form wins (14.2 vs 17.1 us at 8192 rows), at H = 768 its
  // straddling middle load costs more than it saves (21.5 vs 18.7 us at 16384 rows): used there only for the fp8 copy
  if (wide_ok && (p->out8 || p->H == 1024)) {
    if (p->H == 768) hipLaunchKernelGGL((ln_bwd_wide_kernel<96>), dim3(p->nblocks), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL((ln_bwd_wide_kernel<128>), dim3(p->nblocks), dim3(256), 0, stream, *p);
    return LAUNCH_OK();
  }
  const int nch = (p->H + 255) / 256;
  switch (nch) {
    case 1: hipLaunchKernelGGL((ln_bwd_kernel<1>), dim3(p->nblocks), dim3(256), 0, stream, *p); break;
    case 2: hipLaunchKernelGGL((ln_bwd_kernel<2>), dim3(p->nblocks), dim3(256), 0, stream, *p); break;
    case 3: hipLaunchKernelGGL((ln_bwd_kernel<3>), dim3(p->nblocks), dim3(256), 0, stream, *p); break;
    default: hipLaunchKernelGGL((ln_bwd_kernel<4>), dim3(p->nblocks), dim3(256), 0, stream, *p); break;
  }
  return LAUNCH_OK();
}
