// Backward of the AlbertModel pooler, gfx950 (plb_encode_bwd_pooled): pooled[b,:] = tanh(W · h[b,0,:] + bias), h the bf16 rows of
// the final hidden state. Four small launches, latency-bound (B <= max_batch, H <= 1024):
//   dpre[b,o] = d_pooled[b,o] * (1 - y*y), y recomputed with pooler_kernel's arithmetic (loss_rows.hip: one wave per output
//               feature, lane l takes columns 4l + 256k, the same float4 expression, wave_sum, tanhf) from the fp32 image of the
//               bf16 row — the values plb_pooler read from the fp32 hidden state of the same call, so y has plb_pooler's bits;
//   dW[o,i]   = sum_b dpre[b,o] * h[b,0,i],  db[o] = sum_b dpre[b,o]      (b ascending, one thread per four columns of a row);
//   dh0[b,i]  = sum_o dpre[b,o] * W[o,i]     (lanes along i: a wave reads 256 contiguous bytes of a row of W; the four waves of a
//               workgroup take one quarter of the rows each, o ascending, and the quarter sums are added in order);
//   dy[row of (b,0), :] = bf16(d_hidden[b,0,:] + dh0[b,:])  (one fp32 add, round to nearest even as seed_dy_kernel), over the
//               B rows only, behind the launch that seeded every row of dy.
// Every sum has a fixed order and there are no atomics: results are bitwise reproducible from run to run. Sample b's row is
// rows[b] (token-packed: the plan's row_start) or b*S.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
DEVI size_t first_row(const int32_t* rows, int b, int S) { return rows ? (size_t)rows[b] : (size_t)b * S; }
DEVI float4 bf4(const bf16_t* p) {
  const uint2 u = *(const uint2*)p;
  return make_float4(bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y));
}

__global__ __launch_bounds__(256) void pooler_dpre_kernel(const bf16_t* hidden, int ldh, const int32_t* rows, int S, int H,
                                                          const float* W, const float* bias, const float* d_pooled, float* dpre) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= H) return;
  const bf16_t* x = hidden + first_row(rows, b, S) * ldh;
  const float* w = W + (size_t)o * H;
  float s = 0.f;
  for (int k = lane * 4; k < H; k += 256) {
    const float4 a = bf4(x + k), c = *(const float4*)(w + k);
    s += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float y = tanhf(s + bias[o]);
    dpre[(size_t)b * H + o] = d_pooled[(size_t)b * H + o] * (1.f - y * y);
  }
}

// one thread per four columns i of row o of dW; the thread of columns 0..3 also sums db[o]
__global__ __launch_bounds__(256) void pooler_dw_kernel(const bf16_t* hidden, int ldh, const int32_t* rows, int B, int S, int H,
                                                        const float* dpre, float* dW, float* db) {
  const int H4 = H / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * H4) return;
  const int o = idx / H4, i = (idx - o * H4) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float sb = 0.f;
  for (int b = 0; b < B; ++b) {
    const float d = dpre[(size_t)b * H + o];
    const float4 h = bf4(hidden + first_row(rows, b, S) * ldh + i);
    acc.x += d * h.x; acc.y += d * h.y; acc.z += d * h.z; acc.w += d * h.w;
    sb += d;
  }
  *(float4*)(dW + (size_t)idx * 4) = acc;
  if (i == 0) db[o] = sb;
}

// One workgroup per (64 columns i, sample b): wave w sums rows [w H/4, (w+1) H/4) of W, o ascending (dpre[b,o] is uniform in
// the wave), then ((q0 + q1) + q2) + q3 through LDS. One wave over all H rows was 166 us at 32 x 768: a chain of H dependent
// loads' latencies on a quarter of the chip.
__global__ __launch_bounds__(256) void pooler_dh0_kernel(int H, const float* __restrict__ W, const float* __restrict__ dpre,
                                                         float* __restrict__ dh0) {
  __shared__ float part[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane, q = H / 4;
  const float* d = dpre + (size_t)b * H + w * q;
  const float* wp = W + (size_t)(w * q) * H + i;
  float acc = 0.f;
#pragma unroll 8
  for (int o = 0; o < q; ++o) acc += d[o] * wp[(size_t)o * H];
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0) dh0[(size_t)b * H + i] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

__global__ __launch_bounds__(256) void seed_dy_first_rows_kernel(const float* d_hidden, const float* dh0, const int32_t* rows, int B,
                                                                 int S, int H4, bf16_t* dy) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H4) return;
  const int b = idx / H4, c = idx - b * H4;
  const size_t H = (size_t)H4 * 4;
  const float4 a = *(const float4*)(dh0 + (size_t)b * H + (size_t)c * 4);
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (d_hidden) g = *(const float4*)(d_hidden + (size_t)b * S * H + (size_t)c * 4);
  uint2 o;
  o.x = pack_bf2(g.x + a.x, g.y + a.y); o.y = pack_bf2(g.z + a.z, g.w + a.w);
  *(uint2*)(dy + first_row(rows, b, S) * H + (size_t)c * 4) = o;
}
}  // namespace

extern "C" int plb_launch_pooler_bwd(const bf16_t* hidden, int ldh, const int32_t* rows, int B, int S, int H, const float* W,
                                     const float* bias, const float* d_pooled, float* dpre, float* dW, float* db, float* dh0,
                                     hipStream_t stream) {
  if (!hidden || !W || !bias || !d_pooled || !dpre || !dW || !db || !dh0) return 1;
  if (B < 1 || S < 1 || H < 64 || H % 64 || ldh < H || ldh % 4) return 1;
  if (((uintptr_t)hidden & 7) || (((uintptr_t)W | (uintptr_t)dW | (uintptr_t)d_pooled) & 15)) return 1;
  if ((int64_t)B * H >= ((int64_t)1 << 31) / 4) return 1;
  ProfScope ps(PLB_K_ROWS, stream, 2.0 * B * H * H * 3.0, 4.0 * H * H * 3.0);
  hipLaunchKernelGGL(pooler_dpre_kernel, dim3((H + 3) / 4, B), dim3(256), 0, stream, hidden, ldh, rows, S, H, W, bias, d_pooled, dpre);
  hipLaunchKernelGGL(pooler_dw_kernel, dim3((unsigned)((H * (H / 4) + 255) / 256)), dim3(256), 0, stream, hidden, ldh, rows, B, S, H,
                     dpre, dW, db);
  hipLaunchKernelGGL(pooler_dh0_kernel, dim3(H / 64, B), dim3(256), 0, stream, H, W, dpre, dh0);
  return LAUNCH_OK();
}

extern "C" int plb_launch_seed_dy_first_rows(const float* d_hidden, const float* dh0, const int32_t* rows, int B, int S, int H,
                                             bf16_t* dy, hipStream_t stream) {
  if (!dh0 || !dy || B < 1 || S < 1 || H < 4 || H % 4) return 1;
  if ((((uintptr_t)d_hidden | (uintptr_t)dh0) & 15) || ((uintptr_t)dy & 7)) return 1;
  if ((int64_t)B * H >= ((int64_t)1 << 31) / 4) return 1;
  ProfScope ps(PLB_K_CAST, stream, 0, (double)B * H * 10.0);
  hipLaunchKernelGGL(seed_dy_first_rows_kernel, dim3((unsigned)((B * (H / 4) + 255) / 256)), dim3(256), 0, stream, d_hidden, dh0, rows,
                     B, S, H / 4, dy);
  return LAUNCH_OK();
}
