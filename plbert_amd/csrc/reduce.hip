// Sums of the PL-BERT step, gfx950: column sums (bias / LayerNorm-affine gradients), slab reduction, and the scalar sums
// of the loss. HBM-bound. Every sum has a fixed order (partial sums per row split, then the splits in split order): no
// atomics, bitwise reproducible from run to run.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
// scratch[split][n] = sum of rows of the split; a block covers 256 columns x its row range:
// 32 lanes x 8 columns per row, 8 rows in flight per block (4 waves x 2 half-waves).
template <bool BF16>
__global__ __launch_bounds__(256) void colsum_kernel(const void* X, size_t R, int N, int ld, float* scratch, int nsplit) {
  __shared__ float red[8][256];
  const int tid = threadIdx.x;
  const int rsub = tid >> 5, cl = tid & 31;
  const int c = blockIdx.x * 256 + cl * 8;
  const size_t rows_per = (R + nsplit - 1) / nsplit;
  const size_t r0 = (size_t)blockIdx.y * rows_per;
  size_t r1 = r0 + rows_per; if (r1 > R) r1 = R;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < N) {
    size_t r = r0 + rsub;
    if (BF16) {  // 4 independent 16-B loads in flight per thread (the sums are latency-bound otherwise)
      const bf16_t* px = (const bf16_t*)X + c;
      for (; r + 24 < r1; r += 32) {
        uint4 u0 = *(const uint4*)(px + r * ld), u1 = *(const uint4*)(px + (r + 8) * ld);
        uint4 u2 = *(const uint4*)(px + (r + 16) * ld), u3 = *(const uint4*)(px + (r + 24) * ld);
        acc[0] += (bf_lo(u0.x) + bf_lo(u1.x)) + (bf_lo(u2.x) + bf_lo(u3.x));
        acc[1] += (bf_hi(u0.x) + bf_hi(u1.x)) + (bf_hi(u2.x) + bf_hi(u3.x));
        acc[2] += (bf_lo(u0.y) + bf_lo(u1.y)) + (bf_lo(u2.y) + bf_lo(u3.y));
        acc[3] += (bf_hi(u0.y) + bf_hi(u1.y)) + (bf_hi(u2.y) + bf_hi(u3.y));
        acc[4] += (bf_lo(u0.z) + bf_lo(u1.z)) + (bf_lo(u2.z) + bf_lo(u3.z));
        acc[5] += (bf_hi(u0.z) + bf_hi(u1.z)) + (bf_hi(u2.z) + bf_hi(u3.z));
        acc[6] += (bf_lo(u0.w) + bf_lo(u1.w)) + (bf_lo(u2.w) + bf_lo(u3.w));
        acc[7] += (bf_hi(u0.w) + bf_hi(u1.w)) + (bf_hi(u2.w) + bf_hi(u3.w));
      }
    }
    if (!BF16) {  // fp32 partial rows (attention / GEMM epilogue column sums): 8 independent 16-B loads in flight per thread
      const float* px = (const float*)X + c;
      for (; r + 24 < r1; r += 32) {
        const float* q0 = px + r * ld;
        const float* q1 = px + (r + 8) * ld;
        const float* q2 = px + (r + 16) * ld;
        const float* q3 = px + (r + 24) * ld;
        const float4 a0 = *(const float4*)q0, b0 = *(const float4*)(q0 + 4), a1 = *(const float4*)q1, b1 = *(const float4*)(q1 + 4);
        const float4 a2 = *(const float4*)q2, b2 = *(const float4*)(q2 + 4), a3 = *(const float4*)q3, b3 = *(const float4*)(q3 + 4);
        acc[0] += (a0.x + a1.x) + (a2.x + a3.x); acc[1] += (a0.y + a1.y) + (a2.y + a3.y);
        acc[2] += (a0.z + a1.z) + (a2.z + a3.z); acc[3] += (a0.w + a1.w) + (a2.w + a3.w);
        acc[4] += (b0.x + b1.x) + (b2.x + b3.x); acc[5] += (b0.y + b1.y) + (b2.y + b3.y);
        acc[6] += (b0.z + b1.z) + (b2.z + b3.z); acc[7] += (b0.w + b1.w) + (b2.w + b3.w);
      }
    }
    for (; r < r1; r += 8) {
      if (BF16) {
        uint4 u = *(const uint4*)((const bf16_t*)X + r * ld + c);
        acc[0] += bf_lo(u.x); acc[1] += bf_hi(u.x); acc[2] += bf_lo(u.y); acc[3] += bf_hi(u.y);
        acc[4] += bf_lo(u.z); acc[5] += bf_hi(u.z); acc[6] += bf_lo(u.w); acc[7] += bf_hi(u.w);
      } else {
        const float* px = (const float*)X + r * ld + c;
        float4 a = *(const float4*)px, b = *(const float4*)(px + 4);
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
        acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rsub][cl * 8 + j] = acc[j];
  __syncthreads();
  const int col = blockIdx.x * 256 + tid;
  if (col < N) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[k][tid];
    scratch[(size_t)blockIdx.y * N + col] = s;
  }
}

// 32 columns per block (one 128-byte line per split row), 8 thread groups over the splits with 4 independent partial sums
// each: a column's sum is two dependent memory round trips deep, not nsplit / 4 (these launches sit on the side stream
// beside the weight-gradient GEMMs: at 10-15 us each, nine of them were a quarter of its busy time). Fixed order per column.
__global__ __launch_bounds__(256) void reduce_cols_kernel(const float* scratch, int nsplit, int N, int Nout, float* out,
                                                          int accumulate, int col0) {
  __shared__ float red[8][32];
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + c;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (j < Nout) {
    const float* px = scratch + col0 + j;
    int k = g;
    for (; k + 24 < nsplit; k += 32) {
      s0 += px[(size_t)k * N]; s1 += px[(size_t)(k + 8) * N]; s2 += px[(size_t)(k + 16) * N]; s3 += px[(size_t)(k + 24) * N];
    }
    for (; k < nsplit; k += 8) s0 += px[(size_t)k * N];
  }
  red[g][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && j < Nout) {
    const float t = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + ((red[4][c] + red[5][c]) + (red[6][c] + red[7][c]));
    out[j] = accumulate ? out[j] + t : t;
  }
}
}  // namespace
extern "C" int plb_launch_colsum(const void* X, int is_bf16, size_t R, int N, int ld, float* out, int Nout,
                                 int accumulate, float* scratch, int nsplit, hipStream_t stream) {
  if (N % 8 || ld % 8 || nsplit <= 0 || Nout > N) return 1;
  ProfScope ps(PLB_K_COLSUM, stream, 0, (double)R * N * (is_bf16 ? 2 : 4));
  dim3 grid((N + 255) / 256, nsplit);
  if (is_bf16) hipLaunchKernelGGL((colsum_kernel<true>), grid, dim3(256), 0, stream, X, R, N, ld, scratch, nsplit);
  else hipLaunchKernelGGL((colsum_kernel<false>), grid, dim3(256), 0, stream, X, R, N, ld, scratch, nsplit);
  if (hipGetLastError() != hipSuccess) return 2;
  hipLaunchKernelGGL(reduce_cols_kernel, dim3((unsigned)((Nout + 31) / 32)), dim3(256), 0, stream, scratch, nsplit, N,
                     Nout, out, accumulate, 0);
  return LAUNCH_OK();
}
// Second half of a column sum whose first half (plb_launch_colsum) left [nsplit][N] partial rows in scratch:
// out[0..Nout) = sums of columns [col0, col0 + Nout). Lets one pass over a matrix feed two gradient tensors.
extern "C" int plb_launch_copy_cols(const float* scratch, int nsplit, int N, int col0, int Nout, float* out,
                                    hipStream_t stream) {
  if (nsplit <= 0 || col0 < 0 || col0 + Nout > N) return 1;
  hipLaunchKernelGGL(reduce_cols_kernel, dim3((unsigned)((Nout + 31) / 32)), dim3(256), 0, stream, scratch, nsplit, N,
                     Nout, out, 0, col0);
  return LAUNCH_OK();
}

namespace {
// out[i] (+)= sum over the splits, in split order (fixed: deterministic). Four slabs are loaded before the first add:
// the loop is a chain of dependent HBM reads otherwise (1.9 TB/s measured with one load in flight per thread).
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* slab, int splits, size_t n, float* out, int accumulate) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    float4 s = accumulate ? *(const float4*)(out + i) : make_float4(0, 0, 0, 0);
    int k = 0;
    for (; k + 4 <= splits; k += 4) {
      const float4 v0 = *(const float4*)(slab + (size_t)k * n + i), v1 = *(const float4*)(slab + (size_t)(k + 1) * n + i);
      const float4 v2 = *(const float4*)(slab + (size_t)(k + 2) * n + i), v3 = *(const float4*)(slab + (size_t)(k + 3) * n + i);
      s.x = (((s.x + v0.x) + v1.x) + v2.x) + v3.x; s.y = (((s.y + v0.y) + v1.y) + v2.y) + v3.y;
      s.z = (((s.z + v0.z) + v1.z) + v2.z) + v3.z; s.w = (((s.w + v0.w) + v1.w) + v2.w) + v3.w;
    }
    for (; k < splits; ++k) {
      float4 v = *(const float4*)(slab + (size_t)k * n + i);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *(float4*)(out + i) = s;
  } else {
    for (size_t j = i; j < n; ++j) {
      float s = accumulate ? out[j] : 0.f;
      for (int k = 0; k < splits; ++k) s += slab[(size_t)k * n + j];
      out[j] = s;
    }
  }
}
}  // namespace
extern "C" int plb_launch_reduce_slabs(const float* slab, int splits, size_t n, float* out, int accumulate,
                                       hipStream_t stream) {
  if (!n) return 0;
  const size_t threads = (n + 3) / 4;
  ProfScope ps(PLB_K_REDUCE, stream, 0, 4.0 * (double)n * (splits + 1));
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, slab, splits, n,
                     out, accumulate);
  return LAUNCH_OK();
}

namespace {
__global__ __launch_bounds__(256) void sum_rows_kernel(const float* x, int n, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}
}  // namespace
extern "C" int plb_launch_sum_rows(const float* x, int n, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, stream, x, n, out);
  return LAUNCH_OK();
}

namespace {
__global__ void add_scalar_kernel(float* out, const float* a, const float* b) { out[0] = a[0] + b[0]; }
}  // namespace
extern "C" int plb_launch_add_scalar(float* out, const float* a, const float* b, hipStream_t stream) {
  hipLaunchKernelGGL(add_scalar_kernel, dim3(1), dim3(1), 0, stream, out, a, b);
  return LAUNCH_OK();
}
