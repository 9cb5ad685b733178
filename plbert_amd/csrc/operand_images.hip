// Operand images of the PL-BERT step, gfx950: the copies of a tensor that the GEMMs read — bf16 casts and transposes of
// the fp32 weights, and the fp8 plumbing (max |x| per site, delayed scaling, e4m3 / e5m2 quantisation). HBM-bound.
// An "amax" argument is one SITE: F8_SLOTS words on separate 64-byte lines (common.h: atomic_max_abs);
// plb_launch_fp8_scales takes the maximum over the slots and clears them.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
__global__ void cast_bf16_kernel(const float* src, bf16_t* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = f2bf(src[i]);
}
}  // namespace
extern "C" int plb_launch_cast_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t stream) {
  if (!n) return 0;
  ProfScope ps(PLB_K_CAST, stream, 0, 6.0 * (double)n);
  hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, dst, n);
  return LAUNCH_OK();
}

namespace {
__global__ void transpose_cast_kernel(const float* src, int R, int C, bf16_t* dst, int ldd) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < R) dst[(size_t)c * ldd + r] = f2bf(tile[tx][k]);
  }
}
}  // namespace
extern "C" int plb_launch_transpose_cast(const float* src, int R, int C, bf16_t* dst, int ldd, hipStream_t stream) {
  ProfScope ps(PLB_K_CAST, stream, 0, 6.0 * (double)R * C);
  hipLaunchKernelGGL(transpose_cast_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, stream, src, R, C, dst, ldd);
  return LAUNCH_OK();
}

namespace {
// Up to 8 transposes in ONE launch (the six weight copies the backward reads are 5 us of launch latency each after every
// optimizer step): block b belongs to the matrix whose tile range contains it.
struct TransposeMulti { const float* src[8]; bf16_t* dst[8]; int R[8], C[8], ldd[8], first[9]; int n; };
__global__ __launch_bounds__(256) void transpose_cast_multi_kernel(TransposeMulti q) {
  __shared__ float tile[32][33];
  int w = 0;
  while (w + 1 < q.n && (int)blockIdx.x >= q.first[w + 1]) ++w;
  const int R = q.R[w], C = q.C[w], ldd = q.ldd[w];
  const int tiles_c = (C + 31) / 32, b = blockIdx.x - q.first[w];
  const int c0 = (b % tiles_c) * 32, r0 = (b / tiles_c) * 32;
  const float* src = q.src[w];
  bf16_t* dst = q.dst[w];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < R) dst[(size_t)c * ldd + r] = f2bf(tile[tx][k]);
  }
}
}  // namespace
// dst[i][c][r] = bf16(src[i][r][c]) for n <= 8 matrices (R[i] x C[i], dst rows ldd[i] elements apart) in one launch
extern "C" int plb_launch_transpose_cast_multi(int n, const float* const* src, const int* R, const int* C, bf16_t* const* dst,
                                               const int* ldd, hipStream_t stream) {
  if (n < 1 || n > 8) return 1;
  TransposeMulti q = {};
  double bytes = 0;
  q.n = n;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i] || R[i] < 1 || C[i] < 1 || ldd[i] < R[i]) return 1;
    q.src[i] = src[i]; q.dst[i] = dst[i]; q.R[i] = R[i]; q.C[i] = C[i]; q.ldd[i] = ldd[i];
    q.first[i + 1] = q.first[i] + ((R[i] + 31) / 32) * ((C[i] + 31) / 32);
    bytes += 6.0 * (double)R[i] * C[i];
  }
  ProfScope ps(PLB_K_CAST, stream, 0, bytes);
  hipLaunchKernelGGL(transpose_cast_multi_kernel, dim3(q.first[n]), dim3(256), 0, stream, q);
  return LAUNCH_OK();
}

namespace {
// ------------------------------------------------------------------------------------ fp8 plumbing
// max |x| over a [rows][cols] matrix (ld elements per row) into one device scalar: per-thread 16-byte strides, wave
// shuffle, one atomic per wave. cols % 8 == 0 (bf16) / % 4 == 0 (fp32).
template <bool BF16>
__global__ __launch_bounds__(256) void amax_kernel(const void* X, size_t rows, int cols, int ld, float* out) {
  const int per = BF16 ? 8 : 4, cpr = cols / per;
  const size_t n = rows * (size_t)cpr;
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t r = i / cpr;
    const int c = (int)(i - r * cpr) * per;
    if (BF16) {
      const uint4 u = *(const uint4*)((const bf16_t*)X + r * ld + c);
      float f[8];
      unpack8(u, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(f[j]));
    } else {
      const float4 v = *(const float4*)((const float*)X + r * ld + c);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomic_max_abs(out, m, blockIdx.x * 4 + (threadIdx.x >> 6));
}
}  // namespace
extern "C" int plb_launch_amax(const void* x, int is_bf16, size_t rows, int cols, int ld, float* amax, hipStream_t stream) {
  if (!rows || cols <= 0 || cols % 8 || ld % 8) return 1;
  const size_t n = rows * (size_t)(cols / (is_bf16 ? 8 : 4));
  unsigned blocks = (unsigned)((n + 255) / 256); if (blocks > 2048) blocks = 2048;
  ProfScope ps(PLB_K_FP8, stream, 0, (double)rows * cols * (is_bf16 ? 2 : 4));
  if (is_bf16) hipLaunchKernelGGL((amax_kernel<true>), dim3(blocks), dim3(256), 0, stream, x, rows, cols, ld, amax);
  else hipLaunchKernelGGL((amax_kernel<false>), dim3(blocks), dim3(256), 0, stream, x, rows, cols, ld, amax);
  return LAUNCH_OK();
}

namespace {
// Delayed scaling: the scale a tensor is quantised with in the NEXT step is fmax / (the maximum seen in this one);
// a site that saw nothing (amax 0) keeps its scale. deq = 1 / scale is what the GEMM epilogues multiply by.
// One wave per site: maximum over the site's F8_SLOTS words, then the update, then the words are cleared.
// group > 1: sites come in runs of `group` entries (the L applications of the shared layer at one operand site) that share
// ONE scale, formed from the largest maximum of the run — the weight-gradient GEMM sums products of two images over all
// applications in one launch with one dequantisation factor, so every application's image must be on the same scale.
// stats (or null): 8 floats per group — [0..3] the last four non-zero maxima of the group, [4] how many calls quantised
// values beyond the format's range by more than the top value's rounding step (this call's true maximum x the scale it was
// quantised with > 1.0625 fmt: those elements were clamped and it shows), [5] the worst such ratio, [6] maxima recorded so far (selects the history slot). Groups from hist_from on
// (the engine: every site) take their scale from the LARGEST maximum of the history instead of the last one: a step whose
// values are larger than the previous step's (a short final batch, the step after a validation pass, a loss spike, or just
// another batch) is then clamped only if it exceeds everything seen in four calls, and the clamp is counted either way.
__global__ __launch_bounds__(64) void fp8_scales_kernel(float* amax, float* scale, float* deq, int n, float fmax, int group,
                                                        int n2, float fmax2, float* stats, int hist_from, float fmt, float fmt2) {
  const int g0 = blockIdx.x * group, lane = threadIdx.x;
  if (g0 >= n) return;
  if (g0 >= n2) { fmax = fmax2; fmt = fmt2; }   // entries [n2, n): the second format's target (one launch for both halves of the site table)
  float a = 0.f;
  for (int i = g0; i < g0 + group && i < n; ++i) {
    float* w = amax + (size_t)i * F8_SLOTS * F8_STRIDE + lane * F8_STRIDE;
    a = fmaxf(a, w[0]);
    w[0] = 0.f;
  }
  a = wave_max(a);
  if (a > 0.f && a < INFINITY) {
    float target = a;
    if (stats) {
      float* st = stats + (size_t)blockIdx.x * 8;
      if (lane == 0) {
        const float used = scale[g0];               // the scale this call's values were quantised with (0 before the first)
        const float ratio = a * used / fmt;
        if (ratio > 1.0625f) { st[4] += 1.f; st[5] = fmaxf(st[5], ratio); }   // beyond the top value by more than its rounding step
        float h[4] = {st[0], st[1], st[2], st[3]};
        unsigned int* const calls = reinterpret_cast<unsigned int*>(st + 6);   // an integer count (a float would stop at 2^24 calls)
        const int slot = (int)(*calls & 3u);
        h[slot] = a;
        st[slot] = a;
        *calls += 1u;
        if ((int)blockIdx.x >= hist_from) target = fmaxf(fmaxf(h[0], h[1]), fmaxf(h[2], h[3]));
      }
      target = __shfl(target, 0);
    }
    for (int i = g0 + lane; i < g0 + group && i < n; i += 64) {
      scale[i] = fmax / target;
      deq[i] = target / fmax;
    }
  }
}
}  // namespace
extern "C" int plb_launch_fp8_scales2(float* amax, float* scale, float* deq, int n, float fmax, int group, int n2, float fmax2,
                                      float* stats, int hist_from, hipStream_t stream) {
  if (n <= 0) return 0;
  if (group < 1) group = 1;
  hipLaunchKernelGGL(fp8_scales_kernel, dim3((n + group - 1) / group), dim3(64), 0, stream, amax, scale, deq, n, fmax, group, n2, fmax2,
                     stats, hist_from, 448.f, 57344.f);
  return LAUNCH_OK();
}
extern "C" int plb_launch_fp8_scales(float* amax, float* scale, float* deq, int n, float fmax, int group, hipStream_t stream) {
  return plb_launch_fp8_scales2(amax, scale, deq, n, fmax, group, n, fmax, nullptr, 0, stream);
}

namespace {
// out[r][c] = fp8(x[r][c] * scale): 8 elements per thread
template <bool BF16>
__global__ __launch_bounds__(256) void quantize_kernel(const void* X, size_t rows, int cols, int ld, const float* scale,
                                                       uint8_t* out, int ldo, int bf8) {
  const int cpr = cols / 8;
  const size_t n = rows * (size_t)cpr;
  const float s = scale[0];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 8;
    float f[8];
    if (BF16) {
      unpack8(*(const uint4*)((const bf16_t*)X + r * ld + c), f);
    } else {
      const float4 a = *(const float4*)((const float*)X + r * ld + c), b = *(const float4*)((const float*)X + r * ld + c + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
    uint2 w;
    w.x = pack_fp8x4(f[0] * s, f[1] * s, f[2] * s, f[3] * s, bf8 != 0);
    w.y = pack_fp8x4(f[4] * s, f[5] * s, f[6] * s, f[7] * s, bf8 != 0);
    *(uint2*)(out + r * ldo + c) = w;
  }
}
}  // namespace
extern "C" int plb_launch_quantize(const void* x, int is_bf16, size_t rows, int cols, int ld, const float* scale,
                                   uint8_t* out, int ldo, int bf8, hipStream_t stream) {
  if (!rows || cols <= 0 || cols % 8 || ld % 8 || ldo % 8) return 1;
  const size_t n = rows * (size_t)(cols / 8);
  unsigned blocks = (unsigned)((n + 255) / 256); if (blocks > 2048) blocks = 2048;
  ProfScope ps(PLB_K_FP8, stream, 0, (double)rows * cols * (is_bf16 ? 3 : 5));
  if (is_bf16) hipLaunchKernelGGL((quantize_kernel<true>), dim3(blocks), dim3(256), 0, stream, x, rows, cols, ld, scale, out, ldo, bf8);
  else hipLaunchKernelGGL((quantize_kernel<false>), dim3(blocks), dim3(256), 0, stream, x, rows, cols, ld, scale, out, ldo, bf8);
  return LAUNCH_OK();
}

namespace {
// The fp8 weight copies of a training step in ONE launch (blockIdx.y = weight): quantise with the scale the previous
// quantisation's maximum gave (delayed scaling: a weight moves by <= lr per step, the clamp covers the rest) and record this
// step's maximum for the next. Contiguous matrices (ld == cols).
struct QuantMulti { const void* src[8]; uint8_t* dst[8]; const float* scale[8]; float* amax[8]; size_t n8[8]; int bf16[8]; };
__global__ __launch_bounds__(256) void quantize_multi_kernel(QuantMulti q) {
  const int w = blockIdx.y;
  const float s = q.scale[w][0];
  const size_t n = q.n8[w];
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float f[8];
    if (q.bf16[w] & 1) {   // bit 0: bf16 source (else fp32); bit 1: e5m2 image (else e4m3)
      unpack8(*(const uint4*)((const bf16_t*)q.src[w] + i * 8), f);
    } else {
      const float4 a = *(const float4*)((const float*)q.src[w] + i * 8), b = *(const float4*)((const float*)q.src[w] + i * 8 + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
    const bool b8 = (q.bf16[w] & 2) != 0;
    uint2 o;
    o.x = pack_fp8x4(f[0] * s, f[1] * s, f[2] * s, f[3] * s, b8);
    o.y = pack_fp8x4(f[4] * s, f[5] * s, f[6] * s, f[7] * s, b8);
    *(uint2*)(q.dst[w] + i * 8) = o;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(f[j]));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomic_max_abs(q.amax[w], m, blockIdx.x * 4 + (threadIdx.x >> 6));
}
}  // namespace
// n <= 8 contiguous matrices (elements[i] % 8 == 0): dst[i] = e4m3(src[i] * scale[i][0]), amax[i] <- max |src[i]|;
// is_bf16[i]: bit 0 = the source is bf16 (else fp32), bit 1 = the image is e5m2 (gradients) instead of e4m3
extern "C" int plb_launch_quantize_multi(int n, const void* const* src, const int* is_bf16, const size_t* elements,
                                         const float* const* scale, uint8_t* const* dst, float* const* amax, hipStream_t stream) {
  if (n < 1 || n > 8) return 1;
  QuantMulti q = {};
  size_t bytes = 0;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i] || !scale[i] || !amax[i] || elements[i] % 8) return 1;
    q.src[i] = src[i]; q.dst[i] = dst[i]; q.scale[i] = scale[i]; q.amax[i] = amax[i]; q.n8[i] = elements[i] / 8; q.bf16[i] = is_bf16[i];
    bytes += elements[i] * ((is_bf16[i] & 1) ? 3 : 5);
  }
  ProfScope ps(PLB_K_FP8, stream, 0, (double)bytes);
  hipLaunchKernelGGL(quantize_multi_kernel, dim3(n == 1 ? 1024 : 128, n), dim3(256), 0, stream, q);   // one matrix: the whole chip
  return LAUNCH_OK();
}
