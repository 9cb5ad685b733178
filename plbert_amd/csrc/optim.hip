// Optimizer of the PL-BERT step, gfx950 (A12): AdamW, gradient accumulation, the global gradient norm with the clipped
// update (include/plbert.h: plb_grad_accum_add, plb_grad_norm, plb_adamw_step_clipped), their segmented forms for parameter
// groups and frozen tensors (plb_adamw_step_groups, plb_grad_norm_groups), and the step status word.
// HBM-bound (30 B/param). Plain float4 loads and stores, no atomics on gradient data, fixed summation order: bitwise
// reproducible from run to run. adamw_kernel and adamw_clipped_kernel stay two kernels: at coef == 1 their outputs are
// bit-identical, and tests/test_gpu_grad_accum.py holds one against the other.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
// torch.optim.AdamW semantics, operation for operation (torch/optim/adamw.py -> adam.py, the default foreach form):
//   p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// The scalars are formed on the host in DOUBLE and rounded once, as torch forms them in Python floats: 1.0f - 0.999f
// is 0.99998713e-3, not 1e-3f — a 1.3e-5 relative error in every second moment (tests/test_gpu_adamw_kernel.py).
// skip: the engine's hand-off error word (or null). Non-zero = a fused LayerNorm launch of this step timed out: its
// gradients are invalid and the whole update is left out (a uniform scalar load and branch; the host learns of it from
// plb_poll_status / plb_status without this launch having waited for anybody).
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, bf16_t* pb, size_t n,
                                                    float decay, float omb1, float b2, float omb2, float eps, float step,
                                                    float bc2_sqrt, float gscale, unsigned int* skip, int count_skip) {
  if (skip && *skip) {   // skip[count_skip] counts the optimizer steps left out (1: the trainable range — the host rewinds
    // its step count by it; 2: the token head, which keeps a step count of its own)
    if (count_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skip + count_skip, 1u);
    return;
  }
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;  // n is a multiple of 4 (checked by the launcher)
  float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i), M = *(const float4*)(m + i), V = *(const float4*)(v + i);
  float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gj = gg[j] * gscale;
    pp[j] *= decay;
    mm[j] = mm[j] + omb1 * (gj - mm[j]);
    vv[j] = b2 * vv[j] + omb2 * (gj * gj);
    const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
    pp[j] -= step * (mm[j] / denom);
  }
  *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
  *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
  *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
  if (pb) { uint2 o; o.x = pack_bf2(pp[0], pp[1]); o.y = pack_bf2(pp[2], pp[3]); *(uint2*)(pb + i) = o; }
}
}  // namespace
extern "C" int plb_launch_adamw(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n, double lr,
                                double beta1, double beta2, double eps, double wd, int step, double grad_scale,
                                unsigned int* skip_if_nonzero, int count_skip, hipStream_t stream) {
  if (n % 4 || step < 1) return 1;
  if (!n) return 0;
  ProfScope ps(PLB_K_ADAMW, stream, 0, (double)n * 30.0);  // p,m,v read+write, g read, bf16 copy
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, p, g, m, v, p_bf16, n,
                     (float)(1.0 - lr * wd), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                     (float)(lr / bc1), (float)sqrt(bc2), (float)grad_scale, skip_if_nonzero, count_skip);
  return LAUNCH_OK();
}

namespace {
// ---- gradient accumulation, global norm, clipped update (include/plbert.h: plb_grad_accum_add, plb_grad_norm,
// plb_adamw_step_clipped). Plain float4 loads and stores, no atomics on gradient data, fixed summation order: bitwise
// reproducible from run to run.
// One pass over a flat range on a FIXED grid of PLB_NORM_PARTS workgroups, whatever n is: workgroup b owns the contiguous
// chunk [b * chunk, (b + 1) * chunk) ∩ [0, n), chunk = plb_norm_chunk(n) floats (a multiple of 1024 = one pass of 256
// threads x float4). phase 0: accum = grads | 1: accum += grads | 2: grads = accum + grads | 3: grads = accum | 4: read
// grads only. With `partials` the workgroup also writes the sum of squares of the values it stored (phase 4: read):
// every thread sums its float4s in index order in fp32, one fused multiply-add (one rounding) per value; wave_sum; the four
// waves' sums through LDS in the order ((w0 + w1) + w2) + w3. Longest chain of fp32 additions behind one partial:
//   4 * chunk / 1024 (a thread's own values) + 6 (wave_sum) + 3 (LDS step) = PLB_NORM_CHAIN(n), plbert_kernels.h.
// A workgroup whose chunk is empty writes 0.
__global__ __launch_bounds__(256) void grad_accum_kernel(float* accum, float* grads, size_t n, size_t chunk, int phase,
                                                         float* partials) {
  __shared__ float red[4];
  const size_t begin = (size_t)blockIdx.x * chunk;
  const size_t end = begin + chunk < n ? begin + chunk : n;   // n and chunk are multiples of 4: no float4 straddles `end`
  float s = 0.f;
  for (size_t i = begin + (size_t)threadIdx.x * 4; i < end; i += 1024) {
    float4 r;
    if (phase == 0) {
      r = *(const float4*)(grads + i);
      *(float4*)(accum + i) = r;
    } else if (phase == 3) {
      r = *(const float4*)(accum + i);
      *(float4*)(grads + i) = r;
    } else if (phase == 4) {
      r = *(const float4*)(grads + i);
    } else {
      const float4 a = *(const float4*)(accum + i), g = *(const float4*)(grads + i);
      r = make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
      *(float4*)((phase == 1 ? accum : grads) + i) = r;
    }
    s = __builtin_fmaf(r.x, r.x, s); s = __builtin_fmaf(r.y, r.y, s);
    s = __builtin_fmaf(r.z, r.z, s); s = __builtin_fmaf(r.w, r.w, s);
  }
  if (!partials) return;   // (uniform)
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
}  // namespace
extern "C" int plb_launch_grad_accum(float* accum, float* grads, size_t n, int phase, float* partials, hipStream_t stream) {
  if (n % 4 || phase < 0 || phase > 3 || !accum || !grads) return 1;
  if (partials && phase < 2) return 1;   // the sum of squares belongs to the pass that leaves the final gradients
  if (((uintptr_t)accum | (uintptr_t)grads) & 15) return 1;
  if (!n && !partials) return 0;
  ProfScope ps(PLB_K_REDUCE, stream, 0, (double)n * (phase == 0 || phase == 3 ? 8.0 : 12.0));
  hipLaunchKernelGGL(grad_accum_kernel, dim3(PLB_NORM_PARTS), dim3(256), 0, stream, accum, grads, n, plb_norm_chunk(n), phase,
                     partials);
  return LAUNCH_OK();
}
extern "C" int plb_launch_grad_sumsq(const float* grads, size_t n, float* partials, hipStream_t stream) {
  if (n % 4 || !grads || !partials || ((uintptr_t)grads & 15)) return 1;
  ProfScope ps(PLB_K_REDUCE, stream, 0, (double)n * 4.0);
  hipLaunchKernelGGL(grad_accum_kernel, dim3(PLB_NORM_PARTS), dim3(256), 0, stream, (float*)nullptr,
                     const_cast<float*>(grads), n, plb_norm_chunk(n), 4, partials);
  return LAUNCH_OK();
}

namespace {
// One workgroup: the partials of all live ranges summed in double in a fixed order (thread t: entries t, t + 256, ...; then a
// tree over the 256 threads), then the constants of torch.nn.utils.clip_grad_norm_ in fp32 as torch forms them:
// out[0] = total_norm = grad_scale * sqrt(sum), out[1] = coef = min(1, max_norm / (total_norm + 1e-6)) (max_norm <= 0: 1),
// out[2] = 1 and coef = 0 when total_norm is not finite, else 0. out[3] (updates left out) is the clipped update's.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* partials, int nparts, double gscale, float max_norm,
                                                               float* out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x) return;
  const float total = (float)(gscale * sqrt(red[0]));
  const bool finite = fabsf(total) <= 3.4028234663852886e38f;   // false for inf and NaN
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(1.f, max_norm / (total + 1e-6f));
  out[0] = total;
  out[1] = finite ? coef : 0.f;
  out[2] = finite ? 0.f : 1.f;
}
}  // namespace
extern "C" int plb_launch_grad_norm_finish(const float* partials, int nparts, double grad_scale, double max_norm, float* out,
                                           hipStream_t stream) {
  if (!partials || !out || nparts < 1) return 1;
  ProfScope ps(PLB_K_REDUCE, stream, 0, (double)nparts * 4.0);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, stream, partials, nparts, grad_scale, (float)max_norm, out);
  return LAUNCH_OK();
}

namespace {
// adamw_kernel's arithmetic with the gradient (g * gscale) * coef, the two products rounded one after the other as torch
// forms g_mean and then clips it. norm: the four floats plb_launch_grad_norm_finish wrote (uniform scalar loads). coef == 1:
// the loop body is adamw_kernel's own expression, so every output is bit-identical to plb_launch_adamw's. norm[2] != 0 (the
// norm was not finite): nothing is written, and with count_nonfinite thread 0 adds 1 to norm[3]. skip is tested first.
template <bool CLIP>
DEVI void adamw_clipped_body(float* p, const float* g, float* m, float* v, bf16_t* pb, size_t i, float decay, float omb1,
                             float b2, float omb2, float eps, float step, float bc2_sqrt, float gscale, float coef) {
  float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i), M = *(const float4*)(m + i), V = *(const float4*)(v + i);
  float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // adamw_kernel's expressions with the contractions hipcc makes there written out (a second use of g * gscale in
    // this kernel would otherwise change which of them it makes): g * gscale - m is ONE fused operation in adamw_kernel,
    // the square takes the rounded product. tests/test_gpu_grad_accum.py holds the two kernels bit-equal at coef == 1.
    float gj = gg[j] * gscale, d;
    if (CLIP) {   // (the empty asm keeps the rounded product out of a fused multiply-add with the subtraction)
      gj *= coef;
      asm("" : "+v"(gj));
      d = gj - mm[j];
    } else {
      d = __builtin_fmaf(gg[j], gscale, -mm[j]);
    }
    mm[j] = __builtin_fmaf(omb1, d, mm[j]);
    vv[j] = __builtin_fmaf(b2, vv[j], omb2 * (gj * gj));
    const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
    pp[j] = __builtin_fmaf(decay, pp[j], -(step * (mm[j] / denom)));
  }
  *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
  *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
  *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
  if (pb) { uint2 o; o.x = pack_bf2(pp[0], pp[1]); o.y = pack_bf2(pp[2], pp[3]); *(uint2*)(pb + i) = o; }
}
__global__ __launch_bounds__(256) void adamw_clipped_kernel(float* p, const float* g, float* m, float* v, bf16_t* pb, size_t n,
                                                            float decay, float omb1, float b2, float omb2, float eps,
                                                            float step, float bc2_sqrt, float gscale, unsigned int* skip,
                                                            int count_skip, float* norm, int count_nonfinite) {
  if (skip && *skip) {
    if (count_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skip + count_skip, 1u);
    return;
  }
  if (norm[2] != 0.f) {
    if (count_nonfinite && blockIdx.x == 0 && threadIdx.x == 0) norm[3] += 1.f;
    return;
  }
  const float coef = norm[1];
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;  // n is a multiple of 4 (checked by the launcher)
  if (coef == 1.0f) adamw_clipped_body<false>(p, g, m, v, pb, i, decay, omb1, b2, omb2, eps, step, bc2_sqrt, gscale, coef);
  else adamw_clipped_body<true>(p, g, m, v, pb, i, decay, omb1, b2, omb2, eps, step, bc2_sqrt, gscale, coef);
}
}  // namespace
extern "C" int plb_launch_adamw_clipped(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n, double lr,
                                        double beta1, double beta2, double eps, double wd, int step, double grad_scale,
                                        unsigned int* skip_if_nonzero, int count_skip, float* norm, int count_nonfinite,
                                        hipStream_t stream) {
  if (n % 4 || step < 1 || !norm) return 1;
  if (!n) return 0;
  ProfScope ps(PLB_K_ADAMW, stream, 0, (double)n * 30.0);  // p,m,v read+write, g read, bf16 copy
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  hipLaunchKernelGGL(adamw_clipped_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, p, g, m, v, p_bf16, n,
                     (float)(1.0 - lr * wd), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                     (float)(lr / bc1), (float)sqrt(bc2), (float)grad_scale, skip_if_nonzero, count_skip, norm,
                     count_nonfinite);
  return LAUNCH_OK();
}

namespace {
// ---- segmented AdamW and the masked sum of squares (include/plbert.h: plb_adamw_step_groups, plb_grad_norm_groups).
// The live segments of one flat range, passed BY VALUE as a kernel argument (about 1 KiB of the kernarg segment: no device
// table, no copy, the launch stays asynchronous and capturable). Bounds count float4s: every boundary is a multiple of 4
// floats (checked by the launcher), so a float4 never straddles one. Segments are sorted and disjoint; whatever lies
// between them is a hole.
struct AdamWSegTable {
  int n;
  unsigned int b4[PLB_NPARAM], e4[PLB_NPARAM];   // [b4, e4) in float4s
  float sc[PLB_NPARAM][7];                       // decay, 1 - beta1, beta2, 1 - beta2, eps, lr / bc1, sqrt(bc2)
};
// The first segment that ends behind float4 q (t.n: none does); q wave-uniform: scalar loads and compares
DEVI int seg_behind(const AdamWSegTable& t, unsigned int q) {
  int s = 0;
  while (s < t.n && t.e4[s] <= q) ++s;
  return s;
}

// One pass over [0, n): adamw_clipped_body with the scalars of the segment each float4 lies in; a float4 in a hole is
// neither loaded nor stored. A 256-thread workgroup covers 1024 floats and bias tensors are 128 to 1024 floats long, so a
// workgroup can straddle several boundaries: the workgroup looks up the first segment that reaches into it (seg_behind:
// uniform, scalar loads and compares); if that segment covers all of it the scalars stay uniform, otherwise every lane selects
// its own among the segments that overlap the workgroup. skip / norm: adamw_clipped_kernel's tests in its order. NORM = false
// (the launcher's norm == null): coef = 1, no flag test, and only the unclipped body is compiled in. A single segment over
// [0, n) gives plb_launch_adamw's (with norm: plb_launch_adamw_clipped's) bits.
template <bool NORM>
__global__ __launch_bounds__(256) void adamw_segments_kernel(float* p, const float* g, float* m, float* v, bf16_t* pb,
                                                             AdamWSegTable t, float gscale, unsigned int* skip,
                                                             int count_skip, float* norm, int count_nonfinite) {
  if (skip && *skip) {
    if (count_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skip + count_skip, 1u);
    return;
  }
  float coef = 1.0f;
  if (NORM) {
    if (norm[2] != 0.f) {
      if (count_nonfinite && blockIdx.x == 0 && threadIdx.x == 0) norm[3] += 1.f;
      return;
    }
    coef = norm[1];
  }
  const unsigned int q0 = blockIdx.x * 256u, qend = q0 + 256u, q = q0 + threadIdx.x;   // (the grid ends at the last e4)
  const int s = seg_behind(t, q0);
  if (s == t.n || t.b4[s] >= qend) return;   // the whole workgroup lies in a hole
  float decay = t.sc[s][0], omb1 = t.sc[s][1], b2 = t.sc[s][2], omb2 = t.sc[s][3], eps = t.sc[s][4], step = t.sc[s][5],
        bc2_sqrt = t.sc[s][6];
  bool live = q >= t.b4[s] && q < t.e4[s];
  for (int k = s + 1; k < t.n && t.b4[k] < qend; ++k) {   // (no trip when segment s covers the workgroup)
    if (q >= t.b4[k] && q < t.e4[k]) {
      live = true;
      decay = t.sc[k][0]; omb1 = t.sc[k][1]; b2 = t.sc[k][2]; omb2 = t.sc[k][3]; eps = t.sc[k][4]; step = t.sc[k][5];
      bc2_sqrt = t.sc[k][6];
    }
  }
  if (!live) return;
  const size_t i = (size_t)q * 4;
  if (!NORM || coef == 1.0f) adamw_clipped_body<false>(p, g, m, v, pb, i, decay, omb1, b2, omb2, eps, step, bc2_sqrt, gscale, coef);
  else adamw_clipped_body<true>(p, g, m, v, pb, i, decay, omb1, b2, omb2, eps, step, bc2_sqrt, gscale, coef);
}

// grad_accum_kernel's phase 4 (same grid, same chunk, same order of additions) with the float4s of the holes replaced by
// zeros: a SELECT, not a product — a NaN or Inf in a frozen tensor's gradient never reaches the sum, and since
// fma(0, 0, s) == s the partials are the bits plb_launch_grad_sumsq gives on a copy whose holes were zero-filled.
__global__ __launch_bounds__(256) void grad_sumsq_segments_kernel(const float* grads, size_t n, size_t chunk, AdamWSegTable t,
                                                                  float* partials) {
  __shared__ float red[4];
  const size_t begin = (size_t)blockIdx.x * chunk;
  const size_t end = begin + chunk < n ? begin + chunk : n;
  float acc = 0.f;
  int s = begin < end ? seg_behind(t, (unsigned int)(begin / 4)) : t.n;
  if (s < t.n && t.b4[s] <= begin / 4 && t.e4[s] >= end / 4) {   // one segment covers the chunk: grad_accum_kernel's loop
    for (size_t i = begin + (size_t)threadIdx.x * 4; i < end; i += 1024) {
      const float4 r = *(const float4*)(grads + i);
      acc = __builtin_fmaf(r.x, r.x, acc); acc = __builtin_fmaf(r.y, r.y, acc);
      acc = __builtin_fmaf(r.z, r.z, acc); acc = __builtin_fmaf(r.w, r.w, acc);
    }
  } else if (s < t.n && t.b4[s] < end / 4) {   // (else the chunk is empty or lies in a hole: 0)
    for (size_t base = begin; base < end; base += 1024) {   // one pass of the workgroup: float4s [q0, qend)
      const size_t q0 = base / 4, qend = (base + 1024 < end ? base + 1024 : end) / 4, q = q0 + threadIdx.x;
      while (s < t.n && t.e4[s] <= q0) ++s;
      bool live = false;
      for (int k = s; k < t.n && t.b4[k] < qend; ++k) live = live || (q >= t.b4[k] && q < t.e4[k]);
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < qend) {
        if (live) r = *(const float4*)(grads + q * 4);
        acc = __builtin_fmaf(r.x, r.x, acc); acc = __builtin_fmaf(r.y, r.y, acc);
        acc = __builtin_fmaf(r.z, r.z, acc); acc = __builtin_fmaf(r.w, r.w, acc);
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// The launchers' checks and the table: at most PLB_NPARAM segments, sorted, disjoint, not empty, inside [0, n), every
// boundary a multiple of 4 floats, step >= 1. Returns false on a refusal.
bool seg_table(const PlbAdamWSegment* segs, int n_segs, size_t n, AdamWSegTable* t) {
  if (n_segs < 0 || n_segs > PLB_NPARAM || (n_segs && !segs) || n % 4 || n / 4 > 0x7fffffffu) return false;
  *t = AdamWSegTable{};
  int64_t prev = 0;
  for (int i = 0; i < n_segs; ++i) {
    const PlbAdamWSegment& sg = segs[i];
    if (sg.begin < prev || sg.end <= sg.begin || sg.end > (int64_t)n || sg.begin % 4 || sg.end % 4 || sg.step < 1) return false;
    prev = sg.end;
    t->b4[i] = (unsigned int)(sg.begin / 4);
    t->e4[i] = (unsigned int)(sg.end / 4);
    const float sc[7] = {sg.decay, sg.omb1, sg.b2, sg.omb2, sg.eps, sg.step_size, sg.bc2_sqrt};
    for (int j = 0; j < 7; ++j) t->sc[i][j] = sc[j];
  }
  t->n = n_segs;
  return true;
}
}  // namespace
extern "C" int plb_launch_adamw_segments(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n,
                                         const PlbAdamWSegment* segs, int n_segs, double grad_scale,
                                         unsigned int* skip_if_nonzero, int count_skip, float* norm, int count_nonfinite,
                                         hipStream_t stream) {
  AdamWSegTable t;
  if (!seg_table(segs, n_segs, n, &t)) return 1;
  if (!n_segs) return 0;
  size_t live = 0;
  for (int i = 0; i < n_segs; ++i) live += (size_t)(segs[i].end - segs[i].begin);
  ProfScope ps(PLB_K_ADAMW, stream, 0, (double)live * 30.0);  // p,m,v read+write, g read, bf16 copy: live segments only
  const dim3 grid((t.e4[n_segs - 1] + 255u) / 256u);
  if (norm)
    hipLaunchKernelGGL(adamw_segments_kernel<true>, grid, dim3(256), 0, stream, p, g, m, v, p_bf16, t, (float)grad_scale,
                       skip_if_nonzero, count_skip, norm, count_nonfinite);
  else
    hipLaunchKernelGGL(adamw_segments_kernel<false>, grid, dim3(256), 0, stream, p, g, m, v, p_bf16, t, (float)grad_scale,
                       skip_if_nonzero, count_skip, norm, count_nonfinite);
  return LAUNCH_OK();
}
extern "C" int plb_launch_grad_sumsq_segments(const float* grads, size_t n, const PlbAdamWSegment* segs, int n_segs,
                                              float* partials, hipStream_t stream) {
  AdamWSegTable t;
  if (!grads || !partials || ((uintptr_t)grads & 15) || !seg_table(segs, n_segs, n, &t)) return 1;
  size_t live = 0;
  for (int i = 0; i < n_segs; ++i) live += (size_t)(segs[i].end - segs[i].begin);
  ProfScope ps(PLB_K_REDUCE, stream, 0, (double)live * 4.0);
  hipLaunchKernelGGL(grad_sumsq_segments_kernel, dim3(PLB_NORM_PARTS), dim3(256), 0, stream, grads, n, plb_norm_chunk(n), t,
                     partials);
  return LAUNCH_OK();
}

namespace {
// one thread, after the last launch of a loss call that can raise the word: this rank's count as a float, for the sum
// over the ranks (plb_launch_status_export)
__global__ void status_export_kernel(const unsigned int* ln_err, float* out) {
  const unsigned int e = *ln_err;
  *out = (float)(e < (1u << 20) ? e : (1u << 20));
}
}  // namespace
extern "C" int plb_launch_status_export(const unsigned int* ln_err, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(status_export_kernel, dim3(1), dim3(1), 0, stream, ln_err, out);
  return LAUNCH_OK();
}

namespace {
// one thread, at the end of a loss call (plb_launch_step_status). summed: the ranks' counts after their all-reduce (or
// null): a word another rank raised becomes this rank's too — every replica skips the update, or none does
__global__ void step_status_kernel(unsigned int* ln_err, float* loss, unsigned int* host_mirror, const float* summed) {
  unsigned int e = *ln_err;
  if (summed) {
    const float f = *summed;
    if (f > 0.5f) {
      const unsigned int g = f < 1048576.f ? (unsigned int)(f + 0.5f) : (1u << 20);
      if (g > e) { e = g; *ln_err = e; }
    }
  }
  if (host_mirror) __hip_atomic_store(host_mirror, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (e && loss) *loss = __builtin_nanf("");
}
}  // namespace
extern "C" int plb_launch_step_status(unsigned int* ln_err, float* loss, unsigned int* host_mirror, const float* summed,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(step_status_kernel, dim3(1), dim3(1), 0, stream, ln_err, loss, host_mirror, summed);
  return LAUNCH_OK();
}
