// LAMB (Adam with a layer-wise trust ratio) over the flat buffers, gfx950: two streaming passes and a small finish kernel per
// range (include/plbert.h: plb_lamb_step holds the definition). HBM-bound: pass 1 moves 24 B/param (p, g, m, v read; m, v
// written), pass 2 18 B/param (p, m, v read; p and the bf16 copy written). Plain float4 loads and stores, no atomics on float
// data, fixed summation order: bitwise reproducible from run to run. No kernel of this unit uses scratch.
//
// WORKGROUPS ARE MAPPED TO TENSORS. A tensor is cut into pieces of 1024 floats (256 threads x float4) counted from ITS OWN first
// float, and a workgroup owns one piece: a piece never reaches into another tensor, so a workgroup has one set of scalars, one
// trust ratio and one pair of partial sums, however short the bias tensors between the matrices are (a tensor of 4 floats
// occupies a workgroup of which one lane works). The table — bounds, first workgroup, result slot and the pre-rounded scalars
// of every live tensor of the range — travels BY VALUE as a kernel argument (about 1.5 KiB of the kernarg segment: no device
// table, no copy, the three launches stay asynchronous and capturable); a workgroup finds its tensor with scalar loads and
// compares. What lies between the tensors of the table is a hole: nothing of it is loaded or stored.
//
// SUMS. Pass 1 leaves, per workgroup, (sum p^2, sum u^2) of its piece in partials[2 b], partials[2 b + 1]: every thread adds
// its 4 squares in index order (one fused multiply-add = one rounding each), wave_sum (6 additions), the four waves through
// LDS in the order ((w0 + w1) + w2) + w3 — the longest chain of fp32 additions behind one partial is 4 + 6 + 3 = 13
// (PLB_LAMB_CHAIN). The finish kernel, one workgroup per result slot, adds a tensor's partials in DOUBLE in a fixed order
// (thread t: partials t, t + 1024, ...; then a tree over the 1024 threads) and writes [wn, un, trust, 1] — or four zeros for a
// slot that is a hole. It is a launch of its own, not a prologue of pass 2: as a prologue every workgroup of a tensor would
// add all of that tensor's partials again, work that grows with the SQUARE of the tensor's size (the 64 000 x 768 token head
// has 48 000 partials and as many workgroups), where the launch costs a few microseconds once per range.
//
// ARITHMETIC. m and v are formed by adamw_clipped_body's expressions (optim.hip), operation for operation, so that after a
// LAMB step exp_avg and exp_avg_sq are bit-identical to those after plb_launch_adamw_clipped from the same state with the same
// betas, grad_scale and coefficient (tests/test_gpu_lamb_kernel.py holds one against the other). u is formed by ONE function
// that both passes call, with contraction off for the whole unit (every fused operation is written out): pass 2 recomputes
// from the stored m and v exactly the u whose squares pass 1 summed. The gradient buffer is only ever read.
//
// SKIPPING. The health word is tested first (skip && *skip), then norm[2]: when either is set no launch of the three stores
// anything — m and v are not advanced, the results of the last step stay in place — and pass 1 alone counts the left-out
// update (skip[count_skip], norm[3]).
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

#pragma clang fp contract(off)

namespace {
struct LambTable {
  int n;                                         // live tensors of the range
  unsigned int b4[PLB_NPARAM], e4[PLB_NPARAM];   // [b4, e4) in float4s (every boundary is a multiple of 4 floats)
  unsigned int wg0[PLB_NPARAM + 1];              // the first workgroup of tensor s; wg0[n] = the grid
  int slot[PLB_NPARAM], adapt[PLB_NPARAM];       // the tensor's place in the results (enum PlbParam); trust ratio on / off
  float sc[PLB_NPARAM][8];                       // 1 - beta1, beta2, 1 - beta2, eps, sqrt(bc2), 1 / bc1, weight_decay, lr
};

// The tensor that owns workgroup b (b < wg0[n]); b is uniform: scalar loads and compares
DEVI int tensor_of(const LambTable& t, unsigned int b) {
  int s = 0;
  while (s + 1 < t.n && t.wg0[s + 1] <= b) ++s;
  return s;
}

// adamw_clipped_body's moments (optim.hip) with the contractions hipcc makes in adamw_kernel written out
template <bool CLIP>
DEVI void lamb_moments(float g, float& m, float& v, float gscale, float coef, float omb1, float b2, float omb2) {
  float gj = g * gscale, d;
  if (CLIP) {   // (the empty asm keeps the rounded product a value of its own, as there)
    gj *= coef;
    asm("" : "+v"(gj));
    d = gj - m;
  } else {
    d = __builtin_fmaf(g, gscale, -m);
  }
  m = __builtin_fmaf(omb1, d, m);
  v = __builtin_fmaf(b2, v, omb2 * (gj * gj));
}
// u = r * (1 / bc1) + weight_decay * p, r = m / (sqrt(v) / sqrt(bc2) + eps): the one expression of both passes
DEVI float lamb_update(float p, float m, float v, float eps, float bc2_sqrt, float inv_bc1, float wd) {
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  return __builtin_fmaf(m / denom, inv_bc1, wd * p);
}

template <bool CLIP>
DEVI void lamb_pass1_body(const float* p, const float* g, float* m, float* v, size_t i, const float* sc, float gscale, float coef,
                          float& sp, float& su) {
  const float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i), M = *(const float4*)(m + i), V = *(const float4*)(v + i);
  const float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w};
  float mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lamb_moments<CLIP>(gg[j], mm[j], vv[j], gscale, coef, sc[0], sc[1], sc[2]);
    const float u = lamb_update(pp[j], mm[j], vv[j], sc[3], sc[4], sc[5], sc[6]);
    sp = __builtin_fmaf(pp[j], pp[j], sp);
    su = __builtin_fmaf(u, u, su);
  }
  *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
  *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

template <bool NORM>
__global__ __launch_bounds__(256) void lamb_pass1_kernel(const float* p, const float* g, float* m, float* v, LambTable t,
                                                         float gscale, unsigned int* skip, int count_skip, float* norm,
                                                         int count_nonfinite, float* partials) {
  __shared__ float red[8];
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
  const int s = tensor_of(t, blockIdx.x);
  const unsigned int q = t.b4[s] + (blockIdx.x - t.wg0[s]) * 256u + threadIdx.x;
  const float sc[7] = {t.sc[s][0], t.sc[s][1], t.sc[s][2], t.sc[s][3], t.sc[s][4], t.sc[s][5], t.sc[s][6]};
  float sp = 0.f, su = 0.f;
  if (q < t.e4[s]) {   // (the last piece of a tensor may be short)
    const size_t i = (size_t)q * 4;
    if (!NORM || coef == 1.0f) lamb_pass1_body<false>(p, g, m, v, i, sc, gscale, coef, sp, su);
    else lamb_pass1_body<true>(p, g, m, v, i, sc, gscale, coef, sp, su);
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sp; red[4 + (threadIdx.x >> 6)] = su; }
  __syncthreads();
  if (threadIdx.x == 0)
    *(float2*)(partials + 2 * (size_t)blockIdx.x) =
        make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// One workgroup of 1024 threads per result slot of [slot_lo, slot_lo + gridDim.x): the tensor's partials in double, then
// results[4 slot ..] = wn, un, trust, 1; a slot without a tensor in the table (a hole) gets four zeros. Thread t adds
// partials t + 1024 k into accumulator k mod 4 (four independent loads in flight: with one accumulator the 48 000 partials of a
// 64 000-token head were 188 dependent load-and-add rounds per thread, 82 us), then ((a0 + a1) + a2) + a3 and a tree over the
// threads: a fixed order.
__global__ __launch_bounds__(1024) void lamb_finish_kernel(LambTable t, int slot_lo, const float* partials, float* results,
                                                           const unsigned int* skip, const float* norm) {
  __shared__ double rp[1024], ru[1024];
  if (skip && *skip) return;
  if (norm && norm[2] != 0.f) return;
  const int slot = slot_lo + (int)blockIdx.x;
  int s = -1;
  for (int k = 0; k < t.n; ++k)
    if (t.slot[k] == slot) s = k;
  float* out = results + 4 * (size_t)slot;
  if (s < 0) {
    if (threadIdx.x == 0) *(float4*)out = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const unsigned int w1 = t.wg0[s + 1];
  double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned int w = t.wg0[s] + threadIdx.x;
  for (; w + 3 * 1024u < w1; w += 4 * 1024u) {
    float2 pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pr[j] = *(const float2*)(partials + 2 * (size_t)(w + j * 1024u));
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] += (double)pr[j].x; b[j] += (double)pr[j].y; }
  }
  for (int j = 0; w < w1; w += 1024u, ++j) {   // (at most three left)
    const float2 pr = *(const float2*)(partials + 2 * (size_t)w);
    a[j] += (double)pr.x;
    b[j] += (double)pr.y;
  }
  rp[threadIdx.x] = ((a[0] + a[1]) + a[2]) + a[3];
  ru[threadIdx.x] = ((b[0] + b[1]) + b[2]) + b[3];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { rp[threadIdx.x] += rp[threadIdx.x + o]; ru[threadIdx.x] += ru[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x) return;
  const float wn = (float)sqrt(rp[0]), un = (float)sqrt(ru[0]);
  const float trust = (t.adapt[s] && wn > 0.f && un > 0.f) ? wn / un : 1.0f;
  *(float4*)out = make_float4(wn, un, trust, 1.0f);
}

__global__ __launch_bounds__(256) void lamb_pass2_kernel(float* p, const float* m, const float* v, bf16_t* pb, LambTable t,
                                                         const float* results, const unsigned int* skip, const float* norm) {
  if (skip && *skip) return;
  if (norm && norm[2] != 0.f) return;
  const int s = tensor_of(t, blockIdx.x);
  const unsigned int q = t.b4[s] + (blockIdx.x - t.wg0[s]) * 256u + threadIdx.x;
  if (q >= t.e4[s]) return;
  const float eps = t.sc[s][3], bc2_sqrt = t.sc[s][4], inv_bc1 = t.sc[s][5], wd = t.sc[s][6];
  const float step = t.sc[s][7] * results[4 * (size_t)t.slot[s] + 2];   // lr * trust (uniform)
  const size_t i = (size_t)q * 4;
  const float4 P = *(const float4*)(p + i), M = *(const float4*)(m + i), V = *(const float4*)(v + i);
  float pp[4] = {P.x, P.y, P.z, P.w};
  const float mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) pp[j] = __builtin_fmaf(-step, lamb_update(pp[j], mm[j], vv[j], eps, bc2_sqrt, inv_bc1, wd), pp[j]);
  *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
  if (pb) { uint2 o; o.x = pack_bf2(pp[0], pp[1]); o.y = pack_bf2(pp[2], pp[3]); *(uint2*)(pb + i) = o; }
}

// The launchers' checks and the table: 1 to PLB_NPARAM tensors, sorted, disjoint, not empty, inside [0, n), every boundary a
// multiple of 4 floats, step >= 1, adapt 0 or 1, result slots inside [0, PLB_NPARAM) and increasing. Returns false on a refusal.
bool lamb_table(const PlbLambSegment* segs, int n_segs, size_t n, LambTable* t) {
  if (n_segs < 1 || n_segs > PLB_NPARAM || !segs || n % 4 || n / 4 > 0x7fffffffu) return false;
  *t = LambTable{};
  int64_t prev = 0;
  int prev_slot = -1;
  uint64_t wg = 0;
  for (int i = 0; i < n_segs; ++i) {
    const PlbLambSegment& sg = segs[i];
    if (sg.begin < prev || sg.end <= sg.begin || sg.end > (int64_t)n || sg.begin % 4 || sg.end % 4 || sg.step < 1) return false;
    if ((sg.adapt != 0 && sg.adapt != 1) || sg.tensor <= prev_slot || sg.tensor >= PLB_NPARAM) return false;
    prev = sg.end;
    prev_slot = sg.tensor;
    t->b4[i] = (unsigned int)(sg.begin / 4);
    t->e4[i] = (unsigned int)(sg.end / 4);
    t->wg0[i] = (unsigned int)wg;
    wg += (uint64_t)(t->e4[i] - t->b4[i] + 255u) / 256u;
    t->slot[i] = sg.tensor;
    t->adapt[i] = sg.adapt;
    const float sc[8] = {sg.omb1, sg.b2, sg.omb2, sg.eps, sg.bc2_sqrt, sg.inv_bc1, sg.weight_decay, sg.lr};
    for (int j = 0; j < 8; ++j) t->sc[i][j] = sc[j];
  }
  if (wg > 0x7fffffffu) return false;
  t->wg0[n_segs] = (unsigned int)wg;
  t->n = n_segs;
  return true;
}
size_t live_floats(const PlbLambSegment* segs, int n_segs) {
  size_t live = 0;
  for (int i = 0; i < n_segs; ++i) live += (size_t)(segs[i].end - segs[i].begin);
  return live;
}
}  // namespace

extern "C" int64_t plb_lamb_workgroups(const PlbLambSegment* segs, int n_segs, size_t n) {
  LambTable t;
  if (n_segs == 0) return 0;
  return lamb_table(segs, n_segs, n, &t) ? (int64_t)t.wg0[t.n] : -1;
}

extern "C" int plb_launch_lamb_pass1(const float* p, const float* g, float* m, float* v, size_t n, const PlbLambSegment* segs,
                                     int n_segs, double grad_scale, unsigned int* skip_if_nonzero, int count_skip, float* norm,
                                     int count_nonfinite, float* partials, hipStream_t stream) {
  LambTable t;
  if (n_segs == 0) return 0;
  if (!p || !g || !m || !v || !partials || !lamb_table(segs, n_segs, n, &t)) return 1;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15 || ((uintptr_t)partials & 7)) return 1;
  ProfScope ps(PLB_K_ADAMW, stream, 0, (double)live_floats(segs, n_segs) * 24.0);   // p, g, m, v read; m, v written
  const dim3 grid(t.wg0[t.n]);
  if (norm)
    hipLaunchKernelGGL(lamb_pass1_kernel<true>, grid, dim3(256), 0, stream, p, g, m, v, t, (float)grad_scale, skip_if_nonzero,
                       count_skip, norm, count_nonfinite, partials);
  else
    hipLaunchKernelGGL(lamb_pass1_kernel<false>, grid, dim3(256), 0, stream, p, g, m, v, t, (float)grad_scale, skip_if_nonzero,
                       count_skip, norm, count_nonfinite, partials);
  return LAUNCH_OK();
}

extern "C" int plb_launch_lamb_finish(const PlbLambSegment* segs, int n_segs, size_t n, int slot_lo, int slot_hi,
                                      const float* partials, float* results, const unsigned int* skip_if_nonzero,
                                      const float* norm, hipStream_t stream) {
  LambTable t;
  if (n_segs == 0) t = LambTable{};
  else if (!lamb_table(segs, n_segs, n, &t)) return 1;
  if (slot_lo < 0 || slot_hi > PLB_NPARAM || slot_lo >= slot_hi || !results || ((uintptr_t)results & 15)) return 1;
  if (n_segs && (!partials || ((uintptr_t)partials & 7) || segs[0].tensor < slot_lo || segs[n_segs - 1].tensor >= slot_hi)) return 1;
  ProfScope ps(PLB_K_REDUCE, stream, 0, (double)t.wg0[t.n] * 8.0);
  hipLaunchKernelGGL(lamb_finish_kernel, dim3(slot_hi - slot_lo), dim3(1024), 0, stream, t, slot_lo, partials, results,
                     skip_if_nonzero, norm);
  return LAUNCH_OK();
}

extern "C" int plb_launch_lamb_pass2(float* p, const float* m, const float* v, bf16_t* p_bf16, size_t n,
                                     const PlbLambSegment* segs, int n_segs, const float* results,
                                     const unsigned int* skip_if_nonzero, const float* norm, hipStream_t stream) {
  LambTable t;
  if (n_segs == 0) return 0;
  if (!p || !m || !v || !results || !lamb_table(segs, n_segs, n, &t)) return 1;
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15 || ((uintptr_t)p_bf16 & 7)) return 1;
  ProfScope ps(PLB_K_ADAMW, stream, 0, (double)live_floats(segs, n_segs) * 18.0);   // p, m, v read; p and the bf16 copy written
  hipLaunchKernelGGL(lamb_pass2_kernel, dim3(t.wg0[t.n]), dim3(256), 0, stream, p, m, v, p_bf16, t, results, skip_if_nonzero,
                     norm);
  return LAUNCH_OK();
}
