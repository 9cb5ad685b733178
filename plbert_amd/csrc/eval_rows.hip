// Evaluation rows of the PL-BERT step, gfx950: what a masked-LM user reads beside the loss — per masked row the arg-max,
// the rank of the label, the top-k classes with their log-probabilities and the row's negative log-likelihood; per sample
// the mean loss and the counts of correct rows; and the top-1 count of the fused token head from the statistics its first
// GEMM pass keeps. They read what a loss call left behind (engine_eval.cpp: plb_masked_report) and take no part in the
// step. Plain vector loads and stores, integer counts and fixed-order fp32 sums: no atomics, no "last block done" counters,
// bitwise reproducible from run to run.
#include <limits.h>

#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
DEVI int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One row per wave, V <= 256 classes, 4 per lane (ce_kernel's layout; V % 4 == 0: a lane's classes are all real or all
// padding). The order of classes is (logit descending, class index ascending). nll restates ce_kernel's expression
// operation for operation — mx + __logf(sum __expf(z - mx)) - z_t with the same reductions — so w * nll is ce_kernel's loss
// row bit for bit.
__global__ __launch_bounds__(256) void masked_report_rows_kernel(const float* logits, int ldl, int V, const int32_t* tgt, int n,
                                                                 int topk, int32_t* pred, int32_t* rank, float* nll,
                                                                 int32_t* topk_ids, float* topk_logprob, float* logits_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= n) return;
  const int c = lane * 4;
  float z[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) z[j] = (c + j < V) ? logits[(size_t)r * ldl + c + j] : -INFINITY;
  if (logits_out && c < V) {
#pragma unroll
    for (int j = 0; j < 4; ++j) logits_out[(size_t)r * V + c + j] = z[j];
  }
  const bool bad = __any((z[0] != z[0]) | (z[1] != z[1]) | (z[2] != z[2]) | (z[3] != z[3])) != 0;
  const float mx = wave_max(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
  float e[4], s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { e[j] = (c + j < V) ? __expf(z[j] - mx) : 0.f; s += e[j]; }
  s = wave_sum(s);
  const int t = tgt[r];
  float zt = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) zt += (c + j == t) ? z[j] : 0.f;
  zt = wave_sum(zt);
  const float lse = mx + __logf(s);
  const float qnan = __uint_as_float(0x7fc00000u);
  if (bad) {  // a row with a NaN logit has no order: never counted correct
    if (lane == 0) {
      if (pred) pred[r] = -1;
      if (rank) rank[r] = V;
      if (nll) nll[r] = qnan;
    }
    if (lane < topk) {
      if (topk_ids) topk_ids[(size_t)r * topk + lane] = -1;
      if (topk_logprob) topk_logprob[(size_t)r * topk + lane] = qnan;
    }
    return;
  }
  if (lane == 0 && nll) nll[r] = mx + __logf(s) - zt;
  if (rank) {  // classes in front of the label: larger logits, and equal logits at a lower index
    int before = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) before += (c + j < V) && (z[j] > zt || (z[j] == zt && c + j < t));
    before = wave_sum_i(before);
    if (lane == 0) rank[r] = before;
  }
  const bool want_list = topk > 0 && (topk_ids || topk_logprob);
  const int picks = want_list ? topk : (pred ? 1 : 0);
  unsigned taken = 0;      // bit j: class c + j is in the list already
  int my_id = -1;          // lane k keeps entry k of the list
  float my_lp = -INFINITY;
  for (int k = 0; k < picks; ++k) {
    float bv = -INFINITY;
    int bi = INT_MAX;      // INT_MAX: no class left (topk > V)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool open = (c + j < V) && !((taken >> j) & 1u);
      if (open && (bi == INT_MAX || z[j] > bv)) { bv = z[j]; bi = c + j; }   // (ascending j: the lowest index of equals stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      const bool take = oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi));
      if (take) { bv = ov; bi = oi; }
    }
    if (bi != INT_MAX && (bi >> 2) == lane) taken |= 1u << (bi & 3);
    if (lane == k) { my_id = bi == INT_MAX ? -1 : bi; my_lp = bi == INT_MAX ? -INFINITY : bv - lse; }
    if (k == 0 && lane == 0 && pred) pred[r] = bi == INT_MAX ? -1 : bi;
  }
  if (want_list && lane < topk) {
    if (topk_ids) topk_ids[(size_t)r * topk + lane] = my_id;
    if (topk_logprob) topk_logprob[(size_t)r * topk + lane] = my_lp;
  }
}
}  // namespace
extern "C" int plb_launch_masked_report_rows(const float* logits, int ldl, int V, const int32_t* tgt, int n, int topk,
                                             int32_t* pred, int32_t* rank, float* nll, int32_t* topk_ids, float* topk_logprob,
                                             float* logits_out, hipStream_t stream) {
  if (V < 4 || V > 256 || V % 4 || ldl < V || topk < 0 || topk > 8 || n < 0) return 1;
  if (n == 0) return 0;
  if (!logits || !tgt) return 1;
  ProfScope ps(PLB_K_CE, stream, 0, (double)n * (4.0 * V + (logits_out ? 4.0 * V : 0.0) + 12.0 + 8.0 * topk));
  hipLaunchKernelGGL(masked_report_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, logits, ldl, V, tgt, n, topk,
                     pred, rank, nll, topk_ids, topk_logprob, logits_out);
  return LAUNCH_OK();
}

namespace {
// One block per sample: the mean of its rows' nll — per-thread chain over the rows 256 apart, wave butterfly, the four
// waves in order (sum_rows_kernel's order), one division — and its counts of rank == 0 and rank < topk.
__global__ __launch_bounds__(256) void masked_report_samples_kernel(const int32_t* offsets, const int32_t* rank, const float* nll,
                                                                    int topk, float* sample_loss, int32_t* sample_top1,
                                                                    int32_t* sample_topk) {
  __shared__ float red[4];
  __shared__ int red1[4], redk[4];
  const int b = blockIdx.x;
  const int j0 = offsets[b], j1 = offsets[b + 1];
  float s = 0.f;
  int c1 = 0, ck = 0;
  for (int j = j0 + threadIdx.x; j < j1; j += 256) {
    if (nll) s += nll[j];
    if (rank) { const int rk = rank[j]; c1 += rk == 0; ck += rk < topk; }
  }
  s = wave_sum(s);
  c1 = wave_sum_i(c1);
  ck = wave_sum_i(ck);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red1[threadIdx.x >> 6] = c1; redk[threadIdx.x >> 6] = ck; }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sample_loss) sample_loss[b] = j1 > j0 ? (red[0] + red[1] + red[2] + red[3]) / (float)(j1 - j0) : 0.f;
    if (sample_top1) sample_top1[b] = red1[0] + red1[1] + red1[2] + red1[3];
    if (sample_topk) sample_topk[b] = redk[0] + redk[1] + redk[2] + redk[3];
  }
}
// One block: totals = {rows, rows with rank == 0, rows with rank < topk, samples that have rows} (integer sums).
__global__ __launch_bounds__(256) void masked_report_totals_kernel(const int32_t* offsets, int B, const int32_t* rank, int topk,
                                                                   int32_t* totals) {
  __shared__ int red[3][4];
  const int n = offsets[B];
  int c1 = 0, ck = 0, ne = 0;
  for (int j = threadIdx.x; j < n; j += 256) { const int rk = rank[j]; c1 += rk == 0; ck += rk < topk; }
  for (int b = threadIdx.x; b < B; b += 256) ne += offsets[b + 1] > offsets[b];
  c1 = wave_sum_i(c1);
  ck = wave_sum_i(ck);
  ne = wave_sum_i(ne);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = c1; red[1][threadIdx.x >> 6] = ck; red[2][threadIdx.x >> 6] = ne; }
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[0] = n;
    totals[1] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    totals[2] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    totals[3] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
  }
}
}  // namespace
extern "C" int plb_launch_masked_report_samples(const int32_t* offsets, int B, const int32_t* rank, const float* nll, int topk,
                                                float* sample_loss, int32_t* sample_top1, int32_t* sample_topk, int32_t* totals,
                                                hipStream_t stream) {
  if (!offsets || B < 1 || B > 1024 || topk < 0 || topk > 8) return 1;
  if ((sample_loss && !nll) || ((sample_top1 || sample_topk || totals) && !rank)) return 1;
  if (!sample_loss && !sample_top1 && !sample_topk && !totals) return 0;
  ProfScope ps(PLB_K_CE, stream, 0, 0.0);
  if (sample_loss || sample_top1 || sample_topk) {
    hipLaunchKernelGGL(masked_report_samples_kernel, dim3((unsigned)B), dim3(256), 0, stream, offsets, rank, nll, topk, sample_loss,
                       sample_top1, sample_topk);
    if (hipGetLastError() != hipSuccess) return 2;
  }
  if (totals) hipLaunchKernelGGL(masked_report_totals_kernel, dim3(1), dim3(256), 0, stream, offsets, B, rank, topk, totals);
  return LAUNCH_OK();
}

namespace {
// Token head, from the statistics of the fused GEMM + cross-entropy pass: one wave per row takes the maximum of the row's
// per-tile maxima; a valid row (w != 0) counts as correct when its target logit EQUALS that maximum. Per block the two
// counts of its four rows go to scratch[2 * block ..]; a second launch adds the blocks' counts.
__global__ __launch_bounds__(256) void token_top1_rows_kernel(const float* pmax, int ntiles, const float* tlogit, const float* w,
                                                              int rows, int32_t* scratch) {
  __shared__ int valid[4], hit[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  int v = 0, h = 0;
  if (t < rows && w[t] != 0.f) {   // (wave-uniform)
    float m = -INFINITY;
    for (int i = lane; i < ntiles; i += 64) m = fmaxf(m, pmax[(size_t)t * ntiles + i]);
    m = wave_max(m);
    v = 1;
    h = tlogit[t] == m;
  }
  if (lane == 0) { valid[wave] = v; hit[wave] = h; }
  __syncthreads();
  if (threadIdx.x == 0) {
    scratch[2 * blockIdx.x] = valid[0] + valid[1] + valid[2] + valid[3];
    scratch[2 * blockIdx.x + 1] = hit[0] + hit[1] + hit[2] + hit[3];
  }
}
__global__ __launch_bounds__(256) void token_top1_finish_kernel(const int32_t* scratch, int nblocks, int32_t* totals2) {
  __shared__ int red[2][4];
  int v = 0, h = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { v += scratch[2 * i]; h += scratch[2 * i + 1]; }
  v = wave_sum_i(v);
  h = wave_sum_i(h);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = v; red[1][threadIdx.x >> 6] = h; }
  __syncthreads();
  if (threadIdx.x == 0) {
    totals2[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    totals2[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}
}  // namespace
extern "C" int plb_launch_token_top1(const float* pmax, int ntiles, const float* tlogit, const float* w, int rows,
                                     int32_t* scratch, int32_t* totals2, hipStream_t stream) {
  if (!pmax || !tlogit || !w || !scratch || !totals2 || ntiles < 1 || rows < 1) return 1;
  const int nblocks = (rows + 3) / 4;
  ProfScope ps(PLB_K_TOKEN_CE, stream, 0, (double)rows * (4.0 * ntiles + 8.0));
  hipLaunchKernelGGL(token_top1_rows_kernel, dim3((unsigned)nblocks), dim3(256), 0, stream, pmax, ntiles, tlogit, w, rows, scratch);
  if (hipGetLastError() != hipSuccess) return 2;
  hipLaunchKernelGGL(token_top1_finish_kernel, dim3(1), dim3(256), 0, stream, scratch, nblocks, totals2);
  return LAUNCH_OK();
}
