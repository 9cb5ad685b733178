// Token-head predictions without logits, gfx950: for n hidden rows, the best (up to 8) classes of z = X[rows[r]] · W^T + bias
// over a vocabulary of NT classes with their log-probabilities, the row's log-sum-exp and, with targets, the target's
// log-probability and its position in the list. No logit is stored (unless the caller asks for the fp32 copy).
//
//  token_topk_strips_kernel  a workgroup owns one 128-row tile and a STRIP of consecutive 128-column tiles. Per column tile
//     it runs the K loop of gemm_nt_kernel (gemm.hip: 128x128 tile, LDS-DMA double buffer, mfma_f32_16x16x32_bf16 with
//     swapped operands, so a lane owns 4 consecutive columns of one row per MFMA tile; the A rows are gathered through the
//     row list by the DMA's per-lane source address) and folds the tile into what it keeps in registers across the strip:
//     per lane and row a sorted list of 8 candidates (value, class) and an online (max, sum of exponentials) pair, the target
//     logit. A NaN logit (or +inf) shows as a NaN sum: the row's flag. Once per strip the 8 lanes that share a row meet in LDS, one thread per row merges them and
//     writes one list + (max, sum, target logit, NaN flag) per (row, strip) to scratch.
//  token_topk_merge_kernel   one wave per row merges the strips, forms lse and the log-probabilities, writes the outputs
//     and, per workgroup of 4 rows, the three counts.
//  token_topk_totals_kernel  adds the workgroups' counts (one workgroup).
//
// Order of classes: (logit descending, class index ascending) — compared as (value, index) PAIRS at every level (lane,
// row of a strip, strips), so the list does not depend on the strip count. Columns >= NT are excluded by a select on the
// column index (the weight rows behind NT belong to somebody else and may decode to NaN / Inf). No atomics, no "last block
// done" counters, fixed merge order: bitwise reproducible. Plain vector stores only.
//
// Budget of the strip kernel (256 threads, one workgroup per CU, i.e. one wave per SIMD and 512 registers per lane): 64
// accumulator registers (AGPRs) + 64 of candidate lists (4 rows x 8 x (value, index)) + 12 of row statistics + 32 of MFMA
// fragments + bias, addressing and temporaries: hipcc 7.x allocates 236 VGPRs + 64 AGPRs, no spill of either register kind,
// no scratch (-Rpass-analysis=kernel-resource-usage; tests/test_cabi_and_host.py holds every kernel to it). The per-value
// work keeps no mask in scalar registers across values: the NaN flag comes from the sum, the target from a rare branch
// (with both as per-value compares the kernel spilled 230 scalar registers). LDS 64 KiB: the K loop's two stages of A and
// B; after a strip's last K loop the same bytes hold the lists [8 lanes][8 entries][128 rows] x (float, int) — exactly
// 64 KiB — and, once the lists are merged, the statistics [8 lanes][128 rows] x float4 (16 KiB).
#include <limits.h>

#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NC = PLB_TOPK_MAX;

// a before b in the report's order
DEVI bool cand_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// Insert (v, i) into a sorted list of NC: a bubble pass with compile-time indices (the lists live in registers).
DEVI void cand_insert(float (&lv)[NC], int (&li)[NC], float v, int i) {
#pragma unroll
  for (int e = 0; e < NC; ++e) {
    const bool b = cand_before(v, i, lv[e], li[e]);
    const float tv = b ? lv[e] : v;
    const int ti = b ? li[e] : i;
    lv[e] = b ? v : lv[e];
    li[e] = b ? i : li[e];
    v = tv; i = ti;
  }
}
DEVI int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct TopkStrips {
  const bf16_t* X; int ldx; const int32_t* rows; int n;
  const bf16_t* W; int ldw; const float* bias; int NT, K;
  int strips, tiles_per_strip, ntiles;
  const int32_t* tgt;
  float* cv; int32_t* ci; float4* st;   // [n][strips][NC], [n][strips]
  float* logits;
};

// One 128x128 tile of logits into what a lane keeps per row. edge (workgroup-uniform): the tile holds columns >= NT. A
// select on the column index turns their accumulators into -inf before anything is computed from them (never arithmetic:
// their weight rows may decode to NaN / Inf), so they add exp(-inf) = 0 to the sum, never raise the maximum, and as candidates (-inf, c >= NT) come behind every real class: the merge kernel drops what it finds with an index
// >= NT. The interior tiles carry no per-column test.
DEVI void fold_tile(const TopkStrips& p, bool edge, f32x4 (&acc)[4][4], int c0, int r0, float (&lv)[4][NC], int (&li)[4][NC],
                    float (&rmax)[4], float (&rsum)[4], float (&rtl)[4], const int (&rtgt)[4],
                    const int (&rlive)[4]) {
  float bz[4][4];
  if (edge) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + ni * 16 + j;
        bz[ni][j] = c < p.NT ? p.bias[c] : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[mi][ni][j] = c < p.NT ? acc[mi][ni][j] : -INFINITY;
      }
  } else {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) bz[ni][j] = p.bias[c0 + ni * 16 + j];
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    float tmax = -INFINITY;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = acc[mi][ni][j] + bz[ni][j];
        acc[mi][ni][j] = v;
        tmax = fmaxf(tmax, v);   // (ignores a NaN: the sum below does not)
      }
    // the target's logit, when its column is one of this lane's 16 (offsets 16 ni + j from c0): a rare branch
    const int dt = rtgt[mi] - c0;
    if ((unsigned)dt < 64u && (dt & 12) == 0) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j) rtl[mi] = dt == ni * 16 + j ? acc[mi][ni][j] : rtl[mi];
    }
    const int r = r0 + mi * 16;
    if (p.logits && r < p.n) {
      float* dst = p.logits + (size_t)r * p.NT;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = c0 + ni * 16 + j;
          if (!edge || c < p.NT) dst[c] = rlive[mi] ? acc[mi][ni][j] : 0.f;
        }
    }
    // online (max, sum): one rescale of the running sum per tile, then the tile's 16 terms in column order
    const float mnew = fmaxf(rmax[mi], tmax);
    const float mref = mnew == -INFINITY ? 0.f : mnew;
    float s = rsum[mi] * __expf(rmax[mi] - mref);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) s += __expf(acc[mi][ni][j] - mref);
    rsum[mi] = s; rmax[mi] = mnew;
    // candidates: only what beats the list's last entry enters (most values do not, after the first tiles)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + ni * 16 + j;
        if (cand_before(acc[mi][ni][j], c, lv[mi][NC - 1], li[mi][NC - 1])) cand_insert(lv[mi], li[mi], acc[mi][ni][j], c);
      }
  }
}

__global__ __launch_bounds__(256) void token_topk_strips_kernel(TopkStrips p) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[2][2][BM * BK];  // [stage][A|B] 64 KiB; lists / statistics at the end
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int strip = blockIdx.x % p.strips, bm = blockIdx.x / p.strips;
  const int t0 = strip * p.tiles_per_strip;
  const int t1 = min(t0 + p.tiles_per_strip, p.ntiles);

  // Staging as in gemm_nt_kernel; the A source rows come from the row list. A position without a row (index < 0, or
  // behind n) reads row 0 of X: its results are never used.
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  const int drow = lane >> 3, dch = lane & 7;
  const bf16_t* gA[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = bm * BM + uw * 32 + i * 8 + drow;
    int src = r < p.n ? (p.rows ? p.rows[r] : r) : 0;
    if (src < 0) src = 0;
    gA[i] = p.X + (size_t)src * p.ldx;
  }
  const size_t sb = (size_t)8 * p.ldw;
  int sch[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sch[i] = (dch ^ ((4 * i + (lane >> 4)) & 7)) * 8;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
#define TK_STAGE(st, kt)                                                                              \
  do {                                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
      __builtin_amdgcn_global_load_lds((gptr_t)(gA[i] + (size_t)(kt) * BK + sch[i]),                  \
                                       (lptr_t)&smem[st][0][(uw * 32 + i * 8) * BK], 16, 0, 0);       \
      __builtin_amdgcn_global_load_lds((gptr_t)(gB + i * sb + (size_t)(kt) * BK + sch[i]),            \
                                       (lptr_t)&smem[st][1][(uw * 32 + i * 8) * BK], 16, 0, 0);       \
    }                                                                                                 \
  } while (0)
#define TK_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

  const int frow = lane & 15, fq = lane >> 4;
  const int fsw = (frow >> 1) & 7;
  const int offA = (wr * 64 + frow) * BK, offB = (wc * 64 + frow) * BK;
#define TK_COMPUTE(st)                                                                                   \
  do {                                                                                                   \
    const bf16_t* sA = smem[st][0];                                                                      \
    const bf16_t* sB = smem[st][1];                                                                      \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                                   \
      const int ch = ((kk * 4 + fq) ^ fsw) << 3;                                                         \
      bf16x8 af[4], bfr[4];                                                                              \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
        af[i] = *(const bf16x8*)&sA[offA + i * 16 * BK + ch];                                            \
        bfr[i] = *(const bf16x8*)&sB[offB + i * 16 * BK + ch];                                           \
      }                                                                                                  \
      _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                   \
        _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                                 \
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);  \
    }                                                                                                    \
  } while (0)

  // what the lane keeps across the strip, per row mi it owns (row bm*128 + wr*64 + mi*16 + frow)
  float lv[4][NC];
  int li[4][NC];
  float rmax[4], rsum[4], rtl[4];
  int rtgt[4];
  int rlive[4];    // the position has a row: its logits are stored as computed (else zeros)
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int e = 0; e < NC; ++e) { lv[mi][e] = -INFINITY; li[mi][e] = INT_MAX; }
    rmax[mi] = -INFINITY; rsum[mi] = 0.f; rtl[mi] = 0.f;
    const int r = bm * BM + wr * 64 + mi * 16 + frow;
    rtgt[mi] = (p.tgt && r < p.n) ? p.tgt[r] : -1;
    rlive[mi] = (r < p.n && (!p.rows || p.rows[r] >= 0)) ? 1 : 0;
  }

  const int nk = p.K / BK;
  for (int t = t0; t < t1; ++t) {
    const bf16_t* gB = p.W + (size_t)(t * BN + uw * 32 + drow) * p.ldw;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    TK_STAGE(0, 0);   // (every wave is behind the barrier that ended the previous tile's last reads)
    TK_LANDED();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) TK_STAGE(cur ^ 1, kt + 1);
      TK_COMPUTE(cur);
      TK_LANDED();
      __syncthreads();
    }
    // fold the tile: lane holds z[m][c0 .. c0+3] per (mi, ni). Only the vocabulary's last tile has columns to exclude.
    const int c0 = t * BN + wc * 64 + fq * 4;
    const int r0 = bm * BM + wr * 64 + frow;
    fold_tile(p, t * BN + BN > p.NT, acc, c0, r0, lv, li, rmax, rsum, rtl, rtgt, rlive);
  }
#undef TK_STAGE
#undef TK_LANDED
#undef TK_COMPUTE

  // lanes -> rows through LDS (the staging buffers are free: the last K loop ended on a barrier; an empty strip never
  // staged). slot = wc*4 + fq: the 8 lanes that share row m.
  __syncthreads();
  float* sv = (float*)&smem[0][0][0];           // [8 slots][NC][128 rows]
  int* si = (int*)&smem[1][0][0];               // the second 32 KiB
  const int slot = wc * 4 + fq;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = wr * 64 + mi * 16 + frow;
#pragma unroll
    for (int e = 0; e < NC; ++e) { sv[(slot * NC + e) * BM + m] = lv[mi][e]; si[(slot * NC + e) * BM + m] = li[mi][e]; }
  }
  __syncthreads();
  float mv[NC];
  int mx[NC];
  if (tid < BM) {   // one thread per row: slot 0's list, then the others' entries until one of a slot fails to enter
#pragma unroll
    for (int e = 0; e < NC; ++e) { mv[e] = sv[e * BM + tid]; mx[e] = si[e * BM + tid]; }
    for (int sl = 1; sl < 8; ++sl)
      for (int e = 0; e < NC; ++e) {
        const float v = sv[(sl * NC + e) * BM + tid];
        const int i = si[(sl * NC + e) * BM + tid];
        if (!cand_before(v, i, mv[NC - 1], mx[NC - 1])) break;
        cand_insert(mv, mx, v, i);
      }
  }
  __syncthreads();
  float4* ss = (float4*)&smem[0][0][0];         // [8 slots][128 rows]
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    ss[slot * BM + wr * 64 + mi * 16 + frow] = make_float4(rmax[mi], rsum[mi], rtl[mi], rsum[mi] != rsum[mi] ? 1.f : 0.f);
  __syncthreads();
  if (tid < BM) {
    const int r = bm * BM + tid;
    if (r < p.n) {
      float4 a = ss[tid];
      for (int sl = 1; sl < 8; ++sl) {   // fixed order: slot 1 .. 7 into slot 0
        const float4 b = ss[sl * BM + tid];
        const float mnew = fmaxf(a.x, b.x);
        const float mref = mnew == -INFINITY ? 0.f : mnew;
        a.y = a.y * __expf(a.x - mref) + b.y * __expf(b.x - mref);
        a.x = mnew;
        a.z += b.z;
        a.w = fmaxf(a.w, b.w);
      }
      const size_t o = (size_t)r * p.strips + strip;
      p.st[o] = a;
#pragma unroll
      for (int e = 0; e < NC; ++e) { p.cv[o * NC + e] = mv[e]; p.ci[o * NC + e] = mx[e]; }
    }
  }
}

// One wave per row, four rows per workgroup. Lane l holds the statistics of strip l and the candidates l and l + 64 of the
// strips' lists (<= 16 x 8 = 128); the list is drawn by topk arg-max rounds over the wave, compared as (value, index).
__global__ __launch_bounds__(256) void token_topk_merge_kernel(const float* cv, const int32_t* ci, const float4* st, int strips,
                                                               const int32_t* rows, const int32_t* tgt, int n, int NT, int topk,
                                                               int32_t* topk_ids, float* topk_logprob, float* lse_out,
                                                               float* target_logprob, int32_t* target_pos, int32_t* counts) {
  __shared__ int cnt[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  int counted = 0, hit0 = 0, hitk = 0;
  if (r < n) {   // (wave-uniform)
    const float qnan = __uint_as_float(0x7fc00000u);
    const bool norow = rows && rows[r] < 0;
    float4 s4 = make_float4(-INFINITY, 0.f, 0.f, 0.f);
    if (lane < strips) s4 = st[(size_t)r * strips + lane];
    const float M = wave_max(s4.x);
    const float mref = M == -INFINITY ? 0.f : M;
    const float S = wave_sum(s4.y * __expf(s4.x - mref));
    const float zt = wave_sum(s4.z);
    const bool bad = __any(s4.w != 0.f) != 0;
    const float lse = M + __logf(S);
    const int t = tgt ? tgt[r] : -1;
    const bool has_t = t >= 0 && t < NT;
    float v[2];
    int ix[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      const bool in = c < strips * NC;
      v[h] = in ? cv[(size_t)r * strips * NC + c] : -INFINITY;
      ix[h] = in ? ci[(size_t)r * strips * NC + c] : INT_MAX;
      if (ix[h] >= NT) { v[h] = -INFINITY; ix[h] = INT_MAX; }   // an empty entry, or a column behind NT (fold_tile)
    }
    int my_id = -1;
    float my_lp = -INFINITY;
    int pos = -1;
    if (!norow && !bad) {
      for (int k = 0; k < topk; ++k) {
        const bool first = cand_before(v[0], ix[0], v[1], ix[1]);
        float bv = first ? v[0] : v[1];
        int bi = first ? ix[0] : ix[1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        // class indices are unique over the strips: the winner leaves its holder's pair
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (bi != INT_MAX && ix[h] == bi) { v[h] = -INFINITY; ix[h] = INT_MAX; }
        if (lane == k) { my_id = bi == INT_MAX ? -1 : bi; my_lp = bi == INT_MAX ? -INFINITY : bv - lse; }
        if (has_t && bi == t && pos < 0) pos = k;
      }
    }
    if (norow) { my_id = -1; my_lp = -INFINITY; }
    if (bad && !norow) { my_id = -1; my_lp = qnan; }
    if (lane < topk) {
      if (topk_ids) topk_ids[(size_t)r * topk + lane] = my_id;
      if (topk_logprob) topk_logprob[(size_t)r * topk + lane] = my_lp;
    }
    if (lane == 0) {
      if (lse_out) lse_out[r] = (norow || bad) ? qnan : lse;
      if (target_logprob) target_logprob[r] = (norow || bad || !has_t) ? qnan : zt - lse;
      if (target_pos) target_pos[r] = pos;
    }
    counted = norow ? 0 : 1;
    hit0 = pos == 0;
    hitk = pos >= 0;
  }
  if (counts) {
    if (lane == 0) { cnt[0][wave] = counted; cnt[1][wave] = hit0; cnt[2][wave] = hitk; }
    __syncthreads();
    if (threadIdx.x < 3)
      counts[3 * blockIdx.x + threadIdx.x] = cnt[threadIdx.x][0] + cnt[threadIdx.x][1] + cnt[threadIdx.x][2] + cnt[threadIdx.x][3];
  }
}

__global__ __launch_bounds__(256) void token_topk_totals_kernel(const int32_t* counts, int nblocks, int32_t* totals) {
  __shared__ int red[3][4];
  int a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { a += counts[3 * i]; b += counts[3 * i + 1]; c += counts[3 * i + 2]; }
  a = wave_sum_i(a); b = wave_sum_i(b); c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x < 3) totals[threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// Row list and targets of a report (engine_eval.cpp: plb_token_report). CSR form (offsets != NULL): entry j of flat belongs
// to the sample b with offsets[b] <= j < offsets[b+1]. Full form: entry j is position (j / S, j % S). A position behind its
// sample's length (or outside [0, S)) has no row: -1.
__global__ __launch_bounds__(256) void token_topk_prepare_kernel(const int32_t* offsets, const int32_t* flat, const int32_t* lengths,
                                                                 const int32_t* row_start, const int64_t* token_ids, int n, int B,
                                                                 int S, int32_t* rows, int32_t* tgt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int b, s;
  if (offsets) {
    int lo = 0, hi = B;   // the last b < B with offsets[b] <= j
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (offsets[mid] <= j) lo = mid; else hi = mid;
    }
    b = lo; s = flat[j];
  } else {
    b = j / S; s = j - b * S;
  }
  const int len = lengths ? clamp_len(lengths[b], S) : S;
  const bool ok = s >= 0 && s < len;
  rows[j] = ok ? (row_start ? row_start[b] : b * S) + s : -1;
  tgt[j] = (ok && token_ids) ? (int32_t)token_ids[(size_t)b * S + s] : -1;
}
}  // namespace

// Strip count of a launch: the policy (strips == 0) fills 256 CUs about twice with row_tiles x strips workgroups; never
// more than PLB_TOPK_MAX_STRIPS or the number of column tiles, and no strip without a tile.
extern "C" int plb_token_topk_strips(int n, int NT, int strips) {
  if (n < 1 || NT < 1 || strips < 0) return 0;
  const int row_tiles = (n + BM - 1) / BM, ntiles = (NT + BN - 1) / BN;
  int s = strips ? strips : (512 + row_tiles - 1) / row_tiles;
  if (s > PLB_TOPK_MAX_STRIPS) s = PLB_TOPK_MAX_STRIPS;
  if (s > ntiles) s = ntiles;
  const int per = (ntiles + s - 1) / s;
  return (ntiles + per - 1) / per;
}

extern "C" size_t plb_token_topk_scratch_bytes(int n) {
  if (n < 0) return 0;
  const size_t rows = (size_t)n;
  return rows * PLB_TOPK_MAX_STRIPS * (PLB_TOPK_MAX * 8 + 16) + (rows + 3) / 4 * 12 + 256;
}

extern "C" int plb_launch_token_topk(const bf16_t* X, int ldx, const int32_t* rows, int n, const bf16_t* W, int ldw,
                                     const float* bias, int NT, int K, int topk, int strips, void* scratch, const int32_t* tgt,
                                     int32_t* topk_ids, float* topk_logprob, float* lse, float* target_logprob,
                                     int32_t* target_pos, float* logits, int32_t* totals, hipStream_t stream) {
  if (n < 0 || NT < 1 || K < BK || K % BK || ldx < K || ldw < K || ldx % 8 || ldw % 8) return 1;
  if (topk < 0 || topk > PLB_TOPK_MAX || strips < 0 || strips > PLB_TOPK_MAX_STRIPS) return 1;
  if ((target_logprob || target_pos || totals) && !tgt) return 1;
  if (n == 0) {
    if (totals && hipMemsetAsync(totals, 0, 3 * sizeof(int32_t), stream) != hipSuccess) return 2;
    return 0;
  }
  if (!X || !W || !bias || !scratch) return 1;
  if ((((uintptr_t)X | (uintptr_t)W) & 3) || ((uintptr_t)scratch & 15)) return 1;   // (operands as the NT GEMMs take them: the flat weight copy's tensors start on 4-byte boundaries)
  const int ns = plb_token_topk_strips(n, NT, strips);
  const int ntiles = (NT + BN - 1) / BN, row_tiles = (n + BM - 1) / BM;
  // scratch: statistics float4 [n][ns] | values float [n][ns][8] | indices int32 [n][ns][8] | counts int32 [ceil(n/4)][3]
  float4* st = (float4*)scratch;
  float* cv = (float*)(st + (size_t)n * ns);
  int32_t* ci = (int32_t*)(cv + (size_t)n * ns * NC);
  int32_t* counts = ci + (size_t)n * ns * NC;
  TopkStrips p;
  p.X = X; p.ldx = ldx; p.rows = rows; p.n = n; p.W = W; p.ldw = ldw; p.bias = bias; p.NT = NT; p.K = K;
  p.strips = ns; p.tiles_per_strip = (ntiles + ns - 1) / ns; p.ntiles = ntiles;
  p.tgt = tgt; p.cv = cv; p.ci = ci; p.st = st; p.logits = logits;
  {
    const double cols = (double)ntiles * BN, mrows = (double)row_tiles * BM;
    ProfScope ps(PLB_K_GEMM_NT_CE, stream, 2.0 * mrows * cols * K,
                 2.0 * (mrows * K + cols * K * row_tiles) + (logits ? 4.0 * n * NT : 0.0) + (double)n * ns * (NC * 8 + 16));
    hipLaunchKernelGGL(token_topk_strips_kernel, dim3((unsigned)(row_tiles * ns)), dim3(256), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return 2;
  }
  const int nblocks = (n + 3) / 4;
  ProfScope ps(PLB_K_TOKEN_CE, stream, 0, (double)n * (ns * (NC * 8 + 16) + 8.0 * topk + 16.0));
  hipLaunchKernelGGL(token_topk_merge_kernel, dim3((unsigned)nblocks), dim3(256), 0, stream, cv, ci, st, ns, rows, tgt, n, NT, topk,
                     topk_ids, topk_logprob, lse, target_logprob, target_pos, totals ? counts : nullptr);
  if (hipGetLastError() != hipSuccess) return 2;
  if (totals) hipLaunchKernelGGL(token_topk_totals_kernel, dim3(1), dim3(256), 0, stream, counts, nblocks, totals);
  return LAUNCH_OK();
}

extern "C" int plb_launch_token_topk_prepare(const int32_t* offsets, const int32_t* flat, const int32_t* lengths,
                                             const int32_t* row_start, const int64_t* token_ids, int n, int B, int S,
                                             int32_t* rows, int32_t* tgt, hipStream_t stream) {
  if (n < 0 || B < 1 || S < 1 || !rows || !tgt) return 1;
  if (offsets ? !flat && n > 0 : (int64_t)n != (int64_t)B * S) return 1;
  if (n == 0) return 0;
  ProfScope ps(PLB_K_TOKEN_CE, stream, 0, 16.0 * n);
  hipLaunchKernelGGL(token_topk_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, offsets, flat, lengths,
                     row_start, token_ids, n, B, S, rows, tgt);
  return LAUNCH_OK();
}
