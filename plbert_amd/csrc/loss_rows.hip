// Loss rows of the PL-BERT step, gfx950: masked-row gather / scatter, masked cross-entropy forward + backward
// (calculate_phoneme_loss, train.py:107-131), the merge step of the fused token-head cross-entropy, and the row
// bookkeeping of token-packed calls (pack_token_targets, unpack_rows, seed_dy) with the pooler and the bf16 -> fp32 copy
// of the encoder's outputs. One wave per row where a row is reduced; HBM- or latency-bound.
// The padded and the packed member of a pair (ce_prepare, token_ce_combine) stay separate entry points: a row's results
// are the same bits in both layouts, and tests/ hold each member against the other.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
__global__ void gather_rows_kernel(const bf16_t* src, int lds_, const int32_t* rows, int n, int npad, int H,
                                   bf16_t* dst, int ldd) {
  const int r = blockIdx.x;
  const int chunks = H / 8;
  const bool live = r < n;
  const size_t srow = live ? (size_t)rows[r] : 0;
  for (int c = threadIdx.x; c < chunks; c += blockDim.x) {
    uint4 v = live ? *(const uint4*)(src + srow * lds_ + c * 8) : make_uint4(0, 0, 0, 0);
    *(uint4*)(dst + (size_t)r * ldd + c * 8) = v;
  }
}
}  // namespace
extern "C" int plb_launch_gather_rows(const bf16_t* src, int lds_, const int32_t* rows, int n, int npad, int H,
                                      bf16_t* dst, int ldd, hipStream_t stream) {
  if (H % 8 || npad <= 0) return 1;
  ProfScope ps(PLB_K_ROWS, stream, 0, 4.0 * (double)npad * H);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(npad), dim3(128), 0, stream, src, lds_, rows, n, npad, H, dst, ldd);
  return LAUNCH_OK();
}

namespace {
__global__ void scatter_rows_kernel(const bf16_t* src, int lds_, const int32_t* rows, int n, int H, bf16_t* dst,
                                    int ldd) {
  const int r = blockIdx.x;
  if (r >= n) return;
  const size_t drow = (size_t)rows[r];
  for (int c = threadIdx.x; c < H / 8; c += blockDim.x)
    *(uint4*)(dst + drow * ldd + c * 8) = *(const uint4*)(src + (size_t)r * lds_ + c * 8);
}
}  // namespace
extern "C" int plb_launch_scatter_rows(const bf16_t* src, int lds_, const int32_t* rows, int n, int H, bf16_t* dst,
                                       int ldd, hipStream_t stream) {
  if (H % 8) return 1;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(n), dim3(128), 0, stream, src, lds_, rows, n, H, dst, ldd);
  return LAUNCH_OK();
}

namespace {
// calculate_phoneme_loss (train.py:107-131): per-sample mean over its masked indices, then mean over
// the samples that have any. One thread per sample.
__global__ void ce_prepare_kernel(const int32_t* offsets, const int32_t* flat, const int64_t* labels, int B, int S,
                                  const int32_t* row_start, int32_t* rows, int32_t* tgt, float* w) {
  // one block per sample; every block counts the non-empty samples itself (B is small)
  __shared__ int cnt[4];
  int c = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) c += offsets[b + 1] > offsets[b];
  c = (int)wave_sum((float)c);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  const int count = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  const int b = blockIdx.x;
  const int j0 = offsets[b], j1 = offsets[b + 1];
  const float wb = (j1 > j0) ? 1.0f / ((float)(j1 - j0) * (float)count) : 0.f;
  for (int j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
    const int idx = flat[j];
    rows[j] = row_start ? row_start[b] + idx : b * S + idx;
    tgt[j] = (int32_t)labels[(size_t)b * S + idx];
    w[j] = wb;
  }
}
}  // namespace
extern "C" int plb_launch_ce_prepare(const int32_t* offsets, const int32_t* flat, const int64_t* labels, int B, int S,
                                     int32_t* rows, int32_t* tgt, float* w, hipStream_t stream) {
  hipLaunchKernelGGL(ce_prepare_kernel, dim3(B), dim3(256), 0, stream, offsets, flat, labels, B, S, nullptr, rows, tgt, w);
  return LAUNCH_OK();
}
extern "C" int plb_launch_ce_prepare_packed(const int32_t* offsets, const int32_t* flat, const int64_t* labels, int B, int S,
                                            const int32_t* row_start, int32_t* rows, int32_t* tgt, float* w,
                                            hipStream_t stream) {
  if (!row_start || B < 1 || S < 1) return 1;
  hipLaunchKernelGGL(ce_prepare_kernel, dim3(B), dim3(256), 0, stream, offsets, flat, labels, B, S, row_start, rows, tgt, w);
  return LAUNCH_OK();
}

namespace {
// nn.CrossEntropyLoss on one row per wave: V <= 256 classes, 4 per lane.
__global__ __launch_bounds__(256) void ce_kernel(const float* logits, int ldl, int V, const int32_t* tgt, const float* w,
                                                 int n, int npad, float* loss_rows, bf16_t* dlogits, int ldd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= npad) return;
  const int c = lane * 4;
  if (r >= n) {  // padding rows: zero gradient
    if (c < ldd) *(uint2*)(dlogits + (size_t)r * ldd + c) = make_uint2(0, 0);
    return;
  }
  float z[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) z[j] = (c + j < V) ? logits[(size_t)r * ldl + c + j] : -INFINITY;
  const float mx = wave_max(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
  float e[4], s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { e[j] = (c + j < V) ? __expf(z[j] - mx) : 0.f; s += e[j]; }
  s = wave_sum(s);
  const int t = tgt[r];
  const float wr = w[r];
  float zt = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) zt += (c + j == t) ? z[j] : 0.f;
  zt = wave_sum(zt);
  if (lane == 0) loss_rows[r] = wr * (mx + __logf(s) - zt);
  const float inv = wr / s;
  if (c < ldd) {
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = (c + j < V) ? e[j] * inv - ((c + j == t) ? wr : 0.f) : 0.f;
    uint2 o; o.x = pack_bf2(g[0], g[1]); o.y = pack_bf2(g[2], g[3]);
    *(uint2*)(dlogits + (size_t)r * ldd + c) = o;
  }
}
}  // namespace
extern "C" int plb_launch_ce_fwd_bwd(const float* logits, int ldl, int V, const int32_t* tgt, const float* w, int n,
                                     int npad, float* loss_rows, bf16_t* dlogits, int ldd, hipStream_t stream) {
  if (V > 256 || ldd > 256 || ldd % 4 || npad <= 0) return 1;
  ProfScope ps(PLB_K_CE, stream, 0, (double)npad * (4.0 * V + 2.0 * ldd));
  hipLaunchKernelGGL(ce_kernel, dim3((npad + 3) / 4), dim3(256), 0, stream, logits, ldl, V, tgt, w, n, npad, loss_rows,
                     dlogits, ldd);
  return LAUNCH_OK();
}

namespace {
// Fused token-head CE, between its two GEMM passes: one wave per row merges the per-tile (max, sum) pairs. The merge of one
// valid row (shared by the padded and the packed kernel: a row's lse / w / loss are the same bits in both layouts).
__device__ __forceinline__ void token_ce_merge_row(const float* pmax, const float* psum, int ntiles, const float* tlogit, int t,
                                                   int lane, int B, int len, float* lse, float* w, float* loss_rows) {
  float m = -INFINITY, l = 0.f;
  for (int i = lane; i < ntiles; i += 64) {
    const float pm = pmax[(size_t)t * ntiles + i], ps = psum[(size_t)t * ntiles + i];
    if (pm > m) { l *= __expf(m - pm); m = pm; }
    // a tile without a real class is (-inf, 0): as a lane's first tile, exp(-inf - -inf) would make its 0 a NaN for good
    if (pm > -INFINITY) l += ps * __expf(pm - m);
  }
  const float M = wave_max(m);
  l = wave_sum(m == -INFINITY ? 0.f : l * __expf(m - M));
  if (lane == 0) {
    const float ls = M + __logf(l), wt = 1.0f / ((float)B * (float)len);
    lse[t] = ls; w[t] = wt; loss_rows[t] = wt * (ls - tlogit[t]);
  }
}
__global__ __launch_bounds__(256) void token_ce_combine_kernel(const float* pmax, const float* psum, int ntiles,
                                                               const float* tlogit, const int32_t* lengths, int B, int S,
                                                               int rows, float* lse, float* w, float* loss_rows) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= rows) return;
  const int T = B * S, b = t / S, sp = t - b * S;
  int len = S;
  if (t < T && lengths) len = clamp_len(lengths[b], S);
  if (t >= T || sp >= len) {
    if (lane == 0) { lse[t] = 0.f; w[t] = 0.f; loss_rows[t] = 0.f; }
    return;
  }
  token_ce_merge_row(pmax, psum, ntiles, tlogit, t, lane, B, len, lse, w, loss_rows);
}
}  // namespace
extern "C" int plb_launch_token_ce_combine(const float* pmax, const float* psum, int ntiles, const float* tlogit,
                                           const int32_t* lengths, int B, int S, int rows, float* lse, float* w,
                                           float* loss_rows, hipStream_t stream) {
  if (ntiles < 1 || rows < B * S) return 1;
  ProfScope ps(PLB_K_TOKEN_CE, stream, 0, (double)rows * ntiles * 8.0);
  hipLaunchKernelGGL(token_ce_combine_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, pmax, psum, ntiles, tlogit, lengths,
                     B, S, rows, lse, w, loss_rows);
  return LAUNCH_OK();
}

namespace {
// The same on token-packed rows: row t belongs to the sample the plan gives it (wave-uniform: one row per wave); the rest
// of a slot and the tail up to `rows` get lse = w = loss = 0, which is what makes pass 2 write exact zeros there.
__global__ __launch_bounds__(256) void token_ce_combine_packed_kernel(const float* pmax, const float* psum, int ntiles,
                                                                      const float* tlogit, const int32_t* lengths,
                                                                      const int32_t* row_start, int B, int S, int rows, float* lse,
                                                                      float* w, float* loss_rows) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= rows) return;
  int b, sp;
  if (!packed_locate(row_start, lengths, B, S, t, &b, &sp)) {
    if (lane == 0) { lse[t] = 0.f; w[t] = 0.f; loss_rows[t] = 0.f; }
    return;
  }
  const int len = clamp_len(lengths[b], S);
  token_ce_merge_row(pmax, psum, ntiles, tlogit, t, lane, B, len, lse, w, loss_rows);
}
}  // namespace
extern "C" int plb_launch_token_ce_combine_packed(const float* pmax, const float* psum, int ntiles, const float* tlogit,
                                                  const int32_t* lengths, const int32_t* row_start, int B, int S, int rows,
                                                  float* lse, float* w, float* loss_rows, hipStream_t stream) {
  if (!pmax || !psum || !tlogit || !lengths || !row_start || !lse || !w || !loss_rows) return 1;
  if (ntiles < 1 || B < 1 || S < 1 || rows < 1) return 1;
  ProfScope ps(PLB_K_TOKEN_CE, stream, 0, (double)rows * ntiles * 8.0);
  hipLaunchKernelGGL(token_ce_combine_packed_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, pmax, psum, ntiles, tlogit,
                     lengths, row_start, B, S, rows, lse, w, loss_rows);
  return LAUNCH_OK();
}

namespace {
// Token targets of a packed dual-head call: ONE pass writes every one of the `rows` int64 targets exactly once —
// token_ids[b, s] on row row_start[b] + s for s < lengths[b], 0 on every other row (the rest of a slot, the tail up to
// `rows`) — so nothing has to clear the buffer first, and token_ids is never read at a pad position (it may hold anything
// there). One lane per two rows (row_start and `rows` are multiples of 128: a pair never straddles two slots): two 8-byte
// loads, one 16-byte store. The sample of a row is found by searching the plan, as the packed embedding kernel does.
__global__ __launch_bounds__(256) void pack_token_targets_kernel(const int64_t* token_ids, const int32_t* lengths,
                                                                 const int32_t* row_start, int B, int S, int pairs, int64_t* out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < pairs; i += gridDim.x * 256) {
    const int r = 2 * i;
    int b, s;
    longlong2 o = make_longlong2(0, 0);
    if (packed_locate(row_start, lengths, B, S, r, &b, &s)) {
      int len = lengths[b];   // written out: through clamp_len hipcc allocates two registers of this kernel differently
      len = len < 1 ? 1 : (len > S ? S : len);
      const int64_t* src = token_ids + (size_t)b * S + s;
      o.x = src[0];
      if (s + 1 < len) o.y = src[1];
    }
    *(longlong2*)(out + r) = o;
  }
}
}  // namespace
extern "C" int plb_launch_pack_token_targets(const int64_t* token_ids, const int32_t* lengths, const int32_t* row_start, int B,
                                             int S, int rows, int64_t* out, hipStream_t stream) {
  if (!token_ids || !lengths || !row_start || !out || B < 1 || S < 1) return 1;
  if (rows < 128 || rows % 128) return 1;   // (a plan's row count: pairs of rows never straddle two slots)
  if (((uintptr_t)token_ids & 7) || ((uintptr_t)out & 15)) return 1;
  const int pairs = rows / 2, blocks = (pairs + 255) / 256;
  ProfScope ps(PLB_K_CAST, stream, 0, (double)rows * 16.0);
  hipLaunchKernelGGL(pack_token_targets_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, token_ids,
                     lengths, row_start, B, S, pairs, out);
  return LAUNCH_OK();
}

namespace {
// token-packed rows (row_start == null: rows already in the padded b*S + s order) to [B,S,C] fp32 with zeros at the pad
// positions: one block per (b, s)
template <typename T>
__global__ __launch_bounds__(256) void unpack_rows_kernel(const T* src, int lds_, const int32_t* row_start, const int32_t* lengths,
                                                          int S, int C, float* dst) {
  const int b = blockIdx.x / S, s = blockIdx.x - b * S;
  const int len = clamp_len(lengths[b], S);
  float* d = dst + (size_t)blockIdx.x * C;
  if (s >= len) {
    for (int c = threadIdx.x; c < C; c += 256) d[c] = 0.f;
    return;
  }
  const T* r = src + (size_t)(row_start ? row_start[b] + s : blockIdx.x) * lds_;
  for (int c = threadIdx.x; c < C; c += 256) {
    if constexpr (sizeof(T) == 2) d[c] = bf2f(r[c]); else d[c] = r[c];
  }
}
}  // namespace
extern "C" int plb_launch_unpack_rows(const void* src, int src_is_bf16, int lds_, const int32_t* row_start,
                                      const int32_t* lengths, int B, int S, int C, float* dst, hipStream_t stream) {
  if (!src || !lengths || !dst || B < 1 || S < 1 || C < 1 || lds_ < C) return 1;
  ProfScope ps(PLB_K_CAST, stream, 0, (double)B * S * C * 6.0);
  if (src_is_bf16)
    hipLaunchKernelGGL(unpack_rows_kernel<bf16_t>, dim3((unsigned)(B * S)), dim3(256), 0, stream, (const bf16_t*)src, lds_,
                       row_start, lengths, S, C, dst);
  else
    hipLaunchKernelGGL(unpack_rows_kernel<float>, dim3((unsigned)(B * S)), dim3(256), 0, stream, (const float*)src, lds_,
                       row_start, lengths, S, C, dst);
  return LAUNCH_OK();
}

namespace {
// Output gradient of the last application from a caller's fp32 [B,S,H] gradient (plb_encode_bwd): ONE pass writes every
// one of the Tp rows of dy exactly once — bf16(d_hidden[b,s,:]) (round to nearest even, as cast_bf16_kernel) on the row that
// holds token (b, s < lengths[b]), zeros on every other row (pad positions, the rest of a packed slot, the tail up to Tp) —
// so nothing has to clear dy first, and d_hidden is never read at a pad position (it may hold anything there). One lane per
// four columns: a 16-byte load, an 8-byte store, 6 bytes of traffic per element. row_start (or null: padded rows b*S + s):
// the sample of a packed row is found by searching the plan, as the packed embedding kernel does.
__global__ __launch_bounds__(256) void seed_dy_kernel(const float* d_hidden, const int32_t* lengths, const int32_t* row_start, int B,
                                                      int S, int H4, unsigned int total, bf16_t* dy) {
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
    uint2 o = make_uint2(0u, 0u);
    if (live) {
      const float4 v = *(const float4*)(d_hidden + ((size_t)b * S + s) * ((size_t)H4 * 4) + (size_t)c * 4);
      o.x = pack_bf2(v.x, v.y); o.y = pack_bf2(v.z, v.w);
    }
    *(uint2*)(dy + (size_t)i * 4) = o;
  }
}
}  // namespace
extern "C" int plb_launch_seed_dy(const float* d_hidden, const int32_t* lengths, const int32_t* row_start, int B, int S, int H,
                                  int Tp, bf16_t* dy, hipStream_t stream) {
  if (!d_hidden || !dy || B < 1 || S < 1 || H < 4 || H % 4 || Tp < 1) return 1;
  if (row_start ? !lengths : (int64_t)Tp < (int64_t)B * S) return 1;   // (packed: the plan's rows; padded: at least B*S of them)
  if (((uintptr_t)d_hidden & 15) || ((uintptr_t)dy & 7)) return 1;
  const int64_t total = (int64_t)Tp * (H / 4);
  if (total >= ((int64_t)1 << 31)) return 1;
  const int64_t blocks = (total + 255) / 256;
  ProfScope ps(PLB_K_CAST, stream, 0, (double)Tp * H * 6.0);
  hipLaunchKernelGGL(seed_dy_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, d_hidden, lengths,
                     row_start, B, S, H / 4, (unsigned int)total, dy);
  return LAUNCH_OK();
}

namespace {
// AlbertModel pooler (modeling_albert.py:403): one wave per output feature, fp32 dot over H, tanh.
__global__ __launch_bounds__(256) void pooler_kernel(const float* hidden, int S, int H, const float* W, const float* bias,
                                                     float* pooled) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= H) return;
  const float* x = hidden + (size_t)b * S * H;
  const float* w = W + (size_t)o * H;
  float s = 0.f;
  for (int k = lane * 4; k < H; k += 256) {
    const float4 a = *(const float4*)(x + k), c = *(const float4*)(w + k);
    s += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
  }
  s = wave_sum(s);
  if (lane == 0) pooled[(size_t)b * H + o] = tanhf(s + bias[o]);
}
}  // namespace
extern "C" int plb_launch_pooler(const float* hidden, int B, int S, int H, const float* W, const float* bias, float* pooled,
                                 hipStream_t stream) {
  if (H % 4 || B < 1 || S < 1) return 1;
  hipLaunchKernelGGL(pooler_kernel, dim3((H + 3) / 4, B), dim3(256), 0, stream, hidden, S, H, W, bias, pooled);
  return LAUNCH_OK();
}

namespace {
__global__ void bf16_to_f32_kernel(const bf16_t* src, int lds_, float* dst, int ldd, int R, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * C) return;
  const size_t r = i / C, c = i % C;
  dst[r * ldd + c] = bf2f(src[r * lds_ + c]);
}
}  // namespace
extern "C" int plb_launch_bf16_to_f32(const bf16_t* src, int lds_, float* dst, int ldd, int R, int C, hipStream_t stream) {
  const size_t n = (size_t)R * C;
  if (!n) return 0;
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, lds_, dst, ldd, R, C);
  return LAUNCH_OK();
}
