// Embeddings of the PL-BERT step, gfx950 (A4 / A11): gather + LayerNorm forward, its backward, and the scatter-add of the
// table gradients.
// AlbertEmbeddings.forward (modeling_albert.py:67-106): LN_E(word[id] + type[0] + pos[s]); E <= 256.
// One wave per token, 16-byte (4 x fp32) table reads, wave-shuffle reductions, fp32 statistics (layer_norm_eps = 1e-12 is
// below bf16 resolution). No atomics anywhere: every sum has a fixed order. Token-packed calls (PlbEmbed.row_start) find
// a row's token through packed_locate (row_common.h).
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
template <bool BWD>
__global__ __launch_bounds__(256) void embed_kernel(PlbEmbed p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = p.E;
  const int c = lane * 4;  // this lane's 4 columns
  const bool act = c < E;
  float4 g4 = make_float4(0, 0, 0, 0), b4 = g4, ty = g4;
  if (act) {
    g4 = *(const float4*)(p.gamma + c);
    b4 = *(const float4*)(p.beta + c);
    ty = *(const float4*)(p.type0 + c);
  }
  float dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};
  const float invE = 1.0f / (float)E;
  for (int t = blockIdx.x * 4 + wave; t < p.T; t += gridDim.x * 4) {
    int src = t, s = 0;
    if (p.row_start) {   // packed row t -> token (b, s) of the padded ids (wave-uniform: one row per wave)
      int b;
      const bool owned = packed_locate(p.row_start, p.lengths, p.B, p.S, t, &b, &s);
      // (fill_slots: a row behind the length but inside the sample's slot and the sequence is a pad position of the ids)
      if (!owned && !(!BWD && p.fill_slots && s < p.S && t < p.row_start[b + 1])) {
        if (act) {
          if (!BWD) *(uint2*)(p.out + (size_t)t * p.ldo + c) = make_uint2(0u, 0u);
          else *(float4*)(p.dx + (size_t)t * E + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        continue;
      }
      src = b * p.S + s;
    } else {
      s = t % p.S;
    }
    long long id = p.ids[src];
    if (id < 0 || id >= p.V) id = 0;  // host validates; never index out of the table
    float x[4] = {0, 0, 0, 0};
    if (act) {
      float4 w = *(const float4*)(p.word + (size_t)id * E + c);
      float4 ps = *(const float4*)(p.pos + (size_t)s * E + c);
      x[0] = w.x + ty.x + ps.x; x[1] = w.y + ty.y + ps.y; x[2] = w.z + ty.z + ps.z; x[3] = w.w + ty.w + ps.w;
    }
    const float mean = wave_sum(x[0] + x[1] + x[2] + x[3]) * invE;
    float d[4], vs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = act ? x[j] - mean : 0.f; vs += d[j] * d[j]; }
    const float rstd = rsqrtf(wave_sum(vs) * invE + p.eps);
    if (!BWD) {
      if (act) {
        uint2 o;
        o.x = pack_bf2(d[0] * rstd * g4.x + b4.x, d[1] * rstd * g4.y + b4.y);
        o.y = pack_bf2(d[2] * rstd * g4.z + b4.z, d[3] * rstd * g4.w + b4.w);
        *(uint2*)(p.out + (size_t)t * p.ldo + c) = o;
      }
    } else {
      float dy[4] = {0, 0, 0, 0}, xh[4], dxh[4], s1 = 0.f, s2 = 0.f;
      if (act) {
        uint2 u = *(const uint2*)(p.dout + (size_t)t * p.lddo + c);
        dy[0] = bf_lo(u.x); dy[1] = bf_hi(u.x); dy[2] = bf_lo(u.y); dy[3] = bf_hi(u.y);
      }
      const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xh[j] = d[j] * rstd;
        dxh[j] = dy[j] * gg[j];
        s1 += dxh[j]; s2 += dxh[j] * xh[j];
        dg[j] += dy[j] * xh[j]; db[j] += dy[j];
      }
      s1 = wave_sum(s1) * invE; s2 = wave_sum(s2) * invE;
      if (act)  // gradient of the pre-LayerNorm sum, consumed by embed_scatter_kernel (no atomics)
        *(float4*)(p.dx + (size_t)t * E + c) =
            make_float4(rstd * (dxh[0] - s1 - xh[0] * s2), rstd * (dxh[1] - s1 - xh[1] * s2),
                        rstd * (dxh[2] - s1 - xh[2] * s2), rstd * (dxh[3] - s1 - xh[3] * s2));
    }
  }
  if (BWD) {
    __shared__ float red[4][2][256];
    if (act) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { red[wave][0][c + j] = dg[j]; red[wave][1][c + j] = db[j]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * E; i += 256) {
      const int which = i / E, col = i % E;
      p.partials[(size_t)blockIdx.x * 2 * E + i] =
          red[0][which][col] + red[1][which][col] + red[2][which][col] + red[3][which][col];
    }
  }
}
}  // namespace
extern "C" int plb_launch_embed_fwd(const PlbEmbed* p, hipStream_t stream) {
  if (p->E % 4 || p->E > 256 || p->T <= 0) return 1;
  if (p->row_start && (!p->lengths || p->B < 1)) return 1;
  int blocks = (p->T + 3) / 4; if (blocks > 2048) blocks = 2048;
  ProfScope ps(PLB_K_EMBED_FWD, stream, 0, (double)p->T * (8 + 2.0 * p->E));
  hipLaunchKernelGGL((embed_kernel<false>), dim3(blocks), dim3(256), 0, stream, *p);
  return LAUNCH_OK();
}
extern "C" int plb_launch_embed_bwd(const PlbEmbed* p, hipStream_t stream) {
  if (p->E % 4 || p->E > 256 || p->T <= 0 || p->nblocks <= 0) return 1;
  if (p->row_start && (!p->lengths || p->B < 1)) return 1;
  ProfScope ps(PLB_K_EMBED_BWD, stream, 0, (double)p->T * (8 + 2.0 * p->E + 8.0 * p->E));
  hipLaunchKernelGGL((embed_kernel<true>), dim3(p->nblocks), dim3(256), 0, stream, *p);
  return LAUNCH_OK();
}

namespace {
// Scatter-add of the embedding gradient without atomics (deterministic): block v < V owns word row v
// (collects the tokens whose id is v into an LDS list, then sums their dx rows in token order), block
// V + s owns position row s (sum over the batch). Row 0 of the word table is the padding row
// (nn.Embedding(padding_idx=0), modeling_albert.py:56): no gradient.
// The token range is walked in chunks of EMB_CHUNK tokens so the list fits LDS for any T (configs/config.yml:16
// is 96 x 512 = 49,152 tokens on one GPU).
constexpr int EMB_CHUNK = 32768;
// PACKED (PlbEmbed.row_start): the ids are still walked in the padded [B,S] order — the lists, and with them the order of
// every sum, are those of the padded call — and only the row of dx a token is read from comes from the plan; pad
// positions (exact zeros in the padded call) are left out.
template <bool PACKED>
__global__ __launch_bounds__(256) void embed_scatter_kernel(PlbEmbed p, int P) {
  extern __shared__ int list[];  // 4 per-wave segments of matching token indices
  __shared__ int wcnt[4];
  __shared__ float4 part[256];
  const int E = p.E, T = PACKED ? p.B * p.S : p.T;
  const int row = blockIdx.x;
  const int EQ = E >> 2;                                   // float4 columns per row
  const int q = threadIdx.x % EQ, grp = threadIdx.x / EQ, ngrp = 256 / EQ;  // E = 128: 32 x 8
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add = [&](int t) {
    const float4 v = *(const float4*)(p.dx + (size_t)t * E + 4 * q);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  };
  if (row < p.V) {
    // each wave scans its own quarter of the chunk (64-token pieces, round-robin) and appends the matches to its
    // own list segment: no block barrier inside the scan. Fixed order -> deterministic.
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = T < EMB_CHUNK ? T : EMB_CHUNK;
    const int cap = (chunk + 3) / 4 + 64;
    for (int c0 = 0; c0 < T && row != 0; c0 += EMB_CHUNK) {
      const int c1 = c0 + EMB_CHUNK < T ? c0 + EMB_CHUNK : T;
      int cnt = 0;
      for (int t0 = c0 + w * 64; t0 < c1; t0 += 256) {
        const int t = t0 + lane;
        bool hit = t < c1 && p.ids[t] == row;
        int trow = t;   // the row of dx that holds token t
        if (PACKED && hit) {
          const int b = t / p.S, sp = t - b * p.S;
          hit = sp < max(p.lengths[b], 1);   // (lengths are clamped to [1, S] everywhere: packed_locate; sp < S always)
          trow = p.row_start[b] + sp;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
        if (hit) list[w * cap + cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = trow;
        cnt += __builtin_popcountll(m);
      }
      if (lane == 0) wcnt[w] = cnt;
      __syncthreads();
      // a few ids (separator, mask) own thousands of tokens: ngrp row groups x 4 loads in flight each
      for (int ww = 0; ww < 4; ++ww) {
        const int n = wcnt[ww];
        const int* l = list + ww * cap;
        int i = grp;
        for (; i + 7 * ngrp < n; i += 8 * ngrp) {   // the mask id owns ~12 % of the tokens: its block is the launch's duration
          float4 v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = *(const float4*)(p.dx + (size_t)l[i + k * ngrp] * E + 4 * q);
          s.x += ((v[0].x + v[1].x) + (v[2].x + v[3].x)) + ((v[4].x + v[5].x) + (v[6].x + v[7].x));
          s.y += ((v[0].y + v[1].y) + (v[2].y + v[3].y)) + ((v[4].y + v[5].y) + (v[6].y + v[7].y));
          s.z += ((v[0].z + v[1].z) + (v[2].z + v[3].z)) + ((v[4].z + v[5].z) + (v[6].z + v[7].z));
          s.w += ((v[0].w + v[1].w) + (v[2].w + v[3].w)) + ((v[4].w + v[5].w) + (v[6].w + v[7].w));
        }
        for (; i + 3 * ngrp < n; i += 4 * ngrp) {
          const int t0 = l[i], t1 = l[i + ngrp], t2 = l[i + 2 * ngrp], t3 = l[i + 3 * ngrp];
          const float4 v0 = *(const float4*)(p.dx + (size_t)t0 * E + 4 * q), v1 = *(const float4*)(p.dx + (size_t)t1 * E + 4 * q);
          const float4 v2 = *(const float4*)(p.dx + (size_t)t2 * E + 4 * q), v3 = *(const float4*)(p.dx + (size_t)t3 * E + 4 * q);
          s.x += (v0.x + v1.x) + (v2.x + v3.x); s.y += (v0.y + v1.y) + (v2.y + v3.y);
          s.z += (v0.z + v1.z) + (v2.z + v3.z); s.w += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; i < n; i += ngrp) add(l[i]);
      }
      __syncthreads();  // the lists are rewritten by the next chunk
    }
  } else {
    const int sidx = row - p.V;  // position row: sum over the batch
    if (sidx < p.S) {
      if (PACKED) {
        for (int b = grp; b < p.B; b += ngrp)
          if (sidx < max(p.lengths[b], 1)) add(p.row_start[b] + sidx);
      } else {
        for (int t = sidx + grp * p.S; t < T; t += ngrp * p.S) add(t);
      }
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (grp == 0) {
    for (int g = 1; g < ngrp; ++g) {
      const float4 v = part[g * EQ + q];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (row < p.V) *(float4*)(p.dword + (size_t)row * E + 4 * q) = s;
    else if (row - p.V < P) *(float4*)(p.dpos + (size_t)(row - p.V) * E + 4 * q) = s;
  }
}
}  // namespace
extern "C" int plb_launch_embed_scatter(const PlbEmbed* p, int P, hipStream_t stream) {
  if ((p->E != 64 && p->E != 128 && p->E != 256) || p->T <= 0) return 1;
  ProfScope ps(PLB_K_EMBED_BWD, stream, 0, (double)p->T * p->E * 8.0);
  if (p->row_start && (!p->lengths || p->B < 1)) return 1;
  const int Tscan = p->row_start ? p->B * p->S : p->T;   // packed: the padded ids are what is scanned
  const int chunk = Tscan < EMB_CHUNK ? Tscan : EMB_CHUNK;
  const size_t lds_bytes = (size_t)(((chunk + 3) / 4 + 64) * 4) * 4;
  if (p->row_start) hipLaunchKernelGGL(embed_scatter_kernel<true>, dim3(p->V + P), dim3(256), lds_bytes, stream, *p, P);
  else hipLaunchKernelGGL(embed_scatter_kernel<false>, dim3(p->V + P), dim3(256), lds_bytes, stream, *p, P);
  return LAUNCH_OK();
}
