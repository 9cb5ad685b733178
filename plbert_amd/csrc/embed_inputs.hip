// Embeddings with per-token sources, gfx950: the row kernel of embed.hip with token_type_ids, position_ids and inputs_embeds,
// and the table gradients those sources need.
// AlbertEmbeddings.forward (modeling_albert.py:67-106) with dropout 0:
//   LN_E((inputs_embeds[b,s] | word[ids[b,s]]) + type[token_type_ids[b,s]] + pos[position_ids[b,s]]); E <= 256.
// One wave per token, 16-byte table reads, wave-shuffle reductions, fp32 statistics; the arithmetic of a row, and its order,
// is embed_kernel's, so a call that passes token_type_ids = 0 and position_ids = s explicitly computes what the plain call
// computes, bit for bit. No atomics anywhere: every sum has a fixed order. Token-packed calls find a row's token through
// packed_locate; the per-token sources are read at the token's padded [B,S] index, like the ids.
// The plain kernels of embed.hip keep serving every call that passes none of the sources.
#include "common.h"
#include "plbert_kernels.h"
#include "row_common.h"

namespace {
// the per-token sources of one launch (device pointers; the launchers fill it from PlbEmbedIn)
struct EmbedSrc {
  const int64_t* tt; const int64_t* pid; const float* xe; const float* type; int NTY, P;
};

DEVI int table_row(const int64_t* keys, int i, int fallback, int rows) {
  long long k = keys ? keys[i] : fallback;
  if (k < 0 || k >= rows) k = 0;  // host validates; never index out of the table
  return (int)k;
}

template <bool BWD>
__global__ __launch_bounds__(256) void embed_inputs_kernel(PlbEmbed p, EmbedSrc x) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = p.E;
  const int c = lane * 4;  // this lane's 4 columns
  const bool act = c < E;
  float4 g4 = make_float4(0, 0, 0, 0), b4 = g4;
  if (act) {
    g4 = *(const float4*)(p.gamma + c);
    b4 = *(const float4*)(p.beta + c);
  }
  float dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};
  const float invE = 1.0f / (float)E;
  for (int t = blockIdx.x * 4 + wave; t < p.T; t += gridDim.x * 4) {
    int src = t, s = 0;
    if (p.row_start) {   // packed row t -> token (b, s) of the padded inputs (wave-uniform: one row per wave)
      int b;
      const bool owned = packed_locate(p.row_start, p.lengths, p.B, p.S, t, &b, &s);
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
    const int ti = table_row(x.tt, src, 0, x.NTY), pi = table_row(x.pid, src, s, x.P);
    float v[4] = {0, 0, 0, 0};
    if (act) {
      float4 w;
      if (x.xe) w = *(const float4*)(x.xe + (size_t)src * E + c);
      else w = *(const float4*)(p.word + (size_t)table_row(p.ids, src, 0, p.V) * E + c);
      const float4 ty = *(const float4*)(x.type + (size_t)ti * E + c);
      const float4 ps = *(const float4*)(p.pos + (size_t)pi * E + c);
      v[0] = w.x + ty.x + ps.x; v[1] = w.y + ty.y + ps.y; v[2] = w.z + ty.z + ps.z; v[3] = w.w + ty.w + ps.w;
    }
    const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * invE;
    float d[4], vs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = act ? v[j] - mean : 0.f; vs += d[j] * d[j]; }
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
      if (act)  // gradient of the pre-LayerNorm sum: the table sums and d_inputs_embeds read it
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

// Rows of a table keyed by a per-token index (position_ids, token_type_ids). One row may own every token of the call (a
// token type; a position when all ids are equal), so no row is one workgroup's: the padded token range is cut into chunks of
// KEY_CHUNK tokens, and workgroup (row, chunk) sums the dx rows of the chunk's tokens that carry the row's key. Each wave scans
// its own quarter of the chunk and appends the matches to its own list segment, so the four segments in wave order are the
// matches in token order; the row groups then sum them at a fixed stride and are added in group order. Partial row
// (chunk, row) is written by every workgroup — zeros where the chunk holds no such token — and plb_launch_reduce_slabs adds the
// chunks in order. Rows [0, nPos) are position rows, the rest token-type rows.
// PACKED: the keys are walked in the padded [B,S] order, so the order of every sum is the padded call's; only the row of dx a
// token is read from comes from the plan, and pad positions are left out.
constexpr int KEY_CHUNK = 512;
template <bool PACKED>
__global__ __launch_bounds__(256) void embed_key_rows_kernel(PlbEmbed p, EmbedSrc x, int nPos, int nTy, float* part_pos,
                                                             float* part_type) {
  __shared__ int list[4][KEY_CHUNK / 4];
  __shared__ int wcnt[4];
  __shared__ float4 part[256];
  const int E = p.E, T = PACKED ? p.B * p.S : p.T;
  const int chunk = blockIdx.y;
  const bool is_pos = (int)blockIdx.x < nPos;
  const int key = is_pos ? blockIdx.x : blockIdx.x - nPos;
  const int64_t* keys = is_pos ? x.pid : x.tt;
  const int rows = is_pos ? x.P : x.NTY;
  const int EQ = E >> 2;                                   // float4 columns per row
  const int q = threadIdx.x % EQ, grp = threadIdx.x / EQ, ngrp = 256 / EQ;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c1 = (chunk + 1) * KEY_CHUNK < T ? (chunk + 1) * KEY_CHUNK : T;
  int cnt = 0;
#pragma unroll
  for (int piece = 0; piece < KEY_CHUNK / 256; ++piece) {
    const int t = chunk * KEY_CHUNK + w * (KEY_CHUNK / 4) + piece * 64 + lane;
    bool hit = false;
    int trow = t;   // the row of dx that holds token t
    if (t < c1) {
      hit = table_row(keys, t, 0, rows) == key;
      if (PACKED) {
        const int b = t / p.S, sp = t - b * p.S;
        hit = hit && sp < clamp_len(p.lengths[b], p.S);
        trow = p.row_start[b] + sp;
      }
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    if (hit) list[w][cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = trow;
    cnt += __builtin_popcountll(m);
  }
  if (lane == 0) wcnt[w] = cnt;
  __syncthreads();
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ww = 0; ww < 4; ++ww) {
    const int n = wcnt[ww];
    const int* l = list[ww];
    int i = grp;
    for (; i + 3 * ngrp < n; i += 4 * ngrp) {   // 4 loads in flight per row group
      const float4 v0 = *(const float4*)(p.dx + (size_t)l[i] * E + 4 * q), v1 = *(const float4*)(p.dx + (size_t)l[i + ngrp] * E + 4 * q);
      const float4 v2 = *(const float4*)(p.dx + (size_t)l[i + 2 * ngrp] * E + 4 * q), v3 = *(const float4*)(p.dx + (size_t)l[i + 3 * ngrp] * E + 4 * q);
      s.x += (v0.x + v1.x) + (v2.x + v3.x); s.y += (v0.y + v1.y) + (v2.y + v3.y);
      s.z += (v0.z + v1.z) + (v2.z + v3.z); s.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; i < n; i += ngrp) {
      const float4 v = *(const float4*)(p.dx + (size_t)l[i] * E + 4 * q);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (grp == 0) {
    for (int g = 1; g < ngrp; ++g) {
      const float4 v = part[g * EQ + q];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float* dst = is_pos ? part_pos + ((size_t)chunk * nPos + key) * E : part_type + ((size_t)chunk * nTy + key) * E;
    *(float4*)(dst + 4 * q) = s;
  }
}

int key_chunks(int tokens) { return (tokens + KEY_CHUNK - 1) / KEY_CHUNK; }

// what every launcher checks; the per-token sources as the kernels take them
int sources(const PlbEmbedIn* x, EmbedSrc* out) {
  if (!x || !x->base) return 1;
  const PlbEmbed* p = x->base;
  if (p->E % 4 || p->E > 256 || p->T <= 0 || p->S < 1) return 1;
  if (p->row_start && (!p->lengths || p->B < 1)) return 1;
  if ((p->ids != nullptr) == (x->inputs_embeds != nullptr)) return 1;   // exactly one of the two
  if (x->NTY < 1 || x->P < 1 || !p->type0 || !p->pos) return 1;
  *out = EmbedSrc{x->token_type_ids, x->position_ids, x->inputs_embeds, p->type0, x->NTY, x->P};
  return 0;
}
}  // namespace

extern "C" size_t plb_embed_inputs_part_floats(int tokens, int P, int NTY, int E) {
  if (tokens < 1 || P < 1 || NTY < 1 || E < 1) return 0;
  return (size_t)key_chunks(tokens) * (size_t)(P + NTY) * (size_t)E;
}

extern "C" int plb_launch_embed_inputs_fwd(const PlbEmbedIn* x, hipStream_t stream) {
  EmbedSrc src;
  if (sources(x, &src)) return 1;
  const PlbEmbed* p = x->base;
  int blocks = (p->T + 3) / 4; if (blocks > 2048) blocks = 2048;
  ProfScope ps(PLB_K_EMBED_FWD, stream, 0, (double)p->T * (24 + 2.0 * p->E + (x->inputs_embeds ? 4.0 * p->E : 0.0)));
  hipLaunchKernelGGL((embed_inputs_kernel<false>), dim3(blocks), dim3(256), 0, stream, *p, src);
  return LAUNCH_OK();
}

extern "C" int plb_launch_embed_inputs_bwd(const PlbEmbedIn* x, hipStream_t stream) {
  EmbedSrc src;
  if (sources(x, &src) || x->base->nblocks <= 0) return 1;
  const PlbEmbed* p = x->base;
  {
    ProfScope ps(PLB_K_EMBED_BWD, stream, 0, (double)p->T * (24 + 2.0 * p->E + 8.0 * p->E));
    hipLaunchKernelGGL((embed_inputs_kernel<true>), dim3(p->nblocks), dim3(256), 0, stream, *p, src);
    if (hipGetLastError() != hipSuccess) return 2;
  }
  if (!x->d_inputs_embeds) return 0;
  // dx in the caller's padded layout, every element written once, zeros at the pad positions
  if (p->lengths) {
    if (p->B < 1) return 1;
    return plb_launch_unpack_rows(p->dx, 0, p->E, p->row_start, p->lengths, p->B, p->S, p->E, x->d_inputs_embeds, stream);
  }
  return hipMemcpyAsync(x->d_inputs_embeds, p->dx, (size_t)p->T * p->E * 4, hipMemcpyDeviceToDevice, stream) == hipSuccess ? 0 : 2;
}

extern "C" int plb_launch_embed_inputs_scatter(const PlbEmbedIn* x, hipStream_t stream) {
  EmbedSrc src;
  if (sources(x, &src)) return 1;
  const PlbEmbed* p = x->base;
  const int E = p->E;
  if ((E != 64 && E != 128 && E != 256) || !p->dx || !p->dword || !p->dpos || !x->dtype_rows || !x->chunk_part) return 1;
  // word rows — and the position rows of a call without position_ids (a strided sum over the batch) — as in a plain call
  if (p->ids) {
    if (int rc = plb_launch_embed_scatter(p, x->position_ids ? 0 : x->P, stream)) return rc;
  } else {
    if (hipMemsetAsync(p->dword, 0, (size_t)p->V * E * 4, stream) != hipSuccess) return 2;
    if (!x->position_ids) {
      PlbEmbed rows_only = *p;
      rows_only.V = 0;
      if (int rc = plb_launch_embed_scatter(&rows_only, x->P, stream)) return rc;
    }
  }
  const int nPos = x->position_ids ? x->P : 0, nTy = x->token_type_ids ? x->NTY : 0;
  const int tokens = p->row_start ? p->B * p->S : p->T;   // packed: the padded positions are what is scanned
  const int nc = key_chunks(tokens);
  float* const part_pos = x->chunk_part;
  float* const part_type = x->chunk_part + (size_t)nc * nPos * E;
  if (nPos + nTy > 0) {
    ProfScope ps(PLB_K_EMBED_BWD, stream, 0, (double)p->T * E * 4.0 * (nPos && nTy ? 2 : 1) + (double)nc * (nPos + nTy) * E * 4.0);
    const dim3 grid(nPos + nTy, nc);
    if (p->row_start) hipLaunchKernelGGL(embed_key_rows_kernel<true>, grid, dim3(256), 0, stream, *p, src, nPos, nTy, part_pos, part_type);
    else hipLaunchKernelGGL(embed_key_rows_kernel<false>, grid, dim3(256), 0, stream, *p, src, nPos, nTy, part_pos, part_type);
    if (hipGetLastError() != hipSuccess) return 2;
  }
  if (nPos)
    if (int rc = plb_launch_reduce_slabs(part_pos, nc, (size_t)nPos * E, p->dpos, 0, stream)) return rc;
  if (nTy) return plb_launch_reduce_slabs(part_type, nc, (size_t)nTy * E, x->dtype_rows, 0, stream);
  // no token_type_ids: row 0 receives every token's gradient = the column sums of dpos, the other rows none
  if (hipMemsetAsync(x->dtype_rows, 0, (size_t)x->NTY * E * 4, stream) != hipSuccess) return 2;
  return plb_launch_colsum(p->dpos, 0, (size_t)x->P, E, E, x->dtype_rows, E, 0, x->chunk_part, 1, stream);
}
