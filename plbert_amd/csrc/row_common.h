// What the row-kernel units (embed / layernorm / reduce / loss_rows / optim / operand_images .hip) share beside common.h:
// the token-packed row lookup, the 8 x bf16 <-> fp32 register forms, and the launchers' profiling bracket and status.
#pragma once
#include "common.h"
#include "plbert_kernels.h"

// A sample's length as every kernel reads it: clamped to [1, S].
DEVI int clamp_len(int len, int S) { return len < 1 ? 1 : (len > S ? S : len); }

// Token-packed rows (PlbEmbed.row_start / PlbAttn.row_start): the sample that owns packed row r and r's position in it.
// Returns false for a row that belongs to no sample (behind a sample's length inside its slot, or behind row_start[B]).
DEVI bool packed_locate(const int32_t* row_start, const int32_t* lengths, int B, int S, int r, int* b_out, int* s_out) {
  int lo = 0, hi = B;   // the last b with row_start[b] <= r (row_start is non-decreasing, row_start[0] = 0)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (row_start[mid] <= r) lo = mid; else hi = mid;
  }
  const int len = clamp_len(lengths[lo], S);
  *b_out = lo; *s_out = r - row_start[lo];
  return *s_out < len;
}

DEVI void unpack8(const uint4& u, float (&f)[8]) {
  f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
  f[4] = bf_lo(u.z); f[5] = bf_hi(u.z); f[6] = bf_lo(u.w); f[7] = bf_hi(u.w);
}
DEVI uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? 0 : 2)
namespace {
struct ProfScope {  // brackets every launch made while it is alive with one pair of HIP events
  int tok; hipStream_t s;
  ProfScope(int cls, hipStream_t st, double flops, double bytes) : tok(plb_prof_begin(cls, st, flops, bytes)), s(st) {}
  ~ProfScope() { plb_prof_end(tok, s); }
};
}  // namespace
