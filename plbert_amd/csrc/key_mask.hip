// Key masks for the attention kernels (PlbAttn.key_words), gfx950: a [B,S] int32 mask becomes one bit per key.
//  Bit j & 31 of word j >> 5 of a sample's row is key j; bits at or past the sample's length are clear, so the words alone
//  say which keys a tile holds. The row stride is 2 * ceil(S / 64) words (or more): every 64-key tile of the attention
//  kernels owns two whole words and a tile read never leaves its row.
#include "row_common.h"

namespace {

// One wave = one 64-key tile of one sample: lane i tests key 64 t + i, the ballot is the tile's two words, lane 0 stores them.
__global__ __launch_bounds__(256) void key_mask_words_kernel(const int32_t* mask, const int32_t* lengths, int S, int tiles,
                                                             int total, uint32_t* words, int ldkw) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);   // (wave-uniform)
  if (item >= total) return;
  const int b = item / tiles, t = item - b * tiles;
  const int len = clamp_len(lengths ? lengths[b] : S, S);
  const int j = t * 64 + lane;
  const bool on = j < len && mask[(size_t)b * S + j] != 0;   // (j < len <= S: the mask is not read past its row)
  const unsigned long long bits = __builtin_amdgcn_ballot_w64(on);
  if (lane == 0) {
    uint32_t* w = words + (size_t)b * ldkw + 2 * t;
    w[0] = (uint32_t)bits;
    w[1] = (uint32_t)(bits >> 32);
  }
}

}  // namespace

extern "C" int plb_launch_key_mask_words(const int32_t* mask, const int32_t* lengths, int B, int S, uint32_t* words, int ldkw,
                                         hipStream_t stream) {
  if (!mask || !words || B < 1 || S < 1) return 1;
  const int tiles = (S + 63) / 64;
  if (ldkw < 2 * tiles) return 1;
  const int64_t total = (int64_t)B * tiles;
  if (total >= ((int64_t)1 << 31)) return 1;
  ProfScope ps(PLB_K_ROWS, stream, 0, (double)B * S * 4.0 + (double)total * 8.0);
  hipLaunchKernelGGL(key_mask_words_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, mask, lengths, S, tiles,
                     (int)total, words, ldkw);
  return LAUNCH_OK();
}
