// The launch plan of the token-major weight-gradient GEMMs (gemm_tn_plan.h) and the two knobs it reads. Plain C++: no HIP,
// no device code.
#include "gemm_tn_plan.h"

#include <stdlib.h>
#include <string.h>

// PLBERT_TN_SPLITS=xcd restores round 1's rule (8 * s splits, s * tiles <= 32: whole splits per XCD, but only 192-216
// of the 256 CUs busy on the model's shapes); default: as many splits as fit one workgroup per CU.
static bool tn_fill_chip() {
  static const bool v = [] { const char* e = getenv("PLBERT_TN_SPLITS"); return !(e && !strcmp(e, "xcd")); }();
  return v;
}
// PLBERT_TN_CUS = n (64..256, default 256): workgroups a big weight-gradient GEMM may occupy. The tail of the backward is
// where the gradient pieces travel; RCCL's kernels need CUs of their own and the one-workgroup-per-CU grids leave 4-16
// (dense.weight: 4). Lowering n trades GEMM width for CUs the collective finds free — a knob for the first real N > 1 run
// (bench.py reports the tail's GEMM time with and without the exchange), read once per process.
static int tn_cus() {
  static const int v = [] {
    const char* e = getenv("PLBERT_TN_CUS");
    const int n = e ? atoi(e) : 256;
    return (n >= 64 && n <= 256) ? n : 256;
  }();
  return v;
}

extern "C" int plb_gemm_tn_plan(int64_t Mtot, int Ncols, int N, int K, int operands, PlbGemmTNPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  const bool fp8 = operands == PLB_TN_FP8;
  if (operands != PLB_TN_BF16 && !fp8) return plan->rc = 1;
  // every kernel walks whole K-tiles of 64 token rows and takes its sizes as int
  if (Mtot <= 0 || Mtot > 0x7fffffffLL - 127 || Mtot % 64 || N <= 0 || K <= 0 || N > Ncols) return plan->rc = 1;
  // The 256x256 pipeline kernels read whole tiles: 256-column multiples, every column of A stored; below 8192 rows the K
  // loop is too short to pay for them. The fp8 kernel has no 128x128 form: its K-tile is 128 rows, and its images exist for
  // the layer weights only. (The engine takes the images where the bf16 plan of the shape is the pipeline kernel AND this
  // one accepts it; a call whose last application was pruned may then hand the fp8 kernel fewer than 8192 rows, and those
  // get the split count of the small rule.)
  const bool fits_pipeline = N == Ncols && Ncols % 256 == 0 && K % 256 == 0;
  const bool big = fits_pipeline && Mtot >= 8192;
  if (fp8 ? (!fits_pipeline || Mtot % 128) : (!big && K % 4)) return plan->rc = 1;
  plan->kernel = fp8 ? PLB_TN_PIPELINE_FP8 : big ? PLB_TN_PIPELINE : PLB_TN_SMALL;

  // Row splits. The small kernel: 128x128 tiles at ~3 workgroups per CU (768 / tiles). The pipeline kernels: one workgroup
  // per CU (128 KiB of LDS each), tiles * splits <= 256 and as close to it as the tile count allows — 24 tiles (the two FFN
  // weights) -> 10 splits = 240 workgroups, 27 (QKV) -> 9 = 243, 9 (dense) -> 28 = 252. The kernel deals the (split, tile)
  // pairs to the XCDs in contiguous runs (xcd_remap), so an XCD still streams a contiguous range of token rows through its
  // L2 (a split may straddle two XCDs). A wide output (token head: tiles >= 256) needs no row splits.
  const int64_t tiles128 = (((int64_t)N + 127) / 128) * (((int64_t)K + 127) / 128), tiles256 = (int64_t)(N / 256) * (K / 256);
  const int64_t tiles = big ? tiles256 : tiles128;
  int64_t splits = 768 / tiles;
  if (big) {
    const int64_t s = 32 / tiles > 0 ? 32 / tiles : 1;
    splits = tiles >= 256 ? 1 : tn_fill_chip() ? (tn_cus() / tiles > 0 ? tn_cus() / tiles : 1) : 8 * s;
  }
  if (splits > Mtot / 64) splits = Mtot / 64;
  if (splits < 1) splits = 1;
  int64_t rps = ((Mtot + splits - 1) / splits + 63) / 64 * 64;
  if (fp8) rps = (rps + 127) / 128 * 128;   // K-tiles of 128 tokens
  splits = (Mtot + rps - 1) / rps;

  const int64_t grid_x = plan->kernel == PLB_TN_SMALL ? tiles128 : tiles256 * splits;
  const int64_t nk = (int64_t)N * K;
  if (grid_x > 0x7fffffffLL || nk > 0x7fffffffffffffffLL / splits) {   // (more than a launch's grid or an int64 holds)
    memset(plan, 0, sizeof(*plan));
    return plan->rc = 1;
  }
  plan->splits = (int)splits;
  plan->rows_per_split = (int)rps;
  plan->direct = splits == 1 && N == Ncols;   // every element is written exactly once
  plan->grid_x = (int)grid_x;
  plan->grid_y = plan->kernel == PLB_TN_SMALL ? (int)splits : 1;
  plan->block = plan->kernel == PLB_TN_SMALL ? 256 : 512;
  plan->slab_floats = plan->direct ? 0 : splits * nk;
  plan->flops = 2.0 * (double)Mtot * N * K;
  return 0;
}
