// The launch plan of the NT GEMM family (gemm_nt_plan.h) and the tuning state it reads. Plain C++: no HIP, no device code.
#include "gemm_nt_plan.h"

#include <stdlib.h>
#include <string.h>

// 0: pick per shape; 128 / 256 / 384 / 1256: force that tile where the shape allows; 64 / -64: per-shape choice of the
// kernel, and every / no launch of the small kernel in its 64x64 form
static int g_nt_tile = 0;
extern "C" void plb_set_gemm_nt_tile(int tile) { g_nt_tile = tile; }

// K-loop form of the pipeline kernel: 1 interleaved (reads / DMA issues in the MFMA shadows), 0 staggered two-barrier loop,
// -1 (default) per tile: measured on 16384 x {768, 2048, 2304} x {768, 2048, 2304}, interleaved wins by
// 5-8 % on 128x384 and 128x256, staggered by 5-10 % on a plain 256x256 launch (whose phase 3 has nothing to
// interleave and phase 4 twelve reads) — but with the GELU epilogues (the only 256x256 launches of the model:
// 16384 x 2048 x 768) interleaved wins again by 6 %: 68.7 vs 72.8 us forward, 70.0 vs 74.7 us backward.
// Only the bf16 forms 0 - 4 and 9 are built in both loop forms; every other form is interleaved.
static int g_nt_prefetch = -1;
extern "C" void plb_set_gemm_nt_prefetch(int on) { g_nt_prefetch = on; }

// PLBERT_NT_SMALL_TILE = 128 | 64 (read once per process): every launch of the small kernel takes that form whatever
// small_tile's rule says, so one library can be compared with itself. The setter's 64 / -64 / 128 go before it.
static int nt_small_tile_env() {
  static const int v = [] {
    const char* e = getenv("PLBERT_NT_SMALL_TILE");
    const int n = e ? atoi(e) : 0;
    return (n == 64 || n == 128) ? n : 0;
  }();
  return v;
}
// Form of a launch that goes to the small kernel. The 128x128 grid of the compact rows of a pruned last application
// (~2,000 rows: 96 workgroups at N 768 and 2048), of the phoneme head (32) and of the map-in's dE product (128) leaves
// most of the 256 CUs idle while every workgroup walks its whole K chain at ~0.8 us per K-tile; the 64x64 form puts four
// times the workgroups on the chip and halves the cost of a K-tile. Measured per shape class, kept where every run of
// the 64 form was below every run of the 128 form: profiles/nt_small_tile_kernel_ab.txt.
static int small_tile(int M, int N) {
  if (g_nt_tile == 64) return 64;
  if (g_nt_tile == -64 || g_nt_tile == 128) return 128;
  if (nt_small_tile_env()) return nt_small_tile_env();
  const long grid128 = (long)(M / 128) * ((N + 127L) / 128);
  return grid128 < 256 ? 64 : 128;
}

// Tile policy of plb_launch_gemm_nt: fill 256 CUs. efficiency = tiles / (rounds * 256) with one workgroup per CU for the
// big tiles; 128x384 moves 4/3 the operand bytes per flop of 256x256, hence the small handicap. 128: the small kernel.
static int pick_tile(int M, int N) {
  const bool ok256 = M % 256 == 0 && N % 256 == 0, ok384 = M % 128 == 0 && N % 384 == 0;
  const bool ok1256 = M % 128 == 0 && N % 256 == 0;
  if (g_nt_tile == 128) return 128;
  if (g_nt_tile == 256) return ok256 ? 256 : 128;
  if (g_nt_tile == 384) return ok384 ? 384 : (ok256 ? 256 : 128);
  if (g_nt_tile == 1256) return ok1256 ? 1256 : 128;
  // (64 / -64 choose the small kernel's form only: the kernel is picked per shape)
  if ((long)M * N < 256L * 256 * 64) return 128;  // small problems: more, smaller workgroups
  auto eff = [&](bool ok, int tm, int tn, double handicap) {
    if (!ok) return 0.0;
    const long t = (long)(M / tm) * (N / tn);
    return handicap * (double)t / (double)(((t + 255) / 256) * 256);
  };
  const double e256 = eff(ok256, 256, 256, 1.0), e384 = eff(ok384, 128, 384, 0.95), e1256 = eff(ok1256, 128, 256, 0.85);
  if (e256 == 0 && e384 == 0 && e1256 == 0) return 128;
  if (e1256 > e256 && e1256 > e384) return 1256;
  return e384 > e256 ? 384 : 256;
}

namespace {
struct Tile { int code, m, n; };
constexpr Tile kT256 = {256, 256, 256}, kT384 = {384, 128, 384}, kT1256 = {1256, 128, 256}, kNone = {0, 0, 0};
Tile pipeline_tile(int code) { return code == 384 ? kT384 : code == 1256 ? kT1256 : kT256; }

// The pipeline tile of a form whose launcher has a rule of its own (everything but the bf16 forms of plb_launch_gemm_nt),
// kNone with *rc = 3 / 1 where the shape has none; kdepth: elements of a K-tile (64 bf16, 128 fp8).
Tile form_tile(int M, int N, int K, int form, bool fp8, int* rc) {
  const int kdepth = fp8 ? 128 : 64;
  *rc = 3;
  switch (form) {
    case PLB_NT_PLAIN: case PLB_NT_GELU: case PLB_NT_GELUBWD:   // fp8 only: 128x384 for the plain epilogue, else 128x256. 256x256 is
      // not built (128 accumulators + 96 registers of operand tuples do not fit 256 VGPRs)
      if (M % 128 || K % kdepth || M <= 0 || N <= 0 || K <= 0) return kNone;
      return form == PLB_NT_PLAIN && N % 384 == 0 ? kT384 : N % 256 == 0 ? kT1256 : kNone;
    case PLB_NT_CE1: case PLB_NT_CE2:   // 256 columns wide; 256 rows where M allows
      *rc = 1;
      if (fp8 || M % 128 || N % 256 || K % kdepth || M <= 0 || N <= 0 || K <= 0) return kNone;
      return M % 256 == 0 ? kT256 : kT1256;
    case PLB_NT_LNFWD: case PLB_NT_LNBWD: {   // 128-row tiles, a row block of at most 4 column tiles, 8 XCDs x whole row blocks
      if (M % 1024 || K % kdepth || M <= 0 || N <= 0 || K <= 0) return kNone;
      const Tile t = N % 384 == 0 ? kT384 : N % 256 == 0 ? kT1256 : kNone;
      return t.n && N / t.n <= 4 ? t : kNone;
    }
    case PLB_NT_GELUD: case PLB_NT_GELUDBWD:   // bf16: 256x256; fp8: 256x256 where M allows (these launches are epilogue-bound:
      // 2 rounds at 16384 x 2048 instead of 4), else 128x256. Forward and backward of a call pick the same tile from the same M.
      if (M % (fp8 ? 128 : 256) || N % 256 || K % kdepth || M <= 0 || N <= 0 || K <= 0) return kNone;
      return M % 256 == 0 ? kT256 : kT1256;
  }
  *rc = 1;   // (fp32 out has no fp8 form)
  return kNone;
}

int form_class(int form, bool fp8) {
  switch (form) {
    case PLB_NT_GELU: case PLB_NT_GELUD: return fp8 ? PLB_K_GEMM_NT_GELU_FP8 : PLB_K_GEMM_NT_GELU;
    case PLB_NT_GELUBWD: case PLB_NT_GELUDBWD: return fp8 ? PLB_K_GEMM_NT_GELUBWD_FP8 : PLB_K_GEMM_NT_GELUBWD;
    case PLB_NT_CE1: case PLB_NT_CE2: return PLB_K_GEMM_NT_CE;
    case PLB_NT_LNFWD: return fp8 ? PLB_K_GEMM_NT_LNFWD_FP8 : PLB_K_GEMM_NT_LNFWD;
    case PLB_NT_LNBWD: return fp8 ? PLB_K_GEMM_NT_LNBWD_FP8 : PLB_K_GEMM_NT_LNBWD;
    case PLB_NT_F32: return PLB_K_GEMM_NT_F32;
  }
  return fp8 ? PLB_K_GEMM_NT_FP8 : PLB_K_GEMM_NT;
}

// algorithmic HBM bytes of the launch: each operand and each output once
double form_bytes(double M, double N, double K, int form, bool fp8, int opts) {
  const double mn = M * N, ab = (fp8 ? 1.0 : 2.0) * (M * K + N * K);
  const double res = (opts & PLB_NT_RES) ? 2.0 * mn : 0.0, c8 = (fp8 && (opts & PLB_NT_C8)) ? mn : 0.0;
  switch (form) {
    case PLB_NT_CE1: case PLB_NT_CE2: return 0.0;
    case PLB_NT_LNFWD: case PLB_NT_LNBWD: return ab + 4.0 * mn + res + c8;   // pre + LayerNorm output | pre + dx
    case PLB_NT_GELUD: case PLB_NT_GELUDBWD:   // the stash and gelu(u) | the stash and dU; fp8: the second as its images
      return fp8 ? ab + 2.0 * mn + ((opts & PLB_NT_OUT16) ? 2.0 * mn : 0.0) + c8 : ab + 4.0 * mn;
  }
  // u and gelu(u) (1), fp32 (9) or one bf16 output; the backward of gelu reads u
  return ab + mn * (form == PLB_NT_F32 || form == PLB_NT_GELU ? 4 : 2) + res + (form == PLB_NT_GELUBWD ? 2.0 * mn : 0.0) + c8;
}
}  // namespace

extern "C" int plb_gemm_nt_plan(int M, int N, int K, int form, int operands, int opts, int tile, PlbGemmNTPlan* plan) {
  memset(plan, 0, sizeof(*plan));
  const bool fp8 = operands != PLB_NT_BF16;
  const bool nt_form = form == PLB_NT_PLAIN || form == PLB_NT_GELU || form == PLB_NT_GELUBWD || form == PLB_NT_F32;
  const bool wants_colpart = (opts & PLB_NT_COLPART) != 0;
  if (form < PLB_NT_PLAIN || form > PLB_NT_F32 || operands < PLB_NT_BF16 || operands > PLB_NT_FP8_E5M2) return plan->rc = 1;
  Tile t = kNone;
  long grid = 0;
  bool both_loops = false;   // is the form built in the staggered K loop too?
  if (tile) {   // plb_launch_gemm_nt_big: the caller's tile
    t = pipeline_tile(tile);
    const bool ce = form == PLB_NT_CE1 || form == PLB_NT_CE2;
    if (fp8 || !(nt_form || ce) || (ce && t.n != 256)) return plan->rc = 1;
    if (M % t.m || N % t.n || K % 64 || M <= 0 || N <= 0 || K <= 0) return plan->rc = 1;
    both_loops = true;
  } else if (!fp8 && nt_form) {   // plb_launch_gemm_nt: per-shape policy over both kernels
    if (M % 128 || K % 64 || N % 4 || M <= 0 || N <= 0 || K <= 0) return plan->rc = 1;
    const int code = pick_tile(M, N);
    if (code == 128) {
      if (wants_colpart) return plan->rc = 1;   // column-sum partials exist in the pipeline kernel only
      // the small kernel, 128x128 or 64x64 (head, map-in and other small products; some run on the engine's side stream,
      // where a launch can sit behind the main stream's grid for longer than it runs) is a class of its own: "gemm_nt" is
      // the pipeline kernel
      plan->tile = plan->tile_m = plan->tile_n = small_tile(M, N);
      plan->kloop = -1;
      grid = (long)(M / plan->tile) * (((long)N + plan->tile - 1) / plan->tile);
      plan->block = 256;
      plan->cls = form == PLB_NT_F32 ? PLB_K_GEMM_NT_F32 : PLB_K_GEMM_NT_SMALL;
    } else {
      t = pipeline_tile(code);
      both_loops = true;
    }
  } else {
    int rc;
    t = form_tile(M, N, K, form, fp8, &rc);
    if (!t.code) return plan->rc = rc;
    both_loops = !fp8 && (form == PLB_NT_CE1 || form == PLB_NT_CE2);
  }
  if (t.code) {
    plan->family = 1;
    plan->tile = t.code; plan->tile_m = t.m; plan->tile_n = t.n;
    const bool plain_256 = t.code == 256 && (form == PLB_NT_PLAIN || form == PLB_NT_F32);
    plan->kloop = !both_loops ? 1 : g_nt_prefetch < 0 ? !plain_256 : g_nt_prefetch != 0;
    grid = (long)(M / t.m) * (N / t.n);
    plan->block = 512;
    plan->cls = form_class(form, fp8);
    // 2 partial rows per row tile (one per wave half); the LayerNorm backward always writes its dgamma | dbeta | sums rows
    if (form == PLB_NT_LNBWD || (wants_colpart && form != PLB_NT_LNFWD)) plan->colpart_rows = 2 * (M / t.m);
  }
  if (grid > 0x7fffffffL) {   // (more workgroups than a launch's grid holds)
    memset(plan, 0, sizeof(*plan));
    return plan->rc = 1;
  }
  plan->grid = (int)grid;
  plan->flops = 2.0 * (double)M * N * K;
  plan->bytes = form_bytes(M, N, K, form, fp8, opts);
  return 0;
}

extern "C" int plb_gemm_nt_colpart_rows(int M, int N, int K) {
  PlbGemmNTPlan pl;
  return plb_gemm_nt_plan(M, N, K, PLB_NT_PLAIN, PLB_NT_BF16, PLB_NT_COLPART, 0, &pl) ? 0 : pl.colpart_rows;
}
extern "C" int plb_gemm_nt_fp8_gelud_tile_rows(int M) {   // (128 also where M has no form: what callers size a stash by)
  PlbGemmNTPlan pl;
  return plb_gemm_nt_plan(M, 256, 128, PLB_NT_GELUD, PLB_NT_FP8_E4M3, 0, 0, &pl) ? 128 : pl.tile_m;
}
