// Internal launch interface between the HIP kernel files and the C-ABI engine (engine.cpp).
// Not installed; the public boundary is include/plbert.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plbert.h"   // PLB_NPARAM, PlbAdamWSegment (the segmented optimizer launches)
#include "gemm_tn_plan.h"            // PlbGemmTNPlan: kernel, row splits and slab need of a token-major weight-gradient GEMM
#include "gemm_nt_plan.h"            // PlbGemmNTPlan and the form / operand / option names of the NT GEMM launchers (+ prof_classes.h)
#include "attn_plan.h"               // PlbAttnPlan: grid, kernel variant, backward form and partial rows of the attention launches

typedef uint16_t bf16_t;

extern "C" {

// ---- per-launch HIP-event profiler (engine_prof.cpp; the classes: PlbKernelClass in prof_classes.h). Off by default: begin()
// then returns -1 at once.
int plb_prof_begin(int cls, hipStream_t s, double flops, double bytes);
void plb_prof_end(int tok, hipStream_t s);

// C[M,N] = A[M,K]·B[N,K]^T (+bias)(+res); M%128==0, K%64==0, N%4==0, B readable for ceil128(N) rows.
typedef struct {
  const bf16_t* A; int lda;
  const bf16_t* B; int ldb;
  int M, N, K;
  int Mstore;                   // rows >= Mstore are computed but not stored
  const float* bias;            // [N] or null
  const bf16_t* res; int ldr;   // residual [M,N] or null
  const bf16_t* aux; int ldaux; // act==2: pre-activation u
  bf16_t* C; int ldc;           // bf16 out (act==1: pre-activation u)
  bf16_t* C2; int ldc2;         // act==1: gelu_new(u)
  float* Cf; int ldcf;          // out_f32
  float* colpart;               // big-tile kernels only, or null: [2*M/TM][N] partial column sums of the output
  // fused GEMM + cross-entropy over a wide vocabulary (big-tile kernels, 256-column tiles; act 3 and 4):
  int ce_cols;                  // real classes: columns >= ce_cols are padding
  const int64_t* ce_tgt;        // [M] target class of each row
  float* ce_pmax; float* ce_psum;  // act 3 out: [M][N/256] per-tile row maximum / sum of exp(logit - maximum)
  float* ce_tlogit;             // act 3 out: [M] logit of the target class
  const float* ce_lse;          // act 4 in: [M] log-sum-exp of the row
  const float* ce_w;            // act 4 in: [M] row weight (0 on rows without loss)
  // A row of weight 0 (a pad position, the rest of a packed slot, a row >= B*S) may hold anything: its target may be any
  // int64 (pass 1 writes ce_tlogit[row] only when the target, converted to int, names one of the N columns; nothing reads
  // that entry), its row of A may be stale, infinite or NaN, and act 4 still SELECTS exact zeros for its whole gradient
  // row: nothing of it reaches another row or colpart.
  // fp8 operand mode (plb_launch_gemm_nt_fp8, gemm_fp8.hip): A and B are 1-byte images (lda / ldb / K count elements)
  const float* deq_a; const float* deq_b;  // device scalars: 1 / scale of each operand
  uint8_t* C8; int ldc8;        // optional fp8 copy of the output that feeds the next fp8 GEMM (act 1: of C2 = gelu; else of C)
  const float* q_scale;         // device scalar: C8 = saturate(value * q_scale[0])
  float* q_amax;                // device scalar: atomic max of |value| over the launch (next step's scale)
  int c8_bf8;                   // C8 format: 0 e4m3, 1 e5m2
  // LayerNorm fused into the epilogue (plb_launch_gemm_nt_ln, gemm_ln.hip; N = the normalised width, a row spans the
  // N / TN column tiles of its row block, which exchange their row partials in global memory inside the launch):
  const float* ln_gamma; const float* ln_beta;  // [N]
  float* ln_mean; float* ln_rstd;               // [M]: written by the forward form, read by the backward form
  float ln_eps;
  unsigned long long* ln_xchg;  // [(M/128)][N/TN producer][N/TN consumer][128 rows][2] tagged granules; zero before and after every launch
  unsigned int* ln_err;         // incremented when a hand-off timed out (results of that launch are then invalid)
  int ln_fault;                 // fault injection (plb_debug_ln_fault; tests only, 0 in every product launch): 1 = the last
                                // column tile of every row block does not publish its partials (its partners time out),
                                // 2 = column tile 0 reports a time-out and leaves the granules it consumed TAGGED (what a
                                // producer's store landing after the time-out looks like to the next launch)
} PlbGemmNT;
// ---- NT GEMM launchers. Each is: plan (gemm_nt_plan.h: kernel, tile, grid, K-loop form, profiler class, partial rows from
// M, N, K, the form and the operand kind) -> argument check of the descriptor's pointers -> profiler scope -> the
// instantiation the plan names. Return codes: 0 launched; 3 the shape has no form here (the caller takes its other path),
// reported before 1, a refused argument; 2 the launch failed. No profiler scope is open behind a refusal.
// The plan itself, for tests, tools and the engine (which sizes and indexes its buffers from it); declared in gemm_nt_plan.h:
int plb_gemm_nt_plan(int M, int N, int K, int form, int operands, int opts, int tile, PlbGemmNTPlan* plan);
// LayerNorm in the epilogue of the GEMM that produces its input (pipeline kernel, 128-row tiles, at most 4 column tiles):
//  mode 5, forward:  C = bf16(A·B^T + bias + res) ("pre", kept for the backward), C2 = LayerNorm(C)·gamma + beta,
//                    ln_mean / ln_rstd written
//  mode 6, backward: dy = bf16(A·B^T + res) is the gradient of the LayerNorm's OUTPUT and is never stored; aux = the
//                    forward's pre, ln_mean / ln_rstd read; C = the gradient of the LayerNorm's input;
//                    colpart[plan rows][3][N] = per (row tile, wave half) dgamma | dbeta | column sums of C
// 3: the caller runs the GEMM and the LayerNorm kernel separately. Takes plb_ln_fault_take() even when it then refuses.
int plb_launch_gemm_nt_ln(const PlbGemmNT* p, int mode, hipStream_t stream);
// gelu_new with the DERIVATIVE stashed: forward C = gelu_new'(A·B^T + bias), C2 = gelu_new(..); backward C = (A·B^T) * aux
// (aux = the forward's C; colpart as in plb_launch_gemm_nt). 3: the caller uses act 1 / 2 for forward AND backward.
int plb_launch_gemm_nt_gelud(const PlbGemmNT* p, int backward, hipStream_t stream);
// fp8 (e4m3 weights; e4m3 or e5m2 activations / gradients) form of plb_launch_gemm_nt on the pipeline kernel, act 0 - 2.
// 3: the caller uses the bf16 GEMM.
int plb_launch_gemm_nt_fp8(const PlbGemmNT* p, int act, int a_bf8, hipStream_t stream);
// fp8-operand forms of plb_launch_gemm_nt_ln (modes 5 / 6) and plb_launch_gemm_nt_gelud (gemm_fp8_ln.hip). A / B are 1-byte
// images, deq_a / deq_b their dequantisation factors; C8 (+ q_scale, q_amax, c8_bf8) is the 1-byte image of the output the
// next fp8 GEMMs read — mode 5: of C2, mode 6: of C, gelu forward: of C2 = gelu(u), gelu backward: of C. In the gelu forms the
// bf16 image (C2 / C) may be NULL: only the fp8 image leaves.
int plb_launch_gemm_nt_fp8_ln(const PlbGemmNT* p, int mode, int a_bf8, hipStream_t stream);
int plb_launch_gemm_nt_fp8_gelud(const PlbGemmNT* p, int backward, int a_bf8, hipStream_t stream);
int plb_gemm_nt_fp8_gelud_tile_rows(int M);  // the plan's tile rows of that launcher at this M (128 where M has no form)
int plb_ln_fault_take(void);  // fault injection state shared by the LayerNorm launchers (plb_debug_ln_fault)
// act 0 - 2, bf16 or fp32 out, on the small or the pipeline kernel as the plan's per-shape policy says; colpart on a shape
// that goes to the small kernel: 1
int plb_launch_gemm_nt(const PlbGemmNT* p, int act, int out_f32, hipStream_t stream);
// the pipeline forms behind it (gemm_big.hip) on the caller's tile: 256 / 384 / 1256 = 128x256; act 3 / 4 = the fused GEMM +
// cross-entropy passes. No profiler scope of its own.
int plb_launch_gemm_nt_big(const PlbGemmNT* p, int tile, int act, int out_f32, hipStream_t stream);
int plb_gemm_nt_colpart_rows(int M, int N, int K);  // the plan's colpart rows of a plb_launch_gemm_nt of this shape (0: none)
// Tuning / test hooks (not part of include/plbert.h), state of the plan unit: force a tile (0 = per-shape policy; 128, 256,
// 384, 1256 = 128x256; 64 / -64 = every / no launch of the small kernel in its 64x64 form) or a K-loop form (-1 = per-launch
// policy, 1 interleaved, 0 staggered) for the launches that follow. PLBERT_NT_SMALL_TILE = 128 | 64 (read once per process)
// forces the small kernel's form where the setter does not.
void plb_set_gemm_nt_tile(int tile);
void plb_set_gemm_nt_prefetch(int on);

// ---- TN (token-major weight-gradient) GEMM launchers (gemm_tn.hip, gemm_tn_fp8.hip). They run the splits their caller
// hands them; which kernel a shape gets and with what splits is the plan's, declared in gemm_tn_plan.h:
int plb_gemm_tn_plan(int64_t Mtot, int Ncols, int N, int K, int operands, PlbGemmTNPlan* plan);
// slab[split][N][K] = A[rows,N]^T · B[rows,K] over the split's rows; Mtot%64==0, rows_per_split%64==0,
// Ncols (readable columns of A) %8==0, K%8==0.
typedef struct {
  const bf16_t* A; int lda; int Ncols;
  const bf16_t* B; int ldb;
  int Mtot, N, K;
  int rows_per_split, splits;
  float* slab;
  const float* deq_a; const float* deq_b;  // fp8 form only (plb_launch_gemm_tn_fp8): 1 / scale of the two 1-byte images
} PlbGemmTN;
int plb_launch_gemm_tn(const PlbGemmTN* p, hipStream_t stream);
// fp8 form of plb_launch_gemm_tn_big (gemm_tn_fp8.hip): A = e5m2 image [rows, Ncols], B = e4m3 image [rows, K], lda / ldb in
// bytes (multiples of 16); Ncols % 256 == 0, K % 256 == 0, rows_per_split % 128 == 0, Mtot % 128 == 0
int plb_launch_gemm_tn_fp8(const PlbGemmTN* p, hipStream_t stream);
// 256x256-tile pipeline version: Ncols % 256 == 0, K % 256 == 0 (gemm_tn.hip)
int plb_launch_gemm_tn_big(const PlbGemmTN* p, hipStream_t stream);

// out[n] (+)= sum over splits of slab[s][n]   (n = count of floats)
int plb_launch_reduce_slabs(const float* slab, int splits, size_t n, float* out, int accumulate, hipStream_t stream);

// Embeddings: e = LN_E(word[ids] + type[0] + pos[t % S]) -> bf16 [T,E]
typedef struct {
  const int64_t* ids; int T, S, E, V;
  const float *word, *pos, *type0, *gamma, *beta;
  float eps;
  bf16_t* out; int ldo;
  // backward
  const bf16_t* dout; int lddo;
  float* dx;                    // fp32 [T,E]: gradient of the pre-LayerNorm embedding sum (written by embed_bwd)
  float *dword, *dpos;          // fp32 [V,E], [P,E]: written by embed_scatter (every row, no atomics)
  float* partials;              // [nblocks][2E] : dgamma | dbeta partial sums
  int nblocks;
  // Token-packed rows (row_start != NULL; include/plbert.h PlbPacking): ids stays the padded [B,S] input, T counts PACKED
  // rows and out / dout / dx are indexed by packed row: sample b's position s < lengths[b] is row row_start[b] + s, its
  // position embedding is pos[s]. Rows that belong to no sample (the rest of a sample's 128-aligned slot, the tail behind
  // row_start[B]) are written as zeros by the forward and the backward and add nothing to partials / dword / dpos.
  // fill_slots (forward only): the rest of a sample's slot — positions lengths[b] <= s < min(S, ceil128(lengths[b])) — is
  // embedded from ids like the pad positions of a padded call instead of written as zeros (a token-packed call in fp8 mode:
  // the sites' maxima then see what the padded call on the batch trimmed to its slots sees). Positions at or past S and
  // the tail stay zeros.
  const int32_t* row_start; const int32_t* lengths; int B; int fill_slots;
} PlbEmbed;
int plb_launch_embed_fwd(const PlbEmbed* p, hipStream_t stream);
int plb_launch_embed_bwd(const PlbEmbed* p, hipStream_t stream);  // grid = p->nblocks; writes dx + partials
int plb_launch_embed_scatter(const PlbEmbed* p, int P, hipStream_t stream);  // dx -> dword [V,E], dpos [P,E]

// Embeddings with per-token sources (embed_inputs.hip): e = LN_E((inputs_embeds[b,s] | word[ids[b,s]]) + type[token_type_ids[b,s]]
// + pos[position_ids[b,s]]). base (HOST pointer, read by the launcher) carries everything the plain launchers read: shapes,
// tables (type0 = row 0 of the token-type table), LayerNorm, outputs, the packing plan; base->lengths may be set in a padded call
// too (B with it) — then d_inputs_embeds gets its zeros at the pad positions. Exactly one of base->ids and inputs_embeds is given.
// The three per-token sources are indexed like ids, by the padded [B,S] position, also in a token-packed call. An index outside
// its table reads row 0 (the host validates).
typedef struct {
  const PlbEmbed* base;
  const int64_t* token_type_ids;  // [B,S] or NULL: row 0
  const int64_t* position_ids;    // [B,S] or NULL: s
  const float* inputs_embeds;     // fp32 [B,S,E] or NULL
  int NTY, P;                     // rows of the token-type and of the position table
  // backward
  float* dtype_rows;              // fp32 [NTY,E]: written by embed_inputs_scatter (every row)
  float* d_inputs_embeds;         // fp32 [B,S,E] or NULL: embed_inputs_bwd unpacks dx into it (zeros at pad positions)
  // embed_inputs_scatter: plb_embed_inputs_part_floats(...) floats — the partial rows of the 512-token chunks, summed in chunk order
  float* chunk_part;
} PlbEmbedIn;
int plb_launch_embed_inputs_fwd(const PlbEmbedIn* p, hipStream_t stream);
int plb_launch_embed_inputs_bwd(const PlbEmbedIn* p, hipStream_t stream);  // grid = base->nblocks; dx + partials (+ d_inputs_embeds)
// dx -> dword [V,E] (zeros with inputs_embeds), dpos [P,E], dtype_rows [NTY,E]. Word rows, and position rows without position_ids,
// are summed by plb_launch_embed_scatter's kernel as in a plain call. A row keyed by position_ids / token_type_ids may own every
// token of the call: the padded token range is cut into chunks of 512, workgroup (row, chunk) sums the chunk's tokens of that row
// in token order into a partial row, and the partial rows are added in chunk order. No atomics; fixed order.
int plb_launch_embed_inputs_scatter(const PlbEmbedIn* p, hipStream_t stream);
// floats of chunk_part for a call of `tokens` padded positions (B*S)
size_t plb_embed_inputs_part_floats(int tokens, int P, int NTY, int E);

// LayerNorm over rows of width H (H%4==0, H<=1024): y = LN(x)*g+b ; stats saved for the backward
typedef struct {
  const bf16_t* x; int ldx;
  const float *gamma, *beta; float eps;
  bf16_t* y; int ldy;
  float *mean, *rstd;           // [T]
  int T, H;
  int Tzero;                    // backward: rows T..Tzero-1 of dx are written as zeros
  // backward: dx = LN'(dy); partials[nblocks][3H] = dgamma | dbeta | column sums of dx (as stored)
  const bf16_t* dy; int lddy;
  bf16_t* dx; int lddx;
  float* partials; int nblocks;
  int accumulate;               // backward: add to partials instead of overwriting (the 12 applications of the shared
                                // layer sum into ONE [nblocks][3H] image: launches are ordered, so is the sum)
  // fp8 copy of the output for the fp8 GEMM that consumes it (H = 768 / 1024 kernels only): forward y8 = e4m3(y * s),
  // backward dx8 = e5m2(dx * s); q_amax collects max |value| (the next step's scale); all NULL = off
  uint8_t* out8; int ld8; const float* q_scale; float* q_amax;
} PlbLayerNorm;
// fp8 plumbing (operand_images.hip). An "amax" argument anywhere in this file is one SITE: 64 words on 64-byte lines (common.h:
// F8_SLOTS x F8_STRIDE floats) that the waves of a launch spread their atomic maxima over; plb_launch_fp8_scales reduces
// n consecutive sites. |x| maximum of a bf16 / fp32 buffer into a site (atomic max; zero it first),
// scale update (delayed scaling: scale = fmax / amax, deq = 1 / scale, amax reset), quantisation of a bf16 / fp32 matrix
int plb_launch_amax(const void* x, int is_bf16, size_t rows, int cols, int ld, float* amax, hipStream_t stream);
// group: runs of `group` consecutive sites share one scale (from the largest maximum of the run); 1 = every site its own.
// A group whose maximum is 0 (nothing seen) or +inf keeps its scale, deq and stats; its slots are cleared either way.
int plb_launch_fp8_scales(float* amax, float* scale, float* deq, int n, float fmax, int group, hipStream_t stream);
// the same with a second target for entries [n2, n) (n2 a multiple of group). stats (or null): 8 floats per group — a
// four-call history of the group's maxima (groups from hist_from on take their scale from its largest entry), the number
// of calls whose values exceeded the format's range under the scale they were quantised with, the worst such ratio
int plb_launch_fp8_scales2(float* amax, float* scale, float* deq, int n, float fmax, int group, int n2, float fmax2,
                           float* stats, int hist_from, hipStream_t stream);
int plb_launch_quantize(const void* x, int is_bf16, size_t rows, int cols, int ld, const float* scale, uint8_t* out, int ldo,
                        int bf8, hipStream_t stream);
// the fp8 copies of up to 8 contiguous weight matrices in one launch: dst[i] = e4m3(src[i] * scale[i][0]); amax[i] (a site)
// collects max |src[i]| for the next step's scale (delayed scaling)
int plb_launch_quantize_multi(int n, const void* const* src, const int* is_bf16, const size_t* elements,
                              const float* const* scale, uint8_t* const* dst, float* const* amax, hipStream_t stream);
int plb_launch_ln_fwd(const PlbLayerNorm* p, hipStream_t stream);
int plb_launch_ln_bwd(const PlbLayerNorm* p, hipStream_t stream);

// out[N] (+)= column sums of X[R,N]; is_bf16 selects the element type. scratch: [nsplit][N] floats.
// Only the first Nout (<= N) sums are written to out.
int plb_launch_colsum(const void* X, int is_bf16, size_t R, int N, int ld, float* out, int Nout, int accumulate,
                      float* scratch, int nsplit, hipStream_t stream);

// out[0..Nout) = column sums [col0, col0+Nout) finished from the [nsplit][N] partial rows a plb_launch_colsum left in scratch
int plb_launch_copy_cols(const float* scratch, int nsplit, int N, int col0, int Nout, float* out, hipStream_t stream);

// pooled[b,:] = tanh(W[H,H] · hidden[b*S*H ..] + bias)  (first token of every sample, fp32)
int plb_launch_pooler(const float* hidden, int B, int S, int H, const float* W, const float* bias, float* pooled,
                      hipStream_t stream);

// Attention over the fused qkv buffer [T,3H] (Q | K | V, head h at columns h*64..h*64+63), head_dim 64.
typedef struct {
  const bf16_t* qkv; int ldqkv;
  const int32_t* lengths;       // [B] valid keys per sample, or null (= S)
  int B, S, NH, H;
  float scale;                  // head_dim^-0.5
  bf16_t* ctx; int ldctx;       // [T,H]
  float* lse;                   // [B,NH,S] MINUS the log-sum-exp of the scaled scores, in units of RAW scores (-lse/scale): the backward starts its S accumulators there
  // backward
  const bf16_t* dctx; int lddctx;
  float* delta;                 // [B,NH,S] scratch between the two backward kernels: MINUS rowsum(dO∘O)
  bf16_t* dqkv; int lddqkv;     // [T,3H]
  float* colpart;               // backward, optional: [B * ceil(S/128) * 4][3H] column sums of dqkv per (sample, 128-row tile, wave)
  int colpart_accumulate;       // add to colpart instead of overwriting (sum over the applications of the shared layer)
  // fp8 mode, optional 1-byte images of the outputs for the fp8 GEMMs that consume them (the values as rounded to bf16,
  // times *scale, saturated): forward ctx8 = e4m3(ctx) [T,H]; backward dqkv8 = e5m2(dqkv) [T,3H]. amax: the site (64 words,
  // common.h) that collects max |value| for the next step's scale. dqkv may be NULL when dqkv8 is given.
  uint8_t* ctx8; int ldctx8; const float* ctx_scale; float* ctx_amax;
  uint8_t* dqkv8; int lddqkv8; const float* dqkv_scale; float* dqkv_amax;
  // Compact-query mode (qoff != NULL; two-kernel backward only): the QUERIES of sample b are rows [qoff[b], qoff[b+1]) of
  // `q` (row stride ldq, head h at columns h*64..) — e.g. the masked positions only — while keys and values stay the S rows
  // of qkv. ctx / dctx are then indexed by the compact row ([Nq, H], Nq = nq_total = qoff[B]), lse / delta are [NH][Nq],
  // and dQ goes to dq ([Nq, lddq]; + its e5m2 image dq8 in fp8 mode) instead of dqkv's Q block; dqkv's K and V blocks
  // (and colpart, row (b * ceil(S/128) + q tile) * 4 + wave as always) are written as in the full form.
  const int32_t* qoff; const bf16_t* q; int ldq; int nq_total; bf16_t* dq; int lddq; uint8_t* dq8; int lddq8;
  // Token-packed rows (row_start != NULL, [B] entries, multiples of 128; needs lengths): sample b's tokens are rows
  // row_start[b].. of qkv / ctx / dctx / dqkv instead of b*S.., in a slot of ceil(lengths[b] / 128) * 128 rows. The 128-row
  // tiles of a sample are those of the padded call, so every valid row is computed exactly as there; tiles that start
  // at or past the length return before any barrier (their colpart rows are zeroed unless accumulating) and nothing
  // outside the slot is read or written. lse / delta / colpart keep their (b, S) indexing.
  const int32_t* row_start;
  // Key masks (key_words != NULL; plb_launch_key_mask_words writes them): bit j & 31 of word j >> 5 of row b (row stride
  // ldkw >= 2 * ceil(S / 64) words: every 64-key tile owns two whole words) says whether key j of sample b takes part in the
  // softmax of the sample's queries; bits at or past lengths[b] are clear. A masked key below the length (a hole) stays a
  // query like any other: it has a context row, a statistic and a dQ row; its dK / dV rows are exact zeros. NULL selects
  // the kernels without the mask; a row of all-ones bits below the length gives their results bit for bit. S <= 2048; not
  // with compact queries; the form of the backward: attn_plan.h.
  const uint32_t* key_words; int ldkw;
} PlbAttn;
// the modes of a descriptor as the plan's flags (attn_plan.h: PlbAttnFlags)
static inline int plb_attn_flags(const PlbAttn* p) {
  return (p->row_start ? PLB_ATTN_PACKED : 0) | (p->key_words ? PLB_ATTN_KEYMASK : 0) | (p->qoff ? PLB_ATTN_COMPACT : 0) |
         (p->dqkv ? PLB_ATTN_OUT_ROWS : 0) | (p->dqkv8 ? PLB_ATTN_OUT_IMAGE : 0);
}
// ---- attention launchers. Each is: plan (attn_plan.h: grid, kernel variant, form of the backward, profiler credit) -> one
// argument check -> profiler scope -> launch. Return codes: 0 launched, 1 refused (no profiler scope is open behind a
// refusal), 2 the launch failed. The plan itself, for tests, tools and the engine; declared in attn_plan.h:
int plb_attn_plan(int B, int S, int NH, int flags, PlbAttnPlan* plan);
// The one argument check of the four launchers: 0 when descriptor p can be launched in `direction`, else 1. Runs before any
// HIP call. Every direction: the plan of (B, S, NH, the descriptor's modes) runs, H = NH * 64, qkv and lse are given,
// ldqkv % 8 == 0, S * ldqkv * 2 < 2^32 (the staging's 32-bit byte offsets count from a sample's first row), packed rows
// come with lengths, key-mask words with ldkw >= 2 * ceil(S / 64). Forward and backward: ctx and the row strides in use
// (multiples of 8), an image with its scale, compact queries with q (and a backward with dq or dq8). Backward: dctx, and
// dqkv or dqkv8. The single kernel: S <= 512, no key mask, no compact queries, not rows AND image.
enum PlbAttnDirection { PLB_ATTN_FWD = 0, PLB_ATTN_BWD = 1, PLB_ATTN_BWD_SINGLE = 2, PLB_ATTN_PROBS = 3 };
int plb_attn_args_check(const PlbAttn* p, int direction);
int plb_launch_attn_fwd(const PlbAttn* p, hipStream_t stream);
// The backward in the form the plan names for the call (attn_plan.h: PlbAttnBwdForm and the policy behind it);
// plb_launch_attn_bwd_fused is the single kernel itself (S <= 512; delta is not written).
int plb_launch_attn_bwd(const PlbAttn* p, hipStream_t stream);
int plb_launch_attn_bwd_fused(const PlbAttn* p, hipStream_t stream);
// Test hook of the gradient exchange (tests/test_gpu_comm_fake_rccl.py): the next loss call leaves out its index-th
// all-reduce piece, as a forgotten tensor would; the call must then fail in pieces_done() instead of training on a
// gradient range that was never exchanged.
void plb_debug_skip_piece(int index);
// Test hook of the LayerNorm hand-off (tests/test_gpu_handoff_fault.py): the next `launches` fused LayerNorm launches run
// with PlbGemmNT.ln_fault = mode (see there). The step they belong to must be reported (plb_poll_status / plb_status),
// must not reach the parameters (the AdamW launch skips) and must leave nothing behind once plb_status has reported it.
void plb_debug_ln_fault(int mode, int launches);
void plb_set_attn_bwd_fused(int on);

// Loss rows: row r of the gathered matrix is token rows[r]
int plb_launch_gather_rows(const bf16_t* src, int lds_, const int32_t* rows, int n, int npad, int H, bf16_t* dst,
                           int ldd, hipStream_t stream);
int plb_launch_scatter_rows(const bf16_t* src, int lds_, const int32_t* rows, int n, int H, bf16_t* dst, int ldd,
                            hipStream_t stream);
// From the CSR index lists: rows[j] = b*S + idx, tgt[j] = labels[b,idx], w[j] = 1/(n_b * count)
int plb_launch_ce_prepare(const int32_t* offsets, const int32_t* flat, const int64_t* labels, int B, int S,
                          int32_t* rows, int32_t* tgt, float* w, hipStream_t stream);
// the same for token-packed rows: rows[j] = row_start[b] + idx (labels stay the padded [B,S] input)
int plb_launch_ce_prepare_packed(const int32_t* offsets, const int32_t* flat, const int64_t* labels, int B, int S,
                                 const int32_t* row_start, int32_t* rows, int32_t* tgt, float* w, hipStream_t stream);
// Token-packed rows back to the padded layout: dst[b, s, 0..C) (fp32, [B,S,C] contiguous) = src[row_start[b] + s, 0..C)
// for s < lengths[b], zeros at the pad positions. src is bf16 (src_is_bf16) or fp32 with row stride lds_ elements.
// row_start == NULL: src is in the padded order already (row b*S + s) — the conversion pass of plb_encode, which hands out
// zeros at the pad positions in either layout.
int plb_launch_unpack_rows(const void* src, int src_is_bf16, int lds_, const int32_t* row_start, const int32_t* lengths,
                           int B, int S, int C, float* dst, hipStream_t stream);
// The output gradient of the last application from an upstream fp32 gradient (plb_encode_bwd): every one of the Tp rows of
// dy [Tp,H] is written exactly once — bf16(d_hidden[b,s,:]), rounded to nearest even, on row row_start[b] + s (row_start
// == NULL: b*S + s) for s < lengths[b] (lengths == NULL, padded only: every position), zeros on every other row: pad
// positions, the rest of a 128-row slot, the tail up to Tp. d_hidden (fp32 [B,S,H], 16-byte aligned) is not read at pad
// positions. H a multiple of 4.
int plb_launch_seed_dy(const float* d_hidden, const int32_t* lengths, const int32_t* row_start, int B, int S, int H, int Tp,
                       bf16_t* dy, hipStream_t stream);
// ---- pooler backward (pooler_bwd.hip; include/plbert.h plb_encode_bwd_pooled)
// pooled[b,:] = tanh(W · h[b,:] + bias) with h[b,:] the fp32 image of row rows[b] (rows == NULL: b*S) of hidden (bf16, row
// stride ldh elements, 8-byte aligned, ldh % 4 == 0). From d_pooled fp32 [B,H]: y recomputed with plb_launch_pooler's
// arithmetic (its bits), dpre = d_pooled * (1 - y*y) [B,H], dW[o,i] = sum_b dpre[b,o] h[b,i] [H,H], db[o] = sum_b dpre[b,o]
// [H], dh0[b,i] = sum_o dpre[b,o] W[o,i] [B,H]; b ascending, o ascending within each quarter of the rows and the four quarter
// sums added in order; no atomics: bitwise reproducible. Every element of the four
// outputs is written exactly once. H a multiple of 64; W, dW and d_pooled 16-byte aligned.
int plb_launch_pooler_bwd(const bf16_t* hidden, int ldh, const int32_t* rows, int B, int S, int H, const float* W,
                          const float* bias, const float* d_pooled, float* dpre, float* dW, float* db, float* dh0,
                          hipStream_t stream);
// Behind plb_launch_seed_dy (or the clear that stands for a NULL d_hidden): row rows[b] (rows == NULL: b*S) of dy [*,H] =
// bf16(d_hidden[b,0,:] + dh0[b,:]), one fp32 add and one round to nearest even; d_hidden == NULL (fp32 [B,S,H] otherwise): a
// zero addend. Only these B rows are written. H a multiple of 4; d_hidden and dh0 16-byte, dy 8-byte aligned.
int plb_launch_seed_dy_first_rows(const float* d_hidden, const float* dh0, const int32_t* rows, int B, int S, int H, bf16_t* dy,
                                  hipStream_t stream);
// ---- per-application outputs (layer_outputs.hip; include/plbert.h PlbLayerOutputs, plb_encode_bwd_layers)
// The attention probabilities of one application from what it left behind: out fp32 [B,NH,S,S], out[b,h,i,j] =
// exp(scale * q_i·k_j - LSE_i) for i, j < lengths[b] — qkv as PlbAttn.qkv (bf16 [T,ldqkv], Q | K | V, head h at columns
// h*64.., 16-byte aligned, ldqkv % 8 == 0), lse as PlbAttn.lse ([B,NH,S], MINUS the log-sum-exp in raw-score units, as
// plb_launch_attn_fwd stored it for the same qkv): one pass, no second normalisation. Key columns j >= lengths[b] and query
// rows i >= lengths[b] are exact zeros; every element of out is written exactly once (no memset, no atomics). row_start
// (or NULL; needs lengths): token-packed rows, sample b's position i is row row_start[b] + i; lse and out keep their (b, S)
// indexing. lengths == NULL: S. Any S >= 1; 16-byte stores when S % 4 == 0 and out is 16-byte aligned.
int plb_launch_attn_probs(const bf16_t* qkv, int ldqkv, const float* lse, const int32_t* lengths, const int32_t* row_start,
                          int B, int S, int NH, float scale, float* out, hipStream_t stream);
// The same with key masks (key_words / ldkw as PlbAttn.key_words, or NULL: the launch above): the column of a masked key is
// exact zeros in every row; a masked key below the length keeps its own row (it is a query like any other). Every element
// is still written exactly once.
int plb_launch_attn_probs_masked(const bf16_t* qkv, int ldqkv, const float* lse, const int32_t* lengths, const int32_t* row_start,
                                 const uint32_t* key_words, int ldkw, int B, int S, int NH, float scale, float* out,
                                 hipStream_t stream);
// ---- key masks (key_mask.hip): words [B][ldkw] (ldkw >= 2 * ceil(S / 64)) from mask int32 [B,S] (nonzero = the key takes
// part) and lengths ([B], or NULL: S; clamped to [1, S] as everywhere): bit j & 31 of word j >> 5 = key j, clear at and past
// the length; the words of a row past 2 * ceil(S / 64) are not written. One wave per 64-key tile, one ballot, two stores.
int plb_launch_key_mask_words(const int32_t* mask, const int32_t* lengths, int B, int S, uint32_t* words, int ldkw,
                              hipStream_t stream);
// A caller's fp32 gradient joins a bf16 residual operand: every one of the Tp rows of out [Tp,H] is written exactly once —
// bf16(float(res[r,:]) + g[b,s,:]), rounded to nearest even, on row r = row_start[b] + s (row_start == NULL: b*S + s) for
// s < lengths[b] (lengths == NULL, padded only: every position), res[r,:] unchanged on every other row: pad positions, the
// rest of a 128-row slot, the tail up to Tp. res, out bf16 [Tp,H] (8-byte aligned, distinct or the same buffer); g fp32
// [B,S,H] (16-byte aligned) is not read at pad positions. H a multiple of 4. Shape and argument rules of plb_launch_seed_dy.
int plb_launch_add_row_grad(const bf16_t* res, const float* g, const int32_t* lengths, const int32_t* row_start, int B, int S,
                            int H, int Tp, bf16_t* out, hipStream_t stream);
// per row: loss_rows[j] = w*(lse - z[tgt]); dlogits[j,:] = w*(softmax - onehot) (bf16, zero padded to ldd cols)
int plb_launch_ce_fwd_bwd(const float* logits, int ldl, int V, const int32_t* tgt, const float* w, int n, int npad,
                          float* loss_rows, bf16_t* dlogits, int ldd, hipStream_t stream);
// loss[0] = sum(loss_rows[0..n))  (single block, deterministic order)
int plb_launch_sum_rows(const float* x, int n, float* out, hipStream_t stream);
// Fused token-head CE, between the two GEMM passes: merge the per-tile (max, sum) of every row into lse, the row
// weight 1 / (B * len) (0 on padded positions and rows >= B*S) and the weighted loss row.
int plb_launch_token_ce_combine(const float* pmax, const float* psum, int ntiles, const float* tlogit,
                                const int32_t* lengths, int B, int S, int rows, float* lse, float* w, float* loss_rows,
                                hipStream_t stream);
// The same merge on token-packed rows (row for row the same operations: a valid row's lse / w / loss are bit-equal to the
// padded launch's): row row_start[b] + s, s < lengths[b], gets lse, w = 1 / (B * len_b) and its loss row; every other one of
// the `rows` rows (the rest of a 128-row slot, the tail behind row_start[B]) gets lse = w = loss = 0.
int plb_launch_token_ce_combine_packed(const float* pmax, const float* psum, int ntiles, const float* tlogit,
                                       const int32_t* lengths, const int32_t* row_start, int B, int S, int rows, float* lse,
                                       float* w, float* loss_rows, hipStream_t stream);
// Token targets of a packed dual-head call: every one of the `rows` (a multiple of 128) entries of out (int64, 16-byte
// aligned) is written exactly once — token_ids[b,s] on row row_start[b] + s for s < lengths[b], 0 on every other row.
// token_ids ([B,S] int64) is not read at pad positions.
int plb_launch_pack_token_targets(const int64_t* token_ids, const int32_t* lengths, const int32_t* row_start, int B, int S,
                                  int rows, int64_t* out, hipStream_t stream);
int plb_launch_add_scalar(float* out, const float* a, const float* b, hipStream_t stream);

// ---- evaluation rows (eval_rows.hip): what a report on a loss call's masked rows is made of. No atomics, fixed-order sums.
// Per row j < n of logits [n][ldl] (fp32; one wave per row, V <= 256, V % 4 == 0 — ce_kernel's layout; columns >= V are never
// read), with the classes ordered by (logit descending, class index ascending — among equal logits the lowest index wins):
//   pred[j] = the first class; rank[j] = the 0-based position of tgt[j] = #{c : z_c > z_t} + #{c < t : z_c == z_t}, so
//   pred == tgt iff rank == 0 and tgt is in the top-k list iff rank < topk; topk_ids[j][0..topk) = the first topk classes and
//   topk_logprob = z - lse (fp32), entries past V (topk > V): id -1, logprob -inf; nll[j] = lse - z_t by ce_kernel's own
//   expression (w[j] * nll[j] is plb_launch_ce_fwd_bwd's loss_rows[j] bit for bit); logits_out[j][0..V) = a copy of the row
//   ([n][V], dense). A row with a NaN logit: pred -1, rank V, nll NaN, ids -1, logprobs NaN. Every output pointer may be
//   NULL. topk in [0, 8]. Returns 1, launching nothing, for any other V or topk.
int plb_launch_masked_report_rows(const float* logits, int ldl, int V, const int32_t* tgt, int n, int topk, int32_t* pred,
                                  int32_t* rank, float* nll, int32_t* topk_ids, float* topk_logprob, float* logits_out,
                                  hipStream_t stream);
// Per sample b < B (<= 1024) of the CSR offsets [B+1]: sample_loss[b] = mean of nll over its rows (per-thread chains 256 rows
// apart, wave butterfly, the four waves in order; 0 for a sample without rows), sample_top1 / sample_topk [b] = its rows with
// rank == 0 / rank < topk; totals int32 [4] = {rows, rows with rank == 0, rows with rank < topk, samples that have rows}.
// topk here is only the counting threshold: a caller hands over min(topk, V), so that the rank V of a NaN row never counts.
// Outputs may be NULL; at most two launches (one when only the totals, or only sample outputs, are wanted).
int plb_launch_masked_report_samples(const int32_t* offsets, int B, const int32_t* rank, const float* nll, int topk,
                                     float* sample_loss, int32_t* sample_top1, int32_t* sample_topk, int32_t* totals,
                                     hipStream_t stream);
// Top-1 count of the fused token head from what its first GEMM pass keeps (PlbGemmNT.ce_pmax [rows][ntiles], ce_tlogit
// [rows]) and the row weights of plb_launch_token_ce_combine: totals2[0] = rows with w != 0 (the valid positions),
// totals2[1] = those whose target logit EQUALS the maximum of the row's ntiles per-tile maxima. The rule is TIE-INCLUSIVE —
// a target that ties for the maximum counts — unlike the phoneme rule above (lowest index wins): the fused head keeps no
// arg-max index, only values, and the equality is exact because ce_tlogit is stored from the very fp32 value that enters
// the tile maximum. scratch: int32 [2 * ceil(rows / 4)]. Two launches.
int plb_launch_token_top1(const float* pmax, int ntiles, const float* tlogit, const float* w, int rows, int32_t* scratch,
                          int32_t* totals2, hipStream_t stream);

// ---- token-head predictions without logits (token_topk.hip): a fused GEMM + top-k + log-sum-exp over the vocabulary.
// For j < n: z[c] = X[rows[j]] · W[c] + bias[c], c < NT (X [.][ldx], W [.][ldw] bf16 with K % 64 == 0 elements used per row,
// ldx / ldw multiples of 8, 4-byte aligned; bias fp32 [NT]; fp32 accumulation). rows == NULL: the identity; rows[j] == -1:
// position j has NO ROW. W is read in whole 128-row tiles, i.e. up to row rup(NT, 128): those rows must be readable, their
// values never count (columns >= NT are excluded by index). Row 0 of X is read on behalf of positions without a row.
// Outputs (device, each may be NULL), classes ordered by (logit descending, class index ascending):
//   topk_ids int32 / topk_logprob fp32 [n][topk], 0 <= topk <= PLB_TOPK_MAX: the first topk classes and z - lse; entries past
//   NT: id -1, -inf. lse fp32 [n]. With tgt (int32 [n]): target_logprob [n] = z[tgt] - lse (NaN for a target outside [0, NT))
//   and target_pos [n] = the 0-based position of tgt in the list, -1 when it is not in it (always -1 with topk == 0).
//   logits fp32 [n][NT]: the kernel's own values. totals int32 [3] = {positions that have a row, those with target_pos == 0,
//   those with target_pos >= 0}.
//   A row with a NaN logit (or +inf, whose softmax is NaN): ids -1, log-probs NaN, lse and target_logprob NaN, target_pos -1
//   (it counts in totals[0] only).
//   A position without a row: ids -1, log-probs -inf, lse and target_logprob NaN, target_pos -1, logits 0; never counted.
// strips: 0 = the policy (plb_token_topk_strips), 1 .. PLB_TOPK_MAX_STRIPS forces the count (ids and target_pos do not depend
// on it; lse and the log-probabilities differ by rounding). scratch: plb_token_topk_scratch_bytes(n) bytes, 16-byte aligned.
// n == 0: totals = zeros, nothing else is written. Three launches (two without totals); no atomics, bitwise reproducible.
// Returns 1, launching nothing, on any argument it cannot run.
#define PLB_TOPK_MAX 8
#define PLB_TOPK_MAX_STRIPS 16
int plb_launch_token_topk(const bf16_t* X, int ldx, const int32_t* rows, int n, const bf16_t* W, int ldw, const float* bias,
                          int NT, int K, int topk, int strips, void* scratch, const int32_t* tgt, int32_t* topk_ids,
                          float* topk_logprob, float* lse, float* target_logprob, int32_t* target_pos, float* logits,
                          int32_t* totals, hipStream_t stream);
// strips the launch above runs for (n, NT, strips): with row_tiles = ceil(n / 128), the policy takes ceil(512 / row_tiles)
// (256 CUs about twice); at most PLB_TOPK_MAX_STRIPS and the number of 128-column tiles; then the fewest strips of that
// tile count per strip (no strip is empty). 0 for n < 1 or NT < 1.
int plb_token_topk_strips(int n, int NT, int strips);
// bytes of scratch for n rows: per row PLB_TOPK_MAX_STRIPS x (8 candidates x 8 B + 16 B of statistics), 3 counts per 4 rows
size_t plb_token_topk_scratch_bytes(int n);
// Row list and targets of a report from the position lists of a call: CSR (offsets int32 [B+1], flat [n]) or, offsets ==
// NULL, every position of [B,S] in order (n == B*S). rows[j] = row_start[b] + s (row_start == NULL: b*S + s) for a position
// s < lengths[b] (lengths == NULL: S), else -1; tgt[j] = token_ids[b,s] (NULL, or no row: -1).
int plb_launch_token_topk_prepare(const int32_t* offsets, const int32_t* flat, const int32_t* lengths, const int32_t* row_start,
                                  const int64_t* token_ids, int n, int B, int S, int32_t* rows, int32_t* tgt,
                                  hipStream_t stream);

// Device-side word masking (mask.hip): labels [B,S] -> masked [B,S], counts [B], idx_padded [B,S],
// then offsets [B+1] and flat (CSR of the modified positions).
typedef struct {
  const int64_t* labels; const int32_t* lengths;  // lengths may be null (= S)
  int B, S;
  uint64_t seed; uint32_t step;
  float word_pred_prob, mask_prob, replace_prob;
  int mask_id, sep_id;
  int64_t* masked; int32_t *counts, *idx_padded, *offsets, *flat;
} PlbMask;
int plb_launch_mask(const PlbMask* p, hipStream_t stream);

// Bit-exact application of host-drawn masking decisions (mask.hip; include/plbert.h plb_apply_mask)
typedef struct {
  const int64_t* ids; const int32_t *sample_off, *word_off, *word_begin, *word_len; const int8_t* action;
  const int64_t* repl; const int64_t* word_token; int64_t sep_token; const int32_t* crop_start;
  int B, S, mask_id;
  int64_t *labels, *masked, *tokens; int32_t *lengths_out, *counts, *idx_padded, *offsets, *flat;
} PlbApplyMask;
int plb_launch_apply_mask(const PlbApplyMask* p, hipStream_t stream);

// AdamW (torch.optim.AdamW semantics) over a flat range; also refreshes the bf16 compute copy.
// skip_if_nonzero (two device words, or null): the launch leaves everything untouched when word 0 is non-zero — the engine's
// hand-off error word, so that a step whose LayerNorm statistics are invalid never reaches the parameters (no host round
// trip); with count_skip = 1 / 2 the launch then adds 1 to that word (optimizer steps left out: trainable range / token head)
int plb_launch_adamw(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n, double lr, double beta1,
                     double beta2, double eps, double wd, int step, double grad_scale, unsigned int* skip_if_nonzero,
                     int count_skip, hipStream_t stream);
// ---- gradient accumulation, global-norm clipping (optim.hip; include/plbert.h plb_grad_accum_add / plb_grad_norm /
// plb_adamw_step_clipped). Both partial-sum launches run on a FIXED grid of PLB_NORM_PARTS workgroups: workgroup b owns
// floats [b * chunk, (b + 1) * chunk) of the range, chunk = plb_norm_chunk(n), and writes partials[b] (0 for an empty chunk).
#define PLB_NORM_PARTS 1024
// floats per workgroup: n / PLB_NORM_PARTS rounded up to whole passes of 256 threads x float4
static inline size_t plb_norm_chunk(size_t n) {
  return (n + (size_t)PLB_NORM_PARTS * 1024 - 1) / ((size_t)PLB_NORM_PARTS * 1024) * 1024;
}
// Longest chain of fp32 additions behind one partial: a thread adds 4 squares per pass (one fused multiply-add each),
// then 6 steps of the wave reduction and 3 additions over the four waves.
#define PLB_NORM_CHAIN(n) (4 * (plb_norm_chunk(n) / 1024) + 6 + 3)
// phase 0: accum = grads | 1: accum += grads | 2: grads = accum + grads | 3: grads = accum. partials (phases 2 and 3 only,
// or null): PLB_NORM_PARTS floats, the sums of squares of the values each workgroup stored. n % 4 == 0, 16-byte pointers.
int plb_launch_grad_accum(float* accum, float* grads, size_t n, int phase, float* partials, hipStream_t stream);
// partials[0 .. PLB_NORM_PARTS) = per-workgroup sums of squares of grads[0, n); nothing is written to grads
int plb_launch_grad_sumsq(const float* grads, size_t n, float* partials, hipStream_t stream);
// out[0] = total_norm = grad_scale * sqrt(sum of the nparts partials, in double, fixed order); out[1] = coef =
// min(1, max_norm / (total_norm + 1e-6)), 1 when max_norm <= 0; total_norm not finite: out[2] = 1 and coef = 0, else
// out[2] = 0. out[3] is left alone (plb_launch_adamw_clipped counts there).
int plb_launch_grad_norm_finish(const float* partials, int nparts, double grad_scale, double max_norm, float* out,
                                hipStream_t stream);
// plb_launch_adamw with the gradient (g * grad_scale) * norm[1]; bit-identical to it when norm[1] == 1. norm[2] != 0: the
// launch writes nothing (after the skip word, which is tested first) and, with count_nonfinite, adds 1 to norm[3].
int plb_launch_adamw_clipped(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n, double lr, double beta1,
                             double beta2, double eps, double wd, int step, double grad_scale,
                             unsigned int* skip_if_nonzero, int count_skip, float* norm, int count_nonfinite,
                             hipStream_t stream);
// ---- segmented AdamW and the masked sum of squares (optim.hip; include/plbert.h plb_adamw_step_groups /
// plb_grad_norm_groups). segs: HOST array of at most PLB_NPARAM live segments of [0, n) (begin / end in floats relative to
// p, sorted, disjoint, not empty, every boundary a multiple of 4; `group` is not read) with their pre-rounded scalars, as
// plb_adamw_plan forms them; the launchers copy them into a by-value kernel argument — nothing is read after the call
// returns. What lies between the segments is a hole: no load and no store of p, m, v or the bf16 copy there.
// One pass over [0, n) with each float4's own segment's scalars. norm == null: plb_launch_adamw's arithmetic (one live
// segment over [0, n): its bits); else plb_launch_adamw_clipped's, with its norm[2] / norm[3] semantics. The skip word is
// tested first, as there. Refused (1): a boundary that is no multiple of 4, unsorted or overlapping segments, more than
// PLB_NPARAM of them, a segment outside [0, n), step < 1. n_segs == 0 launches nothing.
int plb_launch_adamw_segments(float* p, const float* g, float* m, float* v, bf16_t* p_bf16, size_t n,
                              const PlbAdamWSegment* segs, int n_segs, double grad_scale, unsigned int* skip_if_nonzero,
                              int count_skip, float* norm, int count_nonfinite, hipStream_t stream);
// plb_launch_grad_sumsq (same grid, chunk and order of additions) with every float4 of a hole taken as zeros (a select: a
// NaN there does not reach the sum): the partials are bit-identical to plb_launch_grad_sumsq's on a zero-filled copy.
int plb_launch_grad_sumsq_segments(const float* grads, size_t n, const PlbAdamWSegment* segs, int n_segs, float* partials,
                                   hipStream_t stream);
// ---- LAMB (lamb.hip; include/plbert.h plb_lamb_step holds the definition). segs: HOST array of 1 to PLB_NPARAM live TENSORS
// of [0, n) (begin / end in floats relative to p, sorted, disjoint, not empty, every boundary a multiple of 4; `tensor` = the
// result slot, increasing; `group` is not read) with their pre-rounded scalars, as plb_lamb_plan forms them; the launchers copy
// them into a by-value kernel argument. Workgroups are mapped to tensors: tensor s owns ceil(floats / 1024) consecutive
// workgroups, each with one piece of 1024 floats counted from the tensor's own start. What lies between the tensors is a hole:
// no load and no store there. Refused (1): what plb_launch_adamw_segments refuses, an adapt that is neither 0 nor 1, slots that
// do not increase or leave [0, PLB_NPARAM). n_segs == 0 launches nothing (the finish then writes zeros to its slots).
// The three launches of one range take the same segs / n_segs / n, skip word and norm. skip_if_nonzero (tested first) or
// norm[2] != 0: no launch stores anything, pass 1 alone counts (skip[count_skip], norm[3] with count_nonfinite).
// Longest chain of fp32 additions behind one partial: 4 squares per thread (one fused multiply-add each), 6 steps of the wave
// reduction, 3 additions over the four waves. The partials of a tensor are added in double.
#define PLB_LAMB_CHAIN (4 + 6 + 3)
// workgroups of the passes over these tensors = pairs of floats pass 1 writes to `partials`; -1: the table is refused
int64_t plb_lamb_workgroups(const PlbLambSegment* segs, int n_segs, size_t n);
// m, v advanced as plb_launch_adamw_clipped advances them (norm == null: coefficient 1, no flag test), bit for bit;
// partials[2 b], partials[2 b + 1] = sum of p^2, sum of u^2 over workgroup b's piece. p and g are only read.
int plb_launch_lamb_pass1(const float* p, const float* g, float* m, float* v, size_t n, const PlbLambSegment* segs, int n_segs,
                          double grad_scale, unsigned int* skip_if_nonzero, int count_skip, float* norm, int count_nonfinite,
                          float* partials, hipStream_t stream);
// results[4 t ..] = wn, un, trust, 1 for every tensor t of segs, and 0, 0, 0, 0 for every other slot of [slot_lo, slot_hi)
int plb_launch_lamb_finish(const PlbLambSegment* segs, int n_segs, size_t n, int slot_lo, int slot_hi, const float* partials,
                           float* results, const unsigned int* skip_if_nonzero, const float* norm, hipStream_t stream);
// p -= (lr * trust) * u with u recomputed from the stored m, v by pass 1's expression, trust = results[4 t + 2]; the bf16
// copy of the new p (p_bf16 null: none). m, v are only read; the gradient buffer is not an argument.
int plb_launch_lamb_pass2(float* p, const float* m, const float* v, bf16_t* p_bf16, size_t n, const PlbLambSegment* segs,
                          int n_segs, const float* results, const unsigned int* skip_if_nonzero, const float* norm,
                          hipStream_t stream);
// End of a loss call: mirror the hand-off error word into host-visible memory (host_mirror: device pointer of a pinned
// host word) and, when it is non-zero, overwrite the loss with NaN — whoever reads the loss sees that the step is invalid
int plb_launch_step_status(unsigned int* ln_err, float* loss, unsigned int* host_mirror, const float* summed, hipStream_t stream);
// *out = the word as a float (the ranks' words are summed by an all-reduce; step_status merges the sum back)
int plb_launch_status_export(const unsigned int* ln_err, float* out, hipStream_t stream);
int plb_launch_cast_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t stream);
// dst[c, r] = bf16(src[r, c]) for r<R, c<C ; dst has ldd >= R columns (zero fill is the caller's job)
int plb_launch_transpose_cast(const float* src, int R, int C, bf16_t* dst, int ldd, hipStream_t stream);
int plb_launch_transpose_cast_multi(int n, const float* const* src, const int* R, const int* C, bf16_t* const* dst,
                                    const int* ldd, hipStream_t stream);
int plb_launch_bf16_to_f32(const bf16_t* src, int lds_, float* dst, int ldd, int R, int C, hipStream_t stream);

}  // extern "C"
