// Launch sequences of the shared layer: embeddings + L applications forward (run_encoder), the layer loop of the backward
// (encoder_bwd), both with the last application full or pruned to the masked rows, and the launch of a token-major
// weight-gradient GEMM as its plan (gemm_tn_plan.h) says. Only writer of u_is_derivative, tn8_call and part_rows_used,
// which the forward of a call leaves for its backward.
#include "engine_internal.h"

// ---- launch descriptors -----------------------------------------------------------------------------------------------
// C[M, N] = A[M, K] · B[N, K]^T on packed operands (lda = ldb = K), every row stored: the callers add bias, residual and
// outputs
PlbGemmNT nt_desc(const bf16_t* A, const bf16_t* B, int64_t M, int N, int K) {
  PlbGemmNT g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = K; g.B = B; g.ldb = K; g.M = (int)M; g.N = N; g.K = K; g.Mstore = (int)M;
  return g;
}

static F8Op f8_op(const uint8_t* a8, const F8Site& a, const F8Weight& w, int a_bf8) { return F8Op{a8, w.img, a.deq, w.deq, a_bf8}; }
static PlbGemmNT f8_operands(const PlbGemmNT* g, const F8Op* f8) {
  PlbGemmNT q = *g;
  q.A = reinterpret_cast<const bf16_t*>(f8->A8); q.B = reinterpret_cast<const bf16_t*>(f8->B8);
  q.deq_a = f8->deq_a; q.deq_b = f8->deq_b;
  return q;
}
// g in form `form` (PlbGemmNTForm: plain and gelu forms, LayerNorm forms, gelu-derivative-stash forms) on bf16 operands or,
// with f8, on their 1-byte images: the launcher of that form and operand kind
static int gemm_nt_any(PlbGemmNT* g, int form, const F8Op* f8, hipStream_t s) {
  PlbGemmNT q;
  if (f8) { q = f8_operands(g, f8); g = &q; }
  const int a_bf8 = f8 ? f8->a_bf8 : 0;
  switch (form) {
    case PLB_NT_LNFWD: case PLB_NT_LNBWD:
      return f8 ? plb_launch_gemm_nt_fp8_ln(g, form, a_bf8, s) : plb_launch_gemm_nt_ln(g, form, s);
    case PLB_NT_GELUD: case PLB_NT_GELUDBWD:
      return f8 ? plb_launch_gemm_nt_fp8_gelud(g, form == PLB_NT_GELUDBWD, a_bf8, s)
                : plb_launch_gemm_nt_gelud(g, form == PLB_NT_GELUDBWD, s);
  }
  return f8 ? plb_launch_gemm_nt_fp8(g, form, a_bf8, s) : plb_launch_gemm_nt(g, form, 0, s);
}
// What the launchers will do is asked, never restated: which fusions a call takes, and how many partial rows its launches
// write, come from the plan of the launch at the call's shape.
PlbGemmNTPlan nt_plan(int64_t M, int N, int K, int form, int operands, int opts) {
  PlbGemmNTPlan pl;
  plb_gemm_nt_plan((int)M, N, K, form, operands, opts, 0, &pl);
  return pl;
}
// the 1-byte image + running maximum a launch writes beside its output (scale in, maxima out)
static void f8_out(PlbGemmNT* g, uint8_t* img, int ld, const F8Site& q, int bf8) {
  g->C8 = img; g->ldc8 = ld; g->q_scale = q.scale; g->q_amax = q.amax; g->c8_bf8 = bf8;
}

// The attention launches of one application of call c on slots sl: the fields forward, backward and the probabilities
// share; the callers add their outputs (and the context buffer of a pruned last application)
static PlbAttn attn_desc(const PlbEngine* e, const Call& c, const Slots& sl) {
  PlbAttn at;
  memset(&at, 0, sizeof(at));
  at.qkv = sl.qkv; at.ldqkv = 3 * e->H; at.lengths = c.lengths; at.B = c.B; at.S = c.S; at.NH = e->NH; at.H = e->H;
  at.scale = 0.125f;
  at.row_start = c.rw.row_start;
  at.key_words = c.rw.key_words; at.ldkw = c.rw.ldkw;
  at.ctx = sl.ctx; at.ldctx = e->H; at.lse = sl.lse;
  return at;
}
// what the attention launchers will do with a descriptor (attn_plan.h), asked like nt_plan
static PlbAttnPlan attn_plan(const PlbAttn& at) {
  PlbAttnPlan pl;
  plb_attn_plan(at.B, at.S, at.NH, plb_attn_flags(&at), &pl);
  return pl;
}
// partial rows per application of the Q/K/V bias gradient that the attention backward stores in a call of B x S
int qkvcol_rows(const PlbEngine* e, int B, int S) {
  PlbAttnPlan pl;
  plb_attn_plan(B, S, e->NH, 0, &pl);
  return pl.colpart_rows;
}
Slots slots(const PlbEngine* e, int64_t Tp, int B, int S, int l, bool stash, int prows, int du_rows) {
  const int64_t H = e->H, I = e->I, sl = stash ? l : 0;
  auto bf = [&](int64_t off, int64_t width) { return e->at<bf16_t>(off) + sl * Tp * width; };
  auto u8 = [&](int64_t off, int64_t width) { return e->at<uint8_t>(off) + sl * Tp * width; };
  auto f32 = [&](int64_t off, int64_t per_layer) { return e->at<float>(off) + sl * per_layer; };
  Slots v;
  memset(&v, 0, sizeof(v));
  v.x = e->at<bf16_t>(e->o_x) + (int64_t)(stash ? l : l & 1) * Tp * H;
  v.y = e->at<bf16_t>(e->o_x) + (int64_t)(stash ? l + 1 : (l + 1) & 1) * Tp * H;
  v.qkv = bf(e->o_qkv, 3 * H); v.ctx = bf(e->o_ctx, H); v.pre1 = bf(e->o_pre1, H); v.a = bf(e->o_a, H);
  v.u = bf(e->o_u, I); v.g = bf(e->o_g, I); v.pre2 = bf(e->o_pre2, H);
  v.mean1 = f32(e->o_mean1, Tp); v.rstd1 = f32(e->o_rstd1, Tp); v.mean2 = f32(e->o_mean2, Tp); v.rstd2 = f32(e->o_rstd2, Tp);
  PlbAttnPlan ap;   // the per-application strides of the attention statistics and of the Q/K/V bias partial rows
  plb_attn_plan(B, S, e->NH, 0, &ap);
  v.lse = f32(e->o_lse, ap.stat_floats);
  v.x8 = u8(e->o_x8, H); v.c8 = u8(e->o_c8, H); v.a8 = u8(e->o_a8, H); v.g8 = u8(e->o_g8, I);
  v.x8n = e->at<uint8_t>(e->o_x8) + (stash ? l + 1 : 0) * Tp * H;   // (one slot: consumed before it is rewritten)
  if (stash) {
    v.dqkv = bf(e->o_dqkv, 3 * H); v.dpre1 = bf(e->o_dpre1, H); v.du = bf(e->o_du, I); v.dpre2 = bf(e->o_dpre2, H);
    v.dp8 = u8(e->o_dp8, H); v.du8 = u8(e->o_du8, I); v.dp18 = u8(e->o_dp18, H); v.dq8 = u8(e->o_dq8, 3 * H);
    v.part1 = f32(e->o_part1, (int64_t)prows * 3 * H); v.part2 = f32(e->o_part2, (int64_t)prows * 3 * H);
    v.qkvcol = f32(e->o_qkvcol, (int64_t)ap.colpart_rows * 3 * H); v.ducol = f32(e->o_ducol, (int64_t)du_rows * I);
  }
  return v;
}

// ---- LayerNorm: in the producing GEMM's epilogue or standalone ----------------------------------------------------------
// LayerNorm in the epilogue of the GEMM that produces its input (gemm_ln.hip, gemm_fp8_ln.hip): the shapes it exists for,
// in bf16 and in fp8 calls alike (the fp8 forms write the 1-byte images the standalone LayerNorm kernels used to write);
// an fp8 CALIBRATION call computes in bf16 (it must equal the bf16 path bit for bit: tests/test_gpu_fp8.py).
// (bit 1: the forward forms of a call, bit 2: the backward forms, whose A operand is a gradient: e5m2 in an fp8 call. K is H,
// I or 3H: multiples of 128 all, plb_create sees to that, so one query stands for the two launches of a direction.)
static bool ln_fusable(const PlbEngine* e, int64_t Tp, int bit, bool f8) {
  const int ops = !f8 ? PLB_NT_BF16 : bit == 1 ? PLB_NT_FP8_E4M3 : PLB_NT_FP8_E5M2;
  return (e->ln_fuse & bit) && nt_plan(Tp, e->H, e->H, bit == 1 ? PLB_NT_LNFWD : PLB_NT_LNBWD, ops).rc == 0;
}
// Does the forward of this call stash gelu_new'(u) instead of u (plb_launch_gemm_nt_gelud)? Recorded in the engine: the
// backward of the same call must read the stash the way the forward wrote it — the stash is in the LANE layout of the
// tile that wrote it (the plan's for the call's operand kind and row count), so forward and backward of a call run in one mode.
static bool gelu_dstash(PlbEngine* e, int64_t Tp, bool f8_call) {
  e->u_is_derivative = e->gelu_dstash_on && nt_plan(Tp, e->I, e->H, PLB_NT_GELUD, f8_call ? PLB_NT_FP8_E4M3 : PLB_NT_BF16).rc == 0;
  return e->u_is_derivative;
}
static void ln_fields(const PlbEngine* e, PlbGemmNT* g, const float* gamma, const float* beta, float* mean, float* rstd) {
  g->ln_gamma = gamma; g->ln_beta = beta; g->ln_mean = mean; g->ln_rstd = rstd; g->ln_eps = e->c.layer_norm_eps;
  g->ln_xchg = e->at<unsigned long long>(e->o_lnx); g->ln_err = e->at<unsigned int>(e->o_lnerr);
}
static LnSlot ln1_slot(const PlbEngine* e, const Slots& v) {
  return LnSlot{e->par(PLB_LN1_W), e->par(PLB_LN1_B), v.pre1, v.mean1, v.rstd1, v.part1};
}
static LnSlot ln2_slot(const PlbEngine* e, const Slots& v) {
  return LnSlot{e->par(PLB_LN2_W), e->par(PLB_LN2_B), v.pre2, v.mean2, v.rstd2, v.part2};
}
// g (C = the LayerNorm's input, + bias / residual) and y = LayerNorm(C) on rows [0, T): the fused form 5 (GEMM + residual +
// LayerNorm in one launch) or the GEMM and the standalone kernel. y8 (or null): y's e4m3 image under site q.
static int gemm_ln_fwd(PlbEngine* e, PlbGemmNT* g, const F8Op* f8, bool fused, const LnSlot& ln, bf16_t* y, int T,
                       uint8_t* y8, const F8Site& q, hipStream_t s) {
  const int H = e->H;
  if (fused) {
    g->C2 = y; g->ldc2 = H;
    ln_fields(e, g, ln.gamma, ln.beta, ln.mean, ln.rstd);
    if (y8) f8_out(g, y8, H, q, 0);
    TRY(gemm_nt_any(g, PLB_NT_LNFWD, f8, s));
    return 0;
  }
  TRY(gemm_nt_any(g, PLB_NT_PLAIN, f8, s));
  PlbLayerNorm p;
  memset(&p, 0, sizeof(p));
  p.x = g->C; p.ldx = H; p.gamma = ln.gamma; p.beta = ln.beta; p.eps = e->c.layer_norm_eps;
  p.y = y; p.ldy = H; p.T = T; p.H = H; p.mean = ln.mean; p.rstd = ln.rstd;
  if (y8) { p.out8 = y8; p.ld8 = H; p.q_scale = q.scale; p.q_amax = q.amax; }
  TRY(plb_launch_ln_fwd(&p, s));
  return 0;
}
// standalone LayerNorm backward: dx = LN'(dy) on rows [0, T), zeros in [T, Tzero), nblocks rows of dgamma | dbeta | column
// sums of dx; dx8 (or null): dx's e5m2 image under site q
static int ln_bwd(PlbEngine* e, const LnSlot& ln, int nblocks, const bf16_t* dy, bf16_t* dx, int T, int Tzero, uint8_t* dx8,
                  const F8Site& q, hipStream_t s) {
  const int H = e->H;
  PlbLayerNorm p;
  memset(&p, 0, sizeof(p));
  p.x = ln.pre; p.ldx = H; p.gamma = ln.gamma; p.T = T; p.H = H; p.Tzero = Tzero; p.mean = ln.mean; p.rstd = ln.rstd;
  p.dy = dy; p.lddy = H; p.dx = dx; p.lddx = H; p.partials = ln.partials; p.nblocks = nblocks;
  if (dx8) { p.out8 = dx8; p.ld8 = H; p.q_scale = q.scale; p.q_amax = q.amax; }
  TRY(plb_launch_ln_bwd(&p, s));
  return 0;
}
// g (C = the gradient of the LayerNorm's OUTPUT, + residual) and that LayerNorm's backward: the fused form 6 (the output
// gradient is never stored: the epilogue writes dx and the partial rows) or the GEMM into C and ln_bwd
static int gemm_ln_bwd(PlbEngine* e, PlbGemmNT* g, const F8Op* f8, bool fused, const LnSlot& ln, int nblocks, bf16_t* dx, int T,
                       int Tzero, uint8_t* dx8, const F8Site& q, hipStream_t s) {
  if (fused) {
    g->C = dx; g->aux = ln.pre; g->ldaux = e->H; g->colpart = ln.partials;
    ln_fields(e, g, ln.gamma, nullptr, ln.mean, ln.rstd);
    if (dx8) f8_out(g, dx8, e->H, q, 1);
    TRY(gemm_nt_any(g, PLB_NT_LNBWD, f8, s));
    return 0;
  }
  TRY(gemm_nt_any(g, PLB_NT_PLAIN, f8, s));
  return ln_bwd(e, ln, nblocks, g->C, dx, T, Tzero, dx8, q, s);
}

// ---- the last application on the masked rows only --------------------------------------------------------------------
// The reference evaluates every position of every application and then reads the masked positions of the LAST one
// (train.py:107-131: pred[b, :len_b][idx_b]). Positions exchange information only inside attention (keys / values), so
// behind the attention of application L-1 nothing a non-masked row computes reaches the loss — forward or backward, where
// its output gradient is exactly zero. A phoneme-only loss call therefore runs dense + LayerNorm, the FFN and the second
// LayerNorm of application L-1 on the ~13 % masked rows alone (gathered, padded to 128), and their backward likewise; Q/K/V
// projection and attention stay on all rows (every key / value is needed), and so does everything below application L-1.
// Results are those of the full evaluation (each row's arithmetic is unchanged; the weight gradients lose only exact
// zeros from their sums). Compact GEMMs of ~2,300 rows do not fill one-tile-per-CU grids, so this part runs on the
// small-shape launches (GEMM + LayerNorm kernels, gelu by act 1 / 2): 168 -> 75 us forward, 164 -> 86 us backward, and the
// three weight-gradient GEMMs that stack its rows read (L-1) Tp + Mc rows instead of L Tp (measured: profiles/r05_*).
// Those figures are with the small NT kernel's 128x128 form (90-240 workgroups on 256 CUs). Its 64x64 form, which
// plb_launch_gemm_nt picks for these grids, takes the three GEMMs of the forward from 62 to 44 us and the three of the
// backward from 62 to 41 us at 1,920 rows (7.8 + 16.3 + 19.6 and 15.2 + 18.1 + 7.3 us by themselves; the head's logits
// 13.7 -> 6.3, its dH 9.2 -> 5.1), results bit for bit the same: profiles/nt_small_tile_kernel_ab.txt; the step:
// 9.085 -> 9.003 ms, profiles/nt_small_tile_step_ab_same_box.txt.
// fp8 calls run this part in bf16 too and add the 1-byte images of the compact rows that their stacked weight-gradient
// GEMMs read. Not taken by dual-head calls (the token loss reads every position), when more than half of the positions
// are masked, and under PLBERT_PRUNE_LAST=0.
static int g_prune_last = -1;   // test / tuning hook (plb_set_prune_last): -1 the environment's choice, 0 off, 1 on
extern "C" void plb_set_prune_last(int on) { g_prune_last = on < 0 ? -1 : (on ? 1 : 0); }
bool prune_enabled() {
  static const bool v = [] { const char* e = getenv("PLBERT_PRUNE_LAST"); return !(e && !strcmp(e, "0")); }();
  return g_prune_last < 0 ? v : g_prune_last != 0;
}
// post-attention part of application L-1 on the compact rows; leaves the final hidden rows in o_hm ([Mc][H]: the head's
// operand) and, in a training call, the compact activations at the START of application L-1's stash slots (sl) — the
// stacked weight-gradient operands then simply end Tp - Mc rows earlier
static int last_application_fwd_pruned(PlbEngine* e, const Prune* pr, bool stash, bool calib, bool tn8, const Slots& sl,
                                       const bf16_t* ctx_att, hipStream_t s) {
  const int H = e->H, I = e->I, L = e->L, Mc = pr->Mc, n = pr->n;
  const F8Site sA(e, F8_A, L - 1), sG(e, F8_G, L - 1), sC(e, F8_C, L - 1);
  // training: compact tensors in their own slots (the backward and the weight gradients read them), the gathered
  // residual rows in a backward temporary; forward-only: the one set of slots, rotated so that nothing is read and
  // written by the same launch (ctx_att = the ctx slot: gathered into the pre1 slot, whose sum then goes to the ctx slot)
  bf16_t* ctxc = stash ? sl.ctx : sl.pre1;
  bf16_t* xc = stash ? e->at<bf16_t>(e->o_da) : sl.a;
  bf16_t* pre1c = stash ? sl.pre1 : sl.ctx;
  bf16_t* ac = stash ? sl.a : sl.pre1;
  TRY(plb_launch_gather_rows(ctx_att, H, pr->rows, n, Mc, H, ctxc, H, s));
  TRY(plb_launch_gather_rows(sl.x, H, pr->rows, n, Mc, H, xc, H, s));
  PlbGemmNT g = nt_desc(ctxc, e->wbf(PLB_DENSE_W), Mc, H, H);
  g.bias = e->par(PLB_DENSE_B); g.res = xc; g.ldr = H; g.C = pre1c; g.ldc = H;
  const LnSlot ln1 = {e->par(PLB_LN1_W), e->par(PLB_LN1_B), pre1c, sl.mean1, sl.rstd1, nullptr};
  if (gemm_ln_fwd(e, &g, nullptr, false, ln1, ac, Mc, nullptr, F8Site(), s)) return 1;
  if (calib) TRY(plb_launch_amax(ac, 1, (size_t)n, H, H, sA.amax, s));
  g = nt_desc(ac, e->wbf(PLB_FFN_W), Mc, I, H);
  g.bias = e->par(PLB_FFN_B); g.C = sl.u; g.ldc = I; g.C2 = sl.g; g.ldc2 = I;
  TRY(plb_launch_gemm_nt(&g, 1, 0, s));
  if (calib) TRY(plb_launch_amax(sl.g, 1, (size_t)n, I, I, sG.amax, s));
  g = nt_desc(sl.g, e->wbf(PLB_FFNO_W), Mc, H, I);
  g.bias = e->par(PLB_FFNO_B); g.res = ac; g.ldr = H; g.C = sl.pre2; g.ldc = H;
  if (gemm_ln_fwd(e, &g, nullptr, false, ln2_slot(e, sl), e->at<bf16_t>(e->o_hm), Mc, nullptr, F8Site(), s)) return 1;
  if (tn8) {
    // fp8 training call: this part itself runs in bf16 (2,000 rows: nothing to gain from fp8 operands), but the stacked
    // weight-gradient GEMMs read 1-byte images of EVERY application: the compact context / a / gelu(u) rows as e4m3 images
    // at the start of this application's image slots, under the sites' scales, their maxima reported like any other's
    const void* src[3] = {ctxc, ac, sl.g}; const int fl[3] = {1, 1, 1};
    const size_t nel[3] = {(size_t)Mc * H, (size_t)Mc * H, (size_t)Mc * I};
    const float* sc[3] = {sC.scale, sA.scale, sG.scale};
    uint8_t* dst[3] = {sl.c8, sl.a8, sl.g8};
    float* am[3] = {sC.amax, sA.amax, sG.amax};
    TRY(plb_launch_quantize_multi(3, src, fl, nel, sc, dst, am, s));
  }
  return 0;
}

// Hidden-state slot `slot` of a call's taps (include/plbert.h: PlbLayerOutputs), when wanted: the fp32 image of the bf16 rows
// x in the caller's [B,S,H] layout, zeros at the pad positions in both layouts (plb_encode's conversion pass).
static int tap_hidden(PlbEngine* e, const Call& c, int slot, const bf16_t* x) {
  float* const out = (c.taps && c.taps->hidden_states) ? c.taps->hidden_states[slot] : nullptr;
  if (!out) return 0;
  if (c.lengths) TRY(plb_launch_unpack_rows(x, 1, e->H, c.rw.row_start, c.lengths, c.B, c.S, e->H, out, c.s));
  else TRY(plb_launch_bf16_to_f32(x, e->H, out, e->H, c.rw.T, e->H, c.s));
  return 0;
}

// The embedding descriptors of a call. PlbEmbed from the engine: tables, LayerNorm affine, eps, the call's shapes and, in a
// packed call, its plan; the forward and the backward tail add what is their own (out, fill_slots | the gradient outputs).
PlbEmbed embed_desc(const PlbEngine* e, const Call& c) {
  PlbEmbed em;
  memset(&em, 0, sizeof(em));
  em.ids = c.ids; em.T = c.rw.T; em.S = c.S; em.E = e->E; em.V = e->V;
  em.word = e->par(PLB_WORD_EMB); em.pos = e->par(PLB_POS_EMB); em.type0 = e->par(PLB_TYPE_EMB);
  em.gamma = e->par(PLB_EMB_LN_W); em.beta = e->par(PLB_EMB_LN_B); em.eps = e->c.layer_norm_eps;
  if (c.rw.row_start) { em.row_start = c.rw.row_start; em.lengths = c.lengths; em.B = c.B; }
  return em;
}
// PlbEmbedIn over `base` from the per-token sources of an EmbedCall (plb_*_inputs): the launches of embed_inputs.hip
PlbEmbedIn embed_in_desc(const PlbEngine* e, const EmbedCall& ec, const PlbEmbed* base) {
  PlbEmbedIn xi;
  memset(&xi, 0, sizeof(xi));
  xi.base = base;
  xi.token_type_ids = ec.in.token_type_ids; xi.position_ids = ec.in.position_ids; xi.inputs_embeds = ec.in.inputs_embeds;
  xi.NTY = e->c.type_vocab_size; xi.P = e->P;
  return xi;
}

// Embeddings + L applications of the shared layer. stash: keep every layer's activations (training)
// or reuse the layer-0 slots (inference). Returns the final hidden buffer in *xout.
// c: the call (Call) — c.ec is what the embeddings read beside the ids (ids is null with inputs_embeds); pr (or null): the
// masked rows a pruned last application runs on.
// c.taps (or null; never with a pruned last application): the per-application outputs the caller asked for — the map-in
// output and every application's output as they are written, the attention probabilities from the qkv rows and the
// log-sum-exp of the attention forward that has just run (without a stash the next application reuses that slot: stream
// order protects it).
// fp8 mode: EVERY large GEMM of the layer runs on 1-byte images — QKV, dense (+ LayerNorm 1), FFN up (+ gelu), FFN output
// (+ LayerNorm 2) on e4m3 images of x, the attention context, a and gelu(u). Each image is written, with the scale its
// site learnt in the previous call, by the launch that produces the tensor (the fused LayerNorm / gelu epilogues, the
// attention kernel; the standalone LayerNorm kernels on shapes without a fused form), one image per layer in a training
// call: the weight-gradient GEMMs read them all at the end of the backward. A calibration call (the first after
// plb_set_fp8, and a training call whose gradient sites have not been seen yet) runs in bf16 and only records the maxima.
int run_encoder(PlbEngine* e, const Call& c, bool stash, bf16_t** xout, const Prune* pr) {
  const int E = e->E, H = e->H, I = e->I, L = e->L, B = c.B, S = c.S;
  const Rows& rw = c.rw;
  hipStream_t s = c.s;
  const int T = rw.T;
  const int64_t Tp = rw.Tp;
  const bool f8 = f8_call(e, Tp, stash);
  const bool calib = e->fp8_on && !f8;
  // Packed fp8 call: the launches that write a 1-byte image beside their rows cover the tail behind the last slot too (the
  // layer-0 quantisation, the standalone LayerNorm forward; the GEMM epilogues store every row anyway), so every image row
  // the next GEMM and the stacked weight-gradient GEMMs read holds a finite value that only this call's inputs decide. The
  // tail rows are those of zero embeddings behind a zero attention output: the same in every call.
  const int T8 = (f8 && rw.row_start) ? (int)Tp : T;
  if (e->fp8_on && e->fp8_wstale) TRY(fp8_quantize_weights(e, s));
  PlbEmbed em = embed_desc(e, c);
  em.out = e->at<bf16_t>(e->o_e); em.ldo = E;
  if (rw.row_start) {   // packed: every row of the call gets a value (zeros where no token sits), the tail included
    em.T = (int)Tp;
    // fp8 mode (plb_set_packed_fp8): the rest of a slot is embedded like the pad positions of a padded call, so the sites'
    // maxima — taken over every row of the slots — are those of the padded call on the batch trimmed to its slots
    em.fill_slots = e->fp8_on;
  }
  if (c.ec.any()) {   // per-token sources (plb_*_inputs): the row kernel of embed_inputs.hip
    const PlbEmbedIn xi = embed_in_desc(e, c.ec, &em);
    TRY(plb_launch_embed_inputs_fwd(&xi, s));
  } else {
    TRY(plb_launch_embed_fwd(&em, s));
  }

  const Slots first = slots(e, Tp, B, S, 0, stash);
  PlbGemmNT g = nt_desc(em.out, e->wbf(PLB_MAP_W), Tp, H, E);
  g.bias = e->par(PLB_MAP_B); g.C = first.x; g.ldc = H;
  TRY(plb_launch_gemm_nt(&g, 0, 0, s));
  if (tap_hidden(e, c, 0, first.x)) return 1;
  if (f8) {  // layer 0 reads the map-in output, which no LayerNorm produced: one quantisation pass
    // (image and the site's maximum in one pass: the rows are contiguous)
    const F8Site sX(e, F8_X, 0);
    const void* src1[1] = {first.x}; const int bf1[1] = {1}; const size_t n1[1] = {(size_t)T8 * H};
    const float* sc1[1] = {sX.scale}; uint8_t* dst1[1] = {first.x8}; float* am1[1] = {sX.amax};
    TRY(plb_launch_quantize_multi(1, src1, bf1, n1, sc1, dst1, am1, s));
  }
  const bool fuse_f = ln_fusable(e, Tp, 1, f8);
  const bool dstash = gelu_dstash(e, Tp, f8);
  // do the weight-gradient GEMMs of this call read the 1-byte images? Then gelu(u), dU and dQKV leave as images alone.
  // (Needs the derivative stash: forms 1 / 2 always write their bf16 outputs.)
  if (stash) e->tn8_call = f8 && e->fp8_tn && dstash && tn8_ok(e, (int64_t)L * Tp);
  const bool tn8 = stash && e->tn8_call;

  for (int l = 0; l < L; ++l) {
    const Slots sl = slots(e, Tp, B, S, l, stash);
    const F8Site sX(e, F8_X, l), sA(e, F8_A, l), sG(e, F8_G, l), sC(e, F8_C, l);
    if (calib) TRY(plb_launch_amax(sl.x, 1, (size_t)T, H, H, sX.amax, s));
    // fused QKV projection
    g = nt_desc(sl.x, e->wbf(PLB_Q_W), Tp, 3 * H, H);
    g.bias = e->par(PLB_Q_B); g.C = sl.qkv; g.ldc = 3 * H;
    const F8Op oq = f8_op(sl.x8, sX, F8Weight(e, F8W_QKV), 0);
    TRY(gemm_nt_any(&g, PLB_NT_PLAIN, f8 ? &oq : nullptr, s));
    PlbAttn at = attn_desc(e, c, sl);
    // pruned last application: the attention output of ALL rows goes to a buffer of its own (training: a backward temporary
    // that the attention backward of this application reads again — its slot holds the compact rows), then only the masked
    // rows continue
    const bool pruned_layer = pr != nullptr && l == L - 1;
    bf16_t* const ctx_att = (pruned_layer && stash) ? e->at<bf16_t>(e->o_dy1) : sl.ctx;
    at.ctx = ctx_att;
    // (pruned: nobody reads the context's image of all rows — the compact rows' image is made with the others, below)
    if (f8 && !pruned_layer) { at.ctx8 = sl.c8; at.ldctx8 = H; at.ctx_scale = sC.scale; at.ctx_amax = sC.amax; }
    // packed fp8-mode call with rows of a slot that no attention workgroup stores (the plan's unwritten_rows). The
    // calibration maxima and the images are taken over every row of the slots: zeros there, not what an earlier call left
    // (bf16 calls leave them alone: finite is enough there)
    if (e->fp8_on && attn_plan(at).unwritten_rows) {
      HIPTRY(hipMemsetAsync(ctx_att, 0, (size_t)T * H * 2, s));
      if (at.ctx8) HIPTRY(hipMemsetAsync(sl.c8, 0, (size_t)T * H, s));
    }
    TRY(plb_launch_attn_fwd(&at, s));
    if (float* const probs = (c.taps && c.taps->attentions) ? c.taps->attentions[l] : nullptr)
      TRY(plb_launch_attn_probs_masked(at.qkv, at.ldqkv, at.lse, at.lengths, at.row_start, at.key_words, at.ldkw, at.B, at.S, at.NH,
                                       at.scale, probs, s));
    // packed: the tail behind the last slot (up to 1,023 rows) is written by no attention workgroup, and what sits there
    // goes through dense / LayerNorm / FFN into the stash the weight-gradient GEMMs read: zeros, not whatever was there
    if (rw.row_start && Tp > T) {
      HIPTRY(hipMemsetAsync(ctx_att + (int64_t)T * H, 0, (size_t)(Tp - T) * H * 2, s));
      if (at.ctx8) HIPTRY(hipMemsetAsync(sl.c8 + (int64_t)T * H, 0, (size_t)(Tp - T) * H, s));   // (the image of those zeros)
    }
    if (calib) TRY(plb_launch_amax(ctx_att, 1, (size_t)T, H, H, sC.amax, s));
    if (pruned_layer) {
      if (last_application_fwd_pruned(e, pr, stash, calib, tn8, sl, ctx_att, s)) return 1;
      *xout = e->at<bf16_t>(e->o_hm);
      break;
    }
    // dense + residual, LayerNorm 1
    g = nt_desc(sl.ctx, e->wbf(PLB_DENSE_W), Tp, H, H);
    g.bias = e->par(PLB_DENSE_B); g.res = sl.x; g.ldr = H; g.C = sl.pre1; g.ldc = H;
    const F8Op od = f8_op(sl.c8, sC, F8Weight(e, F8W_D), 0);
    if (gemm_ln_fwd(e, &g, f8 ? &od : nullptr, fuse_f, ln1_slot(e, sl), sl.a, T8, f8 ? sl.a8 : nullptr, sA, s)) return 1;
    if (calib) TRY(plb_launch_amax(sl.a, 1, (size_t)T, H, H, sA.amax, s));
    // FFN: u = a W1^T + b1, g = gelu_new(u); pre2 = g W2^T + b2 + a
    g = nt_desc(sl.a, e->wbf(PLB_FFN_W), Tp, I, H);
    g.bias = e->par(PLB_FFN_B); g.C = sl.u; g.ldc = I; g.C2 = sl.g; g.ldc2 = I;
    if (f8) f8_out(&g, sl.g8, I, sG, 0);
    const F8Op o1 = f8_op(sl.a8, sA, F8Weight(e, F8W_1), 0);
    // calls on tile multiples stash gelu_new'(u) in the "u" slot (gelu_dstash): the forward's sigmoid serves the
    // activation and its derivative, and the backward epilogue multiplies instead of evaluating the derivative. In an
    // fp8 call gelu(u) itself leaves as its e4m3 image ALONE: nothing reads it in bf16 (FFN output GEMM and weight
    // gradient take the image)
    if (dstash) {
      if (tn8) { g.C2 = nullptr; g.ldc2 = 0; }
      TRY(gemm_nt_any(&g, PLB_NT_GELUD, f8 ? &o1 : nullptr, s));
    } else {
      TRY(gemm_nt_any(&g, PLB_NT_GELU, f8 ? &o1 : nullptr, s));
    }
    if (calib) TRY(plb_launch_amax(sl.g, 1, (size_t)T, I, I, sG.amax, s));
    // FFN output + residual, LayerNorm 2 (+ the next application's input image)
    g = nt_desc(sl.g, e->wbf(PLB_FFNO_W), Tp, H, I);
    g.bias = e->par(PLB_FFNO_B); g.res = sl.a; g.ldr = H; g.C = sl.pre2; g.ldc = H;
    const F8Op o2 = f8_op(sl.g8, sG, F8Weight(e, F8W_2), 0);
    const bool next8 = f8 && l + 1 < L;
    if (gemm_ln_fwd(e, &g, f8 ? &o2 : nullptr, fuse_f, ln2_slot(e, sl), sl.y, T8, next8 ? sl.x8n : nullptr,
                    next8 ? F8Site(e, F8_X, l + 1) : F8Site(), s))
      return 1;
    if (tap_hidden(e, c, l + 1, sl.y)) return 1;
    *xout = sl.y;
  }
  return 0;
}

// dW[N,K] = A^T B over Mtot rows -> out (overwrite): the kernel, the row splits and the slab need are the plan's
// (gemm_tn_plan.h). site_a >= 0: an fp8 call on the per-layer 1-byte images, A = e5m2 gradient image [Mtot, N], B = e4m3
// activation image [Mtot, K] (lda / ldb in bytes), one dequantisation factor per operand site (shared by the L applications).
int weight_grad(PlbEngine* e, const void* A, int lda, int Ncols, const void* Bm, int ldb, int64_t Mtot, int N, int K,
                float* out, hipStream_t s, bool side_slab, int site_a, int site_b) {
  const bool f8 = site_a >= 0;
  PlbGemmTNPlan pl;
  if (plb_gemm_tn_plan(Mtot, Ncols, N, K, f8 ? PLB_TN_FP8 : PLB_TN_BF16, &pl)) return fail("weight_grad: no kernel takes the shape");
  PlbGemmTN t;
  memset(&t, 0, sizeof(t));
  t.A = static_cast<const bf16_t*>(A); t.lda = lda; t.Ncols = Ncols; t.B = static_cast<const bf16_t*>(Bm); t.ldb = ldb;
  t.Mtot = (int)Mtot; t.N = N; t.K = K; t.splits = pl.splits; t.rows_per_split = pl.rows_per_split;
  const bool direct = pl.direct != 0;   // every element is written exactly once: no slab, no reduce
  if (pl.slab_floats > (side_slab ? e->slab2_floats : e->slab_floats))
    return fail(f8 ? "weight_grad8: slab too small" : "weight_grad: slab too small");
  t.slab = direct ? out : e->at<float>(side_slab ? e->o_slab2 : e->o_slab);
  if (f8) { t.deq_a = f8_deq(e, f8_site(e, site_a, 0)); t.deq_b = f8_deq(e, f8_site(e, site_b, 0)); }
  if (pl.kernel == PLB_TN_SMALL) {
    TRY(plb_launch_gemm_tn(&t, s));   // (opens its own profiler scope)
  } else {
    const int tok = plb_prof_begin(f8 ? PLB_K_GEMM_TN_FP8 : PLB_K_GEMM_TN, s, pl.flops, 0.0);
    TRY(f8 ? plb_launch_gemm_tn_fp8(&t, s) : plb_launch_gemm_tn_big(&t, s));
    plb_prof_end(tok, s);
  }
  if (!direct) TRY(plb_launch_reduce_slabs(t.slab, t.splits, (size_t)N * K, out, 0, s));
  return 0;
}

// ---- layers in reverse --------------------------------------------------------------------------------------------------
// LayerNorm 2, FFN, LayerNorm 1 and dense of application l on all rows, down to dCtx (o_dctx). dy: the application's output
// gradient (read by the LayerNorm-2 backward of the last application only: for the others, the dX GEMM of application l+1
// ran it — attention_bwd_dx).
static int post_attention_bwd(PlbEngine* e, const Bwd& c, int l, const Slots& sl, const bf16_t* dy) {
  const int H = e->H, I = e->I, T = c.call.rw.T, Tp = (int)c.call.rw.Tp;
  hipStream_t s = c.call.s;
  const F8Site sDP(e, F8_DP, l), sDU(e, F8_DU, l), sDP1(e, F8_DP1, l);
  if (l == e->L - 1 && ln_bwd(e, ln2_slot(e, sl), c.prows, dy, sl.dpre2, T, Tp, c.f8 ? sl.dp8 : nullptr, sDP, s)) return 1;
  if (c.calib) TRY(plb_launch_amax(sl.dpre2, 1, (size_t)T, H, H, sDP.amax, s));
  // dU = (dpre2 · W2) ∘ gelu'(u)
  PlbGemmNT g = nt_desc(sl.dpre2, e->at<bf16_t>(e->o_w2T), Tp, I, H);
  g.aux = sl.u; g.ldaux = I; g.C = sl.du; g.ldc = I;
  if (c.du_rows > 0) g.colpart = sl.ducol;
  if (c.f8) f8_out(&g, sl.du8, I, sDU, 1);
  const F8Op ou = f8_op(sl.dp8, sDP, F8Weight(e, F8W_2T), 1);
  if (e->u_is_derivative) {   // what the forward of THIS call stashed; fp8: dU leaves as its e5m2 image alone
    if (e->tn8_call) g.C = nullptr;
    TRY(gemm_nt_any(&g, PLB_NT_GELUDBWD, c.f8 ? &ou : nullptr, s));
  } else {
    TRY(gemm_nt_any(&g, PLB_NT_GELUBWD, c.f8 ? &ou : nullptr, s));
  }
  if (c.calib) TRY(plb_launch_amax(sl.du, 1, (size_t)T, I, I, sDU.amax, s));
  // dA = dU · W1 + dpre2 is the gradient of LayerNorm 1's output. Fused: its backward runs in this GEMM's epilogue and dA
  // is never stored (dpre1 = the gradient of the LayerNorm's input, + the dgamma | dbeta | bias-gradient partials)
  g = nt_desc(sl.du, e->at<bf16_t>(e->o_w1T), Tp, H, I);
  g.res = sl.dpre2; g.ldr = H; g.C = e->at<bf16_t>(e->o_da); g.ldc = H;
  const F8Op oa = f8_op(sl.du8, sDU, F8Weight(e, F8W_1T), 1);
  if (gemm_ln_bwd(e, &g, c.f8 ? &oa : nullptr, c.fuse_b, ln1_slot(e, sl), c.prows, sl.dpre1, T, Tp, c.f8 ? sl.dp18 : nullptr,
                  sDP1, s))
    return 1;
  if (c.calib) TRY(plb_launch_amax(sl.dpre1, 1, (size_t)T, H, H, sDP1.amax, s));
  // dCtx = dpre1 · Wd
  g = nt_desc(sl.dpre1, e->at<bf16_t>(e->o_wdT), Tp, H, H);
  g.C = e->at<bf16_t>(e->o_dctx); g.ldc = H;
  const F8Op oc = f8_op(sl.dp18, sDP1, F8Weight(e, F8W_DT), 1);
  TRY(gemm_nt_any(&g, PLB_NT_PLAIN, c.f8 ? &oc : nullptr, s));
  return 0;
}

// ---- backward of the pruned last application: the compact part (LayerNorm 2, FFN, LayerNorm 1, dense) on the Mc
// masked rows — small-shape launches, the forward's compact activations at the start of this application's slots —
// then its gradients are scattered back to token rows (zeros elsewhere: that is what the full evaluation computes
// there) for the attention backward and the dX GEMM, which run on all rows: dCtx into o_dctx, dpre1 into o_da.
static int last_application_bwd_pruned(PlbEngine* e, const Bwd& c, const Slots& sl, const Prune* pr) {
  const int H = e->H, I = e->I, L = e->L, Mc = pr->Mc, n = pr->n;
  const int64_t Tp = c.call.rw.Tp;
  hipStream_t s = c.call.s;
  const F8Site sDP(e, F8_DP, L - 1), sDU(e, F8_DU, L - 1), sDP1(e, F8_DP1, L - 1);
  bf16_t* const dac = e->at<bf16_t>(e->o_da);       // dA of the compact rows, then (full) dpre1 scattered to token rows
  bf16_t* const dctxc = e->at<bf16_t>(e->o_dy0);    // dCtx of the compact rows (dy is not used by this application)
  bf16_t* const dctx = e->at<bf16_t>(e->o_dctx);
  if (ln_bwd(e, ln2_slot(e, sl), c.prows, e->at<bf16_t>(e->o_dhm), sl.dpre2, Mc, Mc, nullptr, F8Site(), s)) return 1;
  if (c.calib) TRY(plb_launch_amax(sl.dpre2, 1, (size_t)n, H, H, sDP.amax, s));
  PlbGemmNT g = nt_desc(sl.dpre2, e->at<bf16_t>(e->o_w2T), Mc, I, H);
  g.aux = sl.u; g.ldaux = I; g.C = sl.du; g.ldc = I;
  TRY(plb_launch_gemm_nt(&g, 2, 0, s));   // (the forward of this part kept u itself: act 1)
  if (c.calib) TRY(plb_launch_amax(sl.du, 1, (size_t)n, I, I, sDU.amax, s));
  if (c.du_rows > 0) {   // this application's block of ffn.bias partial rows: its column sums in row 0, zeros below
    TRY(plb_launch_colsum(sl.du, 1, (size_t)Mc, I, I, sl.ducol, I, 0, e->at<float>(e->o_scratch), 16, s));
    if (c.du_rows > 1) HIPTRY(hipMemsetAsync(sl.ducol + I, 0, (size_t)(c.du_rows - 1) * I * 4, s));
  }
  g = nt_desc(sl.du, e->at<bf16_t>(e->o_w1T), Mc, H, I);
  g.res = sl.dpre2; g.ldr = H; g.C = dac; g.ldc = H;
  if (gemm_ln_bwd(e, &g, nullptr, false, ln1_slot(e, sl), c.prows, sl.dpre1, Mc, Mc, nullptr, F8Site(), s)) return 1;
  if (c.calib) TRY(plb_launch_amax(sl.dpre1, 1, (size_t)n, H, H, sDP1.amax, s));
  if (e->tn8_call) {   // fp8 call: the compact gradient rows as e5m2 images for the stacked weight-gradient GEMMs
    const void* src[3] = {sl.dpre2, sl.du, sl.dpre1}; const int fl[3] = {3, 3, 3};
    const size_t nel[3] = {(size_t)Mc * H, (size_t)Mc * I, (size_t)Mc * H};
    const float* sc[3] = {sDP.scale, sDU.scale, sDP1.scale};
    uint8_t* dst[3] = {sl.dp8, sl.du8, sl.dp18};
    float* am[3] = {sDP.amax, sDU.amax, sDP1.amax};
    TRY(plb_launch_quantize_multi(3, src, fl, nel, sc, dst, am, s));
  }
  g = nt_desc(sl.dpre1, e->at<bf16_t>(e->o_wdT), Mc, H, H);
  g.C = dctxc; g.ldc = H;
  TRY(plb_launch_gemm_nt(&g, 0, 0, s));
  // back to token rows: dCtx and dpre1 are zero wherever no masked position sits
  HIPTRY(hipMemsetAsync(dctx, 0, (size_t)Tp * H * 2, s));
  TRY(plb_launch_scatter_rows(dctxc, H, pr->rows, n, H, dctx, H, s));
  HIPTRY(hipMemsetAsync(dac, 0, (size_t)Tp * H * 2, s));   // (dA has been consumed by the LayerNorm backward above)
  TRY(plb_launch_scatter_rows(sl.dpre1, H, pr->rows, n, H, dac, H, s));
  return 0;
}

// End of application l's backward, on all rows: the attention backward of dCtx (o_dctx; ctx = the forward's attention
// output), then dX = dQKV · Wqkv + res into dx — the gradient of LayerNorm 2's output of application l-1, whose backward
// follows (in the GEMM's epilogue where fused) and writes dpre2 of application l-1.
// d_in (or null): the caller's fp32 [B,S,H] gradient of hidden_states[l], the INPUT of application l (plb_encode_bwd_layers).
// It must enter before the fused LayerNorm backward of application l-1 runs in the GEMM's epilogue, i.e. through res:
// res' = res + d_in goes to o_da, which is dead here (dA of this application was consumed by its LayerNorm-1 backward; the
// pruned path uses the buffer the same way); res itself (dpre1: the weight-gradient GEMMs read it) is left alone.
static int attention_bwd_dx(PlbEngine* e, const Bwd& c, int l, const Slots& sl, bf16_t* ctx, const bf16_t* res,
                            bf16_t* dx, const float* d_in) {
  const Call& call = c.call;
  const Rows& rw = call.rw;
  const int H = e->H, T = rw.T;
  const int64_t Tp = rw.Tp;
  hipStream_t s = call.s;
  if (d_in) {
    bf16_t* const res_in = e->at<bf16_t>(e->o_da);
    HB_R(s, res, Tp * H * 2, "residual operand of the dX GEMM");
    HB_W(s, res_in, Tp * H * 2, "residual operand + the caller's gradient of this application's input");
    TRY(plb_launch_add_row_grad(res, d_in, call.lengths, rw.row_start, call.B, call.S, H, (int)Tp, res_in, s));
    res = res_in;
  }
  const F8Site sDQ(e, F8_DQ, l);
  PlbAttn at = attn_desc(e, call, sl);
  at.ctx = ctx;
  at.dctx = e->at<bf16_t>(e->o_dctx); at.lddctx = H; at.delta = e->at<float>(e->o_delta); at.dqkv = sl.dqkv; at.lddqkv = 3 * H;
  at.colpart = sl.qkvcol; at.colpart_accumulate = 0;
  if (c.f8) {   // dQKV leaves as its e5m2 image (alone, once the weight gradient reads images too)
    at.dqkv8 = sl.dq8; at.lddqkv8 = 3 * H; at.dqkv_scale = sDQ.scale; at.dqkv_amax = sDQ.amax;
    if (e->tn8_call) at.dqkv = nullptr;
  }
  // rows of a packed slot that no launch of this call writes (the plan's unwritten_rows) and the weight-gradient GEMMs
  // read: zeros (their true value: no token sits there), not what an earlier call left — and their e5m2 image likewise: a
  // stale byte there can be a NaN encoding, and 0 x NaN in the stacked weight-gradient GEMM is NaN
  if (attn_plan(at).unwritten_rows) {
    if (at.dqkv) HIPTRY(hipMemsetAsync(sl.dqkv, 0, (size_t)T * 3 * H * 2, s));
    if (at.dqkv8) HIPTRY(hipMemsetAsync(sl.dq8, 0, (size_t)T * 3 * H, s));
  }
  TRY(plb_launch_attn_bwd(&at, s));
  if (Tp > T) {
    if (at.dqkv) HIPTRY(hipMemsetAsync(sl.dqkv + (int64_t)T * 3 * H, 0, (size_t)(Tp - T) * 3 * H * 2, s));
    if (c.f8) HIPTRY(hipMemsetAsync(sl.dq8 + (int64_t)T * 3 * H, 0, (size_t)(Tp - T) * 3 * H, s));
  }
  if (c.calib) TRY(plb_launch_amax(sl.dqkv, 1, (size_t)T, 3 * H, 3 * H, sDQ.amax, s));
  PlbGemmNT g = nt_desc(sl.dqkv, e->at<bf16_t>(e->o_wqkvT), Tp, H, 3 * H);
  g.res = res; g.ldr = H; g.C = dx; g.ldc = H;
  const F8Op ox = f8_op(sl.dq8, sDQ, F8Weight(e, F8W_QKVT), 1);
  if (l == 0) {   // the gradient of the embeddings' map-in output: the tail takes it
    TRY(gemm_nt_any(&g, PLB_NT_PLAIN, c.f8 ? &ox : nullptr, s));
    return 0;
  }
  const Slots below = slots(e, Tp, call.B, call.S, l - 1, true, c.prows, c.du_rows);
  return gemm_ln_bwd(e, &g, c.f8 ? &ox : nullptr, c.fuse_b, ln2_slot(e, below), c.prows, below.dpre2, T, (int)Tp,
                     c.f8 ? below.dp8 : nullptr, F8Site(e, F8_DP, l - 1), s);
}

// The layer loop of the backward. dy: in, the output gradient of the last application; out, the gradient of the map-in
// output. *du_rows: the ffn.bias partial rows per application it left for the tail.
// fp8 mode: every dX GEMM reads e5m2 images of its gradient operand — dU = dpre2·W2 and dA = dU·W1 (+ LayerNorm 1
// backward), dCtx = dpre1·Wd, dX = dQKV·Wqkv (+ LayerNorm 2 backward of the layer below) — written by the launch that
// produces the gradient (fused LayerNorm-backward / gelu-backward epilogues, the attention-backward kernels, the
// standalone LayerNorm backward), one image per layer for the weight-gradient GEMMs at the end.
int encoder_bwd(PlbEngine* e, const Call& call, const Prune* pr, bf16_t** dy, int* du_rows, const float* const* d_below) {
  const int I = e->I, L = e->L;
  Bwd c = {call};
  const int Tp = (int)call.rw.Tp;
  c.f8 = f8_call(e, Tp, true);
  c.calib = e->fp8_on && !c.f8;
  // ffn.bias gradient from the dU GEMM's epilogue: the partial rows its launch writes (none on the small kernel: the tail
  // then sums dU itself)
  const int ops = c.f8 ? PLB_NT_FP8_E5M2 : PLB_NT_BF16;
  const PlbGemmNTPlan du = nt_plan(Tp, I, e->H, e->u_is_derivative ? PLB_NT_GELUDBWD : PLB_NT_GELUBWD, ops, PLB_NT_COLPART);
  c.du_rows = du.rc ? 0 : du.colpart_rows;
  // LayerNorm backward inside the dX GEMM that produces its output gradient (gemm_ln.hip). Rows of partials per layer:
  // the fused launch's (the one standalone launch left — LayerNorm 2 of the last application, whose output gradient comes
  // from the head — then uses as many blocks), else the LayerNorm kernel's block count.
  c.fuse_b = ln_fusable(e, Tp, 2, c.f8);
  c.prows = c.fuse_b ? nt_plan(Tp, e->H, e->H, PLB_NT_LNBWD, ops).colpart_rows : e->ln_blocks;
  const int qkv_rows = qkvcol_rows(e, call.B, call.S);
  if (c.du_rows > e->ducol_rows || c.prows > e->part_rows || qkv_rows > e->qkvcol_rows)
    return fail("encoder_bwd: the plans write %d ffn.bias, %d LayerNorm and %d Q/K/V bias partial rows per application, %d, %d and %d are reserved",
                c.du_rows, c.prows, qkv_rows, e->ducol_rows, e->part_rows, e->qkvcol_rows);
  e->part_rows_used = c.prows;
  bf16_t* dx = e->at<bf16_t>(e->o_dy1);
  for (int l = L - 1; l >= 0; --l) {
    const Slots sl = slots(e, call.rw.Tp, call.B, call.S, l, true, c.prows, c.du_rows);
    if (pr && l == L - 1) {
      // the attention output of all rows is the backward temporary o_dy1 (the ctx slot holds the compact rows)
      if (last_application_bwd_pruned(e, c, sl, pr)) return 1;
      if (attention_bwd_dx(e, c, l, sl, e->at<bf16_t>(e->o_dy1), e->at<bf16_t>(e->o_da), dx, nullptr)) return 1;
    } else {
      if (post_attention_bwd(e, c, l, sl, *dy)) return 1;
      if (attention_bwd_dx(e, c, l, sl, sl.ctx, sl.dpre1, dx, d_below ? d_below[l] : nullptr)) return 1;
    }
    bf16_t* tmp = *dy; *dy = dx; dx = tmp;
  }
  *du_rows = c.du_rows;
  return 0;
}
