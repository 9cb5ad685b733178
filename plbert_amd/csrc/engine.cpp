// C-ABI engine of the PL-BERT hot path (include/plbert.h): owns the workspace layout and the
// launch sequence of one forward / loss+backward / AdamW step.  No device allocation, no host
// synchronisation: everything is enqueued on the caller's HIP stream, so a caller may capture a
// step into a hipGraph.
//
// Memory plan (sized for 288 GB HBM3E): every activation of all L applications of the shared layer
// is stashed in bf16 as [L][Tp][width] (Tp = tokens rounded up to 128), and so is every gradient
// that feeds a weight gradient.  Weight sharing then turns the 12 per-layer dW products of the
// reference's autograd into ONE token-major GEMM per weight with reduction length L*Tp, which is
// split over the grid into fp32 slabs and reduced in fixed order (deterministic, no atomics).
//
// This unit: the parameter layout, the workspace carve (plb_create / plb_bind), the weight copies (plb_sync_weights;
// sync_transposes also ends every update of engine_optim.cpp) and the entry points that are one launch. Only writer of
// PlbEngine's layout and capacity block, the workspace offsets, the bound buffers, the side stream and its events and
// tok_pad_zeroed; tok_steps is written here (plb_set_token_head_steps), by plb_status and by the updates of engine_optim.cpp.
// The other units: engine_prof.cpp, engine_comm.cpp, engine_fp8.cpp, engine_layers.cpp, engine_calls.cpp, engine_eval.cpp,
// engine_optim.cpp.
#include <stdarg.h>

#include <new>

#include "engine_internal.h"

static thread_local char g_err[512] = "";
int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}
extern "C" const char* plb_last_error(void) { return g_err; }

static void layout_params(PlbEngine* e) {
  const int64_t V = e->V, E = e->E, H = e->H, I = e->I, P = e->P, NP = e->NP, NT = e->NT;
  int64_t sz[PLB_NPARAM];
  sz[PLB_WORD_EMB] = V * E; sz[PLB_POS_EMB] = P * E; sz[PLB_TYPE_EMB] = (int64_t)e->c.type_vocab_size * E;
  sz[PLB_EMB_LN_W] = E; sz[PLB_EMB_LN_B] = E;
  sz[PLB_MAP_W] = H * E; sz[PLB_MAP_B] = H;
  sz[PLB_LN2_W] = H; sz[PLB_LN2_B] = H;
  sz[PLB_Q_W] = sz[PLB_K_W] = sz[PLB_V_W] = H * H;
  sz[PLB_Q_B] = sz[PLB_K_B] = sz[PLB_V_B] = H;
  sz[PLB_DENSE_W] = H * H; sz[PLB_DENSE_B] = H;
  sz[PLB_LN1_W] = H; sz[PLB_LN1_B] = H;
  sz[PLB_FFN_W] = I * H; sz[PLB_FFN_B] = I;
  sz[PLB_FFNO_W] = H * I; sz[PLB_FFNO_B] = H;
  sz[PLB_HEAD_W] = NP * H; sz[PLB_HEAD_B] = NP;
  sz[PLB_POOL_W] = H * H; sz[PLB_POOL_B] = H;
  sz[PLB_TOK_W] = NT * H; sz[PLB_TOK_B] = NT;
  int64_t off = 0;
  for (int i = 0; i < PLB_NPARAM; ++i) {
    e->poff[i] = off;
    e->psize[i] = sz[i];
    off += sz[i];
    if (i == PLB_HEAD_B) e->ptrain = off;
  }
  e->ptotal = off;
}

namespace {
struct Carve {  // bump allocator over the workspace, 256-B aligned regions
  int64_t off = 0;
  int64_t take(int64_t bytes) {
    int64_t o = off;
    off = rup(off + bytes, 256);
    return o;
  }
};
}  // namespace

// fp32 floats of slab a weight-gradient GEMM of this shape needs (gemm_tn_plan.h): splits * N * K. A launch that writes
// its output directly (one split: the token head) needs none, but its output's worth stays reserved as it always was, so
// the workspace layout does not move.
static int64_t tn_slab_floats(int64_t Mtot, int Ncols, int N, int K) {
  PlbGemmTNPlan pl;
  if (plb_gemm_tn_plan(Mtot, Ncols, N, K, PLB_TN_BF16, &pl)) return 0;
  return pl.direct ? (int64_t)N * K : pl.slab_floats;
}

extern "C" int plb_create(const PlbConfig* cfg, PlbEngine** out) {
  if (!cfg || !out) return fail("plb_create: null argument");
  const PlbConfig& c = *cfg;
  if (c.hidden_size != c.num_attention_heads * 64) return fail("plb_create: head_dim must be 64 (hidden %d, heads %d)", c.hidden_size, c.num_attention_heads);
  if (c.embedding_size % 64 || c.embedding_size > 256) return fail("plb_create: embedding_size must be a multiple of 64, <= 256");
  if (c.hidden_size % 128 || c.hidden_size > 1024) return fail("plb_create: hidden_size must be a multiple of 128, <= 1024");
  if (c.intermediate_size % 128) return fail("plb_create: intermediate_size must be a multiple of 128");
  if (c.num_phonemes < 4 || c.num_phonemes % 4 || c.num_phonemes > 256) return fail("plb_create: num_phonemes must be a multiple of 4 in [4,256]");
  if (c.num_tokens < 0 || c.num_tokens % 4) return fail("plb_create: num_tokens must be a non-negative multiple of 4");
  if (c.max_seq < 1 || c.max_seq > c.max_position_embeddings) return fail("plb_create: max_seq must be in [1, max_position_embeddings]");
  if (c.max_batch < 1 || c.num_hidden_layers < 1 || c.vocab_size < 1 || c.type_vocab_size < 1) return fail("plb_create: bad sizes");
  PlbEngine* e = new (std::nothrow) PlbEngine();
  if (!e) return fail("plb_create: out of host memory");
  e->c = c;
  e->E = c.embedding_size; e->H = c.hidden_size; e->I = c.intermediate_size; e->L = c.num_hidden_layers;
  e->NH = c.num_attention_heads; e->V = c.vocab_size; e->P = c.max_position_embeddings;
  e->NP = c.num_phonemes; e->NT = c.num_tokens;
  layout_params(e);
  const int64_t E = e->E, H = e->H, I = e->I, L = e->L;
  const int64_t T = (int64_t)c.max_batch * c.max_seq;
  const int64_t Tp = rup(T, 128);
  e->infer = c.inference_only != 0;
  const bool tr = !e->infer;
  const int64_t Ls = tr ? L : 1;  // layers of activations kept
  e->Tcap = Tp;
  e->NMcap = Tp;
  // LayerNorm-backward partial rows (tools/ln_bench.py --blocks): 512 workgroups are 22 % faster than 1024 at H = 1024
  // (12.1 vs 15.5 us standalone) and level at H = 768 (2 % faster alone, +-0.01 ms inside the step, where they also halve
  // the side stream's pass over the partials); PLBERT_LN_BLOCKS overrides
  e->ln_blocks = 512;
  if (const char* v = getenv("PLBERT_LN_BLOCKS")) { const int n = atoi(v); if (n >= 64 && n <= 4096) e->ln_blocks = n; }
  e->emb_blocks = 2048;
  // LayerNorm in the GEMM epilogues (gemm_ln.hip): PLBERT_LN_FUSE = off | fwd | bwd | both (default both)
  if (const char* v = getenv("PLBERT_LN_FUSE"))
    e->ln_fuse = !strcmp(v, "off") ? 0 : !strcmp(v, "fwd") ? 1 : !strcmp(v, "bwd") ? 2 : 3;
  e->part_rows = e->ln_blocks > (int)(2 * Tp / 128) ? e->ln_blocks : (int)(2 * Tp / 128);
  if (const char* v = getenv("PLBERT_GELU_STASH")) e->gelu_dstash_on = strcmp(v, "u") != 0;
  if (const char* v = getenv("PLBERT_FP8_TN")) e->fp8_tn = strcmp(v, "0") != 0;
  if (const char* v = getenv("PLBERT_HB_AUDIT")) e->hb.on = strcmp(v, "0") != 0;
  Carve cv;
  // bf16 weight copies: the flat copy (+ slack so 128-row B tiles never leave the buffer) and transposes
  e->o_wbf = cv.take((e->ptotal + 256 * (H > I ? H : I)) * 2);
  if (tr) {
    e->o_wqkvT = cv.take(rup(H, 128) * 3 * H * 2);
    e->o_wdT = cv.take(rup(H, 128) * H * 2);
    e->o_w1T = cv.take(rup(H, 128) * I * 2);
    e->o_w2T = cv.take(rup(I, 128) * H * 2);
    e->o_wpT = cv.take(rup(H, 128) * 256 * 2);
    e->o_winT = cv.take(rup(E, 128) * H * 2);
  }
  // forward stash (training: every layer; inference: one layer, two ping-pong slots of x)
  e->o_e = cv.take(Tp * E * 2);
  e->o_x = cv.take((tr ? L + 1 : 2) * Tp * H * 2);
  e->o_qkv = cv.take(Ls * Tp * 3 * H * 2);
  e->o_ctx = cv.take(Ls * Tp * H * 2);
  e->o_pre1 = cv.take(Ls * Tp * H * 2);
  e->o_a = cv.take(Ls * Tp * H * 2);
  e->o_u = cv.take(Ls * Tp * I * 2);
  e->o_g = cv.take(Ls * Tp * I * 2);
  e->o_pre2 = cv.take(Ls * Tp * H * 2);
  const int64_t stat = (int64_t)c.max_batch * e->NH * c.max_seq * 4;
  e->o_lse = cv.take(Ls * stat);
  e->o_mean1 = cv.take(Ls * Tp * 4); e->o_rstd1 = cv.take(Ls * Tp * 4);
  e->o_mean2 = cv.take(Ls * Tp * 4); e->o_rstd2 = cv.take(Ls * Tp * 4);
  // exchange granules of the LayerNorm epilogues: [Tp/128][nbn][nbn][128][2] x 8 B, nbn <= 4 column tiles; zero between launches
  e->lnx_bytes = (Tp / 128) * 16 * 128 * 2 * 8;
  e->o_lnx = cv.take(e->lnx_bytes);
  e->o_lnerr = cv.take(256);
  if (tr) {
    e->o_delta = cv.take(stat);
    // backward stash (operands of the batched dW GEMMs)
    e->o_dqkv = cv.take(L * Tp * 3 * H * 2);
    e->o_dpre1 = cv.take(L * Tp * H * 2);
    e->o_du = cv.take(L * Tp * I * 2);
    e->o_dpre2 = cv.take(L * Tp * H * 2);
    e->o_dy0 = cv.take(Tp * H * 2); e->o_dy1 = cv.take(Tp * H * 2);
    e->o_da = cv.take(Tp * H * 2); e->o_dctx = cv.take(Tp * H * 2);
    e->o_de = cv.take(Tp * E * 2);
  }
  // loss rows
  const int64_t NM = e->NMcap;
  e->o_hm = cv.take(NM * H * 2);
  e->o_logm = cv.take(NM * 256 * 4);
  e->o_dlog = cv.take(NM * 256 * 2);
  e->o_rows = cv.take(NM * 4); e->o_tgt = cv.take(NM * 4); e->o_w = cv.take(NM * 4); e->o_lrows = cv.take(NM * 4);
  // (plb_masked_report reads o_logm and o_tgt — and o_tpmax, o_ttl, o_tw below — as the last loss call left them: nothing but
  // the heads of a loss call writes those regions: phoneme_head, token_head and the ce_prepare launch of loss_impl in
  // engine_calls.cpp.)
  if (tr) {
    e->o_dhm = cv.take(NM * H * 2);
    // reductions
    // the slab of the weight-gradient GEMMs: the largest need over the four layer weights (all L applications stacked),
    // map-in, the phoneme head (reads 256 columns, stores NP rows) and the token head
    int64_t slab = 0;
    {
      const int64_t Mtot = L * Tp;
      const int ntp = (int)rup(e->NT, 256);
      const int shapes[7][3] = {{(int)(3 * H), (int)(3 * H), (int)H}, {(int)H, (int)H, (int)H}, {(int)I, (int)I, (int)H}, {(int)H, (int)H, (int)I},
                                {(int)H, (int)H, (int)E}, {256, e->NP, (int)H}, {ntp, ntp, (int)H}};   // Ncols, N, K
      for (int i = 0; i < (e->NT ? 7 : 6); ++i) {
        const int64_t f = tn_slab_floats(i < 4 ? Mtot : Tp, shapes[i][0], shapes[i][1], shapes[i][2]);
        if (f > slab) slab = f;
      }
    }
    e->slab_floats = slab;
    e->o_slab = cv.take(slab * 4);
    e->o_part1 = cv.take(L * e->part_rows * 3 * H * 4);  // per LN-backward block: dgamma | dbeta | column sums of dx
    e->o_part2 = cv.take(L * e->part_rows * 3 * H * 4);
    e->o_parte = cv.take((int64_t)e->emb_blocks * 2 * E * 4);
    e->o_dxe = cv.take(Tp * E * 4);
    e->ducol_rows = (int)(2 * Tp / 128);   // (2 per row tile of the narrowest pipeline tile, 128 rows)
    e->o_ducol = cv.take(L * e->ducol_rows * I * 4);  // column-sum partials of dU from the GEMM epilogue
    e->qkvcol_rows = qkvcol_rows(e, c.max_batch, c.max_seq);
    // ... of dQKV from the attention-backward stores, one set per application: the kernels only STORE their partial rows
    // (summing over the applications in place made every wave end on a global read-modify-write: +0.19 ms per step)
    e->o_qkvcol = cv.take((int64_t)L * e->qkvcol_rows * 3 * H * 4);
    e->o_scratch = cv.take(512 * (3 * H > I ? 3 * H : I) * 4);  // colsum partials: up to 512 row splits
    e->o_scratch2 = cv.take(512 * (3 * H > I ? 3 * H : I) * 4);
    e->slab2_floats = tn_slab_floats(Tp, (int)H, (int)H, (int)E);   // map-in on the side stream
    e->o_slab2 = cv.take(e->slab2_floats * 4);
  }
  if (e->NT) {
    const int64_t NTp = rup(e->NT, 256);
    e->NTp = (int)NTp;
    e->o_bt = cv.take(NTp * 4);
    e->o_tlrows = cv.take(Tp * 4);
    e->o_tpmax = cv.take(Tp * (NTp / 256) * 4);
    e->o_tpsum = cv.take(Tp * (NTp / 256) * 4);
    e->o_ttl = cv.take(Tp * 4); e->o_tlse = cv.take(Tp * 4); e->o_tw = cv.take(Tp * 4);
    e->o_ttgt = cv.take(Tp * 8);
    e->o_tloss = cv.take(256);
    // zero-padded [NTp,H] bf16 copy of the token head for the fused GEMM + CE passes (the flat copy's rows past NT
    // belong to the next tensor)
    if (tr) {
      e->o_wtT = cv.take(rup(H, 128) * NTp * 2);
      e->o_tdl = cv.take(Tp * NTp * 2);
      e->o_tscr = cv.take(32 * NTp * 4);
      e->tcolp_rows = (int)(2 * (Tp / 128));
      e->o_tcolp = cv.take(e->tcolp_rows * NTp * 4);
      e->o_tgrad = cv.take(NTp * H * 4);
    }
  }
  // fp8 mode: 1-byte operand images of every layer kept (training: all of them, for the weight gradients) and the weight copies
  e->o_x8 = cv.take(Ls * Tp * H); e->o_a8 = cv.take(Ls * Tp * H); e->o_g8 = cv.take(Ls * Tp * I); e->o_c8 = cv.take(Ls * Tp * H);
  e->o_wq8 = cv.take(rup(3 * H, 128) * H + 256 * H);
  e->o_wd8 = cv.take(rup(H, 128) * H + 256 * H);
  e->o_w18 = cv.take(rup(I, 128) * H + 256 * H);
  e->o_w28 = cv.take(rup(H, 128) * I + 256 * I);
  if (tr) {
    e->o_dp8 = cv.take(L * Tp * H); e->o_du8 = cv.take(L * Tp * I); e->o_dp18 = cv.take(L * Tp * H); e->o_dq8 = cv.take(L * Tp * 3 * H);
    e->o_w2T8 = cv.take(rup(I, 128) * H + 256 * H);
    e->o_w1T8 = cv.take(rup(H, 128) * I + 256 * I);
    e->o_wqT8 = cv.take(rup(H, 128) * 3 * H + 256 * 3 * H);
    e->o_wdT8 = cv.take(rup(H, 128) * H + 256 * H);
  }
  e->f8n = 8 * (int)L + 8;
  e->o_f8amax = cv.take((int64_t)e->f8n * 64 * 16 * 4); e->o_f8scale = cv.take(e->f8n * 4); e->o_f8deq = cv.take(e->f8n * 4);
  e->o_f8stats = cv.take(8 * 8 * 4);   // per operand site: maxima history, clamped-call count, worst overshoot (operand_images.hip: fp8_scales_kernel)
  // What plb_masked_report itself writes: regions of its own, carved last (every other region keeps its offset) — the ranks
  // and row losses of a report whose caller takes none, plb_launch_token_top1's per-block counts.
  e->o_rep_rank = cv.take(NM * 4); e->o_rep_nll = cv.take(NM * 4);
  if (e->NT) e->o_rep_tok = cv.take((Tp / 4) * 2 * 4);
  // What plb_token_report itself writes, carved behind everything else for the same reason. Proportional to the row
  // capacity, not to the vocabulary: 4 + 4 B of row list and target and plb_token_topk_scratch_bytes (16 strips x (8
  // candidates x 8 B + 16 B of statistics) + 3 counts per 4 rows) = 1291 B per row of Tcap.
  if (e->NT) {
    e->o_tr_rows = cv.take(Tp * 4); e->o_tr_tgt = cv.take(Tp * 4);
    e->o_tr_scratch = cv.take((int64_t)plb_token_topk_scratch_bytes((int)Tp));
  }
  // The partial rows of plb_launch_embed_inputs_scatter (a backward with position_ids / token_type_ids), carved last like the
  // regions above: one [max_position_embeddings + type_vocab_size][E] block of floats per 512 positions of the capacity.
  if (tr) e->o_embpart = cv.take((int64_t)plb_embed_inputs_part_floats((int)Tp, e->P, c.type_vocab_size, (int)E) * 4);
  // The key-mask words of a plb_*_masked call (key_mask.hip), carved last like the regions above: two words per 64 keys.
  e->o_keywords = cv.take((int64_t)c.max_batch * 2 * ((c.max_seq + 63) / 64) * 4);
  // dpre and dh0 of the pooler backward (plb_encode_bwd_pooled; pooler_bwd.hip), carved last like the regions above
  if (tr) { e->o_pool_dpre = cv.take((int64_t)c.max_batch * H * 4); e->o_pool_dh0 = cv.take((int64_t)c.max_batch * H * 4); }
  e->ws_bytes = cv.off;
  *out = e;
  return 0;
}

extern "C" void plb_destroy(PlbEngine* e) {
  if (!e) return;
  (void)plb_comm_destroy(e);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->side) (void)hipStreamDestroy(e->side);
  if (e->host_err) (void)hipHostFree(e->host_err);
  for (auto& t : e->trace) { (void)hipEventDestroy(t.released); (void)hipEventDestroy(t.done); }
  for (auto ev : e->trace_pool) (void)hipEventDestroy(ev);
  for (auto ev : {e->tr_call0, e->tr_tail0, e->tr_tail1}) if (ev) (void)hipEventDestroy(ev);
  delete e;
}

extern "C" int plb_param_layout(const PlbEngine* e, int64_t* offsets, int64_t* sizes, int64_t* total, int64_t* trainable) {
  if (!e) return fail("plb_param_layout: null engine");
  for (int i = 0; i < PLB_NPARAM; ++i) {
    if (offsets) offsets[i] = e->poff[i];
    if (sizes) sizes[i] = e->psize[i];
  }
  if (total) *total = e->ptotal;
  if (trainable) *trainable = e->ptrain;
  return 0;
}

extern "C" int64_t plb_workspace_bytes(const PlbEngine* e) { return e ? e->ws_bytes : -1; }

extern "C" int plb_bind(PlbEngine* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* workspace,
                        int64_t workspace_bytes) {
  if (!e || !params || !workspace) return fail("plb_bind: null argument");
  if (workspace_bytes < e->ws_bytes) return fail("plb_bind: workspace too small (%lld < %lld)", (long long)workspace_bytes, (long long)e->ws_bytes);
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return fail("plb_bind: buffers must be 16-byte aligned");
  if ((uintptr_t)workspace & 255) return fail("plb_bind: workspace must be 256-byte aligned");
  e->params = params; e->grads = grads; e->m = exp_avg; e->v = exp_avg_sq;
  e->ws = (char*)workspace;
  e->rep_valid = false;   // (plb_masked_report: what a loss call left lies in the workspace bound before)
  drop_final(e, "plb_bind bound a workspace since");
  if (!e->host_err) {  // once, outside any launch sequence
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess && h) {
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
        e->host_err = (unsigned int*)h;
        e->host_err_dev = (unsigned int*)d;
        *e->host_err = 0;
      } else {
        (void)hipHostFree(h);
      }
    }
    if (!e->host_err) return fail("plb_bind: cannot allocate the pinned status word");
  }
  if (!e->side && grads && !getenv("PLBERT_NO_SIDE_STREAM")) {  // created once, outside any launch sequence (a step may be graph-captured)
    // (default priority: at the highest one the step measured the same, 10.20-10.22 ms either way)
    if (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess) e->side = nullptr;
    if (e->side && (hipEventCreateWithFlags(&e->ev_fork, kStreamOrderEvent) != hipSuccess ||
                    hipEventCreateWithFlags(&e->ev_join, kStreamOrderEvent) != hipSuccess)) {
      (void)hipStreamDestroy(e->side);
      e->side = nullptr;
    }
  }
  return 0;
}

int sync_transposes(PlbEngine* e, hipStream_t s, bool exact_fp8) {
  const int H = e->H, I = e->I, E = e->E;

  if (e->NT) {  // bias of the token head padded to NTp columns (fused GEMM + CE passes)
    if (!e->tok_pad_zeroed) HIPTRY(hipMemsetAsync(e->at<float>(e->o_bt), 0, (size_t)e->NTp * 4, s));
    HIPTRY(hipMemcpyAsync(e->at<float>(e->o_bt), e->par(PLB_TOK_B), (size_t)e->NT * 4, hipMemcpyDeviceToDevice, s));
  }
  if (e->infer) {  // the transposed copies serve the backward only
    e->tok_pad_zeroed = true;
    if (e->fp8_on) return fp8_quantize_weights(e, s, exact_fp8 || e->fp8_wstale);
    return 0;
  }
  // fused QKV [3H,H] -> [H,3H]; the three tensors are adjacent in the flat buffer
  // (one launch for all of them: each is a few microseconds of work behind 5 us of launch latency)
  const float* tsrc[8] = {e->par(PLB_Q_W), e->par(PLB_DENSE_W), e->par(PLB_FFN_W), e->par(PLB_FFNO_W), e->par(PLB_HEAD_W),
                          e->par(PLB_MAP_W)};
  bf16_t* tdst[8] = {e->at<bf16_t>(e->o_wqkvT), e->at<bf16_t>(e->o_wdT), e->at<bf16_t>(e->o_w1T), e->at<bf16_t>(e->o_w2T),
                     e->at<bf16_t>(e->o_wpT), e->at<bf16_t>(e->o_winT)};
  int tR[8] = {3 * H, H, I, H, e->NP, H}, tC[8] = {H, H, H, I, H, E}, tld[8] = {3 * H, H, I, H, 256, H};
  int nt = 6;
  if (e->NT) {  // transposed weight of the token head, padded to NTp columns
    if (!e->tok_pad_zeroed) HIPTRY(hipMemsetAsync(e->at<bf16_t>(e->o_wtT), 0, (size_t)rup(H, 128) * e->NTp * 2, s));
    tsrc[nt] = e->par(PLB_TOK_W); tdst[nt] = e->at<bf16_t>(e->o_wtT); tR[nt] = e->NT; tC[nt] = H; tld[nt] = e->NTp;
    ++nt;
  }
  TRY(plb_launch_transpose_cast_multi(nt, tsrc, tR, tC, tdst, tld, s));
  e->tok_pad_zeroed = true;
  if (e->fp8_on) return fp8_quantize_weights(e, s, exact_fp8 || e->fp8_wstale);
  return 0;
}

extern "C" int plb_sync_weights(PlbEngine* e, void* stream) {
  if (!e || !e->ws) return fail("plb_sync_weights: engine not bound");
  drop_stash(e, "plb_sync_weights refreshed the compute copies since");
  drop_final(e, "plb_sync_weights refreshed the compute copies since: the hidden state is that of the weights before");
  end_accum_window(e, "plb_sync_weights refreshed the compute copies");
  hipStream_t s = (hipStream_t)stream;
  TRY(plb_launch_cast_bf16(e->params, e->at<bf16_t>(e->o_wbf), (size_t)e->ptotal, s));
  return sync_transposes(e, s);
}

extern "C" int plb_pooler(PlbEngine* e, const float* hidden, int32_t B, int32_t S, float* pooled, void* stream) {
  if (!e || !e->ws) return fail("plb_pooler: engine not bound");
  if (!hidden || !pooled || B < 1 || S < 1) return fail("plb_pooler: bad argument");
  TRY(plb_launch_pooler(hidden, B, S, e->H, e->par(PLB_POOL_W), e->par(PLB_POOL_B), pooled, (hipStream_t)stream));
  return 0;
}

// The plan of a token-packed call, on the host (include/plbert.h). Slots start on multiples of 128 — the row tile of the
// attention kernels, so a sample's tiles are those of the padded call — and the row count is rounded up to the coarsest of
// 1024 (LayerNorm in the GEMM epilogues) / 256 (gelu' stash) / 128 that still leaves fewer rows than the padded call.
#ifndef PLB_PACK_GRAN_MAX
#define PLB_PACK_GRAN_MAX 1024   // A/B builds: 256 / 128 leave out the coarser roundings
#endif
extern "C" int plb_packing_plan(const int32_t* lengths, int32_t B, int32_t S, int32_t* row_start, int32_t* rows,
                                int32_t* used) {
  if (!lengths || !row_start || !rows || !used) return fail("plb_packing_plan: null argument");
  if (B < 1 || S < 1 || (int64_t)B * S > (int64_t)1 << 30) return fail("plb_packing_plan: bad shape %d x %d", B, S);
  const int64_t padded = rup((int64_t)B * S, 128);
  int64_t at = 0;
  bool full = true;
  for (int b = 0; b < B; ++b) {
    const int len = lengths[b] < 1 ? 1 : (lengths[b] > S ? S : lengths[b]);
    full = full && len == S;
    at += rup(len, 128);
  }
  const int64_t gran = (PLB_PACK_GRAN_MAX >= 1024 && rup(at, 1024) < padded) ? 1024
                       : (PLB_PACK_GRAN_MAX >= 256 && rup(at, 256) < padded) ? 256 : 128;
  if (full || rup(at, gran) >= padded) {   // nothing to gain: the plan IS the padded layout, the engine runs the padded path
    for (int b = 0; b <= B; ++b) row_start[b] = b * S;
    *rows = (int32_t)padded; *used = B * S;
    return 0;
  }
  at = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lengths[b] < 1 ? 1 : (lengths[b] > S ? S : lengths[b]);
    row_start[b] = (int32_t)at;
    at += rup(len, 128);
  }
  row_start[B] = (int32_t)at;
  *used = (int32_t)at;
  *rows = (int32_t)rup(at, gran);
  return 0;
}

extern "C" int plb_last_application_rows(const PlbEngine* e, int64_t* rows, int64_t* of) {
  if (!e) return fail("plb_last_application_rows: null engine");
  if (rows) *rows = e->last_app_rows[0];
  if (of) *of = e->last_app_rows[1];
  return 0;
}

extern "C" int plb_last_call_rows(const PlbEngine* e, int64_t* rows, int64_t* of) {
  if (!e) return fail("plb_last_call_rows: null engine");
  if (rows) *rows = e->last_exec_rows[0];
  if (of) *of = e->last_exec_rows[1];
  return 0;
}

// Host state only: nothing on the device changes and a live plb_encode stash stays live.
extern "C" int plb_set_packed_dual(PlbEngine* e, int32_t on) {
  if (!e) return fail("plb_set_packed_dual: null engine");
  e->packed_dual = on != 0;
  return 0;
}
extern "C" int plb_set_packed_fp8(PlbEngine* e, int32_t on) {
  if (!e) return fail("plb_set_packed_fp8: null engine");
  e->packed_fp8 = on != 0;
  return 0;
}

extern "C" int32_t plb_token_head_steps(const PlbEngine* e) { return e ? e->tok_steps : -1; }
extern "C" int plb_set_token_head_steps(PlbEngine* e, int32_t steps) {
  if (!e || steps < 0) return fail("plb_set_token_head_steps: bad argument");
  e->tok_steps = steps;
  return 0;
}

extern "C" int plb_apply_mask(const int64_t* ids, const int32_t* sample_off, const int32_t* word_off,
                              const int32_t* word_begin, const int32_t* word_len, const int8_t* action, const int64_t* repl,
                              const int64_t* word_token, int64_t sep_token, const int32_t* crop_start, int32_t B, int32_t S,
                              int32_t mask_id, int64_t* labels, int64_t* masked, int64_t* tokens, int32_t* lengths_out,
                              int32_t* idx_offsets, int32_t* idx_flat, int32_t* scratch, void* stream) {
  if (!ids || !sample_off || !word_off || !word_begin || !word_len || !action || !repl || !crop_start || !labels || !masked ||
      !lengths_out || !idx_offsets || !idx_flat || !scratch)
    return fail("plb_apply_mask: null argument");
  if ((tokens != nullptr) != (word_token != nullptr)) return fail("plb_apply_mask: tokens and word_token go together");
  if (S < 1 || S > 1024 || B < 1 || B > 1024) return fail("plb_apply_mask: needs 1 <= S <= 1024, 1 <= B <= 1024");
  PlbApplyMask m;
  memset(&m, 0, sizeof(m));
  m.ids = ids; m.sample_off = sample_off; m.word_off = word_off; m.word_begin = word_begin; m.word_len = word_len;
  m.action = action; m.repl = repl; m.word_token = word_token; m.sep_token = sep_token; m.crop_start = crop_start;
  m.B = B; m.S = S; m.mask_id = mask_id;
  m.labels = labels; m.masked = masked; m.tokens = tokens; m.lengths_out = lengths_out;
  m.counts = scratch; m.idx_padded = scratch + B; m.offsets = idx_offsets; m.flat = idx_flat;
  TRY(plb_launch_apply_mask(&m, (hipStream_t)stream));
  return 0;
}

extern "C" int plb_mask_batch(const int64_t* labels, const int32_t* lengths, int32_t B, int32_t S, uint64_t seed,
                              uint32_t step, float word_pred_prob, float phoneme_mask_prob, float replace_prob,
                              int32_t mask_id, int32_t sep_id, int64_t* masked, int32_t* idx_offsets, int32_t* idx_flat,
                              int32_t* scratch, void* stream) {
  if (!labels || !masked || !idx_offsets || !idx_flat || !scratch) return fail("plb_mask_batch: null argument");
  if (S < 1 || S > 512 || B < 1 || B > 1024) return fail("plb_mask_batch: needs 1 <= S <= 512, 1 <= B <= 1024");
  PlbMask m;
  memset(&m, 0, sizeof(m));
  m.labels = labels; m.lengths = lengths; m.B = B; m.S = S; m.seed = seed; m.step = step;
  m.word_pred_prob = word_pred_prob; m.mask_prob = phoneme_mask_prob; m.replace_prob = replace_prob;
  m.mask_id = mask_id; m.sep_id = sep_id;
  m.masked = masked; m.counts = scratch; m.idx_padded = scratch + B; m.offsets = idx_offsets; m.flat = idx_flat;
  TRY(plb_launch_mask(&m, (hipStream_t)stream));
  return 0;
}
