// Internal interface of the engine units (engine*.cpp). Not installed and included by nothing else: the public boundary is
// include/plbert.h, the launch interface to the kernel files is plbert_kernels.h. It holds what more than one unit needs:
// PlbEngine, the small value types that travel between the stages of a call, the error / audit macros and the prototypes
// of the functions that cross a unit boundary. Everything declared here that is not extern "C" has hidden visibility.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/plbert.h"
#include "plbert_kernels.h"

#pragma GCC visibility push(hidden)

int fail(const char* fmt, ...);   // engine.cpp: sets the text plb_last_error returns; always 1

// Events that only order one HIP stream of this engine behind another: no timing, and a DEVICE-scope release when
// recorded (the default is a system-scope release, i.e. an L2 write-back for the host's benefit: nobody on the host
// reads what these events publish).
static const unsigned kStreamOrderEvent = hipEventDisableTiming | hipEventReleaseToDevice;

inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

#define TRY(x)                                                                    \
  do {                                                                            \
    int rc_ = (x);                                                                \
    if (rc_) return fail("%s failed (rc %d) at %s:%d", #x, rc_, __FILE__, __LINE__); \
  } while (0)
#define HIPTRY(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return fail("%s: %s at %s:%d", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
// a launch (or memset / collective) enqueued on `stream` reads / writes these bytes
#define HB_R(stream, ptr, bytes, what) do { if (e->hb.on) e->hb.access(hb_idx(e, stream), (ptr), (size_t)(bytes), false, what); } while (0)
#define HB_W(stream, ptr, bytes, what) do { if (e->hb.on) e->hb.access(hb_idx(e, stream), (ptr), (size_t)(bytes), true, what); } while (0)

typedef void* RcclComm;   // opaque communicator (engine_comm.cpp: the RCCL types restated from rccl.h)

// ---- happens-before audit of the backward's three streams (debug: PLBERT_HB_AUDIT=1 / plb_debug_hb_audit) --------------
// A host-side MODEL of the ordering the engine asks HIP for, kept beside the real calls: every stream carries a vector
// clock; an event record snapshots the recording stream's clock, a stream wait merges the snapshot into the waiter's.
// Every access to a buffer that more than one stream touches in a loss call (a flat gradient range, the partial-row
// tables, the scratch / slab areas, ...) is logged as (byte range, stream, that stream's tick, read or write), and is
// checked on entry against every logged access of ANOTHER stream to overlapping bytes where at least one of the two
// writes: the earlier one must be inside the later stream's clock, i.e. ordered before it by a record / wait chain.
// It reasons about the calls the engine makes, not about timing: a missing hipStreamWaitEvent is reported on every
// run, not once in eighty. DESIGN.md section 4 carries the table this checks. (wait / access: engine_comm.cpp)
struct HbAudit {
  enum { MAIN = 0, SIDE = 1, COMM = 2, NS = 3 };
  typedef std::array<uint64_t, NS> VC;
  struct Acc { const char* what; uintptr_t a, b; int st; uint64_t tick; bool wr; };
  bool on = false;
  int break_wait = -1;     // test hook: the MODEL forgets its n-th wait of the next loss call (the HIP call is still made)
  int waits = 0;
  VC vc[NS] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  std::map<hipEvent_t, VC> ev;
  std::vector<Acc> log;
  int64_t checks = 0;
  int violations = 0;
  std::string first;
  static const char* name(int st) { return st == MAIN ? "main" : st == SIDE ? "side" : "comm"; }
  void record(hipEvent_t e, int st) { vc[st][st] += 1; ev[e] = vc[st]; }
  void wait(int st, hipEvent_t e);
  void access(int st, const void* p, size_t bytes, bool wr, const char* what);
  // Everything logged so far is ordered before the main stream's present: start the next call with an empty log.
  void new_call() { log.clear(); waits = 0; }
};

// Members in blocks by the unit that writes them (plb_create value-initialises the engine: the order carries no meaning).
struct PlbEngine {
  // ---- layout, capacity and per-process knobs: engine.cpp (plb_create), constant afterwards ----
  PlbConfig c;
  int64_t poff[PLB_NPARAM], psize[PLB_NPARAM], ptotal, ptrain;
  int E, H, I, L, NH, V, P, NP, NT;
  int64_t Tcap;   // padded token capacity
  int64_t NMcap;  // padded masked-row capacity
  int NTp = 0;    // token (grapheme) head: NT padded to 256 columns (NT > 0 only)
  bool infer = false;           // inference-only workspace: one layer of activations, no gradient stash
  int qkvcol_rows = 0;  // partial rows per layer of the Q/K/V bias gradient: the attention plan's at (max_batch, max_seq)
  int64_t slab2_floats;
  int64_t slab_floats;
  int64_t ws_bytes;
  int ln_blocks, emb_blocks;
  int part_rows = 0;            // rows per layer reserved in o_part1 / o_part2
  int ducol_rows = 0;           // rows per layer reserved in o_ducol, rows reserved in o_tcolp: upper bounds of what a launch's
  int tcolp_rows = 0;           // plan (gemm_nt_plan.h) may write at the token capacity; every call checks its plans against them
  int ln_fuse = 3;              // bit 0: LayerNorm forward in the producing GEMM's epilogue, bit 1: LayerNorm backward
  int64_t lnx_bytes = 0;
  bool gelu_dstash_on = true;   // PLBERT_GELU_STASH=u restores the pre-activation stash
  bool fp8_tn = true;           // fp8 calls run the weight-gradient GEMMs on the 1-byte images too (PLBERT_FP8_TN=0: bf16 operands)
  int f8n = 0;
  // ---- caller's switches: engine.cpp ----
  bool packed_dual = false;     // plb_set_packed_dual: dual-head loss calls follow a plan that packs (off: they run padded)
  bool packed_fp8 = false;      // plb_set_packed_fp8: calls in fp8 mode follow a plan that packs (off: they run padded)
  // ---- workspace offsets (bytes): engine.cpp (plb_create) ----
  int64_t o_wbf, o_wqkvT, o_wdT, o_w1T, o_w2T, o_wpT, o_winT;
  int64_t o_e, o_x, o_qkv, o_ctx, o_pre1, o_a, o_u, o_g, o_pre2;
  int64_t o_lse, o_delta, o_mean1, o_rstd1, o_mean2, o_rstd2;
  int64_t o_dqkv, o_dpre1, o_du, o_dpre2;
  int64_t o_dy0, o_dy1, o_da, o_dctx, o_de;
  int64_t o_hm, o_logm, o_dlog, o_dhm, o_rows, o_tgt, o_w, o_lrows;
  int64_t o_slab, o_part1, o_part2, o_parte, o_scratch, o_dxe, o_ducol, o_slab2, o_scratch2, o_qkvcol = 0;
  int64_t o_lnx = 0, o_lnerr = 0;
  int64_t o_embpart = 0;   // chunk partial rows of the table sums keyed by position_ids / token_type_ids (embed_inputs.hip)
  int64_t o_keywords = 0;  // key-mask words of a plb_*_masked call (key_mask.hip): [max_batch][2 * ceil(max_seq / 64)] uint32
  int64_t o_pool_dpre = 0, o_pool_dh0 = 0;   // pooler backward of plb_encode_bwd_pooled (pooler_bwd.hip): fp32 [max_batch][H] each
  // plb_masked_report's own regions (engine_eval.cpp): ranks and row losses when the caller takes none, the token head's
  // per-block counts. No other entry point reads or writes them.
  int64_t o_rep_rank = 0, o_rep_nll = 0, o_rep_tok = 0;
  // plb_token_report's own regions (engine_eval.cpp; NT > 0 only): the row list and gathered targets its prepare launch
  // writes, the scratch of plb_launch_token_topk. No other entry point reads or writes them.
  int64_t o_tr_rows = 0, o_tr_tgt = 0, o_tr_scratch = 0;
  // token (grapheme) head training: padded copies and the [Tp][NTp] logit / gradient images (NT > 0 only)
  int64_t o_bt = 0, o_wtT = 0, o_tdl = 0, o_tlrows = 0, o_tscr = 0, o_tgrad = 0, o_tloss = 0;
  int64_t o_tpmax = 0, o_tpsum = 0, o_ttl = 0, o_tlse = 0, o_tw = 0, o_ttgt = 0, o_tcolp = 0;
  // per-layer 1-byte images [Ls][Tp][width] of every GEMM operand that is an activation (e4m3: layer input x, context,
  // attention-block output a, gelu output g) or a gradient (e5m2: dpre2, dU, dpre1, dQKV): read by the next NT GEMM and,
  // all layers at once, by the token-major weight-gradient GEMMs
  int64_t o_x8 = 0, o_a8 = 0, o_g8 = 0, o_c8 = 0, o_dp8 = 0, o_du8 = 0, o_dp18 = 0, o_dq8 = 0;
  int64_t o_wq8 = 0, o_wd8 = 0, o_w18 = 0, o_w28 = 0, o_w2T8 = 0, o_w1T8 = 0, o_wqT8 = 0, o_wdT8 = 0;
  int64_t o_f8amax = 0, o_f8scale = 0, o_f8deq = 0, o_f8stats = 0;
  // ---- fp8 state: engine_fp8.cpp (plb_set_fp8, fp8_quantize_weights); the call stages arm fp8_ready / fp8_bwd_ready ----
  // fp8 mode (plb_set_fp8): transient 1-byte images of the fp8 GEMMs' activation / gradient operands, fp8 weight copies
  // and the per-(site, layer) delayed-scaling state [amax | scale | deq] (+ one entry per weight copy)
  bool fp8_on = false, fp8_ready = false, fp8_bwd_ready = false, fp8_wstale = true;
  // ---- what the forward of a call leaves for its backward: engine_layers.cpp ----
  bool u_is_derivative = false; // what the "u" slots hold after the last forward
  bool tn8_call = false;        // ... decided per training call by its forward (shapes), read by its backward
  int part_rows_used = 0;       // rows per layer the last backward wrote
  // ---- what a call leaves for the next one: engine_calls.cpp (tok_pad_zeroed: engine.cpp; tok_steps: engine_optim.cpp) ----
  // Last application on the masked rows only (a phoneme-only loss call: nothing but the masked positions' final hidden
  // states reaches the loss, so behind the attention of application L-1 only those rows are computed): decided by the
  // forward of a call, read by its backward. pruned_rows = the compact row count (a multiple of 128), 0 = the call was full.
  int pruned_rows = 0;
  int64_t last_app_rows[2] = {0, 0};   // token rows the last loss call ran the post-attention part of its last application on | of
  int64_t last_exec_rows[2] = {0, 0};   // token rows the last forward / loss call executed | the B*S it stood for (plb_last_call_rows)
  bool tok_grads_live = false;  // the last loss call produced token-head gradients (AdamW then steps them)
  bool head_grads_live = true;  // ... phoneme-head gradients (false after plb_encode_bwd: AdamW then stops at PLB_HEAD_W)
  bool pool_grads_live = false; // the last plb_encode_bwd_pooled call took a d_pooled: the pooler range holds gradients
  bool tok_pad_zeroed = false;  // pad columns of the transposed copy are zeroed once
  int tok_steps = 0;            // AdamW steps the token head has taken (its own bias correction)
  // ---- what the last loss call left for plb_masked_report (engine_eval.cpp): set by loss_impl in engine_calls.cpp, cleared by
  // plb_bind. o_logm / o_tgt hold the rep_n masked rows' logits and labels; after a dual-head call o_tpmax / o_ttl / o_tw hold
  // the token head's statistics of rep_tok_rows rows.
  bool rep_valid = false, rep_dual = false;
  int rep_n = 0, rep_B = 0;
  int64_t rep_tok_rows = 0;
  // ---- the final hidden state of the last call that ran the encoder on every row, for plb_token_report (engine_eval.cpp):
  // recorded by the entry points of engine_calls.cpp through note_final, ended through drop_final by every call that runs
  // the encoder again, moves the weights (plb_adamw_step[_clipped], plb_sync_weights, plb_broadcast_params) or binds
  // (fin_dead_by: which one — the text plb_token_report fails with). fin_x is the last slot of o_x, which nothing but
  // run_encoder writes (engine_layers.cpp: the map-in GEMM writes slot 0, LayerNorm 2 of application l slot l + 1; the
  // backward only reads the slots), so the state is intact until the next encoder run.
  bool fin_live = false;
  const char* fin_dead_by = "no call has run the encoder on this engine since plb_bind";
  const bf16_t* fin_x = nullptr;
  int fin_B = 0, fin_S = 0;
  int64_t fin_rows = 0, fin_used = 0;           // Tp and T of that call
  const int32_t* fin_row_start = nullptr;       // its plan's table (null: it ran padded)
  // ---- gradient accumulation window and norm partials: engine_optim.cpp (grads_fresh is set, and norm_nparts cleared, by
  // begin_training_call in engine_calls.cpp; the calls that move the weights end a window through end_accum_window) ----
  float* accum = nullptr;       // plb_grad_accum_bind: the caller's buffer, `total` floats like grads
  bool grads_fresh = false;     // a backward entry point wrote the gradient buffer and no add has consumed it yet
  bool win_open = false;        // between a FIRST add and its LAST
  const char* win_closed_by = "no FIRST add has opened one";
  bool win_head = false, win_tok = false, win_pool = false;   // union of what the window's micro-steps produced (the encoder range always is)
  bool win_reduced = false;     // the window's micro-steps came in all-reduced (overlap on) or not: they must agree
  const float* norm_src = nullptr;   // the LAST add left norm_nparts partials behind the four result floats of this buffer
  int norm_nparts = 0;
  bool norm_reduced = false;    // ... taken from gradients in this exchange state
  // ---- encode stash: engine_calls.cpp (every unit ends its life through drop_stash) ----
  // plb_encode / plb_encode_bwd: the stash of a differentiable forward is live until a call writes the workspace or moves
  // the weights (stash_dead_by: which one — the text plb_encode_bwd fails with)
  bool stash_live = false;
  const char* stash_dead_by = "no plb_encode has run on this engine";
  int stash_B = 0, stash_S = 0;
  int64_t stash_rows = 0, stash_used = 0;       // Tp and T of the plb_encode call
  const int32_t* stash_row_start = nullptr;     // its plan's table (null: it ran padded)
  bool stash_masked = false;                    // it ran with a key mask (plb_encode_masked): its backward takes the mask again
  // ---- exchange, status and trace: engine_comm.cpp (begin_training_call in engine_calls.cpp resets the per-call counters) ----
  // data-parallel exchange (plb_comm_*): RCCL communicator, its stream, and the join event of the pieces in flight
  RcclComm comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_piece = nullptr, ev_comm_done = nullptr;
  bool overlap = true;          // issue the all-reduce piecewise inside plb_loss_fwd_bwd
  bool comm_pending = false;    // pieces were issued: whoever touches the gradient buffer next joins ev_comm_done (join_comm)
  bool grads_reduced = false;   // the gradients of the last loss call have been all-reduced
  int64_t piece_floats = 0;     // floats submitted as pieces by the current loss call (must add up to the gradient range)
  int32_t piece_count = 0;      // collectives the last step issued (pieces by the loss call + in-stream all-reduces)
  // the step's health word travels too (one float, summed over the ranks): every rank skips, or none
  hipEvent_t ev_status = nullptr;
  bool status_pending = false;  // the word's all-reduce is in flight on the communication stream
  int32_t status_collectives = 0;
  float* last_loss = nullptr;   // where the last loss call put its loss (plb_status_import turns it into NaN)
  HbAudit hb;
  // exchange trace (plb_comm_trace): timing events around every piece of the last loss call
  struct PieceTrace { int64_t a, b; hipEvent_t released, done; };
  bool trace_on = false;
  std::vector<PieceTrace> trace;
  std::vector<hipEvent_t> trace_pool;
  hipEvent_t tr_call0 = nullptr, tr_tail0 = nullptr, tr_tail1 = nullptr;
  bool tr_tail_valid = false;   // the last traced call reached its tail (a zero-loss call has none)
  // ---- bound buffers, side stream, status mirror: engine.cpp (plb_bind) ----
  // side stream: the tail of the backward (embedding chain, bias / LayerNorm column sums) runs beside the
  // four large weight-gradient GEMMs
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // host-visible mirror of the hand-off error word (pinned, device-mapped): written by the last launch of every loss
  // call, read by plb_poll_status without synchronising
  unsigned int* host_err = nullptr;
  unsigned int* host_err_dev = nullptr;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  char* ws = nullptr;

  template <typename T>
  T* at(int64_t off) const { return reinterpret_cast<T*>(ws + off); }
  bf16_t* wbf(int which) const { return at<bf16_t>(o_wbf) + poff[which]; }
  float* par(int which) const { return params + poff[which]; }
  float* grd(int which) const { return grads + poff[which]; }
};

// ---- fp8 mode ---------------------------------------------------------------------------------------------------------
// Sites: activations X (layer input), A (attention block output), G (gelu output) in e4m3; gradients DP (dpre2) and DU
// in e5m2 (their range within a tensor is what e5m2's five exponent bits are for); weights W* in e4m3.
enum { F8_X = 0, F8_A, F8_G, F8_C, F8_DP, F8_DU, F8_DP1, F8_DQ, F8_NSITE };   // 4 activation sites, then 4 gradient sites
enum { F8_AMAX_WORDS = 64 * 16 };  // floats per site in the amax array (common.h: F8_SLOTS x F8_STRIDE)
enum { F8W_QKV = 0, F8W_D, F8W_1, F8W_2, F8W_2T, F8W_1T, F8W_QKVT, F8W_DT, F8W_N };

// ---- token-packed calls (include/plbert.h: PlbPacking) ------------------------------------------------------------------
// The rows of one call. Padded: sample b at rows b*S.., T = B*S real rows, Tp = T rounded up to 128. Packed: sample b at
// rows row_start[b].. (128-aligned slots holding its valid tokens only), T = the rows the slots cover, Tp = the plan's row
// count. Everything between the embeddings and the loss rows sees only T and Tp; rows [T, Tp) are the tail the padded path
// has always had when B*S is no multiple of 128 (no attention workgroup writes them, their gradients are kept at zero).
struct Rows {
  const int32_t* row_start;   // device, or null: padded
  int T; int64_t Tp;
  // key-mask words of a plb_*_masked call (PlbAttn.key_words / ldkw), or null: every attention launch of the call takes them
  const uint32_t* key_words = nullptr; int ldkw = 0;
};

// One fp8 operand site of one application: the delayed scale its images are written with, the running maximum the writing
// launch records, the dequantisation factor its readers apply
struct F8Site {
  float* scale = nullptr;
  float* amax = nullptr;
  float* deq = nullptr;
  F8Site() = default;
  F8Site(const PlbEngine* e, int kind, int l);
};
// The e4m3 copy of a weight (fp8_quantize_weights) and its dequantisation factor
struct F8Weight {
  const uint8_t* img;
  const float* deq;
  F8Weight(const PlbEngine* e, int w);
};

// One NT GEMM of the fp8 set: the fp8 launch when the call runs in fp8 mode (A8 / B8 images, their dequantisation
// factors), else the bf16 launch on A / B. g carries everything else (shapes, bias, residual, outputs).
struct F8Op { const uint8_t* A8; const uint8_t* B8; const float* deq_a; const float* deq_b; int a_bf8; };

// ---- stash slots of one application -----------------------------------------------------------------------------------
// Slot l of a stacked buffer starts at l · Tp · width: the slots of a call are packed with the call's own padded token
// count, not the capacity, so the token-major weight-gradient GEMMs read L · Tp contiguous rows. Per-application blocks
// with other strides: lse B·NH·S floats, the LayerNorm-backward partials prows·3H, the Q/K/V bias partial rows
// qkvcol_rows(B, S)·3H (the call's, not the capacity PlbEngine::qkvcol_rows), the ffn.bias partial rows du_rows·I.
// stash (training): L+1 slots of x (the input of application l+1 is the output of l) and L of everything else;
// otherwise one slot of everything and two ping-pong slots of x.
struct Slots {
  bf16_t *x, *y;                                    // the application's input and output
  bf16_t *qkv, *ctx, *pre1, *a, *u, *g, *pre2;      // activations
  float *mean1, *rstd1, *mean2, *rstd2, *lse;       // LayerNorm statistics, attention log-sum-exp
  uint8_t *x8, *x8n, *c8, *a8, *g8;                 // 1-byte images (x8n: the next application's input image)
  // stash only: the gradients that feed the weight-gradient GEMMs, their images, the partial-row blocks
  bf16_t *dqkv, *dpre1, *du, *dpre2;
  uint8_t *dp8, *du8, *dp18, *dq8;
  float *part1, *part2, *qkvcol, *ducol;
};

// One LayerNorm of one application: affine parameters, its input (kept by the forward, read by the backward), statistics
// and backward partial rows
struct LnSlot { const float* gamma; const float* beta; const bf16_t* pre; float* mean; float* rstd; float* partials; };

// The masked rows a pruned last application runs on (engine_layers.cpp: last_application_fwd_pruned): n rows, Mc = n padded to 128
struct Prune { const int32_t* rows; int n; int Mc; };

// What a call feeds its embeddings beside the ids (include/plbert.h: PlbEmbedInputs) and, in a backward, where the gradient of
// the pre-LayerNorm sum goes (fp32 [B,S,E], or null). All members null: a plain call — the launches of embed.hip, as before.
struct EmbedCall {
  PlbEmbedInputs in;
  float* d_inputs_embeds;
  bool any() const { return in.token_type_ids || in.position_ids || in.inputs_embeds || d_inputs_embeds; }
};

// One encoder call, as every stage from its entry point down to the launches sees it. The implementation of the entry point
// builds it once, behind its refusals (a loss call too: ids = masked_ids, an empty EmbedCall, no taps); the stages take it by
// const reference and nothing else about the call. Nothing in it is derived from another member.
struct Call {
  const char* who;                // the entry point, as its texts name it
  const int64_t* ids;             // [B,S], or null with ec.in.inputs_embeds
  const int32_t* lengths;         // [B], or null: every sample is full
  int B, S;
  Rows rw;                        // its rows and, in a plb_*_masked call, its key-mask words
  EmbedCall ec;
  const PlbLayerOutputs* taps;    // per-application outputs the caller asked for (include/plbert.h), or null
  hipStream_t s;
};

// What the backward stages of one call share beside the call: its precision mode, the partial-row layout of its layer loop.
struct Bwd {
  const Call& call;
  bool f8, calib;   // fp8 operands | an fp8-mode call that only records the maxima
  bool fuse_b;      // LayerNorm backward in the epilogue of the dX GEMM that produces its output gradient
  int prows;        // LayerNorm-backward partial rows per application
  int du_rows;      // ffn.bias partial rows per application (0: the tail sums dU itself)
};

// The pieces of the overlapped exchange in issue order (engine_comm.cpp: kPieces)
enum { kPieceHead = 0, kPieceQkvW, kPieceFfnW, kPieceSmall, kPieceFfnoW = kPieceSmall + 5, kPieceDenseW, kNPieces };

// ---- functions that cross a unit boundary ---------------------------------------------------------------------------------
// engine_comm.cpp
int hb_idx(const PlbEngine* e, hipStream_t s);
hipError_t ev_record(PlbEngine* e, hipEvent_t ev, hipStream_t s);
hipError_t ev_wait(PlbEngine* e, hipStream_t s, hipEvent_t ev);
int reduce_piece(PlbEngine* e, int64_t a, int64_t b, hipStream_t after);
bool overlapping(const PlbEngine* e);
int join_comm(PlbEngine* e, hipStream_t s);
int pieces_done(PlbEngine* e);
int64_t piece_begin(const PlbEngine* e, int i);
int64_t piece_end(const PlbEngine* e, int i);
int reduce_pieces(PlbEngine* e, int from, int to, hipStream_t after);
int status_exchange(PlbEngine* e, hipStream_t s);
int status_finish(PlbEngine* e, float* loss, hipStream_t s);
// engine_fp8.cpp
int f8_site(const PlbEngine* e, int site, int l);
float* f8_deq(const PlbEngine* e, int i);
int fp8_quantize_weights(PlbEngine* e, hipStream_t s, bool exact = true);
int fp8_update_scales(PlbEngine* e, hipStream_t s);
bool f8_call(const PlbEngine* e, int64_t Tp, bool train);
bool tn8_ok(const PlbEngine* e, int64_t Mtot);
// engine_layers.cpp
PlbGemmNT nt_desc(const bf16_t* A, const bf16_t* B, int64_t M, int N, int K);
// the plan (gemm_nt_plan.h) of a packed [M, N] x K launch: what the launcher of that form and operand kind will do
PlbGemmNTPlan nt_plan(int64_t M, int N, int K, int form, int operands = PLB_NT_BF16, int opts = 0);
int qkvcol_rows(const PlbEngine* e, int B, int S);   // the attention plan's colpart_rows at the call's shape
Slots slots(const PlbEngine* e, int64_t Tp, int B, int S, int l, bool stash, int prows = 0, int du_rows = 0);
bool prune_enabled();
int run_encoder(PlbEngine* e, const Call& c, bool stash, bf16_t** xout, const Prune* pr);
PlbEmbed embed_desc(const PlbEngine* e, const Call& c);
PlbEmbedIn embed_in_desc(const PlbEngine* e, const EmbedCall& ec, const PlbEmbed* base);
int weight_grad(PlbEngine* e, const void* A, int lda, int Ncols, const void* Bm, int ldb, int64_t Mtot, int N, int K,
                float* out, hipStream_t s, bool side_slab = false, int site_a = -1, int site_b = -1);   // sites: an fp8 call
int encoder_bwd(PlbEngine* e, const Call& c, const Prune* pr, bf16_t** dy, int* du_rows, const float* const* d_below);
// engine_calls.cpp
void drop_stash(PlbEngine* e, const char* by);
void drop_final(PlbEngine* e, const char* by);
// engine.cpp
int sync_transposes(PlbEngine* e, hipStream_t s, bool exact_fp8 = true);
// engine_optim.cpp
inline int64_t pool_end(const PlbEngine* e) { return e->poff[PLB_POOL_B] + e->psize[PLB_POOL_B]; }   // end of the pooler range
void end_accum_window(PlbEngine* e, const char* by);

#pragma GCC visibility pop
