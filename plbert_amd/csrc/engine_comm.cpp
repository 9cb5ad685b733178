// Data-parallel exchange of the engine: the run-time RCCL loader, the gradient pieces and the step's health word
// (issued from the stages of a loss call in engine_calls.cpp), plb_comm_* / plb_status*, and the happens-before audit's
// model with the two stream-ordering calls that feed it. Only writer of PlbEngine's communicator, its stream and events,
// overlap and the trace switch; the per-call counters and the trace records are also reset by begin_training_call.
#include <dlfcn.h>

#include "engine_internal.h"

// ---- RCCL, resolved at run time -----------------------------------------------------------------------------
// The library is not linked against RCCL: a Python host has torch's own librccl.so.1 mapped already (one RCCL per
// process), a C / C++ host gets the system one. Only the handful of entry points of the gradient exchange are bound;
// types restated from rccl.h (the NCCL API): opaque communicator, 128-byte unique id, int result / enum codes.
namespace {
struct RcclId { char internal[128]; };
enum { kNcclSuccess = 0, kNcclFloat32 = 7, kNcclSum = 0 };
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(RcclComm*, int, RcclId, int) = nullptr;
  int (*CommDestroy)(RcclComm) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
  int (*GetVersion)(int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
RcclApi g_rccl;
const char* rccl_load() {  // nullptr on success, else what failed
  if (g_rccl.ok) return nullptr;
  const char* env = getenv("PLBERT_RCCL_LIB");
  void* h = nullptr;
  if (env && *env) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // already in the process (torch's copy)
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return "cannot load librccl.so.1 (set PLBERT_RCCL_LIB)";
  g_rccl.handle = h;
#define RSYM(field, name) \
  *(void**)(&g_rccl.field) = dlsym(h, name); \
  if (!g_rccl.field) return "librccl lacks " name
  RSYM(GetUniqueId, "ncclGetUniqueId");
  RSYM(CommInitRank, "ncclCommInitRank");
  RSYM(CommDestroy, "ncclCommDestroy");
  RSYM(AllReduce, "ncclAllReduce");
  RSYM(Broadcast, "ncclBroadcast");
  RSYM(GetVersion, "ncclGetVersion");
  RSYM(GetErrorString, "ncclGetErrorString");
#undef RSYM
  g_rccl.ok = true;
  return nullptr;
}
}  // namespace

void HbAudit::wait(int st, hipEvent_t e) {
  const int n = waits++;
  if (n == break_wait) { break_wait = -1; return; }
  auto it = ev.find(e);
  if (it == ev.end()) return;   // never recorded: HIP treats the wait as a no-op, so does the model
  for (int i = 0; i < NS; ++i) if (it->second[i] > vc[st][i]) vc[st][i] = it->second[i];
}
void HbAudit::access(int st, const void* p, size_t bytes, bool wr, const char* what) {
  if (!p || !bytes) return;
  const uintptr_t a = (uintptr_t)p, b = a + bytes;
  vc[st][st] += 1;
  for (const Acc& x : log) {
    if (x.st == st || !(wr || x.wr) || x.b <= a || b <= x.a) continue;
    ++checks;
    if (x.tick > vc[st][x.st]) {
      if (!violations++) {
        char m[384];
        snprintf(m, sizeof(m), "%s of '%s' on the %s stream is not ordered after the %s of '%s' on the %s stream", wr ? "write" : "read",
                 what, name(st), x.wr ? "write" : "read", x.what, name(x.st));
        first = m;
      }
    }
  }
  log.push_back(Acc{what, a, b, st, vc[st][st], wr});
}

// Stream-ordering calls of the engine go through these two: the HIP call, and — audit on — the same step in the model.
int hb_idx(const PlbEngine* e, hipStream_t s) {
  if (e->side && s == e->side) return HbAudit::SIDE;
  if (e->comm_stream && s == e->comm_stream) return HbAudit::COMM;
  return HbAudit::MAIN;
}
hipError_t ev_record(PlbEngine* e, hipEvent_t ev, hipStream_t s) {
  const hipError_t r = hipEventRecord(ev, s);
  if (e->hb.on) e->hb.record(ev, hb_idx(e, s));
  return r;
}
hipError_t ev_wait(PlbEngine* e, hipStream_t s, hipEvent_t ev) {
  const hipError_t r = hipStreamWaitEvent(s, ev, 0);
  if (e->hb.on) e->hb.wait(hb_idx(e, s), ev);
  return r;
}

// ---- gradient exchange pieces ---------------------------------------------------------------------------------
// One sum all-reduce of grads[a, b) on the communication stream, ordered after everything enqueued on `after` so far.
static int g_debug_skip_piece = -1;   // test hook (plb_debug_skip_piece): drop the n-th piece of a loss call
extern "C" void plb_debug_skip_piece(int index) { g_debug_skip_piece = index; }

static hipEvent_t trace_event(PlbEngine* e) {
  if (!e->trace_pool.empty()) { hipEvent_t v = e->trace_pool.back(); e->trace_pool.pop_back(); return v; }
  hipEvent_t v = nullptr;
  (void)hipEventCreate(&v);   // timing enabled
  return v;
}
int reduce_piece(PlbEngine* e, int64_t a, int64_t b, hipStream_t after) {
  if (!e->comm || b <= a) return 0;
  if (g_debug_skip_piece >= 0 && e->piece_count == g_debug_skip_piece) {  // what a forgotten tensor looks like
    g_debug_skip_piece = -1;
    e->piece_count += 1;
    return 0;
  }
  PlbEngine::PieceTrace tr{a, b, nullptr, nullptr};
  if (e->trace_on) {
    tr.released = trace_event(e); tr.done = trace_event(e);
    (void)hipEventRecord(tr.released, after);
  }
  HIPTRY(ev_record(e, e->ev_piece, after));
  HIPTRY(ev_wait(e, e->comm_stream, e->ev_piece));
  HB_W(e->comm_stream, e->grads + a, (b - a) * 4, "all-reduce piece (in place)");
  const int rc = g_rccl.AllReduce(e->grads + a, e->grads + a, (size_t)(b - a), kNcclFloat32, kNcclSum, e->comm, e->comm_stream);
  if (rc != kNcclSuccess) return fail("ncclAllReduce: %s", g_rccl.GetErrorString(rc));
  if (e->trace_on) {
    (void)hipEventRecord(tr.done, e->comm_stream);
    e->trace.push_back(tr);
  }
  e->comm_pending = true;
  e->piece_floats += b - a;
  e->piece_count += 1;
  return 0;
}
bool overlapping(const PlbEngine* e) { return e->comm && e->overlap; }
// All-reduce pieces still in flight on the communication stream read and write the gradient buffer: `s` waits for them.
// (comm_pending implies a communicator: only reduce_piece sets it, behind its own e->comm test, and plb_comm_destroy clears it)
int join_comm(PlbEngine* e, hipStream_t s) {
  if (!e->comm_pending) return 0;
  HIPTRY(ev_wait(e, s, e->ev_comm_done));
  e->comm_pending = false;
  return 0;
}
// Close the pieces issued so far: later joins wait on ev_comm_done.
int pieces_done(PlbEngine* e) {
  if (e->hb.on && e->hb.violations)
    return fail("happens-before audit: %d violation(s), first: %s", e->hb.violations, e->hb.first.c_str());
  if (!e->comm_pending) return 0;
  // the pieces are disjoint by construction; together they must be exactly the range AdamW is about to consume (a
  // one-rank communicator would not show a forgotten tensor: its all-reduce is the identity)
  const int64_t want = (e->pool_grads_live ? pool_end(e) : e->ptrain) + (e->tok_grads_live ? e->ptotal - e->poff[PLB_TOK_W] : 0);
  if (e->piece_floats != want)
    return fail("gradient exchange covered %lld of %lld floats", (long long)e->piece_floats, (long long)want);
  HIPTRY(ev_record(e, e->ev_comm_done, e->comm_stream));
  e->grads_reduced = true;
  return 0;
}
// The pieces of the overlapped exchange, in issue order, as [begin, end) parameter boundaries of the flat gradient buffer
// (PLB_HEAD_B + 1: the end of the trainable range). A collective sequence must be the same on every rank: the regular call
// (the phoneme head, then the tail) and a rank without masked phonemes (zero_loss_call) both issue exactly this list. The
// token head's piece of a dual-head call is not in it: a dual-head call never takes the zero-loss path.
struct PieceRange { int begin, end; };
static const PieceRange kPieces[] = {
    {PLB_HEAD_W, PLB_HEAD_B + 1},   // the phoneme head: final before the layer loop (the status word travels behind it)
    {PLB_Q_W, PLB_Q_B},             // the weights, each as soon as its weight-gradient GEMM has written it ...
    {PLB_FFN_W, PLB_FFN_B},
    // ... the small tensors between them in the flat order, from the side stream
    {PLB_WORD_EMB, PLB_Q_W}, {PLB_Q_B, PLB_DENSE_W}, {PLB_DENSE_B, PLB_FFN_W}, {PLB_FFN_B, PLB_FFNO_W}, {PLB_FFNO_B, PLB_HEAD_W},
    {PLB_FFNO_W, PLB_FFNO_B},
    {PLB_DENSE_W, PLB_DENSE_B}};   // the smallest weight goes last
static_assert(sizeof(kPieces) / sizeof(kPieces[0]) == kNPieces, "piece table");
int64_t piece_begin(const PlbEngine* e, int i) { return e->poff[kPieces[i].begin]; }
int64_t piece_end(const PlbEngine* e, int i) { return e->poff[kPieces[i].end]; }
// kPieces[from, to), each ordered after everything enqueued on `after` so far
int reduce_pieces(PlbEngine* e, int from, int to, hipStream_t after) {
  for (int i = from; i < to; ++i)
    if (reduce_piece(e, piece_begin(e, i), piece_end(e, i), after)) return 1;
  return 0;
}

// ---- the step's health word, agreed between the ranks -----------------------------------------------------------
// A fused LayerNorm hand-off that times out (never observed) raises the error word of THE RANK IT HAPPENED ON; that
// rank's gradients are invalid — and have been summed into every replica by the time AdamW runs. So the word travels
// too: one float per rank (its count), summed over the communicator inside the loss call, after the last launch that
// can raise it (the layer loop; the tail has no hand-offs) and before the call's status launch. Every rank then sees a
// non-zero word, returns a NaN loss, skips the update (and every later one, until plb_status has reported) and raises
// from its next status poll: replicas stay bit-identical. Overlapped form: on the communication stream, between the head
// piece and the first weight's (it is long done when the tail's last GEMM ends; the main stream joins it before the
// status launch); serial form: in the caller's stream. The SAME position in the collective sequence on every rank,
// including a rank that takes the zero-loss path.
static float* status_float(const PlbEngine* e) { return e->at<float>(e->o_lnerr) + 16; }
int status_exchange(PlbEngine* e, hipStream_t s) {
  if (!e->comm) return 0;
  float* f = status_float(e);
  TRY(plb_launch_status_export(e->at<unsigned int>(e->o_lnerr), f, s));
  hipStream_t cs = overlapping(e) ? e->comm_stream : s;
  if (cs != s) {
    HIPTRY(ev_record(e, e->ev_piece, s));
    HIPTRY(ev_wait(e, cs, e->ev_piece));
  }
  const int rc = g_rccl.AllReduce(f, f, 1, kNcclFloat32, kNcclSum, e->comm, cs);
  if (rc != kNcclSuccess) return fail("ncclAllReduce (status word): %s", g_rccl.GetErrorString(rc));
  if (cs != s) {
    HIPTRY(ev_record(e, e->ev_status, cs));
    e->status_pending = true;
  }
  e->status_collectives += 1;
  return 0;
}
// last launch of a loss call: merge the ranks' word (if it travelled), NaN loss + host mirror when it is set
int status_finish(PlbEngine* e, float* loss, hipStream_t s) {
  if (e->status_pending) {
    HIPTRY(ev_wait(e, s, e->ev_status));
    e->status_pending = false;
  }
  e->last_loss = loss;
  TRY(plb_launch_step_status(e->at<unsigned int>(e->o_lnerr), loss, e->host_err_dev, e->comm ? status_float(e) : nullptr, s));
  return 0;
}

// ---- data-parallel exchange -------------------------------------------------------------------------------------
extern "C" int plb_comm_unique_id(uint8_t id[PLB_COMM_ID_BYTES]) {
  if (!id) return fail("plb_comm_unique_id: null argument");
  if (const char* err = rccl_load()) return fail("plb_comm_unique_id: %s", err);
  RcclId u;
  memset(&u, 0, sizeof(u));
  const int rc = g_rccl.GetUniqueId(&u);
  if (rc != kNcclSuccess) return fail("ncclGetUniqueId: %s", g_rccl.GetErrorString(rc));
  static_assert(sizeof(u) == PLB_COMM_ID_BYTES, "unique id size");
  memcpy(id, &u, sizeof(u));
  return 0;
}

extern "C" int plb_comm_destroy(PlbEngine* e) {
  if (!e) return fail("plb_comm_destroy: null engine");
  if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);
  if (e->comm && g_rccl.ok) (void)g_rccl.CommDestroy(e->comm);
  e->comm = nullptr; e->comm_rank = 0; e->comm_world = 1; e->comm_pending = false;
  if (e->ev_piece) { (void)hipEventDestroy(e->ev_piece); e->ev_piece = nullptr; }
  if (e->ev_comm_done) { (void)hipEventDestroy(e->ev_comm_done); e->ev_comm_done = nullptr; }
  if (e->ev_status) { (void)hipEventDestroy(e->ev_status); e->ev_status = nullptr; }
  e->status_pending = false;
  if (e->comm_stream) { (void)hipStreamDestroy(e->comm_stream); e->comm_stream = nullptr; }
  return 0;
}

extern "C" int plb_comm_init(PlbEngine* e, const uint8_t id[PLB_COMM_ID_BYTES], int32_t rank, int32_t world) {
  if (!e || !id) return fail("plb_comm_init: null argument");
  if (!e->grads) return fail("plb_comm_init: bind the gradient buffer first (plb_bind)");
  if (world < 1 || rank < 0 || rank >= world) return fail("plb_comm_init: rank %d of %d", rank, world);
  if (e->comm) return fail("plb_comm_init: the engine already has a communicator");
  if (const char* err = rccl_load()) return fail("plb_comm_init: %s", err);
  // priority stream: the collective's few workgroups should get CUs ahead of the next GEMM's grid
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  HIPTRY(hipStreamCreateWithPriority(&e->comm_stream, hipStreamNonBlocking, hi));
  HIPTRY(hipEventCreateWithFlags(&e->ev_piece, kStreamOrderEvent));
  HIPTRY(hipEventCreateWithFlags(&e->ev_comm_done, kStreamOrderEvent));
  HIPTRY(hipEventCreateWithFlags(&e->ev_status, kStreamOrderEvent));
  RcclId u;
  memcpy(&u, id, sizeof(u));
  const int rc = g_rccl.CommInitRank(&e->comm, world, u, rank);
  if (rc != kNcclSuccess) {
    e->comm = nullptr;
    (void)plb_comm_destroy(e);
    return fail("ncclCommInitRank(rank %d of %d): %s", rank, world, g_rccl.GetErrorString(rc));
  }
  e->comm_rank = rank; e->comm_world = world;
  return 0;
}

extern "C" int plb_comm_info(const PlbEngine* e, int32_t* rank, int32_t* world, int32_t* rccl_version) {
  if (!e) return fail("plb_comm_info: null engine");
  if (rank) *rank = e->comm_rank;
  if (world) *world = e->comm ? e->comm_world : 1;
  if (rccl_version) {
    int v = 0;
    if (g_rccl.ok) (void)g_rccl.GetVersion(&v);
    *rccl_version = v;
  }
  return 0;
}

extern "C" int plb_status_ex(PlbEngine* e, int32_t* ln_exchange_timeouts, int32_t* skipped_updates) {
  if (!e || !e->ws) return fail("plb_status: engine not bound");
  unsigned int v[3] = {0, 0, 0};
  HIPTRY(hipDeviceSynchronize());
  HIPTRY(hipMemcpy(v, e->at<unsigned int>(e->o_lnerr), sizeof(v), hipMemcpyDeviceToHost));
  if (ln_exchange_timeouts) *ln_exchange_timeouts = (int32_t)v[0];
  if (skipped_updates) *skipped_updates = (int32_t)v[1];
  if (v[0]) {
    // the token head counts its own AdamW steps on the host (tok_steps): take back the ones the device left out (word 2)
    e->tok_steps = e->tok_steps > (int)v[2] ? e->tok_steps - (int)v[2] : 0;
    // Reported once, then gone: a producer whose store landed after its consumer had given up leaves a tagged granule
    // that the next launch would take for a fresh one, so the exchange buffer is zeroed again (the device is idle
    // here) together with the error word and its host mirror. The next step starts clean.
    HIPTRY(hipMemset(e->at<char>(e->o_lnx), 0, (size_t)e->lnx_bytes));
    HIPTRY(hipMemset(e->at<char>(e->o_lnerr), 0, 256));
    HIPTRY(hipDeviceSynchronize());
    if (e->host_err) *(volatile unsigned int*)e->host_err = 0;
  }
  return 0;
}
extern "C" int plb_status(PlbEngine* e, int32_t* ln_exchange_timeouts) { return plb_status_ex(e, ln_exchange_timeouts, nullptr); }

extern "C" int plb_poll_status(const PlbEngine* e, int32_t* ln_exchange_timeouts) {
  if (!e || !e->ws || !e->host_err) return fail("plb_poll_status: engine not bound");
  if (ln_exchange_timeouts) *ln_exchange_timeouts = (int32_t)*(volatile const unsigned int*)e->host_err;
  return 0;
}

// A host that exchanges the gradients ITSELF (torch.distributed fallback, a foreign communicator) must let the health word
// travel with them: export after the loss call, sum the float over the ranks, import before plb_adamw_step.
extern "C" int plb_status_export(PlbEngine* e, float* out, void* stream) {
  if (!e || !e->ws || !out) return fail("plb_status_export: bad argument");
  TRY(plb_launch_status_export(e->at<unsigned int>(e->o_lnerr), out, (hipStream_t)stream));
  return 0;
}
extern "C" int plb_status_import(PlbEngine* e, const float* summed, void* stream) {
  if (!e || !e->ws || !summed) return fail("plb_status_import: bad argument");
  TRY(plb_launch_step_status(e->at<unsigned int>(e->o_lnerr), e->last_loss, e->host_err_dev, summed, (hipStream_t)stream));
  return 0;
}

// ---- debug: happens-before audit, exchange trace -------------------------------------------------------------------------
extern "C" int plb_debug_hb_audit(PlbEngine* e, int32_t on, int32_t break_wait) {
  if (!e) return fail("plb_debug_hb_audit: null engine");
  e->hb = HbAudit();
  e->hb.on = on != 0;
  e->hb.break_wait = break_wait;
  return 0;
}
extern "C" int plb_debug_hb_report(const PlbEngine* e, int64_t* checks, int32_t* violations, char* first, int32_t first_bytes) {
  if (!e) return fail("plb_debug_hb_report: null engine");
  if (checks) *checks = e->hb.checks;
  if (violations) *violations = e->hb.violations;
  if (first && first_bytes > 0) snprintf(first, (size_t)first_bytes, "%s", e->hb.first.c_str());
  return 0;
}
extern "C" int plb_comm_trace(PlbEngine* e, int32_t on) {
  if (!e) return fail("plb_comm_trace: null engine");
  e->trace_on = on != 0;
  return 0;
}
// Timing of the last loss call's pieces, in milliseconds since the call's first launch: when the piece was released (the
// launch that completed its range had finished) and when its all-reduce had finished; tail_ms[2] = begin / end of the tail
// of weight-gradient GEMMs on the caller's stream. Synchronises on the events. Returns the number of pieces in *n.
extern "C" int plb_comm_trace_read(PlbEngine* e, int32_t max_pieces, int32_t* n, int64_t* begin, int64_t* end, float* released_ms,
                                   float* done_ms, float* tail_ms) {
  if (!e || !n) return fail("plb_comm_trace_read: bad argument");
  *n = 0;
  if (!e->tr_call0) return 0;
  if (tail_ms) { tail_ms[0] = tail_ms[1] = 0.f; }
  if (tail_ms && e->tr_tail_valid) {
    HIPTRY(hipEventSynchronize(e->tr_tail1));
    HIPTRY(hipEventElapsedTime(&tail_ms[0], e->tr_call0, e->tr_tail0));
    HIPTRY(hipEventElapsedTime(&tail_ms[1], e->tr_call0, e->tr_tail1));
  }
  for (auto& t : e->trace) {
    if (*n >= max_pieces) break;
    HIPTRY(hipEventSynchronize(t.done));
    if (begin) begin[*n] = t.a;
    if (end) end[*n] = t.b;
    if (released_ms) HIPTRY(hipEventElapsedTime(&released_ms[*n], e->tr_call0, t.released));
    if (done_ms) HIPTRY(hipEventElapsedTime(&done_ms[*n], e->tr_call0, t.done));
    *n += 1;
  }
  return 0;
}

extern "C" int plb_comm_pieces(const PlbEngine* e, int32_t* collectives, int64_t* floats) {
  if (!e) return fail("plb_comm_pieces: null engine");
  if (collectives) *collectives = e->piece_count;
  if (floats) *floats = e->piece_floats;
  return 0;
}

extern "C" int plb_set_grad_overlap(PlbEngine* e, int32_t overlap) {
  if (!e) return fail("plb_set_grad_overlap: null engine");
  e->overlap = overlap != 0;
  return 0;
}

extern "C" int plb_broadcast_params(PlbEngine* e, int32_t root, void* stream) {
  if (!e || !e->ws) return fail("plb_broadcast_params: engine not bound");
  drop_stash(e, "plb_broadcast_params moved the weights since");
  drop_final(e, "plb_broadcast_params moved the weights since");
  end_accum_window(e, "plb_broadcast_params moved the weights");
  if (!e->comm) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int rc = g_rccl.Broadcast(e->params, e->params, (size_t)e->ptotal, kNcclFloat32, root, e->comm, s);
  if (rc != kNcclSuccess) return fail("ncclBroadcast: %s", g_rccl.GetErrorString(rc));
  return plb_sync_weights(e, stream);
}

extern "C" int plb_allreduce_grads(PlbEngine* e, void* stream) {
  if (!e || !e->ws) return fail("plb_allreduce_grads: engine not bound");
  if (!e->comm) return 0;
  if (!e->grads) return fail("plb_allreduce_grads: no gradient buffer bound");
  hipStream_t s = (hipStream_t)stream;
  if (e->comm_pending) return join_comm(e, s);   // the loss call issued the pieces: join them
  if (e->grads_reduced) return 0;
  HB_W(s, e->grads, e->ptotal * 4, "in-stream all-reduce of the gradient buffer");
  // (live pooler gradients lie right behind the trainable range: the same collective covers them)
  const int64_t first = e->pool_grads_live ? pool_end(e) : e->ptrain;
  int rc = g_rccl.AllReduce(e->grads, e->grads, (size_t)first, kNcclFloat32, kNcclSum, e->comm, s);
  e->piece_count = 1;
  e->piece_floats = first;
  if (rc == kNcclSuccess && e->tok_grads_live) {
    const int64_t o = e->poff[PLB_TOK_W];
    rc = g_rccl.AllReduce(e->grads + o, e->grads + o, (size_t)(e->ptotal - o), kNcclFloat32, kNcclSum, e->comm, s);
    e->piece_count = 2;
    e->piece_floats += e->ptotal - o;
  }
  if (rc != kNcclSuccess) return fail("ncclAllReduce: %s", g_rccl.GetErrorString(rc));
  e->grads_reduced = true;
  return 0;
}
