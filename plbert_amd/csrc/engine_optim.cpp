// The optimizer path: gradient accumulation, the global gradient norm and every update entry point (include/plbert.h:
// plb_grad_accum_*, plb_grad_norm, plb_grad_norm_groups; plb_adamw_step, plb_adamw_step_clipped, plb_adamw_plan,
// plb_adamw_step_groups; plb_lamb_plan, plb_lamb_step). Host bookkeeping of a window of micro-steps plus launches of
// optim.hip and lamb.hip; no workspace of its own: the accumulator, the norm buffer and the LAMB buffer are the caller's.
// Only writer of PlbEngine's accumulation block (grads_fresh / norm_nparts are also reset by begin_training_call,
// engine_calls.cpp); after a LAST add it sets head_grads_live, tok_grads_live, pool_grads_live and grads_reduced to what the
// window accumulated.
// The four update entries share one preamble (begin_update) and, with the two norm entries, one description of the ranges a
// step covers (step_ranges); the hyper-parameter refusals are written once (check_groups).
#include <cmath>

#include "engine_internal.h"

void end_accum_window(PlbEngine* e, const char* by) {
  if (e && e->win_open) { e->win_open = false; e->win_closed_by = by; }
}

namespace {
// ---- what the update and norm entries share --------------------------------------------------------------------------------
// The texts an update entry leaves behind. drop_stash, drop_final and end_accum_window keep them by pointer: literals only.
struct Update { const char *who, *stash, *final_state, *window, *reads; };
#define UPDATE_ENTRY(fn, label)                                                                                      \
  {fn, fn " moved the weights since", fn " moved the weights since: ask between the loss call and the optimizer step", \
   fn " moved the weights", label " (reads the gradient buffer)"}

// The preamble of an update: bound, training engine, the entry's own refusals (`own`: 0 or what fail returned), and only
// then what changes state: the stash, the final hidden state and an open accumulation window end, the exchange is joined.
template <class Own>
int begin_update(PlbEngine* e, const Update& u, hipStream_t s, Own own) {
  if (!e || !e->ws || !e->grads || !e->m || !e->v) return fail("%s: optimizer buffers not bound", u.who);
  if (e->infer) return fail("%s: inference-only engine", u.who);
  if (own()) return 1;
  drop_stash(e, u.stash);
  drop_final(e, u.final_state);
  end_accum_window(e, u.window);
  if (join_comm(e, s)) return 1;
  HB_R(s, e->grads, e->ptotal * 4, u.reads);
  return 0;
}

// One range of the flat buffers that a step covers with a launch of its own. There are at most three: the trainable range up
// to the phoneme head (after plb_encode_bwd the head has no gradient: no update, as torch skips a parameter whose .grad is
// None; parameters, both moments and the bf16 copy of the head stay as they are); the pooler, which only a
// plb_encode_bwd_pooled call with a d_pooled (or a window of such calls) gives a gradient, and which shares the engine's step
// count as the phoneme head does; and the token head, which only dual-head steps train and which keeps its OWN step count:
// torch.optim.AdamW keeps one per parameter, so a head that starts training late gets its own bias correction. The pooler and
// the token head are never live together (plb_encode_bwd* clears tok_grads_live, a loss call clears pool_grads_live, an
// accumulation window that would hold both is refused), so the pooler takes the token head's slot of partial sums. It counts
// no left-out update of its own: word 1 counts the step for the engine's count, word 2 rewinds the token head's.
struct StepRange {
  int64_t a, b;          // [a, b); a is also the offset into params / grads / exp_avg / exp_avg_sq / the bf16 copy
  int step;              // the range's step count
  int skip_slot;         // which of the step's launches this is to the skip word
  int count_nonfinite;   // 1: the launch that counts an update left out for a non-finite norm (once per step)
  int part;              // where its partial sums of squares go behind the four result floats of a norm buffer
  bool token;
  size_t n() const { return (size_t)(b - a); }
};
// (tok_grads_live implies NT > 0: a dual-head call on an engine without a token head is refused before it sets the flag, and
// a LAST add sets it from a window that formed it with NT > 0)
template <class Launch>
int step_ranges(PlbEngine* e, int step, Launch launch) {
  const StepRange enc = {0, e->head_grads_live ? e->ptrain : e->poff[PLB_HEAD_W], step, 1, 1, 0, false};
  if (launch(enc)) return 1;
  if (e->pool_grads_live) {
    const StepRange pool = {e->poff[PLB_POOL_W], pool_end(e), step, 0, 0, PLB_NORM_PARTS, false};
    if (launch(pool)) return 1;
  }
  if (!e->tok_grads_live || e->NT <= 0) return 0;
  const StepRange tok = {e->poff[PLB_TOK_W], e->ptotal, e->tok_steps + 1, 2, 0, PLB_NORM_PARTS, true};
  return launch(tok) ? 1 : 0;
}
// An update launch of the token head counts its step: exactly where the launch is made, not where the range is described
void count_step(PlbEngine* e, const StepRange& r) { if (r.token) e->tok_steps = r.step; }

struct Bufs { float *p, *g, *m, *v; bf16_t* w; unsigned int* skip; };
Bufs bufs(const PlbEngine* e, const StepRange& r) {
  return {e->params + r.a, e->grads + r.a, e->m + r.a, e->v + r.a, e->at<bf16_t>(e->o_wbf) + r.a, e->at<unsigned int>(e->o_lnerr)};
}

// The norm of the ranges plb_adamw_step is about to step: one sum-of-squares launch per range (`sumsq`), each into its own
// slot of partials, or the partials a LAST add left (have_partials); then the finish launch.
template <class Sumsq>
int grad_norm(PlbEngine* e, bool have_partials, double grad_scale, double max_norm, float* norm_buf, hipStream_t s, Sumsq sumsq) {
  int nparts = e->norm_nparts;
  if (!have_partials) {
    if (join_comm(e, s)) return 1;
    nparts = 0;
    if (step_ranges(e, 1, [&](const StepRange& r) {
          HB_R(s, e->grads + r.a, r.n() * 4, r.token ? "gradient norm (reads the token head's gradients)"
                                                     : "gradient norm (reads the gradient buffer)");
          HB_W(s, norm_buf + 4 + r.part, PLB_NORM_PARTS * 4, "gradient norm (writes the partial sums)");
          nparts += PLB_NORM_PARTS;
          return sumsq(r, norm_buf + 4 + r.part);
        }))
      return 1;
    e->norm_nparts = 0;   // (these partials are not a LAST add's: a later have_partials call must not take them for such)
  }
  HB_R(s, norm_buf + 4, (size_t)nparts * 4, "gradient norm (reads the partial sums)");
  HB_W(s, norm_buf, 16, "gradient norm (writes norm, coefficient and flag)");
  TRY(plb_launch_grad_norm_finish(norm_buf + 4, nparts, grad_scale, max_norm, norm_buf, s));
  return 0;
}
}  // namespace

extern "C" int64_t plb_grad_norm_floats(const PlbEngine* e) {
  // 4 result floats + one set of partials per range a launch can cover on its own: encoder, phoneme head, token head
  return e ? 4 + 3 * (int64_t)PLB_NORM_PARTS : -1;
}

extern "C" int plb_grad_accum_bind(PlbEngine* e, float* accum) {
  if (!e) return fail("plb_grad_accum_bind: null engine");
  if ((uintptr_t)accum & 15) return fail("plb_grad_accum_bind: the buffer must be 16-byte aligned");
  end_accum_window(e, "plb_grad_accum_bind changed the buffer");
  e->accum = accum;
  return 0;
}

namespace {
struct Seg { int64_t a, b; int phase; };   // phase 4: sum of squares only
}

extern "C" int plb_grad_accum_add(PlbEngine* e, int32_t phase, float* norm_buf, void* stream) {
  if (!e) return fail("plb_grad_accum_add: null engine");
  if (e->infer) return fail("plb_grad_accum_add: inference-only engine");
  if (!e->accum) return fail("plb_grad_accum_add: no accumulation buffer bound (plb_grad_accum_bind)");
  if (phase < 0 || phase > 2) return fail("plb_grad_accum_add: phase %d is none of 0 (first), 1 (add), 2 (last)", phase);
  if (norm_buf && phase != 2) return fail("plb_grad_accum_add: partial sums belong to the LAST add (phase 2)");
  if ((uintptr_t)norm_buf & 15) return fail("plb_grad_accum_add: norm_buf must be 16-byte aligned");
  if (phase != 0 && !e->win_open)
    return fail("plb_grad_accum_add: phase %d without a FIRST add: no window is open (%s)", phase, e->win_closed_by);
  if (!e->grads_fresh)
    return fail("plb_grad_accum_add: the gradient buffer holds nothing new: no backward call has run since the last add "
                "(the same gradients would be added twice)");
  if (!e->ws || !e->grads) return fail("plb_grad_accum_add: gradient buffer not bound");
  if (phase != 0 && e->grads_reduced != e->win_reduced)
    return fail("plb_grad_accum_add: this micro-step's gradients are %s, the window's are %s", e->grads_reduced ? "all-reduced" : "local",
                e->win_reduced ? "all-reduced" : "local");
  // What this micro-step produced | what the window holds so far. The encoder range is always both.
  const bool head = e->head_grads_live, tok = e->tok_grads_live && e->NT > 0, pool = e->pool_grads_live;
  const bool uhead = phase == 0 ? false : e->win_head, utok = phase == 0 ? false : e->win_tok, upool = phase == 0 ? false : e->win_pool;
  if ((tok || utok) && (pool || upool))
    return fail("plb_grad_accum_add: this window would hold gradients of both the token head (a dual-head loss call) and the "
                "pooler (plb_encode_bwd_pooled with a d_pooled): the norm buffer has three sets of partial sums, and the two "
                "share one");
  hipStream_t s = (hipStream_t)stream;
  if (join_comm(e, s)) return 1;   // this micro-step's all-reduce pieces
  const bool want_sq = norm_buf != nullptr;
  auto pick = [&](bool produced, bool in_union) -> int {   // -1: nothing to launch
    if (phase == 0) return produced ? 0 : -1;
    if (phase == 1) return !produced ? -1 : in_union ? 1 : 0;   // a range that joins the window now starts from this copy
    if (produced) return in_union ? 2 : want_sq ? 4 : -1;       // ... and at LAST it already is the sum
    return in_union ? 3 : -1;                                   // zeros from this micro-step: its part of grads is not read
  };
  const int64_t hw = e->poff[PLB_HEAD_W], tw = e->poff[PLB_TOK_W];
  Seg seg[4];
  int nseg = 0;
  seg[nseg++] = Seg{0, hw, pick(true, phase != 0)};
  const int ph = pick(head, uhead);
  if (ph >= 0) {
    if (ph == seg[0].phase) seg[0].b = e->ptrain;   // adjacent and alike: one launch
    else seg[nseg++] = Seg{hw, e->ptrain, ph};
  }
  const int pp = pick(pool, upool);
  if (pp >= 0) {
    if (seg[nseg - 1].b == e->ptrain && seg[nseg - 1].phase == pp) seg[nseg - 1].b = pool_end(e);   // adjacent and alike again
    else seg[nseg++] = Seg{e->ptrain, pool_end(e), pp};
  }
  const int pt = e->NT > 0 ? pick(tok, utok) : -1;
  if (pt >= 0) seg[nseg++] = Seg{tw, e->ptotal, pt};
  int nparts = 0;
  for (int i = 0; i < nseg; ++i) {
    const Seg& g = seg[i];
    float* part = want_sq ? norm_buf + 4 + nparts : nullptr;
    const size_t n = (size_t)(g.b - g.a);
    if (g.phase != 3 && g.phase != 4) HB_R(s, e->grads + g.a, n * 4, "gradient accumulation (reads the gradient buffer)");
    if (g.phase == 4) HB_R(s, e->grads + g.a, n * 4, "sum of squares (reads the gradient buffer)");
    if (g.phase != 0 && g.phase != 4) HB_R(s, e->accum + g.a, n * 4, "gradient accumulation (reads the accumulator)");
    if (g.phase < 2) HB_W(s, e->accum + g.a, n * 4, "gradient accumulation (writes the accumulator)");
    if (g.phase == 2 || g.phase == 3) HB_W(s, e->grads + g.a, n * 4, "gradient accumulation (writes the gradient buffer)");
    if (part) HB_W(s, part, PLB_NORM_PARTS * 4, "gradient accumulation (writes the partial sums)");
    if (g.phase == 4) TRY(plb_launch_grad_sumsq(e->grads + g.a, n, part, s));
    else TRY(plb_launch_grad_accum(e->accum + g.a, e->grads + g.a, n, g.phase, part, s));
    if (part) nparts += PLB_NORM_PARTS;
  }
  e->grads_fresh = false;
  e->win_head = uhead || head;
  e->win_tok = utok || tok;
  e->win_pool = upool || pool;
  if (phase == 0) { e->win_open = true; e->win_reduced = e->grads_reduced; }
  if (phase == 2) {
    e->win_open = false;
    e->win_closed_by = "the LAST add closed it";
    // plb_allreduce_grads, plb_grad_norm and either AdamW entry now cover exactly what the window accumulated
    e->head_grads_live = e->win_head;
    e->tok_grads_live = e->win_tok;
    e->pool_grads_live = e->win_pool;
    e->grads_reduced = e->win_reduced;
    e->norm_src = norm_buf; e->norm_nparts = nparts; e->norm_reduced = e->grads_reduced;
  }
  return 0;
}

extern "C" int plb_grad_norm(PlbEngine* e, double grad_scale, double max_norm, float* norm_buf, int32_t have_partials,
                             void* stream) {
  if (!e) return fail("plb_grad_norm: null engine");
  if (e->infer) return fail("plb_grad_norm: inference-only engine");
  if (!norm_buf || ((uintptr_t)norm_buf & 15)) return fail("plb_grad_norm: norm_buf must be a 16-byte aligned device buffer");
  if (have_partials) {
    if (e->norm_src != norm_buf || e->norm_nparts < 1)
      return fail("plb_grad_norm: have_partials, but the last plb_grad_accum_add(LAST) left none in this buffer");
    if (e->grads_reduced != e->norm_reduced)
      return fail("plb_grad_norm: the partial sums were taken before the gradient exchange");
  }
  if (!e->ws || !e->grads) return fail("plb_grad_norm: gradient buffer not bound");
  hipStream_t s = (hipStream_t)stream;
  return grad_norm(e, have_partials != 0, grad_scale, max_norm, norm_buf, s, [&](const StepRange& r, float* partials) {
    TRY(plb_launch_grad_sumsq(e->grads + r.a, r.n(), partials, s));
    return 0;
  });
}

// ---- the plain and the clipped update (include/plbert.h: plb_adamw_step, plb_adamw_step_clipped) ---------------------------
extern "C" int plb_adamw_step(PlbEngine* e, double lr, double beta1, double beta2, double eps, double weight_decay,
                              int32_t step, double grad_scale, void* stream) {
  static const Update u = UPDATE_ENTRY("plb_adamw_step", "AdamW");
  hipStream_t s = (hipStream_t)stream;
  if (begin_update(e, u, s, [&] { return step < 1 ? fail("plb_adamw_step: step counts from 1") : 0; })) return 1;
  if (step_ranges(e, step, [&](const StepRange& r) {
        const Bufs x = bufs(e, r);
        count_step(e, r);
        TRY(plb_launch_adamw(x.p, x.g, x.m, x.v, x.w, r.n(), lr, beta1, beta2, eps, weight_decay, r.step, grad_scale, x.skip,
                             r.skip_slot, s));
        return 0;
      }))
    return 1;
  return sync_transposes(e, s, false);   // fp8 copies: delayed scaling from here on (the weights moved by one AdamW step)
}

extern "C" int plb_adamw_step_clipped(PlbEngine* e, double lr, double beta1, double beta2, double eps, double weight_decay,
                                      int32_t step, double grad_scale, const float* norm_buf, void* stream) {
  static const Update u = UPDATE_ENTRY("plb_adamw_step_clipped", "clipped AdamW");
  hipStream_t s = (hipStream_t)stream;
  if (begin_update(e, u, s, [&] {
        if (step < 1) return fail("plb_adamw_step_clipped: step counts from 1");
        return norm_buf ? 0 : fail("plb_adamw_step_clipped: norm_buf is null (plb_grad_norm writes it)");
      }))
    return 1;
  float* norm = const_cast<float*>(norm_buf);   // (the launch counts the updates it leaves out in norm[3])
  HB_W(s, norm, 16, "clipped AdamW (reads the coefficient, counts a left-out update)");
  if (step_ranges(e, step, [&](const StepRange& r) {
        const Bufs x = bufs(e, r);
        count_step(e, r);
        TRY(plb_launch_adamw_clipped(x.p, x.g, x.m, x.v, x.w, r.n(), lr, beta1, beta2, eps, weight_decay, r.step, grad_scale,
                                     x.skip, r.skip_slot, norm, r.count_nonfinite, s));
        return 0;
      }))
    return 1;
  return sync_transposes(e, s, false);
}

// ---- parameter groups and frozen tensors (include/plbert.h: plb_adamw_plan, plb_adamw_step_groups, plb_grad_norm_groups)
namespace {
// The tensors the next AdamW entry steps, whatever the caller's groups say: plb_adamw_step's ranges
bool steps_tensor(const PlbEngine* e, int i) {
  if (e->psize[i] == 0) return false;
  if (i == PLB_POOL_W || i == PLB_POOL_B) return e->pool_grads_live;
  if (i == PLB_HEAD_W || i == PLB_HEAD_B) return e->head_grads_live;
  if (i == PLB_TOK_W || i == PLB_TOK_B) return e->tok_grads_live && e->NT > 0;
  return true;
}
bool in_token_head(int i) { return i == PLB_TOK_W || i == PLB_TOK_B; }

int check_group_of(const PlbEngine* e, const int32_t* group_of, int32_t n_groups, const char* who) {
  if (!e) return fail("%s: null engine", who);
  if (!group_of) return fail("%s: group_of is null", who);
  if (n_groups < 1) return fail("%s: n_groups %d: there must be at least one group", who, n_groups);
  for (int i = 0; i < PLB_NPARAM; ++i)
    if (group_of[i] < -1 || group_of[i] >= n_groups)
      return fail("%s: group_of[%d] = %d is outside [-1, %d)", who, i, group_of[i], n_groups);
  return 0;
}

// The scalars of one group at one step count: formed in double, rounded once (optim.hip: plb_launch_adamw)
void group_scalars(const PlbAdamWGroup& g, int step, PlbAdamWSegment* s) {
  const double bc1 = 1.0 - pow(g.beta1, step), bc2 = 1.0 - pow(g.beta2, step);
  s->step = step;
  s->decay = (float)(1.0 - g.lr * g.weight_decay);
  s->omb1 = (float)(1.0 - g.beta1);
  s->b2 = (float)g.beta2;
  s->omb2 = (float)(1.0 - g.beta2);
  s->eps = (float)g.eps;
  s->step_size = (float)(g.lr / bc1);
  s->bc2_sqrt = (float)sqrt(bc2);
}
bool same_scalars(const PlbAdamWSegment& a, const PlbAdamWSegment& b) {
  return a.group == b.group && a.step == b.step && !memcmp(&a.decay, &b.decay, 7 * sizeof(float));
}

// groups == null: the live tensors only (plb_grad_norm_groups), merged wherever they are adjacent
int plan_segments(const PlbEngine* e, const PlbAdamWGroup* groups, const int32_t* group_of, int32_t step,
                  PlbAdamWSegment* segs) {
  int n = 0;
  for (int i = 0; i < PLB_NPARAM; ++i) {
    if (group_of[i] < 0 || !steps_tensor(e, i)) continue;
    PlbAdamWSegment s;
    memset(&s, 0, sizeof(s));
    s.begin = e->poff[i];
    s.end = e->poff[i] + e->psize[i];
    s.step = 1;
    if (groups) {
      s.group = group_of[i];
      group_scalars(groups[group_of[i]], in_token_head(i) ? e->tok_steps + 1 : step, &s);
    }
    // (a segment never reaches from one launch of step_ranges into the next: none is merged across PLB_POOL_W, and a dead
    // pooler lies between the trainable range and the token head)
    if (n && i != PLB_POOL_W && segs[n - 1].end == s.begin && same_scalars(segs[n - 1], s)) segs[n - 1].end = s.end;
    else segs[n++] = s;
  }
  return n;
}

// The hyper-parameter refusals of both group types; LAMB's adapt is checked on top, group by group
int check_adapt(const PlbAdamWGroup&, int, const char*) { return 0; }
int check_adapt(const PlbLambGroup& g, int k, const char* who) {
  return g.adapt != 0 && g.adapt != 1 ? fail("%s: group %d: adapt %d is neither 0 nor 1", who, k, g.adapt) : 0;
}
template <class Group>
int check_groups(const Group* groups, int32_t n_groups, int32_t step, const char* who) {
  if (!groups) return fail("%s: groups is null", who);
  for (int k = 0; k < n_groups; ++k) {
    const Group& g = groups[k];
    if (!(g.lr >= 0.0) || !std::isfinite(g.lr)) return fail("%s: group %d: lr %g is negative or not finite", who, k, g.lr);
    if (!(g.eps >= 0.0) || !std::isfinite(g.eps)) return fail("%s: group %d: eps %g is negative or not finite", who, k, g.eps);
    if (!(g.beta1 >= 0.0 && g.beta1 < 1.0)) return fail("%s: group %d: beta1 %g is outside [0, 1)", who, k, g.beta1);
    if (!(g.beta2 >= 0.0 && g.beta2 < 1.0)) return fail("%s: group %d: beta2 %g is outside [0, 1)", who, k, g.beta2);
    if (!std::isfinite(g.weight_decay)) return fail("%s: group %d: weight_decay is not finite", who, k);
    if (check_adapt(g, k, who)) return 1;
  }
  if (step < 1) return fail("%s: step counts from 1", who);
  return 0;
}

// The segments of [a, b) among segs, rebased to a
template <class Segment>
int range_segments(const Segment* segs, int n, int64_t a, int64_t b, Segment* out) {
  int k = 0;
  for (int i = 0; i < n; ++i)
    if (segs[i].begin >= a && segs[i].end <= b) {
      out[k] = segs[i];
      out[k].begin -= a;
      out[k++].end -= a;
    }
  return k;
}
}  // namespace

extern "C" int plb_adamw_plan(const PlbEngine* e, const PlbAdamWGroup* groups, int32_t n_groups, const int32_t* group_of,
                              int32_t step, PlbAdamWSegment* segs, int32_t* n_segs) {
  if (check_group_of(e, group_of, n_groups, "plb_adamw_plan")) return 1;
  if (check_groups(groups, n_groups, step, "plb_adamw_plan")) return 1;
  if (!segs || !n_segs) return fail("plb_adamw_plan: null output");
  if (e->infer) return fail("plb_adamw_plan: inference-only engine");
  *n_segs = plan_segments(e, groups, group_of, step, segs);
  return 0;
}

extern "C" int plb_adamw_step_groups(PlbEngine* e, const PlbAdamWGroup* groups, int32_t n_groups, const int32_t* group_of,
                                     int32_t step, double grad_scale, const float* norm_buf, void* stream) {
  static const Update u = UPDATE_ENTRY("plb_adamw_step_groups", "grouped AdamW");
  hipStream_t s = (hipStream_t)stream;
  if (begin_update(e, u, s, [&] { return check_group_of(e, group_of, n_groups, u.who) || check_groups(groups, n_groups, step, u.who); }))
    return 1;
  float* norm = const_cast<float*>(norm_buf);   // (the launch counts the updates it leaves out in norm[3])
  if (norm) HB_W(s, norm, 16, "grouped AdamW (reads the coefficient, counts a left-out update)");
  PlbAdamWSegment all[PLB_NPARAM], part[PLB_NPARAM];
  const int n = plan_segments(e, groups, group_of, step, all);
  if (step_ranges(e, step, [&](const StepRange& r) {
        const int k = range_segments(all, n, r.a, r.b, part);
        if (!k) return 0;   // a range without a live segment launches nothing
        const Bufs x = bufs(e, r);
        count_step(e, r);   // (the plan gave the token head's segments this count)
        TRY(plb_launch_adamw_segments(x.p, x.g, x.m, x.v, x.w, (size_t)part[k - 1].end, part, k, grad_scale, x.skip,
                                      r.skip_slot, norm, r.count_nonfinite, s));
        return 0;
      }))
    return 1;
  return sync_transposes(e, s, false);
}

extern "C" int plb_grad_norm_groups(PlbEngine* e, const int32_t* group_of, double grad_scale, double max_norm, float* norm_buf,
                                    void* stream) {
  if (!e) return fail("plb_grad_norm_groups: null engine");
  if (e->infer) return fail("plb_grad_norm_groups: inference-only engine");
  if (check_group_of(e, group_of, 1 << 30, "plb_grad_norm_groups")) return 1;
  if (!norm_buf || ((uintptr_t)norm_buf & 15)) return fail("plb_grad_norm_groups: norm_buf must be a 16-byte aligned device buffer");
  if (!e->ws || !e->grads) return fail("plb_grad_norm_groups: gradient buffer not bound");
  hipStream_t s = (hipStream_t)stream;
  PlbAdamWSegment all[PLB_NPARAM], part[PLB_NPARAM];
  const int n = plan_segments(e, nullptr, group_of, 1, all);
  // plb_grad_norm's ranges, grids and partial slots; holes contribute exact zeros
  return grad_norm(e, false, grad_scale, max_norm, norm_buf, s, [&](const StepRange& r, float* partials) {
    TRY(plb_launch_grad_sumsq_segments(e->grads + r.a, r.n(), part, range_segments(all, n, r.a, r.b, part), partials, s));
    return 0;
  });
}

// ---- LAMB (include/plbert.h: plb_lamb_floats, plb_lamb_plan, plb_lamb_step; kernels: lamb.hip)
namespace {
// lamb_buf: [4 * PLB_NPARAM results][partials of the trainable range][partials of the token head, or of the pooler: the two
// are never live together]. A range of n floats in k tensors has at most n / 1024 + k workgroups (one pair of floats each).
int64_t lamb_main_pairs(const PlbEngine* e) { return e->ptrain / 1024 + PLB_NPARAM; }
int64_t lamb_tok_pairs(const PlbEngine* e) {
  const int64_t tok = e->ptotal - e->poff[PLB_TOK_W], pool = pool_end(e) - e->poff[PLB_POOL_W];
  return (tok > pool ? tok : pool) / 1024 + 2;
}

// One segment per live tensor, never merged: the trust ratio is a tensor's own
int plan_lamb(const PlbEngine* e, const PlbLambGroup* groups, const int32_t* group_of, int32_t step, PlbLambSegment* segs) {
  int n = 0;
  for (int i = 0; i < PLB_NPARAM; ++i) {
    if (group_of[i] < 0 || !steps_tensor(e, i)) continue;
    const PlbLambGroup& g = groups[group_of[i]];
    const PlbAdamWGroup a = {g.lr, g.beta1, g.beta2, g.eps, g.weight_decay};
    PlbAdamWSegment sc;
    const int k = in_token_head(i) ? e->tok_steps + 1 : step;
    group_scalars(a, k, &sc);   // the AdamW scalars: omb1, b2, omb2, eps and sqrt(bc2) are shared bit for bit
    PlbLambSegment s;
    memset(&s, 0, sizeof(s));
    s.begin = e->poff[i];
    s.end = e->poff[i] + e->psize[i];
    s.tensor = i;
    s.group = group_of[i];
    s.step = k;
    s.adapt = g.adapt;
    s.omb1 = sc.omb1; s.b2 = sc.b2; s.omb2 = sc.omb2; s.eps = sc.eps; s.bc2_sqrt = sc.bc2_sqrt;
    s.inv_bc1 = (float)(1.0 / (1.0 - pow(g.beta1, k)));
    s.weight_decay = (float)g.weight_decay;
    s.lr = (float)g.lr;
    segs[n++] = s;
  }
  return n;
}
}  // namespace

extern "C" int64_t plb_lamb_floats(const PlbEngine* e) {
  return e ? (4 * (int64_t)PLB_NPARAM + 2 * (lamb_main_pairs(e) + lamb_tok_pairs(e)) + 3) / 4 * 4 : -1;
}

extern "C" int plb_lamb_plan(const PlbEngine* e, const PlbLambGroup* groups, int32_t n_groups, const int32_t* group_of,
                             int32_t step, PlbLambSegment* segs, int32_t* n_segs) {
  if (check_group_of(e, group_of, n_groups, "plb_lamb_plan")) return 1;
  if (check_groups(groups, n_groups, step, "plb_lamb_plan")) return 1;
  if (!segs || !n_segs) return fail("plb_lamb_plan: null output");
  if (e->infer) return fail("plb_lamb_plan: inference-only engine");
  *n_segs = plan_lamb(e, groups, group_of, step, segs);
  return 0;
}

extern "C" int plb_lamb_step(PlbEngine* e, const PlbLambGroup* groups, int32_t n_groups, const int32_t* group_of, int32_t step,
                             double grad_scale, const float* norm_buf, float* lamb_buf, void* stream) {
  static const Update u = UPDATE_ENTRY("plb_lamb_step", "LAMB");
  hipStream_t s = (hipStream_t)stream;
  if (begin_update(e, u, s, [&] {
        if (check_group_of(e, group_of, n_groups, u.who) || check_groups(groups, n_groups, step, u.who)) return 1;
        return !lamb_buf || ((uintptr_t)lamb_buf & 15) ? fail("plb_lamb_step: lamb_buf must be a 16-byte aligned device buffer") : 0;
      }))
    return 1;
  float* norm = const_cast<float*>(norm_buf);   // (pass 1 counts the updates it leaves out in norm[3])
  if (norm) HB_W(s, norm, 16, "LAMB (reads the coefficient, counts a left-out update)");
  HB_W(s, lamb_buf, plb_lamb_floats(e) * 4, "LAMB (writes the partial sums and the trust ratios)");
  PlbLambSegment all[PLB_NPARAM], part[PLB_NPARAM];
  const int n = plan_lamb(e, groups, group_of, step, all);
  // A range without a live tensor launches nothing. The finishes of the ranges that do run share the result slots between
  // them, cut at the first tensor of each later range: every tensor that is in no range's table is marked as a hole.
  StepRange run[3];
  int nrun = 0;
  if (step_ranges(e, step, [&](const StepRange& r) {
        if (range_segments(all, n, r.a, r.b, part)) run[nrun++] = r;
        return 0;
      }))
    return 1;
  auto first_tensor = [&](const StepRange& r) { int i = 0; while (e->poff[i] < r.a) ++i; return i; };
  int ri = 0;
  if (step_ranges(e, step, [&](const StepRange& r) {
        const int k = range_segments(all, n, r.a, r.b, part);
        if (!k) return 0;
        const int lo = ri == 0 ? 0 : first_tensor(run[ri]), hi = ri + 1 < nrun ? first_tensor(run[ri + 1]) : (int)PLB_NPARAM;
        ++ri;
        const Bufs x = bufs(e, r);
        const size_t nn = (size_t)part[k - 1].end;
        float* partials = lamb_buf + 4 * PLB_NPARAM + (r.a ? 2 * lamb_main_pairs(e) : 0);   // (the pooler in the token head's place)
        count_step(e, r);   // (the plan gave the token head's tensors this count)
        TRY(plb_launch_lamb_pass1(x.p, x.g, x.m, x.v, nn, part, k, grad_scale, x.skip, r.skip_slot, norm, r.count_nonfinite,
                                  partials, s));
        TRY(plb_launch_lamb_finish(part, k, nn, lo, hi, partials, lamb_buf, x.skip, norm, s));
        TRY(plb_launch_lamb_pass2(x.p, x.m, x.v, x.w, nn, part, k, lamb_buf, x.skip, norm, s));
        return 0;
      }))
    return 1;
  return sync_transposes(e, s, false);
}
