// fp8 mode of the engine: the delayed-scaling state machine (which calls run on 1-byte images, the per-site and per-weight
// scales, the e4m3 weight copies) and plb_set_fp8 / plb_fp8_state / plb_fp8_stats. Sites and weight copies are named in
// engine_internal.h. Only writer of fp8_on and fp8_wstale; clears fp8_ready / fp8_bwd_ready, which the call stages arm.
#include "engine_internal.h"

int f8_site(const PlbEngine* e, int site, int l) { return site * e->L + l; }
static int f8_w(const PlbEngine* e, int w) { return F8_NSITE * e->L + w; }
static float* f8_amax(const PlbEngine* e, int i) { return e->at<float>(e->o_f8amax) + (int64_t)i * F8_AMAX_WORDS; }
static float* f8_scale(const PlbEngine* e, int i) { return e->at<float>(e->o_f8scale) + i; }
float* f8_deq(const PlbEngine* e, int i) { return e->at<float>(e->o_f8deq) + i; }
// every GEMM of the fp8 set has a plan at this token count (else the whole call runs in bf16): the four products of the
// forward on e4m3 activations, the four dX products of the backward on e5m2 gradients (the fused forms are taken where
// they have a plan too, the unfused ones must exist)
static bool fp8_shapes_ok(const PlbEngine* e, int64_t Tp) {
  const int H = e->H, I = e->I;
  if (!(H == 768 || H == 1024)) return false;
  const struct { int N, K, form, ops; } set[8] = {
      {3 * H, H, PLB_NT_PLAIN, PLB_NT_FP8_E4M3}, {H, H, PLB_NT_PLAIN, PLB_NT_FP8_E4M3}, {I, H, PLB_NT_GELU, PLB_NT_FP8_E4M3},
      {H, I, PLB_NT_PLAIN, PLB_NT_FP8_E4M3}, {I, H, PLB_NT_GELUBWD, PLB_NT_FP8_E5M2}, {H, I, PLB_NT_PLAIN, PLB_NT_FP8_E5M2},
      {H, H, PLB_NT_PLAIN, PLB_NT_FP8_E5M2}, {H, 3 * H, PLB_NT_PLAIN, PLB_NT_FP8_E5M2}};
  for (const auto& g : set)
    if (nt_plan(Tp, g.N, g.K, g.form, g.ops).rc) return false;
  return true;
}
// per-tensor e4m3 copies of the fp8 GEMMs' weights.
// exact = true (after plb_sync_weights / plb_set_fp8: the weights may be anything): maximum, scale, quantisation — three
//   passes. exact = false (after an AdamW step): ONE launch quantises all copies with the scale the previous
//   quantisation's maxima give and records the new maxima (a weight moves by <= lr per step; values are clamped).
int fp8_quantize_weights(PlbEngine* e, hipStream_t s, bool exact) {
  const int H = e->H, I = e->I;
  struct W { int w; const void* src; int bf16; int rows, cols; int64_t dst; } ws[F8W_N] = {
      {F8W_QKV, e->par(PLB_Q_W), 0, 3 * H, H, e->o_wq8},
      {F8W_D, e->par(PLB_DENSE_W), 0, H, H, e->o_wd8},
      {F8W_1, e->par(PLB_FFN_W), 0, I, H, e->o_w18},
      {F8W_2, e->par(PLB_FFNO_W), 0, H, I, e->o_w28},
      {F8W_2T, e->infer ? nullptr : e->at<bf16_t>(e->o_w2T), 1, I, H, e->o_w2T8},
      {F8W_1T, e->infer ? nullptr : e->at<bf16_t>(e->o_w1T), 1, H, I, e->o_w1T8},
      {F8W_QKVT, e->infer ? nullptr : e->at<bf16_t>(e->o_wqkvT), 1, H, 3 * H, e->o_wqT8},
      {F8W_DT, e->infer ? nullptr : e->at<bf16_t>(e->o_wdT), 1, H, H, e->o_wdT8}};
  if (exact) {
    HIPTRY(hipMemsetAsync(f8_amax(e, f8_w(e, 0)), 0, F8W_N * F8_AMAX_WORDS * sizeof(float), s));
    for (auto& w : ws) {
      if (!w.src) continue;
      TRY(plb_launch_amax(w.src, w.bf16, (size_t)w.rows, w.cols, w.cols, f8_amax(e, f8_w(e, w.w)), s));
    }
  }
  // amax -> scale (and the maxima are cleared: the quantisation below records this step's)
  TRY(plb_launch_fp8_scales(f8_amax(e, f8_w(e, 0)), f8_scale(e, f8_w(e, 0)), f8_deq(e, f8_w(e, 0)), F8W_N, 448.f, 1, s));
  const void* src[8]; int bf[8]; size_t n[8]; const float* sc[8]; uint8_t* dst[8]; float* am[8];
  int k = 0;
  for (auto& w : ws) {
    if (!w.src) continue;
    src[k] = w.src; bf[k] = w.bf16; n[k] = (size_t)w.rows * w.cols; sc[k] = f8_scale(e, f8_w(e, w.w));
    dst[k] = e->at<uint8_t>(w.dst); am[k] = f8_amax(e, f8_w(e, w.w));
    ++k;
  }
  TRY(plb_launch_quantize_multi(k, src, bf, n, sc, dst, am, s));
  e->fp8_wstale = false;
  return 0;
}
// end of a call in fp8 mode: this call's maxima become the next call's scales (delayed scaling, history 1)
int fp8_update_scales(PlbEngine* e, hipStream_t s) {
  const int L = e->L;
  // One scale per SITE, shared by its L applications (their maxima are recorded per application): the weight-gradient
  // GEMMs sum the products of two images over all applications under one dequantisation factor.
  // X, A, G, C: e4m3, 448. Gradients (DP, DU, DP1, DQ): e5m2, mapped to HALF the format's range — a step whose gradients
  // are up to 2x the previous step's (a smaller batch: the loss is a mean over samples) still fits; five exponent bits
  // have the binade to spare. One launch for the whole site table.
  // Every site: the scale comes from the LARGEST maximum of the last four calls (a call whose gradients are a multiple of the
  // previous call's — or whose batch simply has larger activations than the previous one: alternating batches clamped the
  // gelu site in a third of the calls of a 20,000-step soak under a history of one — is clamped only beyond that), and every
  // site counts the calls in which values were clamped (plb_fp8_stats): a clamped step is visible instead of silent.
  TRY(plb_launch_fp8_scales2(f8_amax(e, 0), f8_scale(e, 0), f8_deq(e, 0), 8 * L, 448.f, L, 4 * L, 28672.f,
                             e->at<float>(e->o_f8stats), 0, s));
  return 0;
}
F8Site::F8Site(const PlbEngine* e, int kind, int l) {
  const int i = f8_site(e, kind, l);
  scale = f8_scale(e, i); amax = f8_amax(e, i); deq = f8_deq(e, i);
}
F8Weight::F8Weight(const PlbEngine* e, int w) {
  static const int64_t PlbEngine::*const kImage[F8W_N] = {&PlbEngine::o_wq8, &PlbEngine::o_wd8, &PlbEngine::o_w18,
                                                           &PlbEngine::o_w28, &PlbEngine::o_w2T8, &PlbEngine::o_w1T8,
                                                           &PlbEngine::o_wqT8, &PlbEngine::o_wdT8};
  img = e->at<uint8_t>(e->*kImage[w]); deq = f8_deq(e, f8_w(e, w));
}
bool f8_call(const PlbEngine* e, int64_t Tp, bool train) {
  return e->fp8_on && e->fp8_ready && (!train || e->fp8_bwd_ready) && fp8_shapes_ok(e, Tp);
}
// Shapes of a call whose weight gradients may read the 1-byte images: each of the four layer weights goes to the pipeline
// kernel in bf16 (gemm_tn_plan.h: 256-column multiples, 8192 rows and more) and has an fp8 form.
bool tn8_ok(const PlbEngine* e, int64_t Mtot) {
  const int H = e->H, I = e->I, shapes[4][2] = {{3 * H, H}, {H, H}, {I, H}, {H, I}};
  for (const auto& nk : shapes) {
    PlbGemmTNPlan bf, f8;
    if (plb_gemm_tn_plan(Mtot, nk[0], nk[0], nk[1], PLB_TN_BF16, &bf) || bf.kernel != PLB_TN_PIPELINE) return false;
    if (plb_gemm_tn_plan(Mtot, nk[0], nk[0], nk[1], PLB_TN_FP8, &f8)) return false;
  }
  return true;
}

extern "C" int plb_set_fp8(PlbEngine* e, int32_t on, void* stream) {
  if (!e || !e->ws) return fail("plb_set_fp8: engine not bound");
  drop_stash(e, "plb_set_fp8 was called since");
  if (on && !(e->H == 768 || e->H == 1024)) return fail("plb_set_fp8: the fp8 path needs hidden_size 768 or 1024");
  if (on && !e->fp8_on) {  // the first call afterwards runs in bf16 and calibrates the scales
    hipStream_t s = (hipStream_t)stream;
    HIPTRY(hipMemsetAsync(f8_amax(e, 0), 0, (size_t)e->f8n * F8_AMAX_WORDS * 4, s));
    HIPTRY(hipMemsetAsync(e->at<float>(e->o_f8stats), 0, 8 * 8 * 4, s));
    HIPTRY(hipMemsetAsync(f8_scale(e, 0), 0, (size_t)e->f8n * 4, s));   // "no scale yet": the calibration call's maxima are not overshoots
    e->fp8_ready = false;      // activation sites: armed by the first forward
    e->fp8_bwd_ready = false;  // gradient sites: armed by the first backward
    e->fp8_wstale = true;
  }
  e->fp8_on = on != 0;
  return 0;
}
extern "C" int plb_fp8_state(const PlbEngine* e, int32_t* enabled, int32_t* calibrated) {
  if (!e) return fail("plb_fp8_state: null engine");
  if (enabled) *enabled = e->fp8_on;
  if (calibrated) *calibrated = e->fp8_ready;
  return 0;
}

// Per operand site (X, A, G, C in e4m3; dpre2, dU, dpre1, dQKV in e5m2): calls since plb_set_fp8 in which the site's values
// exceeded the format's range under the delayed scale they were quantised with (those elements were clamped), and the
// worst overshoot (true maximum x scale / format maximum; <= 1 = never clamped). Synchronises `stream`.
extern "C" int plb_fp8_stats(PlbEngine* e, float clamped_calls[8], float worst_overshoot[8], void* stream) {
  if (!e || !e->ws) return fail("plb_fp8_stats: engine not bound");
  float st[64];
  HIPTRY(hipMemcpyAsync(st, e->at<float>(e->o_f8stats), sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPTRY(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < 8; ++i) {
    if (clamped_calls) clamped_calls[i] = st[i * 8 + 4];
    if (worst_overshoot) worst_overshoot[i] = st[i * 8 + 5];
  }
  return 0;
}
