// s4p_icp_pass.inc -- what one call runs on the device and the one refine loop: what a pass needs beforehand (prepare), the
// six passes over one search / finish skeleton, the source order of a refine, and refine_loop.

namespace {

// a validated s4p_icp_robust: the loss, the selection and its inputs
struct RobustCfg {
  int32_t loss = 0;
  int mode = kSelNone;
  uint64_t kq = 0;          // TRIMMED: ceil(trim_fraction * n_Q)
  double scale = 0.0, c = 0.0, smin = 0.0;
};

int32_t robust_cfg(s4p_icp_ctx* h, int32_t metric, const s4p_icp_robust* R, RobustCfg* out) {
  if (!R) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: null parameters");
  if (metric != S4P_ICP_METRIC_POINT && metric != S4P_ICP_METRIC_PLANE) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: unknown metric");
  RobustCfg C;
  C.loss = R->loss;
  C.smin = 1e-6 * double(h->d);
  if (R->loss == S4P_ICP_LOSS_TRIMMED) {
    if (!(R->trim_fraction > 0.0 && R->trim_fraction <= 1.0))
      return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: trim_fraction must be in (0, 1]");
    C.mode = kSelTrim;
    C.kq = uint64_t(std::ceil(R->trim_fraction * double(h->n_q)));
  } else if (R->loss == S4P_ICP_LOSS_HUBER || R->loss == S4P_ICP_LOSS_TUKEY) {
    if (!(R->c > 0.0) || !std::isfinite(R->c)) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: c must be finite and > 0");
    if (std::isnan(R->scale) || !(R->scale < INFINITY)) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: scale must be finite");
    C.c = R->c;
    C.scale = R->scale > 0.0 ? R->scale : 0.0;
    C.mode = R->scale > 0.0 ? kSelNone : kSelMedian;
  } else {
    return fail(h, S4P_ICP_ERR_BAD_ARG, "robust: unknown loss");
  }
  *out = C;
  return S4P_ICP_OK;
}

// What a sums call or a refine minimises: the metric, its parameter, and for the robust variants the validated loss.
enum Metric { kPoint = 0, kPlane = 1, kGicp = 2, kColor = 3, kSymm = 4, kInfo = 5 };   // kInfo: the information sums, no refine
struct PassKind {
  int metric = kPoint;
  double param = 0.0;       // generalized: epsilon; coloured: lambda
  bool robust = false;      // point / plane on the weighted sums of cfg
  RobustCfg cfg;
  bool plane() const { return metric != kPoint; }                                  // the 31 sums and their 6x6 solve
  int nsums() const { return metric == kInfo ? S4P_ICP_INFO_NSUMS : (plane() ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS); }
};

// the sums of one pass on the host; n: the correspondence count (sums[0], or the robust count with w > 0)
struct PassOut {
  double sums[kSumsCap];
  double n;
  double info[S4P_ICP_ROBUST_NINFO];
};

int32_t ready_for(s4p_icp_ctx* h, const PassKind& K) {
  if (K.metric == kGicp) return gicp_ready(h, K.param);
  if (K.metric == kColor) return color_ready(h, K.param);
  if (K.metric == kSymm) return symm_ready(h);
  if (K.metric == kInfo) return ready(h);
  return K.plane() ? plane_ready(h) : ready(h);
}

// the one place the plane slab is allocated
int32_t plane_slab(s4p_icp_ctx* h) { ICP_HIP(h->pslab.ensure(size_t(kMaxBlocks) * kPlanePitch)); return S4P_ICP_OK; }

// the stored source normals in the order of `src` (w = original source index), for the generalized and symmetric sums and
// the normal test
int32_t gather_source_normals(s4p_icp_ctx* h, const float4* src) {
  ICP_LAUNCH(k_gather_source_normals, blocks_for(h->n_q), h->sn[0], h->sn[1], h->sn[2], src, uint64_t(h->n_q), h->snrm);
  return S4P_ICP_OK;
}

// the plain point / plane metrics under rejection run robust_pass with every weight 1
bool weighted(const s4p_icp_ctx* h, const PassKind& K) { return K.robust || (h->rej_on && K.metric <= kPlane); }

// Before the passes of a sums call or a refine of kind K over `src` (K null: s4p_icp_rejection, which has no sums and
// always rejects): every buffer they use, each on its first use, and what the metric and the rejection read in src's order
// (the source normals, gathered once whoever needs them; the source intensities), the rejection's counters and the source
// grid (reciprocity).  Nothing is built or allocated inside the iteration loop.
int32_t prepare(s4p_icp_ctx* h, const float4* src, const PassKind* K) {
  // gicp: a metric that reads the source normals (generalized, symmetric)
  const bool rej = h->rej_on || !K, gicp = K && (K->metric == kGicp || K->metric == kSymm), color = K && K->metric == kColor;
  const bool info = K && K->metric == kInfo;
  const bool nm = rej && h->rej.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  if (nm && !h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "rejection by normals: target normals first (set_target_normals or estimate_normals)");
  if (nm && !h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "rejection by normals: source normals first (set_source_normals)");
  if (rej || gicp || color || info || (K && K->robust)) {            // a split pass: k_search's slots and keys
    ICP_HIP(h->rslot.ensure(size_t(h->n_q)));
    ICP_HIP(h->rkey.ensure(size_t(h->n_q)));
  }
  // the information pass writes its 11 sums into rows of the plane slab (kInfo also counts as plane() below: metric != kPoint)
  if (rej || info || (K && K->plane())) if (int32_t rc = plane_slab(h)) return rc;
  if (K && weighted(h, *K)) {
    constexpr int kOut = S4P_ICP_PLANE_NSUMS + S4P_ICP_ROBUST_NINFO;
    ICP_HIP(h->rhist.ensure(kDigits * kBins));
    ICP_HIP(h->rst.ensure(1));
    ICP_HIP(h->rsum.ensure(kOut));
    ICP_HIP(h->rhsum.ensure(kOut));
  }
  if (gicp) if (int32_t rc = gather_source_normals(h, src)) return rc;
  if (color) ICP_LAUNCH(k_gather_source_intensity, blocks_for(h->n_q), h->si, src, uint64_t(h->n_q), h->sint);
  if (rej) {
    ICP_HIP(h->rcnt.ensure(4));
    ICP_HIP(h->rhcnt.ensure(4));
    if (h->rej.reciprocal) if (int32_t rc = source_grid_ready(h)) return rc;
    if (nm && !gicp) if (int32_t rc = gather_source_normals(h, src)) return rc;
  }
  return S4P_ICP_OK;
}

// T- of include/s4p_icp_reject.h: the transposed float entries and t-_a = float(-((m_0a t_0 + m_1a t_1) + m_2a t_2)) in double
Tf reverse_map(const Tf& T) {
  Tf R;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) R.m[4 * a + b] = T.m[4 * b + a];
    R.m[4 * a + 3] = float(-((double(T.m[a]) * double(T.m[3]) + double(T.m[4 + a]) * double(T.m[7])) + double(T.m[8 + a]) * double(T.m[11])));
  }
  return R;
}

// k_reject on the slots and keys k_search has just written for (T, src), after prepare for this src; the counters follow
// the pass's sums to the host (reject_done after the pass's synchronisation).  code: optional, per visited lane.
int32_t launch_reject(s4p_icp_ctx* h, const Tf& T, const float4* src, uint8_t* code) {
  ICP_HIP(hipMemsetAsync(h->rcnt, 0, 4 * sizeof(unsigned long long), h->st));
  RejectArgs A;
  A.T = T; A.Ti = reverse_map(T); A.g = h->g; A.gs = h->gs; A.src = src; A.snrm = h->snrm; A.nrm = h->nrm; A.n = uint64_t(h->n_q);
  A.d2max = h->d2max; A.oriented = h->rej.normal_mode == S4P_ICP_REJECT_NORMALS_ORIENTED; A.ncos = h->rej.normal_cos;
  A.slot = h->rslot; A.key = h->rkey; A.code = code; A.counts = h->rcnt;
  const int nb = blocks_for(h->n_q);
  const bool rc = h->rej.reciprocal != 0, nm = h->rej.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  if (rc && nm) ICP_LAUNCH((k_reject<true, true>), nb, A);
  else if (rc) ICP_LAUNCH((k_reject<true, false>), nb, A);
  else if (nm) ICP_LAUNCH((k_reject<false, true>), nb, A);
  else ICP_LAUNCH((k_reject<false, false>), nb, A);      // s4p_icp_rejection with everything off
  ICP_HIP(hipMemcpyAsync(h->rhcnt, h->rcnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
  h->rej_pending = true;
  return S4P_ICP_OK;
}

// after the synchronisation that follows launch_reject
void reject_done(s4p_icp_ctx* h) {
  for (int k = 0; k < 4; ++k) h->rej_counts[k] = int64_t(h->rhcnt[k]);
  h->rej_pending = false;
}

// The one correspondence search of a split pass: the winner's slot and residual key per visited lane of (T, src), and the
// rejection behind it when it is on (or when the caller wants the per-lane code: s4p_icp_rejection).
int32_t launch_search(s4p_icp_ctx* h, const Tf& T, const float4* src, bool plane, uint8_t* code = nullptr) {
  SearchArgs S;
  S.T = T; S.g = h->g; S.src = src; S.nrm = h->nrm; S.n = uint64_t(h->n_q); S.d2max = h->d2max; S.slot = h->rslot; S.key = h->rkey;
  if (plane) ICP_LAUNCH(k_search<true>, blocks_for(h->n_q), S);
  else ICP_LAUNCH(k_search<false>, blocks_for(h->n_q), S);
  if (h->rej_on || code) return launch_reject(h, T, src, code);
  return S4P_ICP_OK;
}

// The end of every pass, behind its final kernel: `count` doubles from dev through the pinned host buffer to out with the
// pass's one synchronisation, and the counters of a rejection that ran in it.
int32_t finish_pass(s4p_icp_ctx* h, const double* dev, double* host, int count, double* out) {
  ICP_HIP(hipMemcpyAsync(host, dev, count * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipEventRecord(h->ev, h->st));
  ICP_HIP(hipEventSynchronize(h->ev));
  std::memcpy(out, host, count * sizeof(double));
  if (h->rej_pending) reject_done(h);
  return S4P_ICP_OK;
}

// One robust pass: one search, the selection, the weighted sums; sums and info on the host.  With the loss kLossOnes: the
// plain point / plane sums under rejection (every weight 1: s4p_icp_sums' / s4p_icp_plane_sums' bits on the surviving pairs,
// as include/s4p_icp_robust.h states).
int32_t robust_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, bool plane, const RobustCfg& C, double* sums, double* info) {
  const uint64_t un = uint64_t(h->n_q);
  const int nb = blocks_for(h->n_q);
  ICP_HIP(hipMemsetAsync(h->rhist, 0, kDigits * kBins * sizeof(uint32_t), h->st));
  ICP_HIP(hipMemsetAsync(h->rst, 0, sizeof(SelState), h->st));
  if (int32_t rc = launch_search(h, T, src, plane)) return rc;
  const int passes = C.mode == kSelNone ? 1 : kDigits;         // without a selection, pass 0 still counts M
  for (int p = 0; p < passes; ++p) {
    ICP_LAUNCH(k_key_hist, nb, h->rkey, un, p, h->rst, h->rhist + p * kBins);
    ICP_LAUNCH(k_key_digit, 1, h->rhist + p * kBins, p, p == passes - 1, C.mode, C.kq, C.scale, C.c, C.smin, h->rst);
  }
  WsumArgs W;
  W.T = T; W.g = h->g; W.src = src; W.nrm = h->nrm; W.n = un; W.slot = h->rslot; W.st = h->rst; W.loss = C.loss;
  W.slab = plane ? h->pslab : h->slab;
  if (plane) {
    ICP_LAUNCH(k_wsum<true>, nb, W);
    ICP_LAUNCH(k_wfinal<true>, 1, W.slab, nb, h->rst, h->rsum);
  } else {
    ICP_LAUNCH(k_wsum<false>, nb, W);
    ICP_LAUNCH(k_wfinal<false>, 1, W.slab, nb, h->rst, h->rsum);
  }
  const int ns = plane ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  double all[S4P_ICP_PLANE_NSUMS + 5];
  if (int32_t rc = finish_pass(h, h->rsum, h->rhsum, ns + 5, all)) return rc;
  std::memcpy(sums, all, ns * sizeof(double));
  for (int k = 0; k < S4P_ICP_ROBUST_NINFO; ++k) info[k] = k < 5 ? all[ns + k] : 0.0;
  info[5] = sums[0];
  return S4P_ICP_OK;
}

// one generalized pass: the search, the 31 sums streamed from the slots
int32_t gicp_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double epsilon, double* out) {
  if (int32_t rc = launch_search(h, T, src, false)) return rc;
  GicpArgs A;
  A.T = T; A.g = h->g; A.src = src; A.snrm = h->snrm; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.slot = h->rslot;
  A.k = 1.0 - epsilon; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_gicp_sum, nb, A);
  ICP_LAUNCH(k_final_plane, 1, h->pslab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_GICP_NSUMS, out);
}

// one symmetric pass: the search, the 31 sums streamed from the slots
int32_t symm_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double* out) {
  if (int32_t rc = launch_search(h, T, src, false)) return rc;
  SymmArgs A;
  A.T = T; A.g = h->g; A.src = src; A.snrm = h->snrm; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.slot = h->rslot; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_symm_sum, nb, A);
  ICP_LAUNCH(k_final_plane, 1, h->pslab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_SYMM_NSUMS, out);
}

// one colour pass: the search, the 31 joint sums streamed from the slots
int32_t color_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double lambda, double* out) {
  if (int32_t rc = launch_search(h, T, src, false)) return rc;
  ColorArgs A;
  A.T = T; A.g = h->g; A.src = src; A.sint = h->sint; A.nrm = h->nrm; A.grad = h->grad; A.n = uint64_t(h->n_q); A.slot = h->rslot;
  A.wg = lambda; A.wc = 1.0 - lambda; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_color_sum, nb, A);
  ICP_LAUNCH(k_final_plane, 1, h->pslab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_COLOR_NSUMS, out);
}

// one information pass (include/s4p_icp_info.h): the search, the 11 sums streamed from the slots
int32_t info_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double* out) {
  if (int32_t rc = launch_search(h, T, src, false)) return rc;
  InfoArgs A;
  A.T = T; A.src = src; A.tgt = h->g.tgt; A.n = uint64_t(h->n_q); A.slot = h->rslot; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_info_sum, nb, A);
  ICP_LAUNCH(k_final_info, 1, h->pslab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_INFO_NSUMS, out);
}

// The information sums of the source as uploaded for T: readiness, prepare, one pass.
int32_t info_call(s4p_icp_ctx* h, const Tf& T, double* sums) {
  PassKind K;
  K.metric = kInfo;
  if (int32_t rc = ready_for(h, K)) return rc;
  if (int32_t rc = prepare(h, h->src, &K)) return rc;
  return info_pass(h, T, h->src, sums);
}

// The fused passes come last of the passes: template kernels are emitted in the order of their first launch in this file,
// and k_match<false> stays the last kernel these parts emit (the end of a kernel's code includes the padding up to the next;
// the batch kernels of s4p_icp_batch.inc come after it).

// the fused point pass: the 17 sums (and, if idx, the per-point answers)
int32_t pass(s4p_icp_ctx* h, const Tf& T, const float4* src, int32_t* idx_dev, float* d2_dev, double* out) {
  MatchArgs A;
  A.T = T; A.g = h->g; A.src = src; A.n = uint64_t(h->n_q); A.d2max = h->d2max; A.idx = idx_dev; A.d2 = d2_dev; A.slab = h->slab;
  const int nb = blocks_for(h->n_q);
  if (idx_dev) ICP_LAUNCH(k_match<true>, nb, A);
  else ICP_LAUNCH(k_match<false>, nb, A);
  ICP_LAUNCH(k_final, 1, h->slab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_NSUMS, out);
}

// the fused point-to-plane pass: the 31 sums
int32_t plane_pass(s4p_icp_ctx* h, const Tf& T, const float4* src, double* out) {
  PlaneArgs A;
  A.T = T; A.g = h->g; A.src = src; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.d2max = h->d2max; A.slab = h->pslab;
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_match_plane, nb, A);
  ICP_LAUNCH(k_final_plane, 1, h->pslab, nb, h->dsum);
  return finish_pass(h, h->dsum, h->hsum, S4P_ICP_PLANE_NSUMS, out);
}

// One pass of kind K over `src` for T, after prepare(h, src, &K).  The plain point / plane metrics run the fused k_match /
// k_match_plane; under rejection they run the split pass with every weight 1.
int32_t run_pass(s4p_icp_ctx* h, const PassKind& K, const Tf& T, const float4* src, PassOut& o) {
  int32_t rc;
  if (weighted(h, K)) {
    RobustCfg ones;
    ones.loss = kLossOnes;
    rc = robust_pass(h, T, src, K.plane(), K.robust ? K.cfg : ones, o.sums, o.info);
    o.n = K.robust ? o.info[4] : o.sums[0];
    return rc;
  }
  if (K.metric == kGicp) rc = gicp_pass(h, T, src, K.param, o.sums);
  else if (K.metric == kColor) rc = color_pass(h, T, src, K.param, o.sums);
  else if (K.metric == kSymm) rc = symm_pass(h, T, src, o.sums);
  else rc = K.plane() ? plane_pass(h, T, src, o.sums) : pass(h, T, src, nullptr, nullptr, o.sums);
  o.n = o.sums[0];
  return rc;
}

// a stage-level sums call: one pass over the source as uploaded, for a float T in the centred frame
int32_t sums_call(s4p_icp_ctx* h, const PassKind& K, const float* T16_centred, double* sums, double* info) {
  if (int32_t rc = prepare(h, h->src, &K)) return rc;
  PassOut o;
  if (int32_t rc = run_pass(h, K, centred_from_float16(T16_centred), h->src, o)) return rc;
  std::memcpy(sums, o.sums, K.nsums() * sizeof(double));
  if (info) std::memcpy(info, o.info, sizeof(o.info));
  return S4P_ICP_OK;
}

// refine's source: as uploaded, or (order_source) in the cell order of its T0-image, so that a wave's lanes read
// neighbouring cells
int32_t source_for(s4p_icp_ctx* h, const s4p_icp_params& P, const double* T, const float4** src) {
  *src = h->src;
  if (!P.order_source) return S4P_ICP_OK;
  Scratch S;
  const uint64_t un = uint64_t(h->n_q);
  uint32_t *keys, *vals, *keys2, *vals2;
  ICP_HIP(S.alloc((void**)&keys, un * 4)); ICP_HIP(S.alloc((void**)&vals, un * 4));
  ICP_HIP(S.alloc((void**)&keys2, un * 4)); ICP_HIP(S.alloc((void**)&vals2, un * 4));
  const int nb = blocks_for(h->n_q);
  ICP_LAUNCH(k_source_keys, nb, h->src, un, to_float(T), h->g, keys, vals);
  if (int32_t rc = sort_pairs(h, S, keys, keys2, vals, vals2, un, h->ncell)) return rc;
  ICP_LAUNCH(k_gather_source, nb, h->src, vals2, un, h->src_ord);
  ICP_HIP(hipStreamSynchronize(h->st));
  *src = h->src_ord;
  return S4P_ICP_OK;
}

// The refine loop of every metric.  K.robust unset: K.metric and K.param are the call's.  K.robust set: robust_metric and
// robust are the caller's, validated here behind the readiness check (as every robust entry point orders them), and `who`
// names the entry point in the messages.  rmse = sqrt(sum (w) d2 / sum (w)) with sum d2 at [1] (the 31 sums) or [16]; the
// count n is the pass's; a degenerate s4p_icp_solve_plane / s4p_icp_solve_symmetric stops the loop
// with T_k.
int32_t refine_loop(s4p_icp_ctx* h, const s4p_icp_params* params, PassKind K, int32_t robust_metric, const s4p_icp_robust* robust,
                    double* T16_inout, s4p_icp_result* result, double* info_out, const char* who) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_inout) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": null transform");
  s4p_icp_params P;
  s4p_icp_default_params(&P);
  if (params) P = *params;
  if (P.max_iterations < 0 || P.min_correspondences < 0 || !(P.rel_tol >= 0.0))
    return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": negative max_iterations / min_correspondences / rel_tol");
  if (int32_t rc = ready_for(h, K)) return rc;
  if (K.robust) if (int32_t rc = robust_cfg(h, robust_metric, robust, &K.cfg)) return rc;
  const bool plane = K.plane();
  s4p_icp_result R;
  std::memset(&R, 0, sizeof(R));
  double T[16], Tn[16], dT[16];
  PassOut o;
  const double* sums = o.sums;
  const int i_d2 = plane ? 1 : 16;
  to_centred(T16_inout, h->c, T);
  const float4* src = nullptr;
  if (int32_t rc = source_for(h, P, T, &src)) return rc;
  if (int32_t rc = prepare(h, src, &K)) return rc;      // what follows the source's order does so once, before the loop
  double prev = 0.0;
  R.status = S4P_ICP_MAX_ITERATIONS;
  for (int k = 0; k < P.max_iterations; ++k) {
    if (int32_t rc = run_pass(h, K, to_float(T), src, o)) return rc;
    const double n = o.n, sw = sums[0];
    const double rmse = sw > 0.0 ? std::sqrt(sums[i_d2] / sw) : 0.0;
    if (k < S4P_ICP_HISTORY) { R.history_rmse[k] = rmse; R.history_n[k] = int64_t(n); R.history_len = k + 1; }
    if (n < double(std::max(P.min_correspondences, 1)) || (K.robust && !plane && !(sw >= 1.0))) { R.status = S4P_ICP_TOO_FEW; break; }
    if (plane) {
      const int32_t rc = K.metric == kSymm ? s4p_icp_solve_symmetric(sums, dT) : s4p_icp_solve_plane(sums, dT);
      if (rc != S4P_ICP_OK) { R.status = S4P_ICP_DEGENERATE; break; }
    } else {
      s4p_icp_solve(sums, dT);
    }
    mat_mul4(dT, T, Tn);
    std::memcpy(T, Tn, sizeof(T));
    R.iterations = k + 1;
    if (k + 1 == P.max_iterations) { R.status = S4P_ICP_MAX_ITERATIONS; break; }
    if (k > 0 && std::fabs(rmse - prev) <= P.rel_tol * prev) { R.status = S4P_ICP_CONVERGED; break; }
    prev = rmse;
  }
  // final pass: the statistics of the returned transform
  if (int32_t rc = run_pass(h, K, to_float(T), src, o)) return rc;
  R.n_corr = int64_t(o.n);
  R.rmse = sums[0] > 0.0 ? std::sqrt(sums[i_d2] / sums[0]) : 0.0;
  R.fitness = double(R.n_corr) / double(h->n_q);
  from_centred(T, h->c, T16_inout);
  if (result) *result = R;
  if (K.robust && info_out) std::memcpy(info_out, o.info, sizeof(o.info));
  return S4P_ICP_OK;
}

}  // namespace
