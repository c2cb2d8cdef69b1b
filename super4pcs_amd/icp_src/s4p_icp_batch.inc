// s4p_icp_batch.inc -- batched multi-start ICP (include/s4p_icp_batch.h): the batch's buffers, one batched pass, the refine
// loop over an active list, the ranking, and the three entry points.

namespace {

constexpr int kBatchSumsCap = S4P_ICP_BATCH_MAX * kSumsCap;

// The buffers of a batch of B poses, made on the first batch call: the slab ([pose][kMaxBlocks] rows), the sums of a launch
// and their pinned copy, the poses on the device and their pinned staging.  Nothing here is touched by the single calls.
int32_t batch_buffers(s4p_icp_ctx* h, int B, bool plane) {
  const size_t need = size_t(B) * kMaxBlocks * (plane ? kPlanePitch : kPitch);
  if (h->bslab.n < need) ICP_HIP(h->bslab.ensure(need));
  ICP_HIP(h->bsum.ensure(kBatchSumsCap));
  ICP_HIP(h->bhsum.ensure(kBatchSumsCap));
  ICP_HIP(h->bposes.ensure(sizeof(BatchPoses)));
  ICP_HIP(h->bstage.ensure(sizeof(BatchPoses)));
  return S4P_ICP_OK;
}

// what every batch entry point refuses, in this order: the batch size, the metric, the state, the rejection
int32_t batch_ready(s4p_icp_ctx* h, int32_t metric, int32_t B, const char* who) {
  if (B < 1 || B > S4P_ICP_BATCH_MAX) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": B must be in 1..64");
  if (metric != S4P_ICP_METRIC_POINT && metric != S4P_ICP_METRIC_PLANE)
    return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": the metric must be point or plane");
  if (int32_t rc = metric == S4P_ICP_METRIC_PLANE ? plane_ready(h) : ready(h)) return rc;
  if (h->rej_on) return fail(h, S4P_ICP_ERR_STATE, std::string(who) + ": correspondence rejection is on and the batch has no split pass (set_rejection off first)");
  return S4P_ICP_OK;
}

// One batched pass over `src`: the staged poses (every T, the first `na` entries of the active list) go up in one copy,
// k_match_batch over (source workgroups, na), k_final_batch over na, and na rows of sums come back through finish_pass.
int32_t batch_pass(s4p_icp_ctx* h, bool plane, int na, const float4* src, double* out) {
  const int ns = plane ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS;
  const BatchPoses* poses = reinterpret_cast<const BatchPoses*>(h->bposes.p);
  ICP_HIP(hipMemcpyAsync(h->bposes, h->bstage, sizeof(BatchPoses), hipMemcpyHostToDevice, h->st));
  MatchBatchArgs A;
  A.poses = poses; A.g = h->g; A.src = src; A.nrm = h->nrm; A.n = uint64_t(h->n_q); A.d2max = h->d2max; A.slab = h->bslab;
  const int nb = blocks_for(h->n_q);
  if (plane) {
    ICP_LAUNCH(k_match_batch<true>, dim3(nb, na), A);
    ICP_LAUNCH(k_final_batch<true>, na, poses, h->bslab, nb, h->bsum);
  } else {
    ICP_LAUNCH(k_match_batch<false>, dim3(nb, na), A);
    ICP_LAUNCH(k_final_batch<false>, na, poses, h->bslab, nb, h->bsum);
  }
  return finish_pass(h, h->bsum, h->bhsum, na * ns, out);
}

// one pose of a batch on the host: refine_loop's locals
struct PoseState {
  double T[16];
  double prev = 0.0;
  s4p_icp_result R;
};

bool ranks_before(const s4p_icp_result& a, int ia, const s4p_icp_result& b, int ib) {
  if (a.n_corr != b.n_corr) return a.n_corr > b.n_corr;
  if (a.n_corr <= 0) return ia < ib;
  if (a.rmse < b.rmse) return true;
  if (b.rmse < a.rmse) return false;
  return ia < ib;
}

}  // namespace

extern "C" {

int32_t s4p_icp_rank_batch(const s4p_icp_result* results, int32_t B, int32_t* order) {
  if (!results || !order || B < 1 || B > S4P_ICP_BATCH_MAX) return S4P_ICP_ERR_BAD_ARG;
  for (int b = 0; b < B; ++b) {                    // insertion: at most 64 entries, and no demand on the comparison
    int at = b;
    while (at > 0 && ranks_before(results[b], b, results[order[at - 1]], order[at - 1])) { order[at] = order[at - 1]; --at; }
    order[at] = b;
  }
  return S4P_ICP_OK;
}

int32_t s4p_icp_sums_batch(s4p_icp_ctx* h, int32_t metric, int32_t B, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "sums_batch: null argument");
  if (int32_t rc = batch_ready(h, metric, B, "sums_batch")) return rc;
  const bool plane = metric == S4P_ICP_METRIC_PLANE;
  if (int32_t rc = batch_buffers(h, B, plane)) return rc;
  BatchPoses* st = reinterpret_cast<BatchPoses*>(h->bstage.p);
  for (int b = 0; b < B; ++b) { st->T[b] = centred_from_float16(T16_centred + 16 * b); st->active[b] = b; }
  return batch_pass(h, plane, B, h->src, sums);
}

// refine_loop's state machine per pose, every comparison as written there; the poses of one launch are at the same k.
int32_t s4p_icp_refine_batch(s4p_icp_ctx* h, const s4p_icp_batch_params* params, int32_t B, double* T16_inout,
                             s4p_icp_result* results, int32_t* order) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_inout || !results) return fail(h, S4P_ICP_ERR_BAD_ARG, "refine_batch: null transforms or results");
  s4p_icp_params P;
  s4p_icp_default_params(&P);
  int32_t metric = S4P_ICP_METRIC_POINT;
  if (params) { P = params->icp; metric = params->metric; }
  if (P.max_iterations < 0 || P.min_correspondences < 0 || !(P.rel_tol >= 0.0))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "refine_batch: negative max_iterations / min_correspondences / rel_tol");
  if (int32_t rc = batch_ready(h, metric, B, "refine_batch")) return rc;
  const bool plane = metric == S4P_ICP_METRIC_PLANE;
  const int ns = plane ? S4P_ICP_PLANE_NSUMS : S4P_ICP_NSUMS, i_d2 = plane ? 1 : 16;
  if (int32_t rc = batch_buffers(h, B, plane)) return rc;
  std::vector<PoseState> S(B);
  std::vector<double> all(size_t(B) * ns);
  std::vector<int> active(B);
  for (int b = 0; b < B; ++b) {
    std::memset(&S[b].R, 0, sizeof(s4p_icp_result));
    S[b].R.status = S4P_ICP_MAX_ITERATIONS;
    to_centred(T16_inout + 16 * b, h->c, S[b].T);
    active[b] = b;
  }
  const float4* src = nullptr;
  if (int32_t rc = source_for(h, P, S[0].T, &src)) return rc;          // ordered once, by the image under start 0
  BatchPoses* st = reinterpret_cast<BatchPoses*>(h->bstage.p);
  int na = B;
  for (int k = 0; k < P.max_iterations && na > 0; ++k) {
    for (int a = 0; a < na; ++a) { st->T[active[a]] = to_float(S[active[a]].T); st->active[a] = active[a]; }
    if (int32_t rc = batch_pass(h, plane, na, src, all.data())) return rc;
    int kept = 0;
    for (int a = 0; a < na; ++a) {
      PoseState& s = S[active[a]];
      s4p_icp_result& R = s.R;
      const double* sums = all.data() + size_t(a) * ns;
      double Tn[16], dT[16];
      const double n = sums[0], sw = sums[0];
      const double rmse = sw > 0.0 ? std::sqrt(sums[i_d2] / sw) : 0.0;
      if (k < S4P_ICP_HISTORY) { R.history_rmse[k] = rmse; R.history_n[k] = int64_t(n); R.history_len = k + 1; }
      if (n < double(std::max(P.min_correspondences, 1))) { R.status = S4P_ICP_TOO_FEW; continue; }
      if (plane) {
        if (s4p_icp_solve_plane(sums, dT) != S4P_ICP_OK) { R.status = S4P_ICP_DEGENERATE; continue; }
      } else {
        s4p_icp_solve(sums, dT);
      }
      mat_mul4(dT, s.T, Tn);
      std::memcpy(s.T, Tn, sizeof(s.T));
      R.iterations = k + 1;
      if (k + 1 == P.max_iterations) { R.status = S4P_ICP_MAX_ITERATIONS; continue; }
      if (k > 0 && std::fabs(rmse - s.prev) <= P.rel_tol * s.prev) { R.status = S4P_ICP_CONVERGED; continue; }
      s.prev = rmse;
      active[kept++] = active[a];                  // still iterating: compacted into the next launch
    }
    na = kept;
  }
  // final pass: the statistics of every returned transform, one launch over all B
  for (int b = 0; b < B; ++b) { st->T[b] = to_float(S[b].T); st->active[b] = b; }
  if (int32_t rc = batch_pass(h, plane, B, src, all.data())) return rc;
  for (int b = 0; b < B; ++b) {
    const double* sums = all.data() + size_t(b) * ns;
    s4p_icp_result& R = S[b].R;
    R.n_corr = int64_t(sums[0]);
    R.rmse = sums[0] > 0.0 ? std::sqrt(sums[i_d2] / sums[0]) : 0.0;
    R.fitness = double(R.n_corr) / double(h->n_q);
    from_centred(S[b].T, h->c, T16_inout + 16 * b);
    results[b] = R;
  }
  if (order) return s4p_icp_rank_batch(results, B, order);
  return S4P_ICP_OK;
}

}  // extern "C"
