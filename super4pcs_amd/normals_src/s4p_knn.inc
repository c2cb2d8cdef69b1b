// s4p_knn.inc -- neighbour lists and outlier removal of libsuper4pcs_normals.so (include/s4p_knn.h, DESIGN.md section
// "Neighbour queries and outlier removal").  Included by s4p_normals.hip after its context and helpers: the functions work
// on an s4p_normals_ctx after set_cloud, on its cloud, grid and stream.
//
// Device path:
//   lists        k_knn_search<K, kLists>: knn_walk of s4p_normals.hip, the walk k_knn_normals runs (rings, box pruning, min /
//                max insertion into K 64-bit keys in registers), then the k keys unpacked into idx / d2 / cnt rows in the
//                caller's order.  knn_search_at orders its queries with QueryStage of s4p_normals.hip, as estimate_at does.
//   statistical  k_knn_search<K, kMean> (8 bytes per point: the mean neighbour distance, no lists) -> k_sor_rows<0> +
//                k_sor_reduce (mu) -> k_sor_rows<1> + k_sor_reduce (sigma, t) -> k_sor_mask (keep, integer count).
//   radius       k_knn_search<K, kFilled>: one byte per point, "all k slots filled".
// Every double sum has a fixed order (a lane's grid-stride terms in order, an LDS tree per workgroup, the rows of the
// workgroups by one workgroup in the same way); the only atomic is the integer count of kept points.
// Work memory comes from the context's arena (Arena and arena_layout of s4p_normals.hip): every entry point states its
// pieces once, and a call allocates when it needs more than any call before.

namespace s4p_nrm {

enum SearchMode { kLists = 0, kMean = 1, kFilled = 2 };

struct SearchArgs {
  GridDev g;
  const float4* qs;           // queries in cell order, w = output slot (bits); in the self form the slot is the point's index
  uint64_t m;
  int32_t k;
  float r2lim;                // fl(r*r), or +inf (unbounded)
  uint32_t self_mask;         // ~0u: the candidate whose index is the query's slot is left out; 0: nothing is
  int32_t* idx;               // kLists: m * k, -1 padded
  float* d2;                  // kLists: m * k, +inf padded
  int32_t* cnt;               // kLists: m, or null
  double* mean;               // kMean: m
  uint8_t* filled;            // kFilled: m
};

// One lane per query, as k_knn_normals; MODE picks what is kept of the list.
template <int K, int MODE>
__global__ __launch_bounds__(kBlock) void k_knn_search(SearchArgs A) {
  for (uint64_t j = blockIdx.x * (uint64_t)kBlock + threadIdx.x; j < A.m; j += (uint64_t)gridDim.x * kBlock) {
    const float4 q = A.qs[j];
    const uint32_t slot = __float_as_uint(q.w);
    uint64_t L[K];
#pragma unroll
    for (int t = 0; t < K; ++t) L[t] = t < K - A.k ? 0ull : ~0ull;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) knn_walk<K>(A.g, q, A.r2lim, slot | ~A.self_mask, L);
    if (MODE == kLists) {
      const uint64_t base = uint64_t(slot) * uint64_t(A.k);
      int32_t cnt = 0;
#pragma unroll
      for (int t = 0; t < K; ++t) {
        if (L[t] == 0ull) continue;                      // the K - k sentinels in front: no candidate's key is 0
        const uint64_t o = base + uint64_t(t - (K - A.k));
        A.idx[o] = int32_t(uint32_t(L[t]));              // ~0 -> -1
        A.d2[o] = key_d2(L[t]);                          // ~0 -> +inf
        cnt += L[t] != ~0ull;
      }
      if (A.cnt) A.cnt[slot] = cnt;
    } else if (MODE == kMean) {
      double s = 0.0;
      int32_t cnt = 0;
#pragma unroll
      for (int t = 0; t < K; ++t) {
        if (L[t] == 0ull || L[t] == ~0ull) continue;
        s += sqrt(double(key_d2(L[t])));
        ++cnt;
      }
      A.mean[slot] = cnt > 0 ? s / double(cnt) : 0.0;
    } else {
      A.filled[slot] = L[K - 1] != ~0ull ? 1 : 0;
    }
  }
}

struct SorDev {
  double mu, sigma, t;
  unsigned long long kept;
};

// a workgroup's sum in a fixed order: sh[] holds one term per lane
__device__ inline double block_sum(double* sh, double v) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < unsigned(w)) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// rows[b] = the workgroup's sum of v[i] (SQ = 0) or of (v[i] - mu)^2 (SQ = 1)
template <int SQ>
__global__ __launch_bounds__(kBlock) void k_sor_rows(const double* v, uint64_t n, const SorDev* st, double* rows) {
  __shared__ double sh[kBlock];
  const double mu = SQ ? st->mu : 0.0;
  double s = 0.0;
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const double d = v[i] - mu;
    s += SQ ? d * d : v[i];
  }
  const double r = block_sum(sh, s);
  if (threadIdx.x == 0) rows[blockIdx.x] = r;
}

// one workgroup: the rows' sum in a fixed order, then mu (stage 0) or sigma, t and the zeroed count (stage 1)
__global__ __launch_bounds__(kBlock) void k_sor_reduce(const double* rows, int nrows, uint64_t n, double ratio, int stage, SorDev* st) {
  __shared__ double sh[kBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < nrows; i += kBlock) s += rows[i];
  const double r = block_sum(sh, s);
  if (threadIdx.x != 0) return;
  if (stage == 0) {
    st->mu = r / double(n);
  } else {
    const double var = n > 1 ? r / double(n - 1) : 0.0;
    const double sigma = sqrt(var);
    st->sigma = sigma;
    st->t = st->mu + ratio * sigma;
    st->kept = 0ull;
  }
}

__global__ __launch_bounds__(kBlock) void k_sor_mask(const double* v, uint64_t n, SorDev* st, uint8_t* keep) {
  const double t = st->t;
  unsigned long long mine = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const bool k = v[i] <= t;
    keep[i] = k ? 1 : 0;
    mine += k;
  }
  __shared__ unsigned long long sh[kBlock];
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < unsigned(w)) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicAdd(&st->kept, sh[0]);       // an integer count: any order gives the same value
}

}  // namespace s4p_nrm

namespace {

int32_t knn_check(s4p_normals_ctx* h, const char* what, int32_t k) {
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, std::string(what) + ": set_cloud first");
  if (k < S4P_KNN_MIN_K || k > S4P_KNN_MAX_K) return fail(h, S4P_NORMALS_ERR_BAD_ARG, std::string(what) + ": k must be in [1, 32]");
  return S4P_NORMALS_OK;
}

template <int MODE>
int32_t launch_search(s4p_normals_ctx* h, SearchArgs& A, float radius) {
  if (A.m == 0) return S4P_NORMALS_OK;
  A.g = h->g;
  A.r2lim = radius > 0.f ? radius * radius : INFINITY;
  const int nb = blocks_for(int64_t(A.m));
  if (A.k <= 8) hipLaunchKernelGGL((k_knn_search<8, MODE>), dim3(nb), dim3(kBlock), 0, h->st, A);
  else if (A.k <= 16) hipLaunchKernelGGL((k_knn_search<16, MODE>), dim3(nb), dim3(kBlock), 0, h->st, A);
  else hipLaunchKernelGGL((k_knn_search<32, MODE>), dim3(nb), dim3(kBlock), 0, h->st, A);
  NRM_HIP(hipGetLastError());
  return S4P_NORMALS_OK;
}

// where a lists call writes: the caller's arrays (device form), or arena copies that are brought back (host form)
struct ListsDev {
  int32_t* idx;
  float* d2;
  int32_t* cnt;
  void take(Arena& ar, uint64_t m, int32_t k, bool with_cnt) {
    idx = ar.take<int32_t>(size_t(m) * size_t(k));
    d2 = ar.take<float>(size_t(m) * size_t(k));
    cnt = with_cnt ? ar.take<int32_t>(m) : nullptr;
  }
};

// lists of m queries (cell order, device) into D, and from there into idx / d2 / cnt in the host form
int32_t lists_impl(s4p_normals_ctx* h, const ListsDev& D, const float4* qs, uint64_t m, int32_t k, float radius, bool exclude_self,
                   int32_t* idx, float* d2, int32_t* cnt, bool device) {
  SearchArgs A{};
  A.qs = qs; A.m = m; A.k = k; A.self_mask = exclude_self ? ~0u : 0u;
  A.idx = D.idx; A.d2 = D.d2; A.cnt = D.cnt;
  if (int32_t rc = launch_search<kLists>(h, A, radius)) return rc;
  if (!device) {
    const size_t mk = size_t(m) * size_t(k);
    NRM_HIP(hipMemcpyAsync(idx, D.idx, mk * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    NRM_HIP(hipMemcpyAsync(d2, D.d2, mk * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (cnt) NRM_HIP(hipMemcpyAsync(cnt, D.cnt, m * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

int32_t search_impl(s4p_normals_ctx* h, int32_t k, float radius, int32_t exclude_self, int32_t* idx, float* d2, int32_t* cnt,
                    bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = knn_check(h, "knn_search", k)) return rc;
  if (!std::isfinite(radius)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search: radius must be finite (<= 0: unbounded)");
  if (exclude_self != 0 && exclude_self != 1) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search: exclude_self must be 0 or 1");
  if (!idx || !d2) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search: null output");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  ListsDev D{idx, d2, cnt};
  if (int32_t rc = arena_layout(h, "knn_search", [&](Arena& ar) { if (!device) D.take(ar, un, k, cnt != nullptr); })) return rc;
  return lists_impl(h, D, h->pts, un, k, radius, exclude_self == 1, idx, d2, cnt, device);
}

int32_t search_at_impl(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k, float radius,
                       int32_t* idx, float* d2, int32_t* cnt, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = knn_check(h, "knn_search_at", k)) return rc;
  if (!std::isfinite(radius)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search_at: radius must be finite (<= 0: unbounded)");
  if (m < 0 || m > kMaxPoints) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search_at: m must be in [0, 2^31 - 2]");
  if (m == 0) return S4P_NORMALS_OK;
  if (!qx || !qy || !qz || !idx || !d2) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "knn_search_at: null argument");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t um = uint64_t(m);
  QueryStage Q;
  if (int32_t rc = Q.plan(h, um)) return rc;
  ListsDev D{idx, d2, cnt};
  if (int32_t rc = arena_layout(h, "knn_search_at", [&](Arena& ar) {
        Q.take(ar);
        if (!device) D.take(ar, um, k, cnt != nullptr);
      })) return rc;
  if (int32_t rc = Q.run(h, qx, qy, qz, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) return rc;
  return lists_impl(h, D, Q.qs, um, k, radius, false, idx, d2, cnt, device);
}

int32_t statistical_impl(s4p_normals_ctx* h, int32_t k, double std_ratio, double* mean_dist, uint8_t* keep, s4p_outliers_stats* stats,
                         bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = knn_check(h, "outliers_statistical", k)) return rc;
  if (!std::isfinite(std_ratio) || std_ratio < 0.0)
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "outliers_statistical: std_ratio must be finite and >= 0");
  if (!keep) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "outliers_statistical: null keep");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  const int nb = blocks_for(h->n);
  const bool own_mean = !device || !mean_dist;
  double *md = mean_dist, *rows = nullptr;
  uint8_t* dkeep = keep;
  SorDev* st = nullptr;
  if (int32_t rc = arena_layout(h, "outliers_statistical", [&](Arena& ar) {
        if (own_mean) md = ar.take<double>(un);
        if (!device) dkeep = ar.take<uint8_t>(un);
        rows = ar.take<double>(size_t(nb));
        st = ar.take<SorDev>(1);
      })) return rc;
  SearchArgs A{};
  A.qs = h->pts; A.m = un; A.k = k; A.self_mask = ~0u; A.mean = md;
  if (int32_t rc = launch_search<kMean>(h, A, -1.f)) return rc;
  for (int stage = 0; stage < 2; ++stage) {
    if (stage == 0) hipLaunchKernelGGL(k_sor_rows<0>, dim3(nb), dim3(kBlock), 0, h->st, (const double*)md, un, (const SorDev*)st, rows);
    else hipLaunchKernelGGL(k_sor_rows<1>, dim3(nb), dim3(kBlock), 0, h->st, (const double*)md, un, (const SorDev*)st, rows);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sor_reduce, dim3(1), dim3(kBlock), 0, h->st, (const double*)rows, nb, un, std_ratio, stage, st);
    NRM_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sor_mask, dim3(nb), dim3(kBlock), 0, h->st, (const double*)md, un, st, dkeep);
  NRM_HIP(hipGetLastError());
  SorDev hs{};
  NRM_HIP(hipMemcpyAsync(&hs, st, sizeof(SorDev), hipMemcpyDeviceToHost, h->st));
  if (!device) {
    NRM_HIP(hipMemcpyAsync(keep, dkeep, un, hipMemcpyDeviceToHost, h->st));
    if (mean_dist) NRM_HIP(hipMemcpyAsync(mean_dist, md, un * sizeof(double), hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  if (stats) {
    stats->n = h->n; stats->mean = hs.mu; stats->stddev = hs.sigma; stats->threshold = hs.t; stats->kept = int64_t(hs.kept);
  }
  return S4P_NORMALS_OK;
}

int32_t radius_impl(s4p_normals_ctx* h, float radius, int32_t min_neighbours, uint8_t* keep, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, "outliers_radius: set_cloud first");
  if (min_neighbours < S4P_KNN_MIN_K || min_neighbours > S4P_KNN_MAX_K)
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "outliers_radius: min_neighbours must be in [1, 32]");
  if (!std::isfinite(radius) || !(radius > 0.f)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "outliers_radius: radius must be finite and > 0");
  if (!keep) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "outliers_radius: null keep");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  uint8_t* dkeep = keep;
  if (int32_t rc = arena_layout(h, "outliers_radius", [&](Arena& ar) { if (!device) dkeep = ar.take<uint8_t>(un); })) return rc;
  SearchArgs A{};
  A.qs = h->pts; A.m = un; A.k = min_neighbours; A.self_mask = ~0u; A.filled = dkeep;
  if (int32_t rc = launch_search<kFilled>(h, A, radius)) return rc;
  if (!device) NRM_HIP(hipMemcpyAsync(keep, dkeep, un, hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_knn_search(s4p_normals_ctx* h, int32_t k, float radius, int32_t exclude_self, int32_t* idx, float* d2, int32_t* cnt) {
  return search_impl(h, k, radius, exclude_self, idx, d2, cnt, false);
}
int32_t s4p_knn_search_device(s4p_normals_ctx* h, int32_t k, float radius, int32_t exclude_self, int32_t* idx, float* d2,
                              int32_t* cnt) {
  return search_impl(h, k, radius, exclude_self, idx, d2, cnt, true);
}

int32_t s4p_knn_search_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                          float radius, int32_t* idx, float* d2, int32_t* cnt) {
  return search_at_impl(h, qx, qy, qz, m, k, radius, idx, d2, cnt, false);
}
int32_t s4p_knn_search_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                 float radius, int32_t* idx, float* d2, int32_t* cnt) {
  return search_at_impl(h, qx, qy, qz, m, k, radius, idx, d2, cnt, true);
}

int32_t s4p_outliers_statistical(s4p_normals_ctx* h, int32_t k, double std_ratio, double* mean_dist, uint8_t* keep,
                                 s4p_outliers_stats* stats) {
  return statistical_impl(h, k, std_ratio, mean_dist, keep, stats, false);
}
int32_t s4p_outliers_statistical_device(s4p_normals_ctx* h, int32_t k, double std_ratio, double* mean_dist, uint8_t* keep,
                                        s4p_outliers_stats* stats) {
  return statistical_impl(h, k, std_ratio, mean_dist, keep, stats, true);
}

int32_t s4p_outliers_radius(s4p_normals_ctx* h, float radius, int32_t min_neighbours, uint8_t* keep) {
  return radius_impl(h, radius, min_neighbours, keep, false);
}
int32_t s4p_outliers_radius_device(s4p_normals_ctx* h, float radius, int32_t min_neighbours, uint8_t* keep) {
  return radius_impl(h, radius, min_neighbours, keep, true);
}

}  // extern "C"
