// s4p_icp_ctx.inc -- the context and what builds its state: owned buffers, the error macro, call scratch, the radix sort, the
// grid plan and build, set_target / set_source, readiness.

// Memory the context owns: move-only, released with its owner.  ensure(count) reallocates only when the count changes, and
// reports the hipError_t so that ICP_HIP keeps mapping an out-of-memory.  PINNED: host memory for the read-backs.  Hidden: the
// library exports nothing of it.
template <typename T, bool PINNED = false>
struct __attribute__((visibility("hidden"))) Buf {
  T* p = nullptr;
  size_t n = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~Buf() { release(); }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr; n = 0;
  }
  hipError_t ensure(size_t count) {
    if (p && n == count) return hipSuccess;
    release();
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
  operator T*() const { return p; }
};
template <typename T> using Pinned = Buf<T, true>;

struct s4p_icp_ctx {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev = nullptr;
  std::string err;
  bool has_target = false, has_source = false, src_dirty = true;
  float c[3] = {0.f, 0.f, 0.f};
  float d = 0.f, d2max = 0.f;
  GridDev g{};
  uint64_t ncell = 0;
  int64_t n_p = 0, n_q = 0;
  Buf<float4> tgt;
  Buf<uint32_t> start;
  Buf<float> qraw[3];
  Buf<float4> src, src_ord;
  Buf<double> slab;                  // blocks_for(n_q) rows of kPitch
  Buf<double> dsum;                  // the 17 point or the 31 plane sums
  Pinned<double> hsum;
  Buf<float4> nrm;                   // target normals, cell order (point-to-plane)
  bool has_normals = false;
  // the split passes (robust, generalized, coloured, rejection), allocated on first use
  Buf<uint32_t> rslot, rkey;         // k_search's slot and key per visited lane
  Buf<double> pslab;                 // plane slab: kMaxBlocks rows of kPlanePitch (point-to-plane too)
  // robust ICP (include/s4p_icp_robust.h)
  Buf<uint32_t> rhist;               // kDigits x kBins
  Buf<SelState> rst;
  Buf<double> rsum;                  // sums + info
  Pinned<double> rhsum;
  // generalized ICP (include/s4p_icp_gicp.h)
  Buf<float> sn[3];                  // source normals as stored, uploaded order
  Buf<float4> snrm;                  // the same in the order of the pass's source
  bool has_src_normals = false;
  // coloured ICP (include/s4p_icp_color.h)
  Buf<float> tint;                   // target intensities, cell order
  Buf<float4> grad;                  // target gradients and intensities, cell order
  bool has_tint = false, has_grad = false;
  Buf<float> si;                     // source intensities, uploaded order
  Buf<float> sint;                   // the same in the order of the pass's source
  bool has_sint = false;
  // correspondence rejection (include/s4p_icp_reject.h)
  s4p_icp_reject rej{};              // validated; everything off by default
  bool rej_on = false;
  GridDev gs{};                      // the source grid (reverse search), built when a pass first needs it
  Buf<float4> sgrid;                 // Q' in its cell order, w = the uploaded source index
  Buf<uint32_t> sstart;
  bool sgrid_valid = false;
  Buf<unsigned long long> rcnt;      // the four counters of a pass
  Pinned<unsigned long long> rhcnt;
  bool rej_pending = false;          // a k_reject of this pass is in flight: its counters follow the sums to the host
  int64_t rej_counts[4] = {0, 0, 0, 0};
  // batched multi-start ICP (include/s4p_icp_batch.h), allocated on the first batch call (s4p_icp_batch.inc)
  Buf<double> bslab;                 // [pose][kMaxBlocks] slab rows
  Buf<double> bsum;                  // one row of sums per pose of a launch
  Pinned<double> bhsum;
  Buf<unsigned char> bposes;         // a BatchPoses: every transform and the active list
  Pinned<unsigned char> bstage;      // its staging, one upload per launch

  // runs before the buffers release themselves; hidden: the library exports its C ABI only
  __attribute__((visibility("hidden"))) ~s4p_icp_ctx() { (void)hipSetDevice(device); }
};

namespace {

std::string g_create_error;
constexpr int kSumsCap = S4P_ICP_PLANE_NSUMS;       // dsum / hsum hold the 17 point or the 31 plane sums
static_assert(S4P_ICP_PLANE_NSUMS >= S4P_ICP_NSUMS && S4P_ICP_PLANE_NSUMS >= S4P_ICP_INFO_NSUMS, "sum buffers");

int32_t fail(s4p_icp_ctx* h, int32_t code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define ICP_HIP(expr)                                                                                             \
  do {                                                                                                            \
    const hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) return fail(h, e_ == hipErrorOutOfMemory ? S4P_ICP_ERR_OOM : S4P_ICP_ERR_HIP,          \
                                      std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while (0)

// a launch of kBlock-thread workgroups on the context's stream, and its error
#define ICP_LAUNCH(kernel, blocks, ...)                                              \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, h->st, __VA_ARGS__);   \
    ICP_HIP(hipGetLastError());                                                      \
  } while (0)

// device temporaries of one call, released on every exit
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*p); else *p = nullptr;
    return e;
  }
};

int end_bit(uint64_t max_key) {
  int b = 1;
  while (b < 32 && (max_key >> b) != 0) ++b;
  return b;
}

// (keys, vals) sorted by key into (keys_out, vals_out): radix sort (stable, deterministic)
int32_t sort_pairs(s4p_icp_ctx* h, Scratch& S, const uint32_t* keys, uint32_t* keys_out, const uint32_t* vals, uint32_t* vals_out,
                   uint64_t n, uint64_t max_key) {
  size_t bytes = 0;
  ICP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, keys_out, vals, vals_out, int(n), 0, end_bit(max_key), h->st));
  void* tmp = nullptr;
  ICP_HIP(S.alloc(&tmp, bytes));
  ICP_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, keys_out, vals, vals_out, int(n), 0, end_bit(max_key), h->st));
  return S4P_ICP_OK;
}

// coordinate sums and float bounds of a cloud on the device: k_stats' per-block partials, combined on the host in row order
int32_t cloud_stats(s4p_icp_ctx* h, Scratch& S, float* const p[3], int64_t n, double sum[3], float lo[3], float hi[3]) {
  const int nb = blocks_for(n);
  double* rows = nullptr;
  ICP_HIP(S.alloc((void**)&rows, size_t(nb) * kStatsPitch * sizeof(double)));
  ICP_LAUNCH(k_stats, nb, p[0], p[1], p[2], uint64_t(n), rows);
  std::vector<double> hr(size_t(nb) * kStatsPitch);
  ICP_HIP(hipMemcpyAsync(hr.data(), rows, hr.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  for (int a = 0; a < 3; ++a) { sum[a] = 0.0; lo[a] = float(hr[3 + a]); hi[a] = float(hr[6 + a]); }
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      sum[a] += hr[size_t(b) * kStatsPitch + a];
      lo[a] = std::min(lo[a], float(hr[size_t(b) * kStatsPitch + 3 + a]));
      hi[a] = std::max(hi[a], float(hr[size_t(b) * kStatsPitch + 6 + a]));
    }
  return S4P_ICP_OK;
}

// grid plan over the centred bounds [plo, phi] of n points: cell edge 1.02 d, enlarged x 1.25 until the dense grid fits the
// cell cap (cf. LcpGridHost::plan)
int32_t plan_grid(s4p_icp_ctx* h, const float plo[3], const float phi[3], uint64_t un, float d, GridDev* g, uint64_t* ncell,
                  const char* who) {
  const uint64_t cap = std::min<uint64_t>(kMaxCells, std::max<uint64_t>(1ull << 20, 2 * un));
  double hh = double(d) * double(kCellFactor);
  int dims[3];
  for (int guard = 0;; ++guard) {
    const double inv = 1.0 / hh;
    bool ok = true;
    uint64_t nc = 1;
    for (int a = 0; a < 3; ++a) {
      const double cc = cell_coord(phi[a], double(plo[a]), inv);
      if (!(cc < 1.0e9)) { ok = false; break; }
      dims[a] = int(cc) + 1;
      nc *= uint64_t(dims[a]);
      if (nc > cap) { ok = false; break; }
    }
    if (ok) { g->h = hh; g->inv_h = inv; *ncell = nc; break; }
    if (guard > 400) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": no grid fits the cloud's extent");
    hh *= 1.25;
  }
  g->ox = plo[0]; g->oy = plo[1]; g->oz = plo[2];
  g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
  return S4P_ICP_OK;
}

// the cell-ordered cloud fl(p - c) (w = the index) into pts and the start of every cell of the planned grid g into start;
// both are entered into g
int32_t build_grid(s4p_icp_ctx* h, Scratch& S, float* const p[3], uint64_t un, const float c[3], GridDev* g, uint64_t ncell,
                   Buf<float4>& pts, Buf<uint32_t>& start) {
  const int nb = blocks_for(int64_t(un));
  uint32_t *keys, *vals, *keys2, *vals2;
  ICP_HIP(S.alloc((void**)&keys, un * 4)); ICP_HIP(S.alloc((void**)&vals, un * 4));
  ICP_HIP(S.alloc((void**)&keys2, un * 4)); ICP_HIP(S.alloc((void**)&vals2, un * 4));
  ICP_LAUNCH(k_cell_keys, nb, p[0], p[1], p[2], un, c[0], c[1], c[2], *g, keys, vals);
  if (int32_t rc = sort_pairs(h, S, keys, keys2, vals, vals2, un, ncell - 1)) return rc;
  ICP_HIP(start.ensure(ncell + 1));
  ICP_HIP(pts.ensure(un));
  ICP_LAUNCH(k_cell_starts, blocks_for(int64_t(ncell) + 1), keys2, un, ncell, start);
  ICP_LAUNCH(k_gather_target, nb, p[0], p[1], p[2], un, c[0], c[1], c[2], vals2, pts);
  ICP_HIP(hipStreamSynchronize(h->st));          // the scratch is freed on return
  g->tgt = pts;
  g->start = start;
  return S4P_ICP_OK;
}

void drop_source_grid(s4p_icp_ctx* h) {
  h->sgrid_valid = false;
  h->sgrid.release(); h->sstart.release();
}

int32_t set_target_impl(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float d, hipMemcpyKind kind) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!x || !y || !z || n < 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: empty or null cloud");
  if (n >= int64_t(0x7FFFFFFF)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: more than 2^31 - 1 points");
  if (!(d > 0.f) || !std::isfinite(d)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: max_distance must be finite and > 0");
  ICP_HIP(hipSetDevice(h->device));
  h->has_target = h->has_normals = h->has_tint = h->has_grad = false;
  // the old target goes before this call's scratch comes, so that the peak stays one target
  h->nrm.release(); h->tint.release(); h->grad.release(); h->tgt.release(); h->start.release();
  drop_source_grid(h);                            // the frame and d are the target's
  Scratch S;
  const uint64_t un = uint64_t(n);
  float* p[3];
  const float* in[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&p[a], un * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(p[a], in[a], un * sizeof(float), kind, h->st));
  }
  // frame and bounds
  double sum[3];
  float lo[3], hi[3];
  if (int32_t rc = cloud_stats(h, S, p, n, sum, lo, hi)) return rc;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target: non-finite coordinates");
    h->c[a] = float(sum[a] / double(n));
  }
  // bounds of P' = fl(P - c): rounding is monotone, so they are fl(lo - c), fl(hi - c)
  float plo[3], phi[3];
  for (int a = 0; a < 3; ++a) { plo[a] = lo[a] - h->c[a]; phi[a] = hi[a] - h->c[a]; }
  if (int32_t rc = plan_grid(h, plo, phi, un, d, &h->g, &h->ncell, "set_target")) return rc;
  h->d = d;
  h->d2max = d * d;
  if (int32_t rc = build_grid(h, S, p, un, h->c, &h->g, h->ncell, h->tgt, h->start)) return rc;
  h->n_p = n;
  h->has_target = true;
  h->src_dirty = true;                          // Q' depends on c
  return S4P_ICP_OK;
}

// The source grid of the reverse search (include/s4p_icp_reject.h): set_target's plan and build over Q' = fl(Q - c) in the
// uploaded order, from the coordinates as uploaded.  Built once; set_source and set_target drop it.
int32_t source_grid_ready(s4p_icp_ctx* h) {
  if (h->sgrid_valid) return S4P_ICP_OK;
  drop_source_grid(h);
  Scratch S;
  double sum[3];
  float lo[3], hi[3];
  float* const q[3] = {h->qraw[0], h->qraw[1], h->qraw[2]};
  if (int32_t rc = cloud_stats(h, S, q, h->n_q, sum, lo, hi)) return rc;
  float plo[3], phi[3];
  for (int a = 0; a < 3; ++a) {
    plo[a] = lo[a] - h->c[a]; phi[a] = hi[a] - h->c[a];
    if (!std::isfinite(plo[a]) || !std::isfinite(phi[a])) return fail(h, S4P_ICP_ERR_BAD_ARG, "rejection: non-finite source coordinates");
  }
  uint64_t ncell = 0;
  if (int32_t rc = plan_grid(h, plo, phi, uint64_t(h->n_q), h->d, &h->gs, &ncell, "rejection")) return rc;
  if (int32_t rc = build_grid(h, S, q, uint64_t(h->n_q), h->c, &h->gs, ncell, h->sgrid, h->sstart)) return rc;
  h->sgrid_valid = true;
  return S4P_ICP_OK;
}

int32_t set_source_impl(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, hipMemcpyKind kind) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!x || !y || !z || n < 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source: empty or null cloud");
  if (n >= int64_t(0x7FFFFFFF)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source: more than 2^31 - 1 points");
  ICP_HIP(hipSetDevice(h->device));
  h->has_source = h->has_src_normals = h->has_sint = false;
  drop_source_grid(h);
  for (int a = 0; a < 3; ++a) ICP_HIP(h->qraw[a].ensure(size_t(n)));
  ICP_HIP(h->src.ensure(size_t(n)));
  ICP_HIP(h->src_ord.ensure(size_t(n)));
  ICP_HIP(h->slab.ensure(size_t(blocks_for(n)) * kPitch));
  h->n_q = n;
  const float* in[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(h->qraw[a], in[a], size_t(n) * sizeof(float), kind, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_source = true;
  h->src_dirty = true;
  return S4P_ICP_OK;
}

int32_t ready(s4p_icp_ctx* h) {
  if (!h->has_target || !h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_target and set_source first");
  ICP_HIP(hipSetDevice(h->device));
  if (h->src_dirty) {
    ICP_LAUNCH(k_center_source, blocks_for(h->n_q), h->qraw[0], h->qraw[1], h->qraw[2], uint64_t(h->n_q), h->c[0], h->c[1], h->c[2], h->src);
    h->src_dirty = false;
  }
  return S4P_ICP_OK;
}

int32_t plane_ready(s4p_icp_ctx* h) {
  if (int32_t rc = ready(h)) return rc;
  if (!h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "target normals first (set_target_normals or estimate_normals)");
  return S4P_ICP_OK;
}

int32_t gicp_ready(s4p_icp_ctx* h, double epsilon) {
  if (!(epsilon >= S4P_ICP_GICP_EPSILON_MIN && epsilon <= S4P_ICP_GICP_EPSILON_MAX))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "gicp: epsilon must be in [1e-6, 1]");
  if (int32_t rc = plane_ready(h)) return rc;
  if (!h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "source normals first (set_source_normals)");
  return S4P_ICP_OK;
}

int32_t symm_ready(s4p_icp_ctx* h) {
  if (int32_t rc = plane_ready(h)) return rc;
  if (!h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "source normals first (set_source_normals)");
  return S4P_ICP_OK;
}

int32_t color_ready(s4p_icp_ctx* h, double lambda) {
  if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "color: lambda must be in [0, 1]");
  if (int32_t rc = plane_ready(h)) return rc;
  if (!h->has_tint) return fail(h, S4P_ICP_ERR_STATE, "target intensity first (set_target_intensity)");
  if (!h->has_grad) return fail(h, S4P_ICP_ERR_STATE, "colour gradients first (estimate_color_gradients)");
  if (!h->has_sint) return fail(h, S4P_ICP_ERR_STATE, "source intensity first (set_source_intensity)");
  return S4P_ICP_OK;
}

}  // namespace
