// s4p_icp_abi.inc -- the extern "C" entry points (include/s4p_icp*.h) and the setters' and read-backs' shared steps.  Every
// entry point keeps its own argument checks and messages, in its own order.

namespace {

// A device array on the host, for the *_device setters: they normalise or check on the host on purpose, so that the host
// and the device entry point store the same bits.
int32_t stage_to_host(s4p_icp_ctx* h, const float* dev, size_t n, std::vector<float>& v) {
  v.resize(n);
  ICP_HIP(hipMemcpy(v.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost));
  return S4P_ICP_OK;
}

// normalised in double, rounded to float; zero or non-finite -> (0, 0, 0).  device: the inputs are device arrays.
int32_t normalise_host(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, size_t n, bool device, std::vector<float> (&v)[3]) {
  std::vector<float> staged[3];
  if (device) {
    const float* in[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) if (int32_t rc = stage_to_host(h, in[a], n, staged[a])) return rc;
    nx = staged[0].data(); ny = staged[1].data(); nz = staged[2].data();
  }
  for (int a = 0; a < 3; ++a) v[a].assign(n, 0.f);
  for (size_t i = 0; i < n; ++i) {
    const double x = nx[i], y = ny[i], z = nz[i];
    const double len = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !(len > 0.0) || !std::isfinite(len)) continue;
    v[0][i] = float(x / len); v[1][i] = float(y / len); v[2][i] = float(z / len);
  }
  return S4P_ICP_OK;
}

// intensities on the host (staged from the device if need be): every value finite
int32_t intensity_host(s4p_icp_ctx* h, const float*& v, size_t n, bool device, std::vector<float>& staged, const char* who) {
  if (device) {
    if (int32_t rc = stage_to_host(h, v, n, staged)) return rc;
    v = staged.data();
  }
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return fail(h, S4P_ICP_ERR_BAD_ARG, std::string(who) + ": non-finite intensity");
  return S4P_ICP_OK;
}

int32_t alloc_normals(s4p_icp_ctx* h) {
  h->has_normals = false;
  h->has_grad = false;                           // the gradients lie in the tangent planes of the normals they were made with
  ICP_HIP(h->nrm.ensure(size_t(h->n_p)));
  return S4P_ICP_OK;
}

// caller normals in the uploaded order -> normalised, cell order
int32_t set_target_normals_impl(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n, bool device) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_normals: set_target first");
  if (!nx || !ny || !nz || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_normals: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  std::vector<float> v[3];
  if (int32_t rc = normalise_host(h, nx, ny, nz, size_t(n), device, v)) return rc;
  if (int32_t rc = alloc_normals(h)) return rc;
  Scratch S;
  float* d[3];
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&d[a], size_t(n) * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(d[a], v[a].data(), size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  }
  ICP_LAUNCH(k_gather_normals, blocks_for(h->n_p), d[0], d[1], d[2], h->tgt, uint64_t(n), h->nrm);
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_normals = true;
  return S4P_ICP_OK;
}

// source normals in the uploaded order -> normalised, stored on the device as they are read back
int32_t set_source_normals_impl(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n, bool device) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_normals: set_source first");
  if (!nx || !ny || !nz || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_normals: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  std::vector<float> v[3];
  if (int32_t rc = normalise_host(h, nx, ny, nz, size_t(n), device, v)) return rc;
  h->has_src_normals = false;
  for (int a = 0; a < 3; ++a) ICP_HIP(h->sn[a].ensure(size_t(n)));
  ICP_HIP(h->snrm.ensure(size_t(n)));
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(h->sn[a], v[a].data(), size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));          // v is released on return
  h->has_src_normals = true;
  return S4P_ICP_OK;
}

// target intensities in the uploaded order -> cell order
int32_t set_target_intensity_impl(s4p_icp_ctx* h, const float* v, int64_t n, bool device) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "set_target_intensity: set_target first");
  if (!v || n != h->n_p) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_target_intensity: null or not one per target point");
  ICP_HIP(hipSetDevice(h->device));
  std::vector<float> staged;
  if (int32_t rc = intensity_host(h, v, size_t(n), device, staged, "set_target_intensity")) return rc;
  h->has_tint = h->has_grad = false;
  ICP_HIP(h->tint.ensure(size_t(n)));
  Scratch S;
  float* d = nullptr;
  ICP_HIP(S.alloc((void**)&d, size_t(n) * sizeof(float)));
  ICP_HIP(hipMemcpyAsync(d, v, size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  ICP_LAUNCH(k_gather_target_intensity, blocks_for(h->n_p), d, h->tgt, uint64_t(n), h->tint);
  ICP_HIP(hipStreamSynchronize(h->st));          // v may be released on return; the scratch is
  h->has_tint = true;
  return S4P_ICP_OK;
}

// source intensities in the uploaded order: kept on the device in that order
int32_t set_source_intensity_impl(s4p_icp_ctx* h, const float* v, int64_t n, bool device) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_source_intensity: set_source first");
  if (!v || n != h->n_q) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_source_intensity: null or not one per source point");
  ICP_HIP(hipSetDevice(h->device));
  std::vector<float> staged;
  if (int32_t rc = intensity_host(h, v, size_t(n), device, staged, "set_source_intensity")) return rc;
  h->has_sint = false;
  ICP_HIP(h->si.ensure(size_t(n)));
  ICP_HIP(h->sint.ensure(size_t(n)));
  ICP_HIP(hipMemcpyAsync(h->si, v, size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));          // v may be released on return
  h->has_sint = true;
  return S4P_ICP_OK;
}

// a cell-ordered float4 array of the target (normals, gradients) -> three host arrays in the uploaded order
int32_t scatter_out(s4p_icp_ctx* h, const float4* cell_ordered, float* x, float* y, float* z) {
  ICP_HIP(hipSetDevice(h->device));
  Scratch S;
  const size_t n = size_t(h->n_p);
  float* d[3];
  for (int a = 0; a < 3; ++a) ICP_HIP(S.alloc((void**)&d[a], n * sizeof(float)));
  ICP_LAUNCH(k_scatter_normals, blocks_for(h->n_p), cell_ordered, h->tgt, uint64_t(n), d[0], d[1], d[2]);
  float* out[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(out[a], d[a], n * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

PassKind kind_of(int metric, double param = 0.0) {
  PassKind K;
  K.metric = metric; K.param = param;
  return K;
}

}  // namespace

extern "C" {

void s4p_icp_default_params(s4p_icp_params* p) {
  if (!p) return;
  p->max_iterations = 30;
  p->min_correspondences = 3;
  p->rel_tol = 1e-6;
  p->order_source = 1;
  p->reserved = 0;
}

const char* s4p_icp_last_error(const s4p_icp_ctx* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t s4p_icp_create(int32_t device, s4p_icp_ctx** out) {
  if (!out) { g_create_error = "null argument"; return S4P_ICP_ERR_BAD_ARG; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: the MI355X path has no CPU fallback";
    return S4P_ICP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_error = "bad device index"; return S4P_ICP_ERR_BAD_ARG; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return S4P_ICP_ERR_HIP; }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    g_create_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return S4P_ICP_ERR_NO_DEVICE;
  }
  s4p_icp_ctx* h = new s4p_icp_ctx();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev, hipEventDisableTiming) != hipSuccess || h->dsum.ensure(kSumsCap) != hipSuccess ||
      h->hsum.ensure(kSumsCap) != hipSuccess) {
    g_create_error = "HIP stream / event / buffer creation failed";
    s4p_icp_destroy(h);
    return S4P_ICP_ERR_HIP;
  }
  *out = h;
  return S4P_ICP_OK;
}

void s4p_icp_destroy(s4p_icp_ctx* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  if (h->ev) (void)hipEventDestroy(h->ev);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;                                      // the buffers release themselves
}

int32_t s4p_icp_set_target(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance) {
  return set_target_impl(h, x, y, z, n, max_distance, hipMemcpyHostToDevice);
}
int32_t s4p_icp_set_target_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance) {
  return set_target_impl(h, x, y, z, n, max_distance, hipMemcpyDeviceToDevice);
}
int32_t s4p_icp_set_source(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_source_impl(h, x, y, z, n, hipMemcpyHostToDevice);
}
int32_t s4p_icp_set_source_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n) {
  return set_source_impl(h, x, y, z, n, hipMemcpyDeviceToDevice);
}

int32_t s4p_icp_frame(const s4p_icp_ctx* h, float* c3) {
  if (!h || !c3) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return S4P_ICP_ERR_STATE;
  for (int a = 0; a < 3; ++a) c3[a] = h->c[a];
  return S4P_ICP_OK;
}

int32_t s4p_icp_correspondences(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !idx || !d2) return fail(h, S4P_ICP_ERR_BAD_ARG, "correspondences: null argument");
  if (int32_t rc = ready(h)) return rc;
  Scratch S;
  int32_t* di;
  float* dd;
  ICP_HIP(S.alloc((void**)&di, size_t(h->n_q) * 4));
  ICP_HIP(S.alloc((void**)&dd, size_t(h->n_q) * 4));
  double sums[S4P_ICP_NSUMS];
  if (int32_t rc = pass(h, centred_from_float16(T16_centred), h->src, di, dd, sums)) return rc;
  ICP_HIP(hipMemcpy(idx, di, size_t(h->n_q) * 4, hipMemcpyDeviceToHost));
  ICP_HIP(hipMemcpy(d2, dd, size_t(h->n_q) * 4, hipMemcpyDeviceToHost));
  return S4P_ICP_OK;
}

int32_t s4p_icp_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "sums: null argument");
  if (int32_t rc = ready(h)) return rc;
  return sums_call(h, kind_of(kPoint), T16_centred, sums, nullptr);
}

int32_t s4p_icp_refine(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result) {
  return refine_loop(h, params, kind_of(kPoint), 0, nullptr, T16_inout, result, nullptr, "refine");
}

int32_t s4p_icp_apply(s4p_icp_ctx* h, const double* T16, float* x, float* y, float* z, int64_t n) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16 || !x || !y || !z || n < 0) return fail(h, S4P_ICP_ERR_BAD_ARG, "apply: null argument");
  if (n == 0) return S4P_ICP_OK;
  ICP_HIP(hipSetDevice(h->device));
  Scratch S;
  float* p[3];
  float* io[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    ICP_HIP(S.alloc((void**)&p[a], size_t(n) * sizeof(float)));
    ICP_HIP(hipMemcpyAsync(p[a], io[a], size_t(n) * sizeof(float), hipMemcpyHostToDevice, h->st));
  }
  ICP_LAUNCH(k_apply_icp, blocks_for(n), to_float(T16), p[0], p[1], p[2], uint64_t(n));
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(io[a], p[a], size_t(n) * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// point-to-plane (include/s4p_icp_plane.h)

int32_t s4p_icp_set_target_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  return set_target_normals_impl(h, nx, ny, nz, n, false);
}
int32_t s4p_icp_set_target_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  return set_target_normals_impl(h, nx, ny, nz, n, true);
}

int32_t s4p_icp_estimate_normals(s4p_icp_ctx* h, float radius, int32_t min_neighbours) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "estimate_normals: set_target first");
  if (!(radius > 0.f) || !(radius <= h->d))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_normals: radius must be in (0, max_distance]");
  if (min_neighbours < 3) return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_normals: min_neighbours must be >= 3");
  ICP_HIP(hipSetDevice(h->device));
  if (int32_t rc = alloc_normals(h)) return rc;
  ICP_LAUNCH(k_normals, blocks_for(h->n_p), h->g, uint64_t(h->n_p), radius * radius, min_neighbours, h->nrm);
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_normals = true;
  return S4P_ICP_OK;
}

int32_t s4p_icp_target_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!nx || !ny || !nz) return fail(h, S4P_ICP_ERR_BAD_ARG, "target_normals: null argument");
  if (!h->has_target || !h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "target_normals: no normals");
  return scatter_out(h, h->nrm, nx, ny, nz);
}

int32_t s4p_icp_plane_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "plane_sums: null argument");
  if (int32_t rc = plane_ready(h)) return rc;
  return sums_call(h, kind_of(kPlane), T16_centred, sums, nullptr);
}

int32_t s4p_icp_refine_plane(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result) {
  return refine_loop(h, params, kind_of(kPlane), 0, nullptr, T16_inout, result, nullptr, "refine");
}

// ---------------------------------------------------------------------------------------------------------------------
// robust ICP (include/s4p_icp_robust.h)

void s4p_icp_robust_defaults(s4p_icp_robust* r, int32_t loss) {
  if (!r) return;
  std::memset(r, 0, sizeof(*r));
  r->loss = loss;
  r->trim_fraction = 1.0;
  r->scale = 0.0;
  r->c = loss == S4P_ICP_LOSS_HUBER ? S4P_ICP_HUBER_C : (loss == S4P_ICP_LOSS_TUKEY ? S4P_ICP_TUKEY_C : 0.0);
}

int32_t s4p_icp_robust_sums(s4p_icp_ctx* h, const float* T16_centred, int32_t metric, const s4p_icp_robust* robust, double* sums,
                            double* info) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "robust_sums: null argument");
  PassKind K = kind_of(metric == S4P_ICP_METRIC_PLANE ? kPlane : kPoint);
  K.robust = true;
  if (int32_t rc = ready_for(h, K)) return rc;
  if (int32_t rc = robust_cfg(h, metric, robust, &K.cfg)) return rc;
  return sums_call(h, K, T16_centred, sums, info);
}

int32_t s4p_icp_refine_robust(s4p_icp_ctx* h, const s4p_icp_params* params, int32_t metric, const s4p_icp_robust* robust,
                              double* T16_inout, s4p_icp_result* result, double* info_out) {
  PassKind K = kind_of(metric == S4P_ICP_METRIC_PLANE ? kPlane : kPoint);
  K.robust = true;
  return refine_loop(h, params, K, metric, robust, T16_inout, result, info_out, "refine_robust");
}

// ---------------------------------------------------------------------------------------------------------------------
// generalized ICP (include/s4p_icp_gicp.h)

int32_t s4p_icp_set_source_normals(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  return set_source_normals_impl(h, nx, ny, nz, n, false);
}
int32_t s4p_icp_set_source_normals_device(s4p_icp_ctx* h, const float* nx, const float* ny, const float* nz, int64_t n) {
  return set_source_normals_impl(h, nx, ny, nz, n, true);
}

int32_t s4p_icp_source_normals(s4p_icp_ctx* h, float* nx, float* ny, float* nz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!nx || !ny || !nz) return fail(h, S4P_ICP_ERR_BAD_ARG, "source_normals: null argument");
  if (!h->has_source || !h->has_src_normals) return fail(h, S4P_ICP_ERR_STATE, "source_normals: no normals");
  ICP_HIP(hipSetDevice(h->device));
  float* out[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) ICP_HIP(hipMemcpyAsync(out[a], h->sn[a], size_t(h->n_q) * sizeof(float), hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  return S4P_ICP_OK;
}

int32_t s4p_icp_gicp_sums(s4p_icp_ctx* h, const float* T16_centred, double epsilon, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "gicp_sums: null argument");
  if (int32_t rc = gicp_ready(h, epsilon)) return rc;
  return sums_call(h, kind_of(kGicp, epsilon), T16_centred, sums, nullptr);
}

int32_t s4p_icp_refine_gicp(s4p_icp_ctx* h, const s4p_icp_params* params, double epsilon, double* T16_inout, s4p_icp_result* result) {
  return refine_loop(h, params, kind_of(kGicp, epsilon), 0, nullptr, T16_inout, result, nullptr, "refine");
}

// ---------------------------------------------------------------------------------------------------------------------
// symmetric ICP (include/s4p_icp_symm.h)

int32_t s4p_icp_symm_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "symm_sums: null argument");
  if (int32_t rc = symm_ready(h)) return rc;
  return sums_call(h, kind_of(kSymm), T16_centred, sums, nullptr);
}

int32_t s4p_icp_refine_symm(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result) {
  return refine_loop(h, params, kind_of(kSymm), 0, nullptr, T16_inout, result, nullptr, "refine");
}

// ---------------------------------------------------------------------------------------------------------------------
// coloured ICP (include/s4p_icp_color.h)

int32_t s4p_icp_set_target_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  return set_target_intensity_impl(h, intensity, n, false);
}
int32_t s4p_icp_set_target_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  return set_target_intensity_impl(h, intensity, n, true);
}
int32_t s4p_icp_set_source_intensity(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  return set_source_intensity_impl(h, intensity, n, false);
}
int32_t s4p_icp_set_source_intensity_device(s4p_icp_ctx* h, const float* intensity, int64_t n) {
  return set_source_intensity_impl(h, intensity, n, true);
}

int32_t s4p_icp_estimate_color_gradients(s4p_icp_ctx* h, float radius, int32_t min_neighbours) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!h->has_target) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: set_target first");
  if (!h->has_normals) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: target normals first");
  if (!h->has_tint) return fail(h, S4P_ICP_ERR_STATE, "estimate_color_gradients: target intensity first");
  if (!(radius > 0.f) || !(radius <= h->d))
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_color_gradients: radius must be in (0, max_distance]");
  if (min_neighbours < S4P_ICP_COLOR_MIN_NEIGHBOURS)
    return fail(h, S4P_ICP_ERR_BAD_ARG, "estimate_color_gradients: min_neighbours must be >= 4");
  ICP_HIP(hipSetDevice(h->device));
  h->has_grad = false;
  ICP_HIP(h->grad.ensure(size_t(h->n_p)));
  ICP_LAUNCH(k_color_gradient, blocks_for(h->n_p), h->g, h->nrm, h->tint, uint64_t(h->n_p), radius * radius, min_neighbours, h->grad);
  ICP_HIP(hipStreamSynchronize(h->st));
  h->has_grad = true;
  return S4P_ICP_OK;
}

int32_t s4p_icp_target_color_gradients(s4p_icp_ctx* h, float* gx, float* gy, float* gz) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!gx || !gy || !gz) return fail(h, S4P_ICP_ERR_BAD_ARG, "target_color_gradients: null argument");
  if (!h->has_target || !h->has_grad) return fail(h, S4P_ICP_ERR_STATE, "target_color_gradients: no gradients");
  return scatter_out(h, h->grad, gx, gy, gz);
}

int32_t s4p_icp_color_sums(s4p_icp_ctx* h, const float* T16_centred, double lambda, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "color_sums: null argument");
  if (int32_t rc = color_ready(h, lambda)) return rc;
  return sums_call(h, kind_of(kColor, lambda), T16_centred, sums, nullptr);
}

int32_t s4p_icp_refine_color(s4p_icp_ctx* h, const s4p_icp_params* params, double lambda, double* T16_inout, s4p_icp_result* result) {
  return refine_loop(h, params, kind_of(kColor, lambda), 0, nullptr, T16_inout, result, nullptr, "refine");
}

// ---------------------------------------------------------------------------------------------------------------------
// correspondence rejection (include/s4p_icp_reject.h)

void s4p_icp_reject_defaults(s4p_icp_reject* r) {
  if (r) std::memset(r, 0, sizeof(*r));
}

int32_t s4p_icp_set_rejection(s4p_icp_ctx* h, const s4p_icp_reject* r) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  s4p_icp_reject R;
  s4p_icp_reject_defaults(&R);
  if (r) {
    if (r->reciprocal != 0 && r->reciprocal != 1) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: reciprocal must be 0 or 1");
    R.reciprocal = r->reciprocal;
    R.normal_mode = r->normal_mode;
    if (r->normal_mode == S4P_ICP_REJECT_NORMALS_UNORIENTED) {
      if (!(r->normal_cos >= 0.0 && r->normal_cos <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: normal_cos must be in [0, 1] (unoriented)");
      R.normal_cos = r->normal_cos;
    } else if (r->normal_mode == S4P_ICP_REJECT_NORMALS_ORIENTED) {
      if (!(r->normal_cos >= -1.0 && r->normal_cos <= 1.0)) return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: normal_cos must be in [-1, 1] (oriented)");
      R.normal_cos = r->normal_cos;
    } else if (r->normal_mode != S4P_ICP_REJECT_NORMALS_OFF) {
      return fail(h, S4P_ICP_ERR_BAD_ARG, "set_rejection: unknown normal_mode");
    }
  }
  h->rej = R;
  h->rej_on = R.reciprocal != 0 || R.normal_mode != S4P_ICP_REJECT_NORMALS_OFF;
  return S4P_ICP_OK;
}

int32_t s4p_icp_rejection(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2, int32_t* why) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !idx || !d2 || !why) return fail(h, S4P_ICP_ERR_BAD_ARG, "rejection: null argument");
  if (int32_t rc = ready(h)) return rc;
  if (int32_t rc = prepare(h, h->src, nullptr)) return rc;
  Scratch S;
  const uint64_t un = uint64_t(h->n_q);
  int32_t *di, *dw;
  float* dd;
  uint8_t* code;
  ICP_HIP(S.alloc((void**)&di, un * 4)); ICP_HIP(S.alloc((void**)&dd, un * 4)); ICP_HIP(S.alloc((void**)&dw, un * 4));
  ICP_HIP(S.alloc((void**)&code, un));
  if (int32_t rc = launch_search(h, centred_from_float16(T16_centred), h->src, false, code)) return rc;
  ICP_LAUNCH(k_reject_out, blocks_for(h->n_q), h->src, h->tgt, h->rslot, h->rkey, code, un, di, dd, dw);
  ICP_HIP(hipMemcpyAsync(idx, di, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipMemcpyAsync(d2, dd, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipMemcpyAsync(why, dw, un * 4, hipMemcpyDeviceToHost, h->st));
  ICP_HIP(hipStreamSynchronize(h->st));
  reject_done(h);
  return S4P_ICP_OK;
}

int32_t s4p_icp_rejection_counts(const s4p_icp_ctx* h, int64_t counts[4]) {
  if (!h || !counts) return S4P_ICP_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k) counts[k] = h->rej_counts[k];
  return S4P_ICP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the information matrix of a pairwise pose (include/s4p_icp_info.h)

int32_t s4p_icp_information_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16_centred || !sums) return fail(h, S4P_ICP_ERR_BAD_ARG, "information_sums: null argument");
  return info_call(h, centred_from_float16(T16_centred), sums);
}

int32_t s4p_icp_information_from_sums(const double* s, const float* c3, double* info36, int64_t* n_corr, double* rmse) {
  if (!s || !c3 || !info36) return S4P_ICP_ERR_BAD_ARG;
  // include/s4p_icp_info.h's order of operations
  const double n = s[0], c[3] = {double(c3[0]), double(c3[1]), double(c3[2])};
  std::memset(info36, 0, 36 * sizeof(double));
  if (n_corr) *n_corr = int64_t(n);
  if (rmse) *rmse = n > 0.0 ? std::sqrt(s[1] / n) : 0.0;
  if (!(n > 0.0)) return S4P_ICP_OK;
  double S[3], P[3][3];
  for (int a = 0; a < 3; ++a) S[a] = s[2 + a] + n * c[a];
  for (int a = 0, o = 5; a < 3; ++a)
    for (int b = a; b < 3; ++b, ++o) P[a][b] = P[b][a] = (s[o] + (s[2 + a] * c[b] + c[a] * s[2 + b])) + n * (c[a] * c[b]);
  const double tr = (P[0][0] + P[1][1]) + P[2][2];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) info36[6 * a + b] = a == b ? tr - P[a][a] : -P[a][b];
  const double X[3][3] = {{0.0, -S[2], S[1]}, {S[2], 0.0, -S[0]}, {-S[1], S[0], 0.0}};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      info36[6 * a + 3 + b] = X[a][b];
      info36[6 * (3 + a) + b] = X[b][a];              // -[S]x
      info36[6 * (3 + a) + 3 + b] = a == b ? n : 0.0;
    }
  return S4P_ICP_OK;
}

int32_t s4p_icp_information(s4p_icp_ctx* h, const double* T16, double* info36, int64_t* n_corr, double* rmse) {
  if (!h) return S4P_ICP_ERR_BAD_ARG;
  if (!T16 || !info36) return fail(h, S4P_ICP_ERR_BAD_ARG, "information: null argument");
  if (!h->has_target || !h->has_source) return fail(h, S4P_ICP_ERR_STATE, "set_target and set_source first");
  double Tc[16], s[S4P_ICP_INFO_NSUMS];
  to_centred(T16, h->c, Tc);
  if (int32_t rc = info_call(h, to_float(Tc), s)) return rc;
  return s4p_icp_information_from_sums(s, h->c, info36, n_corr, rmse);
}

}  // extern "C"
