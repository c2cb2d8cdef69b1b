/* s4p_normals.h -- C ABI of libsuper4pcs_normals.so: k-nearest-neighbour normal estimation for whole point clouds on an
 * MI355X (gfx950).  No CPU fallback: without a device, s4p_normals_create fails with S4P_NORMALS_ERR_NO_DEVICE.
 *
 * Contract (DESIGN.md section "Normal estimation"):
 *  - Cloud X: n float points (SoA), in the caller's coordinates (no re-centring).  Queries: X itself (estimate) or m
 *    caller points (estimate_at).
 *  - d2(q, j) = dx*dx + (dy*dy + dz*dz) in float, dx = fl(x_j - q_x).
 *  - N(q): the k points of X with the smallest (d2, index), compared lexicographically (ties to the smaller index); with
 *    radius r > 0 only points with d2 <= fl(r*r) count ("hybrid"), with r <= 0 the search is unbounded (pure kNN).
 *  - |N(q)| < 3 gives the normal (0, 0, 0).  Otherwise, with e_j = x_j - q in double summed in ascending (d2, index) order,
 *    C = sum e e^T / |N| - m m^T (m = sum e / |N|); a trace of C that is not > 0 gives (0, 0, 0); else the unit eigenvector
 *    of C's smallest eigenvalue (cyclic Jacobi in double, first on ties), signed so that its component of largest
 *    magnitude (the first of equal ones) is positive, rounded to float.
 *  - out: one (nx, ny, nz) float triple per query, interleaved (3 floats per query), in the caller's query order.  Two calls
 *    give the same bits; host and device forms give the same bits.  A non-finite query gets (0, 0, 0).
 *
 * Limits (S4P_NORMALS_ERR_BAD_ARG outside them): 1 <= n <= 2^31 - 2 finite points; 3 <= k <= 32; radius finite
 * (<= 0: unbounded); 0 <= m <= 2^31 - 2; non-null pointers (queries and out may be null when m == 0).  The cloud's scale:
 * set_cloud refuses a cloud whose planned cell edge (about the distance to the 16th neighbour, at least 2^-20 of the
 * largest extent; s4p_normals_grid reports it) is below 2^-43, about 1.1e-13.  Under it squared distances between
 * neighbours fall into float's subnormal range, where the contract's float d2 cannot order them: rescale such a cloud.  A
 * cloud of identical points (extent 0) is accepted.  Large scales have no limit: where d2 overflows, the lists hold the
 * +inf the float expression gives, ordered by index.
 */
#ifndef S4P_NORMALS_H_
#define S4P_NORMALS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_NORMALS_OK 0
#define S4P_NORMALS_ERR_BAD_ARG (-1)
#define S4P_NORMALS_ERR_NO_DEVICE (-2)
#define S4P_NORMALS_ERR_HIP (-3)
#define S4P_NORMALS_ERR_OOM (-4)
#define S4P_NORMALS_ERR_STATE (-7)

#define S4P_NORMALS_MIN_K 3
#define S4P_NORMALS_MAX_K 32

typedef struct s4p_normals_ctx s4p_normals_ctx;

/* The grid set_cloud planned (for profiles): cell edge h = the median distance to the 16th neighbour over a fixed, seeded
 * sample of the cloud (enlarged x1.25 until the dense grid fits its cell cap), and the occupancy it gave. */
typedef struct s4p_normals_grid_info {
  double cell;                     /* h */
  double spacing;                  /* the sampled 16th-neighbour distance h was planned from */
  int32_t dims[3];
  int32_t reserved;
  int64_t cells;                   /* dims[0] * dims[1] * dims[2] */
  int64_t nonempty;                /* cells holding at least one point */
  double mean_per_cell;            /* n / nonempty */
  int64_t p99_per_cell;            /* 99th percentile of the points per non-empty cell */
  int64_t max_per_cell;
} s4p_normals_grid_info;

int32_t s4p_normals_create(int32_t device, s4p_normals_ctx** out);
void s4p_normals_destroy(s4p_normals_ctx* h);
const char* s4p_normals_last_error(const s4p_normals_ctx* h);   /* h may be null: the error of the last failed create */

/* the cloud X: host SoA, or device SoA on the context's device (copied device to device); builds the grid */
int32_t s4p_normals_set_cloud(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n);
int32_t s4p_normals_set_cloud_device(s4p_normals_ctx* h, const float* x, const float* y, const float* z, int64_t n);

/* normals of X itself: out[3 n], host or device memory */
int32_t s4p_normals_estimate(s4p_normals_ctx* h, int32_t k, float radius, float* out);
int32_t s4p_normals_estimate_device(s4p_normals_ctx* h, int32_t k, float radius, float* out);

/* normals at m query positions (SoA) from their neighbours in X: out[3 m]; host forms read and write host memory, device
 * forms device memory */
int32_t s4p_normals_estimate_at(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                float radius, float* out);
int32_t s4p_normals_estimate_at_device(s4p_normals_ctx* h, const float* qx, const float* qy, const float* qz, int64_t m, int32_t k,
                                       float radius, float* out);

int32_t s4p_normals_grid(s4p_normals_ctx* h, s4p_normals_grid_info* info);

#ifdef __cplusplus
}
#endif
#endif
