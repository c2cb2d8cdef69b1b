/* s4p_icp.h -- C ABI of libsuper4pcs_icp.so: point-to-point ICP that refines a registration on the full-resolution
 * clouds, on an MI355X (gfx950).  No CPU fallback: without a device, s4p_icp_create fails with S4P_ICP_ERR_NO_DEVICE.
 *
 * Conventions (DESIGN.md section "ICP refinement"):
 *  - P is the target, Q the source; a transform T maps Q onto P (p = T q), 4x4 row-major.
 *  - s4p_icp_set_target computes the frame c = float(mean of P, summed in double) and keeps P' = fl(P - c);
 *    s4p_icp_set_source keeps Q' = fl(Q - c).  The stage calls (correspondences, sums) take a float T in that CENTRED frame;
 *    s4p_icp_refine and s4p_icp_apply take a double T in the CALLER's frame.
 *  - Correspondence of source j for T: q^ = T q'_j rounded like k_apply, ((m0*x + m1*y) + m2*z) + m3 without contraction;
 *    d2(i, j) = dx*dx + (dy*dy + dz*dz); c(j) = the i with the least d2 among d2 <= fl(d*d), ties to the smallest i, else -1.
 *  - Sums (S4P_ICP_NSUMS doubles) over matched pairs: [0] n, [1..3] sum q^, [4..6] sum p', [7..15] sum q^ p'^T (row-major,
 *    entry 3a+b = sum q^_a p'_b), [16] sum d2.
 */
#ifndef S4P_ICP_H_
#define S4P_ICP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_ICP_OK 0
#define S4P_ICP_ERR_BAD_ARG (-1)
#define S4P_ICP_ERR_NO_DEVICE (-2)
#define S4P_ICP_ERR_HIP (-3)
#define S4P_ICP_ERR_OOM (-4)
#define S4P_ICP_ERR_STATE (-7)

#define S4P_ICP_NSUMS 17
#define S4P_ICP_HISTORY 64

/* s4p_icp_result.status */
#define S4P_ICP_MAX_ITERATIONS 0     /* k + 1 == max_iterations */
#define S4P_ICP_CONVERGED 1          /* |rmse_k - rmse_{k-1}| <= rel_tol * rmse_{k-1} */
#define S4P_ICP_TOO_FEW 2            /* n < min_correspondences: T_k kept */

typedef struct s4p_icp_ctx s4p_icp_ctx;

typedef struct s4p_icp_params {
  int32_t max_iterations;          /* default 30 */
  int32_t min_correspondences;     /* default 3 */
  double rel_tol;                  /* default 1e-6 */
  int32_t order_source;            /* 1: visit the source in the cell order of its T0-image (default); 0: as uploaded */
  int32_t reserved;
} s4p_icp_params;

typedef struct s4p_icp_result {
  int32_t iterations;              /* solves applied to T0 */
  int32_t status;                  /* S4P_ICP_MAX_ITERATIONS / _CONVERGED / _TOO_FEW */
  int64_t n_corr;                  /* final pass, for the returned transform */
  double rmse;                     /* final pass: sqrt(sum d2 / n_corr) (0 if n_corr == 0) */
  double fitness;                  /* final pass: n_corr / n_Q */
  int32_t history_len;             /* min(iterations evaluated, S4P_ICP_HISTORY) */
  int32_t reserved;
  double history_rmse[S4P_ICP_HISTORY];   /* rmse_k of T_k, k = 0.. */
  int64_t history_n[S4P_ICP_HISTORY];     /* n of T_k */
} s4p_icp_result;

void s4p_icp_default_params(s4p_icp_params* p);

int32_t s4p_icp_create(int32_t device, s4p_icp_ctx** out);
void s4p_icp_destroy(s4p_icp_ctx* h);
const char* s4p_icp_last_error(const s4p_icp_ctx* h);   /* h may be null: the error of the last failed create */

/* host SoA (float32) */
int32_t s4p_icp_set_target(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance);
int32_t s4p_icp_set_source(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n);
/* device SoA (float32, on the context's device): copied device to device */
int32_t s4p_icp_set_target_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n, float max_distance);
int32_t s4p_icp_set_source_device(s4p_icp_ctx* h, const float* x, const float* y, const float* z, int64_t n);

int32_t s4p_icp_frame(const s4p_icp_ctx* h, float* c3);

/* stage calls, centred frame, float T (16, row-major, last row ignored); outputs in the uploaded source order */
int32_t s4p_icp_correspondences(s4p_icp_ctx* h, const float* T16_centred, int32_t* idx, float* d2);
int32_t s4p_icp_sums(s4p_icp_ctx* h, const float* T16_centred, double* sums);

/* Horn's closed form on S4P_ICP_NSUMS sums: dT maps q^ onto p' (row-major 4x4).  Host only; needs no device.
 * Returns S4P_ICP_ERR_BAD_ARG when n < 1. */
int32_t s4p_icp_solve(const double* sums, double* dT16);

/* T16_inout: start transform in, refined transform out (caller frame, double).  params may be null (defaults). */
int32_t s4p_icp_refine(s4p_icp_ctx* h, const s4p_icp_params* params, double* T16_inout, s4p_icp_result* result);

/* x, y, z (host, n points, caller frame) <- float(T) applied in k_apply's order, on the device */
int32_t s4p_icp_apply(s4p_icp_ctx* h, const double* T16, float* x, float* y, float* z, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
