/* s4p_voxel.h -- voxel-grid downsampling in libsuper4pcs_normals.so, on an MI355X (gfx950).  The functions work on an
 * s4p_normals_ctx (include/s4p_normals.h), which supplies the device, the stream, the work memory and
 * s4p_normals_last_error; the cloud is passed per call, and a cloud given to s4p_normals_set_cloud stays as it is.
 * No CPU fallback.
 *
 * Contract (DESIGN.md section "Voxel-grid downsampling and multi-scale ICP"):
 *  - Voxel of a point: v = (double)voxel; (ix, iy, iz) with i = floor((double)x / v), IEEE division, then floor.  The lattice
 *    is anchored at the world origin: it does not depend on the cloud, and two clouds share it.
 *  - A point with a non-finite coordinate is dropped (voxel_of = -1).
 *  - Output row r is the r-th occupied voxel in ascending (iz, iy, ix); m is their number.
 *  - A voxel's members are in ascending input index.  With c their number and t_0 .. t_{c-1} a channel's values as
 *    doubles, the sum has a fixed two-level order: block b covers the positions [64 b, min(64 b + 64, c)); s_b = t_{64 b},
 *    then s_b += t_j for the following positions in order; S = s_0, then S += s_b for b = 1, 2, ... in order.  The output
 *    is (float)(S / (double)c).  For c <= 64 this is the plain sequential sum.
 *  - x, y, z and every attribute channel are averaged this way, with no weighting and no renormalisation.  An attribute
 *    value is taken as it is: a NaN attribute gives a NaN mean.
 *  - Host forms read and write host memory, _device forms memory of the context's device (m_out is host memory in both).
 *    Two calls give the same bits; host and device forms give the same bits.
 *
 * Limits (S4P_NORMALS_ERR_BAD_ARG outside them): 1 <= n <= 2^31 - 2; voxel finite and > 0; 0 <= nattr <= 8; attr and
 * out_attr null exactly when nattr == 0; non-null x, y, z, out_xyz and m_out; the index extent of every axis
 * (max - min + 1 over the finite points) <= 2^21.  A cloud with no finite point returns S4P_NORMALS_OK with m = 0.
 */
#ifndef S4P_VOXEL_H_
#define S4P_VOXEL_H_

#include <stdint.h>

#include "s4p_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S4P_VOXEL_MAX_ATTR 8
#define S4P_VOXEL_MAX_EXTENT 2097152           /* 2^21 voxels per axis */
#define S4P_VOXEL_BLOCK 64                     /* positions per block of the two-level sum */

int32_t s4p_voxel_downsample(s4p_normals_ctx* h,
    const float* x, const float* y, const float* z, int64_t n, float voxel,
    const float* attr, int32_t nattr,   /* n*nattr interleaved; null iff nattr == 0 */
    float* out_xyz,      /* 3*n floats of capacity, interleaved; first 3*m written */
    float* out_attr,     /* n*nattr of capacity; null iff nattr == 0 */
    int32_t* out_count,  /* n of capacity, may be null */
    int32_t* voxel_of,   /* n, may be null: output row of each input point, -1 if dropped */
    int64_t* m_out);
int32_t s4p_voxel_downsample_device(s4p_normals_ctx* h,
    const float* x, const float* y, const float* z, int64_t n, float voxel,
    const float* attr, int32_t nattr, float* out_xyz, float* out_attr, int32_t* out_count, int32_t* voxel_of,
    int64_t* m_out);

#ifdef __cplusplus
}
#endif
#endif
