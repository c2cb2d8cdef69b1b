// s4p_icp.hip -- libsuper4pcs_icp.so: point-to-point and point-to-plane ICP on the full-resolution clouds, with robust
// losses, generalized and coloured ICP (include/s4p_icp.h, include/s4p_icp_plane.h, include/s4p_icp_robust.h, include/s4p_icp_gicp.h,
// include/s4p_icp_color.h, DESIGN.md sections "ICP refinement", "Point-to-plane ICP", "Robust ICP", "Generalized ICP" and "Coloured ICP").  One translation unit, in the parts listed below.
//
// Device path:
//   set_target   k_stats (per-block double sums and float bounds of P) -> host frame c and grid plan ->
//                k_cell_keys (cell of fl(P - c)) -> radix sort of (cell, index) -> k_cell_starts + k_gather_target:
//                the target as cell-ordered float4 (x', y', z', index bits) and the start of every cell.
//   refine       once: k_source_keys (cell of the T0-image) -> radix sort -> k_gather_source (the source in that order);
//                per iteration: k_match (correspondence + 17 double sums per lane -> wave -> workgroup -> one slab row),
//                k_final (fixed-order sum of the slab), one pinned read-back, host solve.
//   plane        (include/s4p_icp_plane.h) target normals, cell-ordered next to tgt: k_normals (estimated) or
//                k_gather_normals (the caller's); per iteration k_match_plane (31 double sums) + k_final_plane, host solve.
//   robust       (include/s4p_icp_robust.h) per iteration k_search (winner slot + residual key per lane), the radix select of
//                the keys (k_key_hist + k_key_digit x 4, on the device), k_wsum + k_wfinal (weighted sums), host solve.
//   generalized  (include/s4p_icp_gicp.h) source normals in the order of the source (k_gather_source_normals); per iteration
//                k_search (winner slot per lane), k_gicp_sum (31 double sums streamed from the slots) + k_final_plane, host solve.
//   symmetric    (include/s4p_icp_symm.h) the generalized metric's inputs; per iteration k_search, k_symm_sum (31 double sums
//                streamed from the slots: the plane term along the sum of both normals) + k_final_plane, host solve
//                (the plane solve's 6x6 path, then the half-way rotation applied twice).
//   coloured     (include/s4p_icp_color.h) target intensities in cell order (k_gather_target_intensity), their tangent-plane
//                gradients (k_color_gradient, k_normals' walk), source intensities in the order of the source
//                (k_gather_source_intensity); per iteration k_search, k_color_sum (31 joint sums) + k_final_plane, host solve.
//   information  (include/s4p_icp_info.h) one call: k_search, k_info_sum (11 double sums over the winners streamed from the
//                slots) + k_final_info, one read-back; the 6x6 matrix on the host.
//   rejection    (include/s4p_icp_reject.h) a state of the context: a second grid over the source (set_target's plan and
//                build), and k_reject between k_search and the sum kernel of every split pass: it clears the slot and key of
//                a pair that fails the normal test or the reverse search.  Off: nothing of it is launched.
// No float or double atomics anywhere (the selection's histograms use integer atomics): every sum has a fixed order, so two calls return identical bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "s4p_icp.h"
#include "s4p_icp_plane.h"
#include "s4p_icp_robust.h"
#include "s4p_icp_gicp.h"
#include "s4p_icp_symm.h"
#include "s4p_icp_color.h"
#include "s4p_icp_reject.h"
#include "s4p_icp_batch.h"
#include "s4p_icp_info.h"
#include "s4p_icp_posegraph.h"


// The parts, in dependency order ("ICP sources: layout"):
//   s4p_icp_k_common.hip.hpp   constants, the grid, the float transform, nearest_t, jacobi_sym, the shared device helpers
//   s4p_icp_k_build.hip.hpp    kernels outside the iteration: statistics, cell keys and starts, gathers and scatters, the
//                              source order, the final apply, target normals and colour gradients
//   s4p_icp_k_pass.hip.hpp     kernels of a pass: the fused k_match / k_match_plane, k_search, k_reject, the selection, the
//                              weighted / generalized / symmetric / coloured sums, the final sums, k_reject_out
//   s4p_icp_solve.inc          host only: Horn's, the plane and the symmetric solve, transform helpers
//   s4p_icp_ctx.inc            owned buffers, the context, ICP_HIP / ICP_LAUNCH, scratch, grid plan and build, set_target / set_source
//   s4p_icp_pass.inc           prepare, the passes over one search / finish skeleton, the one refine loop
//   s4p_icp_abi.inc            the extern "C" entry points
#include "s4p_icp_k_common.hip.hpp"
#include "s4p_icp_k_build.hip.hpp"
#include "s4p_icp_k_pass.hip.hpp"
#include "s4p_icp_solve.inc"
#include "s4p_icp_ctx.inc"
#include "s4p_icp_pass.inc"
#include "s4p_icp_abi.inc"
// batched multi-start ICP (include/s4p_icp_batch.h), after the existing parts so that their kernels keep their places:
//   s4p_icp_k_batch.hip.hpp    k_match_batch, k_final_batch: a pose per row of workgroups
//   s4p_icp_batch.inc          the batch's buffers, the batched pass, the refine loop over an active list, the ranking
#include "s4p_icp_k_batch.hip.hpp"
#include "s4p_icp_batch.inc"
// pose-graph optimisation (include/s4p_icp_posegraph.h): host only, no kernel
#include "s4p_icp_posegraph.inc"
