"""super4pcs_amd: MI355X-native (gfx950) hot path of Super4PCS global registration.

Layout (only what the path needs):
  csrc/        hand-written HIP kernels + the C ABI (include/s4p_capi.h) + host structures
  capi.py      ctypes binding of the C ABI (plumbing)
  icp_src/     ICP refinement (lib/libsuper4pcs_icp.so, include/s4p_icp.h): s4p_icp.hip over its s4p_icp_k_*.hip.hpp and *.inc parts; icp.py its ctypes binding
  normals_src/ kNN normal estimation, neighbour lists and outlier removal (lib/libsuper4pcs_normals.so, include/s4p_normals.h,
               include/s4p_knn.h); normals.py and knn.py their ctypes bindings
  matcher.py   Python mirror of the reference matcher interface on top of the C++ engine
  datasets.py  synthetic cloud generators of the BASELINE.json configs
  build.py     hipcc build of lib/libsuper4pcs_amd.so for gfx950
"""
__all__ = ["capi", "datasets", "build", "icp"]
