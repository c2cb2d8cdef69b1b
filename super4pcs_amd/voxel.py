"""ctypes binding of include/s4p_voxel.h (libsuper4pcs_normals.so): voxel-grid downsampling on the device.

    from super4pcs_amd import voxel
    xyz_m, attrs_m, normals_m, counts, voxel_of = voxel.voxel_downsample(P, 0.01)                  # means of the occupied voxels
    xyz_m, rgb_m, n_m, counts, voxel_of = voxel.voxel_downsample(P, 0.01, attrs=rgb, normals=N)

A point's voxel is floor((double)x / (double)voxel_size) per axis on a lattice anchored at the world origin, so two clouds
share it.  Output rows are the occupied voxels in ascending (iz, iy, ix); every channel is the mean of the voxel's members
in ascending input index, summed in double in the fixed order of the header, rounded to float.  Points with a non-finite
coordinate are dropped (voxel_of = -1).  Clouds are (N, 3) float32 numpy arrays, or (N, 3) float32 torch tensors on the GPU
(they go through the _device entry point and the results are torch tensors on the same device); both give the same bits.
There is no CPU fallback: without a device, VoxelGrid() raises NormalsError with code -2.
"""
import ctypes as C

import numpy as np

from . import _binding as _B
from . import normals as _N
from ._binding import TWIN
from .normals import NormalsError, session

MAX_ATTR = 8

_VP = C.c_void_p
SIGNATURES = {                                         # include/s4p_voxel.h
    "s4p_voxel_downsample" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64, C.c_float, _VP, C.c_int32, _VP, _VP, _VP, _VP, C.POINTER(C.c_int64)],
}
SYMBOLS = _B.names(SIGNATURES)


def load_library(path=None):
    """The normals library with the s4p_voxel.h entry points declared; a library without them is an error."""
    return _N.load_library(path, SIGNATURES)


def _attr_block(attrs, n, dev, like):
    """(contiguous (n, nattr) float32 block of the kind of the cloud, nattr); an (n,) input is one channel."""
    if attrs is None:
        return None, 0
    if dev:
        import torch
        if not (_B.is_torch(attrs) and attrs.is_cuda and attrs.device == like.device and attrs.dtype == torch.float32):
            raise ValueError("with a GPU cloud, attributes are float32 tensors on the same device")
        a = attrs.reshape(attrs.shape[0], -1).contiguous()
    else:
        if _B.is_torch(attrs):
            raise ValueError("with a numpy cloud, attributes are numpy arrays")
        a = np.asarray(attrs)
        a = np.ascontiguousarray(a.reshape(a.shape[0], -1), dtype=np.float32)
    if a.shape[0] != n:
        raise ValueError("attributes have %d rows, the cloud %d" % (a.shape[0], n))
    if a.shape[1] < 1 or a.shape[1] > MAX_ATTR:
        raise ValueError("1 to %d attribute channels (normals count as 3), got %d" % (MAX_ATTR, a.shape[1]))
    return a, int(a.shape[1])


class VoxelGrid(_N.Normals):
    """An s4p_normals context (one GPU) with the voxel-grid downsample.  The cloud is passed per call; a cloud given to
    set_cloud, and what estimate returns on it, stay as they are."""
    _load = staticmethod(load_library)

    def downsample(self, xyz, voxel_size, attrs=None):
        """(xyz_m (m, 3) float32, attrs_m (m, nattr) float32 or None, counts (m,) int32, voxel_of (n,) int32)."""
        dev, ptr, n, keep = _B.cols(xyz)
        like = xyz if dev else None
        a, nattr = _attr_block(attrs, n, dev, like)
        out_xyz, pxyz = _B.empty(like, (n, 3), np.float32)
        out_attr, pattr = _B.empty(like, (n, nattr), np.float32) if nattr else (None, None)
        counts, pcnt = _B.empty(like, (n,), np.int32)
        vof, pvof = _B.empty(like, (n,), np.int32)
        pa = None if a is None else (a.data_ptr() if dev else a.ctypes.data)
        m = C.c_int64(0)
        self._call("s4p_voxel_downsample", like, *ptr, n, float(voxel_size), pa, nattr, pxyz, pattr, pcnt, pvof, C.byref(m))
        m = int(m.value)
        return out_xyz[:m], (None if out_attr is None else out_attr[:m]), counts[:m], vof


def renormalise(mean_normals):
    """Unit normals from averaged ones: n / sqrt((x*x + y*y) + z*z) in double, rounded to float; a mean of norm 0, or a
    non-finite one, gives (0, 0, 0), "no normal".  Done on the host for both kinds of input, so that they agree in bits."""
    if _B.is_torch(mean_normals):
        import torch
        return torch.from_numpy(renormalise(mean_normals.cpu().numpy())).to(mean_normals.device)
    d = np.asarray(mean_normals, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        out = (d / nn[:, None]).astype(np.float32)
    bad = ~(np.isfinite(nn) & (nn > 0)) | ~np.isfinite(out).all(1)
    out[bad] = 0
    return out


def voxel_downsample(xyz, voxel_size, attrs=None, normals=None, device=0):
    """Voxel-grid downsample of xyz at voxel_size: (xyz_m, attrs_m | None, normals_m | None, counts, voxel_of).  attrs
    ((n,) or (n, c)) are averaged per voxel as they are.  normals ride as three extra channels and are renormalised
    afterwards (renormalise); at most 8 channels in all.  numpy in gives numpy out, a GPU torch tensor in gives tensors on
    its device, with the same bits."""
    is_t = _B.is_torch(xyz)
    block, na = attrs, 0
    if attrs is not None:
        block = attrs.reshape(attrs.shape[0], -1) if is_t else np.asarray(attrs, np.float32).reshape(len(attrs), -1)
        na = int(block.shape[1])
    if normals is not None:
        if is_t:
            import torch
            nrm = normals.reshape(-1, 3)
            block = nrm if block is None else torch.cat([block, nrm], dim=1)
        else:
            nrm = np.asarray(normals, np.float32).reshape(-1, 3)
            block = nrm if block is None else np.concatenate([block, nrm], axis=1)
    with session(VoxelGrid, None, device) as ctx:
        xyz_m, block_m, counts, vof = ctx.downsample(xyz, voxel_size, block)
    attrs_m = normals_m = None
    if attrs is not None:
        attrs_m = block_m[:, :na]
        if len(attrs.shape) == 1:
            attrs_m = attrs_m[:, 0]
    if normals is not None:
        normals_m = renormalise(block_m[:, na:na + 3])
    return xyz_m, attrs_m, normals_m, counts, vof
