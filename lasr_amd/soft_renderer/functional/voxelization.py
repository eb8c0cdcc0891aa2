"""Mesh voxelisation (reference: soft_renderer/functional/voxelization.py:41-57 over the `soft_renderer.cuda.voxelization`
extension): the HIP kernels of csrc/export.hip, a surface launch and a fill launch, with no host synchronisation."""
import torch

from ... import _lib

MAX_SIZE = 256                    # LASR_VOXEL_MAX_SIZE of include/lasr_ops.h


def voxelization(faces, size, normalize=False):
    """faces [B,F,3,3] float32 or float64 on the GPU -> voxels [B,size,size,size] int32, indexed by the face-vertex coordinates
    0, 1, 2: 1 where a voxel is on the surface (the reference's column scans along the three axes and the vertex voxels) or
    enclosed by it (not 6-connected through empty voxels to the grid's boundary).  Unless `normalize`, the coordinates are
    multiplied by `size` first, as the reference does (which ignores normalize=True).  Departure: size is limited to 256
    (64 MB of output per mesh); the reference has no limit."""
    _lib.need_cuda(faces)
    if faces.dtype not in (torch.float32, torch.float64):
        raise TypeError('voxelization takes float32 or float64 faces, got %s' % faces.dtype)
    if faces.ndimension() != 4 or faces.shape[2:] != (3, 3):
        raise ValueError('faces must be [B, F, 3, 3], got %s' % (tuple(faces.shape),))
    size = int(size)
    if not 1 <= size <= MAX_SIZE:
        raise ValueError('voxel size must be in [1, %d], got %d' % (MAX_SIZE, size))
    faces = faces.clone()
    if not normalize:
        faces *= size
    faces = faces.contiguous()
    B, F = faces.shape[:2]
    h = _lib.lib()
    voxels = torch.empty(B, size, size, size, dtype=torch.int32, device=faces.device)
    ws = torch.empty(max(int(h.lasr_voxelize_workspace_bytes(B, size)), 1), dtype=torch.uint8, device=faces.device)
    _lib.call('lasr_voxelize_f64' if faces.dtype == torch.float64 else 'lasr_voxelize', faces, voxels, None, ws, ws.numel(), B, F, size)
    return voxels
