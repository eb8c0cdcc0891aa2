"""The posed sequence on the device: what the bake, the tracks and the reprojection scores all take.

T frames of one mesh in camera space with OpenCV axes: verts [T,V,3], faces [F,3] shared by every frame, K [T,4] = the pixel
intrinsics fx fy px py of the H x W frame, as in lasr_amd/vis.py.  A frame is rasterised in hard mode on the square of side
IS = max(H, W) with the NDC mapping of vis.shade (face_index_raster); the near and far planes are taken around the depths of the
frames rasterised together (depth_range).  Callers walk the frames a chunk at a time (Posed.chunks): one raster launch per chunk,
so device memory is bounded by the chunk and not by the video.  The chunk size is the caller's own CHUNK_FRAMES, by default the
one of vis.py.
"""
import torch

from .. import _lib
from .. import vis

CHUNK_FRAMES = vis.CHUNK_FRAMES


def ndc_vertices(verts, K, IS):
    """Camera-space verts [N,V,3] and K [N,4] (fx fy px py, pixels) -> [N,V,3] (NDC x, NDC y, depth) of the IS x IS raster:
    sx = 2u/IS - 1, sy = 1 - 2v/IS (row 0 is the top), the mapping of vis.shade."""
    x, y, z = verts.unbind(2)
    sx = 2 * (K[:, 0:1] * x / z + K[:, 2:3]) / IS - 1
    sy = 1 - 2 * (K[:, 1:2] * y / z + K[:, 3:4]) / IS
    return torch.stack([sx, sy, z], 2)


def depth_range(verts):
    """(near, far) around the depths of verts [N,V,3] for the hard-mode raster."""
    z = verts[..., 2]
    zmin, zmax = float(z.min()), float(z.max())
    if not (zmin > 0 and zmax < float('inf')):
        raise ValueError('bake_texture: every vertex must lie in front of the camera (depths span %g .. %g)' % (zmin, zmax))
    return 0.5 * zmin, 2. * zmax


def face_index_raster(verts, faces, K, IS):
    """Hard-mode raster of N frames -> aggrs_info [N,2,IS,IS] (plane 1: nearest face per pixel or -1)."""
    near, far = depth_range(verts)
    fv = ndc_vertices(verts, K, IS)[:, faces.long()].contiguous()
    return vis.hard_raster(fv, IS, near, far)


class Posed:
    """The record: verts float32 [T,V,3], faces32 int32 [F,3], K float32 [T,4], all detached and contiguous, with T, V, F, H, W,
    IS = max(H, W) and device.  The constructor only normalises; sequence() checks first."""

    def __init__(self, verts, faces, K, H, W):
        self.T, self.V, self.F = int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0])
        self.H, self.W = int(H), int(W)
        self.IS = max(self.H, self.W)
        self.device = verts.device
        self.verts = verts.detach().float().contiguous()
        self.faces32 = faces.to(torch.int32).contiguous()
        self.K = K.detach().float().reshape(self.T, 4).contiguous()

    def chunks(self, n, raster=True, only=None):
        """Yields (i, j, verts[i:j], K[i:j], raster) for i = 0, n, 2n, ...: raster is face_index_raster of the chunk, or None with
        raster=False.  only: a set of chunk indices i // n; the others are skipped without rasterising."""
        for i in range(0, self.T, n):
            if only is not None and i // n not in only:
                continue
            j = min(i + n, self.T)
            v, k = self.verts[i:j], self.K[i:j]
            yield i, j, v, k, face_index_raster(v, self.faces32, k, self.IS) if raster else None


def sequence(who, verts, faces, K, H, W, max_size):
    """The checked record: verts [T, V >= 1, 3], faces integer [F,3] that index the V vertices, K of T * 4 elements, 1 <= H, W <=
    max_size.  who names the caller in the messages."""
    for name, t in (('verts', verts), ('faces', faces), ('K', K)):
        if not torch.is_tensor(t):
            raise TypeError('%s: %s must be a tensor' % (who, name))
    _lib.need_cuda(verts, faces, K)
    if verts.ndimension() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
        raise ValueError('%s: verts must be [T, V >= 1, 3], got %s' % (who, tuple(verts.shape)))
    T, V = verts.shape[:2]
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('%s: faces must be integer [F, 3], got %s %s' % (who, faces.dtype, tuple(faces.shape)))
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError('%s: faces must index the %d vertices' % (who, V))
    if K.numel() != T * 4:
        raise ValueError('%s: K must be [T = %d, 4] (fx fy px py), got %s' % (who, T, tuple(K.shape)))
    H, W = int(H), int(W)
    if not (1 <= H and 1 <= W and max(H, W) <= max_size):
        raise ValueError('%s: frames of %d x %d: each side must be 1..%d' % (who, H, W, max_size))
    return Posed(verts, faces, K, H, W)
