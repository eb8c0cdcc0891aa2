"""Diagnostic renders of extract.py --render and scripts/eval_mesh.py --render (reference: pytorch3d 0.4.0's MeshRenderer with
OrthographicCameras(), PointLights() in white, RasterizationSettings(cull_backfaces=True), SoftPhongShader and the default
BlendParams: nnutils/predictor.py:115-150, 296-335, scripts/eval_mesh.py:78-93, 170-192).

Visibility is the hard-mode rasteriser of soft_renderer (lasr_sr_forward_bg with func_id_rgb = func_id_alpha = 0), as in
lasr_amd/vis.py; lasr_phong_shade (csrc/phong.hip) shades and blends every pixel from its face-index map.  DESIGN.md section 4.8
states the conventions.  Vertices are in pytorch3d world coordinates, which the default orthographic camera maps to NDC
unchanged: pixel (r, c) of an S x S image sits at x = 1 - (2c + 1)/S, y = 1 - (2r + 1)/S (+X left, +Y up), depth z.
"""
import ctypes

import torch

from . import _lib
from .soft_renderer.functional import vertex_normals
from .vis import hard_raster

CHUNK_FRAMES = 16                 # frames per raster + shade launch pair (the raster's maps of 16 512^2 frames: 32 MB)
DEPTH_OFFSET = 1000.              # depth offset in units of the scene's depth range: the raster's 1/z interpolation stays ordered


def cull_mask(verts, faces):
    """bool [N,F]: faces turned away from the camera (pytorch3d's cull_backfaces), i.e. whose normal (v1 - v0) x (v2 - v0)
    has n_z > 0 (the camera looks along +z)."""
    p = verts[:, faces]
    e1, e2 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]
    return e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0] > 0


def raster_inputs(verts, faces, cull_backfaces=True):
    """The hard raster's input for pytorch3d-world vertices [N,V,3]: per face corner (raster NDC x = -x, y, offset depth), with
    culled faces moved in front of the near plane -> (fv [N,F,3,3], near, far).  Points with z < 0 fall in front of near, as
    pytorch3d's rasteriser drops them; the offset makes 1/z interpolation order faces by their linear z."""
    z = verts[..., 2]
    lo = float(torch.clamp(z.min(), max=0.))
    hi = float(torch.clamp(z.max(), min=0.))
    rng = max(hi - lo, 1e-6)
    off = DEPTH_OFFSET * rng - lo                                   # z = 0 -> off >= 1000 rng
    rv = torch.stack([-verts[..., 0], verts[..., 1], z + off], 2)
    fv = rv[:, faces].contiguous()                                   # N,F,3,3
    if cull_backfaces:
        cull = cull_mask(verts, faces)
        fv[..., 2] = torch.where(cull[..., None], torch.full_like(fv[..., 2], 0.5 * off), fv[..., 2])
    return fv, off, off + 2 * rng + 1.


def render(verts, faces, colors, S, background=(1., 1., 1.), return_maps=False, cull_backfaces=True):
    """pytorch3d-style Phong render of N meshes sharing one face list.

    verts [N,V,3] (pytorch3d world = view coordinates), faces [F,3] (outward winding: the caller applies vis.fix_inversion),
    colors [N,V,3] or [V,3] (vertex texels), S: image side.  -> float32 RGBA [N,S,S,4] on the device, unclamped: rgb blended over
    `background`, alpha = pytorch3d's silhouette probability.  With return_maps also the kernel's inputs of the last chunk;
    cull_backfaces=False keeps the faces turned away (the reference always culls).
    """
    if not verts.is_cuda:
        raise TypeError('phong.render: verts must be a HIP tensor (there is no CPU path)')
    dev = verts.device
    N, V = verts.shape[:2]
    faces = torch.as_tensor(faces, dtype=torch.long, device=dev)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or int(faces.min()) < 0 or int(faces.max()) >= V:
        raise ValueError('phong.render: faces must be [F,3] indices of the %d vertices' % V)
    if not (1 <= int(S) <= 8192):
        raise ValueError('phong.render: image side %r out of range' % (S,))
    if len(background) != 3:
        raise ValueError('phong.render: background is an RGB triple')
    S = int(S)
    verts = verts.float().contiguous()
    colors = torch.as_tensor(colors, dtype=torch.float32, device=dev).expand(N, V, 3)
    F = faces.shape[0]
    bg = (ctypes.c_float * 3)(*[float(c) for c in background])
    faces4 = torch.cat([faces, torch.zeros_like(faces[:, :1])], 1).int().contiguous()
    out = torch.empty(N, S, S, 4, device=dev)
    maps = None
    with torch.cuda.device(dev):
        for i in range(0, N, CHUNK_FRAMES):
            v = verts[i:i + CHUNK_FRAMES]
            n = v.shape[0]
            vn = vertex_normals(v, faces[None].expand(n, F, 3))
            zero = torch.zeros_like(v[..., :1])
            vert_rec = torch.cat([v, zero, vn, zero, colors[i:i + n], zero], 2).contiguous()
            fv, near, far = raster_inputs(v, faces, cull_backfaces)
            raster = hard_raster(fv, S, near, far)
            _lib.call('lasr_phong_shade', vert_rec, faces4, raster, bg, out[i:i + n], n, V, F, S)
            if return_maps:
                maps = dict(vert_rec=vert_rec, faces=faces4, raster=raster, fv=fv, near=near, far=far)
    return (out, maps) if return_maps else out
