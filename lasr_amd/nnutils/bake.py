"""Bake the video frames onto a reconstruction as per-face surface textures (scripts/bake_texture.py).

This is the project's own addition: the reference has no counterpart.  Every texel of the [F, R*R, 3] surface-texture tensor the
rasteriser samples (texture_type='surface') is projected into every frame, tested for visibility against a hard-mode raster of
that frame's mesh, and averaged with the weight |n . d|^power (lasr_bake_accumulate / lasr_bake_resolve, csrc/bake.hip).

Scenes are in camera space with OpenCV axes and pixel intrinsics fx fy px py of the H x W frame, as in lasr_amd/vis.py; the
raster is the square of side IS = max(H, W) with the NDC mapping of vis.shade.  Frames are processed CHUNK_FRAMES at a time: one
raster and one accumulate launch per chunk, one resolve launch at the end.
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


def bake_texture(verts, faces, K, frames, masks=None, texture_res=8, power=2, fallback=None):
    """verts [T,V,3] camera space, faces [F,3] (shared), K [T,4] = fx fy px py (pixels), frames uint8 [T,H,W,3], masks [T,H,W]
    (> 0 = foreground) or None, fallback [V,3] vertex colours (0-1) for texels no frame sees, or None for 0.5 grey.
    -> (textures [F, R*R, 3] float32, weight [F, R*R] float32) on the device; weight is the summed |n . d|^power."""
    for name, t in (('verts', verts), ('faces', faces), ('K', K), ('frames', frames), ('masks', masks), ('fallback', fallback)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError('bake_texture: %s must be a tensor' % name)
    _lib.need_cuda(verts, faces, K, frames, masks, fallback)
    dev = verts.device
    R, power = int(texture_res), int(power)
    if verts.ndimension() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
        raise ValueError('bake_texture: verts must be [T, V >= 1, 3], got %s' % (tuple(verts.shape),))
    T, V = verts.shape[:2]
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('bake_texture: faces must be integer [F, 3], got %s %s' % (faces.dtype, tuple(faces.shape)))
    F = faces.shape[0]
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError('bake_texture: faces must index the %d vertices' % V)
    if frames.dtype != torch.uint8 or frames.ndimension() != 4 or frames.shape[0] != T or frames.shape[3] != 3:
        raise ValueError('bake_texture: frames must be uint8 [T = %d, H, W, 3], got %s %s' % (T, frames.dtype, tuple(frames.shape)))
    H, W = int(frames.shape[1]), int(frames.shape[2])
    IS = max(H, W)
    if not (1 <= H and 1 <= W and IS <= _lib.BAKE_MAX_SIZE):
        raise ValueError('bake_texture: frames of %d x %d: each side must be 1..%d' % (H, W, _lib.BAKE_MAX_SIZE))
    if K.numel() != T * 4:
        raise ValueError('bake_texture: K must be [T = %d, 4] (fx fy px py), got %s' % (T, tuple(K.shape)))
    if masks is not None and tuple(masks.shape) != (T, H, W):
        raise ValueError('bake_texture: masks must be [%d, %d, %d] like the frames, got %s' % (T, H, W, tuple(masks.shape)))
    if fallback is not None and tuple(fallback.shape) != (V, 3):
        raise ValueError('bake_texture: fallback must be [V = %d, 3] vertex colours, got %s' % (V, tuple(fallback.shape)))
    if not 1 <= R <= _lib.BAKE_MAX_RES:
        raise ValueError('bake_texture: texture_res must be 1..%d, got %d' % (_lib.BAKE_MAX_RES, R))
    if not 0 <= power <= _lib.BAKE_MAX_POWER:
        raise ValueError('bake_texture: power must be an integer in 0..%d, got %d' % (_lib.BAKE_MAX_POWER, power))
    if F * R * R * 4 > 0x7fffffff:
        raise ValueError('bake_texture: %d faces x %d texels exceed the 32-bit texel index' % (F, R * R))

    verts = verts.detach().float().contiguous()
    faces32 = faces.to(torch.int32).contiguous()
    K = K.detach().float().reshape(T, 4).contiguous()
    frames = frames.contiguous()
    if masks is not None:
        masks = (masks > 0).to(torch.uint8).contiguous()
    if fallback is not None:
        fallback = fallback.detach().float().contiguous()
    accum = torch.zeros(F, R * R, 4, dtype=torch.float32, device=dev)
    textures = torch.empty(F, R * R, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(F, R * R, dtype=torch.float32, device=dev)
    if F == 0:
        return textures, weight
    for i in range(0, T, CHUNK_FRAMES):
        j = min(i + CHUNK_FRAMES, T)
        v, k, fr = verts[i:j], K[i:j], frames[i:j]
        raster = face_index_raster(v, faces32, k, IS)
        _lib.call('lasr_bake_accumulate', v, faces32, k, raster, fr, masks[i:j] if masks is not None else None, accum, j - i, V, F, R,
                  IS, H, W, power)
    _lib.call('lasr_bake_resolve', accum, faces32, fallback, textures, weight, V, F, R)
    return textures, weight


def render_baked(verts, faces, K, textures, H, W, background=(0., 0., 0.)):
    """The baked mesh seen from N cameras: verts [N,V,3] camera space, faces [F,3], K [N,4], textures [F,R*R,3] -> float32
    [N,4,H,W] (rgb, alpha): a hard-mode SoftRenderer with texture_type='surface' rasterises the mesh under the NDC mapping of
    the bake's own raster (face_index_raster), cropped to H x W."""
    from .. import soft_renderer as sr
    _lib.need_cuda(verts, faces, K, textures)
    N = verts.shape[0]
    IS = max(int(H), int(W))
    verts = verts.detach().float().contiguous()
    K = K.detach().float().reshape(N, 4)
    near, far = depth_range(verts)
    renderer = sr.SoftRenderer(image_size=IS, background_color=list(background), near=near, far=far, fill_back=True,
                               sigma_val=1e-12, aggr_func_rgb='hard', dist_func='hard', aggr_func_alpha='hard',
                               texture_type='surface', camera_mode='look_at')
    mesh = sr.Mesh(ndc_vertices(verts, K, IS), faces.to(torch.int32)[None].expand(N, -1, -1).contiguous(),
                   textures=textures.detach().float()[None].expand(N, -1, -1, -1).contiguous(), texture_type='surface')
    with torch.no_grad():                              # the vertices are in NDC already: the rasteriser stage alone
        out = renderer.rasterizer(mesh)
    return out[:, :, :H, :W]
