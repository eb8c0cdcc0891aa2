"""Bake the video frames onto a reconstruction as per-face surface textures (scripts/bake_texture.py).

This is the project's own addition: the reference has no counterpart.  Every texel of the [F, R*R, 3] surface-texture tensor the
rasteriser samples (texture_type='surface') is projected into every frame, tested for visibility against a hard-mode raster of
that frame's mesh, and averaged with the weight |n . d|^power (lasr_bake_accumulate / lasr_bake_resolve, csrc/bake.hip).

Scenes are the posed sequences of lasr_amd/nnutils/posed.py, which states the conventions (camera space, intrinsics, the raster of
side IS = max(H, W)) and holds the raster helpers re-exported here.  Frames are processed CHUNK_FRAMES at a time (posed.py's
default): one raster and one accumulate launch per chunk, one resolve launch at the end.

complete_texture fills the texels no frame saw (opt-in; csrc/bake_fill.hip): mirror_fill copies the texel of the mirror image
over the symmetry plane of the rest shape, blend_fill smooths what is still unfilled over the texel adjacency (face_neighbours).
"""
import torch

from .. import _lib
from . import posed
from .posed import ndc_vertices, depth_range, face_index_raster   # noqa: F401  (their home is posed.py; tests and tools call them here)

CHUNK_FRAMES = posed.CHUNK_FRAMES


def bake_texture(verts, faces, K, frames, masks=None, texture_res=8, power=2, fallback=None):
    """verts [T,V,3] camera space, faces [F,3] (shared), K [T,4] = fx fy px py (pixels), frames uint8 [T,H,W,3], masks [T,H,W]
    (> 0 = foreground) or None, fallback [V,3] vertex colours (0-1) for texels no frame sees, or None for 0.5 grey.
    -> (textures [F, R*R, 3] float32, weight [F, R*R] float32) on the device; weight is the summed |n . d|^power."""
    for name, t in (('frames', frames), ('masks', masks), ('fallback', fallback)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError('bake_texture: %s must be a tensor' % name)
    _lib.need_cuda(frames, masks, fallback)
    R, power = int(texture_res), int(power)
    H, W = frames.shape[1:3] if frames.ndimension() == 4 else (1, 1)     # frames of another rank are refused below, by name
    seq = posed.sequence('bake_texture', verts, faces, K, H, W, _lib.BAKE_MAX_SIZE)
    dev, faces32, T, V, F, H, W = seq.device, seq.faces32, seq.T, seq.V, seq.F, seq.H, seq.W
    if frames.dtype != torch.uint8 or frames.ndimension() != 4 or frames.shape[0] != T or frames.shape[3] != 3:
        raise ValueError('bake_texture: frames must be uint8 [T = %d, H, W, 3], got %s %s' % (T, frames.dtype, tuple(frames.shape)))
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
    for i, j, v, k, raster in seq.chunks(CHUNK_FRAMES):
        _lib.call('lasr_bake_accumulate', v, faces32, k, raster, frames[i:j], masks[i:j] if masks is not None else None, accum, j - i,
                  V, F, R, seq.IS, H, W, power)
    _lib.call('lasr_bake_resolve', accum, faces32, fallback, textures, weight, V, F, R)
    return textures, weight


# ---- completing the atlas where no frame looked (csrc/bake_fill.hip; DESIGN.md section 4.11, "Fill") -----------------------------
# Own addition like the bake: parity is to the restatement in tests/bake_fill_restated.py and to closed forms only.
SEEN, MIRRORED, BLENDED = 0, 1, 2                     # the codes of `source`
MIRROR_REASONS = ('too far', 'normals disagree', 'source unseen', 'no valid face')   # src = -1 - reason (LASR_BAKE_MIRROR_*)


def _atlas(name, faces, textures, other, other_name):
    """Shared argument checks of the fills: faces integer [F,3], textures [F,R*R,3], `other` [F,R*R] -> (F, R)."""
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('%s: faces must be integer [F, 3], got %s %s' % (name, faces.dtype, tuple(faces.shape)))
    F = faces.shape[0]
    if textures.ndimension() != 3 or textures.shape[0] != F or textures.shape[2] != 3 or not textures.is_floating_point():
        raise ValueError('%s: textures must be floating [F = %d, R*R, 3], got %s %s' % (name, F, textures.dtype, tuple(textures.shape)))
    RR = int(textures.shape[1])
    R = int(round(RR ** 0.5))
    if R * R != RR or not 1 <= R <= _lib.BAKE_MAX_RES:
        raise ValueError('%s: textures hold %d texels per face, not R*R with R in 1..%d' % (name, RR, _lib.BAKE_MAX_RES))
    if tuple(other.shape) != (F, RR):
        raise ValueError('%s: %s must be [%d, %d] like the textures, got %s' % (name, other_name, F, RR, tuple(other.shape)))
    if F * RR * 4 > 0x7fffffff:
        raise ValueError('%s: %d faces x %d texels exceed the 32-bit texel index' % (name, F, RR))
    return F, R


def face_neighbours(faces, num_verts=None):
    """faces [F,3] integer (device) -> nbr int32 [F,3]: nbr[f, k] = (g * 3 + k') * 2 + same names the face g and its edge k' that
    share edge k of f (edge k lies opposite corner k and runs from corner (k+1)%3 to corner (k+2)%3; same = 1 when both edges start
    at the same vertex), or -1: an edge with anything but exactly two incident faces, or a face with a repeated or out-of-range
    index (negative, or >= num_verts where given).  Sort / unique on the device; a cold path."""
    if not torch.is_tensor(faces):
        raise TypeError('face_neighbours: faces must be a tensor')
    _lib.need_cuda(faces)
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('face_neighbours: faces must be integer [F, 3], got %s %s' % (faces.dtype, tuple(faces.shape)))
    F = faces.shape[0]
    if F * 6 + 5 > 0x7fffffff:
        raise ValueError('face_neighbours: %d faces exceed the 32-bit neighbour code' % F)
    f = faces.long()
    good = (f >= 0).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    if num_verts is not None:
        good &= (f < int(num_verts)).all(1)
    p, q = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)                # ends of edge id = f * 3 + k
    ids = torch.arange(3 * F, device=f.device)
    base = (int(f.max()) + 1) if F else 1
    key = torch.where(good.repeat_interleave(3), torch.minimum(p, q) * base + torch.maximum(p, q), -1 - ids)
    key, order = torch.sort(key, stable=True)
    _, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    twice = counts[inverse] == 2
    first = twice.clone()
    first[1:] &= key[1:] != key[:-1]                                               # the first entry of each pair
    a, b = order[first], order[torch.roll(first, 1)]                               # and the second, which follows it
    same = (p[a] == p[b]).long()
    nbr = torch.full((3 * F,), -1, dtype=torch.long, device=f.device)
    nbr[a] = b * 2 + same
    nbr[b] = a * 2 + same
    return nbr.to(torch.int32).reshape(F, 3)


def mirror_fill(rest_verts, faces, textures, weight, axis=0, tol=0.05):
    """Texels with weight == 0 take the texel their mirror image falls on: rest_verts [V,3] is the rest shape (rig.npz of extract.py
    --rig), symmetric about the plane x[axis] = 0; tol is the largest accepted distance between the mirrored sample point and
    the surface as a fraction of the rest bounding-box diagonal.  -> (textures (a copy, filled), source uint8 [F,R*R]: 0 seen,
    1 mirrored, 2 left for blend_fill, info: texels int32 [M], src int32 [M] (g R R + j' or -1 - reason of MIRROR_REASONS), d2
    [M], max_d2)."""
    for name, t in (('rest_verts', rest_verts), ('faces', faces), ('textures', textures), ('weight', weight)):
        if not torch.is_tensor(t):
            raise TypeError('mirror_fill: %s must be a tensor' % name)
    _lib.need_cuda(rest_verts, faces, textures, weight)
    if rest_verts.ndimension() != 2 or rest_verts.shape[1] != 3 or rest_verts.shape[0] < 1:
        raise ValueError('mirror_fill: rest_verts must be [V >= 1, 3], got %s' % (tuple(rest_verts.shape),))
    V = rest_verts.shape[0]
    F, R = _atlas('mirror_fill', faces, textures, weight, 'weight')
    axis, tol = int(axis), float(tol)
    if axis not in (0, 1, 2):
        raise ValueError('mirror_fill: axis must be 0, 1 or 2, got %d' % axis)
    if not 0. <= tol < float('inf'):
        raise ValueError('mirror_fill: tol must be a finite fraction >= 0, got %g' % tol)
    rest = rest_verts.detach().float().contiguous()
    faces32 = faces.to(torch.int32).contiguous()
    textures = textures.detach().float().contiguous()
    weight = weight.detach().float().contiguous()
    unseen = ~(weight > 0)
    texels = torch.nonzero(unseen.reshape(-1)).reshape(-1).to(torch.int32)
    M = int(texels.shape[0])
    diag = float((rest.max(0).values - rest.min(0).values).norm())
    max_d2 = (tol * diag) ** 2
    if not max_d2 < float('inf'):
        raise ValueError('mirror_fill: rest_verts must be finite')
    out = textures.clone()
    src = torch.full((M,), -1 - len(MIRROR_REASONS), dtype=torch.int32, device=rest.device)
    d2 = torch.full((M,), float('inf'), dtype=torch.float32, device=rest.device)
    _lib.call('lasr_bake_mirror', rest, faces32, texels, textures, weight, out, src, d2, V, F, R, M, axis, max_d2, on=rest)
    source = unseen.to(torch.uint8) * BLENDED
    source.view(-1)[texels[src >= 0].long()] = MIRRORED
    return out, source, dict(texels=texels, src=src, d2=d2, max_d2=max_d2)


def blend_fill(textures, source, faces, iters=64):
    """`iters` Jacobi iterations over the texel adjacency (face_neighbours): every texel with source == 2 becomes the mean of its
    edge neighbours, seen and mirrored texels stay fixed.  Ping-pong between two buffers, one launch each (as
    maskprop.meanfield); the input is not written.  -> textures [F,R*R,3]."""
    for name, t in (('textures', textures), ('source', source), ('faces', faces)):
        if not torch.is_tensor(t):
            raise TypeError('blend_fill: %s must be a tensor' % name)
    _lib.need_cuda(textures, source, faces)
    F, R = _atlas('blend_fill', faces, textures, source, 'source')
    iters = int(iters)
    if iters < 0:
        raise ValueError('blend_fill: iters must be >= 0, got %d' % iters)
    cur = textures.detach().float().contiguous()
    if iters == 0 or F == 0:
        return cur.clone()
    fixed = (source != BLENDED).to(torch.uint8).contiguous()
    nbr = face_neighbours(faces).contiguous()
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    for k in range(iters):
        dst = bufs[k & 1]
        _lib.call('lasr_bake_blend', cur, dst, fixed, nbr, F, R)
        cur = dst
    return cur


def complete_texture(faces, textures, weight, fill='mirror', rest_verts=None, axis=0, tol=0.05, iters=64):
    """The atlas of bake_texture completed where weight == 0.  fill 'mirror': mirror_fill over rest_verts, then blend_fill on what
    it left; 'blend': blend_fill alone.  -> (textures, source uint8 [F,R*R]: 0 seen, 1 mirrored, 2 blended, info of mirror_fill or
    None)."""
    if fill not in ('mirror', 'blend'):
        raise ValueError("complete_texture: fill must be 'mirror' or 'blend', got %r" % (fill,))
    info = None
    if fill == 'mirror':
        if rest_verts is None:
            raise ValueError('complete_texture: the mirror fill needs rest_verts (rig.npz of extract.py --rig)')
        textures, source, info = mirror_fill(rest_verts, faces, textures, weight, axis, tol)
    else:
        for name, t in (('faces', faces), ('textures', textures), ('weight', weight)):
            if not torch.is_tensor(t):
                raise TypeError('complete_texture: %s must be a tensor' % name)
        _lib.need_cuda(faces, textures, weight)
        _atlas('complete_texture', faces, textures, weight, 'weight')
        source = (~(weight > 0)).to(torch.uint8) * BLENDED
    return blend_fill(textures, source, faces, iters), source, info


def render_baked(verts, faces, K, textures, H, W, background=(0., 0., 0.)):
    """The baked mesh seen from N cameras: verts [N,V,3] camera space, faces [F,3], K [N,4], textures [F,R*R,3] -> float32
    [N,4,H,W] (rgb, alpha): a hard-mode SoftRenderer with texture_type='surface' rasterises the mesh under the NDC mapping of
    the bake's own raster (face_index_raster), cropped to H x W."""
    from .. import soft_renderer as sr
    _lib.need_cuda(verts, faces, K, textures)
    seq = posed.Posed(verts, faces, K, H, W)
    N = seq.T
    near, far = depth_range(seq.verts)
    renderer = sr.SoftRenderer(image_size=seq.IS, background_color=list(background), near=near, far=far, fill_back=True,
                               sigma_val=1e-12, aggr_func_rgb='hard', dist_func='hard', aggr_func_alpha='hard',
                               texture_type='surface', camera_mode='look_at')
    mesh = sr.Mesh(ndc_vertices(seq.verts, seq.K, seq.IS), seq.faces32[None].expand(N, -1, -1).contiguous(),
                   textures=textures.detach().float()[None].expand(N, -1, -1, -1).contiguous(), texture_type='surface')
    with torch.no_grad():                              # the vertices are in NDC already: the rasteriser stage alone
        out = renderer.rasterizer(mesh)
    return out[:, :, :H, :W]
