"""Visualisation renders of reconstructed meshes (render_vis.py; reference: render_vis.py, which renders with pyrender / OpenGL).

Visibility is the hard-mode rasteriser of soft_renderer (lasr_sr_forward_bg with func_id_rgb = func_id_alpha = 0): one raster per
layer from the camera, one orthographic raster of the whole scene from the light; lasr_vis_shade (csrc/vis.hip) shades and
composites every output pixel from those face-index maps.  DESIGN.md section 4.4 states the shading model and its constants.

Scenes live in camera space with OpenCV axes (x right, y down, z forward); a perspective camera with intrinsics fx fy px py in
pixels of the uncropped H x W frame renders into a square raster of side IS = max(H, W), cropped to H x W.  All frames of one
call share one face list; frames are processed CHUNK_FRAMES at a time, one batched launch of each kind per chunk.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .soft_renderer.functional import surface_normals, vertex_normals

K_AMBIENT = 0.4                   # pyrender scene ambient light 0.4 (render_vis.py:231)
K_DIFFUSE = 1.0                   # diffuse weight of the directional light (this project's own; pyrender's PBR is not matched)
ALBEDO_SCALE = 0.6                # 0.6 * vertex colour (render_vis.py:235); the kernel applies it
SURFACE_ALPHA = 192. / 255.       # alpha of the translucent surface with --vis_bones (render_vis.py:151)
LIGHT_THETA = 7 * math.pi / 9     # render_vis.py:174-175: the light travels along (0, sin t, -cos t) in OpenCV camera axes
LIGHT_DIR = (0.0, math.sin(LIGHT_THETA), -math.cos(LIGHT_THETA))
SHADOW_MAP_SIZE = 1024            # texels per side of the light raster
NEAR, FAR = 1e-3, 1000.           # render_vis.py:273
CHUNK_FRAMES = 8
BASE_COLOR = 102. / 255.          # trimesh's default vertex colour of a mesh without colours


def light_frame():
    """Orthonormal (u, v, d): d = LIGHT_DIR (the direction the light travels), u = x, v = d x u."""
    d = np.asarray(LIGHT_DIR, np.float64)
    u = np.array([1., 0., 0.])
    v = np.cross(d, u)
    return u, v / np.linalg.norm(v), d


def signed_volume(verts, faces):
    """Signed volume of a triangle mesh (verts [V,3], faces [F,3]); positive for outward-facing windings."""
    v = verts.double() if torch.is_tensor(verts) else torch.as_tensor(verts, dtype=torch.float64)
    f = torch.as_tensor(faces, dtype=torch.long, device=v.device)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((p0 * torch.cross(p1, p2, dim=1)).sum() / 6.)


def fix_inversion(verts, faces):
    """Faces with their winding reversed when the mesh's signed volume is negative (stands in for trimesh.repair.fix_inversion)."""
    faces = torch.as_tensor(faces, dtype=torch.long)
    return faces[:, [0, 2, 1]].contiguous() if signed_volume(verts, faces) < 0 else faces


def floor_quad(verts):
    """White floor under a camera-space mesh (verts [V,3]) as render_vis.py:259-264 places the reference's two-triangle
    wood.obj: x over [10 min x, 10 max x], y at the mesh's lowest point (max y, y down), z over [0.5 min z, 10 max z]."""
    v = torch.as_tensor(verts, dtype=torch.float32)
    x0, x1 = 10 * float(v[:, 0].min()), 10 * float(v[:, 0].max())
    z0, z1 = 0.5 * float(v[:, 2].min()), 10 * float(v[:, 2].max())
    y = float(v[:, 1].max())
    fv = torch.tensor([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], dtype=torch.float32)
    ff = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.long)
    return fv, ff, torch.ones(4, 3)


def turntable_camera(i, count=150):
    """[R | T] of turntable frame i (render_vis.py:186-193): rotation about y by -2 pi i / count, 20 units in front."""
    a = -i * 2 * math.pi / count
    R = np.array([[math.cos(a), 0., math.sin(a)], [0., 1., 0.], [-math.sin(a), 0., math.cos(a)]])
    return R, np.array([0., 0., 20.])


def label_colormap(n):
    """First n colours of the PASCAL-VOC label colormap, uint8 [n,3]: bit 3k + c of the label index becomes bit 7 - k of
    channel c."""
    cmap = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        cmap[i] = rgb
    return cmap


def uv_sphere(radius=0.05, rings=16, segments=16):
    """Closed UV sphere: poles on +-z, rings - 1 latitude circles of `segments` vertices.  -> verts [V,3] float64, faces [F,3]."""
    th = np.linspace(0, np.pi, rings + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, segments, endpoint=False)
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.cos(th)[:, None].repeat(segments, 1)], -1).reshape(-1, 3)
    verts = np.concatenate([[[0., 0., 1.]], ring, [[0., 0., -1.]]]) * radius
    last, faces = len(verts) - 1, []
    for s in range(segments):
        t = (s + 1) % segments
        faces.append([0, 1 + s, 1 + t])
        for r in range(rings - 3):
            a, b = 1 + r * segments, 1 + (r + 1) * segments
            faces += [[a + s, b + s, b + t], [a + s, b + t, a + t]]
        a = 1 + (rings - 3) * segments
        faces.append([a + s, last, a + t])
    return verts, np.asarray(faces, np.int64)


def gaussian_spheres(ctl_ts, ctl_rs, log_ctl, Rmat, Tmat):
    """The bones' Gaussian ellipsoids in camera space (nnutils/predictor.py:233-281 of the reference): per bone a uv_sphere()
    divided by exp(0.5 clamp(log_ctl, -2, 2)), rotated by R(ctl_rs) (row vectors times its transpose), moved to ctl_ts, then
    posed as obj_to_cam poses it with an identity skin: each sphere follows its own bone, then the body (written out here, so
    that it runs on any device).  ctl_ts / log_ctl [J,3], ctl_rs
    [J,4] (x, y, z, w), Rmat [J+1,3,3] / Tmat [J+1,3] (body first).  -> verts [J*Vs,3], faces [J*Fs,3], colors uint8 [J*Vs,3]."""
    from .nnutils.mesh_net import quaternion_to_rotation_matrix
    sv, sf = uv_sphere()
    J = ctl_ts.shape[0]
    dev = ctl_ts.device
    s = torch.as_tensor(sv, dtype=torch.float32, device=dev)[None] / torch.exp(0.5 * log_ctl.float().clamp(-2, 2))[:, None]
    R = quaternion_to_rotation_matrix(ctl_rs.float())
    pts = s.matmul(R.transpose(1, 2)) + ctl_ts.float()[:, None]                     # J,Vs,3
    Vs = sv.shape[0]
    Rm, Tm = Rmat.float().reshape(-1, 3, 3), Tmat.float().reshape(-1, 1, 3)
    verts = ((pts.matmul(Rm[1:]) + Tm[1:]).matmul(Rm[0]) + Tm[0]).reshape(-1, 3)
    faces = np.concatenate([sf + k * Vs for k in range(J)])
    colors = np.repeat(label_colormap(J), Vs, 0)
    return verts, faces, colors


def hard_raster(fv, IS, near, far):
    """Hard-mode raster of fv [N,F,3,3] (NDC x, y, depth) -> aggrs_info [N,2,IS,IS] (depth, face index or -1)."""
    N, F = fv.shape[:2]
    dev = fv.device
    tex = torch.zeros(N, F, 1, 3, device=dev)
    aggrs = torch.empty(N, 2, IS, IS, device=dev)
    colors = torch.empty(N, 4, IS, IS, device=dev)
    ws = torch.empty(max(_lib.lib().lasr_sr_workspace_bytes(N, F, 1, IS), 1), dtype=torch.uint8, device=dev)
    bg = (ctypes.c_float * 3)(0., 0., 0.)
    _lib.call('lasr_sr_forward_bg', fv, tex, None, aggrs, colors, ws, ws.numel(), N, F, 1, 3, IS, float(near), float(far), None, 1e-3,
              1e-12, 0, math.log(1. / 1e-4 - 1.), 1e-4, 0, 0, 0, 1, bg, 0)
    return aggrs


def _raster(h, fv, IS, near, far, stream):
    """hard_raster under its earlier signature, for callers that still pass the handle and the current stream."""
    return hard_raster(fv, IS, near, far)


def _face_planes(lv, faces):
    """Light-space plane w = a u + b v + c of every face: lv [N,V,3] (u, v, w), faces [F,3] -> [N,F,3]."""
    p = lv[:, faces]                                                            # N,F,3,3
    n = torch.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0], dim=2)
    nn = n.norm(dim=2)
    ok = n[..., 2].abs() > 1e-3 * nn                                            # faces seen edge-on from the light: flat plane
    nw = torch.where(ok, n[..., 2], torch.ones_like(nn))
    a = torch.where(ok, -n[..., 0] / nw, torch.zeros_like(nn))
    b = torch.where(ok, -n[..., 1] / nw, torch.zeros_like(nn))
    p0 = p[:, :, 0]
    c = torch.where(ok, p0[..., 2] - a * p0[..., 0] - b * p0[..., 1], p[..., 2].mean(2))
    return torch.stack([a, b, c], 2)


def shade(verts, faces, colors, K, IS, H, W, n_opaque=None, casters=None, smooth=True, background=(1., 1., 1.), frames=None,
          return_maps=False):
    """Render N frames of one scene layout.

    verts [N,V,3] camera space, faces [F,3] (shared), colors [N,V,3] or [V,3] in 0-1, K [N,4] = fx fy px py (pixels).
    Faces [0, n_opaque) are the opaque layer, the rest the translucent surface (n_opaque None or F: one opaque layer).
    casters: bool [V], the vertices the shadow map must cover (default all; the floor need not be).  frames [N,H,W,3] uint8:
    blended with the render (--overlay).  -> uint8 [N,H,W,3] on the device, and with return_maps the kernel's inputs too.
    """
    dev = verts.device
    N, V = verts.shape[:2]
    faces = torch.as_tensor(faces, dtype=torch.long, device=dev)
    F = faces.shape[0]
    F0 = F if n_opaque is None else int(n_opaque)
    if not (0 < F0 <= F) or faces.numel() == 0 or int(faces.min()) < 0 or int(faces.max()) >= V:
        raise ValueError('shade: faces must index the %d vertices, and the opaque layer must hold 1..%d faces' % (V, F))
    if not (1 <= H <= IS and 1 <= W <= IS):
        raise ValueError('shade: the H x W crop must fit the IS x IS raster')
    verts = verts.float().contiguous()
    colors = torch.as_tensor(colors, dtype=torch.float32, device=dev).expand(N, V, 3)
    K = torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(N, 4)
    x, y, z = verts.unbind(2)
    sx = 2 * (K[:, 0:1] * x / z + K[:, 2:3]) / IS - 1                         # u = fx x / z + px -> NDC of the square raster
    sy = 1 - 2 * (K[:, 1:2] * y / z + K[:, 3:4]) / IS                         # v down, NDC y up: row 0 is the top
    fb = faces[None].expand(N, F, 3)
    vn = vertex_normals(verts, fb)
    fn = surface_normals(verts[:, faces])
    vert_rec = torch.stack([x, y, z, sx, vn[..., 0], vn[..., 1], vn[..., 2], sy,
                            colors[..., 0], colors[..., 1], colors[..., 2], torch.zeros_like(x)], 2).contiguous()
    # light space: orthographic along LIGHT_DIR; the map covers the casters' extent
    u, v, d = (torch.tensor(a, dtype=torch.float32, device=dev) for a in light_frame())
    lv = torch.stack([verts @ u, verts @ v, verts @ d], 2)                      # N,V,3
    cl = lv if casters is None else lv[:, torch.as_tensor(casters, dtype=torch.bool, device=dev)]
    lo, hi = cl.amin(1), cl.amax(1)                                              # N,3
    half = (hi[:, :2] - lo[:, :2]).amax(1) * 0.525 + 1e-6
    ctr = (hi[:, :2] + lo[:, :2]) / 2
    shadow_xf = torch.stack([ctr[:, 0], ctr[:, 1], 1 / half, torch.zeros_like(half)], 1).contiguous()
    wlo, whi = lv[..., 2].amin(1), lv[..., 2].amax(1)
    rng = (whi - wlo).clamp_min(1e-6)
    off = 1000 * rng                                                             # 1/z interpolation of the raster stays ordered
    planes = _face_planes(lv, faces)
    face_rec = torch.cat([fn, torch.zeros_like(fn[..., :1]), planes, torch.zeros_like(fn[..., :1])], 2).contiguous()
    faces4 = torch.cat([faces, torch.zeros_like(faces[:, :1])], 1).int().contiguous()
    params = _lib.VisParams()
    params.light_u[:], params.light_v[:], params.light_d[:] = (list(map(float, a.tolist())) for a in (u, v, d))
    params.k_ambient, params.k_diffuse, params.surface_alpha = K_AMBIENT, K_DIFFUSE, SURFACE_ALPHA
    params.shadow_bias = 0.
    params.background[:] = [float(c) for c in background]
    params.smooth, params.overlay = int(bool(smooth)), int(frames is not None)

    out = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    packed = None
    if frames is not None:
        fr = torch.as_tensor(frames, device=dev).to(torch.uint8)
        packed = torch.cat([fr, torch.full_like(fr[..., :1], 255)], 3).contiguous().view(torch.int32).reshape(N, H, W)
    maps = {}
    with torch.cuda.device(dev):
        cam = torch.stack([sx, sy, z], 2)[:, faces].contiguous()                # N,F,3,3
        raster0 = hard_raster(cam[:, :F0].contiguous(), IS, NEAR, FAR)
        raster1 = hard_raster(cam[:, F0:].contiguous(), IS, NEAR, FAR) if F0 < F else None
        lnd = torch.stack([(lv[..., 0] - ctr[:, :1]) / half[:, None], (lv[..., 1] - ctr[:, 1:]) / half[:, None],
                           lv[..., 2] - wlo[:, None] + off[:, None]], 2)[:, faces].contiguous()
        # one light raster for the whole chunk: near / far around every frame's offset depth range
        shadow = hard_raster(lnd, SHADOW_MAP_SIZE, float(off.min()) * 0.5, float((off + 2 * rng).max()))
        params.shadow_bias = float(rng.max()) * 1e-5
        _lib.call('lasr_vis_shade', vert_rec, faces4, face_rec, raster0, raster1, shadow, shadow_xf, packed, out, N, V, F, F0, IS,
                  SHADOW_MAP_SIZE, H, W, ctypes.byref(params))
    rgb = out.view(torch.uint8).reshape(N, H, W, 4)[..., :3]
    if return_maps:
        maps = dict(vert_rec=vert_rec, faces=faces4, face_rec=face_rec, raster0=raster0, raster1=raster1, shadow=shadow,
                    shadow_xf=shadow_xf, frames=packed, params=params, F0=F0, IS=IS, S=SHADOW_MAP_SIZE)
        return rgb, maps
    return rgb


def render_chunks(scenes, IS, H, W, smooth=True, overlay=False, frames=None, device='cuda'):
    """scenes: list of dicts per frame with 'verts' [V,3] (camera space), 'faces' [F,3], 'colors' [V,3] (0-1), 'K' (fx, fy, px,
    py), 'n_opaque' (faces of the opaque layer, first) and 'casters' (bool [V]).  Consecutive frames with the same face list go
    through shade() CHUNK_FRAMES at a time.  frames: list of uint8 [H,W,3] for the overlay.  Yields uint8 [n, H, W, 3] on the
    device per chunk, in order, so that a caller can move each chunk off the device before the next is rendered."""
    i = 0
    bg = (0., 0., 0.) if overlay else (1., 1., 1.)
    while i < len(scenes):
        j = i + 1
        while (j < len(scenes) and j - i < CHUNK_FRAMES and scenes[j]['n_opaque'] == scenes[i]['n_opaque']
               and scenes[j]['faces'].shape == scenes[i]['faces'].shape and torch.equal(scenes[j]['faces'], scenes[i]['faces'])):
            j += 1
        chunk = scenes[i:j]
        verts = torch.stack([torch.as_tensor(s['verts'], dtype=torch.float32) for s in chunk]).to(device)
        colors = torch.stack([torch.as_tensor(s['colors'], dtype=torch.float32) for s in chunk]).to(device)
        K = torch.tensor([list(s['K']) for s in chunk], dtype=torch.float32, device=device)
        fr = None
        if overlay:
            fr = torch.stack([torch.as_tensor(np.ascontiguousarray(f)) for f in frames[i:j]]).to(device)
        yield shade(verts, chunk[0]['faces'].to(device), colors, K, IS, H, W, n_opaque=chunk[0]['n_opaque'],
                    casters=chunk[0]['casters'], smooth=smooth, background=bg, frames=fr)
        i = j


def render_sequence(scenes, IS, H, W, smooth=True, overlay=False, frames=None, device='cuda'):
    """render_chunks() concatenated: uint8 [len(scenes), H, W, 3] on the device."""
    return torch.cat(list(render_chunks(scenes, IS, H, W, smooth, overlay, frames, device)), 0)
