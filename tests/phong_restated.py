"""Float64 numpy restatement of lasr_phong_shade (lasr_amd/csrc/phong.hip): pytorch3d 0.4.0's
phong_shading + softmax_rgb_blend for OrthographicCameras(), white PointLights() at (0, 1, 0), shininess 64, sigma = gamma = 1e-4,
znear = 1, zfar = 100, one face per pixel, fed a face-index map (the hard raster's)."""
import numpy as np

SIGMA = GAMMA = 1e-4
ZNEAR, ZFAR, BLEND_EPS = 1., 100., 1e-10
K_EPS = 1e-8
LIGHT = np.array([0., 1., 0.])


def pixel_ndc(S):
    """(x [S,S], y [S,S]) pytorch3d NDC of the pixel centres: +X left, +Y up, row 0 on top."""
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    return 1. - (2. * c + 1.) / S, 1. - (2. * r + 1.) / S


def vertex_normals(verts, faces):
    """Area-weighted unit vertex normals (pytorch3d's Meshes.verts_normals_packed; eps 1e-6)."""
    v = np.asarray(verts, np.float64)
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    acc = np.zeros_like(v)
    np.add.at(acc, faces[:, 1], np.cross(p2 - p1, p0 - p1))
    np.add.at(acc, faces[:, 2], np.cross(p0 - p2, p1 - p2))
    np.add.at(acc, faces[:, 0], np.cross(p1 - p0, p2 - p0))
    return acc / np.maximum(np.linalg.norm(acc, axis=1, keepdims=True), 1e-6)


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-6)


def _edge(px, py, a, b):
    return (px - a[..., 0]) * (b[..., 1] - a[..., 1]) - (py - a[..., 1]) * (b[..., 0] - a[..., 0])


def _seg_d2(px, py, a, b):
    e = b - a
    l2 = (e ** 2).sum(-1)
    safe = np.where(l2 <= K_EPS, 1., l2)
    t = np.clip((e[..., 0] * (px - a[..., 0]) + e[..., 1] * (py - a[..., 1])) / safe, 0., 1.)
    dx, dy = a[..., 0] + t * e[..., 0] - px, a[..., 1] + t * e[..., 1] - py
    deg = (px - b[..., 0]) ** 2 + (py - b[..., 1]) ** 2
    return np.where(l2 <= K_EPS, deg, dx * dx + dy * dy)


def phong_colour(p, n, texel):
    """(1 + relu(n.l)) texel + [n.l > 0] relu(v.(2 (n.l) n - l))^64 at points p [...,3] with normals n, texels [...,3]."""
    n = _normalize(n)
    l = _normalize(LIGHT - p)
    v = _normalize(-p)
    ndl = (n * l).sum(-1)
    refl = 2. * ndl[..., None] * n - l
    spec = np.maximum((v * refl).sum(-1), 0.) ** 64 * (ndl > 0)
    return (1. + np.maximum(ndl, 0.))[..., None] * texel + spec[..., None]


def blend(colour, d2, z, background):
    """softmax_rgb_blend of one face per pixel: -> rgb [...,3], alpha [...]."""
    prob = 1. / (1. + np.exp(-d2 / SIGMA))
    z_inv = (ZFAR - z) / (ZFAR - ZNEAR)
    m = np.maximum(z_inv, BLEND_EPS)
    w = prob * np.exp((z_inv - m) / GAMMA)
    delta = np.maximum(np.exp((BLEND_EPS - m) / GAMMA), BLEND_EPS)
    bg = np.asarray(background, np.float64)
    rgb = (w[..., None] * colour + delta[..., None] * bg) / (w + delta)[..., None]
    return rgb, prob


def shade(verts, faces, colors, face_map, background=(1., 1., 1.)):
    """verts [V,3], faces [F,3], colors [V,3], face_map [S,S] (face index or -1, row 0 on top) -> RGBA float64 [S,S,4]."""
    verts = np.asarray(verts, np.float64)
    colors = np.asarray(colors, np.float64)
    faces = np.asarray(faces, np.int64)
    S = face_map.shape[0]
    out = np.zeros((S, S, 4))
    out[..., :3] = np.asarray(background, np.float64)
    f = np.asarray(face_map).astype(np.int64)
    cov = (f >= 0) & (f < len(faces))
    if not cov.any():
        return out
    xs, ys = pixel_ndc(S)
    px, py = xs[cov], ys[cov]
    tri = faces[f[cov]]
    vn = vertex_normals(verts, faces)
    a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    area = _edge(c[:, 0], c[:, 1], a, b) + K_EPS
    w0 = _edge(px, py, b, c) / area
    w1 = _edge(px, py, c, a) / area
    w2 = _edge(px, py, a, b) / area
    W = np.stack([w0, w1, w2], 1)[..., None]
    p = (W * np.stack([a, b, c], 1)).sum(1)
    n = (W * vn[tri]).sum(1)
    t = (W * colors[tri]).sum(1)
    col = phong_colour(p, n, t)
    a2, b2, c2 = a[:, :2], b[:, :2], c[:, :2]
    d2 = np.minimum(np.minimum(_seg_d2(px, py, a2, b2), _seg_d2(px, py, b2, c2)), _seg_d2(px, py, c2, a2))
    rgb, alpha = blend(col, d2, p[:, 2], background)
    out[cov, :3] = rgb
    out[cov, 3] = alpha
    return out
