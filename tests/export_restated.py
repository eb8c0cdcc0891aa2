"""numpy restatement of the reference's export-side kernels, the yardstick of csrc/export.hip (tests only).

Written from the definitions in third_party/softras/soft_renderer (functional/voxelization.py, functional/save_obj.py,
cuda/voxelization_cuda_kernel.cu, cuda/create_texture_image_cuda_kernel.cu): the same expressions in the same order, each numpy
operation rounding once in the input's dtype (float32 or float64), so no operation is fused.
"""
import numpy as np
from scipy import ndimage


def _columns(lo, hi, S):
    """For each face the integer columns [lo, hi] clipped to [0, S-1] (lo/hi float arrays) -> (face index, column) pairs."""
    lo = np.clip(lo, 0, S - 1).astype(np.int64)
    hi = np.clip(hi, -1, S - 1).astype(np.int64)
    return lo, np.maximum(hi - lo + 1, 0)


def _sub1(faces, S, perm, margin):
    """voxelize_sub1 on the coordinates permuted by `perm` (= (Y, X, Z)), over every column (y, x) of each face's bounding box
    widened by `margin` (margin=None: every column of the grid, as the reference).  Returns occupied (y, x, z) triples."""
    T = faces.dtype.type
    Y, X, Z = (faces[:, :, perm[i]] for i in range(3))                     # [F, 3] each
    F = faces.shape[0]
    if margin is None:
        ylo = np.zeros(F); yhi = np.full(F, S - 1.); xlo = np.zeros(F); xhi = np.full(F, S - 1.)
    else:
        ylo, yhi = np.floor(Y.min(1)) - margin, np.ceil(Y.max(1)) + margin
        xlo, xhi = np.floor(X.min(1)) - margin, np.ceil(X.max(1)) + margin
    y0, ny = _columns(ylo, yhi, S)
    x0, nx = _columns(xlo, xhi, S)
    cnt = ny * nx
    fi = np.repeat(np.arange(F), cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    y = y0[fi] + k // nx[fi]
    x = x0[fi] + k % nx[fi]
    Yf, Xf, Zf = Y[fi], X[fi], Z[fi]
    y1d = Yf[:, 1] - Yf[:, 0]; x1d = Xf[:, 1] - Xf[:, 0]; z1d = Zf[:, 1] - Zf[:, 0]
    y2d = Yf[:, 2] - Yf[:, 0]; x2d = Xf[:, 2] - Xf[:, 0]; z2d = Zf[:, 2] - Zf[:, 0]
    ypd = y.astype(T) - Yf[:, 0]
    xpd = x.astype(T) - Xf[:, 0]
    det = x1d * y2d - x2d * y1d
    with np.errstate(divide='ignore', invalid='ignore'):
        t1 = (y2d * xpd - x2d * ypd) / det
        t2 = (-y1d * xpd + x1d * ypd) / det
        zf = np.floor(t1 * z1d + t2 * z2d + Zf[:, 0])
        ok = (det != 0) & ~(t1 < 0) & ~(t2 < 0) & ~(1 < t1 + t2) & (zf >= 0) & (zf < S)
    y, x, z = y[ok], x[ok], zf[ok].astype(np.int64)
    out = []
    for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1)):
        yi, xi = y - dy, x - dx
        m = (yi >= 0) & (xi >= 0)
        out.append((yi[m], xi[m], z[m]))
    return [np.concatenate(c) for c in zip(*out)]


def surface(faces, S, margin=2):
    """Occupancy before the fill: the union of voxelize_sub1 along the three axes (voxelization.py:9-17; the permutation
    [2,1,0] / [0,2,1] / none followed by the transpose back) and voxelize_sub2.  faces [F,3,3] in voxel units -> bool [S,S,S].
    margin: see _sub1 (the kernel widens by 1; a wider margin here would reveal a column it skipped)."""
    occ = np.zeros((S, S, S), bool)
    for perm, back in (((2, 1, 0), lambda y, x, z: (z, x, y)), ((0, 2, 1), lambda y, x, z: (y, z, x)),
                       ((0, 1, 2), lambda y, x, z: (y, x, z))):
        y, x, z = _sub1(faces, S, perm, margin)
        occ[back(y, x, z)] = True
    v = np.floor(faces.reshape(-1, 3))
    m = np.all((v >= 0) & (v < S), axis=1)
    v = v[m].astype(np.int64)
    occ[v[:, 0], v[:, 1], v[:, 2]] = True
    return occ


def fill(occ):
    """voxelize_sub3 + voxelize_sub4 to the fixed point: empty voxels 6-connected through empty voxels to an empty boundary
    voxel are visible; returns 1 - visible as int32."""
    lab, _ = ndimage.label(~occ)                     # default structure in 3-D: 6-connectivity
    border = np.unique(np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(),
                                       lab[:, :, 0].ravel(), lab[:, :, -1].ravel()]))
    visible = np.isin(lab, border[border > 0])
    return (1 - visible).astype(np.int32)


def fill_sweeps(occ):
    """The same fixed point the reference's way (sub3, then sub4 sweeps until nothing changes; Jacobi sweeps here, which reach
    the same unique fixed point): a cross-check of fill() for small grids."""
    empty = ~occ
    vis = np.zeros_like(occ)
    b = np.zeros_like(occ)
    b[0] = b[-1] = True; b[:, 0] = b[:, -1] = True; b[:, :, 0] = b[:, :, -1] = True
    vis[b & empty] = True
    while True:
        n = vis.copy()
        n[1:] |= vis[:-1]; n[:-1] |= vis[1:]
        n[:, 1:] |= vis[:, :-1]; n[:, :-1] |= vis[:, 1:]
        n[:, :, 1:] |= vis[:, :, :-1]; n[:, :, :-1] |= vis[:, :, 1:]
        n &= empty
        n |= vis
        if (n == vis).all():
            break
        vis = n
    return (1 - vis).astype(np.int32)


def voxelization(faces, size, normalize=False, margin=2):
    """srf.voxelization: faces [B,F,3,3] (float32 / float64 numpy) -> [B,S,S,S] int32."""
    faces = faces.copy()
    if not normalize:
        faces *= faces.dtype.type(size)
    return np.stack([fill(surface(f, size, margin)) for f in faces])


def atlas_layout(num_faces, texture_res, dtype=np.float32):
    """The tile layout of create_texture_image (integer tile rows): (tile_width, tile_height, corners [F,3,2] in pixels)."""
    tile_width = int((num_faces - 1.) ** 0.5) + 1
    tile_height = int((num_faces - 1.) / tile_width) + 1
    fn = np.arange(num_faces)
    c, r = fn % tile_width, fn // tile_width
    R = texture_res
    v = np.zeros((num_faces, 3, 2), dtype)
    v[:, 0] = np.stack([c * R + R / 2, r * R + 1], 1)
    v[:, 1] = np.stack([c * R + 1, (r + 1) * R - 2], 1)
    v[:, 2] = np.stack([(c + 1) * R - 2, (r + 1) * R - 2], 1)
    return tile_width, tile_height, v


def texture_image(textures, texture_res=16):
    """create_texture_image (save_obj.py:9-37 with the kernel create_texture_image_cuda_kernel.cu:10-61): textures [F,R*R,3] ->
    (image [H,W,3] with v = 0 the bottom row, vt [F,3,2])."""
    T = textures.dtype.type
    F = textures.shape[0]
    R = int(round(textures.shape[1] ** 0.5))
    tw, th, v = atlas_layout(F, texture_res, textures.dtype)
    H, W = th * texture_res, tw * texture_res
    image = np.ones((H, W, 3), textures.dtype)
    y, x = np.divmod(np.arange(H * W), W)
    fn = x // texture_res + (y // texture_res) * tw
    m = fn < F
    y, x, fn = y[m], x[m], fn[m]
    eps = T(np.float32(1e-5))                       # the reference passes eps as a C float
    p = v[fn]
    p0x, p0y, p1x, p1y, p2x, p2y = p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 0], p[:, 2, 1]
    fi = [p1y - p2y, p2x - p1x, p1x * p2y - p2x * p1y,
          p2y - p0y, p0x - p2x, p2x * p0y - p0x * p2y,
          p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y]
    den = p2x * (p0y - p1y) + p0x * (p1y - p2y) + p1x * (p2y - p0y)
    fi = [a / (den + eps) for a in fi]
    xf, yf = x.astype(T), y.astype(T)
    w, w_sum = [], T(0)
    for k in range(3):
        wk = fi[3 * k] * xf + fi[3 * k + 1] * yf + fi[3 * k + 2]
        wk = np.fmax(np.fmin(wk, T(1)), T(0))
        w.append(wk)
        w_sum = w_sum + wk
    w = [wk / (w_sum + eps) for wk in w]
    w_x = (w[0] * T(R)).astype(np.int64)
    w_y = (w[1] * T(R)).astype(np.int64)
    lower = (w[0] + w[1]) * T(R) - w_x.astype(T) - w_y.astype(T) <= 1
    t = np.where(lower, w_y * R + w_x, (R - 1 - w_y) * R + (R - 1 - w_x))
    image[y, x] = textures[fn, t]
    vt = v.copy()
    vt[:, :, 0] /= textures.dtype.type(W - 1)
    vt[:, :, 1] /= textures.dtype.type(H - 1)
    return image[::-1], vt
