"""float64 numpy restatement of the texture bake (include/lasr_ops.h: lasr_bake_accumulate / lasr_bake_resolve) and
the fixtures tests/test_bake_cpu.py and tests/test_bake_gpu.py share.  The bake is this project's own addition, so this file is
what the kernel is checked against; it takes the raster's face-index plane as an input and flags the texels whose discrete choices
(nearest pixel, mask taps) sit within UNDECIDED_PX of a boundary, where float32 and float64 may legitimately differ."""
import numpy as np

UNDECIDED_PX = 1e-4          # 13 float32 ulps at coordinate 64
SEED = 7                     # of the icosphere fixture's frames (test_bake_cpu.py checks the undecided share it gives)


def surface_texel(c0, c1, R):
    """numpy copy of sr_device.h: surface_texel."""
    ix, iy = int(c0 * R), int(c1 * R)
    if (c0 + c1) * R - ix - iy <= 1:
        return iy * R + ix
    return (R - 1 - iy) * R + (R - 1 - ix)


def centroids(R):
    """(c0, c1, c2) [R*R] each: barycentric centroid of the region surface_texel maps to texel j = iy R + ix."""
    j = np.arange(R * R)
    iy, ix = j // R, j % R
    low = ix + iy <= R - 1
    c0 = np.where(low, (ix + 1. / 3.) / R, (R - 1 - ix + 2. / 3.) / R)
    c1 = np.where(low, (iy + 1. / 3.) / R, (R - 1 - iy + 2. / 3.) / R)
    return c0, c1, 1. - c0 - c1


def project(verts, faces, K, R):
    """Texel sample points of every frame: verts [T,V,3], faces [F,3], K [T,4] -> P [T,F,R*R,3], u, v [T,F,R*R]."""
    verts, K = np.asarray(verts, np.float64), np.asarray(K, np.float64)
    c0, c1, c2 = centroids(R)
    tri = verts[:, np.asarray(faces)]                                              # T,F,3,3
    P = (c0[None, None, :, None] * tri[:, :, None, 0] + c1[None, None, :, None] * tri[:, :, None, 1]
         + c2[None, None, :, None] * tri[:, :, None, 2])
    z = np.where(P[..., 2] > 0, P[..., 2], 1.)
    u = K[:, 0, None, None] * P[..., 0] / z + K[:, 2, None, None]
    v = K[:, 1, None, None] * P[..., 1] / z + K[:, 3, None, None]
    return P, u, v


def _near(x, offset):
    y = x - offset
    return np.abs(y - np.round(y)) < UNDECIDED_PX


def bake(verts, faces, K, face_index, frames, masks=None, R=8, power=2, fallback=None):
    """face_index [T, >=H, >=W]: the hard raster's plane 1 (row 0 on top).  -> textures [F,R*R,3], weight [F,R*R],
    undecided bool [F,R*R]."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces)
    frames = np.asarray(frames)
    T, H, W = frames.shape[:3]
    F, RR = faces.shape[0], R * R
    P, u, v = project(verts, faces, K, R)
    tri = verts[:, faces]
    n = np.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    n = n / np.linalg.norm(n, axis=2, keepdims=True)
    acc = np.zeros((F, RR, 4))
    undecided = np.zeros((F, RR), bool)
    fid = np.arange(F)[:, None]
    for t in range(T):
        ok = (P[t, ..., 2] > 0) & (u[t] >= 0) & (u[t] < W) & (v[t] >= 0) & (v[t] < H)
        near = _near(u[t], 0.) | _near(v[t], 0.)
        if masks is not None:
            near |= _near(u[t], 0.5) | _near(v[t], 0.5)
        undecided |= ok & near
        col = np.clip(np.floor(u[t]).astype(int), 0, W - 1)
        row = np.clip(np.floor(v[t]).astype(int), 0, H - 1)
        ok &= face_index[t][row, col] == fid
        su, sv = u[t] - 0.5, v[t] - 0.5
        fu, fv = np.floor(su), np.floor(sv)
        tx, ty = su - fu, sv - fv
        x0, x1 = np.clip(fu.astype(int), 0, W - 1), np.clip(fu.astype(int) + 1, 0, W - 1)
        y0, y1 = np.clip(fv.astype(int), 0, H - 1), np.clip(fv.astype(int) + 1, 0, H - 1)
        if masks is not None:
            m = np.asarray(masks[t]) > 0
            ok &= m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]
        img = frames[t].astype(np.float64) / 255.
        rgb = (((1 - tx) * (1 - ty))[..., None] * img[y0, x0] + (tx * (1 - ty))[..., None] * img[y0, x1]
               + ((1 - tx) * ty)[..., None] * img[y1, x0] + (tx * ty)[..., None] * img[y1, x1])
        d = P[t] / np.linalg.norm(P[t], axis=2, keepdims=True)
        cs = np.abs((n[t][:, None, :] * d).sum(2))
        w = np.ones_like(cs)
        for _ in range(int(power)):
            w = w * cs
        w = np.where(ok, w, 0.)
        acc[..., :3] += w[..., None] * rgb
        acc[..., 3] += w
    c0, c1, c2 = centroids(R)
    if fallback is None:
        fb = np.full((F, RR, 3), 0.5)
    else:
        fc = np.asarray(fallback, np.float64)[faces]                              # F,3,3
        fb = c0[None, :, None] * fc[:, None, 0] + c1[None, :, None] * fc[:, None, 1] + c2[None, :, None] * fc[:, None, 2]
    seen = acc[..., 3] > 0
    tex = np.where(seen[..., None], acc[..., :3] / np.where(seen, acc[..., 3], 1.)[..., None], fb)
    return tex, acc[..., 3], undecided


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
H, W, IS = 48, 64, 64


def numpy_face_index(verts, faces, K, size=IS):
    """A hand-made face-index plane [T,size,size]: nearest face (by interpolated 1/z) covering each pixel centre, -1 elsewhere."""
    verts, K = np.asarray(verts, np.float64), np.asarray(K, np.float64)
    T = verts.shape[0]
    out = -np.ones((T, size, size))
    yy, xx = np.mgrid[:size, :size] + 0.5
    for t in range(T):
        u = K[t, 0] * verts[t, :, 0] / verts[t, :, 2] + K[t, 2]
        v = K[t, 1] * verts[t, :, 1] / verts[t, :, 2] + K[t, 3]
        best = np.zeros((size, size))
        for f, (a, b, c) in enumerate(np.asarray(faces)):
            den = (u[b] - u[a]) * (v[c] - v[a]) - (u[c] - u[a]) * (v[b] - v[a])
            if den == 0:
                continue
            w0 = ((u[b] - xx) * (v[c] - yy) - (u[c] - xx) * (v[b] - yy)) / den
            w1 = ((u[c] - xx) * (v[a] - yy) - (u[a] - xx) * (v[c] - yy)) / den
            w2 = 1 - w0 - w1
            iz = w0 / verts[t, a, 2] + w1 / verts[t, b, 2] + w2 / verts[t, c, 2]
            hit = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (iz > best)
            best[hit], out[t][hit] = iz[hit], f
    return out


def smooth_frames(T, seed, h=H, w=W):
    """Low-pass noise as uint8 [T,h,w,3]: a coarse random grid, bilinearly enlarged."""
    rng = np.random.default_rng(seed)
    gh, gw = h // 8 + 2, w // 8 + 2
    grid = rng.uniform(0.1, 0.9, (T, gh, gw, 3))
    y, x = (np.arange(h) + 0.5) / 8., (np.arange(w) + 0.5) / 8.
    y0, x0 = y.astype(int), x.astype(int)
    ty, tx = (y - y0)[None, :, None, None], (x - x0)[None, None, :, None]
    g = lambda a, b: grid[:, a][:, :, b]                                            # noqa: E731
    img = (1 - ty) * ((1 - tx) * g(y0, x0) + tx * g(y0, x0 + 1)) + ty * ((1 - tx) * g(y0 + 1, x0) + tx * g(y0 + 1, x0 + 1))
    return np.round(img * 255).astype(np.uint8)


def max_gradient(frames):
    """Largest difference between adjacent pixels, 0-1 units."""
    f = np.asarray(frames).astype(np.float64) / 255.
    return max(np.abs(np.diff(f, axis=1)).max(), np.abs(np.diff(f, axis=2)).max())


def icosphere_case(T=4, seed=SEED):
    """Icosphere subdivided once (42 vertices, 80 faces) seen by T cameras a quarter turn apart, 48 x 64 frames of smooth noise,
    silhouette masks from the hand-made raster.  verts float32 [T,42,3], faces int64 [80,3], K float32 [T,4], frames, masks."""
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(2)
    assert v.shape == (42, 3) and f.shape == (80, 3)
    tilt = np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    verts = []
    for t in range(T):
        a = 0.2 + t * np.pi / 2
        yaw = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        verts.append(v.astype(np.float64) @ (tilt @ yaw).T + np.array([0.03, -0.02, 4.]))
    verts = np.stack(verts).astype(np.float32)
    K = np.tile(np.array([[75., 73., 32.3, 24.2]], np.float32), (T, 1))
    frames = smooth_frames(T, seed)
    masks = (numpy_face_index(verts, f, K)[:, :H, :W] >= 0).astype(np.uint8) * 128
    return verts, f, K, frames, masks


def ramp_image(a, b, c, h=H, w=W):
    """uint8-exact affine image I(r, col) = a (col + 0.5) + b (r + 0.5) + c in 0..255, the same in the three channels + (0, 1, 2)."""
    r, col = np.mgrid[:h, :w]
    img = a * (col + 0.5) + b * (r + 0.5) + c
    out = np.stack([img, img + 1, img + 2], -1)
    assert np.all(out == np.round(out)) and out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
