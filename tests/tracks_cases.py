"""Case generators shared by tests/test_tracks_cpu.py and tests/test_tracks_gpu.py: a few frames of 64 x 48 pixels (48 rows, 64
columns; px != py, fx != fy, so a row / column or H / W swap shows), meshes of at most 320 faces, and a hand-made face-index raster
for the suite that has no device."""
import numpy as np

H, W, IS = 48, 64, 64
SEED = 11                    # of the parity case's sub-pixel queries (test_tracks_cpu.py checks the undecided share it gives)


def face_index(verts, faces, K, h=H, w=W):
    """Hand-made face-index planes [T,h,w]: of the faces whose projection holds the pixel centre, the nearest by interpolated 1/z;
    -1 where there is none."""
    verts, K, faces = np.asarray(verts, np.float64), np.asarray(K, np.float64), np.asarray(faces)
    T = verts.shape[0]
    out = -np.ones((T, h, w))
    y, x = np.mgrid[:h, :w] + 0.5
    for t in range(T):
        z = verts[t, :, 2]
        u = K[t, 0] * verts[t, :, 0] / z + K[t, 2]
        v = K[t, 1] * verts[t, :, 1] / z + K[t, 3]
        nearest = np.zeros((h, w))
        for f, (a, b, c) in enumerate(faces):
            area = (u[b] - u[a]) * (v[c] - v[a]) - (u[c] - u[a]) * (v[b] - v[a])
            if area == 0:
                continue
            wa = ((u[b] - x) * (v[c] - y) - (u[c] - x) * (v[b] - y)) / area
            wb = ((u[c] - x) * (v[a] - y) - (u[a] - x) * (v[c] - y)) / area
            wc = 1. - wa - wb
            inv = wa / z[a] + wb / z[b] + wc / z[c]
            take = (wa >= 0) & (wb >= 0) & (wc >= 0) & (inv > nearest)
            nearest[take] = inv[take]
            out[t][take] = f
    return out


def pad(planes, size=IS):
    """[T,h,w] -> [T,size,size] with -1 outside, the shape the device raster has."""
    T, h, w = planes.shape
    out = -np.ones((T, size, size))
    out[:, :h, :w] = planes
    return out


def centres(mask, t):
    """Pixel-centre queries (t, row + 0.5, col + 0.5) of the True pixels of mask [h,w], row-major."""
    r, c = np.nonzero(mask)
    return np.stack([np.full(r.shape, float(t)), r + 0.5, c + 0.5], 1)


# ---- 1 / 7: a fronto-parallel quad that translates ------------------------------------------------------------------------------------
QUAD_K = np.array([60., 58., 31.7, 23.3])
QUAD_Z0 = 2.
QUAD_HALF = (0.6, 0.45)
QUAD_STEP = np.array([0.35, 0.1, 0.15])
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]])


def quad_case(T=4):
    """Two triangles at depth QUAD_Z0 moved by QUAD_STEP a frame: columns 13.7 .. 49.7, rows 10.25 .. 36.35 in frame 0; by frame 3
    the right-hand part has left the 64-pixel-wide frame.  -> verts float32 [T,4,3], faces, K float32 [T,4]."""
    hx, hy = QUAD_HALF
    base = np.array([[-hx, -hy, QUAD_Z0], [hx, -hy, QUAD_Z0], [hx, hy, QUAD_Z0], [-hx, hy, QUAD_Z0]])
    verts = np.stack([base + t * QUAD_STEP for t in range(T)]).astype(np.float32)
    return verts, QUAD_FACES, np.tile(QUAD_K.astype(np.float32), (T, 1))


def quad_queries():
    """Pixel centres on a 3-pixel grid inside the quad of frame 0, and the same shifted by sub-pixel offsets.  Pixels within 1.5
    pixels of the diagonal the two triangles share are left out: a shifted query may cross it, and is then clamped onto the face
    that owns the pixel centre (by design), which the closed form of a plane does not know about."""
    r, c = np.mgrid[12:35:3, 15:48:3]
    q = np.stack([np.zeros(r.size), r.ravel() + 0.5, c.ravel() + 0.5], 1)
    fx, fy, px, py = QUAD_K
    a = np.array([px - fx * QUAD_HALF[0] / QUAD_Z0, py - fy * QUAD_HALF[1] / QUAD_Z0])      # corner 0 -> corner 2, (u, v)
    d = np.array([fx * QUAD_HALF[0], fy * QUAD_HALF[1]]) * 2 / QUAD_Z0
    dist = np.abs((q[:, 2] - a[0]) * d[1] - (q[:, 1] - a[1]) * d[0]) / np.hypot(*d)
    q = q[dist > 1.5]
    off = np.array([[0., 0.21, -0.37], [0., -0.45, 0.4], [0., 0.13, 0.29]])
    return np.concatenate([q] + [q + o for o in off])


def quad_closed_form(queries, T=4):
    """Analytic pinhole tracks [Q,T,2] (u, v) of points that ride the plane z = QUAD_Z0 of frame 0."""
    fx, fy, px, py = QUAD_K
    X = np.stack([(queries[:, 2] - px) / fx * QUAD_Z0, (queries[:, 1] - py) / fy * QUAD_Z0, np.full(len(queries), QUAD_Z0)], 1)
    P = X[:, None, :] + np.arange(T)[None, :, None] * QUAD_STEP[None, None, :]
    return np.stack([fx * P[..., 0] / P[..., 2] + px, fy * P[..., 1] / P[..., 2] + py], -1)


# ---- 3: a small near rectangle slides across a far quad ---------------------------------------------------------------------------------
OCC_K = np.array([60., 58., 31.7, 23.3])
OCC_FAR_Z, OCC_NEAR_Z = 4., 2.
OCC_NEAR_HALF = (0.2, 0.15)
OCC_NEAR_X = (-0.62, -0.31, 0.0, 0.31, 0.62)            # centre of the near rectangle per frame


def occluder_case():
    """Far quad (faces 0, 1) filling columns 7.7 .. 55.7, rows 5.9 .. 40.7; near rectangle (faces 2, 3; no vertex shared with the far
    quad) of 12 x 8.7 pixels whose centre moves 9.3 pixels a frame.  T = 5."""
    T = len(OCC_NEAR_X)
    far = np.array([[-1.6, -1.2, OCC_FAR_Z], [1.6, -1.2, OCC_FAR_Z], [1.6, 1.2, OCC_FAR_Z], [-1.6, 1.2, OCC_FAR_Z]])
    hx, hy = OCC_NEAR_HALF
    verts = []
    for x in OCC_NEAR_X:
        near = np.array([[x - hx, -hy, OCC_NEAR_Z], [x + hx, -hy, OCC_NEAR_Z], [x + hx, hy, OCC_NEAR_Z], [x - hx, hy, OCC_NEAR_Z]])
        verts.append(np.concatenate([far, near]))
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    return np.stack(verts).astype(np.float32), faces, np.tile(OCC_K.astype(np.float32), (T, 1))


def occluder_rect(t):
    """Projection of the near rectangle in frame t: (u_left, u_right, v_top, v_bottom)."""
    fx, fy, px, py = OCC_K
    hx, hy = OCC_NEAR_HALF
    x = OCC_NEAR_X[t]
    return (fx * (x - hx) / OCC_NEAR_Z + px, fx * (x + hx) / OCC_NEAR_Z + px, -fy * hy / OCC_NEAR_Z + py, fy * hy / OCC_NEAR_Z + py)


def occluder_queries():
    """Pixel centres of the far quad on a 2-pixel grid along the rows the near rectangle crosses, right of where it starts."""
    r, c = np.mgrid[14:33:2, 22:54:2]
    return np.stack([np.zeros(r.size), r.ravel() + 0.5, c.ravel() + 0.5], 1)


def inside_by(u, v, rect):
    """How far (u, v) lies inside the axis-parallel rectangle: the distance to the nearest side when inside (> 0), minus the largest
    per-axis excess when outside (< 0)."""
    ul, ur, vt, vb = rect
    return np.minimum(np.minimum(u - ul, ur - u), np.minimum(v - vt, vb - v))


# ---- 4: an octahedron yawed through 180 degrees -------------------------------------------------------------------------------------------
OCTA_K = np.array([150., 145., 31.7, 23.3])
OCTA_C = np.array([0.02, -0.03, 4.])
OCTA_R = 0.55
OCTA_ANGLES = np.deg2rad(10. + 45. * np.arange(5))
OCTA_BASE = OCTA_R * np.array([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
OCTA_FACES = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def yaw(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def octahedron_case():
    verts = np.stack([OCTA_BASE @ yaw(a).T + OCTA_C for a in OCTA_ANGLES]).astype(np.float32)
    return verts, OCTA_FACES, np.tile(OCTA_K.astype(np.float32), (len(OCTA_ANGLES), 1))


def octahedron_n_dot_p(face, bary):
    """Closed form of n . P per frame for the point bary (c0, c1, c2) of `face`: with p0 the point and n0 the normal in the body
    frame, n_t . P_t = n0 . p0 + (R_t n0) . C  (R_t n0 . R_t p0 = n0 . p0).  -> [T]."""
    tri = OCTA_BASE[OCTA_FACES[face]]
    n0 = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    p0 = bary @ tri
    return np.array([n0 @ p0 + (yaw(a) @ n0) @ OCTA_C for a in OCTA_ANGLES])


# ---- 5 / 6: a wobbling geodesic sphere ----------------------------------------------------------------------------------------------------
SPHERE_K = np.array([75., 73., 32.3, 24.2])


def sphere_case(T=5):
    """Geodesic sphere of 320 faces that turns 35 degrees a frame about a tilted axis, breathes and bends differently in every
    frame (non-rigid), and drifts to the left (the way its front turns) until a part of it leaves the frame.  -> verts float32 [T,162,3], faces, K."""
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(4)
    assert v.shape == (162, 3) and f.shape == (320, 3)
    v = v.astype(np.float64)
    tilt = np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    verts = []
    for t in range(T):
        w = v * (1. + 0.10 * np.sin(3. * v[:, 1:2] + 0.9 * t) + 0.06 * np.cos(4. * v[:, 0:1] - 0.7 * t))
        w = w @ (tilt @ yaw(0.2 + np.deg2rad(35.) * t)).T
        verts.append(w + np.array([0.3 - 0.4 * t, 0.03 - 0.02 * t, 4. + 0.1 * t]))
    return np.stack(verts).astype(np.float32), f, np.tile(SPHERE_K.astype(np.float32), (T, 1))


def sphere_queries(planes, per_frame=60, seed=SEED):
    """Every covered pixel centre of frame 0, then per_frame seeded queries in each later frame: a covered pixel's corner plus an
    offset in [0.15, 0.85]^2, so that floor() of the query is not a matter of rounding."""
    rng = np.random.default_rng(seed)
    h, w = planes.shape[1:]
    qs = [centres(planes[0, :H, :W] >= 0, 0)]
    for t in range(1, planes.shape[0]):
        r, c = np.nonzero(planes[t, :H, :W] >= 0)
        pick = rng.choice(len(r), per_frame, replace=False)
        off = rng.uniform(0.15, 0.85, (per_frame, 2))
        qs.append(np.stack([np.full(per_frame, float(t)), r[pick] + off[:, 0], c[pick] + off[:, 1]], 1))
    return np.concatenate(qs)


# ---- 8: the preview ---------------------------------------------------------------------------------------------------------------------------
def splat_case(seed=5, Q=40, T=3):
    """Random tracks over T noise frames: some outside the frame, some hidden, the last two queries at one pixel in frame 0."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    tracks = np.stack([rng.uniform(-3, W + 3, (Q, T)), rng.uniform(-3, H + 3, (Q, T))], -1).astype(np.float32)
    tracks[Q - 2, 0] = tracks[Q - 1, 0] = (20.25, 30.75)
    tracks[0, 1] = (0.5, 0.5)                                         # a disc clipped by the corner
    tracks[1, 2] = (W - 0.25, H - 0.25)
    inside = (tracks[..., 0] >= 0) & (tracks[..., 0] < W) & (tracks[..., 1] >= 0) & (tracks[..., 1] < H)
    state = np.where(inside, np.where(rng.uniform(size=(Q, T)) < 0.7, 1, 2), 3).astype(np.uint8)
    state[Q - 2:, 0] = 1
    state[0, 1] = state[1, 2] = 1
    colors = rng.integers(0, 256, (Q, 3), dtype=np.uint8)
    return frames, tracks, state, colors
