"""Restatement of the shape scores (include/lasr_ops.h) in plain numpy, and the seeded fixtures
tests/test_meshcheck_cpu.py and tests/test_meshcheck_gpu.py share.  Nothing here imports the package or torch: the kernels of
lasr_amd/csrc/meshcheck.hip and the passes of lasr_amd/nnutils/meshcheck.py are compared against this file, not the other way round.

This file is the definition.  Every function takes the working precision `dt` (float64 by default) and computes in it alone: run
in float32 it follows the kernel's operation order (no contraction), and its distance from the float64 run is what the condition
of the GPU equalities is derived from.  verts is float32 [T,V,3] (or [V,3]: one frame), faces int32 [F,3], one topology for all
frames.  Touching and coplanar overlap do not count (every sign test is strict), and faces that share a vertex are never tested:
a fold between two neighbours goes unseen.
"""
import functools

import numpy as np

EDGES = ((0, 1), (1, 2), (2, 0))


def orient(a, b, c, d, dt=np.float64):
    """((b - a) x (c - a)) . (d - a) over the leading axes of [..., 3] arrays, in dt, in the operation order of the kernel."""
    a, b, c, d = (np.asarray(x).astype(dt) for x in (a, b, c, d))
    ux, uy, uz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    wx, wy, wz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
    cx, cy, cz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
    ex, ey, ez = d[..., 0] - a[..., 0], d[..., 1] - a[..., 1], d[..., 2] - a[..., 2]
    return ((cx * ex + cy * ey) + cz * ez).astype(dt)


def pierces(p, q, a, b, c, dt=np.float64):
    """Edge (p, q) against triangle (a, b, c) -> (bool [...], the five determinants [..., 5])."""
    dp, dq = orient(a, b, c, p, dt), orient(a, b, c, q, dt)
    s0, s1, s2 = orient(p, q, a, b, dt), orient(p, q, b, c, dt), orient(p, q, c, a, dt)
    crosses = ((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))
    inside = ((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0))
    return crosses & inside, np.stack([dp, dq, s0, s1, s2], -1)


def candidates(verts, faces):
    """One frame [V,3] -> the candidate pairs (i [n], j [n]), i < j, in lexicographic order: no shared vertex index, boxes overlap
    (closed comparisons on the float32 inputs)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces)
    tri = verts[faces]                                                            # [F,3,3]
    lo, hi = tri.min(1), tri.max(1)
    over = ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all(-1)
    share = (faces[:, None, :, None] == faces[None, :, None, :]).any((-1, -2))
    i, j = np.nonzero(np.triu(over & ~share, 1))
    return i, j


def pair_determinants(verts, faces, i, j, dt=np.float64):
    """-> (hit bool [n], dets [n,30]): per pair the three edges of i against j, then the three edges of j against i, five
    determinants each."""
    tri = np.asarray(verts, np.float32)[np.asarray(faces)].astype(dt)
    A, B = tri[i], tri[j]
    hit, dets = np.zeros(len(i), bool), []
    for X, Y in ((A, B), (B, A)):
        for e0, e1 in EDGES:
            h, d = pierces(X[:, e0], X[:, e1], Y[:, 0], Y[:, 1], Y[:, 2], dt)
            hit |= h
            dets.append(d)
    return hit, (np.concatenate(dets, -1) if len(i) else np.zeros((0, 30), dt))


def _frames(verts):
    verts = np.asarray(verts, np.float32)
    return verts[None] if verts.ndim == 2 else verts


def self_intersections(verts, faces, dt=np.float64):
    """-> per frame a dict: n_candidates, n_pairs, face_count [F], n_faces, ratio, pairs [n,2] sorted."""
    faces = np.asarray(faces)
    F, out = faces.shape[0], []
    for v in _frames(verts):
        i, j = candidates(v, faces)
        hit, _ = pair_determinants(v, faces, i, j, dt)
        pairs = np.stack([i[hit], j[hit]], -1).astype(np.int64).reshape(-1, 2)
        count = np.bincount(pairs.reshape(-1), minlength=F).astype(np.int32)
        n_faces = int((count > 0).sum())
        out.append(dict(n_candidates=len(i), n_pairs=len(pairs), face_count=count, n_faces=n_faces, ratio=n_faces / F if F else 0.,
                        pairs=pairs))
    return out


def det_spread(verts, faces):
    """max |det32 - det64| and min |det64| over the 30 determinants of every candidate pair of every frame (0, inf without one)."""
    spread, least = 0., np.inf
    for v in _frames(verts):
        i, j = candidates(v, faces)
        if len(i):
            d64 = pair_determinants(v, faces, i, j, np.float64)[1]
            d32 = pair_determinants(v, faces, i, j, np.float32)[1]
            spread, least = max(spread, float(np.abs(d32.astype(np.float64) - d64).max())), min(least, float(np.abs(d64).min()))
    return spread, least


def uncertain(verts, faces, bound):
    """The candidate pairs (frame, i, j) with any of their 30 determinants within `bound` of zero in float64."""
    out = []
    for t, v in enumerate(_frames(verts)):
        i, j = candidates(v, faces)
        if len(i):
            near = (np.abs(pair_determinants(v, faces, i, j, np.float64)[1]) <= bound).any(-1)
            out += [(t, int(a), int(b)) for a, b in zip(i[near], j[near])]
    return out


def volume_area_terms(verts, faces):
    """float64 from the float32 inputs: (volume terms [T,F] before the division by 6, area terms [T,F])."""
    tri = _frames(verts)[:, np.asarray(faces)].astype(np.float64)                 # [T,F,3,3]
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    vol = ((a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]))
           + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))
    u, w = b - a, c - a
    nx, ny, nz = (u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                  u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0])
    return vol, 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def volume_area(verts, faces):
    """-> (volume [T], area [T]) float64: sum_f a . (b x c) / 6, positive for outward-facing faces, and sum_f 0.5 |(b-a) x (c-a)|."""
    vol, area = volume_area_terms(verts, faces)
    return vol.sum(1) / 6., area.sum(1)


def jitter(verts, dt=np.float64):
    """[T]: the mean over the vertices of |v_{t+1} - 2 v_t + v_{t-1}| over the diagonal of frame t's bounding box; NaN for the
    first and the last frame."""
    v = _frames(verts).astype(dt)
    T = v.shape[0]
    out = np.full(T, np.nan, dt)
    for t in range(1, T - 1):
        d = (v[t + 1] - dt(2) * v[t]) + v[t - 1]
        acc = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(dt).mean(dtype=dt)
        e = v[t].max(0) - v[t].min(0)
        out[t] = acc / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return out


def evaluate(verts, faces):
    """Everything scripts/eval_shape.py reports, per frame, in float64."""
    res = self_intersections(verts, faces)
    vol, area = volume_area(verts, faces)
    return dict(n_pairs=np.array([r['n_pairs'] for r in res], np.int64), n_faces=np.array([r['n_faces'] for r in res], np.int64),
                face_count=np.stack([r['face_count'] for r in res]), volume=vol, area=area, jitter=jitter(verts),
                truncated=np.zeros(len(res), bool))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def icosphere(level, seed, radial=0.03, positional=0.02):
    """A unit icosphere of 20 * 4^level outward-facing faces whose vertices are moved, seeded, by `radial` of their radius and by
    `positional` per coordinate: the plain icosphere is full of exactly coplanar quadruples.  -> verts float32 [V,3], faces int32."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    rng = np.random.default_rng(seed)
    v = v * (1 + radial * rng.uniform(-1, 1, (len(v), 1))) + positional * rng.uniform(-1, 1, v.shape)
    return v.astype(np.float32), np.array(f, np.int32)


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


TWO2_OFFSETS = ((3.0, 0.2, 0.1), (0.8, 0.1, 0.05), (0.45, 0.1, 0.05))             # far apart, overlapping, overlapping more


@functools.lru_cache(None)
def two2():
    """Two jittered level-2 spheres in one face list of 640 faces, three frames: the second sphere is rotated, scaled by 0.9 and
    offset per frame.  -> verts [3,324,3], faces [640,3]."""
    va, fa = icosphere(2, 11)
    vb, fb = icosphere(2, 12)
    vb = 0.9 * vb.astype(np.float64) @ _rotation(13).T
    verts = np.stack([np.concatenate([va, (vb + np.array(o)).astype(np.float32)]) for o in TWO2_OFFSETS]).astype(np.float32)
    return verts, np.concatenate([fa, fb + len(va)]).astype(np.int32)


@functools.lru_cache(None)
def pinch2():
    """A jittered level-2 sphere with its topmost vertex pushed through the opposite side."""
    v, f = icosphere(2, 21)
    v = v.copy()
    k = int(np.argmax(v[:, 2]))
    v[k] = (-1.3 * v[k].astype(np.float64) + np.array([0.013, -0.021, 0.])).astype(np.float32)
    return v[None], f


@functools.lru_cache(None)
def tile_case(n):
    """n faces (one tile of 256, or one face more) of the overlapping frame of two2, half from each sphere, nearest the other
    sphere first; the last face is one that intersects another, so that with 257 faces the one-face tile takes part."""
    verts, faces = two2()
    v = verts[1]
    cen = v[faces].astype(np.float64).mean(1)
    d = np.array(TWO2_OFFSETS[1])
    a = np.argsort(-(cen[:320] @ d), kind='stable')[:128]
    b = 320 + np.argsort(cen[320:] @ d, kind='stable')[:n - 128]
    sub = faces[np.concatenate([a, b])]
    count = self_intersections(v, sub)[0]['face_count']
    k = int(np.nonzero(count[128:] > 0)[0][-1]) + 128
    order = np.concatenate([np.delete(np.arange(n), k), [k]])
    return v[None], np.ascontiguousarray(sub[order])


@functools.lru_cache(None)
def wobble():
    """Five frames of a jittered level-2 sphere that drifts, breathes and shakes: the jitter fixture."""
    v, f = icosphere(2, 31)
    rng = np.random.default_rng(32)
    frames = [(v.astype(np.float64) * (1 + 0.05 * np.sin(t)) + np.array([0.1 * t, 0.02 * t * t, 0.]) + 0.01 * rng.normal(size=v.shape))
              for t in range(5)]
    return np.stack(frames).astype(np.float32), f


def _single(level, seed):
    v, f = icosphere(level, seed)
    return v[None], f


def _inverted():
    v, f = _single(2, 2)
    return v, np.ascontiguousarray(f[:, ::-1])


FIXTURES = {
    'ico1': lambda: _single(1, 1),
    'ico2': lambda: _single(2, 2),
    'two2': two2,
    'pinch2': pinch2,
    'tile256': lambda: tile_case(256),
    'tile257': lambda: tile_case(257),
    'inverted': _inverted,
    'wobble': wobble,
}


@functools.lru_cache(None)
def fixture(name):
    """-> (verts float32 [T,V,3], faces int32 [F,3])."""
    verts, faces = FIXTURES[name]()
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)


@functools.lru_cache(None)
def expected(name):
    """The float64 restatement of a fixture, computed once and shared: evaluate() plus the per-frame results."""
    verts, faces = fixture(name)
    return dict(evaluate(verts, faces), frames=self_intersections(verts, faces))


COPY_GRID, COPY_STEP = 2. ** -16, 8.


@functools.lru_cache(None)
def copies_base():
    """The overlapping frame of two2 with every coordinate rounded to a multiple of 2^-16."""
    verts, faces = two2()
    return (np.round(verts[1].astype(np.float64) / COPY_GRID) * COPY_GRID).astype(np.float32)[None], faces


@functools.lru_cache(None)
def copies_case(n):
    """n copies of copies_base() in one face list, copy k moved by 8 (k % 8, k / 8 % 8, k / 64): a mesh of 640 n faces whose answer
    costs one restatement of 640.  Every coordinate stays a multiple of 2^-16 below 64, so each copy is an exact translate, every
    difference of two of its vertices is the base's, exactly, in float32 as in float64, and so is every determinant; the boxes of two
    copies are 5 apart, so no pair joins two copies.  -> (verts [1,324 n,3], faces [640 n,3], expected: n_pairs, face_count, pairs)."""
    v0, f0 = copies_base()
    V0, F0 = v0.shape[1], f0.shape[0]
    shift = np.array([[k % 8, k // 8 % 8, k // 64] for k in range(n)], np.float64) * COPY_STEP
    verts = (v0[0].astype(np.float64)[None] + shift[:, None]).reshape(1, n * V0, 3)
    assert (verts == verts.astype(np.float32)).all() and np.abs(verts).max() < 64
    faces = (f0[None].astype(np.int64) + V0 * np.arange(n)[:, None, None]).reshape(n * F0, 3).astype(np.int32)
    base = self_intersections(v0, f0)[0]
    pairs = (base['pairs'][None] + F0 * np.arange(n)[:, None, None]).reshape(-1, 2)
    return verts.astype(np.float32), faces, dict(n_pairs=n * base['n_pairs'], face_count=np.tile(base['face_count'], n), pairs=pairs)


def write_sequence(root, name, verts, faces):
    """What scripts/eval_shape.py reads under `root`: configs/<name>.config, one (blank) frame image per mesh and
    <root>/out-<name>/pred<i>.ply.  -> the test directory."""
    import os
    from PIL import Image
    from lasr_amd.ext_utils.ply import write_ply
    img_dir = os.path.join(root, 'database', 'DAVIS', 'JPEGImages', 'Full-Resolution', name)
    test = os.path.join(root, 'out-' + name)
    for d in (img_dir, test, os.path.join(root, 'configs')):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(root, 'configs', '%s.config' % name), 'w') as f:
        f.write('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/%s/\ndframe = 1\ncan_frame = 0\ninit_frame = 0\n'
                'end_frame = -1\n' % name)
    for i in range(len(verts)):
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(os.path.join(img_dir, '%05d.png' % i))
        write_ply(os.path.join(test, 'pred%d.ply' % i), verts[i], faces, colors=np.full((verts.shape[1], 3), 102))
    return test
